"""The `direct` integrator (include/msk_gpu.h at msk_direct_params; csrc/msk_direct.h): per camera sample one
primary ray, N light samples and M BSDF samples at its hit, combined by the power heuristic over the sample counts.

CPU: the plugin and the mirror load <integrator type="direct"> and refuse the same things in the same words; exports and struct
layout; the pair layout; the launch geometry as a stand-alone native program; the float64 estimator's variance on the pixels test 4
probes.  GPU: (1, 1) is `path` at max_depth = 2, bit for bit, on every scene feature; the two pure strategies and mixtures meet
float64 closed forms; a point light's N terms over N; more samples cut the variance; the tree in HBM, shards and a crop window give
the same bits; statistics; refusals.

The closed-form rule is test_delta_light_mirror.py's (and test_envmap.py's): spp doubles from 4096 until the standard error of the
mean, from the per-sample values, is at most 0.5 % of the expectation (four doublings at the most); then
|mean - E| <= 6 standard errors + 1e-3 E per channel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import delta_ref as D
import direct_ref as DR
import radiometry_ref as R
import test_delta_light_mirror as DM
import test_envmap as EV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FW, FH, BS = 24, 20, 16                  # films of 24 x 20 with blocks of 16: partial blocks in both directions
CAM = EV.PLANE_CAMERA
# a 4 x 4 lamp four units above the plane, wound to face down (test_envmap's LAMP is 1 x 1 at height 10: a BSDF sample finds
# that one three times in a thousand)
LAMP4 = [(2.0, 4.0, -2.0), (2.0, 4.0, 2.0), (-2.0, 4.0, 2.0), (-2.0, 4.0, -2.0)]
PROBE = np.array([(x, y) for y in range(EV.CROP[1], EV.CROP[1] + 4) for x in range(EV.CROP[0], EV.CROP[0] + 4)], np.int32)     # 16 pixels
# test 4's pixels (film 24 x 20 of the Cornell box): the floor and the short box's top where the boxes shadow part of the lamp —
# test_more_samples_help_in_float64 checks the condition on them for the float64 estimator
VAR_PIXELS = [(9, 9), (10, 9), (11, 9), (9, 10), (10, 10), (11, 10), (9, 11), (10, 11), (11, 11), (9, 12), (10, 12), (9, 13), (10, 13),
              (9, 14), (10, 14), (9, 15)]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def all_pixels(w=FW, h=FH):
    return np.array([(x, y) for y in range(h) for x in range(w)], np.int32)


# ===================================================================================================== CPU
def direct_xml(hm, directory, props=None, **kw):
    return hm.write_scene_xml(hm.cbox_meshes(), str(directory), FW, FH, 4, integrator_props=props, integrator_type="direct", **kw)


REFUSALS = [({"light_samples": -1}, '"light_samples" must be >= 0'), ({"bsdf_samples": -3}, '"bsdf_samples" must be >= 0'),
            ({"light_samples": 0, "bsdf_samples": 0}, '"light_samples" and "bsdf_samples" must not both be 0'),
            ({"light_samples": 4097}, '"light_samples" must be at most 4096'), ({"bsdf_samples": 5000}, '"bsdf_samples" must be at most 4096'),
            ({"gpu_devices": "0,1"}, '"gpu_devices": the "direct" integrator renders on one device')]


def test_host_plugin_and_mirror(hostmirror, abi, tmp_path):
    """<integrator type="direct"> loads through the host library and through the mirror; defaults (1, 1); every refusal names its
    property, in the same words on both sides"""
    hostlib = EV.host_library()
    xml = direct_xml(hostmirror, tmp_path / "defaults")
    assert '<integrator type="direct">' in open(xml).read()
    sc = hostlib.HostScene(xml)
    assert sc.direct_params() == (1, 1)
    flat = sc.flatten()
    assert (flat.params.spp, flat.params.rng_mode, flat.params.hide_emitters, flat.params.block_size) == (4, abi.MSK_RNG_COUNTER, 0, 32)
    assert (flat.params.sample_first, flat.params.sample_stride, flat.params.block_first, flat.params.block_stride) == (0, 1, 0, 1)
    sc.close()
    kind, props = hostmirror.read_integrator(xml)
    assert kind == "direct" and (props["light_samples"], props["bsdf_samples"]) == (1, 1)
    assert props == hostmirror.direct_integrator() and props["block_size"] == 32 and props["hide_emitters"] is False
    # properties: the counts, and hide_emitters under the plugin convention of "path" (honor_properties)
    for given, hide in (({"light_samples": 4, "bsdf_samples": 2, "block_size": 16, "hide_emitters": True}, 0),
                        ({"light_samples": 0, "bsdf_samples": 4096, "hide_emitters": True, "honor_properties": True, "gpu_device": 0}, 1)):
        xml = direct_xml(hostmirror, tmp_path / ("p%d" % hide), given)
        sc = hostlib.HostScene(xml)
        assert sc.direct_params() == (given["light_samples"], given["bsdf_samples"])
        p = sc.flatten().params
        assert p.hide_emitters == hide and p.block_size == given.get("block_size", 32)
        sc.close()
        kind, props = hostmirror.read_integrator(xml)
        assert kind == "direct" and all(props[k] == v for k, v in given.items())
    # a "path" scene has no direct parameters
    sc = hostlib.HostScene(hostmirror.write_scene_xml(hostmirror.cbox_meshes(), str(tmp_path / "path"), FW, FH, 4))
    assert sc.direct_params() is None
    sc.close()
    assert hostmirror.read_integrator(str(tmp_path / "path" / "scene.xml"))[0] == "path"
    for i, (given, text) in enumerate(REFUSALS):
        xml = direct_xml(hostmirror, tmp_path / ("r%d" % i), given)
        with pytest.raises(hostlib.HostError) as he:
            hostlib.HostScene(xml)
        with pytest.raises(ValueError) as me:
            hostmirror.read_integrator(xml)
        assert text in str(he.value) and text in str(me.value), (given, str(he.value), str(me.value))
        assert str(me.value) in str(he.value)                      # the same words


def test_exports_and_struct(abi, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msk_gpu.h"\nint main(){printf("%zu %zu %zu %zu %d\\n",sizeof(msk_direct_params),'
                   'offsetof(msk_direct_params,light_samples),offsetof(msk_direct_params,bsdf_samples),sizeof(msk_render_params),MSK_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    d = abi.DirectParams
    assert got == [C.sizeof(d), d.light_samples.offset, d.bsdf_samples.offset, C.sizeof(abi.RenderParams), abi.MSK_ABI_VERSION]
    assert got[:3] == [8, 0, 4] and got[4] == 8                   # the ABI stays version 8 and only grows
    import __graft_entry__ as ge
    ge.build_gpu_library()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("msk_gpu_render_direct", "msk_gpu_render_direct_device", "msk_gpu_sample_pixels_direct"):
        assert name in abi.EXPORTS and getattr(lib, name) is not None
    assert b"k_direct" in open(abi.LIB_PATH, "rb").read()


def test_pair_layout():
    lay = DR.pair_layout(1, 1)
    assert (lay["light"], lay["bsdf_lobe"], lay["bsdf_direction"]) == ([3], [4], [5])      # `path`'s first bounce
    assert (lay["film"], lay["wavelengths"], lay["aperture"]) == (0, 1, 2)
    for n in range(9):
        for m in range(9):
            d = DR.draws(n, m)
            assert len(d) == 3 + n + 2 * m and len(set(d)) == len(d) and sorted(d) == list(range(3 + n + 2 * m)), (n, m)
            lay = DR.pair_layout(n, m)
            assert lay["light"] == [3 + i for i in range(n)]
            assert all(lay["bsdf_direction"][j] == lay["bsdf_lobe"][j] + 1 == 3 + n + 2 * j + 1 for j in range(m))


def test_weight_restatement():
    """the weights are a partition of unity where both strategies can make the direction, and the pure strategies weigh 1"""
    rng = np.random.RandomState(3)
    pl, pb = rng.uniform(0.01, 5, 256), rng.uniform(0.01, 5, 256)
    for n, m in ((1, 1), (3, 2), (8, 8), (16, 1)):
        # sum over the two strategies of (count x density x weight / count) / (mixture numerator) = 1: n pl wl / n + m pb wb / m over ... the balance identity of the power heuristic
        wl, wb = DR.weight(n, pl, m, pb), DR.weight(m, pb, n, pl)
        assert np.allclose(wl + wb, 1.0, rtol=0, atol=1e-15)
    assert np.all(DR.weight(4, pl, 0, pb) == 1.0) and np.all(DR.weight(4, pb, 0, pl) == 1.0)
    assert np.all(DR.weight(4, np.zeros(4), 2, np.ones(4)) == 0.0)
    assert np.all(DR.weight(1, pl, 1, pb) == pl ** 2 / (pl ** 2 + pb ** 2))


def test_native_plan_check(tmp_path):
    exe = str(tmp_path / "direct_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "direct_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.split()[0] == "cases" and int(r.stdout.split()[1]) > 10000


def test_more_samples_help_in_float64(hostmirror):
    """Test 4's condition, checked where it can be reasoned about: on every pixel of VAR_PIXELS the float64 estimator's variance at
    (8, 8) is below 0.4 of its variance at (1, 1), and the latter is at least half the squared mean — so the geometric part carries
    the renderer's per-sample variance there, not the wavelength draw both runs share (direct_ref's docstring)."""
    flat = hostmirror.cbox_scene(FW, FH)
    tris = DR.Triangles(flat)
    assert len(tris.lamp) == 2 and abs(tris.lamp_area - 130.0 * 105.0) < 1e-6
    for (x, y) in VAR_PIXELS:
        rng = np.random.RandomState(1000 * y + x)
        g1 = DR.estimate(flat, tris, (x, y), 1, 1, 1024, rng, R.camera_ray)
        g8 = DR.estimate(flat, tris, (x, y), 8, 8, 1024, rng, R.camera_ray)
        assert g1.mean() > 0 and abs(g8.mean() - g1.mean()) < 0.25 * g1.mean(), (x, y, g1.mean(), g8.mean())
        assert g1.var() >= 0.5 * g1.mean() ** 2 and g8.var() <= 0.4 * g1.var(), (x, y, g1.var() / g1.mean() ** 2, g8.var() / g1.var())


# ===================================================================================================== GPU: scenes
def mixed_meshes(hm):
    """(b) the Cornell box with a `bitmap` floor, a `twosided` `roughconductor` short box, a `roughdielectric` tall box and a
    `dielectric` blob"""
    meshes = hm.cbox_meshes()
    by = {m.name: m for m in meshes}
    floor = by["cbox_floor"]
    floor.bsdf = {"type": "diffuse", "texture": {"type": "bitmap", "pixels": np.random.RandomState(2).uniform(0.1, 0.9, (4, 4, 3)).astype(F), "scale": (3, 3)}}
    floor.texcoords = [((0, 0), (1, 0), (1, 1), (0, 1)) for _ in floor.faces]
    by["cbox_smallbox"].bsdf = {"type": "roughconductor", "alpha": 0.2, "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14), "twosided": True}
    by["cbox_largebox"].bsdf = {"type": "roughdielectric", "alpha": 0.1, "int_ior": 1.5, "ext_ior": 1.0}
    glass = hm.blob_mesh("glass", (400, 80, 120), 70, 5, 5, hm.WHITE, seed=2)
    glass.bsdf = {"type": "dielectric"}
    return meshes + [glass]


def open_box(hm):
    return [m for m in hm.cbox_meshes() if m.name not in ("cbox_ceiling", "cbox_back")]


def anchor_flat(hm, name):
    if name == "a_cbox":
        return hm.cbox_scene(FW, FH)
    if name == "b_mixed":
        return hm.flatten(mixed_meshes(hm), FW, FH)
    if name == "c_envmap":
        return hm.flatten(EV.variant_meshes(hm), FW, FH, env=EV.env_spec(EV.lit_image(), EV.skew_rotation(), scale=40.0))
    if name == "d_point_mirror_sky":
        ball = hm.blob_mesh("mirror", (170, 100, 330), 90, 6, 6, hm.WHITE, seed=4)
        ball.bsdf = dict(DM.GOLD_RGB)
        return hm.flatten(open_box(hm) + [ball], FW, FH, env=DM.SKY, points=[DM.point_spec((120.0, 420.0, 200.0), (4e5, 3e5, 2e5))])
    raise KeyError(name)


def test_anchor_scenes_hold_what_they_say(hostmirror, abi):
    fb, fc, fd = (anchor_flat(hostmirror, k) for k in ("b_mixed", "c_envmap", "d_point_mirror_sky"))      # (they own what the descriptors point into)
    b = fb.desc
    types = {b.bsdfs[i].type for i in range(b.n_bsdfs)}
    assert {abi.MSK_BSDF_DIFFUSE, abi.MSK_BSDF_ROUGHCONDUCTOR, abi.MSK_BSDF_ROUGHDIELECTRIC, abi.MSK_BSDF_DIELECTRIC} <= types
    assert any(b.bsdfs[i].back_bsdf >= 0 for i in range(b.n_bsdfs)) and b.n_texels > 0
    c = fc.desc
    assert any(c.emitters[i].type == abi.MSK_EMITTER_ENVMAP for i in range(c.n_emitters))
    d = fd.desc
    assert {d.emitters[i].type for i in range(d.n_emitters)} == {abi.MSK_EMITTER_AREA, abi.MSK_EMITTER_CONSTANT, abi.MSK_EMITTER_POINT}
    assert any(d.bsdfs[i].type == abi.MSK_BSDF_CONDUCTOR for i in range(d.n_bsdfs))


# ===================================================================================================== GPU 1: the anchor
ANCHORS = [("a_cbox", 0), ("a_cbox", 1), ("b_mixed", 0), ("c_envmap", 0), ("d_point_mirror_sky", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,hide", ANCHORS, ids=lambda v: str(v))
def test_one_one_is_path_at_depth_two_bit_for_bit(gpu_ctx, hostmirror, abi, name, hide):
    """(1) msk_gpu_sample_pixels_direct at (1, 1) against msk_gpu_sample_pixels at max_depth = 2, rr_depth = 5: every X, Y, Z of
    every sample, the film positions, and the two films, as bits"""
    g = abi.Scene(gpu_ctx, anchor_flat(hostmirror, name))
    try:
        prm = abi.render_params(spp=6, seed=11, max_depth=2, rr_depth=5, hide_emitters=hide, block_size=BS)
        want, wpos = g.sample_pixels(prm, all_pixels())
        got, gpos = g.sample_pixels_direct(prm, all_pixels(), 1, 1)
        assert np.array_equal(bits(gpos), bits(wpos))
        bad = (bits(got) != bits(want)).any(-1)
        assert not bad.any(), (name, hide, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:3], want[bad][:3])
        assert np.isfinite(want).all() and want.max() > 0
        film_p, st_p = g.render(prm)
        film_d, st_d = g.render_direct(prm, 1, 1)
        assert np.array_equal(bits(film_d), bits(film_p)), (name, hide, float(np.abs(film_d - film_p).max()))
        assert st_d.samples == st_p.samples == FW * FH * 6 and st_d.invalid_samples == st_p.invalid_samples
    finally:
        g.close()


# ===================================================================================================== GPU 2: closed forms
def probe_rays(desc, m=4):
    t, w = R.gauss_legendre(m)
    yy, xx = np.meshgrid(EV.CROP[1] + 4 * t, EV.CROP[0] + 4 * t, indexing="ij")
    o, d = R.camera_ray(desc, xx, yy)
    return o, d, w[:, None] * w[None, :]


def lamp_scene(hm):
    lamp = hm.MeshSpec("lamp", [tuple(LAMP4)], hm.LUMINAIRE, radiance=(40, 30, 20))
    return hm.flatten([DM.plane(hm), lamp], EV.W48, EV.W48, camera=CAM)


def lamp_expected(desc, m):
    """rho / pi * Le * polygon_irradiance, the mean over the 16 probed pixels"""
    o, d, w = probe_rays(desc, m)
    geom = float((w * R.polygon_irradiance(R.hit_plane(o, d, (0, 0, 0), (0, 1, 0)), (0, 1, 0), np.array(LAMP4, np.float64))).sum())
    return R.expected_xyz(D.emitter_spectrum(desc, 0) * DM.rho_over_pi(desc), DM.cie_of(desc)) * geom


def sky_scene(hm):
    return hm.flatten([DM.plane(hm)], EV.W48, EV.W48, camera=CAM, env=DM.SKY)


def test_closed_form_expectations_have_converged(hostmirror):
    flat = lamp_scene(hostmirror)         # (owns the arrays the descriptor points into)
    d = flat.desc
    e4, e8 = lamp_expected(d, 4), lamp_expected(d, 8)
    assert np.all(e4 > 0) and np.all(np.abs(e4 - e8) <= 1e-5 * e8)
    o, dd, _ = probe_rays(d)
    x = R.hit_plane(o, dd, (0, 0, 0), (0, 1, 0))
    assert np.all(np.abs(x[..., [0, 2]]) < 25)                      # the probed pixels see the plane


def direct_mean(g, abi, what, expected, n, m, pixels=PROBE, **kw):
    """the rule's procedure (module docstring) through msk_gpu_sample_pixels_direct -> (mean, standard error)"""
    spp = 4096
    for _ in range(5):
        xyz, _ = g.sample_pixels_direct(abi.render_params(spp=spp, seed=7, **kw), pixels, n, m)
        v = xyz.reshape(-1, 3).astype(np.float64)
        mean, se = v.mean(0), v.std(0, ddof=1) / np.sqrt(len(v))
        print("DIRECT %s (%d, %d) spp %d: expected %s mean %s se/|E| %s dev/|E| %s" % (what, n, m, spp, expected, mean, se / expected, (mean - expected) / expected))
        if np.all(se <= 5e-3 * expected):
            return mean, se
        spp *= 2
    raise AssertionError("the standard error stays above 0.5 %% of the expectation: %s" % (se / expected,))


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(4, 0), (0, 4), (3, 2)])
def test_area_light_meets_the_closed_form(gpu_ctx, hostmirror, abi, n, m):
    """(2) a diffuse floor under a polygonal area light: the two pure strategies and a mixture"""
    flat = lamp_scene(hostmirror)
    expected = lamp_expected(flat.desc, 4)
    g = abi.Scene(gpu_ctx, flat)
    try:
        mean, se = direct_mean(g, abi, "lamp", expected, n, m)
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


@pytest.mark.gpu
def test_constant_sky_meets_rho_l(gpu_ctx, hostmirror, abi):
    """(2) (2, 2) on a diffuse floor under a `constant` sky alone: rho L — the sky counts with its own direction's density"""
    flat = sky_scene(hostmirror)
    expected = R.expected_xyz(D.emitter_spectrum(flat.desc, 0) * DM.rho_over_pi(flat.desc), DM.cie_of(flat.desc)) * np.pi
    g = abi.Scene(gpu_ctx, flat)
    try:
        mean, se = direct_mean(g, abi, "sky", expected, 2, 2)
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


# ===================================================================================================== GPU 3: the point light
@pytest.mark.gpu
def test_point_light_is_n_terms_over_n(gpu_ctx, hostmirror, abi):
    """(3) one `point` light, M = 0: N = 3 adds three identical terms over 3 — N = 1 to 1e-5 relative per sample — and both meet
    I cos / d^2 * rho / pi"""
    flat, expected, _ = DM.closed_form_case(hostmirror, "a_plane")
    g = abi.Scene(gpu_ctx, flat)
    try:
        prm = abi.render_params(spp=64, seed=7)
        one, _ = g.sample_pixels_direct(prm, EV.crop_pixels(), 1, 0)
        three, _ = g.sample_pixels_direct(prm, EV.crop_pixels(), 3, 0)
        assert one.min() > 0 and np.all(np.abs(three - one) <= 1e-5 * one)
        for n in (1, 3):
            mean, se = direct_mean(g, abi, "point", expected, n, 0, pixels=EV.crop_pixels())
            assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), (n, (mean - expected) / expected, se / expected)
    finally:
        g.close()


# ===================================================================================================== GPU 4: more samples help
@pytest.mark.gpu
def test_more_samples_cut_the_variance(gpu_ctx, hostmirror, abi):
    """(4) the Cornell box: the per-pixel sample variance at (8, 8) is below that at (1, 1) on every probed pixel with non-zero
    variance (test_more_samples_help_in_float64 has why these pixels)"""
    g = abi.Scene(gpu_ctx, hostmirror.cbox_scene(FW, FH))
    try:
        px = np.array(VAR_PIXELS, np.int32)
        prm = abi.render_params(spp=512, seed=5)
        a, _ = g.sample_pixels_direct(prm, px, 1, 1)
        b, _ = g.sample_pixels_direct(prm, px, 8, 8)
    finally:
        g.close()
    va, vb = a.astype(np.float64).var(1, ddof=1), b.astype(np.float64).var(1, ddof=1)
    print("DIRECT variance ratio (8, 8) / (1, 1), Y:", (vb[:, 1] / va[:, 1]).round(3).tolist())
    assert np.all(va > 0)
    assert np.all(vb[va > 0] < va[va > 0]), (vb / va).tolist()


# ===================================================================================================== GPU 5: variants and shards
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a_cbox", "b_mixed", "c_envmap"])
def test_tree_in_hbm_gives_the_same_bits(gpu_ctx, hostmirror, abi, monkeypatch, name):
    """(5) the same scene created with MSK_LDS_SCENE_KB=0 (k_direct<6>: the tree in HBM) against the LDS-resident form (k_direct<0>)"""
    monkeypatch.delenv("MSK_LDS_SCENE_KB", raising=False)
    prm = abi.render_params(spp=4, seed=3, block_size=BS)
    g = abi.Scene(gpu_ctx, anchor_flat(hostmirror, name))
    want, wpos = g.sample_pixels_direct(prm, all_pixels(), 3, 2)
    film_w, _ = g.render_direct(prm, 3, 2)
    g.close()
    monkeypatch.setenv("MSK_LDS_SCENE_KB", "0")
    g = abi.Scene(gpu_ctx, anchor_flat(hostmirror, name))
    got, gpos = g.sample_pixels_direct(prm, all_pixels(), 3, 2)
    film_g, _ = g.render_direct(prm, 3, 2)
    g.close()
    assert want.max() > 0 and np.array_equal(bits(gpos), bits(wpos))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(film_g), bits(film_w))


@pytest.mark.gpu
def test_shards_and_crop(gpu_ctx, hostmirror, abi):
    """(5) sample shards (0, 2) and (1, 2) together are the whole call's samples; a crop window holds the whole film's pixels"""
    flat = hostmirror.cbox_scene(FW, FH)
    g = abi.Scene(gpu_ctx, flat)
    whole, wpos = g.sample_pixels_direct(abi.render_params(spp=7, seed=9), all_pixels(), 2, 2)
    parts = [g.sample_pixels_direct(abi.render_params(spp=7, seed=9, sample_first=r, sample_stride=2), all_pixels(), 2, 2) for r in (0, 1)]
    film, st = g.render_direct(abi.render_params(spp=4, seed=9, block_size=BS), 2, 2)
    half = [g.render_direct(abi.render_params(spp=4, seed=9, block_size=BS, sample_first=r, sample_stride=2), 2, 2) for r in (0, 1)]
    g.close()
    assert parts[0][0].shape[1] == 4 and parts[1][0].shape[1] == 3
    for r in (0, 1):
        assert np.array_equal(bits(parts[r][0]), bits(whole[:, r::2])) and np.array_equal(bits(parts[r][1]), bits(wpos[:, r::2]))
    assert half[0][1].samples == half[1][1].samples == FW * FH * 2 and st.samples == FW * FH * 4
    assert np.allclose(half[0][0] + half[1][0], film, rtol=2e-6, atol=1e-6)       # (film sums in another order: not bits)
    crop = (5, 3, 12, 9)
    g = abi.Scene(gpu_ctx, hostmirror.cbox_scene(FW, FH, crop=crop))
    window, _ = g.render_direct(abi.render_params(spp=4, seed=9, block_size=BS), 2, 2)
    g.close()
    assert window.shape == (9, 12, 5)
    assert np.array_equal(bits(window), bits(film[3:12, 5:17])) and window[..., :3].max() > 0


@pytest.mark.gpu
def test_passes_of_several_launches(gpu_ctx, hostmirror, abi):
    """(5) a pass is cut into launches of a bounded number of rays (mskplan::make_direct_plan); a record does not care which launch
    wrote it.  25 M records at (1, 1) are two launches: the film is `path`'s at max_depth = 2, bit for bit.  1.3 M records at
    (256, 256) are ten launches of 2048 waves — more than the eight one timed wait covers: the film's pixels inside a crop window
    are those of the window rendered alone, which is one launch."""
    g = abi.Scene(gpu_ctx, hostmirror.cbox_scene(256, 256))
    prm = abi.render_params(spp=384, seed=4, max_depth=2)
    film_d, st_d = g.render_direct(prm, 1, 1)
    film_p, st_p = g.render(prm)
    g.close()
    assert st_d.samples == st_p.samples == 256 * 256 * 384 and st_d.iterations == 2 and st_d.passes == 1
    assert np.array_equal(bits(film_d), bits(film_p)) and film_d[..., :3].max() > 0
    prm = abi.render_params(spp=128, seed=4)
    g = abi.Scene(gpu_ctx, hostmirror.cbox_scene(128, 80))
    film, st = g.render_direct(prm, 256, 256)
    g.close()
    assert st.samples == 128 * 80 * 128 and st.iterations == 10 and st.shadow_rays <= 256 * st.samples and st.segments <= 257 * st.samples
    g = abi.Scene(gpu_ctx, hostmirror.cbox_scene(128, 80, crop=(36, 36, 20, 12)))      # inside ONE block of 32 x 32
    window, wst = g.render_direct(prm, 256, 256)
    g.close()
    assert wst.iterations == 1 and wst.samples < st.samples
    assert np.array_equal(bits(window), bits(film[36:48, 36:56])) and window[..., :3].max() > 0


# ===================================================================================================== GPU 6: statistics
@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1, 1), (4, 2), (0, 3), (5, 0)])
def test_stats(gpu_ctx, hostmirror, abi, n, m):
    g = abi.Scene(gpu_ctx, hostmirror.cbox_scene(FW, FH))
    film, st = g.render_direct(abi.render_params(spp=8, seed=2, block_size=BS), n, m)
    g.close()
    samples = FW * FH * 8
    assert st.samples == samples and st.shadow_rays <= n * samples and samples <= st.segments <= (1 + m) * samples
    assert (n == 0) == (st.shadow_rays == 0) and (m == 0) == (st.segments == samples)
    assert st.invalid_samples == 0 and st.passes == 1 and st.iterations >= 1 and st.ms_total > 0 and st.ms_resolve > 0
    assert (st.launches_trace, st.launches_shade, st.launches_wavefront, st.bytes_shade, st.bytes_trace) == (0, 0, 0, 0, 0)
    assert np.isfinite(film).all() and film[..., :3].max() > 0


# ===================================================================================================== GPU 7: refusals
@pytest.mark.gpu
def test_refusals(gpu_ctx, hostmirror, abi):
    flat = hostmirror.cbox_scene(FW, FH)
    g = abi.Scene(gpu_ctx, flat)
    try:
        for call, code, text in ((lambda: g.render_direct(EV.pcg(abi, spp=2), 1, 1), abi.MSK_ERR_UNSUPPORTED, "MSK_RNG_PCG_BLOCK"),
                                 (lambda: g.sample_pixels_direct(EV.pcg(abi, spp=2), PROBE, 1, 1), abi.MSK_ERR_UNSUPPORTED, "MSK_RNG_PCG_BLOCK"),
                                 (lambda: g.render_direct(abi.render_params(spp=2), 0, 0), abi.MSK_ERR_INVALID_ARG, "must not both be 0"),
                                 (lambda: g.render_direct(abi.render_params(spp=2), 4097, 1), abi.MSK_ERR_INVALID_ARG, '"light_samples"'),
                                 (lambda: g.sample_pixels_direct(abi.render_params(spp=2), PROBE, 1, 4097), abi.MSK_ERR_INVALID_ARG, '"bsdf_samples"')):
            with pytest.raises(abi.MskError) as e:
                call()
            assert e.value.code == code and text in str(e.value), str(e.value)
        film, _ = g.render_direct(abi.render_params(spp=2, rr_depth=0, max_depth=-7), 1, 1)      # rr_depth / max_depth are ignored
        assert film[..., :3].max() > 0
    finally:
        g.close()
    group = abi.Context([0, 0])
    try:
        gs = abi.Scene(group, flat)
        with pytest.raises(abi.MskError) as e:
            gs.render_direct(abi.render_params(spp=2), 1, 1)
        assert e.value.code == abi.MSK_ERR_UNSUPPORTED and "group" in str(e.value)
        gs.close()
    finally:
        group.close()


# ===================================================================================================== GPU: the plugin and the command line
@pytest.mark.gpu
def test_plugin_and_cli_render_a_direct_scene(gpu_ctx, hostmirror, abi, tmp_path):
    """<integrator type="direct"> through scene->integrator()->render() is msk_gpu_render_direct's film; misaki-cli writes an image"""
    hostlib = EV.host_library()
    xml = direct_xml(hostmirror, tmp_path, {"light_samples": 2, "bsdf_samples": 3, "block_size": BS})
    sc = hostlib.HostScene(xml)
    film, rgba, st = sc.render()
    flat = sc.flatten()
    g = abi.Scene(gpu_ctx, flat)
    want, wst = g.render_direct(flat.params, 2, 3)
    g.close()
    sc.close()
    assert st.samples == wst.samples == FW * FH * 4 and np.array_equal(bits(film), bits(want)) and film[..., :3].max() > 0
    import test_host_library as HL
    out = tmp_path / "image.exr"
    r = subprocess.run([HL._cli(), xml, "-o", str(out), "-D", "spp=2", "-q"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = out.read_bytes()
    assert len(raw) > FW * FH * 16 and np.frombuffer(raw[-FW * FH * 16:], np.float32).max() > 0      # (as test_host_library reads it)
