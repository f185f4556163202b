"""The `mask` BSDF (include/msk_gpu.h at msk_mask_desc; DESIGN.md section 9, departures 6-8): an opacity cutout with a null lobe.

In this file the oracle sees no mask (its restatement of the mask, and the device against it bit for bit, are in
test_widened_oracle_parity.py); here the device is held in three ways: to the fp32 restatement (mask_ref.py) bit for bit through the probes,
to the oracle where it can follow (a = 1 is the nested BSDF, to the bit), and to float64 closed forms.

CPU: the restatement checks itself; the packer, its refusals and the launch plan as a stand-alone native program (also under
AddressSanitizer / UBSan); the two flatteners; exports and struct layouts; the closed forms' own convergence.
GPU: probes; a = 1 parity; closed forms; execution variants; refusals.

Measured on an MI355X when the feature was added (counter RNG, crop of 8 x 8 pixels, spp as the procedure chose it): see the
prints of test_rendered_radiance_meets_the_closed_form; every case sat inside 6 standard errors + 1e-3 of its expectation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bitmap_ref as BR
import delta_ref as D
import mask_ref as M
import radiometry_ref as R
import test_delta_light_mirror as DM
import test_envmap as EV
import test_launch_plan as LP
import test_table_placement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CAM, W48, CROP = EV.PLANE_CAMERA, EV.W48, EV.CROP
SKY = DM.SKY
RHO = (0.6, 0.5, 0.4)
bits = DM.bits
UV_QUAD = [((0, 0), (1, 0), (1, 1), (0, 1))]
INV_PI = F(0.31830988618379067154)
CUTOUT = np.array([[1, 0], [0, 1]], F)                                   # (c): the 2 x 2 nearest image


def masked(nested=None, opacity=0.5):
    spec = {"type": "mask", "bsdf": nested or {"type": "diffuse"}}
    if opacity is not None:
        spec["opacity"] = opacity
    return spec


def image(pixels, filt="nearest", **kw):
    return dict({"type": "bitmap", "pixels": np.asarray(pixels, F), "filter": filt}, **kw)


# ===================================================================================================== CPU: the restatement
def test_restatement_checks_itself():
    """fp32 against float64: the opacity lookups (away from texel borders), the lobe choice, the constants' special cases"""
    rng = np.random.RandomState(3)
    vals = rng.uniform(0, 1, (2, 3)).astype(F)
    to_uv = (1.5, 0.25, 0.125, -0.5, 2.0, 0.75)
    uv = rng.uniform(-2, 2, (4096, 2)).astype(F)
    for filt in (1, 2):
        mask = {"filter": filt, "values": vals, "to_uv": to_uv}
        fu, fv = BR.frac_uv(to_uv, uv)
        px, py = fu.astype(np.float64) * 3 - (0.5 if filt == 2 else 0.0), fv.astype(np.float64) * 2 - (0.5 if filt == 2 else 0.0)
        far = (np.abs(px - np.round(px)) > 1e-3) & (np.abs(py - np.round(py)) > 1e-3) & (fu > 1e-3) & (fu < 1 - 1e-3) & (fv > 1e-3) & (fv < 1 - 1e-3)
        a32, a64 = M.opacity32(mask, uv), M.opacity64(mask, uv)
        assert far.sum() > 3000 and np.all(np.abs(a32[far] - a64[far]) <= 4e-6), float(np.abs(a32[far] - a64[far]).max())
        assert np.all((a32 >= 0) & (a32 <= 1))
    # an image of equal values is the constant, to the bit (a + t (a - a))
    for c in (0.0, 2.0 ** -24, 0.3, 1.0 - 2.0 ** -24, 1.0):
        flat_img = {"filter": 2, "values": np.full((2, 3), c, F), "to_uv": to_uv}
        assert np.array_equal(bits(M.opacity32(flat_img, uv)), bits(M.opacity32({"filter": 0, "opacity": c}, uv)))
    # the lobe choice: a = 0 never nested, a = 1 always and exactly; the rescaled u.x stays in [0, 1)
    u = np.concatenate([rng.uniform(0, 1, 4093), [0.0, 0.5, 1.0 - 2.0 ** -24]]).astype(F)
    assert not M.pick32(np.zeros_like(u), u)[0].any()
    nested, ux = M.pick32(np.ones_like(u), u)
    assert nested.all() and np.array_equal(bits(ux), bits(u))
    a = rng.uniform(0.01, 1, 4096).astype(F)
    nested, ux = M.pick32(a, u)
    assert np.all(ux[nested] < 1.0) and np.all(ux[nested] >= 0) and np.array_equal(ux[~nested], u[~nested])
    assert np.allclose(ux[nested], u[nested].astype(np.float64) / a[nested], rtol=1e-7)
    # sample32 / eval32 with a hand-made X against the float64 forms
    def x32(k, wi, s1, uu):
        return np.stack([uu[:, 0], uu[:, 1], np.ones(len(k), F)], -1), np.full(len(k), 0.25, F), np.full((len(k), 4), 0.5, F), np.ones(len(k), F), np.ones(len(k), bool)
    wi = np.tile(np.array([0.0, 0.6, 0.8], F), (4096, 1))
    got = M.sample32(a, wi, u, np.stack([u, u[::-1]], -1), x32, False)
    for i in (0, 1, 2, 4093, 4094, 4095):
        wo, pdf, val = M.sample64(float(a[i]), (float(u[i]), float(u[::-1][i])), lambda q: (np.array([q[0], q[1], 1.0]), 0.25, 0.5))
        assert got["null"][i] == (wo is None) and abs(got["pdf"][i] - pdf) <= 1e-6 and np.all(np.abs(got["value"][i] - val) <= 1e-7)
        assert got["delta"][i] == (wo is None) and got["ok"][i]
        assert np.array_equal(got["wo"][i], -wi[i]) if wo is None else np.allclose(got["wo"][i], wo, atol=1e-6)
    v, p = M.eval32(a, np.full((4096, 4), 0.5, F), np.full(4096, 0.25, F))
    assert np.allclose(v, 0.5 * a[:, None].astype(np.float64), rtol=1e-7) and np.allclose(p, 0.25 * a.astype(np.float64), rtol=1e-7)


@pytest.mark.parametrize("a", [0.0, 0.25, 0.5, 1.0])
def test_sampling_reproduces_eval(a):
    """Lobe frequencies and the a-weighted mean of sample() over a quadrature in u reproduce eval: the integral of value * g(wo)
    over the nested branch is the integral of eval(wo) g(wo) over the hemisphere, g = 1 and g = wo.z^2 (polynomials in u: the rule is exact); the null branch has
    measure 1 - a = its pdf and value 1.  The reference's a^2 weighting, restated, is off by the factor a."""
    rho = 0.7
    x = M.diffuse_sample64(rho)
    t, w = R.gauss_legendre(32)
    ours, written, null_mass, pdf_ok = np.zeros(2), np.zeros(2), 0.0, True
    for lo, hi in ((0.0, a), (a, 1.0)):
        if hi <= lo:
            continue
        for tx, wx in zip(lo + (hi - lo) * t, (hi - lo) * w):
            for ty, wy in zip(t, w):
                wo, pdf, val = M.sample64(a, (tx, ty), x)
                wo2, pdf2, val2 = M.sample_as_written64(a, (tx, ty), x)
                if wo is None:
                    null_mass += wx * wy * val
                    pdf_ok &= pdf == 1.0 - a and val2 == 1.0
                    continue
                _, p_eval = M.diffuse_eval64(rho, wo)
                pdf_ok &= abs(pdf - a * p_eval) <= 1e-12
                ours += wx * wy * val * np.array([1.0, wo[2] ** 2])
                written += wx * wy * val2 * np.array([1.0, wo2[2] ** 2])
    # integral of a rho / pi cos over the hemisphere = a rho; times cos^2: a rho / 2
    want = a * rho * np.array([1.0, 0.5])
    assert pdf_ok and abs(null_mass - (1.0 - a)) <= 1e-12
    assert np.all(np.abs(ours - want) <= 1e-6 * max(a, 1e-9) + 1e-12), (ours, want)
    assert np.all(np.abs(written - a * want) <= 1e-6 * max(a, 1e-9) + 1e-12)          # a^2: off by the factor a
    if 0 < a < 1:
        assert np.all(np.abs(written - want) >= (1 - a) * want * 0.999)


def test_as_written_would_miss_closed_form_a(hostmirror):
    """closed form (a) at a = 0.25 from the float64 side: the restated mask.cpp:47,53,68 (sample_as_written64) over the quadrature
    of test_sampling_reproduces_eval reflects a^2 rho where this back end reflects a rho; on the scene of (a) that is 0.1875 rho L
    less, far outside the test's bound of six standard errors (at most 3 %) + 0.1 % of the expectation"""
    a = 0.25
    flat = quad_under_sky(hostmirror, a)
    t, w = R.gauss_legendre(16)
    reflected = {"ours": 0.0, "written": 0.0}           # the nested branch's mass of value (in units of rho): integral over u.x < a
    for tx, wx in zip(a * t, a * w):
        for ty, wy in zip(t, w):
            reflected["ours"] += wx * wy * M.sample64(a, (tx, ty), M.diffuse_sample64(1.0))[2]
            reflected["written"] += wx * wy * M.sample_as_written64(a, (tx, ty), M.diffuse_sample64(1.0))[2]
    assert abs(reflected["ours"] - a) <= 1e-12 and abs(reflected["written"] - a * a) <= 1e-12
    ours, written = (mixed_xyz(flat.desc, 0, 0, reflected[k], 1.0 - a) for k in ("ours", "written"))
    expected = closed_form_case(hostmirror, "a_quad_025")[1]
    assert np.all(np.abs(ours - expected) <= 1e-12 * expected)
    lost = mixed_xyz(flat.desc, 0, 0, 0.1875, 0.0)
    assert np.all(np.abs((ours - written) - lost) <= 1e-9 * lost)
    assert np.all(ours - written > 0.031 * expected + 1e-3 * expected), (ours - written) / expected


# ===================================================================================================== CPU: native, layout, hosts
@pytest.fixture(scope="module")
def native_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mask_tables")
    src = os.path.join(ROOT, "tests", "native", "mask_tables_check.cpp")
    plain, san = str(d / "mask_tables_check"), str(d / "mask_tables_check_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    return plain, san


def test_native_packer_check(native_exe):
    """layout, every refusal, a scene without masks packing to the parent's bytes, the plan's byte sums: plain and sanitized"""
    for exe in native_exe:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[0] == "ok", r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("knobs", LP.KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_plan_with_a_mask(native_exe, knobs):
    """has_mask selects SHADE_MASK over every other family and changes nothing else; without it the plan is what it was"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs)
    r = subprocess.run([native_exe[0], "plan"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.split() == ["cases", str(7 * 256 * 4 * len(LP.REGION_SIZES) * len(LP.LDS))]


def test_exports_and_struct_layouts(abi, tmp_path):
    src = tmp_path / "off.c"
    names = ("bsdf", "opacity", "filter", "to_uv", "width", "height", "values")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msk_gpu.h"\nint main(){printf("%zu ' + "%zu " * len(names) + '%zu %zu %zu %zu %zu %zu %d\\n",sizeof(msk_mask_desc),'
                   + ",".join("offsetof(msk_mask_desc,%s)" % n for n in names) +
                   ',sizeof(msk_scene_masks),offsetof(msk_scene_masks,ext),offsetof(msk_scene_masks,n_masks),offsetof(msk_scene_masks,masks),sizeof(msk_scene_ext),sizeof(msk_bsdf_desc),MSK_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    k, e = abi.MaskDesc, abi.SceneMasks
    assert got == [C.sizeof(k)] + [getattr(k, n).offset for n in names] + [C.sizeof(e), e.ext.offset, e.n_masks.offset, e.masks.offset, C.sizeof(abi.SceneExt),
                                                                            C.sizeof(abi.BsdfDesc), abi.MSK_ABI_VERSION]
    assert got[:8] == [56, 0, 4, 8, 12, 36, 40, 48] and got[8:] == [40, 0, 24, 32, 24, 132, 8]       # (the last three: what they were)
    import __graft_entry__ as ge
    ge.build_gpu_library()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("msk_gpu_scene_create_masks", "msk_gpu_mask_sample", "msk_gpu_mask_eval"):
        assert name in abi.EXPORTS and getattr(lib, name) is not None
    blob = open(abi.LIB_PATH, "rb").read()
    for kname in (b"k_shade_gen_m", b"k_wavefront_m", b"k_wavefront_h_m", b"k_path_serial_m", b"k_mask_probe"):
        assert kname in blob, kname


def quad(hm, name, bsdf, y=0.0, size=1.0, reflectance=RHO, uv=False):
    s = float(size)
    return hm.MeshSpec(name, [((-s, y, s), (s, y, s), (s, y, -s), (-s, y, -s))], reflectance, bsdf=bsdf, texcoords=UV_QUAD if uv else None)


def flattener_meshes(hm):
    rng = np.random.RandomState(5)
    grey, colour = rng.uniform(0, 1, (2, 3)).astype(F), rng.uniform(0, 1, (3, 2, 3)).astype(F)
    shared = {"type": "roughconductor", "alpha": 0.2, "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14)}
    return [quad(hm, "constant", masked(None, 0.375), 0.0),
            quad(hm, "grey_image", masked({"type": "conductor"}, image(grey, "nearest", scale=(3, 2))), 0.2, uv=True),
            quad(hm, "colour_image", masked({"type": "dielectric"}, image(colour, "bilinear", matrix=(0.5, 0.25, 0.125, 0, -1.5, 2, 0.75, 0, 0, 0, 1, 0, 0, 0, 0, 1))), 0.3, uv=True),
            quad(hm, "twosided_default", masked({"type": "diffuse", "twosided": True}, None), 0.4),
            quad(hm, "colour", masked(None, (0.2, 0.7, 0.4)), 0.5),
            quad(hm, "grey_rgb", masked(None, (0.3, 0.3, 0.3)), 0.6),
            quad(hm, "shared_plain", dict(shared), 0.7),
            quad(hm, "shared_masked", masked(dict(shared), 0.0), 0.8)]          # (eight shapes: the loader orders more than that by their generated names)


def test_the_two_flatteners_agree(hostmirror, abi, tmp_path):
    """a constant mask, the default opacity, image masks (grey and coloured, nearest and bilinear, scaled and under a matrix),
    mask(twosided(diffuse)), colour opacities, and a BSDF shared by a masked and an unmasked mesh: the same descriptors byte for
    byte; every refusal in the same words"""
    hostlib = EV.host_library()
    meshes = flattener_meshes(hostmirror)
    xml = hostmirror.write_scene_xml(meshes, str(tmp_path / "s"), 16, 16, 1, camera=CAM)
    text = open(xml).read()
    assert text.count('<bsdf type="mask">') == 7 and text.count('name="opacity"') == 6 and text.count('<bsdf type="twosided">') == 1
    h = hostlib.HostScene(xml).flatten()
    m = hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, coeff_lookup=hostlib.srgb_model_fetch)
    assert h.desc.n_bsdfs == m.desc.n_bsdfs == 8 and len(h.masks) == len(m.masks) == 7
    for i in range(8):
        assert bytes(h.desc.bsdfs[i]) == bytes(m.desc.bsdfs[i]), i
    assert [k.bsdf for k in m.masks] == [0, 1, 2, 3, 4, 5, 7]          # two meshes that share X, one masked: two entries, one mask
    for a, b in zip(h.masks, m.masks):
        assert (a.bsdf, a.filter, a.width, a.height) == (b.bsdf, b.filter, b.width, b.height) and list(a.to_uv) == list(b.to_uv), b.bsdf
        assert bits(np.array([a.opacity])) == bits(np.array([b.opacity])), b.bsdf
        if b.filter:
            n = b.width * b.height
            assert np.array_equal(bits(np.ctypeslib.as_array(a.values, (n,))), bits(np.ctypeslib.as_array(b.values, (n,)))), b.bsdf
    k = m.masks
    assert [x.filter for x in k] == [0, 1, 2, 0, 0, 0, 0] and (k[1].width, k[1].height, k[2].width, k[2].height) == (3, 2, 2, 3)
    assert (k[0].opacity, k[3].opacity, k[5].opacity, k[6].opacity) == (0.375, 0.5, F(0.3), 0.0)
    assert k[4].opacity == (F(0.212671) * F(0.2) + F(0.715160) * F(0.7)) + F(0.072169) * F(0.4)
    assert list(k[1].to_uv) == [3, 0, 0, 0, 2, 0] and list(k[2].to_uv) == [0.5, 0.25, 0.125, -1.5, 2, 0.75]
    assert m.desc.bsdfs[3].back_bsdf == 3 and m.desc.bsdfs[1].type == abi.MSK_BSDF_CONDUCTOR and m.desc.bsdfs[6].type == m.desc.bsdfs[7].type == abi.MSK_BSDF_ROUGHCONDUCTOR
    # the refusals, worded alike
    inner = '<bsdf type="mask"><float name="opacity" value="0.5"/><bsdf type="diffuse"/></bsdf>'
    cases = [({"type": "mask", "twosided": True, "bsdf": {"type": "diffuse"}}, '<bsdf type="twosided">' + inner + '</bsdf>', hostmirror.MASK_TWOSIDED),
             (masked(masked(None, 0.5), 0.5), '<bsdf type="mask">' + inner + '</bsdf>', hostmirror.MASK_NESTED),
             ({"type": "mask", "opacity": 0.5}, '<bsdf type="mask"><float name="opacity" value="0.5"/></bsdf>', hostmirror.MASK_CHILDREN),
             (None, '<bsdf type="mask"><bsdf type="diffuse"/><bsdf type="diffuse"/></bsdf>', hostmirror.MASK_CHILDREN),
             (dict(masked(None, 0.5), alpha={"type": "checkerboard", "color0": (0.1, 0.1, 0.1), "color1": (0.2, 0.2, 0.2)}),
              '<bsdf type="mask"><texture name="alpha" type="checkerboard"><rgb name="color0" value="0.1"/><rgb name="color1" value="0.2"/></texture><bsdf type="diffuse"/></bsdf>',
              hostmirror.MASK_UNKNOWN % "alpha")]
    plain = hostmirror.write_scene_xml([quad(hostmirror, "q", None)], str(tmp_path / "r"), 16, 16, 1, camera=CAM)
    text = open(plain).read()
    start, end = text.index("<bsdf"), text.index("</bsdf>") + len("</bsdf>")
    for n, (spec, element, words) in enumerate(cases):
        if spec is not None:
            with pytest.raises(ValueError) as e:
                hostmirror.flatten([quad(hostmirror, "q", spec)], 16, 16, camera=CAM)
            assert words in str(e.value)
        path = tmp_path / "r" / ("bad%d.xml" % n)
        path.write_text(text[:start] + element + text[end:])
        with pytest.raises(hostlib.HostError) as e:
            hostlib.HostScene(str(path)).flatten()
        assert words in str(e.value), (n, str(e.value))


# ===================================================================================================== float64 expectations
def sky_xyz(desc, e):
    return R.expected_xyz(D.emitter_spectrum(desc, e), DM.cie_of(desc))


def mixed_xyz(desc, e, b, reflected, through):
    """E[XYZ] of `reflected` rho L + `through` L"""
    l_s, rop = D.emitter_spectrum(desc, e), DM.rho_over_pi(desc, b)
    return R.expected_xyz(R.Spectrum(lambda lam: l_s(lam) * (reflected * np.pi * rop(lam) + through), l_s.breaks), DM.cie_of(desc))


def quad_under_sky(hm, a, flip=False, twosided=True):
    spec = masked({"type": "diffuse", "twosided": True} if twosided else {"type": "diffuse"}, a)
    return hm.flatten([DM.plane(hm, spec, flip=flip)], W48, W48, camera=CAM, env=SKY)


LIGHT_Z = 1.2                                                            # over the floor points the crop sees (z = 0.69 .. 1.72)
LIGHT = [(1.0, 1.0, LIGHT_Z - 1.0), (1.0, 1.0, LIGHT_Z + 1.0), (-1.0, 1.0, LIGHT_Z + 1.0), (-1.0, 1.0, LIGHT_Z - 1.0)]       # 2 x 2 at height 1, wound to face down (as DM.LAMP)
SCREEN_Y, SCREEN_HALF = 0.9, 1.4


def cutout_light_flat(hm, a=0.5):
    """(b) a diffuse floor, a one-sided 2 x 2 light at height 1 and a black masked screen just under it, larger than it"""
    s = SCREEN_HALF
    screen = hm.MeshSpec("screen", [((-s, SCREEN_Y, LIGHT_Z + s), (s, SCREEN_Y, LIGHT_Z + s), (s, SCREEN_Y, LIGHT_Z - s), (-s, SCREEN_Y, LIGHT_Z - s))], (0.0, 0.0, 0.0), bsdf=masked({"type": "diffuse", "twosided": True}, a))
    lamp = hm.MeshSpec("lamp", [tuple(LIGHT)], hm.LUMINAIRE, radiance=(40, 30, 20))
    return hm.flatten([DM.plane(hm), screen, lamp], W48, W48, camera=CAM)


def cutout_light_expected(desc, a, m):
    o, d, w = DM.crop_rays(desc, m)
    x = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
    # every segment from a seen floor point to the light crosses the screen, and the camera's rays pass beside it
    rel = x[..., [0, 2]] - np.array([0.0, LIGHT_Z])
    assert np.all(np.abs(rel) < 1.0) and np.all((1 - SCREEN_Y) * np.abs(rel) + SCREEN_Y * 1.0 < SCREEN_HALF)
    t = (SCREEN_Y - o[1]) / d[..., 1]
    assert np.all((o[2] + t * d[..., 2]) > LIGHT_Z + SCREEN_HALF)
    g = float((w * R.polygon_irradiance(x, (0, 1, 0), np.array(LIGHT, np.float64))).sum())
    return (1.0 - a) * g * R.expected_xyz(D.emitter_spectrum(desc, 0) * DM.rho_over_pi(desc, 0), DM.cie_of(desc))


CANOPY = [(-20.0, 1.0, 1.0), (20.0, 1.0, 1.0), (20.0, 1.0, -30.0), (-20.0, 1.0, -30.0)]


def canopy_flat(hm):
    """(d) a diffuse floor seen beside an a = 0 canopy that hangs over it: the floor receives the sky through the canopy"""
    canopy = hm.MeshSpec("canopy", [tuple(CANOPY)], RHO, bsdf=masked({"type": "diffuse", "twosided": True}, 0.0))
    return hm.flatten([DM.plane(hm), canopy], W48, W48, camera=CAM, env=SKY)


def closed_form_case(hm, name):
    """-> (flat, expectation at 4 x 4 nodes over the crop, the same at 8 x 8, render parameters)"""
    if name.startswith("a_quad_"):
        a = {"a_quad_0": 0.0, "a_quad_025": 0.25, "a_quad_1": 1.0}[name]
        flat = quad_under_sky(hm, a)
        e = mixed_xyz(flat.desc, 0, 0, a, 1.0 - a)
        return flat, e, e, dict(max_depth=2)
    if name == "b_light_through_a_cutout":
        flat = cutout_light_flat(hm)
        return flat, cutout_light_expected(flat.desc, 0.5, 4), cutout_light_expected(flat.desc, 0.5, 8), dict(max_depth=3)
    if name in ("d_floor_beside_the_canopy", "d_floor_beside_the_canopy_hidden"):
        flat = canopy_flat(hm)
        o, d, _ = DM.crop_rays(flat.desc, 8)
        t = (1.0 - o[1]) / d[..., 1]
        assert np.all(o[2] + t * d[..., 2] > 1.5)                        # the camera sees the floor beside the canopy, not through it
        e = mixed_xyz(flat.desc, 0, 0, 1.0, 0.0)
        return flat, e, e, dict(max_depth=3, hide_emitters=int(name.endswith("hidden")))
    if name == "e_one_sided_from_behind":
        flat = quad_under_sky(hm, 0.5, flip=True, twosided=False)
        e = mixed_xyz(flat.desc, 0, 0, 0.0, 0.5)
        return flat, e, e, dict(max_depth=2)
    raise KeyError(name)


CASES = ["a_quad_0", "a_quad_025", "a_quad_1", "b_light_through_a_cutout", "d_floor_beside_the_canopy", "d_floor_beside_the_canopy_hidden", "e_one_sided_from_behind"]


@pytest.mark.parametrize("name", CASES)
def test_expectations_have_converged(hostmirror, name):
    """the 4 x 4 Gauss-Legendre rule over the crop against 8 x 8 (the cases without geometry have one expectation everywhere); and
    the wavelength quadrature of expected_xyz at 16 against 32 nodes"""
    flat, e4, e8, _ = closed_form_case(hostmirror, name)
    print("MASK %s: expectation %s (8 x 8 nodes: %s)" % (name, e4, e8))
    assert np.all(e4 > 0) and np.all(np.abs(e4 - e8) <= 1e-5 * e8)
    s = D.emitter_spectrum(flat.desc, 0) * DM.rho_over_pi(flat.desc, 0)
    assert np.all(np.abs(R.expected_xyz(s, DM.cie_of(flat.desc), 16) - R.expected_xyz(s, DM.cie_of(flat.desc), 32)) <= 1e-5 * R.expected_xyz(s, DM.cie_of(flat.desc), 32))


# ===================================================================================================== GPU 1: the probes
NESTED = {"diffuse_bitmap": {"type": "diffuse", "texture": {"type": "bitmap", "pixels": np.random.RandomState(8).uniform(0.1, 0.9, (2, 3, 3)).astype(F), "scale": (2, 3)}},
          "roughconductor": {"type": "roughconductor", "alpha": (0.2, 0.35), "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14)},
          "roughdielectric": {"type": "roughdielectric", "alpha": 0.15, "int_ior": 1.5, "ext_ior": 1.0},
          "dielectric": {"type": "dielectric"},
          "conductor": dict(DM.GOLD_RGB)}
PROBE_IMAGE = np.array([[0.0, 0.25, 1.0], [0.75, 0.5, 2.0 ** -24]], F)                   # 3 x 2
PROBE_TO_UV = (1.5, 0.25, 0.125, 0, -0.5, 2.0, 0.75, 0, 0, 0, 1, 0, 0, 0, 0, 1)
OPACITIES = {"a0": 0.0, "a_tiny": 2.0 ** -24, "a_half": 0.5, "a_below_one": 1.0 - 2.0 ** -24, "a1": 1.0,
             "nearest": image(PROBE_IMAGE, "nearest", matrix=PROBE_TO_UV), "bilinear": image(PROBE_IMAGE, "bilinear", matrix=PROBE_TO_UV)}


def probe_entries():
    """(name, nested spec) of the ten entries: five X, one-sided and twosided (a dielectric has no twosided form: it comes twice)"""
    out = []
    for name, spec in NESTED.items():
        out.append((name, dict(spec)))
        out.append((name + "_twosided", dict(spec, twosided=True) if name not in ("dielectric", "roughdielectric") else dict(spec)))
    return out


def probe_inputs(rng, n):
    """uv on and beside texel borders of the 3 x 2 image under PROBE_TO_UV's inverse, at negative coordinates and anywhere; wi on
    both faces; u.x around the opacities"""
    m = np.array(PROBE_TO_UV, np.float64).reshape(4, 4)
    a2, t2 = m[:2, :2], np.array([m[0, 2], m[1, 2]])
    tex = np.stack([rng.randint(-4, 5, n) / 3.0, rng.randint(-3, 4, n) / 2.0], -1)      # texel borders (and, shifted by half, centres)
    tex[n // 4:n // 2] += [0.5 / 3.0, 0.25]
    tex[n // 2:] = rng.uniform(-1.5, 1.5, (n - n // 2, 2))
    uv = np.linalg.solve(a2, (tex - t2).T).T.astype(F)
    uv[::7] = np.nextafter(uv[::7], F(10))
    uv[3::7] = np.nextafter(uv[3::7], F(-10))
    wi = rng.normal(size=(n, 3))
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(F)
    wi[::16] = [0, 0, 1]
    wi[5::16, 2] = -np.abs(wi[5::16, 2])
    wo = rng.normal(size=(n, 3))
    wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(F)
    su = rng.uniform(0, 1, (n, 3)).astype(F)
    su[::5, 1] = rng.choice(np.array([0.0, 2.0 ** -25, 2.0 ** -24, 0.25, 0.5, np.nextafter(F(0.5), F(0)), 0.75, 1.0 - 2.0 ** -24], F), len(su[::5]))
    wl = rng.uniform(360, 830, (n, 4)).astype(F)
    return uv, wi, wo, su, wl


def nested_restatement(oracle, abi, flat, b, name, uv, wl):
    """-> (x_sample, x_eval, x_delta) of BSDF entry b through the oracle (dielectric, roughdielectric, roughconductor, and the
    directions of diffuse), delta_ref (conductor) and bitmap_ref (the diffuse reflectance)"""
    d = flat.desc
    descs = [d.bsdfs[i] for i in range(d.n_bsdfs)]
    bd = d.bsdfs[b]
    base = name.replace("_twosided", "")
    refl = None
    if base == "diffuse_bitmap":
        td = d.textures[bd.reflectance_texture - 1]
        coeffs = flat.texels[td.first_texel:td.first_texel + td.width * td.height].reshape(td.height, td.width, 3)
        refl = BR.lookup(BR.oracle_texels(oracle, coeffs), td.width, td.height, "bilinear", list(td.to_uv), uv, wl)

    def flip(w):
        w = np.array(w, F)
        if bd.back_bsdf >= 0 and w[2] < 0:
            return w * np.array([1, 1, -1], F), True
        return w, False

    def x_sample(k, wi, s1, u):
        wo, pdf, val, eta, ok = np.zeros((len(k), 3), F), np.zeros(len(k), F), np.zeros((len(k), 4), F), np.ones(len(k), F), np.zeros(len(k), bool)
        for j, i in enumerate(k):
            if base == "conductor":
                w, fl = flip(wi[j])
                if w[2] > 0:
                    v = D.conductor_sample32(w[2:3], D.spectrum32(oracle, bd.eta, wl[i:i + 1]), D.spectrum32(oracle, bd.k, wl[i:i + 1]), D.spectrum32(oracle, bd.specular_reflectance, wl[i:i + 1]))
                    wo[j], pdf[j], val[j], ok[j] = (-w[0], -w[1], -w[2] if fl else w[2]), 1.0, v[0], True
                elif fl:
                    wo[j, 2] = -0.0
                continue
            o, p, v, e, typ = oracle.bsdf_sample2(descs, b, wi[j], float(s1[j]), u[j], wl[i])
            wo[j], pdf[j], val[j], eta[j], ok[j] = o, p, v, e, typ != 0
            if refl is not None:
                val[j] = refl[i] if p > 0 else 0.0
        return wo, pdf, val, eta, ok

    def x_eval(wi, wo):
        val, pdf = np.zeros((len(wi), 4), F), np.zeros(len(wi), F)
        for i in range(len(wi)):
            if base in ("conductor", "dielectric"):
                continue
            v, p = oracle.bsdf_eval(descs, b, wi[i], wo[i], wl[i])
            val[i], pdf[i] = v, p
            if refl is not None:
                w, fl = flip(wi[i])
                co = F(-wo[i][2]) if fl else F(wo[i][2])
                inside = w[2] > 0 and co > 0
                val[i] = ((refl[i] * INV_PI).astype(F) * co).astype(F) if inside else 0.0     # (refl * MSK_INV_PI_F) * cos_o
        return val, pdf
    return x_sample, x_eval, base in ("conductor", "dielectric")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(OPACITIES))
def test_probes_equal_the_restatement_bit_for_bit(gpu_ctx, oracle, hostmirror, abi, kind):
    """(1) msk_gpu_mask_sample / msk_gpu_mask_eval against mask_ref over the nested restatements: 10 entries x 64 inputs per kind of
    opacity (7 kinds: 4480 inputs)"""
    entries = probe_entries()
    meshes = [quad(hostmirror, name, masked(spec, OPACITIES[kind]), 0.1 * i, uv=True) for i, (name, spec) in enumerate(entries)]
    meshes.append(hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20)))
    flat = hostmirror.flatten(meshes, 16, 16, camera=CAM, coeff_lookup=None)
    g = abi.Scene(gpu_ctx, flat)
    rng = np.random.RandomState(sorted(OPACITIES).index(kind))
    try:
        for b, (name, _) in enumerate(entries):
            uv, wi, wo_in, su, wl = probe_inputs(rng, 64)
            k = flat.masks[b]
            mask = {"filter": k.filter, "opacity": k.opacity, "to_uv": list(k.to_uv)}
            if k.filter:
                mask["values"] = np.ctypeslib.as_array(k.values, (k.height, k.width))
            a = M.opacity32(mask, uv)
            x_sample, x_eval, x_delta = nested_restatement(oracle, abi, flat, b, name, uv, wl)
            want = M.sample32(a, wi, su[:, 0], su[:, 1:], x_sample, x_delta)
            wo_pdf, value, flags = g.mask_sample(b, uv, wi, su, wl)
            assert np.array_equal(flags[:, 2] != 0, want["null"]), (kind, name)
            assert np.array_equal(flags[:, 1] != 0, want["delta"]), (kind, name)
            assert np.all(flags[want["null"], 3] == 1)
            for what, got, ref in (("wo", wo_pdf[:, :3], want["wo"]), ("pdf", wo_pdf[:, 3], want["pdf"]), ("value", value, want["value"]), ("eta", flags[:, 0], want["eta"])):
                bad = (bits(got) != bits(ref)).reshape(len(a), -1).any(-1)
                assert not bad.any(), (kind, name, what, int(bad.sum()), got[bad][:3], ref[bad][:3], a[bad][:3], su[bad][:3], wi[bad][:3])
            a_pdf, ev = g.mask_eval(b, uv, wi, wo_in, wl)
            xv, xp = x_eval(wi, wo_in)
            rv, rp = M.eval32(a, xv, xp)
            assert np.array_equal(bits(a_pdf[:, 0]), bits(a)), (kind, name, a_pdf[:4, 0], a[:4])
            for what, got, ref in (("eval", ev, rv), ("eval pdf", a_pdf[:, 1], rp)):
                bad = (bits(got) != bits(ref)).reshape(len(a), -1).any(-1)
                assert not bad.any(), (kind, name, what, int(bad.sum()), got[bad][:3], ref[bad][:3])
            if kind == "a0":
                assert want["null"].all() and not ev.any()
            if kind == "a1":
                assert not want["null"].any()
        with pytest.raises(abi.MskError) as err:
            g.mask_sample(len(entries) + 1, uv[:1], wi[:1], su[:1], wl[:1])
        assert "out of range" in str(err.value) and err.value.code == abi.MSK_ERR_INVALID_ARG
    finally:
        g.close()


# ===================================================================================================== GPU 2: a = 1 is the nested BSDF
def with_masks(abi, flat, values=None):
    """the same scene with a mask of 1 on every entry: a constant, or the image `values`"""
    n = flat.desc.n_bsdfs
    arr = (abi.MaskDesc * n)()
    for b in range(n):
        arr[b].bsdf, arr[b].opacity, arr[b].filter = b, 1.0, 0
        if values is not None:
            arr[b].filter, arr[b].height, arr[b].width = 2, values.shape[0], values.shape[1]
            arr[b].values = values.ctypes.data_as(C.POINTER(C.c_float))
            arr[b].to_uv[:] = [1, 0, 0, 0, 1, 0]
    flat.masks = arr
    flat.keep.append(values)
    return flat


PARITY_PARAMS = [("counter", 0), ("counter", 1), ("pcg", 0), ("pcg", 1)]
PARITY_KNOBS = [{}, {"MSK_LDS_SCENE_KB": "0"}, {"MSK_FUSED": "1"}, {"MSK_LDS_SCENE_KB": "0", "MSK_FUSED_HBM": "0"}, {"MSK_LDS_SCENE_KB": "0", "MSK_FUSED": "1"}]


def parity_prm(abi, rng, hide):
    return abi.render_params(spp=4, seed=3, hide_emitters=hide) if rng == "counter" else EV.pcg(abi, spp=4, seed=3, hide_emitters=hide)


def some_pixels(w, h):
    return np.array([(x, y) for y in range(0, h, 5) for x in range(0, w, 3)], np.int32)


@pytest.fixture(scope="module")
def cbox_oracle(oracle, hostmirror, abi):
    """the oracle's films and samples of the Cornell box WITHOUT masks at 32 x 32, 4 spp: computed once, never changed"""
    o = oracle.scene(hostmirror.cbox_scene(32, 32))
    out = {}
    for rng, hide in PARITY_PARAMS:
        film, st = o.render(parity_prm(abi, rng, hide), threads=8)
        film.setflags(write=False)
        out[(rng, hide)] = (film, st.samples)
    xyz, pos = o.sample_pixels(parity_prm(abi, "counter", 0), some_pixels(32, 32))
    xyz.setflags(write=False)
    out["samples"] = (xyz, pos)
    o.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", PARITY_KNOBS, ids=EV.variant_id)
@pytest.mark.parametrize("form", ["constant", "image"])
def test_opacity_one_is_the_nested_bsdf_to_the_bit(gpu_ctx, hostmirror, abi, cbox_oracle, monkeypatch, form, knobs):
    """(2) the Cornell box with a mask of 1 on every entry runs the new family (the probe answers, and it answers only where
    has_mask is set: the field the plan reads, test_plan_with_a_mask) and makes the ORACLE's film and samples of the box without
    masks: both RNG modes, with and without hide_emitters, tree in LDS and in HBM, fused kernels on and off"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    flat = with_masks(abi, hostmirror.cbox_scene(32, 32), np.ones((2, 2), F) if form == "image" else None)
    g, g0 = abi.Scene(gpu_ctx, flat), abi.Scene(gpu_ctx, hostmirror.cbox_scene(32, 32))
    try:
        one = np.ones((1, 3), F)
        a_pdf, _ = g.mask_eval(0, one[:, :2] * F(0.3), one * F(0.577), one * F(0.577), np.full((1, 4), 550, F))
        assert a_pdf[0, 0] == 1.0
        with pytest.raises(abi.MskError):
            g0.mask_eval(0, one[:, :2], one, one, np.full((1, 4), 550, F))
        for rng, hide in PARITY_PARAMS:
            film, st = g.render(parity_prm(abi, rng, hide))
            ref, n = cbox_oracle[(rng, hide)]
            assert st.samples == n == 32 * 32 * 4
            assert np.array_equal(bits(film), bits(ref)), (form, knobs, rng, hide, float(np.abs(film - ref).max()))
            assert film[..., :3].max() > 0
            if rng == "counter" and not knobs:
                _, st0 = g0.render(parity_prm(abi, rng, hide))       # (16 B more per segment in the general variant than in the diffuse one the plain box runs)
                assert (st.segments, st.shadow_rays) == (st0.segments, st0.shadow_rays) and st.bytes_shade > st0.bytes_shade
            if rng == "counter" and knobs == {"MSK_FUSED": "1"}:
                assert st.launches_wavefront > 0 and st.launches_shade == 0
        xyz, pos = g.sample_pixels(parity_prm(abi, "counter", 0), some_pixels(32, 32))
        assert np.array_equal(bits(xyz), bits(cbox_oracle["samples"][0])) and np.array_equal(bits(pos), bits(cbox_oracle["samples"][1]))
    finally:
        g.close(); g0.close()


@pytest.mark.gpu
def test_opacity_one_on_the_mixed_scene(gpu_ctx, hostmirror, abi):
    """(2) the mixed-material scene of test_direct_integrator.py (bitmap floor, twosided rough conductor, rough dielectric, glass)
    with a mask of 1 on every entry against the same scene without masks, which the parent's family renders: film and samples"""
    import test_direct_integrator as DI
    g0 = abi.Scene(gpu_ctx, hostmirror.flatten(DI.mixed_meshes(hostmirror), DI.FW, DI.FH))
    g = abi.Scene(gpu_ctx, with_masks(abi, hostmirror.flatten(DI.mixed_meshes(hostmirror), DI.FW, DI.FH), np.ones((2, 2), F)))
    try:
        for prm in (abi.render_params(spp=6, seed=11), EV.pcg(abi, spp=3, seed=11), abi.render_params(spp=6, seed=11, hide_emitters=1, max_depth=4)):
            film, st = g.render(prm)
            ref, st0 = g0.render(prm)
            assert np.array_equal(bits(film), bits(ref)), (prm.rng_mode, float(np.abs(film - ref).max()))
            assert st.samples == st0.samples and film[..., :3].max() > 0
        xyz, pos = g.sample_pixels(abi.render_params(spp=6, seed=11), DI.all_pixels())
        want, wpos = g0.sample_pixels(abi.render_params(spp=6, seed=11), DI.all_pixels())
        assert np.array_equal(bits(xyz), bits(want)) and np.array_equal(bits(pos), bits(wpos))
    finally:
        g.close(); g0.close()


# ===================================================================================================== GPU 3: closed forms
def sampled_mean(g, abi, what, expected, pixels=None, **params):
    """test_envmap.sampled_mean's procedure with this test's render parameters: spp doubles from 4096 until the standard error (from
    the per-sample values) is at most 0.5 % of the expectation, four doublings at the most"""
    spp = 4096
    for _ in range(5):
        xyz, _ = g.sample_pixels(abi.render_params(spp=spp, seed=7, **params), EV.crop_pixels() if pixels is None else pixels)
        v = xyz.reshape(-1, 3).astype(np.float64)
        mean, se = v.mean(0), v.std(0, ddof=1) / np.sqrt(len(v))
        print("MASK %s %s spp %d: expected %s mean %s se/|E| %s dev/|E| %s" % (what, params, spp, expected, mean, se / expected, (mean - expected) / expected))
        if np.all(se <= 5e-3 * expected):
            return mean, se
        spp *= 2
    raise AssertionError("the standard error stays above 0.5 %% of the expectation: %s" % (se / expected,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_rendered_radiance_meets_the_closed_form(gpu_ctx, hostmirror, abi, name):
    """(3 a, b, d, e) counter RNG through msk_gpu_sample_pixels: |mean - E| <= 6 standard errors + 1e-3 E per channel.
    (a) a rho L + (1 - a) L: at a = 0.25 the reference's a^2 would miss by 19 % of rho L.  (b) (1 - a) rho / pi Le G at
    max_depth = 3, and exactly zero at max_depth = 2.  (d) the floor beside an a = 0 canopy receives the sky through it, with and
    without hide_emitters: rho L.  (e) a one-sided diffuse X seen from behind at a = 0.5: (1 - a) L."""
    flat, expected, _, params = closed_form_case(hostmirror, name)
    g = abi.Scene(gpu_ctx, flat)
    try:
        mean, se = sampled_mean(g, abi, name, expected, **params)
        if name == "b_light_through_a_cutout":
            xyz, _ = g.sample_pixels(abi.render_params(spp=256, seed=7, max_depth=2), EV.crop_pixels())
            assert not xyz.any()                                         # the next-event sample is blocked and the path ends on the screen
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


def cutout_quad_flat(hm, opacity, far=False, extra=()):
    """the plane of (a) with texcoords (uv = (0.5, 0.5) at the origin, where the crop looks); far: moved out of every ray's way"""
    m = DM.plane(hm, masked({"type": "diffuse", "twosided": True}, opacity))
    m.texcoords = UV_QUAD
    if far:
        m.faces = [tuple((x, y + 500.0, z) for x, y, z in m.faces[0])]
        m.faces = [tuple(reversed(m.faces[0]))]
    return hm.flatten([m] + list(extra), W48, W48, camera=CAM, env=SKY)


def centre_pixels():
    """8 x 8 pixels around the film's centre: they see the plane around the origin, where the four quadrants of its uv square meet"""
    return np.array([(x, y) for y in range(20, 28) for x in range(20, 28)], np.int32)


def quadrant_pixels(hm, flat):
    """the centre pixels whose four corners see the plane inside one quadrant of its uv square -> {(x > 0, z > 0): pixels}"""
    out = {}
    for x, y in centre_pixels():
        yy, xx = np.meshgrid([y, y + 1.0], [x, x + 1.0], indexing="ij")
        o, d = R.camera_ray(flat.desc, xx, yy)
        p = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
        q = {(bool(px > 0), bool(pz > 0)) for px, pz in zip(p[..., 0].ravel(), p[..., 2].ravel())}
        if len(q) == 1 and np.all(np.abs(p[..., [0, 2]]) > 1e-3):
            out.setdefault(q.pop(), []).append((x, y))
    return {k: np.array(v, np.int32) for k, v in out.items()}


@pytest.mark.gpu
def test_image_cutout(gpu_ctx, hostmirror, abi):
    """(3 c) the 2 x 2 nearest image {1, 0; 0, 1}: pixels inside a quadrant give rho L or exactly the sky's value — the samples of the
    same pixels with the quad out of the way, bit for bit (the null path through a = 0 is deterministic)"""
    flat = cutout_quad_flat(hostmirror, image(CUTOUT, "nearest"))
    quads = quadrant_pixels(hostmirror, flat)
    assert len(quads) == 4 and all(len(v) >= 4 for v in quads.values()), {k: len(v) for k, v in quads.items()}
    g, g_sky = abi.Scene(gpu_ctx, flat), abi.Scene(gpu_ctx, cutout_quad_flat(hostmirror, 1.0, far=True))
    try:
        prm = abi.render_params(spp=64, seed=7)
        kinds = {}
        for key, px in quads.items():
            xyz, _ = g.sample_pixels(prm, px)
            sky, _ = g_sky.sample_pixels(prm, px)
            kinds[key] = bool(np.array_equal(bits(xyz), bits(sky)))
            assert sky.min() > 0
            if not kinds[key]:
                mean, se = sampled_mean(g, abi, "c opaque quadrant %s" % (key,), mixed_xyz(flat.desc, 0, 0, 1.0, 0.0), pixels=px, max_depth=2)
                e = mixed_xyz(flat.desc, 0, 0, 1.0, 0.0)
                assert np.all(np.abs(mean - e) <= 6 * se + 1e-3 * e), (key, (mean - e) / e)
        # the image's diagonal is opaque, the other two quadrants are holes
        assert sorted(kinds.values()) == [False, False, True, True], kinds
        assert kinds[(True, True)] == kinds[(False, False)] and kinds[(True, False)] == kinds[(False, True)]
    finally:
        g.close(); g_sky.close()


BEHIND = [(-1.0, -1.0, -1.67), (1.0, -1.0, -1.67), (1.0, -1.0, -3.67), (-1.0, -1.0, -3.67)]       # faces up, where the crop's rays go on to


@pytest.mark.gpu
@pytest.mark.parametrize("with_lamp", [False, True], ids=["sky", "area_light"])
def test_scattered_under_hide_emitters(gpu_ctx, hostmirror, abi, with_lamp):
    """(3 d) through an a = 0 quad: under hide_emitters the sky is exactly 0, and so is an area light behind the quad (departure 8;
    max_depth = 2 ends the path on the light, whose surface would go on to reflect the sky); without hide_emitters the same pixels
    give L: the samples of the scene with the quad out of the way (where the emitter is seen at depth 1), bit for bit"""
    extra = [hostmirror.MeshSpec("lamp", [tuple(BEHIND)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))] if with_lamp else []
    g = abi.Scene(gpu_ctx, cutout_quad_flat(hostmirror, 0.0, extra=extra))
    g_open = abi.Scene(gpu_ctx, cutout_quad_flat(hostmirror, 1.0, far=True, extra=extra))
    try:
        hidden, _ = g.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=2, hide_emitters=1), EV.crop_pixels())
        shown, _ = g.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=2), EV.crop_pixels())
        direct, _ = g_open.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=1), EV.crop_pixels())
        assert not hidden.any(), float(hidden.max())
        assert direct.min() > 0 and np.array_equal(bits(shown), bits(direct))
        rows = lambda f: f[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, :3]
        assert not rows(g.render(EV.pcg(abi, spp=4, seed=7, max_depth=2, hide_emitters=1))[0]).any()
        assert rows(g.render(EV.pcg(abi, spp=4, seed=7, max_depth=2))[0]).min() > 0
    finally:
        g.close(); g_open.close()


# ===================================================================================================== GPU 4: execution variants
def variant_meshes(hm, pads=()):
    """test_envmap's box (open Cornell box, area light, bitmap floor, glass ball) with masks: an image cutout on the tall box, a
    half-open mirror for the short one, a half-open glass ball; a point light and a `constant` sky beside the area light"""
    meshes = EV.variant_meshes(hm, pads)
    by = {m.name: m for m in meshes}
    big, small = by["cbox_largebox"], by["cbox_smallbox"]
    big.bsdf = masked({"type": "diffuse", "twosided": True}, image(np.random.RandomState(4).randint(0, 2, (4, 4)).astype(F), "bilinear", scale=(3, 2)))
    big.texcoords = [((0, 0), (1, 0), (1, 1), (0, 1)) for _ in big.faces]
    small.bsdf = masked(dict(DM.GOLD_RGB, twosided=True), 0.5)
    by["glass"].bsdf = masked({"type": "dielectric"}, 0.75)
    return meshes


def variant_flat(hm, which, crop=None):
    kw = dict(env=SKY, points=[DM.BOX_POINT], crop=crop)
    if which == "lds":
        return hm.flatten(variant_meshes(hm), 48, 48, **kw)
    filler = hm.blob_mesh("filler", (150, 420, 400), 60, 16, 16, hm.WHITE, seed=9)
    base = hm.flatten(variant_meshes(hm, [filler]), 48, 48, **kw)
    pads = T.faceless_pads(hm, T.SMALL_TABLES_F4 + 1 - T.table_plan(base)["small_f4"])
    return hm.flatten(variant_meshes(hm, [filler] + pads), 48, 48, **kw)


@pytest.fixture(scope="module")
def variant_reference(gpu_ctx, hostmirror, abi):
    """the default variant's samples and films of the two scenes (no knob set): computed once, never changed"""
    saved = {k: os.environ.pop(k) for k in DM.KNOBS if k in os.environ}
    out = {}
    try:
        for which in ("lds", "hbm"):
            flat = variant_flat(hostmirror, which)
            g = abi.Scene(gpu_ctx, flat)
            xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
            film, st = g.render(abi.render_params(spp=8, seed=5))
            serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
            g.close()
            for a in (xyz, pos, film, serial):
                a.setflags(write=False)
            assert np.isfinite(film).all() and film[..., :3].max() > 0
            out[which] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, samples=st.samples)
    finally:
        os.environ.update(saved)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which,env,expect", [("lds", e, x) for e, x in DM.LDS_VARIANTS] + [("hbm", e, x) for e, x in DM.HBM_VARIANTS],
                         ids=lambda v: EV.variant_id(v) if isinstance(v, dict) else str(v).replace(" ", "_"))
def test_every_execution_variant(gpu_ctx, abi, variant_reference, monkeypatch, which, env, expect):
    """(4) samples, film and serial film byte-equal to the default variant's, over the variants of the delta tests"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = variant_reference[which]
    g = abi.Scene(gpu_ctx, want["flat"])
    gx, gp = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
    film, st = g.render(abi.render_params(spp=8, seed=5))
    serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
    g.close()
    got = "trace %d shade %d wavefront %d" % (st.launches_trace, st.launches_shade, st.launches_wavefront)
    print("MASK variant %s %s: %s" % (which, EV.variant_id(env), got))
    assert np.array_equal(bits(gp), bits(want["pos"])) and np.array_equal(bits(gx), bits(want["xyz"])), env
    assert np.array_equal(bits(film), bits(want["film"])), (env, float(np.abs(film - want["film"]).max()))
    assert np.array_equal(bits(serial), bits(want["serial"])), env
    assert st.samples == want["samples"]
    if expect == EV.SPLIT:
        assert st.launches_wavefront == 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == EV.FUSED_PART:
        assert st.launches_wavefront > 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == EV.FUSED_ALL:
        assert st.launches_wavefront > 0 and st.launches_shade == 0 and st.launches_trace == 0, got
    else:
        assert st.launches_shade > 0 and st.launches_trace > 0, got


@pytest.mark.gpu
def test_shards_and_crop(gpu_ctx, hostmirror, abi, variant_reference, monkeypatch):
    """(4) Sample shards: the films of shards (0, 2) and (1, 2) sum to the whole film (another order of summation: not bits), and
    each shard's film is the same bits with the tree in HBM.  msk_gpu_sample_pixels IGNORES the shard selectors (include/msk_gpu.h:
    only msk_gpu_sample_pixels_direct honours them, and `direct` refuses a mask scene), so a shard's own samples cannot be read
    back through it: what is held is that a call with shard selectors returns the whole call's samples and positions, bit for
    bit.  MSK_RNG_PCG_BLOCK refuses sample shards.  A crop window holds the whole film's pixels bit for bit; its serial film has
    no counterpart in the whole film (one PCG32 stream per block, and the window has blocks of its own), so it is held to the same
    window rendered with the tree in HBM, bit for bit, as the window's counter-RNG film is."""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = variant_reference["lds"]
    shard = lambda r: abi.render_params(spp=8, seed=5, sample_first=r, sample_stride=2)
    g = abi.Scene(gpu_ctx, want["flat"])
    half = [g.render(shard(r)) for r in (0, 1)]
    xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5, sample_first=1, sample_stride=2), EV.crop_pixels())
    with pytest.raises(abi.MskError) as e:
        g.render(EV.pcg(abi, spp=2, seed=5, sample_first=1, sample_stride=2))
    assert e.value.code == abi.MSK_ERR_UNSUPPORTED
    g.close()
    assert half[0][1].samples == half[1][1].samples == 48 * 48 * 4
    assert np.allclose(half[0][0] + half[1][0], want["film"], rtol=2e-6, atol=1e-6)       # (film sums in another order: not bits)
    assert not np.array_equal(bits(half[0][0]), bits(half[1][0]))
    assert np.array_equal(bits(xyz), bits(want["xyz"])) and np.array_equal(bits(pos), bits(want["pos"]))
    crop = (5, 3, 24, 18)
    g = abi.Scene(gpu_ctx, variant_flat(hostmirror, "lds", crop=crop))
    window, _ = g.render(abi.render_params(spp=8, seed=5))
    serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
    g.close()
    assert window.shape == (18, 24, 5) and window[..., :3].max() > 0
    assert np.array_equal(bits(window), bits(want["film"][3:21, 5:29]))
    assert serial.shape == (18, 24, 5) and np.isfinite(serial).all() and serial[..., :3].max() > 0
    monkeypatch.setenv("MSK_LDS_SCENE_KB", "0")
    g = abi.Scene(gpu_ctx, want["flat"])
    half_hbm = [g.render(shard(r))[0] for r in (0, 1)]
    g.close()
    g = abi.Scene(gpu_ctx, variant_flat(hostmirror, "lds", crop=crop))
    window_hbm, _ = g.render(abi.render_params(spp=8, seed=5))
    serial_hbm, _ = g.render(EV.pcg(abi, spp=2, seed=5))
    g.close()
    for r in (0, 1):
        assert np.array_equal(bits(half_hbm[r]), bits(half[r][0])), r
    assert np.array_equal(bits(window_hbm), bits(window)) and np.array_equal(bits(serial_hbm), bits(serial))


@pytest.mark.gpu
def test_aov_sees_a_masked_surface_as_a_surface(gpu_ctx, hostmirror, abi):
    """an "aov" render of an a = 0 quad: the primary-hit channels (depth, position, uv, both normals) are those of the same quad
    without a mask, bit for bit; the nested path integrator's RGB goes through the mask kernels with the record groups and shows
    the sky through the quad"""
    plain = DM.plane(hostmirror, {"type": "diffuse", "twosided": True})
    plain.texcoords = UV_QUAD
    g0 = abi.Scene(gpu_ctx, hostmirror.flatten([plain], W48, W48, camera=CAM, env=SKY))
    g = abi.Scene(gpu_ctx, cutout_quad_flat(hostmirror, 0.0))
    try:
        prm = abi.render_params(spp=4, seed=3, max_depth=3)
        types = [abi.MSK_AOV_DEPTH, abi.MSK_AOV_POSITION, abi.MSK_AOV_UV, abi.MSK_AOV_GEO_NORMAL, abi.MSK_AOV_SH_NORMAL]
        film, st = g.render_aov(prm, types)
        ref, st0 = g0.render_aov(prm, types)
        assert film.shape == ref.shape == (W48, W48, 5 + 12) and st.samples == st0.samples
        assert np.array_equal(bits(film[..., 3:]), bits(ref[..., 3:])) and np.abs(ref[..., 5:]).max() > 0
        assert not film[..., :3].any() and not ref[..., :3].any()                  # (no radiance without the nested path's record)
        rgba, _ = g.render_aov(prm, types + [abi.MSK_AOV_PATH_RGBA])
        ref_rgba, _ = g0.render_aov(prm, types + [abi.MSK_AOV_PATH_RGBA])
        assert np.array_equal(bits(rgba[..., 3:17]), bits(ref_rgba[..., 3:17])) and np.isfinite(rgba).all()
        # X, Y, Z (weighted sums with the same weights): rho <= 0.6 at every wavelength, so the sky seen through the quad is at least
        # 1 / 0.6 times the lit quad in each; the nested R, G, B record is filled too
        rows = lambda f, c: f[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, c]
        assert np.all(rows(rgba, slice(0, 3)) > 1.3 * rows(ref_rgba, slice(0, 3))) and rows(ref_rgba, slice(0, 3)).min() > 0
        assert rows(rgba, slice(17, 20)).min() > 0 and rows(ref_rgba, slice(17, 20)).min() > 0
    finally:
        g.close(); g0.close()


# ===================================================================================================== GPU 5: refusals
@pytest.mark.gpu
def test_refusals(gpu_ctx, hostmirror, abi):
    """(5) `direct` on a mask scene: MSK_ERR_UNSUPPORTED by name; each bad descriptor: MSK_ERR_INVALID_ARG by name"""
    flat = quad_under_sky(hostmirror, 0.5)
    g = abi.Scene(gpu_ctx, flat)
    try:
        prm = abi.render_params(spp=2, seed=1)
        for call in (lambda: g.render_direct(prm, 1, 1), lambda: g.sample_pixels_direct(prm, EV.crop_pixels()[:2], 1, 1)):
            with pytest.raises(abi.MskError) as e:
                call()
            assert e.value.code == abi.MSK_ERR_UNSUPPORTED and "mask" in str(e.value) and "direct" in str(e.value)
        film, _ = g.render(prm)                                          # (`path` renders it)
        assert film[..., :3].max() > 0
    finally:
        g.close()
    vals = np.array([0.5, 1.0], F)

    def desc(**kw):
        k = abi.MaskDesc()
        k.bsdf, k.opacity, k.filter = 0, 0.5, 0
        k.to_uv[:] = [1, 0, 0, 0, 1, 0]
        for name, v in kw.items():
            setattr(k, name, v)
        return k
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    bad = np.array([0.5, 1.5], F)
    nan = np.array([np.nan, 0.5], F)
    cases = [([desc(bsdf=1)], "bsdf 1 out of range"), ([desc(), desc(opacity=0.25)], "already has a mask"), ([desc(opacity=1.5)], "not in [0, 1]"),
             ([desc(opacity=-0.5)], "not in [0, 1]"), ([desc(opacity=float("nan"))], "not in [0, 1]"), ([desc(filter=3)], "filter 3"), ([desc(filter=-1)], "filter -1"),
             ([desc(filter=2, width=0, height=2, values=ptr(vals))], "0 x 2"), ([desc(filter=1, width=2, height=0, values=ptr(vals))], "2 x 0"),
             ([desc(filter=1, width=2, height=1)], "values array is missing"), ([desc(filter=2, width=2, height=1, values=ptr(bad))], "value 1"),
             ([desc(filter=2, width=2, height=1, values=ptr(nan))], "value 0")]
    for masks, words in cases:
        with pytest.raises(abi.MskError) as e:
            abi.Scene(gpu_ctx, quad_under_sky(hostmirror, 0.5), masks=masks)
        assert e.value.code == abi.MSK_ERR_INVALID_ARG and words in str(e.value) and "mask" in str(e.value), (words, str(e.value))
    ok = abi.Scene(gpu_ctx, quad_under_sky(hostmirror, 0.5), masks=[desc(filter=2, width=2, height=1, values=ptr(vals))])
    ok.close()
