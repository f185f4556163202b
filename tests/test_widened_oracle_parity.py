"""The widened twin: `bitmap`, `envmap`, `point`, `conductor` and `mask` in the CPU oracle (oracle/oracle.cpp, D11-D18), and the
device held to it bit for bit.

CPU layer (the twin earns trust before the device is held to it):
  (a) the oracle's hooks against the Python fp32 restatements (bitmap_ref, envmap_ref, delta_ref, mask_ref) on the very inputs the
      GPU probe tests generate, as uint32, no exclusions;
  (b) the twin's renders against the float64 expectations the device already meets, by the same procedure and acceptance: spp
      doubling from 4096 until se <= 5e-3 E, then |mean - E| <= 6 se + 1e-3 E;
  (c) identities that need no tolerance;
  (d) the path tallies of every parity scene at the parameters used on the GPU — the variant scenes, every film of the
      all-features grid on its own, the `direct` anchors: each branch a scene is meant to exercise is reached at least 100 times in
      ONE counter-RNG render (the 2-spp MSK_RNG_PCG_BLOCK films of the grid: at least once; the test says why).
GPU layer: every comparison is array_equal on the uint32 view; no pixel or sample is left out.
  (e) the default configuration against the twin on the variant scenes of test_envmap / test_delta_light_mirror / test_mask_bsdf at
      the parameters of their `variant_reference` fixtures, which ties every execution variant of those files to the oracle;
  (f) one all-features scene over RNG x hide_emitters x depth limits, in both table placements, with a crop window and sample shards;
  (g) "aov" on the mask scene; (h) `direct` at (1, 1) against the twin at max_depth = 2.

Counters.  samples are equal.  shadow_rays: the device traces a shadow ray only for a next-event term that is not zero, the oracle
for every sample with a density; the oracle tallies the former too (`shadow_rays_nonzero`), and that is what the device's count
must equal.  segments: the oracle counts the ray of every BSDF sample that has a lobe.  The MSK_RNG_PCG_BLOCK kernels do the same:
equal counts.  The wavefront kernels count the ray of a path that is still alive after the bounce: a sample with a lobe that leaves a
zero throughput and has no shadow ray pending ends there without one (`segments_dropped`), and a failed sample with a shadow ray
pending keeps its slot for one more, zero, ray (`segments_extra`).  The oracle tallies both, and the device's count must equal
the oracle's minus the first plus the second, exactly."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bitmap_ref as BR
import delta_ref as D
import mask_ref as M
import oracle_binding
import test_bitmap_texture as BT
import test_delta_light_mirror as DM
import test_direct_integrator as DI
import test_envmap as EV
import test_mask_bsdf as MB

F = np.float32
KNOBS = DM.KNOBS


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(what, got, want, *context):
    bad = (bits(got) != bits(want)).reshape(len(got), -1).any(-1)
    assert not bad.any(), (what, int(bad.sum()), np.asarray(got)[bad][:3], np.asarray(want)[bad][:3]) + context


# ===================================================================================================== (a) hooks against the restatements
@pytest.mark.parametrize("name", BT.PROBE_IMAGES)
def test_a_texture_hook_equals_bitmap_ref(hostmirror, oracle, name):
    """msk_oracle_eval_texture against bitmap_ref.lookup on test_bitmap_texture's probe scene and points: both filters, three to_uv"""
    flat, images, index = BT.probe_flat(hostmirror)
    o = oracle.scene(flat)
    h, w = images[name].shape[:2]
    rng = np.random.RandomState(5)
    uv = BT.probe_points(rng, w, h)
    wl = rng.uniform(360, 830, (len(uv), 4)).astype(F)
    for filt in ("bilinear", "nearest"):
        for uvn in BT.TO_UVS:
            k = index[(name, filt, uvn)]
            t = flat.desc.textures[k - 1]
            coeffs = flat.texels[t.first_texel:t.first_texel + w * h].reshape(h, w, 3)
            want = BR.lookup(BR.oracle_texels(oracle, coeffs), w, h, filt, list(t.to_uv), uv, wl)
            assert_bits("texture", o.eval_texture(k, uv, wl), want, name, filt, uvn)
    # the checkerboards of the same scene through the same hook: color0 / color1 as msk_oracle_checkerboard picks them
    for uvn in BT.TO_UVS:
        k = index[("checker", uvn)]
        t = flat.desc.textures[k - 1]
        got = o.eval_texture(k, uv[:256], wl[:256])
        want = np.stack([oracle.srgb_model_eval((t.color0 if oracle.checkerboard(t, float(a), float(b)) == 0 else t.color1)[:], l) for (a, b), l in zip(uv[:256], wl[:256])])
        assert_bits("checkerboard", got, want, uvn)
    o.close()


@pytest.mark.parametrize("rot", sorted(EV.ROTATIONS))
@pytest.mark.parametrize("name", sorted(EV.images()))
def test_a_envmap_hooks_equal_envmap_ref(hostmirror, oracle, name, rot):
    """msk_oracle_env_sample / _env_eval against envmap_ref.Env32 on test_envmap's probe inputs; the "excluded case" of envmap_ref
    concerns pdf(direction(sample)) round trips, not two implementations of the same operations: nothing is left out"""
    env = EV.env_spec(EV.images()[name], EV.ROTATIONS[rot], scale=1.5)
    e32, _, _, _ = EV.restatements(hostmirror, oracle, env)
    flat = hostmirror.flatten(EV.plane_meshes(hostmirror), 16, 16, camera=EV.PLANE_CAMERA, env=env)
    u, d, wl = EV.probe_inputs(e32, np.random.RandomState(17))
    o = oracle.scene(flat)
    od, ouv, opdf = o.env_sample(u)
    orad, op = o.env_eval(d, wl)
    o.close()
    rd, ruv, rpdf, _ = e32.sample(u)
    rrad, rp, _ = e32.eval_dir(d, wl)
    for what, a, b in (("uv", ouv, ruv), ("direction", od, rd), ("sampled pdf", opdf, rpdf), ("radiance", orad, rrad), ("pdf", op, rp)):
        assert_bits(what, a, b, name, rot)


def test_a_point_and_conductor_hooks_equal_delta_ref(hostmirror, oracle):
    """msk_oracle_point_sample / _conductor_sample against delta_ref on test_delta_light_mirror's probe inputs"""
    pos, p, wl, cos = DM.probe_inputs()
    flat = DM.probe_flat(hostmirror, pos)
    d = flat.desc
    _, d65 = hostmirror.cie_tables()
    o = oracle.scene(flat)
    for e, position in ((1, pos), (2, np.array(DM.PROBE_POINT_2, F))):
        od, ov = o.point_sample(e, p, wl)
        ed = d.emitters[e]
        inten = D.intensity32(oracle, ed.radiance[:], (d65 * F(ed.d65_scale)).astype(F), wl)
        rd, rv = D.point_sample32(position, p, inten)
        assert_bits("d, dist", od, rd, e)
        assert_bits("value", ov, rv, e)
    assert not o.point_sample(1, p[-1:], wl[-1:])[0].any() and not o.point_sample(1, p[-1:], wl[-1:])[1].any()      # the position itself: zeros
    for b in range(3):
        bd = d.bsdfs[b]
        rv = D.conductor_sample32(cos, D.spectrum32(oracle, bd.eta, wl), D.spectrum32(oracle, bd.k, wl), D.spectrum32(oracle, bd.specular_reflectance, wl))
        assert_bits("conductor", o.conductor_sample(b, cos, wl), rv, b)
    assert np.all(o.conductor_sample(0, cos, wl)[cos > 0] == 1.0)             # the defaults: a perfect mirror
    o.close()


@pytest.mark.parametrize("kind", sorted(MB.OPACITIES))
def test_a_mask_hooks_equal_mask_ref(hostmirror, oracle, abi, kind):
    """msk_oracle_mask_sample / _mask_eval against mask_ref over the nested restatements, on test_mask_bsdf's probe scene and inputs:
    10 entries x 64 inputs per kind of opacity"""
    entries = MB.probe_entries()
    meshes = [MB.quad(hostmirror, name, MB.masked(spec, MB.OPACITIES[kind]), 0.1 * i, uv=True) for i, (name, spec) in enumerate(entries)]
    meshes.append(hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20)))
    flat = hostmirror.flatten(meshes, 16, 16, camera=MB.CAM, coeff_lookup=None)
    o = oracle.scene(flat)
    rng = np.random.RandomState(sorted(MB.OPACITIES).index(kind))
    for b, (name, _) in enumerate(entries):
        uv, wi, wo_in, su, wl = MB.probe_inputs(rng, 64)
        k = flat.masks[b]
        mask = {"filter": k.filter, "opacity": k.opacity, "to_uv": list(k.to_uv)}
        if k.filter:
            mask["values"] = np.ctypeslib.as_array(k.values, (k.height, k.width))
        a = M.opacity32(mask, uv)
        x_sample, x_eval, x_delta = MB.nested_restatement(oracle, abi, flat, b, name, uv, wl)
        want = M.sample32(a, wi, su[:, 0], su[:, 1:], x_sample, x_delta)
        wo_pdf, value, flags = o.mask_sample(b, uv, wi, su, wl)
        assert np.array_equal(flags[:, 2] != 0, want["null"]) and np.array_equal(flags[:, 1] != 0, want["delta"]), (kind, name)
        assert np.array_equal(flags[:, 3] != 0, want["ok"]), (kind, name)
        for what, got, ref in (("wo", wo_pdf[:, :3], want["wo"]), ("pdf", wo_pdf[:, 3], want["pdf"]), ("value", value, want["value"]), ("eta", flags[:, 0], want["eta"])):
            assert_bits(what, got, ref, kind, name)
        a_pdf, ev = o.mask_eval(b, uv, wi, wo_in, wl)
        rv, rp = M.eval32(a, *x_eval(wi, wo_in))
        assert_bits("opacity", a_pdf[:, 0], a, kind, name)
        assert_bits("eval", ev, rv, kind, name)
        assert_bits("eval pdf", a_pdf[:, 1], rp, kind, name)
    o.close()


# ===================================================================================================== (b) closed forms on the twin
def sample_pixels_threaded(o, prm, pixels, threads=8):
    """msk_oracle_sample_pixels is single-threaded and pixels are independent: the listed pixels in `threads` parts side by side"""
    pixels = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
    parts = np.array_split(np.arange(len(pixels)), threads)
    with ThreadPoolExecutor(threads) as pool:
        out = list(pool.map(lambda idx: o.sample_pixels(prm, pixels[idx]), parts))
    return np.concatenate([x for x, _ in out]), np.concatenate([p for _, p in out])


def twin_mean(o, abi, what, expected, pixels=None, **params):
    """the procedure of test_envmap.sampled_mean / test_mask_bsdf.sampled_mean on the twin: spp doubles from 4096 until the standard
    error is at most 0.5 % of the expectation, four doublings at the most"""
    spp = 4096
    for _ in range(5):
        xyz, _ = sample_pixels_threaded(o, abi.render_params(spp=spp, seed=7, **params), EV.crop_pixels() if pixels is None else pixels)
        v = xyz.reshape(-1, 3).astype(np.float64)
        mean, se = v.mean(0), v.std(0, ddof=1) / np.sqrt(len(v))
        print("TWIN %s %s spp %d: expected %s mean %s se/|E| %s dev/|E| %s" % (what, params, spp, expected, mean, se / expected, (mean - expected) / expected))
        if np.all(se <= 5e-3 * expected):
            return mean, se
        spp *= 2
    raise AssertionError("the standard error stays above 0.5 %% of the expectation: %s" % (se / expected,))


def meets(mean, se, expected):
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


@pytest.mark.parametrize("name", MB.CASES)
def test_b_twin_meets_the_mask_closed_forms(hostmirror, oracle, abi, name):
    flat, expected, _, params = MB.closed_form_case(hostmirror, name)
    o = oracle.scene(flat)
    mean, se = twin_mean(o, abi, name, expected, **params)
    if name == "b_light_through_a_cutout":
        xyz, _ = o.sample_pixels(abi.render_params(spp=256, seed=7, max_depth=2), EV.crop_pixels())
        assert not xyz.any()                                             # the next-event sample is blocked and the path ends on the screen
    o.close()
    meets(mean, se, expected)


@pytest.mark.parametrize("name", DM.CASES)
def test_b_twin_meets_the_delta_closed_forms(hostmirror, oracle, abi, name):
    flat, expected, _ = DM.closed_form_case(hostmirror, name)
    o = oracle.scene(flat)
    mean, se = twin_mean(o, abi, name, expected, max_depth=3 if name == "e_mirror_then_lamp" else 2)
    if name == "e_mirror_then_lamp":
        xyz, _ = o.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=2), EV.crop_pixels())
        assert not xyz.any()                                             # at max_depth = 2 the path ends on the wall, before its next-event sample
    o.close()
    meets(mean, se, expected)


@pytest.mark.parametrize("floor", sorted(EV.FLOORS))
def test_b_twin_meets_the_envmap_plane_quadrature(hostmirror, oracle, abi, floor):
    flat, env = EV.plane_scene(hostmirror, floor)
    _, e64, _, _ = EV.restatements(hostmirror, None, env)
    expected = EV.expected_plane_xyz(flat, e64, floor)
    o = oracle.scene(flat)
    mean, se = twin_mean(o, abi, "envmap plane " + floor, expected, max_depth=2)
    o.close()
    meets(mean, se, expected)


@pytest.mark.parametrize("first", [False, True], ids=["envmap_last", "envmap_first"])
def test_b_twin_meets_envmap_plus_one_area_light(hostmirror, oracle, abi, first):
    import radiometry_ref as R
    lamp = DM.LAMP
    img = EV.lit_image()
    img[0:2] = 0
    env = EV.env_spec(img, EV.IDENTITY, scale=3.0)
    meshes = EV.plane_meshes(hostmirror) + [hostmirror.MeshSpec("lamp", [tuple(lamp)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))]
    flat = hostmirror.flatten(meshes, EV.W48, EV.W48, camera=EV.PLANE_CAMERA, env=dict(env, first=first))
    d = flat.desc
    assert d.n_emitters == 2 and d.emitters[0 if first else 1].type == abi.MSK_EMITTER_ENVMAP
    _, e64, _, _ = EV.restatements(hostmirror, None, env)
    ea = d.emitters[1 if first else 0]
    le = R.srgb_d65(ea.radiance[:], np.array(d.d65[:95], np.float64), ea.d65_scale)
    expected = EV.expected_plane_xyz(flat, e64, "diffuse", area=(np.array(lamp, np.float64), le))
    o = oracle.scene(flat)
    mean, se = twin_mean(o, abi, "sky + lamp", expected, max_depth=2)
    o.close()
    meets(mean, se, expected)


# ===================================================================================================== (c) identities on the twin
def twin_films(oracle, abi, flat, prms):
    o = oracle.scene(flat)
    out = [o.render(p, threads=8)[0] for p in prms]
    o.close()
    return out


def identity_params(abi):
    return [MB.parity_prm(abi, rng, hide) for rng, hide in MB.PARITY_PARAMS]


@pytest.mark.parametrize("form", ["constant", "image"])
def test_c_opacity_one_is_the_unmasked_film(hostmirror, oracle, abi, form):
    """a = 1 on every entry (a constant, or a bilinear image of ones): u.x / 1 and 1 * pdf are exact, the film is the unmasked one"""
    prms = identity_params(abi)
    values = np.ones((3, 2), F) if form == "image" else None
    for scene in (lambda: hostmirror.cbox_scene(32, 32), lambda: hostmirror.flatten(DI.mixed_meshes(hostmirror), 32, 32)):
        plain = twin_films(oracle, abi, scene(), prms)
        masked = twin_films(oracle, abi, MB.with_masks(abi, scene(), values), prms)
        for a, b in zip(plain, masked):
            assert np.array_equal(bits(a), bits(b)) and a[..., :3].max() > 0


@pytest.mark.parametrize("filt", ["bilinear", "nearest"])
def test_c_uniform_bitmap_is_the_constant_reflectance(hostmirror, oracle, abi, filt):
    img = np.broadcast_to(np.asarray(BT.C0, F), (5, 3, 3))
    plain = hostmirror.cbox_meshes()
    floor = next(m for m in plain if m.name == "cbox_floor")
    floor.reflectance = BT.C0
    floor.texcoords = [((0, 0), (1, 0), (1, 1), (0, 1)) for _ in floor.faces]
    prms = identity_params(abi)
    a = twin_films(oracle, abi, hostmirror.flatten(plain, 32, 32), prms)
    b = twin_films(oracle, abi, BT.checker_floor_scene(hostmirror, 32, 32, BT.bitmap(img, filt, scale=(3, 2))), prms)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)) and x[..., :3].max() > 0


@pytest.mark.parametrize("hide", [0, 1])
def test_c_uniform_envmap_is_the_constant_sky(hostmirror, oracle, abi, hide):
    """texels (0.5, 0.4, 0.3): w = 2 max = 1, a power of two.  At max_depth = 1 (what is seen directly) on the open Cornell box; and
    at every depth where light arrives by delta lobes alone (a mirror plane under the sky: no next-event sample, weight 1): the two
    emitters sample differently, so a next-event sample would part the films."""
    img = np.broadcast_to(np.array([0.5, 0.4, 0.3], F), (3, 4, 3))
    meshes = lambda: [m for m in hostmirror.cbox_meshes() if m.name not in ("cbox_ceiling", "cbox_back")]
    prms = [abi.render_params(spp=4, seed=3, max_depth=1, hide_emitters=hide), EV.pcg(abi, spp=2, seed=3, max_depth=1, hide_emitters=hide)]
    a = twin_films(oracle, abi, hostmirror.flatten(meshes(), 48, 48, env=EV.env_spec(img, EV.skew_rotation())), prms)
    b = twin_films(oracle, abi, hostmirror.flatten(meshes(), 48, 48, env={"radiance": (0.5, 0.4, 0.3)}), prms)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)) and (x[..., :3].max() > 0 or hide)
    prms = [abi.render_params(spp=4, seed=3, hide_emitters=hide), EV.pcg(abi, spp=2, seed=3, hide_emitters=hide)]
    mirror = lambda env: hostmirror.flatten([DM.plane(hostmirror, DM.GOLD_RGB)], 48, 48, camera=DM.CAM, env=env)
    a = twin_films(oracle, abi, mirror(EV.env_spec(img, EV.skew_rotation())), prms)
    b = twin_films(oracle, abi, mirror({"radiance": (0.5, 0.4, 0.3)}), prms)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)) and x[..., :3].max() > 0


def test_c_black_from_behind_and_from_below(hostmirror, oracle, abi):
    """test_delta_light_mirror's (7 f) on the twin: a one-sided conductor seen from behind, under a sky, and a point light below a
    one-sided diffuse plane are exactly 0 in both RNG modes; the same conductor from the front is not"""
    behind = hostmirror.flatten([DM.plane(hostmirror, DM.GOLD, flip=True)], EV.W48, EV.W48, camera=DM.CAM, env=DM.SKY)
    below = hostmirror.flatten([DM.plane(hostmirror)], EV.W48, EV.W48, camera=DM.CAM, points=[DM.point_spec((0.7, -2.5, 0.4))])
    front = hostmirror.flatten([DM.plane(hostmirror, DM.GOLD)], EV.W48, EV.W48, camera=DM.CAM, env=DM.SKY)
    for flat, black in ((behind, True), (below, True), (front, False)):
        o = oracle.scene(flat)
        xyz, _ = o.sample_pixels(abi.render_params(spp=64, seed=7), EV.crop_pixels())
        film, _ = o.render(EV.pcg(abi, spp=2, seed=7), threads=8)
        o.close()
        rows = film[EV.CROP[1]:EV.CROP[1] + 8, EV.CROP[0]:EV.CROP[0] + 8, :3]
        assert np.isfinite(xyz).all() and np.isfinite(film).all()
        assert (not xyz.any() and not rows.any()) if black else (xyz.min() > 0 and rows.min() > 0)


def test_c_an_unused_conductor_entry_changes_nothing(hostmirror, oracle, abi):
    """no sky: departure 5 has nothing to decide, and the entry is named by no mesh"""
    prms = identity_params(abi)
    for scene in DM.parity_scenes(hostmirror).values():
        a = twin_films(oracle, abi, scene(), prms)
        b = twin_films(oracle, abi, DM.with_trailing_conductor(hostmirror, abi, scene()), prms)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)) and x[..., :3].max() > 0


def test_c_the_oracle_refuses_what_the_library_refuses(hostmirror, oracle, abi):
    import ctypes as C
    flat = lambda: hostmirror.flatten(EV.plane_meshes(hostmirror), 16, 16, camera=EV.PLANE_CAMERA, env=EV.env_spec(EV.images()["3x5"]), points=[DM.point_spec()])
    oracle.scene(flat()).close()
    f = flat()
    f.envmap.to_world[0] = 2.0                                           # no rotation
    with pytest.raises(ValueError):
        oracle.scene(f)
    with pytest.raises(ValueError):                                      # a point emitter without its msk_point_desc
        oracle.scene(flat(), points=[])
    f = flat()
    with pytest.raises(ValueError):                                      # ... and with two
        oracle.scene(f, points=[f.points[0], f.points[0]])
    for bad in (abi.MaskDesc(0, 1.5, 0), abi.MaskDesc(0, -0.0 - 1e-3, 0), abi.MaskDesc(0, float("nan"), 0), abi.MaskDesc(7, 0.5, 0)):
        with pytest.raises(ValueError):
            oracle.scene(flat(), masks=[bad])
    vals = np.array([0.5, 1.25], F)
    img = abi.MaskDesc(0, 0.0, 2, (1, 0, 0, 0, 1, 0), 2, 1, vals.ctypes.data_as(C.POINTER(C.c_float)))
    with pytest.raises(ValueError):                                      # an image value outside [0, 1]
        oracle.scene(flat(), masks=[img])


# ===================================================================================================== the parity scenes
def all_features_meshes(hm):
    """The open Cornell box (no ceiling, no back wall: the environment is in view and lights the box) with: an area lamp in the
    open back that faces the camera; a bilinear bitmap floor under a skewed to_uv; the short box a bilinear image mask over a rough
    conductor; the tall box a rough dielectric; a glass ball under a 0.75 mask; a twosided mirror ball; two 0.5-masked one-sided
    diffuse screens in front of the box, one facing the camera — it covers the lamp as the camera sees it, so that half of those
    rays reach the lamp through a null lobe, unscattered: departure 8 — and one facing away: the one-sided X is met from both sides."""
    meshes = [m for m in DI.open_box(hm) if m.name != "cbox_luminaire"]
    meshes.insert(0, hm.MeshSpec("lamp", [((290, 345, 500), (290, 540, 500), (545, 540, 500), (545, 345, 500))], hm.LUMINAIRE, radiance=(40, 40, 40)))
    by = {m.name: m for m in meshes}
    floor = by["cbox_floor"]
    floor.bsdf = {"type": "diffuse", "texture": {"type": "bitmap", "pixels": np.random.RandomState(12).uniform(0.1, 0.9, (3, 5, 3)).astype(F), "matrix": BT.SKEW}}
    floor.texcoords = [((0, 0), (1, 0), (1, 1), (0, 1)) for _ in floor.faces]
    small, big = by["cbox_smallbox"], by["cbox_largebox"]
    small.bsdf = MB.masked({"type": "roughconductor", "alpha": 0.2, "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14)},
                           MB.image(np.random.RandomState(13).uniform(0, 1, (3, 4)).astype(F) ** 2, "bilinear", scale=(2, 3)))
    small.texcoords = [((0, 0), (1, 0), (1, 1), (0, 1)) for _ in small.faces]
    big.bsdf = {"type": "roughdielectric", "alpha": 0.15, "int_ior": 1.5, "ext_ior": 1.0}
    glass = hm.blob_mesh("glass", (400, 80, 120), 70, 5, 5, hm.WHITE, seed=2)
    glass.bsdf = MB.masked({"type": "dielectric"}, 0.75)
    mirror = hm.blob_mesh("mirror", (250, 640, 280), 90, 5, 5, hm.WHITE, seed=4)
    mirror.bsdf = dict(DM.GOLD_RGB, twosided=True)
    facing = hm.MeshSpec("screen_facing", [((280, 310, 30), (280, 450, 30), (460, 450, 30), (460, 310, 30))], MB.RHO, bsdf=MB.masked({"type": "diffuse"}, 0.5))
    away = hm.MeshSpec("screen_away", [((190, 20, 30), (190, 540, 30), (10, 540, 30), (10, 20, 30))], MB.RHO, bsdf=MB.masked({"type": "diffuse"}, 0.5))      # (the other winding)
    for wall in ("cbox_greenwall", "cbox_redwall"):      # the same 0.5 mask over the walls' one-sided diffuse: light leaves the box through them
        by[wall].bsdf = MB.masked({"type": "diffuse"}, 0.5)
    return meshes + [glass, mirror, facing, away]


ALL_SKIES = {"envmap": lambda: EV.env_spec(EV.lit_image(), EV.skew_rotation(), scale=40.0), "constant": lambda: {"radiance": (12.0, 15.0, 20.0)}}
ALL_POINT = DM.point_spec((300.0, 420.0, 150.0), (4e5, 3e5, 2e5))
ALL_DEPTHS = [dict(max_depth=-1, rr_depth=2), dict(max_depth=2), dict(max_depth=5, rr_depth=100)]


def all_features_flat(hm, sky, crop=None):
    return hm.flatten(all_features_meshes(hm), 32, 32, env=ALL_SKIES[sky](), points=[ALL_POINT], crop=crop)


def all_features_params(abi):
    """counter RNG x PCG x hide_emitters 0 / 1 x three depth limits, 8 spp (PCG: 2)"""
    out = []
    for rng in ("counter", "pcg"):
        for hide in (0, 1):
            for depth in ALL_DEPTHS:
                kw = dict(seed=5, hide_emitters=hide, **depth)
                out.append(abi.render_params(spp=8, **kw) if rng == "counter" else EV.pcg(abi, spp=2, **kw))
    return out


def variant_params(abi):
    """the parameters of the `variant_reference` fixtures: sample_pixels at spp 16, a film at spp 8, a MSK_RNG_PCG_BLOCK film at spp 2, seed 5"""
    return abi.render_params(spp=16, seed=5), abi.render_params(spp=8, seed=5), EV.pcg(abi, spp=2, seed=5)


VARIANT_SCENES = {"envmap": lambda hm, which: EV.variant_flat(hm, which), "box_none": lambda hm, which: DM.box_flat(hm, which, "none"),
                  "box_envmap": lambda hm, which: DM.box_flat(hm, which, "envmap"), "mask": lambda hm, which: MB.variant_flat(hm, which)}
VARIANT_IDS = [(name, which) for name in VARIANT_SCENES for which in ("lds", "hbm")]

_twin_cache = {}


def counted(oracle, fn):
    """fn() with the oracle's path tallies of exactly that call"""
    oracle.path_tallies()
    out = fn()
    return out, oracle.path_tallies()


def twin_of_variant(oracle, hm, abi, name, which):
    """the twin's samples, film, serial film, counters and tallies of a variant scene: computed once, never changed"""
    key = ("variant", name, which)
    if key not in _twin_cache:
        flat = VARIANT_SCENES[name](hm, which)
        o = oracle.scene(flat)
        p_xyz, p_film, p_serial = variant_params(abi)
        (xyz, pos), _ = counted(oracle, lambda: sample_pixels_threaded(o, p_xyz, EV.crop_pixels()))
        (film, st), tally = counted(oracle, lambda: o.render(p_film, threads=8))
        (serial, sst), stally = counted(oracle, lambda: o.render(p_serial, threads=8))
        o.close()
        for a in (xyz, pos, film, serial):
            a.setflags(write=False)
        _twin_cache[key] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, st=(st.samples, st.segments), tally=tally,
                                sst=(sst.samples, sst.segments), stally=stally)
    return _twin_cache[key]


def twin_of_all_features(oracle, hm, abi, sky):
    key = ("all", sky)
    if key not in _twin_cache:
        o = oracle.scene(all_features_flat(hm, sky))
        out = []
        for prm in all_features_params(abi):
            (film, st), tally = counted(oracle, lambda: o.render(prm, threads=8))
            film.setflags(write=False)
            out.append(dict(film=film, st=(st.samples, st.segments), tally=tally))
        o.close()
        _twin_cache[key] = out
    return _twin_cache[key]


# ===================================================================================================== (d) coverage
EVERY = set(oracle_binding.Oracle.PATH_TALLIES[:11])                    # the named path events (the last two entries are the counters' tallies)
# what each scene is meant to exercise (at least 100 times in its spp-8 film) and what it cannot produce at all (exactly 0); a tally in
# neither set may occur and is not required of that scene
POINT_T, NULL_T = {"point_unoccluded", "point_occluded"}, {"null_lobe", "emitter_after_null", "rr_after_null", "area_emitter_hidden"}
VARIANT_COVERAGE = {
    # image sky, area lamp, bitmap floor, glass ball; no point light, no mask, and no `constant` sky for departure 5
    "envmap": dict(meant={"envmap_miss_after_smooth", "emitter_after_delta", "texel_wrap", "envmap_pole_clamp"}, cannot=POINT_T | NULL_T | {"sky_own_density"}),
    # no sky at all: mirror, glass, point light, bitmap floor.  Without a sky a mirror or glass bounce reaches an emitter only by
    # finding the small lamp: a handful of times in this film; that tally is neither required nor impossible here
    "box_none": dict(meant={"point_unoccluded", "point_occluded", "texel_wrap"}, cannot=NULL_T | {"sky_own_density", "envmap_miss_after_smooth", "envmap_pole_clamp"}),
    "box_envmap": dict(meant={"point_unoccluded", "point_occluded", "emitter_after_delta", "envmap_miss_after_smooth", "texel_wrap", "envmap_pole_clamp"}, cannot=NULL_T | {"sky_own_density"}),
    # `constant` sky, point light, masks over diffuse (image), mirror and glass; hide_emitters is 0 in these parameters
    "mask": dict(meant={"null_lobe", "emitter_after_null", "emitter_after_delta", "sky_own_density", "point_unoccluded", "point_occluded", "texel_wrap"},
                 cannot={"envmap_miss_after_smooth", "envmap_pole_clamp", "area_emitter_hidden"}),
}


@pytest.mark.parametrize("name,which", VARIANT_IDS)
def test_d_variant_scenes_reach_their_branches(hostmirror, oracle, abi, name, which):
    t = twin_of_variant(oracle, hostmirror, abi, name, which)["tally"]
    cov = VARIANT_COVERAGE[name]
    print("TALLY %s %s: %s" % (name, which, t))
    for k in sorted(cov["meant"]):
        assert t[k] >= 100, (name, which, k, t)
    for k in sorted(cov["cannot"]):
        assert t[k] == 0, (name, which, k, t)
    assert cov["meant"] | cov["cannot"] <= EVERY


def all_features_coverage(abi, sky, prm):
    """(meant, cannot) of ONE film of the grid.  An image sky cannot produce a departure-5 hit, a `constant` sky neither an envmap miss
    nor a pole clamp; an area emitter is hidden only under hide_emitters; Russian roulette runs only in the films with rr_depth = 2
    (rr_depth = 5 lies behind max_depth = 2, rr_depth = 100 behind max_depth = 5)"""
    cannot = {"sky_own_density"} if sky == "envmap" else {"envmap_miss_after_smooth", "envmap_pole_clamp"}
    if not prm.hide_emitters:
        cannot |= {"area_emitter_hidden"}
    if prm.rr_depth != 2:
        cannot |= {"rr_after_null"}
    return EVERY - cannot, cannot


@pytest.mark.parametrize("sky", sorted(ALL_SKIES))
def test_d_the_all_features_scene_reaches_every_branch(hostmirror, oracle, abi, sky):
    """PER FILM, not summed: the counter RNG addresses its draws, so the films of the grid that differ in a depth limit or in
    hide_emitters repeat each other's paths, and a sum over them would count the same events again.  Every counter-RNG film (8 spp)
    reaches each of its meant tallies at least 100 times on its own.  The MSK_RNG_PCG_BLOCK films hold 2 spp, a quarter of the
    samples (2048): Russian roulette ends a path after a null bounce with probability 0.05, so 100 such ends would need about as
    many null bounces as the film has samples.  They are not held to 100: each meant tally must occur in them, and what a film
    cannot produce is 0 in both modes."""
    runs = twin_of_all_features(oracle, hostmirror, abi, sky)
    for prm, run in zip(all_features_params(abi), runs):
        t = run["tally"]
        what = "all-features %s rng %d hide %d max_depth %d rr_depth %d" % (sky, prm.rng_mode, prm.hide_emitters, prm.max_depth, prm.rr_depth)
        print("TALLY %s: %s" % (what, t))
        meant, cannot = all_features_coverage(abi, sky, prm)
        assert meant | cannot == EVERY
        for k in sorted(meant):
            assert t[k] >= (100 if prm.rng_mode == abi.MSK_RNG_COUNTER else 1), (what, k, t)
        for k in sorted(cannot):
            assert t[k] == 0, (what, k, t)


# the `direct` anchors of (h) at (h)'s parameters (max_depth = 2: one bounce).  Neither holds a mask
DIRECT_SPP = 512       # 24 x 20 pixels, where the glass ball fills a pixel or two: at the anchors' own 6 spp a mirror or glass bounce reaches an
                       # emitter a handful of times, at 192 spp 60 times on the envmap anchor; 512 spp make it 100 and more on both
DIRECT_COVERAGE = {
    "c_envmap": dict(meant={"envmap_miss_after_smooth", "emitter_after_delta", "texel_wrap", "envmap_pole_clamp"}, cannot=POINT_T | NULL_T | {"sky_own_density"}),
    "d_point_mirror_sky": dict(meant={"point_unoccluded", "point_occluded", "sky_own_density", "emitter_after_delta"}, cannot=NULL_T | {"envmap_miss_after_smooth", "envmap_pole_clamp", "texel_wrap"}),
}


def direct_params(abi):
    return abi.render_params(spp=DIRECT_SPP, seed=11, max_depth=2, rr_depth=5, block_size=DI.BS)


def twin_of_direct_anchor(oracle, hm, abi, name):
    key = ("direct", name)
    if key not in _twin_cache:
        flat = DI.anchor_flat(hm, name)
        o = oracle.scene(flat)
        (xyz, pos), _ = counted(oracle, lambda: sample_pixels_threaded(o, direct_params(abi), DI.all_pixels()))
        (film, st), tally = counted(oracle, lambda: o.render(direct_params(abi), threads=8))
        o.close()
        for a in (xyz, pos, film):
            a.setflags(write=False)
        _twin_cache[key] = dict(flat=flat, xyz=xyz, pos=pos, film=film, samples=st.samples, tally=tally)
    return _twin_cache[key]


@pytest.mark.parametrize("name", sorted(DIRECT_COVERAGE))
def test_d_direct_anchors_reach_their_branches(hostmirror, oracle, abi, name):
    t = twin_of_direct_anchor(oracle, hostmirror, abi, name)["tally"]
    cov = DIRECT_COVERAGE[name]
    print("TALLY direct anchor %s: %s" % (name, t))
    assert cov["meant"] | cov["cannot"] == EVERY
    for k in sorted(cov["meant"]):
        assert t[k] >= 100, (name, k, t)
    for k in sorted(cov["cannot"]):
        assert t[k] == 0, (name, k, t)


# ===================================================================================================== GPU layer
def no_knobs(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_counters(what, st, twin_st, tally, rng_mode, abi):
    """(see the module's docstring) samples equal; shadow rays = the twin's non-zero next-event terms; segments = the twin's count
    by the device's own rule, exactly"""
    print("COUNTERS %s: device samples %d segments %d shadow_rays %d; twin samples %d segments %d shadow_rays_nonzero %d dead_samples %d dropped %d extra %d" % (
        what, st.samples, st.segments, st.shadow_rays, twin_st[0], twin_st[1], tally["shadow_rays_nonzero"], tally["dead_samples"], tally["segments_dropped"], tally["segments_extra"]))
    assert st.samples == twin_st[0], what
    assert st.shadow_rays == tally["shadow_rays_nonzero"], what
    assert tally["segments_dropped"] + tally["segments_extra"] <= tally["dead_samples"]
    if rng_mode == abi.MSK_RNG_COUNTER:
        assert int(st.segments) == int(twin_st[1]) - tally["segments_dropped"] + tally["segments_extra"], what
    else:
        assert int(st.segments) == int(twin_st[1]), what


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", VARIANT_IDS)
def test_e_default_configuration_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, monkeypatch, name, which):
    no_knobs(monkeypatch)
    want = twin_of_variant(oracle, hostmirror, abi, name, which)
    p_xyz, p_film, p_serial = variant_params(abi)
    g = abi.Scene(gpu_ctx, want["flat"])
    try:
        xyz, pos = g.sample_pixels(p_xyz, EV.crop_pixels())
        film, st = g.render(p_film)
        serial, sst = g.render(p_serial)
    finally:
        g.close()
    assert np.array_equal(bits(pos), bits(want["pos"])), (name, which)
    bad = (bits(xyz) != bits(want["xyz"])).any(-1)
    assert not bad.any(), (name, which, int(bad.sum()), np.argwhere(bad)[:4].tolist(), xyz[bad][:3], want["xyz"][bad][:3])
    assert np.array_equal(bits(film), bits(want["film"])), (name, which, int((bits(film) != bits(want["film"])).sum()), float(np.abs(film - want["film"]).max()))
    assert np.array_equal(bits(serial), bits(want["serial"])), (name, which, int((bits(serial) != bits(want["serial"])).sum()))
    check_counters("%s %s film" % (name, which), st, want["st"], want["tally"], p_film.rng_mode, abi)
    check_counters("%s %s serial film" % (name, which), sst, want["sst"], want["stally"], p_serial.rng_mode, abi)


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["default", "hbm"])
@pytest.mark.parametrize("sky", sorted(ALL_SKIES))
def test_f_all_features_scene_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, monkeypatch, sky, placement):
    no_knobs(monkeypatch, **({"MSK_LDS_SCENE_KB": "0"} if placement == "hbm" else {}))
    runs = twin_of_all_features(oracle, hostmirror, abi, sky)
    g = abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky))
    try:
        for prm, want in zip(all_features_params(abi), runs):
            film, st = g.render(prm)
            what = "all-features %s %s rng %d hide %d max_depth %d rr_depth %d" % (sky, placement, prm.rng_mode, prm.hide_emitters, prm.max_depth, prm.rr_depth)
            assert np.array_equal(bits(film), bits(want["film"])), (what, int((bits(film) != bits(want["film"])).sum()), float(np.abs(film - want["film"]).max()))
            assert film[..., :3].max() > 0
            check_counters(what, st, want["st"], want["tally"], prm.rng_mode, abi)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sky", sorted(ALL_SKIES))
def test_f_crop_window_shards_and_samples(gpu_ctx, hostmirror, oracle, abi, monkeypatch, sky):
    """a crop window (both RNG modes); the two sample shards (0, 2) and (1, 2), each against the twin's film of the same shard; and
    the samples of every pixel (msk_gpu_sample_pixels ignores the shard selectors, as msk_oracle_sample_pixels does)"""
    no_knobs(monkeypatch)
    crop = (5, 3, 20, 18)
    prms = [abi.render_params(spp=8, seed=5, rr_depth=2), EV.pcg(abi, spp=2, seed=5, rr_depth=2)]
    o, g = oracle.scene(all_features_flat(hostmirror, sky, crop=crop)), abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky, crop=crop))
    try:
        for prm in prms:
            film, st = g.render(prm)
            ref, rst = o.render(prm, threads=8)
            assert film.shape == ref.shape == (18, 20, 5) and st.samples == rst.samples
            assert np.array_equal(bits(film), bits(ref)), (sky, prm.rng_mode, int((bits(film) != bits(ref)).sum()))
    finally:
        g.close(); o.close()
    o, g = oracle.scene(all_features_flat(hostmirror, sky)), abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky))
    try:
        for r in (0, 1):
            prm = abi.render_params(spp=8, seed=5, rr_depth=2, sample_first=r, sample_stride=2)
            film, st = g.render(prm)
            ref, rst = o.render(prm, threads=8)
            assert st.samples == rst.samples == 32 * 32 * 4
            assert np.array_equal(bits(film), bits(ref)), (sky, r, int((bits(film) != bits(ref)).sum()))
        px = np.array([(x, y) for y in range(32) for x in range(32)], np.int32)
        prm = abi.render_params(spp=4, seed=5, rr_depth=2, hide_emitters=1)
        xyz, pos = g.sample_pixels(prm, px)
        rxyz, rpos = sample_pixels_threaded(o, prm, px)
        assert np.array_equal(bits(pos), bits(rpos))
        bad = (bits(xyz) != bits(rxyz)).any(-1)
        assert not bad.any(), (sky, int(bad.sum()), np.argwhere(bad)[:4].tolist(), xyz[bad][:3], rxyz[bad][:3])
    finally:
        g.close(); o.close()


@pytest.mark.gpu
def test_g_aov_on_the_mask_scene_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, monkeypatch):
    """every channel of an "aov" render with the nested path integrator: a masked surface is a surface to the primary-hit channels"""
    no_knobs(monkeypatch)
    flat = twin_of_variant(oracle, hostmirror, abi, "mask", "lds")["flat"]
    types = [abi.MSK_AOV_DEPTH, abi.MSK_AOV_POSITION, abi.MSK_AOV_UV, abi.MSK_AOV_GEO_NORMAL, abi.MSK_AOV_SH_NORMAL, abi.MSK_AOV_PATH_RGBA]
    prm = abi.render_params(spp=4, seed=5)
    o, g = oracle.scene(flat), abi.Scene(gpu_ctx, flat)
    try:
        for t in (types, types[:5]):
            film, st = g.render_aov(prm, t)
            ref, rst = o.render_aov(prm, t, threads=8)
            assert film.shape == ref.shape and st.samples == rst.samples
            for c in range(film.shape[-1]):
                assert np.array_equal(bits(film[..., c]), bits(ref[..., c])), (len(t), c, int((bits(film[..., c]) != bits(ref[..., c])).sum()))
        assert np.abs(ref[..., 5:]).max() > 0
    finally:
        g.close(); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DIRECT_COVERAGE))
def test_h_direct_one_one_equals_the_twin_at_depth_two(gpu_ctx, hostmirror, oracle, abi, monkeypatch, name):
    """one hop to the reference instead of two: msk_gpu_sample_pixels_direct / msk_gpu_render_direct at (1, 1) against the twin's
    `path` at max_depth = 2, on the anchors of test_direct_integrator at the spp layer (d) needs (DIRECT_SPP)"""
    no_knobs(monkeypatch)
    want = twin_of_direct_anchor(oracle, hostmirror, abi, name)
    prm = direct_params(abi)
    g = abi.Scene(gpu_ctx, want["flat"])
    try:
        got, gpos = g.sample_pixels_direct(prm, DI.all_pixels(), 1, 1)
        film, st = g.render_direct(prm, 1, 1)
    finally:
        g.close()
    assert np.array_equal(bits(gpos), bits(want["pos"]))
    bad = (bits(got) != bits(want["xyz"])).any(-1)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:3], want["xyz"][bad][:3])
    assert st.samples == want["samples"] == DI.FW * DI.FH * DIRECT_SPP
    assert np.array_equal(bits(film), bits(want["film"])), (name, int((bits(film) != bits(want["film"])).sum()), float(np.abs(film - want["film"]).max()))
