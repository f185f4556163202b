"""The twin of the `thinlens` sensor and of the `spot` / `directional` emitters (oracle/oracle.cpp, D23 and D24), and the device
held to it bit for bit: the `_l` kernel family (k_shade_gen_l, k_wavefront_l, k_wavefront_h_l, k_direct<*, true>) and the delta
lights' films.

The layout is test_widened_oracle_parity's and test_plastic_oracle_parity's, whose helpers this file imports.
CPU layer (the twin earns trust before the device is held to it):
  (a)  msk_oracle_camera_sample against lens_ref.camera_ray32 on the inputs of test_thinlens' probe and on the disk map's creases,
       as uint32 (the signs of zeros included); the pinhole through the same hook against msk_oracle_camera_ray;
  (b)  the twin's renders against the float64 expectations the device meets, by those tests' own procedures and bounds: every case
       of test_spot_directional, the lens radiance cases, the sharp and the blurred edge, the mix scene of test_thinlens;
  (c)  identities that need no tolerance, (c') refusals;
  (d)  the path and direct tallies of every parity scene at the parameters the GPU layer uses, per film.
GPU layer (default knobs): every comparison is array_equal on the uint32 view; counters through check_counters.
  (e)  the anchors of test_every_execution_variant of test_thinlens / test_spot_directional, taken from those files' own
       `variant_reference` fixtures, against the twin;
  (f)  one all-features scene with a spot, a sun, both plastics and a lens: both skies, both table placements; 32 x 32 over the whole
       grid of depth limits x hide_emitters, the ragged 37 x 29 over the grid's first and last entry; without the lens under
       MSK_RNG_PCG_BLOCK;
  (g)  a crop window, both sample shards, every pixel's samples, every "aov" channel;
  (h)  k_direct with a lens and with spot / sun against the oracle's `direct`;
  (i)  the device's probes against the twin's hooks on the inputs of (a)."""
import ctypes as C

import numpy as np
import pytest

import envmap_ref as E
import lens_ref as L
import light_ref as LR
import oracle_binding
import test_delta_light_mirror as DM
import test_direct_integrator as DI
import test_direct_oracle_parity as DP
import test_envmap as EV
import test_plastic_bsdf as TP
import test_plastic_oracle_parity as PP
import test_radiometry_closed_form as RC
import test_spot_directional as SD
import test_thinlens as TL
import test_widened_oracle_parity as WP
from test_spot_directional import variant_reference as light_variant_reference      # noqa: F401  (the fixtures themselves: (e))
from test_thinlens import variant_reference as lens_variant_reference               # noqa: F401
from test_widened_oracle_parity import assert_bits, bits, check_counters, counted, meets, no_knobs, sample_pixels_threaded, twin_mean

F = np.float32
TOP = F(1 - 2.0 ** -24)                  # the largest float below 1
BIG_RADIUS = 300.0                       # a lens sixty focus distances wide: directions far from the axis
PATH_NAMES = oracle_binding.Oracle.PATH_TALLIES
DIRECT_NAMES = oracle_binding.Oracle.DIRECT_TALLIES
SPOT_T = {"spot_beam", "spot_ramp", "spot_dark", "spot_occluded", "spot_unoccluded"}
SUN_T = {"sun_occluded", "sun_unoccluded"}
LENS_T = {"lens_disk_first", "lens_disk_second"}
NEW = SPOT_T | SUN_T | LENS_T
EVERY = PP.EVERY | NEW
assert NEW == set(PATH_NAMES[25:]) and len(PATH_NAMES) == 34 and len(DIRECT_NAMES) == 28
# What no render can produce, so no tally exists for it: the disk map's centre branch (x == 0 and y == 0 needs u = (0.5, 0.5) exactly,
# one pair in 2^46) and a spot's dist == 0 (a surface point that is the spot's position).  Both belong to the hook tests: (a) feeds
# u = (0.5, 0.5) to msk_oracle_camera_sample, and test_plastic_oracle_parity's light hook test feeds the spot its own position.
CANNOT_PRODUCE = ("the disk map's centre branch", "a spot at dist == 0")


# ===================================================================================================== (a) the camera hook
def crease_inputs():
    """the branches of the concentric map and its creases, by hand: -> (u float32[n, 2], class per row).  x = 2 u.x - 1, y = 2 u.y - 1"""
    rows = [((0.5, 0.5), "centre")]
    rows += [((t, t), "tie") for t in (0.0, 0.125, 0.25, 0.75, 0.875, float(TOP))]                   # x == y
    rows += [((t, 1.0 - t), "tie") for t in (0.125, 0.25, 0.75, 0.875)]                              # x == -y (1 - t is exact)
    rows += [((0.5, t), "x0") for t in (0.0, 0.25, 0.75, float(TOP))]                                # x == 0, y != 0: the second branch
    rows += [((t, 0.5), "y0") for t in (0.0, 0.25, 0.75, float(TOP))]                                # y == 0, x != 0: the first branch
    rows += [((0.0, 0.3), "edge"), ((0.3, 0.0), "edge"), ((float(TOP), 0.3), "edge"), ((0.3, float(TOP)), "edge"), ((0.0, float(TOP)), "edge"), ((float(TOP), 0.0), "edge")]
    return np.array([r[0] for r in rows], F), [r[1] for r in rows]


def hook_inputs():
    """test_thinlens.probe_inputs() and behind them the creases, each at three film positions"""
    pos, u = TL.probe_inputs()
    cu, _ = crease_inputs()
    cpos = np.array([(32.0, 32.0), (0.25, 63.5), (47.125, 3.0)], F)
    return np.concatenate([pos, np.repeat(cpos, len(cu), 0)]), np.concatenate([u, np.tile(cu, (3, 1))])


def disk_branch(u):
    """the branch of square_to_uniform_disk_concentric a pair takes, from the map's own fp32 expressions: 0 centre, 1 first, 2 second"""
    u = np.ascontiguousarray(u, F).reshape(-1, 2)
    x, y = (F(2) * u[:, 0] - F(1)).astype(F), (F(2) * u[:, 1] - F(1)).astype(F)
    return np.where((x == 0) & (y == 0), 0, np.where((x * x).astype(F) > (y * y).astype(F), 1, 2))


HOOK_LENSES = [(0.0, TL.FOCUS), (TL.RADIUS, TL.FOCUS), (BIG_RADIUS, TL.FOCUS)]
HOOK_CAMERAS = {"z": TL.Z_CAM, "skew": TL.SKEW_CAM}


def hook_flat(hm, camera, lens=None):
    mesh = [TL.emitting_quad(hm, -1.0, 1.0, 4.0)]
    return hm.flatten(mesh, 64, 64, camera=TL.lens_cam(camera, *lens) if lens else camera)


def test_a_the_hand_made_inputs_take_the_branches_they_are_named_for():
    u, kind = crease_inputs()
    br = disk_branch(u)
    x, y = (F(2) * u[:, 0] - F(1)).astype(F), (F(2) * u[:, 1] - F(1)).astype(F)
    for k, (b, xx, yy) in zip(kind, zip(br, x, y)):
        if k == "centre":
            assert b == 0
        elif k == "tie":
            assert abs(xx) == abs(yy) and b == 2, (k, xx, yy)                 # x x > y y is false on a tie: the second branch
        elif k == "x0":
            assert xx == 0 and yy != 0 and b == 2
        elif k == "y0":
            assert yy == 0 and xx != 0 and b == 1
    assert u.min() == 0 and u.max() == TOP and TOP < 1 and np.nextafter(TOP, F(2)) == 1
    _, pu = TL.probe_inputs()
    assert set(disk_branch(pu).tolist()) == {0, 1, 2}


def test_a_on_a_tie_either_branch_of_the_disk_map_gives_the_same_point(oracle):
    """|x| == |y| goes to the second branch (x x > y y is false there).  The first branch would give the same bits: its angle is
    +-(pi / 4) where the second's is pi / 2 -+ pi / 4, fl(pi / 2) = 2 fl(pi / 4) exactly, and det_sincos mirrors a quadrant exactly.  So
    `x x >= y y` is the same function as `x x > y y`, no test can tell one from the other, and this one says why none has to"""
    t = np.random.RandomState(5).uniform(0, 1, 512).astype(F)
    cu, kind = crease_inputs()
    u = np.concatenate([cu[[k == "tie" for k in kind]], np.stack([t, t], -1), np.stack([t, (F(1) - t).astype(F)], -1)])
    x, y = (F(2) * u[:, 0] - F(1)).astype(F), (F(2) * u[:, 1] - F(1)).astype(F)
    keep = (np.abs(x) == np.abs(y)) & (x != 0)
    u, x, y = u[keep], x[keep], y[keep]
    assert len(u) > 700 and (x == y).sum() > 200 and (x == -y).sum() > 200
    sn, cs = E.det_sincos(oracle, (L.PI_4 * (y / x).astype(F)).astype(F))
    first = np.stack([(x * cs).astype(F), (x * sn).astype(F)], -1)
    assert_bits("the first branch on a tie", first, L.disk32(oracle, u))
    assert_bits("msk_oracle_warps on a tie", np.array([oracle.warps(q)[1] for q in u], F), first)


@pytest.mark.parametrize("cam", sorted(HOOK_CAMERAS))
def test_a_camera_hook_equals_lens_ref(hostmirror, oracle, cam):
    """msk_oracle_camera_sample against lens_ref.camera_ray32, every one of the eight floats of every ray as uint32: nothing is left
    out, a zero's sign included.  R = 0 goes through the lens code; the large lens reaches directions far from the axis."""
    pos, u = hook_inputs()
    for radius, focus in HOOK_LENSES:
        flat = hook_flat(hostmirror, HOOK_CAMERAS[cam], (radius, focus))
        assert flat.lens is not None and flat.lens.aperture_radius == F(radius)
        o = oracle.scene(flat)
        try:
            assert o.lens is flat.lens                                       # a flat with a lens does not reach the oracle as a pinhole
            got = o.camera_sample(pos, u)
            with pytest.raises(ValueError):
                o.camera_sample(pos)
        finally:
            o.close()
        want = L.camera_ray32(oracle, flat.desc, pos, u, (radius, focus))
        assert np.isfinite(got).all()
        assert_bits("camera ray", got, want, cam, radius)
        if radius == 0.0:
            pin = L.camera_ray32(oracle, flat.desc, pos)
            assert np.array_equal(got[:, :3], pin[:, :3])                    # the pinhole's origin as numbers (msk_lens_desc)
            if cam == "skew":
                assert_bits("origin at R = 0", got[:, :3], pin[:, :3])       # ... and as bits where no coordinate of it is zero
        else:
            assert (np.linalg.norm((got[:, :3] - got[0, :3]).astype(np.float64), axis=1) > 0).any()


@pytest.mark.parametrize("cam", sorted(HOOK_CAMERAS))
def test_a_pinhole_through_the_hook_is_camera_ray(hostmirror, oracle, cam):
    """a scene without a lens: the hook ignores aperture_u and gives msk_oracle_camera_ray's ray (which stays as it was) and lens_ref's"""
    pos, u = hook_inputs()
    flat = hook_flat(hostmirror, HOOK_CAMERAS[cam])
    assert flat.lens is None
    o = oracle.scene(flat)
    try:
        got, got_u = o.camera_sample(pos), o.camera_sample(pos, u)
        old = np.array([o.camera_ray(0.5, float(p[0]), float(p[1]))[0] for p in pos[:1200]], F)
    finally:
        o.close()
    assert_bits("hook with u", got_u, got)
    assert_bits("msk_oracle_camera_ray", got[:1200], old)
    assert_bits("lens_ref pinhole", got, L.camera_ray32(oracle, flat.desc, pos))


def test_a_a_hard_edged_spot_is_lit_on_its_edge(hostmirror, oracle):
    """what test_plastic_oracle_parity's light hook test leaves open: cos_cutoff == cos_beam == c.  The falloff is tested in the
    contract's order, c >= cos_beam first, so the point on the edge is lit at full intensity; with `c > cos_beam` it would fall to
    c <= cos_cutoff and be dark (with a ramp between the two cosines the slip cannot show: t = 1 gives f = 1 as well)"""
    pos, p, wl = SD.probe_points()
    flat = SD.probe_flat(hostmirror)
    sp_pos, sp_axis, cc, cb = SD.light_of(flat, 2)
    c = LR.spot_cosine32(sp_pos, sp_axis, p)
    f = LR.falloff32(c, cc, cb)
    k = int(np.argmax((f > 0.3) & (f < 0.7)))
    hard = SD.probe_flat(hostmirror, (c[k], c[k]))
    o = oracle.scene(hard)
    try:
        lp, la, lc, lb = SD.light_of(hard, 2)
        assert lc == lb == c[k]
        gd, gv = o.light_sample(2, p, wl)
    finally:
        o.close()
    rd, rv, pdf = LR.spot_sample32(lp, la, lc, lb, p, SD.emitter_value32(hostmirror, oracle, hard, 2, wl))
    assert_bits("d, dist", gd, rd)
    assert_bits("value", gv, rv)
    assert pdf[k] == 1 and gv[k].min() > 0 and set(np.unique(LR.falloff32(c[np.isfinite(c)], lc, lb)).tolist()) == {0.0, 1.0}
    inv = F(1) / gd[k, 3]
    assert_bits("full intensity on the edge", gv[k:k + 1], ((SD.emitter_value32(hostmirror, oracle, hard, 2, wl)[k:k + 1] * inv).astype(F) * inv).astype(F))


# ===================================================================================================== (b) float64 expectations on the twin
@pytest.mark.parametrize("name", SD.CASES)
def test_b_twin_meets_the_spot_and_sun_closed_forms(hostmirror, oracle, abi, name):
    """test_spot_directional.test_rendered_radiance_meets_the_closed_form on the twin: the same cases, depth limits, pixels, procedure
    and bound; in the dark and in the shadow exactly 0, and in the dark no shadow ray.  And what the new tallies need: on the three
    spot cases every next-event sample of the block takes the branch the case is named for, and no other"""
    flat, expected, _, _ = SD.closed_form_case(hostmirror, name)
    depth = 3 if name == "e_mirror_then_spot" else 2
    o = oracle.scene(flat)
    try:
        if name in SD.SPOT_CASES:
            (xyz, _), t = counted(oracle, lambda: o.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=depth), SD.case_pixels(name)))
            zone = {"a_beam": "spot_beam", "a_transition": "spot_ramp", "a_dark": "spot_dark"}[name]
            assert t[zone] == 64 * 64 and sum(t[k] for k in ("spot_beam", "spot_ramp", "spot_dark")) == 64 * 64, t
            assert t["spot_unoccluded"] == (0 if name == "a_dark" else 64 * 64) and t["spot_occluded"] == 0 and not any(t[k] for k in SUN_T | LENS_T), t
        if name in SD.BLACK:
            xyz, _ = o.sample_pixels(abi.render_params(spp=256, seed=7, max_depth=depth), SD.case_pixels(name))
            assert np.isfinite(xyz).all() and not xyz.any()
            (film, st), t = counted(oracle, lambda: o.render(abi.render_params(spp=8, seed=7, max_depth=depth), threads=8))
            c = SD.CROP
            assert np.isfinite(film).all() and not film[c[1]:c[1] + 8, c[0]:c[0] + 8, :3].any() and film[..., :3].max() > 0 and t["shadow_rays_nonzero"] > 0
            if name == "a_dark":
                d = oracle.scene(SD.dark_film_flat(hostmirror))
                (film, st), t = counted(oracle, lambda: d.render(abi.render_params(spp=8, seed=7, max_depth=depth), threads=8))
                d.close()
                assert st.samples == SD.W48 * SD.W48 * 8 and st.shadow_rays == 0 and t["shadow_rays_nonzero"] == 0 and not film[..., :3].any()
                assert t["spot_dark"] == st.samples and t["spot_beam"] == t["spot_ramp"] == 0, t      # every hit: f == 0, pdf 0
            else:
                assert t["sun_occluded"] >= 64 * 8 and t["sun_unoccluded"] > 0, t
            return
        mean, se = twin_mean(o, abi, "%s path" % name, expected, pixels=SD.case_pixels(name), max_depth=depth)
        if name == "e_mirror_then_spot":
            xyz, _ = o.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=2), SD.case_pixels(name))
            assert not xyz.any()
    finally:
        o.close()
    meets(mean, se, expected)


@pytest.mark.parametrize("direct", [False, True], ids=["path", "direct"])
@pytest.mark.parametrize("name", sorted(TL.RADIANCE_CASES))
def test_b_twin_lens_does_not_change_radiance(hostmirror, oracle, abi, name, direct):
    """test_thinlens.run_lens_radiance with the CPU side of test_radiometry_closed_form: the same expectation, sigma and cap"""
    TL.run_lens_radiance(name, RC.CpuSide(oracle, abi), hostmirror, abi, direct)


def test_b_twin_in_focus_it_is_sharp(hostmirror, oracle, abi):
    TL.check_sharp(oracle.scene, hostmirror, abi)


@pytest.mark.parametrize("depth", TL.BLUR_DEPTHS)
def test_b_twin_out_of_focus_it_blurs_by_the_right_amount(hostmirror, oracle, abi, depth):
    TL.check_blur(oracle.scene, hostmirror, abi, depth)


def check_each_sample_follows_its_own_aperture_sample(make_scene, oracle, hm, abi, depth):
    """test_thinlens' blurred edge, sample by sample instead of in the sum: the screen at z_e = depth f fills the side x > x0, and sample
    s of pixel p is lit exactly when the ray from ITS lens point, disk64(counter_pair(key(seed, p, s), 2)) R, to the focus point of
    its film position crosses the plane z = z_e on the lit side.  Float64 from the contract's text; what the distribution tests cannot
    see is seen here: the two components of pair 2 swapped, another pair, a mirrored disk.  Left out, under test_thinlens' margin
    m = 2^-17 f and for its reason: samples that cross within m of x0; their share is capped at 0.5 % first."""
    z_e = depth * TL.FOCUS
    edge, full, x0, side = TL.edge_setup(hm, abi, z_e)
    seed, spp = 23, 64
    prm = abi.render_params(spp=spp, seed=seed, max_depth=1)
    ge = make_scene(edge)
    try:
        xyz, pos = ge.sample_pixels(prm, TL.EDGE_PIXELS)
    finally:
        ge.close()
    u = np.array([[oracle.counter_pair(seed, int(y) * 64 + int(x), k, 2) for k in range(spp)] for x, y in TL.EDGE_PIXELS], np.float64)
    m = TL.to_world64(edge.desc)
    a = L.disk64(u.reshape(-1, 2)).reshape(len(TL.EDGE_PIXELS), spp, 2) * TL.RADIUS
    lens_w = a[..., 0:1] * m[:3, 0] + a[..., 1:2] * m[:3, 1] + m[:3, 3]
    focus_w = TL.focus_world64(edge.desc, pos.astype(np.float64), TL.FOCUS)
    t = (z_e - lens_w[..., 2]) / (focus_w[..., 2] - lens_w[..., 2])
    cross = lens_w[..., 0] + t * (focus_w[..., 0] - lens_w[..., 0])
    out = np.abs(cross - x0) < TL.MARGIN
    assert out.mean() <= 5e-3
    lit, want = xyz.any(-1), side * (cross - x0) > 0
    wrong = (lit != want) & ~out
    print("LENS per sample z_e = %.1f f: %d samples, %d lit, %d left out, %d wrong" % (depth, lit.size, int(lit.sum()), int(out.sum()), int(wrong.sum())))
    assert not wrong.any(), (depth, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    assert 0.2 < lit.mean() < 0.8
    b = L.disk64(u.reshape(-1, 2)[:, ::-1]).reshape(a.shape) * TL.RADIUS                   # (the slip this test is for: u.y, u.x)
    swapped = b[..., 0:1] * m[:3, 0] + b[..., 1:2] * m[:3, 1] + m[:3, 3]
    cs = swapped[..., 0] + t * (focus_w[..., 0] - swapped[..., 0])
    assert ((side * (cs - x0) > 0) != want).mean() > 0.1                 # ... would move a tenth of the samples across the edge


@pytest.mark.parametrize("depth", TL.BLUR_DEPTHS)
def test_b_twin_samples_follow_their_own_aperture_sample(hostmirror, oracle, abi, depth):
    check_each_sample_follows_its_own_aperture_sample(oracle.scene, oracle, hostmirror, abi, depth)


def test_b_twin_meets_the_mix_expectation(hostmirror, oracle, abi):
    """a mask, a spot in its ramp and an envmap under a lens (test_thinlens.mix_flats) against mix_expected, by twin_mean / meets:
    the procedure and bound of test_a_lens_over_mask_spot_and_envmap"""
    fe, fc = TL.mix_flats(hostmirror)
    expected = TL.mix_expected(fe, fc, 4)
    o = oracle.scene(fe)
    try:
        assert o.lens is not None and o.masks is not None and o.lights is not None and o.envmap is not None
        mean, se = twin_mean(o, abi, "lens over mask, spot, envmap", expected, pixels=SD.block_pixels(TL.MIX_BLOCK))
        (film, st), t = counted(oracle, lambda: o.render(abi.render_params(spp=4, seed=7), threads=8))
    finally:
        o.close()
    meets(mean, se, expected)
    assert np.isfinite(film).all() and st.samples == 48 * 48 * 4 and t["null_lobe"] > 100 and t["spot_ramp"] > 100 and min(t[k] for k in LENS_T) > 100, t


# ===================================================================================================== (c) identities on the twin
@pytest.mark.parametrize("hide", [0, 1])
def test_c_direct_one_one_is_path_at_depth_two_through_a_lens(hostmirror, oracle, abi, hide):
    """test_thinlens.test_direct_one_one_is_path_at_depth_two on the twin: the lens box under the envmap; samples, film positions and
    films as bits; and the pinhole's samples are others"""
    flat = TL.box_flat(hostmirror, abi, "lds", "envmap", size=(DI.FW, DI.FH))
    prm = abi.render_params(spp=6, seed=11, max_depth=2, rr_depth=5, hide_emitters=hide, block_size=DI.BS)
    o = oracle.scene(flat)
    try:
        want, wpos = sample_pixels_threaded(o, prm, DI.all_pixels())
        got, gpos = DP.oracle_samples(o, prm, DI.all_pixels(), 1, 1)
        film_p, st_p = o.render(prm, threads=8)
        film_d, st_d = o.render_direct(prm, 1, 1, threads=8)
    finally:
        o.close()
    assert_bits("positions", gpos.reshape(-1, 2), wpos.reshape(-1, 2))
    assert_bits("samples", got.reshape(-1, 3), want.reshape(-1, 3), hide)
    assert np.isfinite(want).all() and want.max() > 0
    assert np.array_equal(bits(film_d), bits(film_p)) and st_d.samples == st_p.samples == DI.FW * DI.FH * 6
    o = oracle.scene(TL.box_flat(hostmirror, abi, "lds", "envmap", size=(DI.FW, DI.FH), lens=None))
    pin, ppos = sample_pixels_threaded(o, prm, DI.all_pixels())
    o.close()
    assert np.array_equal(bits(ppos), bits(wpos)) and not np.array_equal(bits(pin), bits(want))


def test_c_the_film_is_the_sum_of_two_sample_shards(hostmirror, oracle, abi):
    """the lens variant scene: shards (0, 2) and (1, 2) add up to the film within test_thinlens.film_sum_bound"""
    want = twin_of_lens_variant(oracle, hostmirror, abi, "lds")
    o = oracle.scene(want["flat"])
    half = [o.render(abi.render_params(spp=8, seed=5, sample_first=r, sample_stride=2), threads=8) for r in (0, 1)]
    o.close()
    assert half[0][1].samples == half[1][1].samples == 48 * 48 * 4
    total = half[0][0].astype(np.float64) + half[1][0]
    assert np.all(np.abs(total - want["film"]) <= TL.film_sum_bound(want["film"], 8) + 1e-30)
    assert not np.array_equal(bits(half[0][0]), bits(half[1][0]))


def test_c_aperture_zero_is_the_pinhole_up_to_the_last_bits_of_the_direction(hostmirror, oracle, abi):
    """R = 0 goes through the lens code: the same film positions as bits; the samples are not the pinhole's bits, and, as
    test_plastic_bsdf.test_the_lens_tier_at_aperture_zero states it and with its bound, the relative difference of half of the lit
    samples stays under 1e-5"""
    prm = abi.render_params(spp=16, seed=5)
    out = []
    for lens in ((0.0, TL.BOX_LENS[1]), None):
        o = oracle.scene(TL.box_flat(hostmirror, abi, "lds", "none", lens=lens))
        assert (o.lens is None) == (lens is None)
        out.append(sample_pixels_threaded(o, prm, EV.crop_pixels()))
        o.close()
    (xyz, pos), (pxyz, ppos) = out
    assert np.array_equal(bits(pos), bits(ppos)) and not np.array_equal(bits(xyz), bits(pxyz))
    a, b = xyz.astype(np.float64).reshape(-1, 3), pxyz.astype(np.float64).reshape(-1, 3)
    lit = (b > 0).all(-1)
    rel = (np.abs(a - b)[lit] / b[lit]).max(-1)
    print("TWIN lens at R = 0: %d lit samples, median relative difference to the pinhole %.3g, 99th percentile %.3g" % (lit.sum(), np.median(rel), np.percentile(rel, 99)))
    assert lit.sum() > 500 and np.median(rel) <= 1e-5


def sky_box_flat(hm, abi, lens=True):
    """the open Cornell box (no ceiling, no back wall) under a `constant` sky and nothing else that would select a newer kernel
    family: diffuse surfaces, one area lamp; with lens, seen through a lens"""
    flat = hm.flatten(DI.open_box(hm), 32, 32, env={"radiance": (12.0, 15.0, 20.0)})
    return TL.with_lens(abi, flat, *ALL_LENS) if lens else flat


def test_c_a_lens_scene_counts_a_constant_sky_with_its_own_density(hostmirror, oracle, abi, packer_constants):
    """msk_lens_desc: a scene with a lens runs kernels of its own, which carry the mask code, and msk_mask_desc: "A `constant` sky
    counts with the density of the ray's own direction" (oracle.cpp, D24).  So an unused plastic entry, which switches that rule on
    in any scene (D22), changes no bit of a lens scene's film and does change the pinhole's, which keeps the stale record (D9).
    Found by the randomised sweep (test_fuzz_parity: seeds 13001, 13005, 13010, 13020, 13031, 13037, every scene of the first sweep
    with a `constant` sky): the twin kept the stale record under a lens"""
    prm = abi.render_params(spp=8, seed=5)
    films, tallies = {}, {}
    for lens in (True, False):
        for extra in (False, True):
            flat = sky_box_flat(hostmirror, abi, lens)
            if extra:
                flat = PP.with_trailing_plastic(hostmirror, abi, flat, TP.plastic(0.4, 0.9, 1.6, True))
            o = PP.open_twin(oracle, packer_constants, flat)
            (film, _), t = counted(oracle, lambda: o.render(prm, threads=8))
            o.close()
            films[lens, extra], tallies[lens, extra] = film, t
    assert np.array_equal(bits(films[True, False]), bits(films[True, True])) and films[True, False][..., :3].max() > 0
    assert not np.array_equal(bits(films[False, False]), bits(films[False, True]))
    print("TALLY lens over a constant sky alone: %s" % tallies[True, False])
    assert tallies[True, False]["sky_own_density"] >= 100 and tallies[False, False]["sky_own_density"] == 0 and tallies[False, True]["sky_own_density"] >= 100


# ----------------------------------------------------------------------------------------------------- (c') refusals
def test_c_the_oracle_refuses_what_the_library_refuses_of_a_lens(hostmirror, oracle, abi):
    """each bad msk_lens_desc field: ValueError at scene creation; R = 0 is valid; a MSK_RNG_PCG_BLOCK render of a lens scene through
    every render entry point: ValueError, where the same scene without its lens renders"""
    lamp = hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))
    flat = hostmirror.flatten([DM.plane(hostmirror), lamp], 16, 16, camera=EV.PLANE_CAMERA)
    for radius, focus in ((-1.0, 5.0), (np.nan, 5.0), (np.inf, 5.0), (-np.inf, 5.0), (-2.0 ** -149, 5.0), (0.5, 0.0), (0.5, -0.0), (0.5, -2.0), (0.5, np.inf), (0.5, -np.inf), (0.5, np.nan)):
        with pytest.raises(ValueError):
            oracle.scene(flat, lens=abi.LensDesc(radius, focus))
    oracle.scene(flat, lens=abi.LensDesc(-0.0, 5.0)).close()                 # -0 is not negative
    o = oracle.scene(flat, lens=abi.LensDesc(0.0, 5.0))
    pin = oracle.scene(flat)
    try:
        pcg, ok = EV.pcg(abi, spp=2, seed=5), abi.render_params(spp=2, seed=5)
        px = EV.crop_pixels()[:2]
        calls = {"render": lambda s, p: s.render(p, threads=2), "render_aov": lambda s, p: s.render_aov(p, [abi.MSK_AOV_DEPTH], threads=2),
                 "sample_pixels": lambda s, p: s.sample_pixels(p, px), "render_direct": lambda s, p: s.render_direct(p, 1, 1, threads=2),
                 "sample_pixels_direct": lambda s, p: s.sample_pixels_direct(p, px, 1, 1), "direct_terms": lambda s, p: s.direct_terms(p, (3, 3), 0, 1, 1)}
        for name, call in calls.items():
            with pytest.raises(ValueError if "direct" in name else oracle_binding.OracleRefusal):      # (the refusal's own type: no other failure passes for it)
                call(o, pcg)
            call(o, ok)                                                       # the counter RNG takes the lens scene through every entry
            if name in ("render", "render_aov"):
                call(pin, pcg)                                                # ... and the pinhole renders under MSK_RNG_PCG_BLOCK as it did
        film, st = o.render(ok, threads=2)
        assert np.isfinite(film).all() and st.samples == 16 * 16 * 2
        assert o.direct_terms(ok, (3, 3), 0, 2, 1)["draws"][:3] == [0, 1, 2] and pin.direct_terms(ok, (3, 3), 0, 2, 1)["draws"][:3] == [0, 1, 3]      # pair 2, and no other draw moves
    finally:
        o.close(); pin.close()
    # msk_oracle_scene_create_lens with lens = NULL is the older entry: the same film as bits
    eln = abi.SceneLens(abi.SceneLights(abi.SceneMasks(abi.SceneExt(None, 0, None), 0, None), 0, None), None)
    h = oracle.lib.msk_oracle_scene_create_lens(C.byref(flat.desc), C.byref(eln))
    assert h
    a, st = np.zeros((16, 16, 5), F), abi.Stats()
    assert oracle.lib.msk_oracle_render(h, C.byref(pcg), a.ctypes.data_as(C.c_void_p), C.byref(st), 2) == 0
    oracle.lib.msk_oracle_scene_destroy(h)
    o = oracle.scene(flat)
    b, _ = o.render(pcg, threads=2)
    o.close()
    assert np.array_equal(bits(a), bits(b)) and a[..., :3].max() > 0


def test_c_the_oracle_refuses_what_the_library_refuses_of_a_light(hostmirror, oracle, abi):
    """the refusals of msk_light_desc that test_plastic_oracle_parity's light hook test does not hold (a sun without its descriptor and a
    direction that is not unit length are there): the list of test_spot_directional.test_gpu_rejects_bad_light_descriptors"""
    lamp = hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))

    def fresh():
        return hostmirror.flatten([DM.plane(hostmirror), lamp], 16, 16, camera=SD.CAM, lights=[SD.spot_spec((0.0, 0.0, 1.4), 40.0, 30.0), SD.sun_spec()])

    def copy(l, **kw):
        c = abi.LightDesc.from_buffer_copy(bytes(l))
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    def refused(flat, lights=None):
        with pytest.raises(ValueError):
            oracle.scene(flat, lights=lights)
    flat = fresh()
    assert [flat.desc.emitters[i].type for i in range(3)] == [0, 4, 5] and [l.emitter for l in flat.lights] == [1, 2]
    sp, su = flat.lights[0], flat.lights[1]
    oracle.scene(flat).close()
    oracle.scene(flat, lights=[su, sp]).close()                              # in any order
    h = oracle.lib.msk_oracle_scene_create(C.byref(fresh().desc))            # the older entry: refused, not defaulted
    assert not h
    refused(flat, [sp]); refused(flat, [su])                                 # one of the two without its descriptor
    refused(flat, [sp, su, sp]); refused(flat, [sp, su, su])                 # two descriptors
    refused(flat, [sp, su, copy(sp, emitter=0)]); refused(flat, [sp, su, copy(sp, emitter=7)])      # another type, out of range
    for bad in (np.inf, -np.inf, np.nan):
        refused(flat, [copy(sp, position=(1, bad)), su])
        refused(flat, [copy(sp, direction=(0, bad)), su])
        refused(flat, [sp, copy(su, direction=(2, bad))])
    oracle.scene(flat, lights=[sp, copy(su, position=(1, np.nan))]).close()  # a sun's position is ignored
    refused(flat, [copy(sp, direction=(1, float(sp.direction[1]) * 1.01)), su])
    refused(flat, [sp, copy(su, direction=(1, 0.0))])
    refused(flat, [copy(sp, cos_cutoff=1.0, cos_beam=1.0), su]); refused(flat, [copy(sp, cos_cutoff=-1.5), su]); refused(flat, [copy(sp, cos_cutoff=np.nan), su])
    refused(flat, [copy(sp, cos_beam=float(np.nextafter(F(sp.cos_cutoff), F(-1)))), su]); refused(flat, [copy(sp, cos_beam=1.25), su]); refused(flat, [copy(sp, cos_beam=np.nan), su])
    oracle.scene(flat, lights=[copy(sp, cos_cutoff=-1.0, cos_beam=-1.0), su]).close()      # the point light
    oracle.scene(flat, lights=[copy(sp, cos_beam=float(sp.cos_cutoff)), su]).close()       # a hard edge
    el = abi.SceneLights(abi.SceneMasks(abi.SceneExt(None, 0, None), 0, None), 2, None)    # n_lights without lights
    assert not oracle.lib.msk_oracle_scene_create_lights(C.byref(flat.desc), C.byref(el))
    for e_id in (1, 2):
        f2 = fresh()
        f2.desc.emitters[e_id].mesh_id = 0
        refused(f2)
    none = hostmirror.flatten([DM.plane(hostmirror), lamp], 16, 16, camera=SD.CAM)
    refused(none, [copy(sp, emitter=0)])
    f9 = fresh()
    f9.desc.emitters[1].type = 9
    refused(f9)


# ===================================================================================================== the parity scenes
ALL_LENS = (18.0, 1050.0)                # in the Cornell box's units: a lens focused on the boxes
# Shaped until every film of (d) reaches every meant tally 100 times.  The spot stands left of the camera's view at half the box's
# height and looks across the floor at the boxes: its cone (half-angles 27 and 46 degrees) is narrow enough for its edge to cross the
# floor, both boxes and the far wall, so beam, ramp and dark all lie on lit surfaces, and the boxes shadow one another from it.  (From
# above the front of the box, as first tried, 36 samples of the max_depth = 2 films lay in the beam and 84 were occluded.)  The sun
# stands low on the left (37 degrees above the horizon): the boxes and the half-open left wall throw long shadows over the floor; at
# the first try, 65 degrees up and shining into the box, 54 of its samples were occluded.
ALL_SPOT = SD.spot_spec((330.0, 80.0, 250.0), 46.0, 27.0, origin=(60.0, 300.0, -40.0), intensity=(6e5, 5e5, 4e5))
ALL_SUN = SD.sun_spec((0.8, -0.6, 0.3), (5.0, 4.5, 4.0))
ALL_SIZES = {"32x32": (32, 32, 32), "37x29": (37, 29, 16)}      # (width, height, block size): the second is ragged, the last 64-lane batch of a region is partial


def all_features_flat(hm, sky, size="32x32", lens=True, crop=None):
    """test_plastic_oracle_parity.all_features_meshes (test_widened_oracle_parity's box: mask, bitmap, conductor, glass, point light,
    sky; with a plastic, roughplastics and the panel) under a spot, a sun and, with lens, a `thinlens` sensor"""
    w, h, _ = ALL_SIZES[size]
    camera = TL.lens_cam(hm.CBOX_CAMERA, *ALL_LENS) if lens else None
    return hm.flatten(PP.all_features_meshes(hm), w, h, env=WP.ALL_SKIES[sky](), points=[WP.ALL_POINT], lights=[ALL_SPOT, ALL_SUN], camera=camera, crop=crop)


def all_features_params(abi, size="32x32"):
    """counter RNG: hide_emitters 0 / 1 x WP.ALL_DEPTHS at 8 spp (the ragged size: the first and the last of them)"""
    bs = ALL_SIZES[size][2]
    grid = [dict(seed=5, hide_emitters=hide, block_size=bs, **depth) for hide in (0, 1) for depth in WP.ALL_DEPTHS]
    return [abi.render_params(spp=8, **kw) for kw in (grid if size == "32x32" else [grid[0], grid[-1]])]


def serial_params(abi):
    """MSK_RNG_PCG_BLOCK at 2 spp, for the scene without its lens"""
    return [EV.pcg(abi, spp=2, seed=5, hide_emitters=hide, **depth) for hide in (0, 1) for depth in WP.ALL_DEPTHS]


_twin_cache = {}


def twin_of_lens_variant(oracle, hm, abi, which):
    """the twin's samples, film, counters and tallies of test_thinlens' variant scene, at that fixture's parameters: once, never changed"""
    key = ("lens", which)
    if key not in _twin_cache:
        flat = TL.box_flat(hm, abi, which, "none", camera=TL.WIDE_CAMERA)
        o = oracle.scene(flat)
        p_xyz, p_film, _ = WP.variant_params(abi)
        (xyz, pos), _ = counted(oracle, lambda: sample_pixels_threaded(o, p_xyz, EV.crop_pixels()))
        (film, st), tally = counted(oracle, lambda: o.render(p_film, threads=8))
        o.close()
        for a in (xyz, pos, film):
            a.setflags(write=False)
        _twin_cache[key] = dict(flat=flat, xyz=xyz, pos=pos, film=film, st=(st.samples, st.segments), tally=tally)
    return _twin_cache[key]


def twin_of_light_variant(oracle, hm, abi, sky, which):
    key = ("light", sky, which)
    if key not in _twin_cache:
        flat = SD.box_flat(hm, which, sky)
        o = oracle.scene(flat)
        p_xyz, p_film, p_serial = WP.variant_params(abi)
        (xyz, pos), _ = counted(oracle, lambda: sample_pixels_threaded(o, p_xyz, EV.crop_pixels()))
        (film, st), tally = counted(oracle, lambda: o.render(p_film, threads=8))
        (serial, sst), stally = counted(oracle, lambda: o.render(p_serial, threads=8))
        o.close()
        for a in (xyz, pos, film, serial):
            a.setflags(write=False)
        _twin_cache[key] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, st=(st.samples, st.segments), tally=tally,
                                sst=(sst.samples, sst.segments), stally=stally)
    return _twin_cache[key]


def twin_of_all_features(oracle, packer_constants, hm, abi, sky, size="32x32", lens=True):
    key = ("all", sky, size, lens)
    if key not in _twin_cache:
        o = PP.open_twin(oracle, packer_constants, all_features_flat(hm, sky, size, lens))
        out = []
        for prm in (all_features_params(abi, size) if lens else serial_params(abi)):
            (film, st), tally = counted(oracle, lambda: o.render(prm, threads=8))
            film.setflags(write=False)
            out.append(dict(film=film, st=(st.samples, st.segments), tally=tally))
        o.close()
        _twin_cache[key] = out
    return _twin_cache[key]


packer_constants = PP.packer_constants      # (the fixture: every plastic's constants are the packer's bits before a twin scene renders)


# ===================================================================================================== (d) coverage
LIGHT_T = SPOT_T | SUN_T | {"point_unoccluded", "point_occluded"}
# test_thinlens' and test_spot_directional's variant boxes: an area lamp, a spot, a sun, a bitmap floor, a glass ball and a mirror
# ball; no point light (point_unoccluded / point_occluded count the spot's and the sun's samples: any delta light), no mask, no
# plastic.  These scenes belong to the `variant_reference` fixtures and are not shaped here.  Without a sky a mirror or glass bounce
# reaches an emitter only by finding the small lamp (emitter_after_delta: 1 to 3): neither required nor impossible there.
VARIANT_CANNOT = WP.NULL_T | set(PATH_NAMES[15:25]) | {"sky_own_density"}
LENS_VARIANT_COVERAGE = dict(meant=LIGHT_T | LENS_T | {"texel_wrap"}, cannot=VARIANT_CANNOT | {"envmap_miss_after_smooth", "envmap_pole_clamp"})
LIGHT_VARIANT_COVERAGE = {
    "none": dict(meant=LIGHT_T | {"texel_wrap"}, cannot=VARIANT_CANNOT | LENS_T | {"envmap_miss_after_smooth", "envmap_pole_clamp"}),
    "envmap": dict(meant=LIGHT_T | {"texel_wrap", "emitter_after_delta", "envmap_miss_after_smooth", "envmap_pole_clamp"}, cannot=VARIANT_CANNOT | LENS_T),
}
LIGHT_VARIANT_IDS = [(sky, which) for sky in ("none", "envmap") for which in ("lds", "hbm")]


def holds(what, t, cov, least=100):
    assert cov["meant"] | cov["cannot"] <= EVERY and not cov["meant"] & cov["cannot"]
    for k in sorted(cov["meant"]):
        assert t[k] >= least, (what, k, t)
    for k in sorted(cov["cannot"]):
        assert t[k] == 0, (what, k, t)
    assert t["point_unoccluded"] + t["point_occluded"] >= sum(t[k] for k in ("spot_occluded", "spot_unoccluded", "sun_occluded", "sun_unoccluded"))
    assert t["spot_beam"] + t["spot_ramp"] >= t["spot_occluded"] + t["spot_unoccluded"]      # (>: a sample whose BSDF value is zero traces no shadow ray on the device, but has a density here)


@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_d_the_lens_variant_scene_reaches_its_branches(hostmirror, oracle, abi, which):
    t = twin_of_lens_variant(oracle, hostmirror, abi, which)["tally"]
    print("TALLY lens variant %s: %s" % (which, t))
    holds(("lens variant", which), t, LENS_VARIANT_COVERAGE)
    assert t["lens_disk_first"] + t["lens_disk_second"] == 48 * 48 * 8       # every camera ray of the film


@pytest.mark.parametrize("sky,which", LIGHT_VARIANT_IDS)
def test_d_the_light_variant_scenes_reach_their_branches(hostmirror, oracle, abi, sky, which):
    run = twin_of_light_variant(oracle, hostmirror, abi, sky, which)
    print("TALLY light variant %s %s film: %s" % (sky, which, run["tally"]))
    print("TALLY light variant %s %s serial film: %s" % (sky, which, run["stally"]))
    holds(("light variant", sky, which), run["tally"], LIGHT_VARIANT_COVERAGE[sky])
    holds(("light variant serial", sky, which), run["stally"], LIGHT_VARIANT_COVERAGE[sky], least=1)


def all_features_coverage(abi, sky, prm, lens):
    """(meant, cannot) of ONE film: test_plastic_oracle_parity's rule for the twenty-one earlier events; the spot's and the sun's seven
    are meant in every film, the lens' two in every film through the lens and impossible without it"""
    meant, cannot = PP.all_features_coverage(abi, sky, prm)
    cannot = set(cannot) | (set() if lens else LENS_T)
    return (set(meant) | NEW) - cannot, cannot


@pytest.mark.parametrize("size", sorted(ALL_SIZES))
@pytest.mark.parametrize("sky", sorted(WP.ALL_SKIES))
def test_d_the_all_features_scene_reaches_every_branch(hostmirror, oracle, abi, packer_constants, sky, size):
    """PER FILM, as test_widened_oracle_parity's (d) and for its reason: every counter-RNG film reaches each of its meant tallies at
    least 100 times on its own; what a film cannot produce is 0"""
    runs = twin_of_all_features(oracle, packer_constants, hostmirror, abi, sky, size)
    for prm, run in zip(all_features_params(abi, size), runs):
        t = run["tally"]
        what = "all-features-lens %s %s hide %d max_depth %d rr_depth %d" % (sky, size, prm.hide_emitters, prm.max_depth, prm.rr_depth)
        print("TALLY %s: %s" % (what, t))
        meant, cannot = all_features_coverage(abi, sky, prm, True)
        assert meant | cannot == EVERY
        holds(what, t, dict(meant=meant, cannot=cannot))


@pytest.mark.parametrize("sky", sorted(WP.ALL_SKIES))
def test_d_the_all_features_scene_without_its_lens_reaches_the_lights_in_the_serial_films(hostmirror, oracle, abi, packer_constants, sky):
    """the 2-spp MSK_RNG_PCG_BLOCK films (a quarter of the samples): each meant tally at least once, as the earlier files hold theirs"""
    runs = twin_of_all_features(oracle, packer_constants, hostmirror, abi, sky, lens=False)
    for prm, run in zip(serial_params(abi), runs):
        what = "all-features-lights serial %s hide %d max_depth %d rr_depth %d" % (sky, prm.hide_emitters, prm.max_depth, prm.rr_depth)
        print("TALLY %s: %s" % (what, run["tally"]))
        meant, cannot = all_features_coverage(abi, sky, prm, False)
        holds(what, run["tally"], dict(meant=meant, cannot=cannot), least=1)


# `direct` (h): test_thinlens' lens box under the envmap (spot, sun, area lamp, image) at the parameters of (h)
DIRECT_NM = SD.DIRECT_NM + [(4, 2)]
DIRECT_SPP = 16                          # at 6 spp (4, 2) reaches the sun's occluded samples 64 times on this 24 x 20 film; 16 spp make it 100 and more
DIRECT_MEANT = {"light_spot_visible", "light_spot_occluded", "light_spot_dark", "light_sun_visible", "light_sun_occluded", "light_area_visible", "light_image",
                "light_point_visible", "light_point_occluded"}
DIRECT_CANNOT = {"light_point_only_visible", "light_point_only_occluded", "light_constant_sky", "bsdf_miss_constant", "bsdf_miss_nothing"}


def direct_prm(abi):
    return abi.render_params(spp=DIRECT_SPP, seed=11, block_size=DI.BS)


def direct_flats(hm, abi):
    """(h)'s scenes: the lens box under the image (k_direct<*, true>) and the same box without its lens (spot and sun through k_direct<*, false>)"""
    return {"lens": TL.box_flat(hm, abi, "lds", "envmap", size=(DI.FW, DI.FH)), "pinhole": TL.box_flat(hm, abi, "lds", "envmap", size=(DI.FW, DI.FH), lens=None)}


def twin_of_direct(oracle, hm, abi, name, n, m):
    key = ("direct", name, n, m)
    if key not in _twin_cache:
        o = oracle.scene(direct_flats(hm, abi)[name])
        try:
            (film, st), tally = DP.counted(oracle, lambda: o.render_direct(direct_prm(abi), n, m, threads=8))
            samples = DP.oracle_samples(o, direct_prm(abi), DI.all_pixels(), n, m)
        finally:
            o.close()
        film.setflags(write=False)
        _twin_cache[key] = dict(film=film, st=DP.stats_of(st), tally=tally, samples=samples)
    return _twin_cache[key]


@pytest.mark.parametrize("name", ["lens", "pinhole"])
def test_d_the_direct_renders_tell_the_delta_lights_apart(hostmirror, oracle, abi, name):
    """(4, 2) at DIRECT_SPP reaches every meant direct tally 100 times; at every (N, M) the spot's and the sun's tallies add up to the
    delta lights' and the scene's impossible ones stay 0"""
    for n, m in DIRECT_NM:
        t = twin_of_direct(oracle, hostmirror, abi, name, n, m)["tally"]
        print("TALLY direct %s (%d, %d): %s" % (name, n, m, {k: v for k, v in t.items() if v}))
        assert t["light_spot_visible"] + t["light_sun_visible"] == t["light_point_visible"] and t["light_spot_occluded"] + t["light_sun_occluded"] == t["light_point_occluded"]
        for k in sorted(DIRECT_CANNOT):
            assert t[k] == 0, (name, n, m, k, t)
        if n == 0:
            assert not any(t[k] for k in DIRECT_MEANT), t
        if (n, m) == (4, 2):
            for k in sorted(DIRECT_MEANT):
                assert t[k] >= 100, (name, k, t)


def test_d_a_point_light_is_told_from_a_spot_and_a_sun(hostmirror, oracle, abi):
    """test_spot_directional's probe scene holds a lamp, a point light, two spots and a sun: the three delta lights' tallies add up"""
    o = oracle.scene(SD.probe_flat(hostmirror))
    (_, st), t = DP.counted(oracle, lambda: o.render_direct(abi.render_params(spp=64, seed=3), 4, 0, threads=8))
    o.close()
    print("TALLY direct probe scene: %s" % {k: v for k, v in t.items() if v})
    vis = [t[k] for k in ("light_spot_visible", "light_sun_visible", "light_point_only_visible")]
    assert min(vis) >= 100 and sum(vis) == t["light_point_visible"] and t["light_spot_dark"] >= 100
    assert t["light_spot_occluded"] + t["light_sun_occluded"] + t["light_point_only_occluded"] == t["light_point_occluded"]


# ===================================================================================================== GPU layer
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_e_the_lens_anchor_equals_the_twin(lens_variant_reference, hostmirror, oracle, abi, which):
    """test_thinlens.variant_reference, the fixture test_every_execution_variant compares every variant with (made with no knob set):
    its samples, film positions and film against the twin's.  The wide camera's rays miss the scene's bounds 10 to 80 % of the time
    (the fixture asserts it): the cull that starts from a per-sample lens origin is in this film"""
    got, want = lens_variant_reference[which], twin_of_lens_variant(oracle, hostmirror, abi, which)
    assert bytes(got["flat"].desc.camera) == bytes(want["flat"].desc.camera) and bytes(got["flat"].lens) == bytes(want["flat"].lens)
    assert np.array_equal(got["flat"].vertices.view(np.uint32), want["flat"].vertices.view(np.uint32))
    assert np.array_equal(bits(got["pos"]), bits(want["pos"])), which
    bad = (bits(got["xyz"]) != bits(want["xyz"])).any(-1)
    assert not bad.any(), (which, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got["xyz"][bad][:3], want["xyz"][bad][:3])
    assert np.array_equal(bits(got["film"]), bits(want["film"])), (which, int((bits(got["film"]) != bits(want["film"])).sum()), float(np.abs(got["film"] - want["film"]).max()))
    assert got["samples"] == want["st"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lds", "hbm"])
def test_e_the_lens_scene_counters_equal_the_twin(gpu_ctx, hostmirror, oracle, abi, monkeypatch, which):
    """the fixture keeps no msk_stats beyond the sample count: the same render again, for check_counters (and the film once more)"""
    no_knobs(monkeypatch)
    want = twin_of_lens_variant(oracle, hostmirror, abi, which)
    g = abi.Scene(gpu_ctx, want["flat"])
    try:
        film, st = g.render(WP.variant_params(abi)[1])
    finally:
        g.close()
    assert np.array_equal(bits(film), bits(want["film"])), which
    check_counters("lens variant %s film" % which, st, want["st"], want["tally"], abi.MSK_RNG_COUNTER, abi)


@pytest.mark.gpu
@pytest.mark.parametrize("sky,which", LIGHT_VARIANT_IDS)
def test_e_the_light_anchors_equal_the_twin(light_variant_reference, gpu_ctx, hostmirror, oracle, abi, monkeypatch, sky, which):
    """test_spot_directional.variant_reference against the twin: samples, film positions, the film, the serial film; then the counters
    of both films from a render of the same scene with no knob set"""
    got, want = light_variant_reference[sky, which], twin_of_light_variant(oracle, hostmirror, abi, sky, which)
    assert np.array_equal(got["flat"].vertices.view(np.uint32), want["flat"].vertices.view(np.uint32))
    assert np.array_equal(bits(got["pos"]), bits(want["pos"])), (sky, which)
    bad = (bits(got["xyz"]) != bits(want["xyz"])).any(-1)
    assert not bad.any(), (sky, which, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got["xyz"][bad][:3], want["xyz"][bad][:3])
    assert np.array_equal(bits(got["film"]), bits(want["film"])), (sky, which, int((bits(got["film"]) != bits(want["film"])).sum()), float(np.abs(got["film"] - want["film"]).max()))
    assert np.array_equal(bits(got["serial"]), bits(want["serial"])), (sky, which, int((bits(got["serial"]) != bits(want["serial"])).sum()))
    assert got["samples"] == want["st"][0]
    no_knobs(monkeypatch)
    _, p_film, p_serial = WP.variant_params(abi)
    g = abi.Scene(gpu_ctx, want["flat"])
    try:
        film, st = g.render(p_film)
        serial, sst = g.render(p_serial)
    finally:
        g.close()
    assert np.array_equal(bits(film), bits(want["film"])) and np.array_equal(bits(serial), bits(want["serial"]))
    check_counters("light variant %s %s film" % (sky, which), st, want["st"], want["tally"], p_film.rng_mode, abi)
    check_counters("light variant %s %s serial film" % (sky, which), sst, want["sst"], want["stally"], p_serial.rng_mode, abi)


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["default", "hbm"])
@pytest.mark.parametrize("size", sorted(ALL_SIZES))
@pytest.mark.parametrize("sky", sorted(WP.ALL_SKIES))
def test_f_all_features_scene_with_a_lens_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, packer_constants, monkeypatch, sky, size, placement):
    """every film of all_features_params: at 32 x 32 the whole grid WP.ALL_DEPTHS x hide_emitters (six films); at the ragged 37 x 29
    with block size 16, where the last 64-lane batch of a region is partial, the grid's first and last entry (two films: no depth
    limit with rr_depth 2 and hide_emitters 0; max_depth 5 with hide_emitters 1).  A MSK_RNG_PCG_BLOCK render is refused"""
    no_knobs(monkeypatch, **({"MSK_LDS_SCENE_KB": "0"} if placement == "hbm" else {}))
    runs = twin_of_all_features(oracle, packer_constants, hostmirror, abi, sky, size)
    g = abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky, size))
    try:
        for prm, want in zip(all_features_params(abi, size), runs):
            film, st = g.render(prm)
            what = "all-features-lens %s %s %s hide %d max_depth %d rr_depth %d" % (sky, size, placement, prm.hide_emitters, prm.max_depth, prm.rr_depth)
            assert np.array_equal(bits(film), bits(want["film"])), (what, int((bits(film) != bits(want["film"])).sum()), float(np.abs(film - want["film"]).max()))
            assert film[..., :3].max() > 0
            check_counters(what, st, want["st"], want["tally"], prm.rng_mode, abi)
        with pytest.raises(abi.MskError):
            g.render(EV.pcg(abi, spp=2, seed=5))
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["default", "hbm"])
@pytest.mark.parametrize("sky", sorted(WP.ALL_SKIES))
def test_f_all_features_scene_without_its_lens_equals_the_twin_in_the_serial_kernels(gpu_ctx, hostmirror, oracle, abi, packer_constants, monkeypatch, sky, placement):
    """the same scene without the lens under MSK_RNG_PCG_BLOCK at 2 spp: the spot and the sun in the serial kernels"""
    no_knobs(monkeypatch, **({"MSK_LDS_SCENE_KB": "0"} if placement == "hbm" else {}))
    runs = twin_of_all_features(oracle, packer_constants, hostmirror, abi, sky, lens=False)
    g = abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky, lens=False))
    try:
        for prm, want in zip(serial_params(abi), runs):
            film, st = g.render(prm)
            what = "all-features-lights serial %s %s hide %d max_depth %d rr_depth %d" % (sky, placement, prm.hide_emitters, prm.max_depth, prm.rr_depth)
            assert np.array_equal(bits(film), bits(want["film"])), (what, int((bits(film) != bits(want["film"])).sum()), float(np.abs(film - want["film"]).max()))
            assert film[..., :3].max() > 0
            check_counters(what, st, want["st"], want["tally"], prm.rng_mode, abi)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hide", [0, 1])
def test_f_a_lens_over_a_constant_sky_and_nothing_else_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, monkeypatch, hide):
    """the scene of test_c_a_lens_scene_counts_a_constant_sky_with_its_own_density: the regression case of the randomised sweep's
    finding, film and counters"""
    no_knobs(monkeypatch)
    prm = abi.render_params(spp=8, seed=5, hide_emitters=hide)
    o, g = oracle.scene(sky_box_flat(hostmirror, abi)), abi.Scene(gpu_ctx, sky_box_flat(hostmirror, abi))
    try:
        (ref, rst), t = counted(oracle, lambda: o.render(prm, threads=8))
        film, st = g.render(prm)
    finally:
        g.close(); o.close()
    assert t["sky_own_density"] >= 100, t
    assert np.array_equal(bits(film), bits(ref)), (hide, int((bits(film) != bits(ref)).sum()), float(np.abs(film - ref).max()))
    check_counters("lens over a constant sky, hide %d" % hide, st, (rst.samples, rst.segments), t, prm.rng_mode, abi)


AOV_TYPES = lambda abi: [abi.MSK_AOV_DEPTH, abi.MSK_AOV_POSITION, abi.MSK_AOV_UV, abi.MSK_AOV_GEO_NORMAL, abi.MSK_AOV_SH_NORMAL, abi.MSK_AOV_PATH_RGBA]


@pytest.mark.gpu
@pytest.mark.parametrize("sky", sorted(WP.ALL_SKIES))
def test_g_crop_window_shards_samples_and_aovs(gpu_ctx, hostmirror, oracle, abi, packer_constants, monkeypatch, sky):
    """the all-features lens scene: a crop window; the two sample shards (0, 2) and (1, 2), each against the twin's film of the same
    shard; the samples of every pixel at spp 4; and every "aov" channel, with and without the nested path integrator"""
    no_knobs(monkeypatch)
    crop = (5, 3, 20, 18)
    prm = abi.render_params(spp=8, seed=5, rr_depth=2)
    o, g = PP.open_twin(oracle, packer_constants, all_features_flat(hostmirror, sky, crop=crop)), abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky, crop=crop))
    try:
        film, st = g.render(prm)
        ref, rst = o.render(prm, threads=8)
        assert film.shape == ref.shape == (18, 20, 5) and st.samples == rst.samples
        assert np.array_equal(bits(film), bits(ref)), (sky, int((bits(film) != bits(ref)).sum()))
    finally:
        g.close(); o.close()
    o, g = PP.open_twin(oracle, packer_constants, all_features_flat(hostmirror, sky)), abi.Scene(gpu_ctx, all_features_flat(hostmirror, sky))
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
        prm = abi.render_params(spp=4, seed=5)
        types = AOV_TYPES(abi)
        for t in (types, types[:5]):
            film, st = g.render_aov(prm, t)
            ref, rst = o.render_aov(prm, t, threads=8)
            assert film.shape == ref.shape and st.samples == rst.samples
            for c in range(film.shape[-1]):
                assert np.array_equal(bits(film[..., c]), bits(ref[..., c])), (sky, len(t), c, int((bits(film[..., c]) != bits(ref[..., c])).sum()))
        assert np.abs(ref[..., 5:]).max() > 0
    finally:
        g.close(); o.close()


@pytest.mark.gpu
def test_g_position_aov_of_the_focus_plane_equals_the_twin(gpu_ctx, hostmirror, oracle, abi, monkeypatch):
    """the scene and parameters of test_thinlens.test_position_aov_of_the_focus_plane, which holds the channel's float64 value: every
    channel of that film, bit for bit"""
    no_knobs(monkeypatch)
    flat = TL.with_lens(abi, hostmirror.flatten([TL.emitting_quad(hostmirror, -20.0, 20.0, TL.FOCUS)], 48, 48, camera=TL.Z_CAM), TL.RADIUS, TL.FOCUS)
    prm = abi.render_params(spp=16, seed=9)
    o, g = oracle.scene(flat), abi.Scene(gpu_ctx, flat)
    try:
        film, st = g.render_aov(prm, [abi.MSK_AOV_POSITION, abi.MSK_AOV_DEPTH])
        ref, rst = o.render_aov(prm, [abi.MSK_AOV_POSITION, abi.MSK_AOV_DEPTH], threads=8)
    finally:
        g.close(); o.close()
    assert film.shape == ref.shape == (48, 48, 9) and st.samples == rst.samples
    for c in range(9):
        assert np.array_equal(bits(film[..., c]), bits(ref[..., c])), (c, int((bits(film[..., c]) != bits(ref[..., c])).sum()))
    assert np.all(np.abs(ref[..., 7].astype(np.float64) / ref[..., 4] - TL.FOCUS) <= 2.0 ** -17 * 6.5)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", DIRECT_NM, ids=lambda v: str(v))
@pytest.mark.parametrize("name", ["lens", "pinhole"])
def test_h_direct_with_a_lens_and_delta_lights_equals_the_oracles_direct(gpu_ctx, hostmirror, oracle, abi, monkeypatch, name, n, m):
    """every sample of every pixel, the film and the four counters, through test_direct_oracle_parity's checker"""
    DP.no_knobs(monkeypatch)
    tw = twin_of_direct(oracle, hostmirror, abi, name, n, m)
    g = abi.Scene(gpu_ctx, direct_flats(hostmirror, abi)[name])
    try:
        got = g.sample_pixels_direct(direct_prm(abi), DI.all_pixels(), n, m)
        film, st = g.render_direct(direct_prm(abi), n, m)
    finally:
        g.close()
    what = "%s (%d, %d)" % (name, n, m)
    DP.assert_samples(what, got, tw["samples"])
    DP.assert_film(what, film, st, tw)
    assert st.samples == DI.FW * DI.FH * DIRECT_SPP and (np.nanmax(film[..., :3]) > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("cam", sorted(HOOK_CAMERAS))
def test_i_camera_probe_equals_the_twins_hook(gpu_ctx, hostmirror, oracle, abi, cam):
    pos, u = hook_inputs()
    for lens in HOOK_LENSES + [None]:
        flat = hook_flat(hostmirror, HOOK_CAMERAS[cam], lens)
        o, g = oracle.scene(flat), abi.Scene(gpu_ctx, flat)
        try:
            got, want = g.camera_sample(pos, u), o.camera_sample(pos, u)
        finally:
            g.close(); o.close()
        assert_bits("camera probe", got, want, cam, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", TL.BLUR_DEPTHS)
def test_i_device_samples_follow_their_own_aperture_sample(gpu_ctx, hostmirror, oracle, abi, depth):
    check_each_sample_follows_its_own_aperture_sample(lambda flat: abi.Scene(gpu_ctx, flat), oracle, hostmirror, abi, depth)


@pytest.mark.gpu
def test_i_light_probe_equals_the_twins_hook(gpu_ctx, hostmirror, oracle, abi):
    """g.light_sample against msk_oracle_light_sample on test_spot_directional's probe scenes and points (the inputs on which
    test_plastic_oracle_parity holds the twin's hook to light_ref): both spots, the sun, a cosine exactly on either edge"""
    pos, p, wl = SD.probe_points()
    flat = SD.probe_flat(hostmirror)
    sp_pos, sp_axis, cc, cb = SD.light_of(flat, 2)
    c = LR.spot_cosine32(sp_pos, sp_axis, p)
    f = LR.falloff32(c, cc, cb)
    k = int(np.argmax((f > 0.3) & (f < 0.7)))
    for what, fl in (("as flattened", flat), ("cos_beam = c", SD.probe_flat(hostmirror, (cc, c[k]))), ("cos_cutoff = c", SD.probe_flat(hostmirror, (c[k], cb))),
                     ("a hard edge at c", SD.probe_flat(hostmirror, (c[k], c[k])))):
        o, g = oracle.scene(fl), abi.Scene(gpu_ctx, fl)
        try:
            for e in (2, 3, 4):
                gd, gv = g.light_sample(e, p, wl)
                od, ov = o.light_sample(e, p, wl)
                assert_bits("d, dist", gd, od, what, e)
                assert_bits("value", gv, ov, what, e)
        finally:
            g.close(); o.close()
