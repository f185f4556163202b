"""The `direct` integrator held to the CPU oracle at any (N, M): include/msk_gpu.h at msk_direct_params, DESIGN.md section 9.

`direct_sample` of oracle/oracle.cpp restates the integrator from the header (not from csrc/msk_direct.h).  The CPU layers prove the
restatement against things that share no code with it; the GPU layers then hold k_direct to it bit for bit.

CPU
  a  (1, 1) is the oracle's own `path` at max_depth = 2, bit for bit: samples, positions, films, `samples` — on the anchors of
     test_direct_integrator and on every scene of test_table_placement that holds no NaN.  The documented exception (a `constant` sky
     whose stale next-event record `path` reads) is shown where it exists: see test_a_the_constant_sky_exception.
  b  the float64 closed forms the device is held to, met by the oracle under the rule of test_direct_integrator's docstring (spp
     doubles from 4096 until the standard error is at most 0.5 % of the expectation, four doublings at the most; then
     |mean - E| <= 6 SE + 1e-3 E), and two more at counts where neither strategy dominates: a lamp over a `roughconductor` plane at
     (2, 3) against float64 quadrature, and a lamp plus a `constant` sky over the diffuse plane at (3, 2).
  c  the factors msk_oracle_direct_terms reports, recombined in numpy fp32 one operation at a time in the header's order
     (direct_ref.recombine_f32, direct_ref.weight_f32), equal the oracle's spectral result bit for bit; the pairs it drew are
     direct_ref.pair_layout's and none is drawn twice.
  d  the oracle's direct tallies of every (scene, N, M) the GPU layers render: each named event is reached at least 100 times on the
     scene that is meant to reach it, and never on a scene that cannot produce it.
  e  the oracle refuses what the library refuses.
  plan: which k_direct<form> and tables_mode each GPU case gets, from the library's own host code (tests/native/direct_plan_probe.cpp).

GPU (one context, one process; knobs are set before abi.Scene is created; every comparison is of bits)
  f  the anchors across counts     g  table placements and the inlined emitter code     h  every form of the kernel
  i  the counts' far end           j  the fill loop's edges                              k  shards and the crop window
  l  msk_gpu_render_direct_device
The oracle's results are computed once per (scene, parameters, counts), cached in the module and never changed."""
import ctypes as C
import functools
import os
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import delta_ref as D
import direct_ref as DR
import oracle_binding
import radiometry_ref as R
import test_delta_light_mirror as DM
import test_direct_integrator as DI
import test_envmap as EV
import test_table_placement as TP
from test_table_placement import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FW, FH, BS = DI.FW, DI.FH, DI.BS
ORACLE_THREADS = 16
KNOBS = tuple(DM.KNOBS) + ("MSK_WIDE_LDS", "MSK_STACK_CAP", "MSK_BVH_LEAF", "MSK_COLLAPSE_OPTIMAL", "MSK_PAD_SCALE")
EVENTS = oracle_binding.Oracle.DIRECT_TALLIES[:21]                       # (the delta lights' seven, appended later: test_lens_light_oracle_parity)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def P(**kw):
    """render parameters as a hashable key: abi.render_params(**dict(key))"""
    return tuple(sorted(kw.items()))


def params(abi, key):
    return abi.render_params(**dict(key))


# ===================================================================================================== scenes
def twosided_back_flat(hm):
    """(e) a `twosided` rough conductor wound so that the camera sees its BACK (the adapter flips wi and wo for every sample of every
    hit), under the 4 x 4 lamp and a `constant` sky: two emitters, a glossy p_b on the flipped side"""
    floor = DM.plane(hm, dict(EV.FLOORS["roughconductor"][0], twosided=True), flip=True)
    lamp = hm.MeshSpec("lamp", [tuple(DI.LAMP4)], hm.LUMINAIRE, radiance=(40, 30, 20))
    return hm.flatten([floor, lamp], FW, FH, camera=DI.CAM, env=DM.SKY)


def tables_dropped_meshes(hm):
    """test_table_placement's `_small_staged` with a 224-triangle blob: at MSK_LDS_SCENE_KB=60 the tree is staged in LDS, the small
    tables (988 float4) would be staged by the wavefront kernels, and beside this tree and its stacks they no longer fit 64 KB:
    make_direct_plan drops them (tables_mode 0)"""
    return hm.cbox_meshes() + TP.ceiling_quads(hm, 23, 12, (8, 8, 8), "lamp") + [TP.blob(hm, 15, 8, conductor=True)]


ANCHOR_NAMES = ("a_cbox", "b_mixed", "c_envmap", "d_point_mirror_sky")
CROP = (5, 3, 12, 9)
EXTRA_KB = {"lds_tree__tables_dropped": "60"}


@functools.lru_cache(maxsize=None)
def scene_flat(hm, key):
    if key in ANCHOR_NAMES:
        return DI.anchor_flat(hm, key)
    if key == "a_cbox_crop":
        return hm.cbox_scene(FW, FH, crop=CROP)
    if key == "a_cbox_5x3":
        return hm.cbox_scene(5, 3)
    if key == "e_twosided_back":
        return twosided_back_flat(hm)
    if key == "lds_tree__tables_dropped":
        return hm.flatten(tables_dropped_meshes(hm), TP.W, TP.H)
    return TP._flat(hm, key)


def scene_env(key):
    """the placement knob a scene is created with (test_table_placement.SCENES; the anchors take the defaults)"""
    kb = TP.SCENES[key][0] if key in TP.SCENES else EXTRA_KB.get(key)
    return {} if kb is None else {"MSK_LDS_SCENE_KB": kb}


# ===================================================================================================== the oracle's results, once
_twin = {}


def counted(oracle, fn):
    oracle.direct_tallies()
    out = fn()
    return out, oracle.direct_tallies()


def stats_of(st):
    return (int(st.samples), int(st.segments), int(st.shadow_rays), int(st.invalid_samples))


def twin_film(oracle, hm, abi, key, prm_key, n, m):
    """the oracle's film, counters and direct tallies of one render"""
    k = ("film", key, prm_key, n, m)
    if k not in _twin:
        o = oracle.scene(scene_flat(hm, key))
        try:
            t0 = time.time()
            (film, st), tally = counted(oracle, lambda: o.render_direct(params(abi, prm_key), n, m, threads=ORACLE_THREADS))
        finally:
            o.close()
        film.setflags(write=False)
        _twin[k] = dict(film=film, st=stats_of(st), tally=tally, seconds=time.time() - t0)
    return _twin[k]


def oracle_samples(o, prm, pixels, n, m, threads=ORACLE_THREADS):
    """msk_oracle_sample_pixels_direct is single-threaded and pixels are independent: the listed pixels in parts side by side"""
    pixels = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
    parts = [p for p in np.array_split(np.arange(len(pixels)), min(threads, len(pixels))) if len(p)]
    with ThreadPoolExecutor(len(parts)) as pool:
        out = list(pool.map(lambda idx: o.sample_pixels_direct(prm, pixels[idx], n, m), parts))
    return np.concatenate([x for x, _ in out]), np.concatenate([p for _, p in out])


def twin_samples(oracle, hm, abi, key, prm_key, pixels, n, m):
    pixels = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
    k = ("samples", key, prm_key, pixels.tobytes(), n, m)
    if k not in _twin:
        o = oracle.scene(scene_flat(hm, key))
        try:
            xyz, pos = oracle_samples(o, params(abi, prm_key), pixels, n, m)
        finally:
            o.close()
        xyz.setflags(write=False); pos.setflags(write=False)
        _twin[k] = (xyz, pos)
    return _twin[k]


# ===================================================================================================== what the GPU layers render
COUNTS_F = [(4, 0), (0, 4), (3, 2), (2, 5), (1, 3), (7, 1), (16, 16)]
# the anchors of layer f: (scene, hide_emitters).  (e) is this file's own: no anchor shows a `twosided` entry from behind
SCENES_F = [("a_cbox", 0), ("a_cbox", 1), ("b_mixed", 0), ("c_envmap", 0), ("d_point_mirror_sky", 0), ("e_twosided_back", 0)]
# spp of layer f, chosen so that the oracle alone reaches every meant event 100 times (layer d).  24 x 20 pixels see the Cornell
# box's lamp in 0.4 % of their samples: hiding it 100 times takes 288 spp; everything else is reached at 32
SPP_F = {("a_cbox", 1): 288}


def prm_f(name, hide):
    return P(spp=SPP_F.get((name, hide), 32), seed=11, hide_emitters=hide, block_size=BS)


PRM_G = P(spp=TP.SPP, seed=TP.SEED)
NM_G = (3, 2)
# layer g: scene -> (k_direct<form>, tables_mode), by place_tree / place_tables / make_direct_plan of msk_plan.h.  A tree in HBM
# leaves at most 20 KB of stacks beside the tables, so the scene's own placement stands: all tables (2), the small ones (1) or none (0).
# A tree in LDS takes its whole stack and the tree: `lds_tree__hbm_tables__small_staged` still fits (62976 B), `lds_tree__tables_dropped`
# does not, and make_direct_plan drops its tables to 0.  test_plan_of_every_gpu_case holds this table to the library's host code.
PLAN_G = {
    "cbox": (0, 2),
    "lds_tree__hbm_tables__small_staged": (0, 1),
    "lds_tree__nothing_staged": (0, 0),
    "lds_tree__tables_dropped": (0, 0),
    "hbm_tree__lds_tables": (6, 2),
    "hbm_tree__small_staged": (6, 1),
    "hbm_tree__nothing_staged__long_cdf": (6, 0),
    "hbm_tree__nothing_staged__long_cdf_below_one": (6, 0),
    "many_emitters__997_env_first": (6, 0),
    "many_emitters__1000_env_last": (6, 0),
    "many_materials": (6, 0),
    "small_f4_1024": (6, 1),
    "small_f4_1025": (6, 0),
    "table_f4_2560": (6, 2),
    "table_f4_2561": (6, 1),
}
IDS_G = ["%s-k_direct%d-tables_mode%d" % (k, v[0], v[1]) for k, v in PLAN_G.items()]

# layer h: knob set -> the form it selects (place_tree: MSK_LDS_SCENE_KB=0 keeps the tree in HBM, where the default walk is the
# half-float 4-wide tree = form 6; every other walk of a tree in HBM — binary, 8-wide, full-precision or byte-quantised 4-wide — and the
# 4-wide tree staged in LDS make make_direct_plan take the binary tree in HBM = form 1).  MSK_STACK_CAP=4 leaves four stack entries in
# LDS: the rest of a lane's stack is the overflow array.  MSK_BVH_BUILD=gpu builds the tree on the device; its placement is the default's.
KNOBS_H = [
    ("defaults", {}, 0),
    ("hbm", {"MSK_LDS_SCENE_KB": "0"}, 6),
    ("hbm_binary", {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "0"}, 1),
    ("hbm_wide8", {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "8"}, 1),
    ("hbm_wide4_full", {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "0"}, 1),
    ("hbm_wide4_byte", {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "1"}, 1),
    ("wide4_in_lds", {"MSK_WIDE_LDS": "1"}, 1),
    ("hbm_overflow_stack", {"MSK_LDS_SCENE_KB": "0", "MSK_STACK_CAP": "4"}, 6),
    ("hbm_binary_overflow_stack", {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "0", "MSK_STACK_CAP": "4"}, 1),
    ("hbm_device_built_tree", {"MSK_LDS_SCENE_KB": "0", "MSK_BVH_BUILD": "gpu"}, 6),
]
SCENES_H = {"b_mixed": P(spp=8, seed=3, block_size=BS), "hbm_tree__small_staged": P(spp=4, seed=TP.SEED)}
TABLES_H = {"b_mixed": 2, "hbm_tree__small_staged": 1}
CASES_H = [(s, k) for s in SCENES_H for k in KNOBS_H]
IDS_H = ["%s-%s-k_direct%d" % (s, k[0], k[2]) for s, k in CASES_H]


def gpu_layer_renders():
    """(scene, parameters, N, M) of every film layers f and g render"""
    out = [(name, prm_f(name, hide), n, m) for name, hide in SCENES_F for n, m in COUNTS_F]
    out += [(name, PRM_G) + NM_G for name in PLAN_G]
    return out


# ===================================================================================================== CPU a: (1, 1) is `path` at depth 2
def path_and_direct(oracle, hm, abi, flat, prm, pixels):
    o = oracle.scene(flat)
    try:
        pixels = np.ascontiguousarray(pixels, np.int32)
        parts = [p for p in np.array_split(np.arange(len(pixels)), ORACLE_THREADS) if len(p)]
        with ThreadPoolExecutor(len(parts)) as pool:
            got = list(pool.map(lambda idx: o.sample_pixels(prm, pixels[idx]), parts))
        want, wpos = np.concatenate([x for x, _ in got]), np.concatenate([p for _, p in got])
        xyz, pos = oracle_samples(o, prm, pixels, 1, 1)
        film_p, st_p = o.render(prm, threads=ORACLE_THREADS)
        film_d, st_d = o.render_direct(prm, 1, 1, threads=ORACLE_THREADS)
    finally:
        o.close()
    return (want, wpos, film_p, st_p), (xyz, pos, film_d, st_d)


@pytest.mark.parametrize("name,hide", DI.ANCHORS, ids=lambda v: str(v))
def test_a_one_one_is_the_oracles_path_on_the_anchors(oracle, hostmirror, abi, name, hide):
    prm = abi.render_params(spp=6, seed=11, max_depth=2, rr_depth=5, hide_emitters=hide, block_size=BS)
    (want, wpos, film_p, st_p), (xyz, pos, film_d, st_d) = path_and_direct(oracle, hostmirror, abi, scene_flat(hostmirror, name), prm, DI.all_pixels())
    assert np.array_equal(bits(pos), bits(wpos))
    bad = (bits(xyz) != bits(want)).any(-1)
    assert not bad.any(), (name, hide, int(bad.sum()), np.argwhere(bad)[:4].tolist(), xyz[bad][:3], want[bad][:3])
    assert np.isfinite(want).all() and want.max() > 0
    assert np.array_equal(bits(film_d), bits(film_p)), (name, hide, float(np.abs(film_d - film_p).max()))
    assert st_d.samples == st_p.samples == FW * FH * 6 and st_d.invalid_samples == st_p.invalid_samples


@pytest.mark.parametrize("name", [k for k in TP.SCENES if k not in TP.NAN_SCENES])
def test_a_one_one_is_the_oracles_path_on_the_table_scenes(oracle, hostmirror, abi, name):
    prm = abi.render_params(spp=2, seed=TP.SEED, max_depth=2, rr_depth=5)
    (want, wpos, film_p, st_p), (xyz, pos, film_d, st_d) = path_and_direct(oracle, hostmirror, abi, scene_flat(hostmirror, name), prm, DI.all_pixels(TP.W, TP.H))
    assert np.array_equal(bits(pos), bits(wpos))
    bad = (bits(xyz) != bits(want)).any(-1)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist(), xyz[bad][:3], want[bad][:3])
    assert np.isfinite(want).all() and want.max() > 0
    assert np.array_equal(bits(film_d), bits(film_p)), (name, float(np.abs(film_d - film_p).max()))
    assert st_d.samples == st_p.samples == TP.W * TP.H * 2 and st_d.invalid_samples == st_p.invalid_samples == 0


def lamp_and_sky_scene(hm):
    lamp = hm.MeshSpec("lamp", [tuple(DI.LAMP4)], hm.LUMINAIRE, radiance=(40, 30, 20))
    return hm.flatten([DM.plane(hm), lamp], EV.W48, EV.W48, camera=DI.CAM, env=DM.SKY)


def test_a_the_constant_sky_exception(oracle, hostmirror, abi):
    """The documented exception, where it exists.  `path` weighs a BSDF ray that escapes to a `constant` sky with the density of the
    bounce's stale next-event record (path.cpp:90-95); `direct` always with the sky's own.  With the sky as the ONLY emitter
    (`sky_scene`) the stale record is the sky's own, whose density does not depend on the direction: the two are equal there, on every
    sample (measured: 0 of 16 x 8 samples differ).  With a second emitter (the lamp) the stale record names the lamp whenever the
    light sample chose it: the two differ on samples whose BSDF ray escaped, and are equal on every sample whose BSDF ray hit
    geometry, was not traced, or whose camera ray missed."""
    prm = abi.render_params(spp=8, seed=11, max_depth=2, rr_depth=5)
    (want, _, _, _), (xyz, _, _, _) = path_and_direct(oracle, hostmirror, abi, DI.sky_scene(hostmirror), prm, DI.PROBE)
    assert np.array_equal(bits(xyz), bits(want)) and want.max() > 0
    flat = lamp_and_sky_scene(hostmirror)
    (want, wpos, _, _), (xyz, pos, _, _) = path_and_direct(oracle, hostmirror, abi, flat, prm, DI.PROBE)
    assert np.array_equal(bits(pos), bits(wpos))
    o = oracle.scene(flat)
    try:
        escaped = np.array([[any(b["escaped"] for b in o.direct_terms(prm, px, s, 1, 1)["bsdf"])
                             for s in range(prm.spp)] for px in DI.PROBE])
    finally:
        o.close()
    differ = (bits(xyz) != bits(want)).any(-1)
    print("SKY EXCEPTION: %d of %d samples escaped to the sky, %d of them differ from `path`" % (escaped.sum(), escaped.size, differ.sum()))
    assert differ.any() and not (differ & ~escaped).any()


# ===================================================================================================== CPU b: closed forms
def oracle_mean(oracle, flat, abi, what, expected, n, m, pixels):
    """the rule's procedure (module docstring) through msk_oracle_sample_pixels_direct -> (mean, standard error)"""
    o = oracle.scene(flat)
    try:
        spp = 4096
        for _ in range(5):
            xyz, _ = oracle_samples(o, abi.render_params(spp=spp, seed=7), pixels, n, m)
            v = xyz.reshape(-1, 3).astype(np.float64)
            mean, se = v.mean(0), v.std(0, ddof=1) / np.sqrt(len(v))
            print("DIRECT-ORACLE %s (%d, %d) spp %d: expected %s mean %s se/|E| %s dev/|E| %s" % (what, n, m, spp, expected, mean, se / expected, (mean - expected) / expected))
            if np.all(se <= 5e-3 * expected):
                return mean, se
            spp *= 2
    finally:
        o.close()
    raise AssertionError("the standard error stays above 0.5 %% of the expectation: %s" % (se / expected,))


def meets(mean, se, expected):
    return np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


@pytest.mark.parametrize("n,m", [(4, 0), (0, 4), (3, 2)])
def test_b_area_light_meets_the_closed_form(oracle, hostmirror, abi, n, m):
    flat = DI.lamp_scene(hostmirror)
    expected = DI.lamp_expected(flat.desc, 4)
    mean, se = oracle_mean(oracle, flat, abi, "lamp", expected, n, m, DI.PROBE)
    ok, why = meets(mean, se, expected)
    assert ok, why


def test_b_constant_sky_meets_rho_l(oracle, hostmirror, abi):
    flat = DI.sky_scene(hostmirror)
    expected = R.expected_xyz(D.emitter_spectrum(flat.desc, 0) * DM.rho_over_pi(flat.desc), DM.cie_of(flat.desc)) * np.pi
    mean, se = oracle_mean(oracle, flat, abi, "sky", expected, 2, 2, DI.PROBE)
    ok, why = meets(mean, se, expected)
    assert ok, why


@pytest.mark.parametrize("n", [1, 3])
def test_b_point_light_meets_the_closed_form(oracle, hostmirror, abi, n):
    flat, expected, _ = DM.closed_form_case(hostmirror, "a_plane")
    mean, se = oracle_mean(oracle, flat, abi, "point", expected, n, 0, EV.crop_pixels())
    ok, why = meets(mean, se, expected)
    assert ok, why


def glossy_scene(hm):
    lamp = hm.MeshSpec("lamp", [tuple(DI.LAMP4)], hm.LUMINAIRE, radiance=(40, 30, 20))
    return hm.flatten([DM.plane(hm, EV.FLOORS["roughconductor"][0]), lamp], EV.W48, EV.W48, camera=DI.CAM)


def glossy_expected(desc, m_pixels, k_lamp):
    """float64: the mean over the probed pixels of Le * integral over the lamp's area of f(wi, wo) cos_o cos_l / d^2, f cos_o =
    F(wi.h) D(h) G1(wi) G1(wo) / (4 cos_i) (GGX, isotropic; eta, k and the specular reflectance constant over the wavelengths),
    by a k_lamp x k_lamp Gauss-Legendre rule over the lamp and m_pixels x m_pixels over the pixels"""
    b = desc.bsdfs[0]
    alpha, eta, kk, spec = float(b.alpha_u), float(b.eta.scale), float(b.k.scale), float(b.specular_reflectance.scale)
    o, d, w = DI.probe_rays(desc, m_pixels)
    x = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
    lamp = np.array(DI.LAMP4, np.float64)
    t, wt = R.gauss_legendre(k_lamp, lamp[:, 0].min(), lamp[:, 0].max())
    s, ws = R.gauss_legendre(k_lamp, lamp[:, 2].min(), lamp[:, 2].max())
    lp = np.stack(np.broadcast_arrays(t[:, None], lamp[0, 1], s[None, :]), -1)                   # [k, k, 3]
    wi = -d[..., None, None, :]                                                                  # [m, m, 1, 1, 3]
    v = lp - x[..., None, None, :]
    d2 = (v * v).sum(-1)
    wo = v / np.sqrt(d2)[..., None]
    ci, co = wi[..., 1], wo[..., 1]                                                              # the plane faces +y, the lamp -y
    h = wi + wo
    h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    hz = h[..., 1]
    sin_of = lambda c: np.sqrt(np.maximum(0.0, 1.0 - c * c))
    f_cos = (R.fresnel_conductor((h * wi).sum(-1), eta, kk) * R.ggx_d(sin_of(hz), 0.0, hz, alpha, alpha) *
             R.smith_g1_ggx(sin_of(ci), 0.0, ci, alpha, alpha) * R.smith_g1_ggx(sin_of(co), 0.0, co, alpha, alpha) / (4.0 * ci))
    g = ((f_cos * co / d2) * (wt[:, None] * ws[None, :])).sum((-1, -2))
    return R.expected_xyz(D.emitter_spectrum(desc, 0) * spec, DM.cie_of(desc)) * float((w * g).sum())


def lamp_and_sky_expected(desc, m):
    """rho / pi * (Le * G + L * (pi - G)), G = polygon_irradiance of the lamp: the lamp's own light, and the sky's cosine-weighted
    hemisphere MINUS the part the lamp hides (a shadow ray towards it is occluded, a BSDF ray finds the lamp's front).  The plain sum
    rho / pi * Le * G + rho * L counts the hidden part of the sky: 1.7 % (X, Y) to 3.2 % (Z) too much with this lamp.  -> (E, the plain sum)"""
    o, d, w = DI.probe_rays(desc, m)
    geom = float((w * R.polygon_irradiance(R.hit_plane(o, d, (0, 0, 0), (0, 1, 0)), (0, 1, 0), np.array(DI.LAMP4, np.float64))).sum())
    sky = [i for i in range(desc.n_emitters) if desc.emitters[i].mesh_id < 0]
    lamp = [i for i in range(desc.n_emitters) if desc.emitters[i].mesh_id >= 0]
    assert len(sky) == len(lamp) == 1 and 0 < geom < np.pi
    le, l = D.emitter_spectrum(desc, lamp[0]), D.emitter_spectrum(desc, sky[0])
    s = R.Spectrum(lambda lam: le(lam) * geom + l(lam) * (np.pi - geom), le.breaks + l.breaks) * DM.rho_over_pi(desc)
    plain = R.Spectrum(lambda lam: le(lam) * geom + l(lam) * np.pi, le.breaks + l.breaks) * DM.rho_over_pi(desc)
    return R.expected_xyz(s, DM.cie_of(desc)), R.expected_xyz(plain, DM.cie_of(desc))


def test_b_expectations_have_converged(hostmirror):
    fg = glossy_scene(hostmirror)
    a, b, c = glossy_expected(fg.desc, 4, 48), glossy_expected(fg.desc, 8, 48), glossy_expected(fg.desc, 4, 96)
    assert np.all(a > 0) and np.all(np.abs(a - b) <= 1e-5 * b) and np.all(np.abs(a - c) <= 1e-5 * c), (a, b, c)
    fs = lamp_and_sky_scene(hostmirror)
    e4, e8 = lamp_and_sky_expected(fs.desc, 4)[0], lamp_and_sky_expected(fs.desc, 8)[0]
    assert np.all(e4 > 0) and np.all(np.abs(e4 - e8) <= 1e-5 * e8)
    o, dd, _ = DI.probe_rays(fg.desc)
    assert np.all(np.abs(R.hit_plane(o, dd, (0, 0, 0), (0, 1, 0))[..., [0, 2]]) < 25)              # the probed pixels see the plane


def test_b_glossy_plane_under_the_lamp_meets_the_quadrature(oracle, hostmirror, abi):
    """(2, 3) over a `roughconductor`: p_b is the GGX lobe's density, not cos / pi, and neither strategy dominates"""
    flat = glossy_scene(hostmirror)
    expected = glossy_expected(flat.desc, 4, 48)
    mean, se = oracle_mean(oracle, flat, abi, "glossy lamp", expected, 2, 3, DI.PROBE)
    ok, why = meets(mean, se, expected)
    assert ok, why


def test_b_lamp_and_sky_meet_the_closed_form(oracle, hostmirror, abi):
    """(3, 2) with two emitters: 1 / n_emitters in every density"""
    flat = lamp_and_sky_scene(hostmirror)
    expected, plain = lamp_and_sky_expected(flat.desc, 4)
    mean, se = oracle_mean(oracle, flat, abi, "lamp + sky", expected, 3, 2, DI.PROBE)
    print("DIRECT-ORACLE lamp + sky: the sum that ignores the sky the lamp hides is off by", (plain - expected) / expected)
    ok, why = meets(mean, se, expected)
    assert ok, why


# ===================================================================================================== CPU c: the terms, recombined
# (2, 3): a division by 2 or 4 is exact, so with M a power of two "(t * w_b) / M" and "(t / M) * w_b" are the same bits; M = 3 tells them apart
@pytest.mark.parametrize("n,m", [(3, 2), (1, 4), (5, 0), (2, 3)])
@pytest.mark.parametrize("name", ["b_mixed", "d_point_mirror_sky"])
def test_c_terms_recombined_in_numpy_fp32(oracle, hostmirror, abi, name, n, m):
    prm = abi.render_params(spp=8, seed=11, block_size=BS)
    pixels = DI.all_pixels()[np.random.RandomState(1).permutation(FW * FH)[:64]]
    lay = DR.pair_layout(n, m)
    o = oracle.scene(scene_flat(hostmirror, name))
    seen = dict(hit=0, light=0, shadow=0, visible=0, point=0, reached=0, mis=0)
    try:
        xyz, _ = o.sample_pixels_direct(prm, pixels, n, m)
        for i, px in enumerate(pixels):
            for s in range(prm.spp):
                t = o.direct_terms(prm, px, s, n, m)
                res, shadows = DR.recombine_f32(t, n, m)
                assert np.array_equal(bits(res), bits(t["result"])), (name, n, m, px.tolist(), s, res, t["result"], t)
                assert shadows == [l["shadow"] for l in t["light"]], (name, px.tolist(), s, t["light"])
                # the pairs: a light sample i drew 3 + i, BSDF sample j its lobe from 3 + N + 2 j and its direction from the next
                assert [l["pair"] for l in t["light"]] == lay["light"][:len(t["light"])] and len(t["light"]) in (0, n)
                assert [b["pair_lobe"] for b in t["bsdf"]] == lay["bsdf_lobe"][:len(t["bsdf"])] and len(t["bsdf"]) == (m if t["hit"] else 0)
                assert [b["pair_dir"] for b in t["bsdf"]] == lay["bsdf_direction"][:len(t["bsdf"])]
                assert len(set(t["draws"])) == len(t["draws"]) and set(t["draws"]) <= set(DR.draws(n, m)) - {lay["aperture"]}
                assert t["draws"][:2] == [lay["film"], lay["wavelengths"]]
                if not t["hit"]:
                    assert not t["light"] and not t["bsdf"] and np.array_equal(bits(t["result"]), bits(np.zeros(4, F) + t["emission"]))
                # the sample's XYZ is the spectral result through the ray weight and the colour matching: zero together
                assert ((t["result"] * t["ray_weight"]) != 0).any() or not (xyz[i, s] != 0).any()
                seen["hit"] += t["hit"]; seen["light"] += len(t["light"]); seen["shadow"] += sum(shadows)
                seen["visible"] += sum(l["shadow"] and not l["occluded"] for l in t["light"]); seen["point"] += sum(l["point"] for l in t["light"])
                seen["reached"] += sum(b["reached"] for b in t["bsdf"])
                seen["mis"] += sum(b["reached"] and 0 < DR.weight_f32(m, b["p_b"], n, b["p_e"]) < 1 for b in t["bsdf"])
    finally:
        o.close()
    print("TERMS %s (%d, %d): %s" % (name, n, m, seen))
    # the check is not vacuous: light terms were added on both scenes; BSDF terms on the scene with a sky (a BSDF ray finds the
    # Cornell box's lamp once in two hundred: a handful of the 512 M samples of `b_mixed`), where the count-weighted heuristic decided
    assert seen["hit"] > 100 and (n == 0 or seen["visible"] > 100)
    if name == "d_point_mirror_sky":
        assert (n == 0 or seen["point"] > 50) and (m == 0 or seen["reached"] > 100) and (m == 0 or n == 0 or seen["mis"] > 10)


def test_c_fp32_weight_follows_the_float64_one():
    rng = np.random.RandomState(5)
    for _ in range(2000):
        na, nb = rng.randint(0, 17), rng.randint(0, 17)
        pa, pb = F(rng.uniform(1e-3, 50)), F(rng.uniform(1e-3, 50))
        w32, w64 = DR.weight_f32(na, pa, nb, pb), float(DR.weight(na, float(pa), nb, float(pb)))
        # u = 2^-24 per rounding: n p carries u, its square 3 u, the sum of the squares 4 u, the quotient 3 u + 4 u + u
        assert w32.dtype == F and abs(float(w32) - w64) <= 8 * 2.0 ** -24 * max(w64, 2.0 ** -126), (na, pa, nb, pb, w32, w64)
    assert DR.weight_f32(3, F(0), 2, F(1)) == 0 and DR.weight_f32(3, F(2), 0, F(1)) == 1
    # with (1, 1) every product by the count is exact: the weight is path's mis_weight
    pa, pb = F(0.3), F(1.7)
    assert DR.weight_f32(1, pa, 1, pb) == F(F(pa * pa) / F(F(pa * pa) + F(pb * pb)))


# ===================================================================================================== CPU d: coverage
# event -> the scene of the GPU layers that is meant to reach it (at least 100 times in ONE of its renders)
HOME = {
    "primary_miss_env": "c_envmap", "primary_emitter_seen": "hbm_tree__nothing_staged__long_cdf", "primary_emitter_hidden": ("a_cbox", 1), "twosided_flipped": "e_twosided_back",
    "light_skipped_delta": "b_mixed", "light_area_visible": "a_cbox", "light_area_occluded": "a_cbox", "light_area_back": "a_cbox",
    "light_constant_sky": "d_point_mirror_sky", "light_image": "c_envmap", "light_point_visible": "d_point_mirror_sky",
    "light_point_occluded": "d_point_mirror_sky", "light_last_emitter": "many_emitters__1000_env_last", "bsdf_not_traced": "b_mixed",
    "bsdf_emitter_front_mis": "a_cbox", "bsdf_emitter_back": "many_emitters__997_env_first", "bsdf_non_emitter": "a_cbox", "bsdf_miss_image": "c_envmap",
    "bsdf_miss_constant": "d_point_mirror_sky", "bsdf_miss_nothing": "a_cbox", "bsdf_emitter_after_delta": "d_point_mirror_sky",
}
NO_SKY = {"primary_miss_env", "light_constant_sky", "light_image", "bsdf_miss_image", "bsdf_miss_constant"}
NO_POINT = {"light_point_visible", "light_point_occluded"}
ONE_EMITTER = {"light_last_emitter"}
NO_DELTA = {"light_skipped_delta", "bsdf_emitter_after_delta"}
NO_TWOSIDED = {"twosided_flipped"}


def cannot(name, hide):
    """what a scene cannot produce at all.  The table-placement family: a closed or open Cornell box, area emitters only (the two
    `many_emitters` scenes add a `constant` sky), no point light, no delta BSDF; its `twosided` entries are seen from the front or
    not at all"""
    out = set() if hide else {"primary_emitter_hidden"}
    if name in ("a_cbox", "cbox", "hbm_tree__lds_tables"):
        out |= NO_SKY | NO_POINT | ONE_EMITTER | NO_DELTA | NO_TWOSIDED
    elif name == "b_mixed":
        out |= NO_SKY | NO_POINT | ONE_EMITTER
    elif name == "c_envmap":
        out |= NO_POINT | {"light_constant_sky", "bsdf_miss_constant", "bsdf_miss_nothing"}
    elif name == "d_point_mirror_sky":
        out |= {"light_image", "bsdf_miss_image", "bsdf_miss_nothing"}
    elif name == "e_twosided_back":
        out |= NO_POINT | NO_DELTA | {"light_image", "bsdf_miss_image", "bsdf_miss_nothing"}
    elif name.startswith("many_emitters"):
        out |= NO_POINT | NO_DELTA | {"light_image", "bsdf_miss_image", "bsdf_miss_nothing"}
    else:
        out |= NO_SKY | NO_POINT | NO_DELTA
    return out


def test_d_the_gpu_layers_renders_reach_every_branch(oracle, hostmirror, abi):
    assert set(HOME) == set(EVENTS)
    best = {e: 0 for e in EVENTS}
    t0 = time.time()
    for name, prm_key, n, m in gpu_layer_renders():
        tw = twin_film(oracle, hostmirror, abi, name, prm_key, n, m)
        hide = dict(prm_key).get("hide_emitters", 0)
        print("TALLY direct %s hide %d (%d, %d) spp %d [%.2f s]: %s" % (name, hide, n, m, dict(prm_key)["spp"], tw["seconds"], {k: v for k, v in tw["tally"].items() if v}))
        for e in sorted(cannot(name, hide)):
            assert tw["tally"][e] == 0, (name, hide, n, m, e, tw["tally"])
        for e, home in HOME.items():
            if home == name or home == (name, hide):
                best[e] = max(best[e], tw["tally"][e])
    print("TALLY direct: the most each event is reached in one render of its scene: %s; all oracle films %.1f s" % (best, time.time() - t0))
    for e in EVENTS:
        assert best[e] >= 100, (e, best)


# ===================================================================================================== CPU e: refusals
def test_e_the_oracle_refuses_what_the_library_refuses(oracle, hostmirror, abi):
    import test_mask_bsdf as MB
    o = oracle.scene(scene_flat(hostmirror, "a_cbox"))
    try:
        ok = abi.render_params(spp=1, seed=1, block_size=BS)
        for call in (lambda: o.render_direct(EV.pcg(abi, spp=1), 1, 1), lambda: o.sample_pixels_direct(EV.pcg(abi, spp=1), DI.VAR_PIXELS, 1, 1),
                     lambda: o.direct_terms(EV.pcg(abi, spp=1), (3, 3), 0, 1, 1),
                     lambda: o.render_direct(ok, 0, 0), lambda: o.sample_pixels_direct(ok, DI.VAR_PIXELS, 0, 0),
                     lambda: o.render_direct(ok, 4097, 1), lambda: o.render_direct(ok, 1, 4097), lambda: o.sample_pixels_direct(ok, DI.VAR_PIXELS, 1, 4097),
                     lambda: o.direct_terms(ok, (3, 3), 0, 4097, 0)):
            with pytest.raises(ValueError):
                call()
        film, st = o.render_direct(abi.render_params(spp=1, seed=1, block_size=BS, rr_depth=1, max_depth=0), 4096, 0)      # the far end is taken; depths are ignored
        film2, _ = o.render_direct(ok, 4096, 0)
        assert st.samples == FW * FH and film[..., :3].max() > 0 and np.array_equal(bits(film), bits(film2))
    finally:
        o.close()
    m = oracle.scene(MB.variant_flat(hostmirror, "lds"))
    try:
        with pytest.raises(ValueError):
            m.render_direct(ok, 1, 1)
        with pytest.raises(ValueError):
            m.sample_pixels_direct(ok, [(1, 1)], 1, 1)
    finally:
        m.close()


# ===================================================================================================== CPU: the plan of every GPU case
@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    """tests/native/direct_plan_probe.cpp as a shared library: (flat, N, M, records, knobs) -> dict of the DirectPlan"""
    so = str(tmp_path_factory.mktemp("direct_plan_probe") / "direct_plan_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(ROOT, "tests", "native", "direct_plan_probe.cpp")])
    lib = C.CDLL(so)

    def probe(monkeypatch, flat, n, m, records, env):
        no_knobs(monkeypatch, **env)
        out, msg = (C.c_int64 * 10)(), C.create_string_buffer(512)
        rc = lib.direct_plan_probe(C.byref(flat.desc), None, n, m, C.c_uint64(records), out, msg, 512)
        assert rc == 0, msg.value
        return dict(zip(("form", "tables_mode", "trace_mode", "stack_entries", "ovf_entries", "lds_bytes", "nodes", "depth", "staged_bytes", "records_per_wave"), out))
    return probe


def no_knobs(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_plan_of_every_gpu_case(plan_probe, hostmirror, monkeypatch):
    """PLAN_G, KNOBS_H and TABLES_H against place_tree / place_tables / make_direct_plan run on the scenes themselves; every form,
    every tables_mode, the overflow stack under both trees and the dropped tables are among the cases"""
    seen = set()
    for name, (form, mode) in PLAN_G.items():
        flat = scene_flat(hostmirror, name)
        p = plan_probe(monkeypatch, flat, NM_G[0], NM_G[1], TP.W * TP.H * TP.SPP, scene_env(name))
        print("PLAN g %s: %s" % (name, p))
        assert (p["form"], p["tables_mode"]) == (form, mode), (name, p)
        assert p["lds_bytes"] <= 64 * 1024
        tp = TP.table_plan(flat)
        own = 2 if tp["lds_tables"] else 1 if tp["small_staged"] else 0
        assert mode == own or (name == "lds_tree__tables_dropped" and (own, mode, form) == (1, 0, 0) and p["staged_bytes"] > 0)
        seen.add((form, mode))
    assert {m for _, m in seen} == {0, 1, 2} and {f for f, _ in seen} == {0, 6}
    forms = set()
    for (scene, (tag, env, form)) in CASES_H:
        p = plan_probe(monkeypatch, scene_flat(hostmirror, scene), 3, 2, 1 << 12, {k: v for k, v in env.items() if k != "MSK_BVH_BUILD"})
        print("PLAN h %s %s: %s" % (scene, tag, p))
        assert (p["form"], p["tables_mode"]) == (form, TABLES_H[scene]), (scene, tag, p)
        assert "overflow" not in tag or (p["stack_entries"] == 4 and p["ovf_entries"] > 0), (scene, tag, p)
        forms.add(form)
    assert forms == {0, 6, 1}


# ===================================================================================================== GPU
def open_scene(abi, gpu_ctx, hm, monkeypatch, key, **env):
    no_knobs(monkeypatch, **dict(scene_env(key), **env))
    return abi.Scene(gpu_ctx, scene_flat(hm, key))


def assert_samples(what, got, want):
    (gx, gp), (wx, wp) = got, want
    assert gx.shape == wx.shape and np.array_equal(bits(gp), bits(wp)), what
    bad = [i for i in range(len(gx)) if not same(gx[i], wx[i])]
    assert not bad, (what, len(bad), bad[:6], gx[bad[0]][:3], wx[bad[0]][:3])


def assert_film(what, film, st, tw):
    assert same(film, tw["film"]), (what, int((bits(film) != bits(tw["film"])).sum()), float(np.nanmax(np.abs(film - tw["film"]))))
    assert stats_of(st) == tw["st"], (what, stats_of(st), tw["st"])


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", COUNTS_F, ids=lambda v: str(v))
@pytest.mark.parametrize("name,hide", SCENES_F, ids=lambda v: str(v))
def test_f_anchors_across_counts(gpu_ctx, hostmirror, oracle, abi, monkeypatch, name, hide, n, m):
    """every sample of every pixel, the film and the four counters against the oracle's"""
    key = prm_f(name, hide)
    tw = twin_film(oracle, hostmirror, abi, name, key, n, m)
    want = twin_samples(oracle, hostmirror, abi, name, key, DI.all_pixels(), n, m)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, name)
    try:
        got = g.sample_pixels_direct(params(abi, key), DI.all_pixels(), n, m)
        film, st = g.render_direct(params(abi, key), n, m)
    finally:
        g.close()
    what = "%s hide %d (%d, %d)" % (name, hide, n, m)
    assert_samples(what, got, want)
    assert_film(what, film, st, tw)
    assert np.nanmax(film[..., :3]) > 0 and st.samples == FW * FH * dict(key)["spp"]


def pixels_g(hm, abi, oracle, name):
    if name in TP.SCENES:
        return TP.pick_pixels(hm, abi, oracle, name)[0]
    return DI.all_pixels(TP.W, TP.H)[np.random.RandomState(7).permutation(TP.W * TP.H)[:40]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLAN_G), ids=IDS_G)
def test_g_table_placements(gpu_ctx, hostmirror, oracle, abi, monkeypatch, name):
    """every placement of the shading tables under k_direct, with the long CDF, the zero-area faces and lamps, the selection clamp at
    997 / 1000 emitters and 310 materials through its inlined emitter code"""
    n, m = NM_G
    tw = twin_film(oracle, hostmirror, abi, name, PRM_G, n, m)
    pixels = pixels_g(hostmirror, abi, oracle, name)
    assert len(pixels) == 40
    want = twin_samples(oracle, hostmirror, abi, name, PRM_G, pixels, n, m)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, name)
    try:
        got = g.sample_pixels_direct(params(abi, PRM_G), pixels, n, m)
        film, st = g.render_direct(params(abi, PRM_G), n, m)
    finally:
        g.close()
    assert_samples(name, got, want)
    assert_film(name, film, st, tw)
    assert np.nanmax(film[..., :3]) > 0


def test_g_every_tables_mode_is_in_the_family():
    assert {v[1] for v in PLAN_G.values()} == {0, 1, 2} and set(TP.SCENES) <= set(PLAN_G)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,knobs", CASES_H, ids=IDS_H)
def test_h_every_form_of_the_kernel(gpu_ctx, hostmirror, oracle, abi, monkeypatch, scene, knobs):
    tag, env, form = knobs
    key = SCENES_H[scene]
    film_size = (FW, FH) if scene == "b_mixed" else (TP.W, TP.H)
    pixels = DI.all_pixels(*film_size)[::7]
    tw = twin_film(oracle, hostmirror, abi, scene, key, 3, 2)
    want = twin_samples(oracle, hostmirror, abi, scene, key, pixels, 3, 2)
    no_knobs(monkeypatch, **env)
    g = abi.Scene(gpu_ctx, scene_flat(hostmirror, scene))
    try:
        got = g.sample_pixels_direct(params(abi, key), pixels, 3, 2)
        film, st = g.render_direct(params(abi, key), 3, 2)
    finally:
        g.close()
    what = "%s %s k_direct<%d>" % (scene, tag, form)
    assert_samples(what, got, want)
    assert_film(what, film, st, tw)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(4096, 4096), (1000, 3)], ids=lambda v: str(v))
def test_i_far_end_samples(gpu_ctx, hostmirror, oracle, abi, monkeypatch, n, m):
    """the 16 pixels of test_direct_integrator.VAR_PIXELS (its PROBE lies outside a 24 x 20 film), 2 spp"""
    key = P(spp=2, seed=13, block_size=BS)
    want = twin_samples(oracle, hostmirror, abi, "a_cbox", key, DI.VAR_PIXELS, n, m)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "a_cbox")
    try:
        got = g.sample_pixels_direct(params(abi, key), DI.VAR_PIXELS, n, m)
    finally:
        g.close()
    assert_samples("(%d, %d)" % (n, m), got, want)
    assert got[0].min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(4096, 1), (1, 4096)], ids=lambda v: str(v))
def test_i_far_end_films(gpu_ctx, hostmirror, oracle, abi, monkeypatch, n, m):
    key = P(spp=1, seed=13, block_size=BS)
    tw = twin_film(oracle, hostmirror, abi, "a_cbox", key, n, m)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "a_cbox")
    try:
        film, st = g.render_direct(params(abi, key), n, m)
    finally:
        g.close()
    assert_film("(%d, %d)" % (n, m), film, st, tw)
    assert film[..., :3].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 3, 64, 65])
def test_j_one_pixel(gpu_ctx, hostmirror, oracle, abi, monkeypatch, spp):
    """fewer records than lanes, exactly a wave, one more than a wave"""
    key = P(spp=spp, seed=17, block_size=BS)
    px = [(10, 12)]
    want = twin_samples(oracle, hostmirror, abi, "b_mixed", key, px, 3, 2)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "b_mixed")
    try:
        got = g.sample_pixels_direct(params(abi, key), px, 3, 2)
    finally:
        g.close()
    assert got[0].shape == (1, spp, 3)
    assert_samples("one pixel, spp %d" % spp, got, want)


@pytest.mark.gpu
def test_j_every_camera_ray_misses(gpu_ctx, hostmirror, oracle, abi, monkeypatch):
    """pixels of `c_envmap` whose every sample leaves the scene: no lane ever holds a hit, every lane keeps drawing until the range is
    empty and each record is the environment's radiance"""
    key = P(spp=40, seed=19, block_size=BS)
    prm = params(abi, key)
    o = oracle.scene(scene_flat(hostmirror, "c_envmap"))
    try:
        misses = [px for px in DI.all_pixels().tolist() if not any(o.direct_terms(prm, px, s, 2, 2)["hit"] for s in range(prm.spp))]
    finally:
        o.close()
    assert len(misses) >= 100, len(misses)
    misses = misses[:100]                                        # 4000 records: 62 waves and a partial one
    want = twin_samples(oracle, hostmirror, abi, "c_envmap", key, misses, 2, 2)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "c_envmap")
    try:
        got = g.sample_pixels_direct(prm, misses, 2, 2)
    finally:
        g.close()
    assert_samples("all misses", got, want)
    assert got[0].max() > 0


@pytest.mark.gpu
def test_j_a_film_of_fifteen_pixels(gpu_ctx, hostmirror, oracle, abi, monkeypatch):
    key = P(spp=1, seed=23, block_size=BS)
    tw = twin_film(oracle, hostmirror, abi, "a_cbox_5x3", key, 3, 2)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "a_cbox_5x3")
    try:
        film, st = g.render_direct(params(abi, key), 3, 2)
    finally:
        g.close()
    assert film.shape == (3, 5, 5) and st.samples == 15
    assert_film("5 x 3 x 1 spp", film, st, tw)


SHARDS_K = [dict(sample_first=0, sample_stride=2), dict(sample_first=1, sample_stride=2), dict(sample_first=2, sample_stride=3), dict(block_first=1, block_stride=2)]


@pytest.mark.gpu
@pytest.mark.parametrize("shard", SHARDS_K, ids=lambda d: "-".join("%s%d" % (k.split("_")[0][0] + k.split("_")[1][0], v) for k, v in d.items()))
def test_k_shards(gpu_ctx, hostmirror, oracle, abi, monkeypatch, shard):
    """each shard's film against the oracle's film of the same shard"""
    key = P(spp=7, seed=9, block_size=BS, **shard)
    tw = twin_film(oracle, hostmirror, abi, "a_cbox", key, 2, 2)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "a_cbox")
    try:
        film, st = g.render_direct(params(abi, key), 2, 2)
    finally:
        g.close()
    assert_film(str(shard), film, st, tw)
    assert 0 < st.samples < FW * FH * 7 and film[..., :3].max() > 0


@pytest.mark.gpu
def test_k_crop_window_and_sharded_samples(gpu_ctx, hostmirror, oracle, abi, monkeypatch):
    key = P(spp=4, seed=9, block_size=BS)
    tw = twin_film(oracle, hostmirror, abi, "a_cbox_crop", key, 2, 2)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "a_cbox_crop")
    try:
        window, st = g.render_direct(params(abi, key), 2, 2)
    finally:
        g.close()
    assert window.shape == (CROP[3], CROP[2], 5) and tw["film"].shape == window.shape
    assert_film("crop window", window, st, tw)
    assert window[..., :3].max() > 0
    key = P(spp=7, seed=9, sample_first=1, sample_stride=2)
    want = twin_samples(oracle, hostmirror, abi, "a_cbox", key, DI.all_pixels(), 2, 2)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "a_cbox")
    try:
        got = g.sample_pixels_direct(params(abi, key), DI.all_pixels(), 2, 2)
    finally:
        g.close()
    assert got[0].shape[1] == 3
    assert_samples("samples of shard (1, 2)", got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("stream", ["library_stream", "torch_stream"])
def test_l_render_direct_device(gpu_ctx, hostmirror, oracle, abi, monkeypatch, stream):
    """the film left in a torch tensor on the device, rendered on the library's stream and on a torch stream of its own"""
    import torch
    key = P(spp=8, seed=3, block_size=BS)
    tw = twin_film(oracle, hostmirror, abi, "b_mixed", key, 3, 2)
    g = open_scene(abi, gpu_ctx, hostmirror, monkeypatch, "b_mixed")
    try:
        host, hst = g.render_direct(params(abi, key), 3, 2)
        dev = torch.full((FH, FW, 5), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device="cuda:0") if stream == "torch_stream" else None
        st = g.render_direct_device(params(abi, key), dev.data_ptr(), 3, 2, stream=s.cuda_stream if s is not None else None)
        back = dev.cpu().numpy()
    finally:
        g.close()
    assert np.array_equal(bits(back), bits(host)) and stats_of(st) == stats_of(hst)
    assert_film("render_direct_device, %s" % stream, back, st, tw)
