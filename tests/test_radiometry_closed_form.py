"""Rendered radiance against float64 closed forms, at sample counts that resolve 1e-3.

Every other GPU test asks whether the HIP path produces the oracle's bits; an error the kernels and the oracle SHARE (a 1 % slip
in an MIS weight, in pdf_emitter_direct, in the Russian-roulette compensation, in a 1/pi, in the wavelength weights) moves both
and passes all of them.  Here the operation under test is the integral: each scenario has an expectation that
tests/radiometry_ref.py evaluates in float64 from textbook radiometry and the reference's formulas, and the Monte-Carlo mean of
`sample_pixels` (every sample's XYZ, unsplatted, summed in float64 on the host) is held to it, from the same code on the CPU
oracle (unmarked) and on the device (`gpu`).

    S1  an emitter seen directly (max_depth 1): wavelength sampling, its weights, spectrum_to_xyz, in absolute terms
    S2  direct lighting of a diffuse plane (max_depth 2) against Lambert's polygon formula: NEE + BSDF sampling under MIS,
        pdf_emitter_direct, the face distribution, emitter selection, 1/pi, the spectral product
    S3  furnaces: the throughput recursion, Russian roulette, occlusion, two-sided walls, tabulated rho and Le
    S4  a plate alone in a uniform environment: L_o = albedo(wi); diffuse, and rough conductors against a quadrature of
        F D G / (4 cos_i)
    S5  the film end to end: sum(XYZ) / sum(W) of rendered furnace films, counter RNG and MSK_RNG_PCG_BLOCK

Tolerance of every comparison (derived, with one measured input):

    tol = Z * 1.1 * sigma / sqrt(N) + q + R * |E|          (+ n * 2^-24 * |E| for the fp32 film of S5)

  sigma  the per-sample standard deviation of that scenario, group of pixels and channel, measured on the CPU oracle with
         >= 2^20 samples by tests/golden/make_radiometry_sigma.py (tests/golden/radiometry_sigma.json); 1.1 covers its own
         estimation error.  Neither side computes its own spread to decide whether it passes.
  Z = 5  two-sided normal tail 5.7e-7 per comparison; the seeds are fixed.
  q      |E(m) - E(2m)| of the quadratures behind E, asserted <= 1e-6 |E|.
  R      2e-5: fp32 rounding inside one sample.  The value a sample returns is a sum of a few contributions, each a product
         chain: wavelength weight and spectrum evaluation (~20 rounded operations), per bounce the BSDF weight times the
         throughput and the roulette division (~6 on the chain; the directions, the intersection and the pdfs feed it through
         ~40 more), the emitter pdf and MIS weight of the last vertex (~30), spectrum_to_xyz (~10).  The deepest scenario
         (rho 0.8 furnace, unbounded depth) has a mean path length of five bounces: ~300 dependent operations at a unit
         roundoff of 6e-8 gives 2e-5 as a worst case with every error of one sign; the errors of different samples are not
         correlated, so the mean sees far less.
  N      follows from sigma: the smallest count at which the statistical term fits under the cap, rounded up to whole calls.

THE CAP, asserted before the deviation so that a loose tolerance cannot hide a failure: tol <= 1e-3 |E| for Y on the device,
5e-3 |E| on the CPU oracle, twice that for X and Z.  Exactly-zero cases assert == 0.

Out of scope, because the estimator as the reference writes it has no closed form: `sample_visible=True` and `roughdielectric`
(their sample() weights are not f cos / pdf: tests/test_rough_dielectric.py documents both), and an area light together with an
environment (integrators/path.cpp:86,104-107 reuses the record of the light sample for the MIS weight of an environment hit).

A finding, pinned as written: an ANISOTROPIC rough conductor does not reflect its albedo.  render/microfacet.h:23-26 samples the
half vector's azimuth with the ratio alpha_u / alpha_v inverted, so sample()'s pdf is not the density it draws from (BSDF
sampling alone returns 0.648 where the albedo is 0.573 at alpha (0.15, 0.5), cos_i 0.5); under MIS with the environment 0.7 %
is left.  The oracle and the kernels restate the reference, so the product is kept and S4's anisotropic case holds both to the
closed form of the estimator as written (radiometry_ref.ggx_conductor_as_written), which is the albedo when alpha_u == alpha_v.

S5 on the device cannot reach its cap with one 64 spp film (921 600 samples, sigma / mean 0.35 in Y: 2e-3), so on both sides
films of consecutive seeds are summed in float64 until N is large enough; every film is 128 x 128 at 64 spp as rendered.
"""
import ctypes as C
import json
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import radiometry_ref as R
from ideal_spectra import ideal_fetch

HERE = os.path.dirname(os.path.abspath(__file__))
SIGMA_PATH = os.path.join(HERE, "golden", "radiometry_sigma.json")

Z, SIGMA_SLACK, R_FP32, Q_MAX = 5.0, 1.1, 2e-5, 1e-6
CAP_GPU = np.array([2e-3, 1e-3, 2e-3])
CAP_CPU = np.array([1e-2, 5e-3, 1e-2])
THREADS = 16


# ----------------------------------------------------------------------------- scene pieces
def quad(c, u, v):
    """A quad centred at c spanned by +-u, +-v; its front (the side of the winding's normal) faces u x v"""
    c, u, v = (np.asarray(a, np.float64) for a in (c, u, v))
    return tuple(tuple(float(x) for x in p) for p in (c - u - v, c + u - v, c + u + v, c - u + v))


def room(hm, lo, hi, rho, radiance, bsdf=None):
    """Six inward-facing walls of the box lo .. hi, one mesh (and one emitter) each"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    ex, ey, ez = np.diag(h)
    walls = [("floor", c - ey, ez, ex), ("ceiling", c + ey, ex, ez), ("left", c - ex, ey, ez), ("right", c + ex, ez, ey),
             ("front", c - ez, ex, ey), ("back", c + ez, ey, ex)]
    return [hm.MeshSpec(n, [quad(p, u, v)], rho, radiance=radiance, bsdf=dict(bsdf) if bsdf else None) for n, p, u, v in walls]


def tables(desc):
    cie = np.ctypeslib.as_array(desc.cie1931_xyz, (3 * R.CIE_SAMPLES,)).astype(np.float64)
    d65 = np.ctypeslib.as_array(desc.d65, (R.CIE_SAMPLES,)).astype(np.float64)
    return cie, d65


def as_spectrum(x):
    """The float64 spectrum of what the scene was given: a scalar (`uniform`) or a hostmirror.Regular table"""
    return R.constant(x) if np.isscalar(x) else R.regular(x.lambda_min, x.lambda_max, x.values)


class Case:
    """flat scene, integrator settings, pixels, groups of pixels that share one expectation, expected(fine) -> float64[G, 3]"""

    def __init__(self, flat, pixels, expected, params=None, pooled=False, film=False):
        self.flat, self.expected, self.params, self.film = flat, expected, dict(params or {}), film
        self.pixels = np.asarray(pixels, np.int32).reshape(-1, 2)
        self.groups = [np.arange(len(self.pixels))] if pooled else [np.array([i]) for i in range(len(self.pixels))]


def grid(m, fine):
    return 2 * m if fine else m


# ----------------------------------------------------------------------------- S1
S1_CAMERA = dict(fov=40.0, near=0.01, far=100.0, origin=(0, 0, 0), target=(0, 0, 1), up=(0, 1, 0))
S1_RADIANCE = {"constant": ("regular", (360, 830, [0.7, 0.7])), "table": ("regular", (360, 830, [0.2, 1.0, 0.4, 1.6, 0.8, 0.1])),
               "srgb_d65": ("rgb", (0.9, 0.5, 0.2))}


def s1_flat(hm, kind, facing=True):
    typ, arg = S1_RADIANCE[kind]
    rad = hm.Regular(*arg) if typ == "regular" else arg
    u, v = ((0, 10, 0), (10, 0, 0)) if facing else ((10, 0, 0), (0, 10, 0))
    light = hm.MeshSpec("light", [quad((0, 0, 4), u, v)], 0.0, radiance=rad)
    return hm.flatten([light], 32, 32, camera=S1_CAMERA), rad


def s1(kind):
    def build(hm):
        flat, rad = s1_flat(hm, kind)
        cie, d65 = tables(flat.desc)
        if isinstance(rad, hm.Regular):
            spec = as_spectrum(rad)
        else:
            e = flat.desc.emitters[0]
            spec = R.srgb_d65(e.radiance[:], d65, e.d65_scale)
        return Case(flat, [(3, 4), (16, 16), (28, 9), (12, 30)], lambda fine: R.expected_xyz(spec, cie, grid(8, fine))[None],
                    dict(max_depth=1), pooled=True)
    return build


# ----------------------------------------------------------------------------- S2
S2_CAMERA = dict(fov=40.0, near=0.01, far=1000.0, origin=(0, 3, -8), target=(0, 0, 0), up=(0, 1, 0))
S2_PIXELS = [(128, 160), (80, 208), (180, 120), (128, 36)]      # the last one looks 19 units down the plane: the lights are 12 degrees up


def s2(lights, rho=0.6):
    """lights: [(faces, radiance)] with hostmirror.Regular radiances; rho: scalar or (lambda_min, lambda_max, values)"""
    def build(hm):
        rho_ = rho if np.isscalar(rho) else hm.Regular(*rho)
        meshes = [hm.MeshSpec("plane", [quad((0, 0, 0), (0, 0, 60), (60, 0, 0))], rho_)]
        rads = []
        for i, (faces, rad) in enumerate(lights):
            rads.append(hm.Regular(*rad))
            meshes.append(hm.MeshSpec("light%d" % i, faces, 0.0, radiance=rads[-1]))
        flat = hm.flatten(meshes, 256, 256, camera=S2_CAMERA)
        cie, _ = tables(flat.desc)
        up = np.array([0.0, 1.0, 0.0])

        def form_factor(o, d, faces):
            assert np.all(d[..., 1] < 0) and o[1] < min(p[1] for f in faces for p in f)      # no camera ray meets a light
            x = R.hit_plane(o, d, (0, 0, 0), up)
            assert np.abs(x).max() < 60
            total = 0.0
            for f in faces:
                v = np.asarray(f, np.float64)
                assert np.all((x - v[0]) @ np.cross(v[1] - v[0], v[2] - v[0]) > 0)           # one-sided: the receiver sees its front
                total = total + R.polygon_irradiance(x, up, v)
            return total

        def expected(fine):
            out = np.zeros((len(S2_PIXELS), 3))
            for (faces, _), rad in zip(lights, rads):
                xyz = R.expected_xyz(as_spectrum(rho_) * as_spectrum(rad), cie, grid(8, fine))
                for i, (px, py) in enumerate(S2_PIXELS):
                    out[i] += R.pixel_mean(lambda o, d: form_factor(o, d, faces), flat.desc, px, py, grid(32, fine)) / np.pi * xyz
            return out
        return Case(flat, S2_PIXELS, expected, dict(max_depth=2))
    return build


def _tri(p, a):
    p = np.asarray(p, np.float64)
    return (tuple(p), tuple(p + (a, 0, 0)), tuple(p + (0, 0, a)))       # faces down (x cross z = -y)


_c40, _s40 = np.cos(np.radians(40.0)), np.sin(np.radians(40.0))
ONE = (360, 830, [1.0, 1.0])
S2_CASES = {
    "one_quad": s2([([quad((0, 4, 0), (1, 0, 0), (0, 0, 1))], ONE)]),
    "tilted_40": s2([([quad((1, 4, 0), (_c40, _s40, 0), (0, 0, 1))], ONE)]),
    "faces_1_10_100": s2([([_tri((-3, 4, -3), 0.4), _tri((-2, 4, 0), 0.4 * np.sqrt(10.0)), _tri((0, 4, -2), 4.0)], ONE)]),
    "two_lights": s2([([quad((-2, 4, 0), (1, 0, 0), (0, 0, 1))], ONE),
                      ([quad((3, 5, 2), (0.5, 0, 0), (0, 0, 0.5))], (360, 830, [3.0, 3.0]))]),
    "spectral_product": s2([([quad((0, 4, 0), (1, 0, 0), (0, 0, 1))], (360, 830, [0.5, 1.0, 2.0, 1.5]))],
                           rho=(360, 830, [0.2, 0.5, 0.8, 0.6, 0.3])),
}


# ----------------------------------------------------------------------------- S3
S3_CAMERA = dict(fov=70.0, near=0.01, far=100.0, origin=(0.3, -0.2, -0.6), target=(0.1, 0.0, 1.0), up=(0, 1, 0))
S3_PIXELS = [(0, 0), (15, 2), (7, 8), (3, 13), (12, 12), (9, 4), (1, 7), (14, 15)]
CBOX_INSIDE = dict(fov=60.0, near=1.0, far=2800.0, origin=(278, 273, 20), target=(278, 273, 21), up=(0, 1, 0))


def s3_meshes(hm, rho, le, boxes=False, twosided=False):
    rad = hm.Regular(*le)
    rho_ = rho if np.isscalar(rho) else hm.Regular(*rho)
    bsdf = {"type": "diffuse", "twosided": True} if twosided else None
    if not boxes:
        return room(hm, (-1, -1, -1), (1, 1, 1), rho_, rad, bsdf)
    inner = hm.cbox_meshes()[6:8]                 # the Cornell box's two boxes (no bottoms: they stand on the floor)
    for m in inner:
        m.reflectance, m.radiance = rho_, rad
    return room(hm, (0, 0, 0), (556, 548.8, 559.2), rho_, rad, bsdf) + inner


def s3(rho, max_depth=-1, rr_depth=5, le=ONE, boxes=False, twosided=False, film=False):
    def build(hm):
        size = 128 if film else 16
        flat = hm.flatten(s3_meshes(hm, rho, le, boxes, twosided), size, size, camera=CBOX_INSIDE if boxes else S3_CAMERA)
        cie, _ = tables(flat.desc)
        rho_s = R.constant(rho) if np.isscalar(rho) else R.regular(*rho)
        radiance = R.regular(*le) * rho_s.map(lambda r: R.furnace(1.0, r, max_depth))
        pixels = [(x, y) for y in range(4, 128, 8) for x in range(4, 128, 8)] if film else S3_PIXELS
        return Case(flat, pixels, lambda fine: R.expected_xyz(radiance, cie, grid(8, fine))[None],
                    dict(max_depth=max_depth, rr_depth=rr_depth), pooled=True, film=film)
    return build


S3_CASES = {"cube_rho%g_depth%d_rr%d" % (rho, d, rr): s3(rho, d, rr) for rho in (0.5, 0.8) for d in (-1, 3) for rr in (1, 5)}
S3_CASES.update({
    "cube_with_boxes": s3(0.5, boxes=True),
    "cube_tables": s3((360, 830, [0.2, 0.5, 0.8, 0.6, 0.3]), le=(360, 830, [0.5, 1.0, 2.0, 1.5])),
    "cube_twosided": s3(0.5, twosided=True),
})


# ----------------------------------------------------------------------------- S4
S4_PIXELS = [(3, 4), (6, 1)]
ETA, K = 0.8, 3.0


def s4(bsdf, cos_i, rho=0.5, back=False, azimuth=0.6):
    """A 2 x 2 plate in the plane y = 0 seen under cos_i from 20 units away through a 1 degree lens, in an environment of
    spectral radiance 1.  back: the plate's winding faces down and the camera sees its back (for "twosided")."""
    def build(hm):
        sin_i = np.sqrt(1.0 - cos_i * cos_i)
        cam = dict(fov=1.0, near=0.1, far=100.0, origin=tuple(20.0 * np.array([sin_i * np.cos(azimuth), cos_i, sin_i * np.sin(azimuth)])),
                   target=(0, 0, 0), up=(0, 1, 0))
        u, v = ((1, 0, 0), (0, 0, 1)) if back else ((0, 0, 1), (1, 0, 0))
        rho_ = rho if np.isscalar(rho) else hm.Regular(*rho)
        spec = None
        if bsdf is not None:
            spec = dict(bsdf, eta=hm.Regular(360, 830, [ETA, ETA]), k=hm.Regular(360, 830, [K, K]))
        plate = hm.MeshSpec("plate", [quad((0, 0, 0), u, v)], rho_, bsdf=spec)
        # ideal_fetch: the default specular_reflectance (1, 1, 1) must be S == 1 exactly (the product's upsampling of white is
        # ~0.98), all the more as eval() multiplies by it and sample() does not (roughconductor.cpp:79 against :99)
        flat = hm.flatten([plate], 8, 8, camera=cam, env={"radiance": hm.Regular(*ONE)}, coeff_lookup=ideal_fetch)
        cie, _ = tables(flat.desc)

        def cosines(o, d):
            x = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
            assert np.abs(x).max() < 1.0                       # every ray of the pixel meets the plate
            return -d[..., 1]

        def expected(fine):
            if bsdf is None:
                return np.tile(R.expected_xyz(as_spectrum(rho_), cie, grid(8, fine)), (len(S4_PIXELS), 1))
            amin = float(np.min(bsdf["alpha"]))
            m = (400 if amin < 0.2 else 200) if cos_i < 0.4 else (200 if amin < 0.2 else 100)
            unit = R.unit_xyz(cie, grid(8, fine))
            if not np.isscalar(bsdf["alpha"]):
                # anisotropic: the value depends on the azimuth of wi in the shading frame; 2 x 2 (4 x 4) Gauss nodes per pixel.
                # NOT the albedo: microfacet.h:23-26 draws the half vector's azimuth with alpha_u / alpha_v where D cos needs
                # alpha_v / alpha_u, and the as-written estimator (kept, restated by oracle and kernels) has the expectation
                # radiometry_ref.ggx_conductor_as_written derives: here 0.7 % above the albedo, which this case would not pass
                fs, ft, fn = R.shading_frame((0, 1, 0))

                def one(c, phi):
                    return R.ggx_conductor_as_written(c, bsdf["alpha"], ETA, K, grid(48, fine), phi, light_pdf=0.25 / np.pi)

                def value(o, d):
                    cosines(o, d)                                       # (checks that the rays meet the plate)
                    x, y, z = -(d @ fs), -(d @ ft), -(d @ fn)           # wi in the shading frame
                    return np.vectorize(one)(z, np.arctan2(y, x))
                return np.stack([R.pixel_gauss(value, flat.desc, px, py, grid(2, fine)) * unit for px, py in S4_PIXELS])
            # the albedo over the pixels' range of incidence: a polynomial through 3 (5) Chebyshev nodes of it
            corners = np.concatenate([cosines(*R.camera_ray(flat.desc, np.array([px, px + 1.0, px, px + 1.0]),
                                                            np.array([py, py, py + 1.0, py + 1.0]))) for px, py in S4_PIXELS])
            lo, hi = corners.min(), corners.max()
            n = 5 if fine else 3
            nodes = (lo + hi) / 2 + (hi - lo) / 2 * np.cos(np.pi * (np.arange(n) + 0.5) / n)
            poly = np.polynomial.Polynomial.fit(nodes, [R.ggx_conductor_albedo(c, bsdf["alpha"], ETA, K, grid(m, fine)) for c in nodes],
                                                n - 1)
            return np.stack([R.pixel_mean(lambda o, d: poly(cosines(o, d)), flat.desc, px, py, grid(8, fine)) * unit
                             for px, py in S4_PIXELS])
        return Case(flat, S4_PIXELS, expected, dict(max_depth=-1))
    return build


def _conductor(alpha, **kw):
    return dict({"type": "roughconductor", "alpha": alpha, "sample_visible": False}, **kw)


S4_CASES = {"diffuse_uniform": s4(None, 0.7), "diffuse_table": s4(None, 0.4, rho=(360, 830, [0.2, 0.5, 0.8, 0.6, 0.3]))}
S4_CASES.update({"conductor_alpha%g_cos%g" % (a, c): s4(_conductor(a), c) for a in (0.1, 0.3, 0.6) for c in (0.2, 0.6, 0.95)})
S4_CASES["conductor_twosided_back"] = s4(_conductor(0.3, twosided=True), 0.6, back=True)
S4_CASES["conductor_anisotropic"] = s4(_conductor((0.15, 0.5)), 0.5, azimuth=0.3)

# ----------------------------------------------------------------------------- S5
S5_CASE = s3(0.5, film=True)
S5_SPP, S5_MARGIN = 64, 4

CASES = {}
for _prefix, _group in (("S2_", S2_CASES), ("S3_", S3_CASES), ("S4_", S4_CASES)):
    CASES.update({_prefix + k: v for k, v in _group.items()})
CASES.update({"S1_" + k: s1(k) for k in S1_RADIANCE})
CASES["S5_film"] = S5_CASE
SAMPLED = sorted(k for k in CASES if k != "S5_film")


# ----------------------------------------------------------------------------- the two sides
class CpuSide:
    caps, max_spp, max_records = CAP_CPU, 1 << 13, None

    def __init__(self, oracle, abi):
        self.oracle, self.abi = oracle, abi
        self.pool = ThreadPoolExecutor(min(THREADS, os.cpu_count() or 1))      # sample_pixels is single-threaded; ctypes drops the GIL

    def scene(self, flat):
        return self.oracle.scene(flat)

    def sums(self, sc, kw, pixels, spp, seeds):
        """float64[P, 3]: the sum of every sample of every seed, per pixel"""
        def one(job):
            i, seed = job
            xyz, _ = sc.sample_pixels(self.abi.render_params(spp, seed=seed, **kw), pixels[i][None])
            return i, np.add.reduce(xyz[0], axis=0, dtype=np.float64)
        out = np.zeros((len(pixels), 3))
        for i, s in self.pool.map(one, [(i, seed) for seed in seeds for i in range(len(pixels))]):
            out[i] += s
        return out

    def render(self, sc, prm):
        return sc.render(prm, threads=min(THREADS, os.cpu_count() or 1))[0]


class GpuSide:
    caps, max_spp, max_records = CAP_GPU, 1 << 20, 1 << 22

    def __init__(self, ctx, abi):
        self.ctx, self.abi = ctx, abi

    def scene(self, flat):
        return self.abi.Scene(self.ctx, flat)

    def sums(self, sc, kw, pixels, spp, seeds):
        pixels = np.ascontiguousarray(pixels, np.int32)
        xyz = np.empty((len(pixels), spp, 3), np.float32)
        out = np.zeros((len(pixels), 3))
        for seed in seeds:
            prm = self.abi.render_params(spp, seed=seed, **kw)
            self.ctx.check(self.ctx.lib.msk_gpu_sample_pixels(sc.handle, C.byref(prm), len(pixels), pixels.ctypes.data_as(C.c_void_p),
                                                              xyz.ctypes.data_as(C.c_void_p), None))
            out += np.add.reduce(xyz, axis=1, dtype=np.float64)
        return out

    def render(self, sc, prm):
        return sc.render(prm)[0]


def load_sigma(name):
    entry = json.load(open(SIGMA_PATH))[name]
    assert entry["samples"] >= 1 << 20
    return np.asarray(entry["sigma"], np.float64)


def expectation(case):
    e, e2 = case.expected(False), case.expected(True)
    q = np.abs(e - e2)
    assert np.all(q <= Q_MAX * np.abs(e2)), (q / np.abs(e2)).max()
    return e2, q


def samples_needed(sigma, e, q, caps, extra=0.0):
    """The smallest N at which Z * 1.1 * sigma / sqrt(N) fits under the cap next to q, the rounding term (and `extra`), with 5 % room"""
    room_ = (caps - R_FP32 - extra) * np.abs(e) - q
    assert np.all(room_ > 0)
    return int(np.ceil(((Z * SIGMA_SLACK * sigma / (0.95 * room_)) ** 2).max()))


def compare(name, side, mean, n, sigma, e, q, extra=0.0):
    """One comparison per group and channel: the cap first, then the deviation.  Every figure is printed before it is asserted."""
    failures = []
    for g in range(len(e)):
        tol = Z * SIGMA_SLACK * sigma[g] / np.sqrt(n[g]) + q[g] + (R_FP32 + extra) * np.abs(e[g])
        dev = np.abs(mean[g] - e[g])
        print("RADIOMETRY %s %s group %d N %d expected %s estimate %s dev/|E| %s tol/|E| %s dev/tol %s" % (
            name, type(side).__name__, g, n[g], e[g].tolist(), mean[g].tolist(), (dev / np.abs(e[g])).tolist(),
            (tol / np.abs(e[g])).tolist(), (dev / tol).tolist()))
        for c in range(3):
            assert tol[c] <= side.caps[c] * abs(e[g, c]), (name, g, "XYZ"[c], "cap", tol[c] / abs(e[g, c]), side.caps[c])
            if not dev[c] <= tol[c]:
                failures.append((name, g, "XYZ"[c], "expected", e[g, c], "got", mean[g, c], "tol", tol[c]))
    assert not failures, failures


def run_sampled(name, side, hm):
    case = CASES[name](hm)
    sigma = load_sigma(name)
    e, q = expectation(case)
    assert sigma.shape == e.shape
    per_pixel = max(-(-samples_needed(sigma[g], e[g], q[g], side.caps) // len(idx)) for g, idx in enumerate(case.groups))
    spp = side.max_spp
    if side.max_records:
        spp = min(spp, 1 << int(np.log2(side.max_records // len(case.pixels))))
    spp = min(spp, 1 << int(np.ceil(np.log2(per_pixel))))
    n_seeds = -(-per_pixel // spp)
    seed0 = zlib.crc32(name.encode()) << 8
    sc = side.scene(case.flat)
    try:
        sums = side.sums(sc, case.params, case.pixels, spp, [seed0 + k for k in range(n_seeds)])
    finally:
        sc.close()
    n = np.array([len(idx) * n_seeds * spp for idx in case.groups])
    mean = np.stack([sums[idx].sum(0) / n[g] for g, idx in enumerate(case.groups)])
    compare(name, side, mean, n, sigma, e, q)


def run_film(side, hm, abi, rng_mode):
    """S5: sum(X, Y, Z) / sum(W) over the interior of 128 x 128 films at 64 spp.  A sample whose whole filter footprint lies in
    the interior adds the same total weight to both sums (up to the ripple of the filter's taps), the others less; adding a
    smaller weight to n equal ones never lowers (sum w)^2 / sum w^2, so the effective count is at least the number of
    whole-footprint samples, which is the N used.  fp32: a film pixel is the float32 sum of at most spp * (2 border + 1)^2
    positive addends, a relative error of at most that count times 2^-24 (a bound, not a measurement)."""
    case = S5_CASE(hm)
    sigma = load_sigma("S5_film")
    e, q = expectation(case)
    fd = case.flat.desc.film
    border = int(np.ceil(fd.filter_radius - 0.5))
    extra = S5_SPP * (2 * border + 1) ** 2 * 2.0 ** -24
    per_film = S5_SPP * (fd.width - 2 * S5_MARGIN - 2 * border) * (fd.height - 2 * S5_MARGIN - 2 * border)
    n_films = -(-samples_needed(sigma[0], e[0], q[0], side.caps, extra) // per_film)
    seed0 = zlib.crc32(b"S5_film") + rng_mode
    total = np.zeros(5)
    sc = side.scene(case.flat)
    try:
        for k in range(n_films):
            film = side.render(sc, abi.render_params(S5_SPP, seed=seed0 + k, rng_mode=rng_mode, **case.params))
            assert film.shape == (128, 128, 5)
            total += film[S5_MARGIN:-S5_MARGIN, S5_MARGIN:-S5_MARGIN].astype(np.float64).sum((0, 1))
    finally:
        sc.close()
    compare("S5_film_rng%d" % rng_mode, side, total[None, :3] / total[4], np.array([n_films * per_film]), sigma, e, q, extra)


def run_zero(side, hm, abi):
    """S1: the emitter seen from behind, and hidden: not a single sample may carry light"""
    for facing, kw in ((False, dict(max_depth=1)), (False, dict(max_depth=-1)), (True, dict(max_depth=1, hide_emitters=1))):
        flat, _ = s1_flat(hm, "table", facing)
        sc = side.scene(flat)
        try:
            sums = side.sums(sc, kw, np.array([(3, 4), (16, 16), (28, 9), (12, 30)], np.int32), 1 << 12, [5, 6])
        finally:
            sc.close()
        assert np.all(sums == 0), (facing, kw, sums)


# ----------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def cpu_side(oracle, abi):
    side = CpuSide(oracle, abi)
    yield side
    side.pool.shutdown()


@pytest.fixture(scope="module")
def gpu_side(gpu_ctx, abi):
    return GpuSide(gpu_ctx, abi)


def test_reference_unit_and_known_values(hostmirror):
    """The float64 reference against values known without it: the Y of unit radiance is within 0.2 % of the CIE normalisation
    the reference scales emitters by (core/spectrum.h:75: the integral of the Y table; the importance-sampled wavelength range
    and the linear interpolation account for the difference), a quad that fills the hemisphere's cap has the cap's form
    factor, a disc its own, F(0) is the textbook value, and a white GGX lobe at normal incidence keeps less than 1 / (1 + alpha^2)."""
    flat = hostmirror.flatten([], 8, 8)                  # (owns the tables the descriptor points into)
    cie, _ = tables(flat.desc)
    unit = R.unit_xyz(cie)
    assert abs(unit[1] / 106.7502593994140625 - 1) < 2e-3 and np.allclose(unit, R.unit_xyz(cie, 32), rtol=1e-12)
    e = R.polygon_irradiance(np.zeros((1, 3)), (0, 0, 1), quad((0, 0, 1e-3), (1e3, 0, 0), (0, 1e3, 0)))
    assert abs(e[0] / np.pi - 1) < 1e-5                                           # the whole hemisphere: pi
    h = 2.0                                                                       # a disc of radius a seen from below its centre:
    ring = [(np.cos(t), np.sin(t), h) for t in np.linspace(0, 2 * np.pi, 2000, endpoint=False)]      # pi a^2 / (a^2 + h^2)
    assert abs(R.polygon_irradiance(np.zeros((1, 3)), (0, 0, 1), ring)[0] / (np.pi / (1 + h * h)) - 1) < 1e-5
    assert abs(R.fresnel_conductor(1.0, 1.5, 3.0) - ((0.5 ** 2 + 9) / (2.5 ** 2 + 9))) < 1e-12
    # |n| -> infinity: F = 1.  At normal incidence the facets tilted past 45 degrees (a share alpha^2 / (1 + alpha^2) of
    # D cos) send the light below the horizon, and shadowing takes a little more
    white = R.ggx_conductor_albedo(1.0, 0.3, 1.0, 1e6, 200)
    assert 0.85 < white < 1 / 1.09 and abs(R.ggx_conductor_albedo(1.0, 0.3, 1.0, 1e6, 400) - white) < 1e-9
    # the as-written estimator of an isotropic lobe is the albedo, by a different parametrisation of the integral
    assert abs(R.ggx_conductor_as_written(0.6, 0.3, ETA, K, 100, 0.4, 0.08) / R.ggx_conductor_albedo(0.6, 0.3, ETA, K, 200) - 1) < 1e-10


@pytest.mark.parametrize("name", SAMPLED)
def test_oracle_radiance_matches_the_closed_form(name, cpu_side, hostmirror):
    run_sampled(name, cpu_side, hostmirror)


@pytest.mark.parametrize("rng_mode", [1, 0])
def test_oracle_film_matches_the_closed_form(rng_mode, cpu_side, hostmirror, abi):
    run_film(cpu_side, hostmirror, abi, rng_mode)


def test_oracle_unseen_emitter_is_exactly_zero(cpu_side, hostmirror, abi):
    run_zero(cpu_side, hostmirror, abi)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SAMPLED)
def test_gpu_radiance_matches_the_closed_form(name, gpu_side, hostmirror):
    run_sampled(name, gpu_side, hostmirror)


@pytest.mark.gpu
@pytest.mark.parametrize("rng_mode", [1, 0])
def test_gpu_film_matches_the_closed_form(rng_mode, gpu_side, hostmirror, abi):
    run_film(gpu_side, hostmirror, abi, rng_mode)


@pytest.mark.gpu
def test_gpu_unseen_emitter_is_exactly_zero(gpu_side, hostmirror, abi):
    run_zero(gpu_side, hostmirror, abi)
