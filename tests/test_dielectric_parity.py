"""The smooth `dielectric` BSDF (glass) against its CPU twin, and the twin against float64.

oracle/oracle.cpp restates SmoothDielectric::sample / eval / pdf (bsdfs/dielectric.cpp:26-82) and the two BSDFFlags conditions of
PathTracer::sample (integrators/path.cpp:56,104-106), so glass is inside the bit-for-bit parity net.  Three layers:

  CPU   the twin against float64 (tests/dielectric_ref.py): lobe choice, pdf, eta, weight and the refracted DIRECTION on a grid of
        incident directions, and the float64 identities of test_smooth_dielectric.py on the twin's own renders — the twin has to
        pass what the device passes before it is trusted;
  both  a check of the refraction geometry that needs no twin: an emitter behind the glass that covers only x > x0, so that the
        refracted direction decides whether a sample is lit (the identities of test_smooth_dielectric.py all sit in a constant
        environment, where a transmitted sample has the same value wherever it goes);
  GPU   the device against the twin, bit for bit (array_equal on the uint32 view, no tolerance): glass next to every other BSDF,
        emitter and integrator setting, under every execution variant.

Tolerances of the CPU layer (none is taken from what the code gives):
  direction   absolute per component 2^-24 (4 + 4 / cos_t): the rounding of 1 - eta_ti^2 (1 - cos_i^2), three roundings of at most
              2^-24 on a value below 1, carried through the square root (d sqrt(x) = dx / (2 sqrt(x))), plus the products' own;
              asserted where the float64 cos_t >= 0.1
  pdf         absolute 2^-24 (8 + 2 / cos_t^2): r = (a_s^2 + a_p^2) / 2 with |a| <= 1, so dr <= |da_s| + |da_p|; each a is a
              quotient (x - y) / (x + y) of positive terms, whose own roundings stay below 4 * 2^-24, and whose derivative by cos_t
              is at most 1 / (2 cos_t) (2 xy / (x + y)^2 <= 1 / 2), times the d cos_t above
  weight      relative 4 * 2^-24: the reciprocal of eta and two products
  ratios      16 * 2^-24 (1 + interface events), the binomial rule, as test_smooth_dielectric.py states them
"""
import numpy as np
import pytest

import dielectric_ref as D
import radiometry_ref as R
import test_smooth_dielectric as S
from test_smooth_dielectric import EPS, ETA, F32, NO_RR, SIZE, quad, box

U = 2.0 ** -24
ETAS = {"1.5": dict(int_ior=1.5, ext_ior=1.0), "1.33": dict(int_ior=1.33, ext_ior=1.0), "default": dict(),
        "1/1.5": dict(int_ior=1.0, ext_ior=1.5)}
DELTA_REFLECTION, DELTA_TRANSMISSION = 8, 16           # oracle.cpp: kDeltaReflection, kDeltaTransmission


# ============================================================================= CPU: the twin's BSDF against float64
def glass_desc(hm, **spec):
    tri = [((0, 0, 0), (1, 0, 0), (0, 1, 0))]
    flat = hm.flatten([hm.MeshSpec("glass", tri, 0.5, bsdf=dict(spec, type="dielectric"))], 8, 8)
    return flat, flat.desc.bsdfs[0]


def incident_grid(eta):
    """wi in fp32: z in {+-1, +-0.5, +-0.05, 0} x five azimuths, and, on the dense side, z on either side of the critical angle"""
    zs = [1.0, -1.0, 0.5, -0.5, 0.05, -0.05, 0.0]
    dense_sign = -1.0 if eta > 1.0 else 1.0
    cos_c = np.sqrt(1.0 - min(eta, 1.0 / eta) ** 2)
    for d in (1e-2, 1e-3, 1e-4):
        zs += [dense_sign * (cos_c + d), dense_sign * (cos_c - d)]
    out = []
    for z in zs:
        for phi in (0.0, 0.7, 2.1, 3.6, 5.5):
            s = np.sqrt(max(0.0, 1.0 - z * z))
            out.append(np.array([s * np.cos(phi), s * np.sin(phi), z], np.float32))
    return out


@pytest.mark.parametrize("name", sorted(ETAS))
def test_twin_sample_against_float64(oracle, hostmirror, name):
    """oracle.bsdf_sample2 on type 3: every output against float64 at the fp32 inputs (module docstring for the bounds)"""
    tint_r, tint_t = 0.5, 0.25                                   # `uniform` spectra: the tint is the same at every wavelength
    flat, b = glass_desc(hostmirror, specular_reflectance=tint_r, specular_transmittance=tint_t, **ETAS[name])
    eta = float(F32(b.ior_eta))
    worst = dict(direction=0.0, pdf=0.0, weight=0.0, norm=0.0)
    n_dir = n_class = n_tir = 0
    for wi in incident_grid(eta):
        w64 = wi.astype(np.float64)
        r64, ct64, eta_it, eta_ti = (float(x) for x in D.fresnel(w64[2], eta))
        wo64, _, _, _, tir = D.refract_local(w64, eta)
        sin_t2 = eta_ti * eta_ti * (1.0 - w64[2] * w64[2])
        # the reference's cos_t comes from wi.z alone (fresnel.h:47-48), Snell's from the transverse part: they agree as far as
        # |wi| = 1 does, which the direction check below allows for
        for x in (0.0, 0.5 * r64, r64 + 0.5 * (1.0 - r64), float(np.nextafter(F32(1), F32(0)))):
            u = (F32(x), F32(0.37))
            for sample1 in (0.0, 0.999):                         # the lobe is NOT chosen by sample1 (dielectric.cpp:37)
                wo, pdf, w, bs_eta, typ = oracle.bsdf_sample2([b], 0, wi, sample1, u)
                assert np.isfinite(wo).all() and np.isfinite(pdf) and np.isfinite(w).all(), (wi, x)
                if w64[2] == 0.0:                                # fresnel.h:57-58: grazing incidence reflects, r_i = 1
                    assert pdf == 1.0 and typ == DELTA_REFLECTION
                if abs(sin_t2 - 1.0) < 1e-5:
                    continue                                     # the band around the critical angle: nothing asserted
                if sin_t2 > 1.0:                                 # beyond it: always reflection, with certainty
                    n_tir += 1
                    assert tir and typ == DELTA_REFLECTION and pdf == 1.0 and bs_eta == 1.0, (wi, x, pdf)
                    assert np.array_equal(wo, np.array([-wi[0], -wi[1], wi[2]], np.float32)) and np.all(w == F32(tint_r))
                    continue
                margin = abs(float(u[0]) - r64)
                tol_pdf = U * (8.0 + 2.0 / (ct64 * ct64))
                if margin <= 2.0 * tol_pdf:
                    continue                                     # (x = 0 at r64 = 0 never occurs: eta != 1)
                n_class += 1
                reflected = float(u[0]) <= r64
                assert typ == (DELTA_REFLECTION if reflected else DELTA_TRANSMISSION), (wi, x, r64, typ)
                assert typ & (DELTA_REFLECTION | DELTA_TRANSMISSION)
                if abs(ct64) < 0.1:
                    continue                                     # nearer the critical angle only the classification
                n_dir += 1
                assert F32(bs_eta) == (F32(1.0) if reflected else F32(eta_it)), (wi, bs_eta, eta_it)
                err = abs(pdf - (r64 if reflected else 1.0 - r64))
                worst["pdf"] = max(worst["pdf"], err / tol_pdf)
                assert err <= tol_pdf, (wi, x, pdf, r64)
                if reflected:
                    assert np.array_equal(wo, np.array([-wi[0], -wi[1], wi[2]], np.float32)), (wi, wo)
                    assert np.all(w == F32(tint_r)), w
                    continue
                tol = U * (4.0 + 4.0 / abs(ct64))
                o64 = wo.astype(np.float64)
                expect = np.array([-eta_ti * w64[0], -eta_ti * w64[1], ct64])
                err = np.abs(o64 - expect).max()
                worst["direction"] = max(worst["direction"], err / tol)
                assert err <= tol, (wi, wo, expect)
                assert o64[2] * w64[2] < 0.0                                              # the opposite hemisphere
                assert abs(o64[0] * w64[1] - o64[1] * w64[0]) <= 2.0 * tol                # the plane of incidence
                assert o64[0] * w64[0] + o64[1] * w64[1] <= 0.0                           # ... on the far side of the normal
                assert abs(np.hypot(o64[0], o64[1]) - eta_ti * np.hypot(w64[0], w64[1])) <= 2.0 * tol      # Snell
                wi_len = abs(w64 @ w64 - 1.0)                                             # fp32 wi is a unit vector only so far
                assert np.abs(o64 - wo64).max() <= tol + 2.0 * eta_ti * eta_ti * wi_len / abs(ct64)        # ... the vector form
                err = abs(np.linalg.norm(o64) - 1.0)
                tol_n = 3.0 * tol + eta_ti * eta_ti * wi_len
                worst["norm"] = max(worst["norm"], err / tol_n)
                assert err <= tol_n
                err = np.abs(w.astype(np.float64) / (tint_t * eta_ti * eta_ti) - 1.0).max()
                worst["weight"] = max(worst["weight"], err / (4.0 * U))
                assert err <= 4.0 * U, (w, eta_ti)
    print("DIELECTRIC twin eta %s: %d classified, %d with direction / pdf / weight, %d beyond the critical angle; worst error / tolerance %s"
          % (name, n_class, n_dir, n_tir, {k: round(v, 3) for k, v in worst.items()}))
    assert n_dir >= 100 and n_class > n_dir and n_tir > 0


def test_twin_eval_pdf_are_zero_and_type_3_has_its_own_branch(oracle, hostmirror):
    """dielectric.cpp:74-82; and bsdf_sample (without the lobe sample) takes the same branch as bsdf_sample2"""
    _, b = glass_desc(hostmirror, int_ior=1.5, ext_ior=1.0, specular_reflectance=1.0, specular_transmittance=1.0)
    rng = np.random.RandomState(1)
    for _ in range(50):
        wi, wo = rng.normal(size=3), rng.normal(size=3)
        wi, wo = wi / np.linalg.norm(wi), wo / np.linalg.norm(wo)
        val, pdf = oracle.bsdf_eval([b], 0, wi, wo)
        assert not val.any() and pdf == 0.0
    wi = np.array([0.6, 0.0, 0.8], np.float32)
    val, pdf = oracle.bsdf_eval([b], 0, wi, np.array([-0.6, 0.0, 0.8], np.float32))       # the mirror direction itself
    assert not val.any() and pdf == 0.0
    for u in ((0.01, 0.3), (0.9, 0.3)):
        a = oracle.bsdf_sample([b], 0, wi, u)
        c = oracle.bsdf_sample2([b], 0, wi, 0.5, u)
        assert np.array_equal(a[0], c[0]) and a[1] == c[1] and np.array_equal(a[2], c[2])
    wo, pdf, w = oracle.bsdf_sample([b], 0, -wi, (0.9, 0.3))                               # from inside: not the one-sided early-out
    assert pdf > 0 and wo[2] > 0 and np.all(w == F32(1.5) * F32(1.5))


# ============================================================================= CPU: the twin's renders against float64
def oracle_sampler(oracle, abi):
    def run(flat, pixels, spp, seed, **kw):
        sc = oracle.scene(flat)
        try:
            return sc.sample_pixels(abi.render_params(spp, seed=seed, **kw), np.asarray(pixels, np.int32))
        finally:
            sc.close()
    return run


def gpu_sampler(abi, gpu_ctx):
    return lambda flat, pixels, spp, seed, **kw: S.sample(abi, gpu_ctx, flat, pixels, spp, seed, **kw)


CPU_SPP = 1 << 14


def interface_case(run, flat, ref, pixels, spp, seed, values, r_of_cos, reflected, sign=1.0, what=""):
    """test_smooth_dielectric.interface_case with the renderer as an argument"""
    xyz, pos = run(flat, pixels, spp, seed, **NO_RR)
    base, bpos = run(ref, pixels, spp, seed, **NO_RR)
    assert np.array_equal(pos, bpos)
    y, spread = S.ratios(xyz, base)
    assert spread <= 4 * EPS
    idx = S.classify(y, values, 1)
    cos = sign * D.incidence_cosines(flat.desc, pos.reshape(-1, 2).astype(np.float64))
    assert np.all(cos > 0.05)
    S.binomial(int((idx == reflected).sum()), r_of_cos(cos), None, what)
    return idx


@pytest.mark.parametrize("degrees", [10, 45, 60, 75])
def test_twin_one_interface_from_outside(oracle, abi, hostmirror, degrees):
    flat, ref = S.interface_scenes(hostmirror, S.ABOVE)
    t = float(F32(1.0) / F32(ETA)) ** 2
    interface_case(oracle_sampler(oracle, abi), flat, ref, S.pixels_at(flat.desc, SIZE, degrees, 4), CPU_SPP, 100 + degrees, [1.0, t],
                   lambda c: D.reflectance(c, ETA), 0, what="twin outside %d deg" % degrees)


def test_twin_one_interface_from_inside(oracle, abi, hostmirror):
    run = oracle_sampler(oracle, abi)
    flat, ref = S.interface_scenes(hostmirror, S.BELOW)
    cos_c = np.cos(D.critical_angle(ETA))
    pixels = S.pixels_at(flat.desc, SIZE, 60, 4, sign=-1.0)
    xyz, pos = run(flat, pixels, CPU_SPP, 7, **NO_RR)
    base, _ = run(ref, pixels, CPU_SPP, 7, **NO_RR)
    cos = -D.incidence_cosines(flat.desc, pos.reshape(-1, 2).astype(np.float64))
    assert np.all((cos > 0.05) & (cos < cos_c - 0.05))
    y, spread = S.ratios(xyz, base)
    assert spread <= 4 * EPS and np.all(S.classify(y, [1.0], 1) == 0)
    pixels = S.pixels_at(flat.desc, SIZE, 25, 4, sign=-1.0)
    xyz, pos = run(flat, pixels, CPU_SPP, 8, **NO_RR)
    base, _ = run(ref, pixels, CPU_SPP, 8, **NO_RR)
    cos = -D.incidence_cosines(flat.desc, pos.reshape(-1, 2).astype(np.float64))
    assert np.all(cos > cos_c + 0.05)
    y, spread = S.ratios(xyz, base)
    assert spread <= 4 * EPS
    idx = S.classify(y, [1.0, float(F32(ETA)) ** 2], 1)
    S.binomial(int((idx == 0).sum()), D.reflectance(-cos, ETA), what="twin inside 25 deg")


def test_twin_tints(oracle, abi, hostmirror):
    flat, ref = S.interface_scenes(hostmirror, S.ABOVE, dict(S.GLASS, specular_reflectance=0.5, specular_transmittance=0.25))
    eta_ti = float(F32(1.0) / F32(ETA))
    interface_case(oracle_sampler(oracle, abi), flat, ref, S.pixels_at(flat.desc, SIZE, 60, 4), CPU_SPP, 21, [0.5, 0.25 * eta_ti * eta_ti],
                   lambda c: D.reflectance(c, ETA), 0, what="twin tints")


def test_twin_lossless_slab(oracle, abi, hostmirror):
    """R <= 0.1 within 45 degrees: one of the 2^16 samples has more than 11 internal reflections with probability < 1e-6"""
    run = oracle_sampler(oracle, abi)
    flat, ref = S.slab_scenes(hostmirror, SIZE, {"radiance": None})
    xyz, pos = run(flat, S.SLAB_PIXELS, CPU_SPP, 31, **NO_RR)
    base, _ = run(ref, S.SLAB_PIXELS, CPU_SPP, 31, **NO_RR)
    r = S.slab_r(flat, pos)
    m = 11
    assert r.max() <= 0.1 and xyz.size // 3 * r.max() ** m < 1e-6
    y, spread = S.ratios(xyz, base)
    assert spread <= 4 * EPS and np.all(S.classify(y, [1.0], m + 2) == 0)


def test_twin_slab_with_russian_roulette(oracle, abi, hostmirror):
    """As test_slab_with_russian_roulette: every live sample carries 0.95^-k, and the mean ratio is 1 within 5 sqrt(V / N) (the
    device's test caps that tolerance at 2e-3 with 2^20 samples; at the 2^16 of this one the statistics allow 6e-3, asserted)"""
    run = oracle_sampler(oracle, abi)
    flat, ref = S.slab_scenes(hostmirror, SIZE, {"radiance": None})
    kw = dict(max_depth=-1, rr_depth=2)
    xyz, pos = run(flat, S.SLAB_PIXELS, CPU_SPP, 41, **kw)
    base, _ = run(ref, S.SLAB_PIXELS, CPU_SPP, 41, **kw)
    y, spread = S.ratios(xyz, base)
    assert spread <= 4 * EPS
    q = float(F32(0.95))
    live = y > 0
    k = np.rint(np.log(y[live]) / -np.log(q))
    assert k.min() >= 0 and k.max() < 64
    err = np.abs(y[live] * q ** k - 1.0)
    tol = EPS * (1 + np.where(k == 0, 1, k + 1))
    print("DIELECTRIC twin roulette: k histogram %s dead %d worst error/tol %.3g" % (np.bincount(k.astype(int)).tolist(), int((~live).sum()), (err / tol).max()))
    assert np.all(err <= tol)
    mean, second = D.slab_roulette_moments(S.slab_r(flat, pos), q)
    tol_mean = 5.0 * np.sqrt((second - mean * mean).mean() / len(y)) + EPS * 3
    print("DIELECTRIC twin roulette: N %d mean ratio %.6f tol %.3g" % (len(y), y.mean(), tol_mean))
    assert tol_mean <= 6e-3 and abs(y.mean() - 1.0) <= tol_mean


# ============================================================================= both: where the refracted ray lands, in float64
H_EMITTER = 1.0
RADIANCE = (0.9, 0.5, 0.2)


def landing(desc, pos, side, h):
    """float64: where the camera ray through film position pos, refracted at the plane y = 0 (Snell, dielectric_ref.refract),
    meets the plane y = -side * h -> (point [n, 3], transmitted possible [n], cos of incidence [n])"""
    o, d = R.camera_ray(desc, pos[..., 0].astype(np.float64), pos[..., 1].astype(np.float64))
    x = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
    t, tir = D.refract(d, np.array([0.0, 1.0, 0.0]), ETA)
    s = (-side * h - x[:, 1]) / t[:, 1]
    return x + t * s[:, None], ~tir, -side * d[:, 1]


def refraction_scene(hm, camera, side, degrees):
    """side +1: the ABOVE camera, the emitter below the glass facing up; -1: the BELOW camera, the emitter above facing down.
    The pixel column is chosen on the film's line of symmetry (world z = 0) at `degrees` of incidence; x0 is where the refracted
    centre of that column lands, so the image of the emitter's edge runs along the column and crosses each of its pixels."""
    probe = hm.flatten([], SIZE, SIZE, camera=camera)
    xs = np.arange(SIZE) + 0.5
    mid = np.stack([xs, np.full(SIZE, SIZE / 2.0)], -1)
    _, _, cos = landing(probe.desc, mid, side, H_EMITTER)
    px = int(np.abs(np.degrees(np.arccos(np.clip(cos, -1, 1))) - degrees).argmin())
    p0, ok, _ = landing(probe.desc, np.array([[px + 0.5, SIZE / 2.0]]), side, H_EMITTER)
    assert ok.all()
    x0 = float(p0[0, 0])
    pixels = np.array([[px, SIZE // 2 - 2 + k] for k in range(4)], np.int32)
    glass = hm.MeshSpec("glass", [S.up_quad(0.0, 50.0)], 0.5, bsdf=dict(S.GLASS))
    y = -side * H_EMITTER
    u, v = ((0, 0, 4.0), (4.0, 0, 0)) if side > 0 else ((4.0, 0, 0), (0, 0, 4.0))         # z x x = +y (faces up); x x z = -y
    light = hm.MeshSpec("light", [quad((x0 + 4.0, y, 0), u, v)], 0.0, radiance=RADIANCE)     # covers x0 < x < x0 + 8, |z| < 4
    flat = hm.flatten([glass, light], SIZE, SIZE, camera=camera)
    edge = float(flat.vertices[flat.desc.meshes[1].first_vertex:, 0].min())              # the edge as the renderers see it, in fp32
    assert abs(edge - x0) <= 1e-6
    x0 = edge
    wall = hm.MeshSpec("light", [quad((0, -side * 5.0, 0), tuple(100 * a for a in u), tuple(100 * a for a in v))], 0.0, radiance=RADIANCE)
    return flat, hm.flatten([wall], SIZE, SIZE, camera=camera), pixels, x0


def refraction_case(run, hm, camera, side, degrees, spp, seed, what):
    """The emitter seen through the glass.  A transmitted sample whose float64 landing point has x < x0 is exactly zero; one
    with x > x0 carries the emitter's radiance times eta_ti^2 (MIS weight 1 after a delta bounce) = the companion's value (the
    emitter seen directly, max_depth 1) times eta_ti^2 within 2 EPS; a reflected sample is zero (nothing is on the camera's
    side).  So on the lit side a sample is lit with probability 1 - R (binomial rule), on the dark side never.  Samples whose
    landing point is within 1e-4 h of x0 are left out: at most 1 % (asserted, from the reference alone)."""
    flat, ref, pixels, x0 = refraction_scene(hm, camera, side, degrees)
    xyz, pos = run(flat, pixels, spp, seed, **NO_RR)
    base, bpos = run(ref, pixels, spp, seed, max_depth=1)
    assert np.array_equal(pos, bpos)
    n_px = len(pixels)
    p, can_pass, cos = landing(flat.desc, pos.reshape(-1, 2), side, H_EMITTER)
    assert can_pass.all() and np.all(cos > 0.05)
    assert np.all((np.abs(p[:, 2]) < 1.0) & (np.abs(p[:, 0] - x0) < 1.0))                 # well inside the emitter's other edges
    near = np.abs(p[:, 0] - x0) < 1e-4 * H_EMITTER
    share = near.mean()
    lit_side = (p[:, 0] > x0) & ~near
    dark_side = (p[:, 0] < x0) & ~near
    per_pixel = lit_side.reshape(n_px, -1).mean(1)
    print("DIELECTRIC refraction %s: x0 %.6f pixels %s left out %d of %d (%.4f %%); lit side per pixel %s" % (
        what, x0, pixels.tolist(), int(near.sum()), len(near), 100 * share, np.round(per_pixel, 3).tolist()))
    assert share <= 0.01
    assert np.all((per_pixel > 0.1) & (per_pixel < 0.9))                                 # both outcomes in every pixel
    y, spread = S.ratios(xyz, base)
    assert spread <= 4 * EPS
    assert np.all(y[dark_side] == 0.0), (int((y[dark_side] != 0).sum()), int(dark_side.sum()))
    eta_ti = float(F32(1.0) / F32(ETA)) if side > 0 else float(F32(ETA))
    lit = lit_side & (y != 0.0)
    assert lit.sum() > 0.3 * lit_side.sum()
    assert np.all(S.classify(y[lit], [eta_ti * eta_ti], 1) == 0)                           # tol = EPS * 2
    S.binomial(int(lit.sum()), 1.0 - D.reflectance(side * cos[lit_side], ETA), what="refraction " + what)


def test_twin_refraction_geometry_from_outside(oracle, abi, hostmirror):
    refraction_case(oracle_sampler(oracle, abi), hostmirror, S.ABOVE, +1, 42.5, CPU_SPP, 61, "twin outside")


def test_twin_refraction_geometry_from_inside(oracle, abi, hostmirror):
    refraction_case(oracle_sampler(oracle, abi), hostmirror, S.BELOW, -1, 25.0, CPU_SPP, 62, "twin inside")


@pytest.mark.gpu
def test_refraction_geometry_from_outside(gpu_ctx, abi, hostmirror):
    refraction_case(gpu_sampler(abi, gpu_ctx), hostmirror, S.ABOVE, +1, 42.5, 1 << 16, 61, "device outside")


@pytest.mark.gpu
def test_refraction_geometry_from_inside(gpu_ctx, abi, hostmirror):
    refraction_case(gpu_sampler(abi, gpu_ctx), hostmirror, S.BELOW, -1, 25.0, 1 << 16, 62, "device inside")


# ============================================================================= GPU against the twin, bit for bit
def prism(c, r, hz):
    """A triangular prism along z, faces outward: two triangles and three quads"""
    c = np.asarray(c, np.float64)
    pts = [c + (r * np.cos(a), r * np.sin(a), 0.0) for a in (np.pi / 2, np.pi / 2 + 2 * np.pi / 3, np.pi / 2 + 4 * np.pi / 3)]
    lo, hi = [p - (0, 0, hz) for p in pts], [p + (0, 0, hz) for p in pts]
    t = lambda *ps: tuple(tuple(float(x) for x in p) for p in ps)
    faces = [t(hi[0], hi[1], hi[2]), t(lo[0], lo[2], lo[1])]
    for i in range(3):
        j = (i + 1) % 3
        faces.append(t(lo[i], lo[j], hi[j], hi[i]))
    return faces


def with_normals(flat, mesh, center):
    """radial vertex normals on one mesh of a flattened scene (mesh.cpp:68-96: the shading frame then differs from the face's)"""
    md = flat.desc.meshes[mesh]
    v = flat.vertices[md.first_vertex:md.first_vertex + md.vertex_count]
    d = v[:, :3] - np.asarray(center, np.float32)
    v[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    md.has_normals = 1
    return flat


def caustic_room(hm, size=64):
    """(a) the closed room of test_smooth_dielectric.room_meshes (diffuse walls, an area light) with a flat-shaded glass cube and a
    glass prism: chains of total internal reflection, next-event sampling after a delta bounce, shadow rays that end on glass"""
    glass = [hm.MeshSpec("cube", box((0.35, -0.69, 0.2), (0.25, 0.3, 0.2)), 0.5, bsdf={"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0}),
             hm.MeshSpec("prism", prism((-0.35, -0.3, 0.1), 0.3, 0.25), 0.5, bsdf={"type": "dielectric"})]
    return hm.flatten(S.room_meshes(hm, glass), size, size, camera=S.ROOM_CAMERA)


def blob_room(hm, int_ior, size=48):
    """(b) a smooth-shaded glass blob in the room of room_meshes (which gives the floor its checkerboard), in front of a back wall
    that gets a checkerboard of its own here"""
    blob = hm.blob_mesh("blob", (0.0, -0.35, 0.1), 0.33, 8, 12, 0.5)
    blob.bsdf = {"type": "dielectric", "int_ior": int_ior, "ext_ior": 1.0}
    meshes = S.room_meshes(hm, [blob])
    for m in meshes:
        if m.name == "back":
            m.bsdf = {"type": "diffuse", "texture": {"type": "checkerboard", "color0": (0.9, 0.3, 0.1), "color1": (0.1, 0.3, 0.8), "scale": (5, 7)}}
    flat = hm.flatten(meshes, size, size, camera=S.ROOM_CAMERA)
    return with_normals(flat, len(meshes) - 1, (0.0, -0.35, 0.1))


OPEN_CAMERA = dict(fov=60.0, near=0.01, far=100.0, origin=(0.2, 0.8, -2.2), target=(0.0, -0.2, 0.0), up=(0, 1, 0))


def every_class_meshes(hm):
    """(c) diffuse (textured and two-sided), rough conductor, rough dielectric and glass whose tints take each spectrum kind the
    flattener accepts (rgb, `uniform`, `regular`), two area emitters; flatten with a constant environment"""
    reg = lambda a, b: hm.Regular(360.0, 830.0, np.linspace(a, b, 7))
    tex = {"type": "diffuse", "twosided": True, "texture": {"type": "checkerboard", "color0": (0.8, 0.8, 0.7), "color1": (0.15, 0.2, 0.35), "scale": (8, 8)}}
    return [hm.MeshSpec("floor", [quad((0, -0.8, 0), (0, 0, 1.5), (1.5, 0, 0))], 0.5, bsdf=tex),
            hm.MeshSpec("screen", [quad((0, 0.0, 1.2), (0, 1.0, 0), (1.4, 0, 0))], (0.6, 0.5, 0.3), bsdf={"type": "diffuse", "twosided": True}),
            hm.MeshSpec("plate", [quad((-0.9, -0.3, 0.3), (0, 0, 0.4), (0.2, 0.4, 0))], 0.5,
                        bsdf={"type": "roughconductor", "alpha": 0.15, "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14), "twosided": True}),
            hm.MeshSpec("frosted", box((0.8, -0.5, 0.4), (0.2, 0.3, 0.2)), 0.5, bsdf={"type": "roughdielectric", "alpha": 0.2, "int_ior": 1.5, "ext_ior": 1.0}),
            hm.MeshSpec("lamp1", [quad((0.0, 1.4, 0.0), (0.3, 0, 0), (0, 0, 0.3))], 0.0, radiance=(18, 16, 12)),
            hm.MeshSpec("lamp2", [quad((-1.3, 0.2, -0.2), (0, 0.2, 0), (0, 0, 0.2))], 0.3, radiance=hm.Regular(400.0, 700.0, [0.02, 0.06, 0.03, 0.08])),
            hm.MeshSpec("cube", box((0.1, -0.5, -0.2), (0.25, 0.3, 0.2)), 0.5,
                        bsdf={"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0, "specular_reflectance": (0.9, 0.6, 0.3), "specular_transmittance": (0.4, 0.8, 0.9)}),
            hm.MeshSpec("prism", prism((-0.45, -0.45, -0.3), 0.3, 0.2), 0.5,
                        bsdf={"type": "dielectric", "int_ior": 1.33, "ext_ior": 1.0, "specular_reflectance": 0.7, "specular_transmittance": 0.85}),
            hm.MeshSpec("pane", [quad((0.5, 0.1, -0.6), (0.4, 0, 0.1), (0, 0.5, 0))], 0.5,
                        bsdf={"type": "dielectric", "int_ior": 1.0, "ext_ior": 1.5, "specular_reflectance": reg(0.3, 1.0), "specular_transmittance": reg(1.0, 0.4)})]


ENV = {"radiance": (0.5, 0.6, 0.8)}


def every_class(hm, size=64, crop=None, pads=()):
    return hm.flatten(every_class_meshes(hm) + list(pads), size, size, camera=OPEN_CAMERA, env=dict(ENV), crop=crop)


BIG_BLOB_CENTRE = (-0.25, 0.25, 0.3)


def every_class_with_a_big_blob(hm, size=64):
    """(c) plus a smooth-shaded glass blob of 480 triangles: the per-triangle tables (6 float4 a triangle) no longer fit the 2560
    float4 of LDS while the small ones are still staged there; with MSK_LDS_SCENE_KB=0 the tree is in HBM too (trace mode 6),
    which is where k_wavefront_h_d runs (msk_gpu.hip: fused_h)"""
    blob = hm.blob_mesh("bigblob", BIG_BLOB_CENTRE, 0.3, 16, 16, 0.5)
    blob.bsdf = {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0, "specular_transmittance": (0.95, 0.9, 0.8)}
    meshes = every_class_meshes(hm) + [blob]
    flat = hm.flatten(meshes, size, size, camera=OPEN_CAMERA, env=dict(ENV))
    return with_normals(flat, len(meshes) - 1, BIG_BLOB_CENTRE)


def every_class_padded(hm):
    """(c) with faceless meshes until the tables are one float4 too many for LDS (the construction of test_table_placement.py);
    the small tables alone then exceed what stage_tables<false> copies, so the shading code reads them from HBM"""
    import test_table_placement as T
    base = T.table_plan(every_class(hm))
    assert base["lds_tables"]
    return every_class(hm, pads=T.faceless_pads(hm, T.LDS_TABLES_F4 + 1 - base["table_f4"]))


def emitting_glass(hm, env, size=48):
    """(d) a glass cube that is also an area emitter, a second glass body and a diffuse floor"""
    meshes = [hm.MeshSpec("floor", [quad((0, -0.8, 0), (0, 0, 1.5), (1.5, 0, 0))], (0.6, 0.6, 0.5)),
              hm.MeshSpec("glow", box((0.2, -0.4, 0.0), (0.3, 0.3, 0.3)), 0.5, radiance=(4, 3, 2), bsdf={"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0}),
              hm.MeshSpec("prism", prism((-0.6, -0.45, -0.2), 0.3, 0.2), 0.5, bsdf={"type": "dielectric"})]
    return hm.flatten(meshes, size, size, camera=OPEN_CAMERA, env=env)


def some_pixels(size, n, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.randint(0, size, (n - 4, 2)), [[0, 0], [size - 1, size - 1], [size // 2, size // 2], [size // 2, size - 1]]]).astype(np.int32)


class Pair:
    """A flattened scene on the device and in the twin"""

    def __init__(self, abi, gpu_ctx, oracle, flat):
        self.abi, self.flat = abi, flat
        self.g, self.o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)

    def close(self):
        self.g.close()
        self.o.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def samples_equal(self, pixels, what="", **kw):
        prm = self.abi.render_params(**kw)
        gx, gp = self.g.sample_pixels(prm, pixels)
        ox, op = self.o.sample_pixels(prm, pixels)
        assert np.array_equal(gp.view(np.uint32), op.view(np.uint32)), what
        bad = (gx.view(np.uint32) != ox.view(np.uint32)).any(-1)
        assert not bad.any(), (what, kw, int(bad.sum()), bad.size, np.argwhere(bad)[:4].tolist())
        assert np.isfinite(gx).all()
        return gx

    def films_equal(self, what="", want=None, **kw):
        prm = self.abi.render_params(**kw)
        film, st = self.g.render(prm)
        ref = want if want is not None else self.o.render(prm, threads=16)[0]
        assert film.shape == ref.shape, (what, film.shape, ref.shape)
        bad = (film.view(np.uint32) != ref.view(np.uint32)).any(-1)
        assert not bad.any(), (what, kw, int(bad.sum()), bad.size, np.argwhere(bad)[:4].tolist())
        assert st.invalid_samples == 0
        return film, st


@pytest.fixture(scope="module")
def room_flat(hostmirror):
    return caustic_room(hostmirror)


@pytest.fixture(scope="module")
def mixed_flat(hostmirror):
    return every_class(hostmirror)


def twin_reference(oracle, abi, flat):
    o = oracle.scene(flat)
    prm = abi.render_params(spp=16, seed=5)
    film, st = o.render(prm, threads=16)
    pixels = some_pixels(64, 128, 3)
    xyz, pos = o.sample_pixels(prm, pixels)
    o.close()
    for a in (film, xyz, pos):
        a.setflags(write=False)
    return dict(film=film, stats=st, pixels=pixels, xyz=xyz, pos=pos)


@pytest.fixture(scope="module")
def mixed_reference(oracle, abi, mixed_flat):
    """the twin's film and sample records of scene (c), computed once for every variant"""
    return twin_reference(oracle, abi, mixed_flat)


@pytest.fixture(scope="module")
def hbm_scenes(oracle, abi, hostmirror):
    """the two scenes whose per-triangle tables leave LDS, each with the twin's film and sample records, computed once"""
    out = {}
    for name, flat in (("big_blob", every_class_with_a_big_blob(hostmirror)), ("padded", every_class_padded(hostmirror))):
        out[name] = (flat, twin_reference(oracle, abi, flat))
    return out


@pytest.mark.gpu
def test_caustic_room_samples_and_films(gpu_ctx, abi, oracle, room_flat):
    """(a) per-sample records at 32 spp and whole films in both RNG modes (f: MSK_RNG_PCG_BLOCK runs k_path_serial_d, whose
    draw order skips the next-event pair at a delta hit)"""
    with Pair(abi, gpu_ctx, oracle, room_flat) as p:
        gx = p.samples_equal(some_pixels(64, 256, 1), "room", spp=32, seed=3)
        assert gx.max() > 0 and (gx.reshape(-1, 3)[:, 1] > 0).mean() > 0.5
        film, st = p.films_equal("room counter", spp=32, seed=3)
        assert st.samples == 64 * 64 * 32 and film[..., :3].max() > 0
        p.films_equal("room pcg", spp=16, seed=7, rng_mode=abi.MSK_RNG_PCG_BLOCK)
        p.films_equal("room pcg block 16", spp=8, seed=8, rng_mode=abi.MSK_RNG_PCG_BLOCK, block_size=16, rr_depth=2)


@pytest.mark.gpu
@pytest.mark.parametrize("int_ior", [1.5, 1.33])
def test_smooth_shaded_glass(gpu_ctx, abi, oracle, hostmirror, int_ior):
    """(b) interpolated shading normals on glass: si.wi.z from the shading frame, to_world of the refracted direction; the
    checkerboard behind the blob makes the direction decide the value"""
    flat = blob_room(hostmirror, int_ior)
    assert flat.desc.meshes[flat.desc.n_meshes - 1].has_normals == 1 and 100 < flat.desc.n_faces < 400
    with Pair(abi, gpu_ctx, oracle, flat) as p:
        centre = np.stack(np.meshgrid(np.arange(12, 36, 2), np.arange(14, 38, 2)), -1).reshape(-1, 2).astype(np.int32)      # on the blob
        p.samples_equal(centre, "blob", spp=32, seed=11)
        p.films_equal("blob", spp=16, seed=12)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "tables_in_hbm", "lds_scene_kb_0"])
def test_every_class_at_once(gpu_ctx, abi, oracle, hostmirror, mixed_flat, mixed_reference, monkeypatch, mode):
    """(c) every BSDF class in one scene with two area emitters and an environment, with the shading tables in LDS, with enough
    materials that they leave it (the construction of test_table_placement.py), and with the tree in HBM"""
    import test_table_placement as T
    flat, want = mixed_flat, mixed_reference
    if mode == "tables_in_hbm":
        flat = every_class_padded(hostmirror)
        plan = T.table_plan(flat)
        print("DIELECTRIC every class: table plan", plan)
        assert plan["table_f4"] == T.LDS_TABLES_F4 + 1 and not plan["lds_tables"]
        want = None
    if mode == "lds_scene_kb_0":
        monkeypatch.setenv("MSK_LDS_SCENE_KB", "0")
    with Pair(abi, gpu_ctx, oracle, flat) as p:
        if want is None:
            p.samples_equal(some_pixels(64, 128, 3), mode, spp=16, seed=5)
            film, _ = p.films_equal(mode, spp=16, seed=5)
        else:
            gx, gp = p.g.sample_pixels(abi.render_params(spp=16, seed=5), want["pixels"])
            assert np.array_equal(gp.view(np.uint32), want["pos"].view(np.uint32))
            assert np.array_equal(gx.view(np.uint32), want["xyz"].view(np.uint32)), mode
            film, _ = p.films_equal(mode, want=want["film"], spp=16, seed=5)
        assert film[..., :3].max() > 0
        p.films_equal(mode + " pcg", spp=8, seed=6, rng_mode=abi.MSK_RNG_PCG_BLOCK)        # (f)


@pytest.mark.gpu
@pytest.mark.parametrize("hide", [0, 1])
@pytest.mark.parametrize("env", [None, "env"])
def test_glass_that_emits(gpu_ctx, abi, oracle, hostmirror, hide, env):
    """(d) a mesh with a `dielectric` BSDF and a radiance: seen directly (or hidden), reached through a delta bounce (MIS weight
    1), and sampled by next-event estimation from the floor"""
    flat = emitting_glass(hostmirror, dict(ENV) if env else None)
    with Pair(abi, gpu_ctx, oracle, flat) as p:
        gx = p.samples_equal(some_pixels(48, 128, 5), "emitting glass", spp=32, seed=9, hide_emitters=hide)
        assert gx.max() > 0
        p.films_equal("emitting glass", spp=16, seed=10, hide_emitters=hide)
        p.films_equal("emitting glass pcg", spp=8, seed=10, hide_emitters=hide, rng_mode=abi.MSK_RNG_PCG_BLOCK)


@pytest.mark.gpu
def test_integrator_properties_with_glass(gpu_ctx, abi, oracle, room_flat):
    """(e) max_depth cutting a path inside glass, Russian roulette from the first bounce on with eta != 1 in q"""
    pixels = some_pixels(64, 96, 2)
    with Pair(abi, gpu_ctx, oracle, room_flat) as p:
        for max_depth in (1, 2, 3, 5, -1):
            for rr_depth in (1, 2, 5):
                p.samples_equal(pixels, "room", spp=16, seed=21, max_depth=max_depth, rr_depth=rr_depth)


VARIANTS = [{"MSK_FUSED": "1"}, {"MSK_SORT": "0", "MSK_STREAMS": "1"}, {"MSK_FUSED_TAIL_PCT": "50"},
            {"MSK_BVH_BUILD": "gpu"}, {"MSK_WIDE_BVH": "8"}, {"MSK_QUANT_BVH": "1"},
            {"MSK_LDS_SCENE_KB": "0", "MSK_FUSED": "1"},
            {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "8"}, {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "1", "MSK_BVH_BUILD": "gpu"}]
variant_id = lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items()))


def variant_equals(p, want, what):
    gx, gp = p.g.sample_pixels(p.abi.render_params(spp=16, seed=5), want["pixels"])
    assert np.array_equal(gp.view(np.uint32), want["pos"].view(np.uint32))
    assert np.array_equal(gx.view(np.uint32), want["xyz"].view(np.uint32)), what
    return p.films_equal(what, want=want["film"], spp=16, seed=5)


@pytest.mark.gpu
@pytest.mark.parametrize("env", VARIANTS, ids=variant_id)
def test_execution_variants_against_the_twin(gpu_ctx, abi, oracle, mixed_flat, mixed_reference, monkeypatch, env):
    """(g) scene (c), whose tables fit LDS, under the library's execution variants, each against the twin: with the tree in LDS
    (k_shade_gen_d<true>, and k_wavefront_d for the thin end or the whole pass) and, for the tree-shape knobs, with the tree in
    HBM, where they take effect.  MSK_FUSED_HBM does nothing to this scene: test_fused_hbm_variants_against_the_twin has it."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with Pair(abi, gpu_ctx, oracle, mixed_flat) as p:
        variant_equals(p, mixed_reference, str(env))


KNOBS = ("MSK_FUSED", "MSK_SORT", "MSK_STREAMS", "MSK_FUSED_HBM", "MSK_FUSED_TAIL_PCT", "MSK_BVH_BUILD", "MSK_WIDE_BVH", "MSK_QUANT_BVH")
SPLIT, FUSED_PART, FUSED_ALL, ANY = "split", "fused part", "fused all", "any"
# tree and per-triangle tables in HBM: msk_gpu.hip takes its fused_h path (k_wavefront_h_d) only there.  Per case: the scene, the
# knobs, and what msk_stats must show of the launches (launches_wavefront counts k_wavefront_h_d, launches_shade k_shade_gen_d<false>)
HBM_VARIANTS = [("big_blob", {"MSK_FUSED_HBM": "0"}, SPLIT),
                ("big_blob", {"MSK_FUSED_HBM": "1"}, ANY),                          # the default: the last 2 % of a pass
                ("big_blob", {"MSK_FUSED_TAIL_PCT": "50"}, FUSED_PART),
                ("big_blob", {"MSK_FUSED": "1"}, FUSED_ALL),
                ("big_blob", {"MSK_FUSED_HBM": "0", "MSK_FUSED": "1"}, SPLIT),
                ("big_blob", {"MSK_SORT": "0", "MSK_STREAMS": "1", "MSK_FUSED_TAIL_PCT": "50"}, FUSED_PART),
                ("big_blob", {"MSK_BVH_BUILD": "gpu", "MSK_FUSED": "1"}, FUSED_ALL),
                ("padded", {"MSK_FUSED_HBM": "0"}, SPLIT),
                ("padded", {"MSK_FUSED_TAIL_PCT": "50"}, FUSED_PART),
                ("padded", {"MSK_FUSED": "1"}, FUSED_ALL)]


def test_hbm_scenes_leave_lds(hostmirror):
    """the plan of the two scenes, by the library's formulas: tables out of LDS for both, the small ones staged only for the blob
    (where the tree lives is pinned by MSK_LDS_SCENE_KB=0 in the GPU test, as test_table_placement.py pins it)"""
    import test_table_placement as T
    big, padded = T.table_plan(every_class_with_a_big_blob(hostmirror)), T.table_plan(every_class_padded(hostmirror))
    print("DIELECTRIC table plans: big blob", big, "padded", padded)
    assert not big["lds_tables"] and big["small_staged"]
    assert not padded["lds_tables"] and not padded["small_staged"] and padded["table_f4"] == T.LDS_TABLES_F4 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,expect", HBM_VARIANTS, ids=lambda v: variant_id(v) if isinstance(v, dict) else str(v).replace(" ", "_"))
def test_fused_hbm_variants_against_the_twin(gpu_ctx, abi, oracle, hbm_scenes, monkeypatch, name, env, expect):
    """(g) k_wavefront_h_d and k_shade_gen_d<false> against the twin: scene (c) with a 480-triangle glass blob, and scene (c)
    padded, both with the tree in HBM (MSK_LDS_SCENE_KB=0: trace mode 6), under MSK_FUSED_HBM 0 and 1, MSK_FUSED=1,
    MSK_FUSED_TAIL_PCT=50 and the unsorted single-stream loop.  The launch counts show which kernels made the film."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MSK_LDS_SCENE_KB", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    flat, want = hbm_scenes[name]
    with Pair(abi, gpu_ctx, oracle, flat) as p:
        film, st = variant_equals(p, want, "%s %s" % (name, env))
    got = "trace %d shade %d wavefront %d" % (st.launches_trace, st.launches_shade, st.launches_wavefront)
    print("DIELECTRIC fused-HBM %s %s: %s" % (name, variant_id(env), got))
    assert film[..., :3].max() > 0 and st.samples == want["stats"].samples
    if expect == SPLIT:
        assert st.launches_wavefront == 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == FUSED_PART:
        assert st.launches_wavefront > 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == FUSED_ALL:
        assert st.launches_wavefront > 0 and st.launches_shade == 0 and st.launches_trace == 0, got


@pytest.mark.gpu
def test_shards_and_crop_window_with_glass(gpu_ctx, abi, oracle, hostmirror, mixed_flat):
    """(g) a sample shard, a tile shard and a crop window of scene (c), as test_gpu_parity.py does for the Cornell box"""
    with Pair(abi, gpu_ctx, oracle, mixed_flat) as p:
        p.films_equal("sample shard", spp=16, seed=5, sample_first=1, sample_stride=3)
        p.films_equal("sample range", spp=16, seed=5, sample_first=9, sample_stride=1)
        p.films_equal("tile shard", spp=16, seed=5, block_first=1, block_stride=2, block_size=16)
        p.samples_equal(some_pixels(64, 32, 4), "sample shard", spp=16, seed=5, sample_first=2, sample_stride=4)
        whole, _ = p.g.render(abi.render_params(spp=8, seed=5))
    crop = (9, 21, 37, 30)
    with Pair(abi, gpu_ctx, oracle, every_class(hostmirror, crop=crop)) as p:
        film, _ = p.films_equal("crop", spp=8, seed=5)
        assert film.shape == (30, 37, 5)
        assert np.array_equal(film.view(np.uint32), whole[21:51, 9:46].view(np.uint32))


@pytest.mark.gpu
def test_aov_integrator_with_glass(gpu_ctx, abi, oracle, room_flat):
    """(h) the "aov" integrator: the primary hit on glass gives the twin's channels, the nested path sample its XYZ"""
    A = abi
    with Pair(abi, gpu_ctx, oracle, room_flat) as p:
        prm = abi.render_params(8, seed=13)
        for types in ([A.MSK_AOV_DEPTH, A.MSK_AOV_POSITION, A.MSK_AOV_PATH_RGBA, A.MSK_AOV_GEO_NORMAL, A.MSK_AOV_UV, A.MSK_AOV_SH_NORMAL],
                      [A.MSK_AOV_SH_NORMAL, A.MSK_AOV_DEPTH]):
            film, _ = p.g.render_aov(prm, types)
            ref, _ = p.o.render_aov(prm, types)
            bad = film.view(np.uint32) != ref.view(np.uint32)
            assert film.shape == ref.shape and not bad.any(), (types, int(bad.sum()), np.argwhere(bad)[:4].tolist())
