"""The `roughplastic` BSDF (include/msk_gpu.h at MSK_BSDF_ROUGHPLASTIC) restated twice, sharing nothing with the code under test.

fp32 side (ggx_sample32, eval32, sample32): numpy float32, one IEEE operation per line, in the order the header and the device
functions it names (sample_ggx, distr_eval, smith_g1, normalized, dot) give.  The plastic's parts (fresnel32, lobes32, the diffuse
base) come from plastic_ref; what varies with the wavelength (rho, s) and the cosine-hemisphere direction come in as arrays; the
three deterministic transcendentals of sample_ggx come from the oracle binding's det_math / det_math2 hooks, as envmap_ref takes them.

float64 side: the same BSDF from the textbook forms, its sampling routine, the hemispherical integrals of eval and pdf by a
panelled tensor Gauss-Legendre rule in (theta, phi), the coat's mass below the horizon by a rule over the microfacet normal, and
the reference's `sample_visible = true` density (roughplastic.cpp:144-146), which the tests show to be biased.
"""
import numpy as np

import envmap_ref as ER
import plastic_ref as P
import radiometry_ref as R

F = np.float32
PI = F(3.14159274101257324)
INV_PI = P.INV_PI
TWO_PI = F(F(2) * PI)


def clamp_alpha(a):
    return max(F(a), F(1e-4))


# ----------------------------------------------------------------------------- fp32
def dot32(a, b):
    """msk_device.h dot: a.x b.x + (a.y b.y + a.z b.z)"""
    t = ((a[:, 1] * b[:, 1]).astype(F) + (a[:, 2] * b[:, 2]).astype(F)).astype(F)
    return ((a[:, 0] * b[:, 0]).astype(F) + t).astype(F)


def normalized32(a):
    z = dot32(a, a)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = (a / np.sqrt(z).astype(F)[:, None]).astype(F)
    return np.where((z > 0)[:, None], n, a).astype(F)


def det_tan(oracle, x):
    return ER._each(oracle.lib.msk_oracle_det_math2, x, 2, (1,))[0]


def ggx_sample32(oracle, u, a):
    """sample_ggx(u, a, a): -> (m float32 [n, 3], pm float32 [n])"""
    u, a = np.asarray(u, F), F(a)
    x, y = u[:, 0], u[:, 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = det_tan(oracle, (PI + (TWO_PI * y).astype(F)).astype(F))
        phi = (ER.det_atan(oracle, (F(a / a) * t).astype(F)) + (PI * np.floor(((F(2) * y).astype(F) + F(0.5)).astype(F))).astype(F)).astype(F)
        s, c = ER.det_sincos(oracle, phi)
        cs, sn = (c / a).astype(F), (s / a).astype(F)
        alpha_sqr = (F(1) / ((cs * cs).astype(F) + (sn * sn).astype(F)).astype(F)).astype(F)
        tan2 = ((alpha_sqr * x).astype(F) / (F(1) - x).astype(F)).astype(F)
        cos_m = (F(1) / np.sqrt((F(1) + tan2).astype(F)).astype(F)).astype(F)
        tmp = (F(1) + (tan2 / alpha_sqr).astype(F)).astype(F)
        den = F(a * a)
        for k in (cos_m, cos_m, cos_m, tmp, tmp):
            den = (den * k).astype(F)
        pm = (INV_PI / den).astype(F)
        pm = np.where(pm < F(1e-20), F(0), pm).astype(F)
        sin_m = np.sqrt(np.maximum((F(1) - (cos_m * cos_m).astype(F)).astype(F), F(0))).astype(F)
    return np.stack([(sin_m * c).astype(F), (sin_m * s).astype(F), cos_m], -1).astype(F), pm


def distr32(m, a):
    """distr_eval(m, a, a)"""
    a = F(a)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cos2 = (m[:, 2] * m[:, 2]).astype(F)
        aa = F(a * a)
        b = ((((m[:, 0] * m[:, 0]).astype(F) / aa).astype(F) + ((m[:, 1] * m[:, 1]).astype(F) / aa).astype(F)).astype(F) / cos2).astype(F)
        root = ((F(1) + b).astype(F) * cos2).astype(F)
        den = ((F(F(PI * a) * a) * root).astype(F) * root).astype(F)
        r = (F(1) / den).astype(F)
        live = (m[:, 2] > 0) & ((r * m[:, 2]).astype(F) > F(1e-20))
    return np.where(live, r, F(0)).astype(F)


def smith32(v, m, a):
    """smith_g1(v, m, a, a)"""
    a = F(a)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ax, ay = (a * v[:, 0]).astype(F), (a * v[:, 1]).astype(F)
        xy = ((ax * ax).astype(F) + (ay * ay).astype(F)).astype(F)
        tan2 = (xy / (v[:, 2] * v[:, 2]).astype(F)).astype(F)
        g = (F(2) / (F(1) + np.sqrt((F(1) + tan2).astype(F)).astype(F)).astype(F)).astype(F)
        dead = (dot32(v, m) * v[:, 2]).astype(F) <= 0
    return np.where(xy == 0, F(1), np.where(dead, F(0), g)).astype(F)


def eval32(wi, wo, rho, s, eta, inv_eta, fdr_int, ssw, nonlinear, alpha):
    """-> (eval float32 [n, 4], pdf float32 [n]); rho, s float32 [n, 4]"""
    wi, wo, s = np.asarray(wi, F), np.asarray(wo, F), np.asarray(s, F)
    a = clamp_alpha(alpha)
    ok, f_i, ps, pd = P.lobes32(wi[:, 2], eta, ssw)
    ok = ok & (wo[:, 2] > 0)
    base, pdf_d = P.eval32(wi, wo, rho, eta, inv_eta, fdr_int, ssw, nonlinear)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        h = normalized32((wo + wi).astype(F))
        d = distr32(h, a)
        g = (smith32(wi, h, a) * smith32(wo, h, a)).astype(F)
        f_h = P.fresnel32(dot32(wi, h), eta)
        c = (((f_h * d).astype(F) * g).astype(F) / (F(4) * wi[:, 2]).astype(F)).astype(F)
        val = ((s * c[:, None]).astype(F) + base).astype(F)
        p_s = ((d * h[:, 2]).astype(F) / (F(4) * dot32(wo, h)).astype(F)).astype(F)
        p_s = np.where(d == 0, F(0), p_s).astype(F)
        pdf = ((ps * p_s).astype(F) + pdf_d).astype(F)
    return np.where(ok[:, None], val, F(0)).astype(F), np.where(ok, pdf, F(0)).astype(F)


def sample32(oracle, wi, sample1, u, hemi, rho, s, eta, inv_eta, fdr_int, ssw, nonlinear, alpha):
    """u float32 [n, 2]; hemi float32 [n, 3] = square_to_cosine_hemisphere(u) -> dict(wo, pdf, value, coat, ok); eta is 1, never delta"""
    wi, hemi, s1 = np.asarray(wi, F), np.asarray(hemi, F), np.asarray(sample1, F)
    a = clamp_alpha(alpha)
    ok, f_i, ps, pd = P.lobes32(wi[:, 2], eta, ssw)
    coat = ok & (s1 < ps)
    m, pm = ggx_sample32(oracle, u, a)
    with np.errstate(invalid="ignore", over="ignore"):
        k = dot32(wi, m)
        refl = (((m * F(2)).astype(F) * k[:, None]).astype(F) - wi).astype(F)
    wo = np.where(coat[:, None], refl, hemi).astype(F)
    wo[~ok] = 0
    dead = coat & ((pm == 0) | (wo[:, 2] <= 0))
    ev, pdf = eval32(wi, wo, rho, s, eta, inv_eta, fdr_int, ssw, nonlinear, alpha)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        val = (ev / pdf[:, None]).astype(F)
    live = ok & ~dead & (pdf > 0)
    return dict(wo=wo, pdf=np.where(ok & ~dead, pdf, F(0)).astype(F), value=np.where(live[:, None], val, F(0)).astype(F), coat=coat, ok=ok)


# ----------------------------------------------------------------------------- float64: the BSDF
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def ggx_d64(cos_m, a):
    c2 = cos_m * cos_m
    return a * a / (np.pi * (c2 * (a * a - 1.0) + 1.0) ** 2)


def smith64(cos_v, a):
    """G1 of GGX for a direction at cos_v > 0, in the form that stays finite at the horizon"""
    c = np.clip(cos_v, 0.0, 1.0)
    return 2.0 * c / (c + np.sqrt(c * c + a * a * (1.0 - c * c)))


def lobes64(cos_i, eta, ssw):
    f_i = P.fresnel64(cos_i, eta)
    ps, pd = f_i * ssw, (1.0 - f_i) * (1.0 - ssw)
    ps = ps / (ps + pd)
    return f_i, ps, 1.0 - ps


def eval64(wi, wo, rho, s, eta, alpha, nonlinear):
    """value with its cosine, for wi, wo float64 [..., 3] on the front side"""
    a = max(float(alpha), 1e-4)
    h = _unit(wi + wo)
    ci, co = wi[..., 2], wo[..., 2]
    spec = P.fresnel64(np.clip((wi * h).sum(-1), 0.0, 1.0), eta) * ggx_d64(h[..., 2], a) * smith64(ci, a) * smith64(co, a) / (4.0 * ci)
    return s * spec + P.eval64(ci, co, rho, eta, nonlinear)


def pdf64(wi, wo, eta, alpha, ssw, visible=False):
    """the mixture density; visible: the reference's density under sample_visible = true (roughplastic.cpp:144-146)"""
    a = max(float(alpha), 1e-4)
    _, ps, pd = lobes64(wi[..., 2], eta, ssw)
    h = _unit(wi + wo)
    d = ggx_d64(h[..., 2], a)
    p_s = d * smith64(wi[..., 2], a) / (4.0 * wi[..., 2]) if visible else d * h[..., 2] / (4.0 * (wo * h).sum(-1))
    return ps * p_s + pd * wo[..., 2] / np.pi


def sample_weights64(cos_i, rho, s, eta, alpha, ssw, nonlinear, log2_n=20, seed=1, visible=False):
    """sample() at 2^log2_n stratified (sample1, u.x, u.y), jittered: -> weights eval / pdf float64 [n] (0 where the sample fails)"""
    n1 = 1 << (log2_n // 3)
    n2 = 1 << ((log2_n - log2_n // 3) // 2)
    n3 = (1 << log2_n) // (n1 * n2)
    rng = np.random.RandomState(seed)
    i, j, k = np.meshgrid(np.arange(n1), np.arange(n2), np.arange(n3), indexing="ij")
    s1 = ((i + rng.uniform(size=i.shape)) / n1).ravel()
    ux = ((j + rng.uniform(size=i.shape)) / n2).ravel()
    uy = ((k + rng.uniform(size=i.shape)) / n3).ravel()
    a = max(float(alpha), 1e-4)
    wi = np.array([np.sqrt(1.0 - cos_i * cos_i), 0.0, cos_i])
    _, ps, _ = lobes64(cos_i, eta, ssw)
    phi = 2.0 * np.pi * uy
    tan2 = a * a * ux / (1.0 - ux)
    cm = 1.0 / np.sqrt(1.0 + tan2)
    sm = np.sqrt(np.maximum(1.0 - cm * cm, 0.0))
    m = np.stack([sm * np.cos(phi), sm * np.sin(phi), cm], -1)
    coat_wo = 2.0 * (m @ wi)[:, None] * m - wi
    r, ph = np.sqrt(ux), 2.0 * np.pi * uy                                  # a cosine-weighted direction: the warp itself is not under test
    base_wo = np.stack([r * np.cos(ph), r * np.sin(ph), np.sqrt(np.maximum(1.0 - ux, 0.0))], -1)
    coat = s1 < ps
    wo = np.where(coat[:, None], coat_wo, base_wo)
    live = wo[:, 2] > 1e-300
    wo_l = wo[live]
    w = np.zeros(len(wo))
    w[live] = eval64(wi, wo_l, rho, s, eta, a, nonlinear) / pdf64(wi, wo_l, eta, a, ssw, visible)
    return w


def hemisphere_rule(order, panels_theta=64, panels_phi=64):
    """panelled tensor Gauss-Legendre nodes over the upper hemisphere in (theta, phi); phi over [0, pi], doubled (the integrands are
    even in phi for wi in the xz plane): -> (wo float64 [n, 3], weights float64 [n]) with the solid angle's sin(theta) inside"""
    th, wt = zip(*(R.gauss_legendre(order, 0.5 * np.pi * k / panels_theta, 0.5 * np.pi * (k + 1) / panels_theta) for k in range(panels_theta)))
    ph, wp = zip(*(R.gauss_legendre(order, np.pi * k / panels_phi, np.pi * (k + 1) / panels_phi) for k in range(panels_phi)))
    th, wt, ph, wp = (np.concatenate(x) for x in (th, wt, ph, wp))
    t, p = np.meshgrid(th, ph, indexing="ij")
    w = (wt * np.sin(th))[:, None] * (2.0 * wp)[None, :]
    return np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], -1).reshape(-1, 3), w.ravel()


def albedo64(cos_i, rho, s, eta, alpha, nonlinear, order=12, panels=64):
    """the integral of eval over the hemisphere"""
    wi = np.array([np.sqrt(1.0 - cos_i * cos_i), 0.0, cos_i])
    wo, w = hemisphere_rule(order, panels, panels)
    return float((w * eval64(wi, wo, rho, s, eta, alpha, nonlinear)).sum())


def pdf_mass64(cos_i, eta, alpha, ssw, order=12, visible=False):
    wi = np.array([np.sqrt(1.0 - cos_i * cos_i), 0.0, cos_i])
    wo, w = hemisphere_rule(order)
    return float((w * pdf64(wi, wo, eta, alpha, ssw, visible)).sum())


def coat_mass_below64(cos_i, alpha, panels=65536, order=8):
    """the probability that the coat's sampled direction lies below the horizon: over the microfacet normal m, density D(m) cos(theta_m);
    at a given theta_m the reflected wo.z = 2 (wi . m) m.z - wi.z is positive for cos(phi_m) > kappa = cos_i (1 - 2 cm^2) / (2 cm si sm)"""
    a = max(float(alpha), 1e-4)
    si = np.sqrt(1.0 - cos_i * cos_i)
    x, w = R.gauss_legendre(order, 0.0, 1.0)
    edges = np.linspace(0.0, 0.5 * np.pi, panels + 1)
    th = (edges[:-1, None] + (edges[1:] - edges[:-1])[:, None] * x[None, :]).ravel()
    wt = ((edges[1:] - edges[:-1])[:, None] * w[None, :]).ravel()
    cm, sm = np.cos(th), np.sin(th)
    kappa = cos_i * (1.0 - 2.0 * cm * cm) / (2.0 * cm * si * sm)
    above = np.arccos(np.clip(kappa, -1.0, 1.0)) / np.pi                # the fraction of phi_m with wo.z > 0
    return float((wt * ggx_d64(cm, a) * cm * sm * 2.0 * np.pi * (1.0 - above)).sum())
