"""float64 reference for the smooth `dielectric` BSDF (numpy only; an extension of radiometry_ref).

Written from the reference's render/fresnel.h:37-63 (the Fresnel term as the plugin computes it), bsdfs/dielectric.cpp:26-72
(lobe choice and weights) and integrators/path.cpp:116-122 (Russian roulette), and from the textbook forms of the same
quantities (the refracted direction: Snell's law in vector form).  It shares no arithmetic with csrc/, oracle/ or hostmirror.
"""
import numpy as np

import radiometry_ref as R


def fresnel(cos_theta_i, eta):
    """fresnel.h:37-63 in float64 -> (r, cos_theta_t, eta_it, eta_ti); cos_theta_i < 0: the ray arrives from the inside"""
    c = np.asarray(cos_theta_i, np.float64)
    eta = float(eta)
    outside = c >= 0.0
    eta_it = np.where(outside, eta, 1.0 / eta)
    eta_ti = np.where(outside, 1.0 / eta, eta)
    ct2 = 1.0 - eta_ti * eta_ti * (1.0 - c * c)
    ci = np.abs(c)
    ct = np.sqrt(np.maximum(ct2, 0.0))                       # math::safe_sqrt
    with np.errstate(invalid="ignore", divide="ignore"):
        a_s = (ci - eta_it * ct) / (ci + eta_it * ct)
        a_p = (ct - eta_it * ci) / (ct + eta_it * ci)
        r = 0.5 * (a_s * a_s + a_p * a_p)
    if eta == 1.0:
        r = np.zeros_like(c)
    else:
        r = np.where(ci == 0.0, 1.0, r)
    return r, ct * np.copysign(1.0, -c), eta_it, eta_ti


def reflectance(cos_theta_i, eta):
    return fresnel(cos_theta_i, eta)[0]


def fresnel_textbook(theta_i, n1, n2):
    """Unpolarised reflectance of the interface n1 -> n2 at incidence theta_i: Snell's law, then
    Rs = ((n1 cos i - n2 cos t) / (n1 cos i + n2 cos t))^2, Rp = ((n1 cos t - n2 cos i) / (n1 cos t + n2 cos i))^2; 1 under TIR"""
    theta_i = np.asarray(theta_i, np.float64)
    s = n1 / n2 * np.sin(theta_i)
    tir = s >= 1.0
    ct = np.sqrt(np.where(tir, 0.0, 1.0 - s * s))
    ci = np.cos(theta_i)
    rs = ((n1 * ci - n2 * ct) / (n1 * ci + n2 * ct)) ** 2
    rp = ((n1 * ct - n2 * ci) / (n1 * ct + n2 * ci)) ** 2
    return np.where(tir, 1.0, 0.5 * (rs + rp))


def transmittance_textbook(theta_i, n1, n2):
    """The transmitted share of the power: (n2 cos t) / (n1 cos i) (ts^2 + tp^2) / 2 with the amplitude coefficients
    ts = 2 n1 cos i / (n1 cos i + n2 cos t), tp = 2 n1 cos i / (n2 cos i + n1 cos t); 0 under TIR"""
    theta_i = np.asarray(theta_i, np.float64)
    s = n1 / n2 * np.sin(theta_i)
    tir = s >= 1.0
    ct = np.sqrt(np.where(tir, 0.0, 1.0 - s * s))
    ci = np.cos(theta_i)
    ts = 2.0 * n1 * ci / (n1 * ci + n2 * ct)
    tp = 2.0 * n1 * ci / (n2 * ci + n1 * ct)
    return np.where(tir, 0.0, (n2 * ct) / (n1 * ci) * 0.5 * (ts * ts + tp * tp))


def refract(d, n, eta):
    """Snell's law in float64, in vector form, knowing nothing of local frames.  d: unit directions of travel [..., 3]; n: the unit
    normal of the interface, pointing to the OUTSIDE (where the index is 1; the inside has `eta`).  With c = -d . n (> 0: the ray
    arrives from outside) and eta_ti = n_incident / n_transmitted, the refracted direction is
    t = eta_ti d + (eta_ti c' - sqrt(1 - eta_ti^2 (1 - c'^2))) n', with n' the normal on the ray's own side and c' = |c|
    -> (t [..., 3], tir [...] = total internal reflection: t is then the mirrored direction d + 2 c' n')"""
    d, n = np.asarray(d, np.float64), np.asarray(n, np.float64)
    c = -(d @ n)
    outside = c >= 0.0
    eta_ti = np.where(outside, 1.0 / float(eta), float(eta))
    ns = np.where(outside[..., None], n, -n)
    ca = np.abs(c)
    ct2 = 1.0 - eta_ti * eta_ti * (1.0 - ca * ca)
    tir = ct2 <= 0.0
    ct = np.sqrt(np.maximum(ct2, 0.0))
    t = eta_ti[..., None] * d + (eta_ti * ca - ct)[..., None] * ns
    return np.where(tir[..., None], d + 2.0 * ca[..., None] * ns, t), tir


def refract_local(wi, eta):
    """The same in the BSDF's local frame (normal = +z, wi pointing AWAY from the surface, as the plugin sees it): Snell's law
    sin_t = eta_ti sin_i in the plane of incidence, on the other side -> (wo [..., 3], cos_t (signed), eta_it, eta_ti, tir)"""
    wi = np.asarray(wi, np.float64)
    t, tir = refract(-wi, np.array([0.0, 0.0, 1.0]), eta)
    outside = wi[..., 2] >= 0.0
    return t, t[..., 2], np.where(outside, float(eta), 1.0 / float(eta)), np.where(outside, 1.0 / float(eta), float(eta)), tir


def critical_angle(eta):
    return np.arcsin(1.0 / eta)


def slab_series(r, terms):
    """A lossless slab seen from outside: the light that comes back after 0, 1, 2, ... pairs of internal reflections and the
    light that passes, as partial sums of `terms` terms -> (reflected, transmitted).  R + T^2 R (1 + R^2 + ...) and
    T^2 (1 + R^2 + ...): together T^2 / (1 - R) + R = 1."""
    r = np.asarray(r, np.float64)
    t = 1.0 - r
    k = np.arange(int(terms)).reshape((-1,) + (1,) * r.ndim)
    geo = (r[None] ** (2 * k)).sum(0)
    return r + t * t * r * geo, t * t * geo


def slab_roulette_moments(r, q=0.95):
    """The slab under Russian roulette from the first bounce on (rr_depth 2), in a constant environment of radiance L, in units
    of L.  A camera ray reflects off the first face with probability R (value 1, no roulette: the reflected ray leaves the
    scene) or enters (T).  Inside, the throughput times eta^2 is 1 or more, so every segment that ends on a face survives with
    probability q and is divided by q (path.cpp:116-122); it then leaves (T) or is reflected once more (R).  A path that
    leaves after k segments inside has the value q^-k and the probability T^2 R^(k-1) q^k.
    -> (mean, second moment): the mean is R + T^2 / (1 - R) = 1; the second moment R + (T^2 / q) / (1 - R / q), finite for R < q."""
    r = np.asarray(r, np.float64)
    assert np.all(r < q)
    t = 1.0 - r
    mean = r + t * t / (1.0 - r)
    second = r + (t * t / q) / (1.0 - r / q)
    return mean, second


def wavelength_sample_moments(spectrum, cie, m=16):
    """Mean and variance, per channel, of the XYZ of ONE camera sample that sees spectral radiance S with certainty: the only
    random input is the wavelength sample u.  The four wavelengths of a sample are those of u, u + 1/4, u + 1/2, u + 3/4 (mod 1)
    and spectrum_to_xyz takes the mean of the four terms (core/spectrum.h:164-181), so the sample is g(u) = 1/4 sum_q f(u + q/4)
    with f = S w cmf at lambda(u).  Composite Gauss-Legendre on [0, 1/4] (g has that period), panels split at every kink of f
    and of its three shifted copies.  -> (mean[3], variance[3])"""
    lam_breaks = np.concatenate([np.linspace(R.CIE_MIN, R.CIE_MAX, R.CIE_SAMPLES), np.asarray(spectrum.breaks, np.float64)])
    ub = R._u_of(lam_breaks)
    ub = ub[(ub > 0.0) & (ub < 1.0)]
    ub = np.unique(np.concatenate([[0.0, 0.25], np.mod(ub, 0.25)]))

    def f(u):
        lam = R.wavelength_of(u)
        return R.cmf(cie, lam) * (spectrum(lam) * R.wavelength_weight(lam))

    m1, m2 = np.zeros(3), np.zeros(3)
    for a, b in zip(ub[:-1], ub[1:]):
        u, w = R.gauss_legendre(m, a, b)
        g = 0.25 * (f(u) + f(u + 0.25) + f(u + 0.5) + f(u + 0.75))
        m1 += (g * w).sum(-1)
        m2 += (g * g * w).sum(-1)
    m1, m2 = 4.0 * m1, 4.0 * m2                              # the density of u on a quarter of its range
    return m1, m2 - m1 * m1


def incidence_cosines(desc, pos, normal=(0.0, 1.0, 0.0)):
    """cos(theta_i) of the camera rays through the film positions pos[..., 2] (pixels) on a plane with `normal`: -d . n"""
    _, d = R.camera_ray(desc, pos[..., 0], pos[..., 1])
    return -(d @ np.asarray(normal, np.float64))
