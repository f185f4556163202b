"""float64 closed forms of the radiometric integrals the path integrator estimates (numpy only).

An independent restatement: written from the formulas of the reference (render/fresnel.h:65-88, render/microfacet.h:11-18,
150-170, core/spectrum.h:82-181, render/srgb.h:8-19, sensors/perspective.cpp:26-40, integrators/path.cpp:33-123) and from
textbook radiometry.  It shares no arithmetic with oracle/, csrc/ or hostmirror: it reads DATA out of the scene descriptor
(camera matrices, CIE / D65 tables, spectrum coefficients, regular tables) and nothing else.

Spectra are callables `S(lambda)` on float64 arrays with an attribute `breaks` = the wavelengths at which they have a kink
(the quadrature over the wavelength sample is split there).  Every quadrature takes its node count as an argument, so a
caller can evaluate it at m and 2m and carry the difference into its tolerance.
"""
import numpy as np

CIE_MIN, CIE_MAX, CIE_SAMPLES = 360.0, 830.0, 95          # core/spectrum.h:71-73
_A, _B, _C = 0.8569106254698279, 1.8275019724092267, 138.88888888888889      # core/spectrum.h:157-162


def gauss_legendre(m, a=0.0, b=1.0):
    x, w = np.polynomial.legendre.leggauss(int(m))
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w


# ----------------------------------------------------------------------------- spectra
class Spectrum:
    def __init__(self, fn, breaks=()):
        self.fn, self.breaks = fn, tuple(float(b) for b in breaks)

    def __call__(self, lam):
        return self.fn(np.asarray(lam, np.float64))

    def __mul__(self, other):
        if np.isscalar(other):
            return Spectrum(lambda l: self(l) * float(other), self.breaks)
        return Spectrum(lambda l: self(l) * other(l), self.breaks + other.breaks)

    def __truediv__(self, other):
        return Spectrum(lambda l: self(l) / other(l), self.breaks + other.breaks)

    def map(self, f):
        """f applied to the values: e.g. rho -> 1 / (1 - rho)"""
        return Spectrum(lambda l: f(self(l)), self.breaks)


def constant(v):
    return Spectrum(lambda l: np.full_like(l, float(v)))


def regular(lambda_min, lambda_max, values):
    """spectra/regular.cpp: piecewise linear through equidistant samples; the grid must cover 360 .. 830"""
    v = np.asarray(values, np.float64)
    assert lambda_min <= CIE_MIN and lambda_max >= CIE_MAX and len(v) >= 2
    grid = np.linspace(float(lambda_min), float(lambda_max), len(v))
    return Spectrum(lambda l: np.interp(l, grid, v), grid)


def srgb_d65(coeff, d65_table, d65_scale):
    """srgb_d65.cpp:13-31 + srgb.h:8-19: sigmoid polynomial times the D65 table (d65.cpp:36-48: regular, 360 .. 830) times the scale"""
    c0, c1, c2 = (float(c) for c in coeff)
    d65 = regular(CIE_MIN, CIE_MAX, d65_table)

    def s(l):
        if np.isinf(c2):
            return np.full_like(l, 1.0 if c2 > 0 else 0.0)
        x = (c0 * l + c1) * l + c2
        return 0.5 + x / (2.0 * np.sqrt(1.0 + x * x))
    return Spectrum(lambda l: s(l) * d65(l) * float(d65_scale), d65.breaks)


# ----------------------------------------------------------------------------- wavelengths -> XYZ
def wavelength_of(u):
    return 538.0 - np.arctanh(_A - _B * u) * _C


def wavelength_weight(lam):
    return 253.82 * np.cosh(0.0072 * (lam - 538.0)) ** 2


def _u_of(lam):
    return (_A - np.tanh((538.0 - lam) / _C)) / _B


def cmf(cie, lam):
    """core/spectrum.h:82-107: the three tables (X | Y | Z, 95 entries each) linearly interpolated, index clamped to 0 .. 93"""
    t = np.asarray(cie, np.float64).reshape(3, CIE_SAMPLES)
    x = (lam - CIE_MIN) * ((CIE_SAMPLES - 1) / (CIE_MAX - CIE_MIN))
    i0 = np.clip(np.floor(x).astype(np.int64), 0, CIE_SAMPLES - 2)
    w1 = x - i0
    return t[:, i0] * (1.0 - w1) + t[:, i0 + 1] * w1


def expected_xyz(spectrum, cie, m=16):
    """E[XYZ] of one camera sample that sees spectral radiance S: the integral over the wavelength sample u in [0, 1] of
    S(lambda(u)) weight(lambda(u)) cmf(lambda(u)) (each of the four shifted wavelengths is uniform in u and spectrum_to_xyz takes
    their mean).  Composite Gauss-Legendre, m nodes per panel, panels split where the CIE tables or S have a kink."""
    lam_breaks = np.concatenate([np.linspace(CIE_MIN, CIE_MAX, CIE_SAMPLES), np.asarray(spectrum.breaks, np.float64)])
    ub = _u_of(lam_breaks)
    ub = np.unique(np.concatenate([[0.0, 1.0], ub[(ub > 0.0) & (ub < 1.0)]]))
    total = np.zeros(3)
    for a, b in zip(ub[:-1], ub[1:]):
        u, w = gauss_legendre(m, a, b)
        lam = wavelength_of(u)
        total += (cmf(cie, lam) * (spectrum(lam) * wavelength_weight(lam) * w)).sum(-1)
    return total


def unit_xyz(cie, m=16):
    return expected_xyz(constant(1.0), cie, m)


# ----------------------------------------------------------------------------- camera
def camera_ray(desc, x, y):
    """perspective.cpp:26-40: near-plane point of film position (x, y) in pixels, normalised, rotated to the world.
    x, y: float64 arrays -> (origin[3], directions[..., 3])"""
    s2c = np.array(desc.camera.sample_to_camera[:], np.float64).reshape(4, 4)
    tw = np.array(desc.camera.to_world[:], np.float64).reshape(4, 4)
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    p = np.stack([x, y, np.zeros_like(x), np.ones_like(x)], -1) @ s2c.T
    near = p[..., :3] / p[..., 3:]
    d = near / np.linalg.norm(near, axis=-1, keepdims=True)
    return tw[:3, 3].copy(), d @ tw[:3, :3].T


def pixel_mean(fn, desc, px, py, m):
    """The mean of fn(origin, directions) over an m x m midpoint grid of pixel (px, py)'s unit square"""
    t = (np.arange(m) + 0.5) / m
    yy, xx = np.meshgrid(py + t, px + t, indexing="ij")
    o, d = camera_ray(desc, xx, yy)
    return np.mean(fn(o, d), axis=(0, 1))


def pixel_gauss(fn, desc, px, py, m):
    """The same mean by an m x m Gauss-Legendre rule: for integrands that are expensive and smooth"""
    t, w = gauss_legendre(m)
    yy, xx = np.meshgrid(py + t, px + t, indexing="ij")
    o, d = camera_ray(desc, xx, yy)
    return float((w[:, None] * w[None, :] * fn(o, d)).sum())


def shading_frame(n):
    """The frame of a flat-shaded mesh hit: s = the first tangent of coordinate_system(n) (core/mathutils.h:186-194) made
    orthogonal to n and normalised, t = n x s (render/interaction.h:55-60) -> (s, t, n)"""
    n = np.asarray(n, np.float64)
    n = n / np.linalg.norm(n)
    sign = np.copysign(1.0, n[2])
    a = -1.0 / (sign + n[2])
    s = np.array([1.0 + sign * n[0] * n[0] * a, sign * n[0] * n[1] * a, -sign * n[0]])
    s = s - n * (n @ s)
    s /= np.linalg.norm(s)
    return s, np.cross(n, s), n


def hit_plane(o, d, point, normal):
    """The points where the rays o + t d meet the plane through `point` with `normal`"""
    n = np.asarray(normal, np.float64)
    t = ((np.asarray(point, np.float64) - o) @ n) / (d @ n)
    assert np.all(t > 0)
    return o + d * t[..., None]


# ----------------------------------------------------------------------------- surfaces
def polygon_irradiance(x, n, vertices):
    """Lambert's formula: the integral of cos(theta) over the solid angle a polygon subtends at x (receiver normal n),
    E = 1/2 sum_i angle(r_i, r_i+1) (normalize(r_i x r_i+1) . n), for a polygon fully above the receiver's horizon.
    x: [..., 3].  The sign of the sum is the polygon's winding seen from x; the magnitude is returned."""
    x = np.asarray(x, np.float64)
    v = np.asarray(vertices, np.float64)
    r = v[:, None] - x.reshape(1, -1, 3)                          # [k, N, 3]
    assert np.all(r @ np.asarray(n, np.float64) > 0), "polygon not above the horizon"
    r /= np.linalg.norm(r, axis=-1, keepdims=True)
    total = np.zeros(r.shape[1])
    for i in range(len(v)):
        a, b = r[i], r[(i + 1) % len(v)]
        c = np.cross(a, b)
        s = np.linalg.norm(c, axis=-1)
        gamma = np.arctan2(s, (a * b).sum(-1))
        total += gamma * ((c / s[:, None]) @ np.asarray(n, np.float64))
    return np.abs(0.5 * total).reshape(x.shape[:-1])


def furnace(le, rho, max_depth):
    """Radiance inside a closed enclosure whose every surface emits le and reflects rho: path.cpp:33-49 adds the emission seen
    by the camera ray and one reflection per depth below max_depth, le * sum_{k < max_depth} rho^k (the series for -1)."""
    if max_depth < 0:
        return le / (1.0 - rho)
    return le * sum(rho ** k for k in range(max_depth))


def fresnel_conductor(cos_i, eta, k):
    """Unpolarised Fresnel reflectance of a conductor with index eta + i k (fresnel.h:65-88), textbook form"""
    c2 = cos_i * cos_i
    s2 = 1.0 - c2
    t1 = eta * eta - k * k - s2
    a2pb2 = np.sqrt(t1 * t1 + 4.0 * eta * eta * k * k)
    a = np.sqrt(0.5 * (a2pb2 + t1))
    rs = (a2pb2 + c2 - 2.0 * cos_i * a) / (a2pb2 + c2 + 2.0 * cos_i * a)
    rp = rs * (a2pb2 * c2 + s2 * s2 - 2.0 * cos_i * a * s2) / (a2pb2 * c2 + s2 * s2 + 2.0 * cos_i * a * s2)
    return 0.5 * (rs + rp)


def ggx_d(mx, my, mz, au, av):
    """GGX normal distribution (microfacet.h:11-18)"""
    return 1.0 / (np.pi * au * av * ((mx / au) ** 2 + (my / av) ** 2 + mz * mz) ** 2)


def smith_g1_ggx(vx, vy, vz, au, av):
    """Smith's separable shadowing term for GGX (microfacet.h:150-170), for v on the upper side"""
    return 2.0 / (1.0 + np.sqrt(1.0 + ((au * vx) ** 2 + (av * vy) ** 2) / (vz * vz)))


def ggx_conductor_albedo(cos_i, alpha, eta, k, m, phi_i=0.0):
    """Directional albedo of a rough conductor: tensor Gauss-Legendre over (cos_o, phi_o) of F(wi.h) D(h) G1(wi) G1(wo) / (4 cos_i)
    = f(wi, wo) cos_o.  alpha: a scalar or (alpha_u, alpha_v); wi = (sin_i cos phi_i, sin_i sin phi_i, cos_i) in the shading frame."""
    au, av = (alpha, alpha) if np.isscalar(alpha) else alpha
    si = np.sqrt(1.0 - cos_i * cos_i)
    wi = np.array([si * np.cos(phi_i), si * np.sin(phi_i), cos_i])
    c, wc = gauss_legendre(m, 0.0, 1.0)
    p, wp = gauss_legendre(2 * m, 0.0, 2.0 * np.pi)
    c, p = c[:, None], p[None, :]
    s = np.sqrt(1.0 - c * c)
    ox, oy, oz = s * np.cos(p), s * np.sin(p), c + 0.0 * p
    hx, hy, hz = ox + wi[0], oy + wi[1], oz + wi[2]
    hn = np.sqrt(hx * hx + hy * hy + hz * hz)
    hx, hy, hz = hx / hn, hy / hn, hz / hn
    f = fresnel_conductor(wi[0] * hx + wi[1] * hy + wi[2] * hz, eta, k) * ggx_d(hx, hy, hz, au, av) * \
        smith_g1_ggx(wi[0], wi[1], wi[2], au, av) * smith_g1_ggx(ox, oy, oz, au, av) / (4.0 * cos_i)
    return float(wc @ f @ wp)


def ggx_conductor_as_written(cos_i, alpha, eta, k, m, phi_i=0.0, light_pdf=0.0):
    """What the reference's path integrator has for its expectation when the lobe is lit by a light that is sampled with the
    constant solid-angle density light_pdf (a uniform environment: 1 / 4 pi; 0: BSDF sampling alone).

    microfacet.h:23-26 draws the azimuth of the half vector from tan(phi) = alpha_u / alpha_v tan(2 pi u), where the density
    D(m) cos(theta_m) it then reports as the pdf needs alpha_v / alpha_u.  The polar angle is drawn correctly for the azimuth,
    so half vectors come with the density r(phi_m) D cos, r = (alpha_v^2 cos^2 + alpha_u^2 sin^2) / (alpha_u^2 cos^2 + alpha_v^2
    sin^2), while the weight f cos / pdf and the power-heuristic weights use D cos.  Light sampling plus BSDF sampling then add
    up to the integral of f cos (p_l^2 + r p_b^2) / (p_l^2 + p_b^2), p_b = D cos(theta_m) / (4 wo.m); r == 1 for an isotropic
    lobe, which gives the albedo back.  r is not continuous at m = n as a function of wo, so this is integrated over the half
    vector instead, d wo = 4 (wi.m) d m: Gauss-Legendre over phi_m and over theta_m up to where wo reaches the horizon,
    2 theta_m = pi / 2 + atan(tan(theta_i) cos(phi_m - phi_i))."""
    au, av = (alpha, alpha) if np.isscalar(alpha) else alpha
    si = np.sqrt(1.0 - cos_i * cos_i)
    wi = np.array([si * np.cos(phi_i), si * np.sin(phi_i), cos_i])
    p, wp = gauss_legendre(2 * m, 0.0, 2.0 * np.pi)
    t, wt = gauss_legendre(m, 0.0, 1.0)
    tmax = 0.25 * np.pi + 0.5 * np.arctan2(si * np.cos(p - phi_i), cos_i)
    th = t[:, None] * tmax[None, :]
    hx, hy, hz = np.sin(th) * np.cos(p), np.sin(th) * np.sin(p), np.cos(th)
    wh = wi[0] * hx + wi[1] * hy + wi[2] * hz
    ox, oy, oz = 2.0 * wh * hx - wi[0], 2.0 * wh * hy - wi[1], 2.0 * wh * hz - wi[2]
    assert oz.min() > 0 and wh.min() > 0
    d = ggx_d(hx, hy, hz, au, av)
    f = fresnel_conductor(wh, eta, k) * d * smith_g1_ggx(wi[0], wi[1], wi[2], au, av) * smith_g1_ggx(ox, oy, oz, au, av) / (4.0 * cos_i)
    cp2, sp2 = np.cos(p) ** 2, np.sin(p) ** 2
    r = (av * av * cp2 + au * au * sp2) / (au * au * cp2 + av * av * sp2)
    pb2, pl2 = (d * hz / (4.0 * wh)) ** 2, float(light_pdf) ** 2
    f = f * (pl2 + r * pb2) / (pl2 + pb2) * 4.0 * wh * np.sin(th)
    return float((wt @ f * tmax) @ wp)
