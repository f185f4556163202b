"""The `point` emitter and the smooth `conductor` (include/msk_gpu.h at msk_point_desc and at MSK_BSDF_CONDUCTOR) restated twice,
sharing nothing with the code under test.

fp32 side (point_sample32, conductor_sample32): numpy float32, one IEEE operation per line, in the order the header gives; the
sigmoid polynomial of an rgb-valued spectrum comes from the oracle binding's srgb_model_eval, which returns the bits the device
function returns (a `uniform` spectrum, coefficients {0, 0, +inf}, is S = 1 and needs no oracle).

float64 side (point_sample64, conductor_sample64, and the closed forms of the render tests): textbook formulas on
radiometry_ref's Spectrum / expected_xyz / fresnel_conductor.
"""
import ctypes as C

import numpy as np

import envmap_ref as E
import radiometry_ref as R

F = np.float32


# ----------------------------------------------------------------------------- spectra, fp32
def sigmoid32(oracle, coeff, wl):
    """S(coeff, l) for wl float32 [n, 4] -> float32 [n, 4]"""
    wl = np.ascontiguousarray(wl, F).reshape(-1, 4)
    c = np.asarray(coeff, F)
    if oracle is None:
        assert np.isinf(c[2]) and c[0] == 0 and c[1] == 0, "an rgb-valued spectrum needs the oracle's srgb_model_eval"
        return np.full(wl.shape, 1.0 if c[2] > 0 else 0.0, F)
    c4 = np.ascontiguousarray(np.concatenate([c, [0]]), F)
    out = np.empty(wl.shape, F)
    fn = oracle.lib.msk_oracle_srgb_model_eval
    for k in range(len(wl)):
        fn(C.c_void_p(c4.ctypes.data), C.c_void_p(wl.ctypes.data + 16 * k), C.c_void_p(out.ctypes.data + 16 * k))
    return out


def spectrum32(oracle, sd, wl):
    """an msk_spectrum_desc that is not tabulated: S(coeff, l) * scale"""
    assert sd.regular == 0
    return (sigmoid32(oracle, sd.coeff[:], wl) * F(sd.scale)).astype(F)


def intensity32(oracle, coeff, table, wl):
    """the emitter's own value: its table (d65 * d65_scale, 95 entries on 360 .. 830) times S(coeff, l)"""
    return (E.regular_eval(table, np.asarray(wl, F).reshape(-1, 4)) * sigmoid32(oracle, coeff, wl)).astype(F)


# ----------------------------------------------------------------------------- the point emitter
def point_sample32(position, p, intensity):
    """position [3], p float32 [n, 3], intensity float32 [n, 4] = I(l) -> ({d.x, d.y, d.z, dist} [n, 4], value [n, 4]); zeros where dist == 0"""
    pos, p = np.asarray(position, F), np.asarray(p, F).reshape(-1, 3)
    dx, dy, dz = (pos[0] - p[:, 0]).astype(F), (pos[1] - p[:, 1]).astype(F), (pos[2] - p[:, 2]).astype(F)
    d2 = ((dx * dx).astype(F) + ((dy * dy).astype(F) + (dz * dz).astype(F)).astype(F)).astype(F)
    dist = np.sqrt(d2).astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F(1) / dist).astype(F)
        d = np.stack([(dx * inv).astype(F), (dy * inv).astype(F), (dz * inv).astype(F), dist], -1)
        value = ((np.asarray(intensity, F) * inv[:, None]).astype(F) * inv[:, None]).astype(F)
    zero = dist == 0
    d[zero] = 0
    value[zero] = 0
    return d, value


def point_sample64(position, p, intensity):
    v = np.asarray(position, np.float64) - np.asarray(p, np.float64).reshape(-1, 3)
    dist = np.linalg.norm(v, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.concatenate([v / dist[:, None], dist[:, None]], 1)
        value = np.asarray(intensity, np.float64) / (dist * dist)[:, None]
    d[dist == 0] = 0
    value[dist == 0] = 0
    return d, value


# ----------------------------------------------------------------------------- the smooth conductor
def fresnel_conductor32(c, eta, k):
    """render/fresnel.h:65-88 in fp32, one operation at a time (the order csrc/msk_device.h evaluates it in)"""
    c, eta, k = np.asarray(c, F), np.asarray(eta, F), np.asarray(k, F)
    c2 = (c * c).astype(F)
    s2 = (F(1) - c2).astype(F)
    s4 = (s2 * s2).astype(F)
    t1 = (((eta * eta).astype(F) - (k * k).astype(F)).astype(F) - s2).astype(F)
    four = ((((F(4) * k).astype(F) * k).astype(F) * eta).astype(F) * eta).astype(F)
    a2pb2 = np.sqrt(((t1 * t1).astype(F) + four).astype(F)).astype(F)
    a = np.sqrt((F(0.5) * (a2pb2 + t1).astype(F)).astype(F)).astype(F)
    term1 = (a2pb2 + c2).astype(F)
    term2 = ((F(2) * c).astype(F) * a).astype(F)
    rs = ((term1 - term2).astype(F) / (term1 + term2).astype(F)).astype(F)
    term3 = ((a2pb2 * c2).astype(F) + s4).astype(F)
    term4 = (term2 * s2).astype(F)
    rp = ((rs * (term3 - term4).astype(F)).astype(F) / (term3 + term4).astype(F)).astype(F)
    return (F(0.5) * (rs + rp).astype(F)).astype(F)


def conductor_sample32(cos_i, eta, k, spec):
    """cos_i float32 [n]; eta, k, spec float32 [n, 4] at the path's wavelengths -> the lobe's value [n, 4], zeros for cos_i <= 0"""
    c = np.asarray(cos_i, F).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (np.asarray(spec, F) * fresnel_conductor32(c[:, None], eta, k)).astype(F)
    v[~(c > 0)] = 0
    return v


def conductor_sample64(cos_i, eta, k, spec):
    c = np.asarray(cos_i, np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.asarray(spec, np.float64) * R.fresnel_conductor(c[:, None], np.asarray(eta, np.float64), np.asarray(k, np.float64))
    v[~(c > 0)] = 0
    return v


# ----------------------------------------------------------------------------- float64 closed forms of the render tests
def sigmoid_spectrum(coeff, scale=1.0):
    c0, c1, c2 = (float(c) for c in coeff)
    if np.isinf(c2):
        return R.constant(scale * (1.0 if c2 > 0 else 0.0))

    def fn(lam):
        x = (c0 * lam + c1) * lam + c2
        return scale * (0.5 + x / (2.0 * np.sqrt(1.0 + x * x)))
    return R.Spectrum(fn)


def emitter_spectrum(desc, e):
    """radiance / intensity of emitter e of a scene descriptor in the srgb_d65 form"""
    ed = desc.emitters[e]
    assert ed.radiance_regular == 0
    return R.srgb_d65(ed.radiance[:], np.array(desc.d65[:95], np.float64), ed.d65_scale)


def point_geometry(x, n, position):
    """cos(theta) / d^2 of a point light at `position` seen from the surface points x [..., 3] with normal n; 0 below the horizon"""
    v = np.asarray(position, np.float64) - np.asarray(x, np.float64)
    d2 = (v * v).sum(-1)
    return np.maximum(v @ np.asarray(n, np.float64), 0.0) / (d2 * np.sqrt(d2))


def reflect(d, n):
    n = np.asarray(n, np.float64)
    return d - 2.0 * (d @ n)[..., None] * n
