"""The `bitmap` texture's lookup (include/msk_gpu.h at msk_texture_desc) restated in numpy float32, one IEEE operation per line.

A texel's spectral value comes from a callable `texel(j, i, wl) -> float32[n, 4]` (row indices, column indices, the points'
wavelengths): `oracle_texels` makes one from the oracle's srgb_model_eval and a coefficient image, the sanity tests pass
hand-made ones.  Everything else is float32 arithmetic written out here and nowhere shared with the code under test."""
import ctypes as C

import numpy as np

F = np.float32


def frac_uv(to_uv, uv):
    """uv' = M (u, v, 1) as Eigen sums a row, a0 + (a1 + a2); then x - floor(x): in [0, 1], 1 itself for a tiny negative x."""
    m = np.asarray(to_uv, F)
    uv = np.asarray(uv, F).reshape(-1, 2)
    u, v = uv[:, 0], uv[:, 1]
    ax = m[1] * v
    ax = ax + m[2] * F(1)
    x = m[0] * u
    x = x + ax
    ay = m[4] * v
    ay = ay + m[5] * F(1)
    y = m[3] * u
    y = y + ay
    return (x - np.floor(x)).astype(F), (y - np.floor(y)).astype(F)


def _nearest_axis(f, n):
    i = (f * F(n)).astype(F).astype(np.int64)          # (int) (f * n): f >= 0, truncation
    return np.minimum(i, n - 1)


def _bilinear_axis(f, n):
    p = (f * F(n)).astype(F)
    p = (p - F(0.5)).astype(F)
    i0 = np.floor(p).astype(np.int64)
    t = (p - i0.astype(F)).astype(F)                   # before the wrap: i0 may be -1 here
    i0 = np.where(i0 < 0, n - 1, i0)
    i0 = np.where(i0 >= n, 0, i0)
    i1 = i0 + 1
    i1 = np.where(i1 >= n, 0, i1)
    return i0, i1, t


def lookup(texel, width, height, filt, to_uv, uv, wl):
    """-> float32[n, 4]: the texture's value at uv float32[n, 2] and wavelengths float32[n, 4]."""
    wl = np.asarray(wl, F).reshape(-1, 4)
    fu, fv = frac_uv(to_uv, uv)
    if filt == "nearest":
        return np.asarray(texel(_nearest_axis(fv, height), _nearest_axis(fu, width), wl), F)
    assert filt == "bilinear", filt
    i0, i1, tx = _bilinear_axis(fu, width)
    j0, j1, ty = _bilinear_axis(fv, height)
    s00, s10 = np.asarray(texel(j0, i0, wl), F), np.asarray(texel(j0, i1, wl), F)
    s01, s11 = np.asarray(texel(j1, i0, wl), F), np.asarray(texel(j1, i1, wl), F)
    tx, ty = tx[:, None], ty[:, None]
    with np.errstate(invalid="ignore"):
        a = (s10 - s00).astype(F)
        a = (tx * a).astype(F)
        a = (s00 + a).astype(F)
        b = (s11 - s01).astype(F)
        b = (tx * b).astype(F)
        b = (s01 + b).astype(F)
        r = (b - a).astype(F)
        r = (ty * r).astype(F)
        return (a + r).astype(F)


def oracle_texels(oracle, coeffs):
    """coeffs float32[H, W, 3] (sigmoid-polynomial coefficients per texel) -> texel(j, i, wl) through oracle.srgb_model_eval,
    the spectrum_eval srgb form at scale 1."""
    coeffs = np.ascontiguousarray(coeffs, F)
    fn = oracle.lib.msk_oracle_srgb_model_eval

    def texel(j, i, wl):
        c = np.ascontiguousarray(coeffs[j, i], F)
        w = np.ascontiguousarray(wl, F)
        out = np.empty((len(c), 4), F)
        cp, wp, op = c.ctypes.data, w.ctypes.data, out.ctypes.data
        for k in range(len(c)):
            fn(C.c_void_p(cp + 12 * k), C.c_void_p(wp + 16 * k), C.c_void_p(op + 16 * k))
        return (out * F(1)).astype(F)
    return texel


def grey_texels(levels):
    """levels float32[H, W] -> texel(j, i, wl): the level at every wavelength (hand-checkable)."""
    levels = np.asarray(levels, F)

    def texel(j, i, wl):
        return np.repeat(levels[j, i][:, None], 4, 1).astype(F)
    return texel
