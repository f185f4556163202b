"""The `envmap` emitter (include/msk_gpu.h at msk_envmap_desc) restated twice, sharing nothing with the code under test.

fp32 side (class Env32): numpy float32, one IEEE operation per line; sin / cos / atan and the sigmoid polynomial come from the
oracle binding's det_math / det_math2 / srgb_model_eval, which return the bits the device functions return.  The cumulative
tables are built here in float64 and rounded to float32, as csrc/msk_envmap.h does.

float64 side (class Env64): radiance, the piecewise-constant density and the quadrature of integral L f cos over the sphere, on
radiometry_ref's Spectrum / expected_xyz.

The rounding case of pdf(direction(sample(u))): the direction is rebuilt into uv through det_sincos, a rotation and det_atan, each
rounded to fp32, so uv comes back within a few 2^-24 of what the sampler made.  When that uv lies within this distance of a cell
border — or when ((i + du) / W) * W itself rounds across i — the lookup lands in the neighbouring cell, whose mass differs.
Env32.sample reports the sampler's cell and Env32.eval_dir the looked-up one; a probe point is excluded exactly when they differ —
the exclusion is defined by that outcome, not by a predicate on the random numbers, and the cap of 0.1 % of the probe points is what
bounds it.  Outside it the two densities are equal bit for bit under the identity; under a rotation R^T (R d) is d only within
three roundings per component (2^-22 absolute on sin theta, which the density divides by), so they agree within
2^-21 / sin theta + 2^-21 relative (include/msk_gpu.h says the same).
"""
import ctypes as C

import numpy as np

import radiometry_ref as R

F = np.float32
PI = F(3.14159274101257324)
TWO_PI = F(F(2) * PI)
TWO_PI2 = F(F(2) * F(PI * PI))
EPS2 = F(2.0 ** -48)
ONE_BELOW = F(1) - F(2.0 ** -24)


# ----------------------------------------------------------------------------- fp32
def _each(fn, x, n_out, pick):
    x = np.ascontiguousarray(x, F).reshape(-1)
    out = np.empty((len(x), n_out), F)
    for k in range(len(x)):
        fn(C.c_float(float(x[k])), C.c_void_p(out.ctypes.data + 4 * n_out * k))
    return [out[:, p].copy() for p in pick]


def det_sincos(oracle, x):
    return _each(oracle.lib.msk_oracle_det_math, x, 4, (0, 1))


def det_atan(oracle, x):
    return _each(oracle.lib.msk_oracle_det_math2, x, 2, (0,))[0]


def atan2(oracle, y, x):
    y, x = np.asarray(y, F), np.asarray(x, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (y / x).astype(F)
    r = det_atan(oracle, np.where(x == 0, F(0), q))
    r = np.where(x < 0, np.where(y >= 0, (r + PI).astype(F), (r - PI).astype(F)), r).astype(F)
    half = F(PI * F(0.5))
    return np.where(x == 0, np.where(y > 0, half, np.where(y < 0, -half, F(0))), r).astype(F)


def regular_eval(table, wl):
    """regular_eval on the 95-entry 360 .. 830 grid (spectra/regular.cpp:73-91)"""
    t, wl = np.asarray(table, F), np.asarray(wl, F)
    x = ((wl - F(360)).astype(F) * F(0.2)).astype(F)
    idx = np.minimum(np.maximum(x, 0).astype(np.int64), 93)
    w1 = (x - idx.astype(F)).astype(F)
    w0 = (F(1) - w1).astype(F)
    return ((w0 * t[idx]).astype(F) + (w1 * t[idx + 1]).astype(F)).astype(F)


def cumulative(w):
    """csrc/msk_envmap.h: sums in double, entry k = float(sum of the first k / total), the last entry 1"""
    w = np.asarray(w, np.float64)
    run = np.cumsum(w)
    out = np.zeros(len(w) + 1, F)
    if run[-1] > 0:
        out[1:] = (run / run[-1]).astype(F)
    out[-1] = F(1)
    return out


def search(cdf, n, u):
    """Distribution1D::sample_reuse (core/distribution.h:106-116): upper bound, clamp, reused fraction (kept below 1)"""
    u = np.asarray(u, F)
    k = np.clip(np.searchsorted(cdf[:n + 1], u, side="right") - 1, 0, n - 1)       # first entry with u < cdf[m], minus one
    c0, c1 = cdf[k], cdf[k + 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = ((u - c0).astype(F) / (c1 - c0).astype(F)).astype(F)
    return k, np.where(ONE_BELOW < frac, ONE_BELOW, frac).astype(F)


class Env32:
    def __init__(self, oracle, texels, weights, to_world, emitter_table):
        """texels float32 [H, W, 4] {c0, c1, c2, w}; weights float32 [H, W]; to_world 3x3; emitter_table float32 [95] = d65 * d65_scale"""
        self.o = oracle
        self.tex = np.ascontiguousarray(texels, F)
        self.H, self.W = self.tex.shape[:2]
        self.R = np.asarray(to_world, F).reshape(3, 3)
        self.table = np.asarray(emitter_table, F)
        wt = np.asarray(weights, F).reshape(self.H, self.W)
        self.cond = np.stack([cumulative(wt[j]) for j in range(self.H)])
        self.marg = cumulative([np.cumsum(wt[j].astype(np.float64))[-1] for j in range(self.H)])      # (row sums added left to right)

    # ---- direction <-> uv
    def to_local(self, d):
        d, r = np.asarray(d, F).reshape(-1, 3), self.R
        col = lambda c: (r[0, c] * d[:, 0] + ((r[1, c] * d[:, 1]).astype(F) + (r[2, c] * d[:, 2]).astype(F)).astype(F)).astype(F)
        return col(0), col(1), col(2)

    def dir_to_uv(self, d):
        lx, ly, lz = self.to_local(d)
        s2 = ((lx * lx).astype(F) + (lz * lz).astype(F)).astype(F)
        u = (atan2(self.o, lx, -lz) / TWO_PI).astype(F)
        u = (u - np.floor(u)).astype(F)
        u = np.where(u < 1, u, F(0)).astype(F)
        v = (atan2(self.o, np.sqrt(s2).astype(F), ly) / PI).astype(F)
        return u, v, np.sqrt(np.where(s2 < EPS2, EPS2, s2)).astype(F)

    # ---- radiance
    def _texel(self, j, i, wl):
        t = np.ascontiguousarray(self.tex[j, i], F)
        w = np.ascontiguousarray(wl, F)
        out = np.empty((len(t), 4), F)
        fn = self.o.lib.msk_oracle_srgb_model_eval
        for k in range(len(t)):
            fn(C.c_void_p(t.ctypes.data + 16 * k), C.c_void_p(w.ctypes.data + 16 * k), C.c_void_p(out.ctypes.data + 16 * k))
        return (out * t[:, 3:4]).astype(F)

    def radiance_uv(self, u, v, wl):
        wl = np.asarray(wl, F).reshape(-1, 4)
        W, H = self.W, self.H
        px = ((u * F(W)).astype(F) - F(0.5)).astype(F)
        i = np.floor(px).astype(np.int64)
        tx = (px - i.astype(F)).astype(F)
        i0 = np.where(i < 0, W - 1, i)
        i0 = np.where(i0 >= W, 0, i0)
        i1 = np.where(i0 + 1 >= W, 0, i0 + 1)
        py = ((v * F(H)).astype(F) - F(0.5)).astype(F)
        j = np.floor(py).astype(np.int64)
        ty = (py - j.astype(F)).astype(F)
        j0, j1 = np.clip(j, 0, H - 1), np.clip(j + 1, 0, H - 1)
        s00, s10, s01, s11 = self._texel(j0, i0, wl), self._texel(j0, i1, wl), self._texel(j1, i0, wl), self._texel(j1, i1, wl)
        tx, ty = tx[:, None], ty[:, None]
        a = (s00 + ((s10 - s00).astype(F) * tx).astype(F)).astype(F)
        b = (s01 + ((s11 - s01).astype(F) * tx).astype(F)).astype(F)
        r = (a + ((b - a).astype(F) * ty).astype(F)).astype(F)
        return (regular_eval(self.table, wl) * r).astype(F)

    # ---- density
    def pdf_cell(self, i, j, sin_theta):
        pr = (self.marg[j + 1] - self.marg[j]).astype(F)
        pc = (self.cond[j, i + 1] - self.cond[j, i]).astype(F)
        p = (((pr * pc).astype(F) * F(self.W)).astype(F) * F(self.H)).astype(F)
        return (p / (TWO_PI2 * sin_theta).astype(F)).astype(F)

    def cell_of(self, u, v):
        i = np.minimum((u * F(self.W)).astype(F).astype(np.int64), self.W - 1)
        j = np.minimum((v * F(self.H)).astype(F).astype(np.int64), self.H - 1)
        return i, j

    def eval_dir(self, d, wl):
        """-> (radiance [n, 4], pdf_omega [n], (i, j) of the looked-up cell)"""
        u, v, st = self.dir_to_uv(d)
        i, j = self.cell_of(u, v)
        return self.radiance_uv(u, v, wl), self.pdf_cell(i, j, st), (i, j)

    def sample(self, u2):
        """u2 float32 [n, 2] -> (direction [n, 3], uv [n, 2], pdf_omega [n], (i, j) of the sampled cell)"""
        u2 = np.asarray(u2, F).reshape(-1, 2)
        j, dv = search(self.marg, self.H, u2[:, 1])
        i, du = np.zeros(len(j), np.int64), np.zeros(len(j), F)
        for row in np.unique(j):
            m = j == row
            i[m], du[m] = search(self.cond[row], self.W, u2[m, 0])
        u = ((i.astype(F) + du).astype(F) / F(self.W)).astype(F)
        v = ((j.astype(F) + dv).astype(F) / F(self.H)).astype(F)
        st, ct = det_sincos(self.o, (PI * v).astype(F))
        sp, cp = det_sincos(self.o, (TWO_PI * u).astype(F))
        lx, ly, lz = (sp * st).astype(F), ct, (-(cp * st)).astype(F)
        s2 = ((lx * lx).astype(F) + (lz * lz).astype(F)).astype(F)
        sin_theta = np.sqrt(np.where(s2 < EPS2, EPS2, s2)).astype(F)
        r = self.R
        row3 = lambda k: (r[k, 0] * lx + ((r[k, 1] * ly).astype(F) + (r[k, 2] * lz).astype(F)).astype(F)).astype(F)
        return np.stack([row3(0), row3(1), row3(2)], 1), np.stack([u, v], 1), self.pdf_cell(i, j, sin_theta), (i, j)


# ----------------------------------------------------------------------------- float64
class Env64:
    """texels [H, W, 4] {c0, c1, c2, w}, weights [H, W], to_world 3x3, the scene's d65 table and the emitter's d65_scale"""

    def __init__(self, texels, weights, to_world, d65_table, d65_scale):
        self.tex = np.asarray(texels, np.float64)
        self.H, self.W = self.tex.shape[:2]
        self.R = np.asarray(to_world, np.float64).reshape(3, 3)
        wt = np.asarray(weights, np.float64).reshape(self.H, self.W)
        self.pmf = wt / wt.sum()
        self.T = R.regular(R.CIE_MIN, R.CIE_MAX, np.asarray(d65_table, np.float64) * float(d65_scale))

    def dir_to_uv(self, d):
        dl = np.asarray(d, np.float64) @ self.R                       # R^T d
        u = np.arctan2(dl[..., 0], -dl[..., 2]) / (2 * np.pi)
        return u - np.floor(u), np.arctan2(np.hypot(dl[..., 0], dl[..., 2]), dl[..., 1]) / np.pi

    def uv_to_dir(self, u, v):
        th, ph = np.pi * v, 2 * np.pi * u
        dl = np.stack([np.sin(ph) * np.sin(th), np.cos(th), -np.cos(ph) * np.sin(th)], -1)
        return dl @ self.R.T

    def corners(self, u, v):
        """the four texels around (u, v) and their bilinear weights: [(flat index, weight)] * 4"""
        px, py = u * self.W - 0.5, v * self.H - 0.5
        i, j = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
        tx, ty = px - i, py - j
        i0, i1 = i % self.W, (i + 1) % self.W
        j0, j1 = np.clip(j, 0, self.H - 1), np.clip(j + 1, 0, self.H - 1)
        return [(j0 * self.W + i0, (1 - tx) * (1 - ty)), (j0 * self.W + i1, tx * (1 - ty)), (j1 * self.W + i0, (1 - tx) * ty), (j1 * self.W + i1, tx * ty)]

    def texel_spectrum(self, k, lam):
        c0, c1, c2, w = self.tex.reshape(-1, 4)[k]
        x = (c0 * lam + c1) * lam + c2
        return w * (0.5 + x / (2.0 * np.sqrt(1.0 + x * x)))

    def radiance(self, d, lam):
        """L(d, lam) for one direction (or an array of them) at one array of wavelengths broadcast against it"""
        u, v = self.dir_to_uv(d)
        return self.T(lam) * sum(wt * self.texel_spectrum_at(k, lam) for k, wt in self.corners(u, v))

    def texel_spectrum_at(self, k, lam):
        t = self.tex.reshape(-1, 4)[k]
        x = (t[..., 0] * lam + t[..., 1]) * lam + t[..., 2]
        return t[..., 3] * (0.5 + x / (2.0 * np.sqrt(1.0 + x * x)))

    def pdf(self, d):
        u, v = self.dir_to_uv(d)
        i, j = np.minimum((u * self.W).astype(np.int64), self.W - 1), np.minimum((v * self.H).astype(np.int64), self.H - 1)
        dl = np.asarray(d, np.float64) @ self.R
        return self.pmf[j, i] * self.W * self.H / (2 * np.pi ** 2 * np.hypot(dl[..., 0], dl[..., 2]))

    def sphere_nodes(self, nu, nv):
        """midpoint rule in (u, v): directions [nv, nu, 3], solid-angle weights [nv, nu], u and v"""
        u, v = (np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv
        uu, vv = np.meshgrid(u, v)
        return self.uv_to_dir(uu, vv), 2 * np.pi ** 2 * np.sin(np.pi * vv) / (nu * nv), uu, vv

    def texel_moments(self, g, nu, nv):
        """c_k = integral of B_k(omega) g(omega) d omega for every texel k (B_k: its bilinear basis function), g(directions) -> values;
        then integral L(omega, lam) g(omega) d omega = T(lam) sum_k c_k w_k S_k(lam)"""
        d, dw, uu, vv = self.sphere_nodes(nu, nv)
        gw = (g(d) * dw).reshape(-1)
        c = np.zeros(self.W * self.H)
        for k, wt in self.corners(uu, vv):
            c += np.bincount(k.reshape(-1), weights=(wt.reshape(-1) * gw), minlength=len(c))
        return c

    def lit_spectrum(self, c, extra=None):
        """the Spectrum lam -> T(lam) sum_k c_k w_k S_k(lam) (times `extra`, a Spectrum, e.g. a reflectance / pi)"""
        ks = np.nonzero(c)[0]

        def fn(lam):
            lam = np.asarray(lam, np.float64)
            return sum(c[k] * self.texel_spectrum(k, lam) for k in ks) + 0.0 * lam
        s = R.Spectrum(fn) * self.T
        return s * extra if extra is not None else s
