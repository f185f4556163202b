"""The "direct" integrator restated for the tests (include/msk_gpu.h at msk_direct_params).

Two things, both independent of the library's code:

1. The random-pair layout of one camera sample (pair_layout, draws): pairs 0-2 are the `path` integrator's (film position,
   wavelengths, aperture), pair 3 + i is light sample i, pairs 3 + N + 2 j and 3 + N + 2 j + 1 are BSDF sample j's lobe choice (.x)
   and direction.

2. A float64 estimator of the same integrand on scenes of diffuse triangles lit by ONE area emitter (estimate): brute-force ray /
   triangle intersection, uniform sampling of the emitter's area, cosine-weighted BSDF sampling, the power heuristic over the sample
   COUNTS.  It works in scalar units — every reflectance 1, emitted radiance 1, no wavelengths — so a sample of the renderer is
   A(wavelengths) * G with G what this estimator draws (for a diffuse scene the geometric part does not depend on the wavelength)
   and A the spectral factor of the sample's four wavelengths, the same draw (pair 1) whatever N and M are.  Hence
       Var[sample] = E[A^2] Var[G] + Var[A] E[G]^2,
   monotone in Var[G]: where Var[G] at (8, 8) is well below Var[G] at (1, 1), so is the renderer's per-sample variance.
"""
import numpy as np


# ----------------------------------------------------------------------------- the pair layout
def pair_layout(n_light, n_bsdf):
    """-> {"film": 0, "wavelengths": 1, "aperture": 2, "light": [pairs], "bsdf_lobe": [pairs], "bsdf_direction": [pairs]}"""
    n, m = int(n_light), int(n_bsdf)
    return {"film": 0, "wavelengths": 1, "aperture": 2,
            "light": [3 + i for i in range(n)],
            "bsdf_lobe": [3 + n + 2 * j for j in range(m)],
            "bsdf_direction": [3 + n + 2 * j + 1 for j in range(m)]}


def draws(n_light, n_bsdf):
    """every pair a sample draws from, as a flat list (one entry per draw that owns its pair)"""
    lay = pair_layout(n_light, n_bsdf)
    return [lay["film"], lay["wavelengths"], lay["aperture"]] + lay["light"] + lay["bsdf_lobe"] + lay["bsdf_direction"]


def weight(na, pa, nb, pb):
    """(na pa)^2 / ((na pa)^2 + (nb pb)^2); 0 where pa is 0"""
    a, b = (na * np.asarray(pa, np.float64)) ** 2, (nb * np.asarray(pb, np.float64)) ** 2
    return np.where(a > 0, a / np.where(a + b > 0, a + b, 1.0), 0.0)


def weight_f32(na, pa, nb, pb):
    """the same weight in fp32, one rounded operation at a time, in the order include/msk_gpu.h pins:
    a = na * pa; b = nb * pb; a = a * a; b = b * b; a > 0 ? a / (a + b) : 0"""
    f = np.float32
    with np.errstate(all="ignore"):
        a, b = f(f(na) * f(pa)), f(f(nb) * f(pb))
        a, b = f(a * a), f(b * b)
        return f(a / f(a + b)) if a > 0 else f(0)


def recombine_f32(terms, n_light, n_bsdf):
    """the spectral result of one camera sample from the factors msk_oracle_direct_terms reports, in numpy fp32, one operation at
    a time in the header's order: emission, then the light samples, then the BSDF samples; a light term is (prod * w_l) / N where its
    shadow ray was traced and found nothing, a BSDF term (prod * w_b) / M where the ray reached an emitter or an environment.
    -> (float32[4], the shadow flags this restatement derives for the light samples)"""
    f = np.float32
    fn, fm = f(n_light), f(n_bsdf)
    shadows = []
    with np.errstate(all="ignore"):
        res = (np.zeros(4, f) + terms["emission"]).astype(f)
        for lt in terms["light"]:
            if lt["p_l"] == 0:
                shadows.append(False)
                continue
            w = f(1) if lt["point"] else weight_f32(fn, lt["p_l"], fm, lt["p_b"])
            t = (lt["prod"].astype(f) * w).astype(f)
            shadow = bool((t != 0).any())
            shadows.append(shadow)
            if shadow and not lt["occluded"]:
                res = (res + (t / fn).astype(f)).astype(f)
        for bt in terms["bsdf"]:
            if bt["reached"]:
                w = weight_f32(fm, bt["p_b"], fn, bt["p_e"])
                t = (bt["prod"].astype(f) * w).astype(f)
                res = (res + (t / fm).astype(f)).astype(f)
    return res, shadows


# ----------------------------------------------------------------------------- geometry, brute force
class Triangles:
    """the flattened scene's triangles in float64: v0, e1, e2, unit normal (e1 x e2), the mesh of each, and which mesh emits"""

    def __init__(self, flat):
        d = flat.desc
        v = np.asarray(flat.vertices, np.float64)[:, :3]
        v0, e1, e2, mesh = [], [], [], []
        self.emitter_mesh = -1
        for k in range(d.n_meshes):
            m = d.meshes[k]
            f = np.asarray(flat.faces, np.int64)[m.first_face:m.first_face + m.face_count] + m.first_vertex
            v0.append(v[f[:, 0]]); e1.append(v[f[:, 1]] - v[f[:, 0]]); e2.append(v[f[:, 2]] - v[f[:, 0]])
            mesh += [k] * m.face_count
            if m.emitter_id >= 0:
                assert self.emitter_mesh < 0, "one area emitter"
                self.emitter_mesh = k
        self.v0, self.e1, self.e2 = np.concatenate(v0), np.concatenate(e1), np.concatenate(e2)
        self.mesh = np.array(mesh)
        c = np.cross(self.e1, self.e2)
        self.area = 0.5 * np.linalg.norm(c, axis=1)
        self.n = c / (2.0 * self.area)[:, None]
        self.lamp = np.nonzero(self.mesh == self.emitter_mesh)[0]
        self.lamp_area = float(self.area[self.lamp].sum())

    def intersect(self, o, d, tmin, tmax):
        """Moeller-Trumbore, every ray against every triangle -> (t, triangle index), t = inf and index -1 on a miss"""
        o, d = np.broadcast_arrays(np.asarray(o, np.float64), np.asarray(d, np.float64))
        p = np.cross(d[:, None, :], self.e2[None])
        det = (self.e1[None] * p).sum(-1)
        ok = np.abs(det) > 1e-14
        inv = 1.0 / np.where(ok, det, 1.0)
        s = o[:, None, :] - self.v0[None]
        u = (s * p).sum(-1) * inv
        q = np.cross(s, self.e1[None])
        v = (d[:, None, :] * q).sum(-1) * inv
        t = (self.e2[None] * q).sum(-1) * inv
        tmin, tmax = np.broadcast_to(tmin, t.shape[:1]), np.broadcast_to(tmax, t.shape[:1])
        hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin[:, None]) & (t < tmax[:, None])
        t = np.where(hit, t, np.inf)
        k = t.argmin(1)
        best = t[np.arange(len(k)), k]
        return best, np.where(np.isfinite(best), k, -1)


def _frame(n):
    a = np.where(np.abs(n[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    s = np.cross(n, a)
    s /= np.linalg.norm(s, axis=1)[:, None]
    return s, np.cross(n, s)


def estimate(flat, tris, pixel, n_light, n_bsdf, n, rng, camera_ray):
    """n draws of G for film pixel (x, y): emission of the primary hit + the N light samples + the M BSDF samples, scalar units.
    camera_ray: radiometry_ref.camera_ray.  Samples whose camera ray misses the scene are 0."""
    N, M = int(n_light), int(n_bsdf)
    x, y = pixel
    o, d = camera_ray(flat.desc, x + rng.random_sample(n), y + rng.random_sample(n))
    o = np.broadcast_to(o, d.shape)
    t, k = tris.intersect(o, d, 0.0, np.inf)
    out = np.zeros(n)
    hit = k >= 0
    idx = np.nonzero(hit)[0]
    if len(idx) == 0:
        return out
    p = o[idx] + d[idx] * t[idx, None]
    ns = tris.n[k[idx]]
    front = (ns * -d[idx]).sum(-1) > 0
    out[idx] += np.where((tris.mesh[k[idx]] == tris.emitter_mesh) & front, 1.0, 0.0)
    eps = 1e-6 * (1.0 + np.abs(p).max(1))
    cdf = np.cumsum(tris.area[tris.lamp]) / tris.lamp_area
    res = np.zeros(len(idx))
    for _ in range(N):
        j = tris.lamp[np.minimum(np.searchsorted(cdf, rng.random_sample(len(idx)), side="right"), len(tris.lamp) - 1)]
        u1, u2 = rng.random_sample(len(idx)), rng.random_sample(len(idx))
        r = np.sqrt(u1)
        lp = tris.v0[j] + tris.e1[j] * (r * (1.0 - u2))[:, None] + tris.e2[j] * (r * u2)[:, None]
        w = lp - p
        dist = np.linalg.norm(w, axis=1)
        w /= dist[:, None]
        cos_l, cos_s = -(w * tris.n[j]).sum(-1), (w * ns).sum(-1)
        ok = (cos_l > 0) & (cos_s > 0) & front
        p_l = np.where(ok, dist * dist / (tris.lamp_area * np.where(ok, cos_l, 1.0)), 0.0)
        p_b = np.where(cos_s > 0, cos_s / np.pi, 0.0)
        tt, _ = tris.intersect(p, w, eps, dist * (1.0 - 1e-4))
        vis = ok & ~np.isfinite(tt)
        res += np.where(vis, (cos_s / np.pi) / np.where(ok, p_l, 1.0) * weight(N, p_l, M, p_b), 0.0) / N
    for _ in range(M):
        u1, u2 = rng.random_sample(len(idx)), rng.random_sample(len(idx))
        r, phi = np.sqrt(u1), 2.0 * np.pi * u2
        s, tt_ = _frame(ns)
        cz = np.sqrt(np.maximum(0.0, 1.0 - u1))
        w = s * (r * np.cos(phi))[:, None] + tt_ * (r * np.sin(phi))[:, None] + ns * cz[:, None]
        p_b = cz / np.pi
        t2, k2 = tris.intersect(p, w, eps, np.inf)
        on = (k2 >= 0) & (tris.mesh[np.maximum(k2, 0)] == tris.emitter_mesh) & front & (cz > 0)
        cos_l = -(w * tris.n[np.maximum(k2, 0)]).sum(-1)
        on &= cos_l > 0
        p_e = np.where(on, t2 * t2 / (tris.lamp_area * np.where(on, cos_l, 1.0)), 0.0)
        res += np.where(on, weight(M, p_b, N, p_e), 0.0) / M
    out[idx] += res
    return out
