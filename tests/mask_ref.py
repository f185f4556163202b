"""The `mask` BSDF (include/msk_gpu.h at msk_mask_desc) restated twice: in numpy float32, one IEEE operation per line, for the
bit-for-bit comparison with the device's probes, and in float64 for the closed forms.  The nested BSDF X is a callable the caller
brings (the CPU oracle's restatements where it can follow, delta_ref's conductor, a hand-made diffuse); the opacity image uses the
bitmap texture's restated lookup (bitmap_ref) with the scalar where S(texel, l) stands.  Nothing here is shared with the code
under test.

A mask is a dict {"filter": 0 | 1 | 2, "opacity": a, "values": float32 [H, W], "to_uv": 6 floats} (msk_mask_desc's fields)."""
import numpy as np

import bitmap_ref as BR

F = np.float32
IDENTITY_UV = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def opacity32(mask, uv):
    """a at uv float32[n, 2] -> float32[n]"""
    uv = np.asarray(uv, F).reshape(-1, 2)
    if mask["filter"] == 0:
        return np.full(len(uv), F(mask["opacity"]), F)
    v = np.asarray(mask["values"], F)
    wl = np.zeros((len(uv), 4), F)
    out = BR.lookup(BR.grey_texels(v), v.shape[1], v.shape[0], "nearest" if mask["filter"] == 1 else "bilinear", mask.get("to_uv", IDENTITY_UV), uv, wl)
    return np.ascontiguousarray(out[:, 0], F)


def opacity64(mask, uv):
    """the same lookup in float64 (texel coordinates from the float64 transform: beside a texel border the two may pick different
    texels; the self-check stays away from the borders by 1e-3 of a texel)"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    if mask["filter"] == 0:
        return np.full(len(uv), float(mask["opacity"]))
    v = np.asarray(mask["values"], np.float64)
    h, w = v.shape
    m = np.asarray(mask.get("to_uv", IDENTITY_UV), np.float64)
    x = m[0] * uv[:, 0] + m[1] * uv[:, 1] + m[2]
    y = m[3] * uv[:, 0] + m[4] * uv[:, 1] + m[5]
    fu, fv = x - np.floor(x), y - np.floor(y)
    if mask["filter"] == 1:
        return v[np.minimum((fv * h).astype(np.int64), h - 1), np.minimum((fu * w).astype(np.int64), w - 1)]
    px, py = fu * w - 0.5, fv * h - 0.5
    i0, j0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    tx, ty = px - i0, py - j0
    i0, j0 = i0 % w, j0 % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    a = v[j0, i0] + tx * (v[j0, i1] - v[j0, i0])
    b = v[j1, i0] + tx * (v[j1, i1] - v[j1, i0])
    return a + ty * (b - a)


def pick32(a, ux):
    """mask.cpp:43-44 by u.x: (nested?, the u.x the nested BSDF gets: u.x / a, one IEEE division)"""
    a, ux = np.asarray(a, F), np.asarray(ux, F)
    nested = ux < a
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = (ux / a).astype(F)
    return nested, np.where(nested, scaled, ux).astype(F)


def sample32(a, wi, sample1, u, x_sample, x_delta):
    """sample() at n points: a float32[n], wi float32[n, 3] (local), sample1 float32[n], u float32[n, 2].
    x_sample(index array, wi, sample1, u) -> (wo [k, 3], pdf [k], value [k, 4], eta [k], ok [k]) of X at those points;
    x_delta = X has no smooth lobe.  -> dict(wo, pdf, value, eta, delta, null, ok), float32 / bool arrays"""
    n = len(a)
    wi, u = np.asarray(wi, F).reshape(n, 3), np.asarray(u, F).reshape(n, 2)
    nested, ux = pick32(a, u[:, 0])
    out = dict(wo=np.zeros((n, 3), F), pdf=np.zeros(n, F), value=np.zeros((n, 4), F), eta=np.ones(n, F), delta=np.zeros(n, bool), null=~nested, ok=np.zeros(n, bool))
    k = np.flatnonzero(nested)
    if len(k):
        wo, pdf, value, eta, ok = x_sample(k, wi[k], np.asarray(sample1, F)[k], np.stack([ux[k], u[k, 1]], -1).astype(F))
        out["wo"][k], out["value"][k], out["eta"][k], out["ok"][k] = wo, value, eta, ok
        out["pdf"][k] = (a[k] * np.asarray(pdf, F)).astype(F)                 # pdf = a * pdf_X, the value stays X's
        out["delta"][k] = x_delta
    z = np.flatnonzero(~nested)
    out["wo"][z] = -wi[z]                                                     # the ray's own direction (local form)
    out["pdf"][z] = (F(1) - a[z]).astype(F)
    out["value"][z] = F(1)
    out["delta"][z], out["ok"][z] = True, True
    return out


def eval32(a, value_x, pdf_x):
    """eval = a * eval_X, pdf = a * pdf_X"""
    a = np.asarray(a, F)
    return (np.asarray(value_x, F) * a[:, None]).astype(F), (a * np.asarray(pdf_x, F)).astype(F)


# ----------------------------------------------------------------------------- float64
def sample64(a, u, x_sample64):
    """one point in float64: u = (u.x, u.y); x_sample64(u) -> (wo, pdf, value).  -> (wo or None for the null lobe, pdf, value)"""
    if u[0] < a:
        wo, pdf, value = x_sample64((u[0] / a, u[1]))
        return wo, a * pdf, value
    return None, 1.0 - a, 1.0


def sample_as_written64(a, u, x_sample64):
    """mask.cpp:47,53,68 as written: the nested value times the opacity AND the nested pdf unscaled; the null lobe (1 - a) / (1 - a)"""
    if u[0] < a:
        wo, pdf, value = x_sample64((u[0] / a, u[1]))
        return wo, pdf, value * a
    return None, 1.0 - a, 1.0


def diffuse_sample64(rho):
    """a float64 Lambertian X for the self-checks: cosine-weighted wo by the concentric-free polar map, value rho, pdf cos / pi"""
    def fn(u):
        r, phi = np.sqrt(u[0]), 2.0 * np.pi * u[1]
        wo = np.array([r * np.cos(phi), r * np.sin(phi), np.sqrt(max(0.0, 1.0 - u[0]))])
        return wo, wo[2] / np.pi, rho
    return fn


def diffuse_eval64(rho, wo):
    return rho / np.pi * max(wo[2], 0.0), max(wo[2], 0.0) / np.pi
