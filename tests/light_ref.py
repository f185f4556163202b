"""The `spot` and `directional` emitters (include/msk_gpu.h at msk_light_desc) restated twice, sharing nothing with the code under
test.  The reference has neither plugin: the header is the specification.

fp32 side (falloff32, spot_sample32, sun_sample32, env_radius32): numpy float32, one IEEE operation per line, in the order the header
gives; d, dist and inv are delta_ref.point_sample32's.

float64 side (falloff64, spot_geometry, sun_geometry): textbook formulas for the closed forms of the render tests.
"""
import numpy as np

import delta_ref as D

F = np.float32
RAY_EPS = F(F(5.9604644775390625e-08) * F(1500))       # core/mathutils.h:10-20, msk_layout.h: MSK_RAY_EPS_F


# ----------------------------------------------------------------------------- fp32
def falloff32(c, cos_cutoff, cos_beam):
    """the cone factor: 1 for c >= cos_beam, else 0 for c <= cos_cutoff, else (t t) (3 - 2 t) with t = (c - cos_cutoff) / (cos_beam - cos_cutoff)"""
    c, cc, cb = np.asarray(c, F), F(cos_cutoff), F(cos_beam)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((c - cc).astype(F) / F(cb - cc)).astype(F)
        s = ((t * t).astype(F) * (F(3) - (F(2) * t).astype(F)).astype(F)).astype(F)
    return np.where(c >= cb, F(1), np.where(c <= cc, F(0), s)).astype(F)


def spot_cosine32(position, axis, p):
    """c = -(d.x a.x + (d.y a.y + d.z a.z)) with d of point_sample32; NaN where dist == 0"""
    pos, a, p = np.asarray(position, F), np.asarray(axis, F), np.asarray(p, F).reshape(-1, 3)
    dx, dy, dz = (pos[0] - p[:, 0]).astype(F), (pos[1] - p[:, 1]).astype(F), (pos[2] - p[:, 2]).astype(F)
    dist = np.sqrt(((dx * dx).astype(F) + ((dy * dy).astype(F) + (dz * dz).astype(F)).astype(F)).astype(F)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1) / dist).astype(F)
        dx, dy, dz = (dx * inv).astype(F), (dy * inv).astype(F), (dz * inv).astype(F)
        return (-((dx * a[0]).astype(F) + ((dy * a[1]).astype(F) + (dz * a[2]).astype(F)).astype(F)).astype(F)).astype(F)


def spot_sample32(position, axis, cos_cutoff, cos_beam, p, intensity):
    """-> ({d.x, d.y, d.z, dist} [n, 4], value [n, 4] = ((I inv) inv) f, pdf [n]); the value zeros where f == 0, everything zeros where dist == 0"""
    d, value = D.point_sample32(position, p, intensity)
    c = spot_cosine32(position, axis, p)
    f = falloff32(c, cos_cutoff, cos_beam)
    with np.errstate(invalid="ignore", over="ignore"):
        value = (value * f[:, None]).astype(F)
    dark = (f == 0) | (d[:, 3] == 0)
    value[dark] = 0
    return d, value, np.where(dark, F(0), F(1)).astype(F)


def env_radius32(vertices):
    """the radius of the sphere around the scene's bounding box (constant.cpp:21-28), as msk_scene_tables.h computes it"""
    v = np.asarray(vertices, F).reshape(-1, 8)[:, :3]
    lo, hi = v.min(0), v.max(0)
    c = ((lo + hi).astype(F) * F(0.5)).astype(F)
    r = (c - hi).astype(F)
    radius = np.sqrt(((r[0] * r[0]).astype(F) + ((r[1] * r[1]).astype(F) + (r[2] * r[2]).astype(F)).astype(F)).astype(F)).astype(F)
    return max(RAY_EPS, F(radius * F(F(1) + RAY_EPS)))


def sun_sample32(direction, env_radius, irradiance):
    """-> ({-w.x, -w.y, -w.z, 2 env_radius} [n, 4], value [n, 4] = E): the same from every reference point"""
    e = np.asarray(irradiance, F).reshape(-1, 4)
    w = np.asarray(direction, F)
    d = np.empty((len(e), 4), F)
    d[:, :3] = -w
    d[:, 3] = F(F(2) * F(env_radius))
    return d, e.copy()


# ----------------------------------------------------------------------------- float64
def falloff64(c, cos_cutoff, cos_beam):
    c = np.asarray(c, np.float64)
    cc, cb = float(cos_cutoff), float(cos_beam)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (c - cc) / (cb - cc)
        s = t * t * (3.0 - 2.0 * t)
    return np.where(c >= cb, 1.0, np.where(c <= cc, 0.0, s))


def spot_cosine64(x, position, axis):
    """the cosine between the spot's axis and the direction from the lamp to x"""
    v = np.asarray(x, np.float64) - np.asarray(position, np.float64)
    return (v @ np.asarray(axis, np.float64)) / np.sqrt((v * v).sum(-1))


def spot_geometry(x, n, position, axis, cos_cutoff, cos_beam):
    """cos(theta) / d^2 times the cone factor, at the surface points x with normal n"""
    return D.point_geometry(x, n, position) * falloff64(spot_cosine64(x, position, axis), cos_cutoff, cos_beam)


def sun_geometry(n, direction):
    """|n . w| of a twosided surface; max(-(n . w), 0) is the one-sided value"""
    return abs(float(np.asarray(n, np.float64) @ np.asarray(direction, np.float64)))
