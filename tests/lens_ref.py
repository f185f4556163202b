"""The camera ray of include/msk_gpu.h (msk_camera_desc, msk_lens_desc) restated in numpy fp32, one rounded operation at a time,
and the float64 geometry the thin-lens tests hold the device to.

fp32: `camera_ray32` is the pinhole (lens=None) or the six steps of msk_lens_desc.  The sine and cosine of the concentric disk map
come from the oracle binding's det_math (as envmap_ref.py takes them): the bits the device's det_sincos returns.  Everything else
is numpy float32 arithmetic, which rounds every operation to nearest as the device does (IEEE division and square root, no
contraction).

float64: the disk map, the focus point, and the fraction of the lens disk from which a film position sees the lit side of an edge
(a circular segment), for the blur test.
"""
import numpy as np

import envmap_ref as E

F = np.float32
PI = E.PI
PI_4, PI_2 = F(PI / F(4)), F(PI / F(2))


def disk32(oracle, u):
    """square_to_uniform_disk_concentric (core/warp.h:17-32) in fp32: u float32[n, 2] -> float32[n, 2]"""
    u = np.ascontiguousarray(u, F).reshape(-1, 2)
    x = (F(2) * u[:, 0] - F(1)).astype(F)
    y = (F(2) * u[:, 1] - F(1)).astype(F)
    zero = (x == 0) & (y == 0)
    first = ~zero & ((x * x).astype(F) > (y * y).astype(F))
    with np.errstate(divide="ignore", invalid="ignore"):
        phi_a = (PI_4 * (y / x).astype(F)).astype(F)
        phi_b = (PI_2 - ((x / y).astype(F) * PI_4).astype(F)).astype(F)
    r = np.where(zero, F(0), np.where(first, x, y)).astype(F)
    phi = np.where(zero, F(0), np.where(first, phi_a, phi_b)).astype(F)
    s, c = E.det_sincos(oracle, phi)
    return np.stack([(r * c).astype(F), (r * s).astype(F)], -1)


def _rows4(m, x, y, z, w):
    """((m0 x + m1 y) + m2 z) + m3 w per row of the row-major 4 x 4 m: Transform4f::apply_point before the division"""
    return [((((m[q, 0] * x).astype(F) + (m[q, 1] * y).astype(F)).astype(F) + (m[q, 2] * z).astype(F)).astype(F) + (m[q, 3] * w).astype(F)).astype(F)
            for q in range(4)]


def _normalized(x, y, z):
    n2 = ((x * x).astype(F) + ((y * y).astype(F) + (z * z).astype(F)).astype(F)).astype(F)
    l = np.sqrt(n2).astype(F)
    ok = n2 > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return [np.where(ok, (c / l).astype(F), c).astype(F) for c in (x, y, z)]


def near_point32(desc, px, py):
    s2c = np.array(desc.camera.sample_to_camera[:], F).reshape(4, 4)
    px, py = np.asarray(px, F), np.asarray(py, F)
    zero, one = np.zeros_like(px), np.ones_like(px)
    r = _rows4(s2c, px, py, zero, one)
    return [(r[k] / r[3]).astype(F) for k in range(3)]


def camera_ray32(oracle, desc, film_pos, u=None, lens=None):
    """-> float32[n, 8] = {o, tnear, d, tfar}.  lens: (aperture_radius, focus_distance) or None for the pinhole (u is then unused)"""
    p = np.ascontiguousarray(film_pos, F).reshape(-1, 2)
    tw = np.array(desc.camera.to_world[:], F).reshape(4, 4)
    near, far = F(desc.camera.near_clip), F(desc.camera.far_clip)
    nx, ny, nz = near_point32(desc, p[:, 0], p[:, 1])
    zero, one = np.zeros_like(nx), np.ones_like(nx)
    if lens is None:
        lx, ly = zero, zero
        dl = _normalized(nx, ny, nz)
    else:
        radius, focus = F(lens[0]), F(lens[1])
        a = disk32(oracle, u)
        lx, ly = (a[:, 0] * radius).astype(F), (a[:, 1] * radius).astype(F)
        ft = (focus / nz).astype(F)
        fx, fy, fz = (nx * ft).astype(F), (ny * ft).astype(F), (nz * ft).astype(F)
        dl = _normalized((fx - lx).astype(F), (fy - ly).astype(F), fz)
    inv_z = (F(1) / dl[2]).astype(F)
    o4 = _rows4(tw, lx, ly, zero, one)
    o = [(o4[k] / o4[3]).astype(F) for k in range(3)]
    d = [((tw[q, 0] * dl[0]).astype(F) + ((tw[q, 1] * dl[1]).astype(F) + (tw[q, 2] * dl[2]).astype(F)).astype(F)).astype(F) for q in range(3)]
    return np.stack(o + [(near * inv_z).astype(F)] + d + [(far * inv_z).astype(F)], -1).astype(F)


# ----------------------------------------------------------------------------- float64
def disk64(u):
    """the concentric map in float64 with libm's sine and cosine"""
    u = np.asarray(u, np.float64).reshape(-1, 2)
    x, y = 2 * u[:, 0] - 1, 2 * u[:, 1] - 1
    first = x * x > y * y
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(first, (np.pi / 4) * (y / x), np.pi / 2 - (x / y) * (np.pi / 4))
    r = np.where(first, x, y)
    zero = (x == 0) & (y == 0)
    r, phi = np.where(zero, 0.0, r), np.where(zero, 0.0, phi)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], -1)


def near_point64(desc, px, py):
    s2c = np.array(desc.camera.sample_to_camera[:], np.float64).reshape(4, 4)
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    p = np.stack([px, py, np.zeros_like(px), np.ones_like(px)], -1) @ s2c.T
    return p[..., :3] / p[..., 3:]


def focus_point64(desc, px, py, focus):
    """near_p * f / near_p.z in camera space: where every lens ray of the film position crosses the plane z = f"""
    n = near_point64(desc, px, py)
    return n * (float(focus) / n[..., 2:3])


def segment_fraction(h):
    """The fraction of the unit disk with x > h (a circular segment), float64; h <= -1 gives 1, h >= 1 gives 0"""
    h = np.clip(np.asarray(h, np.float64), -1.0, 1.0)
    return (np.arccos(h) - h * np.sqrt(1.0 - h * h)) / np.pi


def lit_fraction(fx, x0, radius, z_e, focus):
    """p: the fraction of the lens (a disk of `radius`) whose rays towards the focus point (x = fx on the plane z = focus) cross the
    plane z = z_e at x > x0.  The ray from lens point a crosses it at a.x (1 - s) + fx s with s = z_e / focus."""
    s = float(z_e) / float(focus)
    k = 1.0 - s
    fx = np.asarray(fx, np.float64)
    if k == 0.0:
        return (fx * s > x0).astype(np.float64)
    t = (x0 - fx * s) / (k * float(radius))             # a.x / radius > t  (k > 0)  or  < t  (k < 0)
    return segment_fraction(t) if k > 0 else 1.0 - segment_fraction(t)
