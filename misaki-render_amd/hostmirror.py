"""Python mirror of the reference's HOST side of the hot path (setup only, no per-sample work).

What the reference's host does before SamplingIntegrator::render runs, restated so that
Python callers (tests, bench.py, smoke) can build the flattened `msk_scene_desc` the C ABI takes:

  * synthetic Cornell-box meshes (the reference ships none) and the
    OBJ loader's quad split + vertex layout (src/librender/shapes/obj.cpp:104-142)
  * PerspectiveCamera matrices (sensors/perspective.cpp:11-19, core/transform.h:169-187)
  * Gaussian reconstruction filter LUT (filters/gaussian.cpp:10-20, rfilter.cpp:12-27)
  * srgb / srgb_d65 texture parameters (spectra/srgb.cpp:13-19, srgb_d65.cpp:13-31) through
    this package's own Jakob-Hanika style spectral upsampling (rgb2spec.py)
  * HDRFilm::image() develop step (films/hdrfilm.cpp:48-90)

The C++ host library (misaki-render_amd/host/) provides the same through the reference's
plugin/Properties/XML interface; this module is the scripting-side equivalent.
"""
import copy
import ctypes as C
import json
import math
import os

import numpy as np

from . import abi

_PKG = os.path.dirname(os.path.abspath(__file__))


def cie_tables():
    """(cie1931_xyz float32[3*95], d65 float32[95]) — the tables the host hands to the back end."""
    d = json.load(open(os.path.join(_PKG, "data", "cie_tables.json")))
    xyz = np.array(d["cie1931_x"] + d["cie1931_y"] + d["cie1931_z"], np.float32)
    return xyz, np.array(d["d65"], np.float32)


# ----------------------------------------------------------------------------- filter
# ONE flattener truth (round 5): this module and the C++ host library (host/src/render.cpp, core.cpp) produce the same bits for
# the camera matrices and the filter table — tests/test_host_library.py holds them to np.array_equal at three film sizes.  What
# they share is the arithmetic, restated here operation for operation: the filter in fp32 with the C library's expf (numpy's
# own vectorised exp differs from it in the last place), the transforms in fp64 — Transform4f keeps a matrix and its inverse,
# products multiply both, inverse() swaps them, one rounding to fp32 at the end — which is NOT the reference's arithmetic
# to the bit: that is Eigen's fp32 4x4 product and its SSE cofactor inverse (transform.h:87-187), not reproducible without Eigen;
# the fp64 path is what those fp32 results approximate, and both of this repository's hosts now round it the same way.
_libm = C.CDLL("libm.so.6")
_libm.expf.restype, _libm.expf.argtypes = C.c_float, [C.c_float]


def _expf(x):
    return np.float32(_libm.expf(C.c_float(float(x))))


def gaussian_filter(stddev=0.5):
    """GaussianFilter ctor + ReconstructionFilter::init_discretization in fp32 (gaussian.cpp:10-20, rfilter.cpp:12-27), with the
    operations and the expf of host/src/render.cpp.  Returns (radius, lut[33])."""
    f = np.float32
    n = abi.MSK_FILTER_RESOLUTION
    stddev = f(stddev)
    radius = f(f(4) * stddev)
    alpha = f(f(-1.0) / f(f(f(2.0) * stddev) * stddev))
    bias = _expf(f(f(alpha * radius) * radius))
    vals = np.zeros(n + 1, np.float32)
    s = f(0)
    for i in range(n):
        x = f(f(radius * f(i)) / f(n))
        vals[i] = max(f(0), f(_expf(f(f(alpha * x) * x)) - bias))
        s = f(s + vals[i])
    s = f(s * f(f(f(2) * radius) / f(n)))
    norm = f(f(1.0) / s)
    for i in range(n):
        vals[i] = f(vals[i] * norm)
    return float(radius), vals


# ----------------------------------------------------------------------------- camera
class _T4:
    """Transform4f of the C++ host (core.h:64-80, core.cpp:80-175): a 4x4 matrix and its inverse in fp64."""

    def __init__(self, m, inv=None):
        self.m = [list(map(float, r)) for r in m]
        self.inv = [list(map(float, r)) for r in inv] if inv is not None else _T4._inverse(self.m)

    @staticmethod
    def _mul(a, b):                      # Matrix4f::operator*: sum over k = 0..3, left to right, from 0
        out = [[0.0] * 4 for _ in range(4)]
        for i in range(4):
            for j in range(4):
                acc = 0.0
                for k in range(4):
                    acc += a[i][k] * b[k][j]
                out[i][j] = acc
        return out

    @staticmethod
    def _inverse(m):                     # Matrix4f::inverse: Gauss-Jordan with partial pivoting
        a = [list(m[i]) + [1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
        for c in range(4):
            p = c
            for r in range(c + 1, 4):
                if abs(a[r][c]) > abs(a[p][c]):
                    p = r
            if a[p][c] == 0.0:
                return [[float("nan")] * 4 for _ in range(4)]
            if p != c:
                a[p], a[c] = a[c], a[p]
            inv = 1.0 / a[c][c]
            for j in range(8):
                a[c][j] *= inv
            for r in range(4):
                if r != c:
                    fct = a[r][c]
                    if fct != 0.0:
                        for j in range(8):
                            a[r][j] -= fct * a[c][j]
        return [a[i][4:] for i in range(4)]

    def __mul__(self, t):
        return _T4(_T4._mul(self.m, t.m), _T4._mul(t.inv, self.inv))

    def inverse(self):
        return _T4(self.inv, self.m)

    def to_float16(self, inverse=False):
        return np.array(self.inv if inverse else self.m, np.float64).astype(np.float32).reshape(16)

    @staticmethod
    def scale(v):
        v = [float(np.float32(x)) for x in v]
        return _T4([[v[0], 0, 0, 0], [0, v[1], 0, 0], [0, 0, v[2], 0], [0, 0, 0, 1]],
                   [[1.0 / v[0], 0, 0, 0], [0, 1.0 / v[1], 0, 0], [0, 0, 1.0 / v[2], 0], [0, 0, 0, 1]])

    @staticmethod
    def translate(v):
        v = [float(np.float32(x)) for x in v]
        return _T4([[1, 0, 0, v[0]], [0, 1, 0, v[1]], [0, 0, 1, v[2]], [0, 0, 0, 1]],
                   [[1, 0, 0, -v[0]], [0, 1, 0, -v[1]], [0, 0, 1, -v[2]], [0, 0, 0, 1]])

    @staticmethod
    def perspective(fov, near, far):
        fov, near, far = np.float32(fov), float(np.float32(near)), float(np.float32(far))
        recip = 1.0 / (far - near)
        cot = 1.0 / math.tan(float(fov / np.float32(2.0)) * (math.pi / 180.0))
        return _T4([[cot, 0, 0, 0], [0, cot, 0, 0], [0, 0, far * recip, -near * far * recip], [0, 0, 1, 0]])

    @staticmethod
    def lookat(origin, target, up):
        o, t, u = ([float(np.float32(x)) for x in v] for v in (origin, target, up))

        def nrm(v):
            l = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            return [v[0] / l, v[1] / l, v[2] / l]

        def crs(a, b):
            return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        d = nrm([t[0] - o[0], t[1] - o[1], t[2] - o[2]])
        left = nrm(crs(nrm(u), d))
        nup = nrm(crs(d, left))
        return _T4([[left[r], nup[r], d[r], o[r]] for r in range(3)] + [[0, 0, 0, 1]])


def perspective_camera(fov, near, far, width, height, origin, target, up):
    """-> (sample_to_camera[16], to_world[16]) row-major float32; sample space is in pixels.

    perspective.cpp:11-19: camera_to_sample = S(w,h,1) S(-.5,-.5a,1) T(-1,-1/a,0) P(fov,near,far), sample_to_camera its inverse;
    to_world = lookat (transform.h:169-178).  The C++ host's arithmetic (see the note above gaussian_filter), bit for bit.
    """
    f = np.float32
    aspect = f(f(width) / f(height))                 # sensor.cpp: size.x / (float) size.y
    c2s = _T4.scale((f(width), f(height), f(1))) * _T4.scale((f(-0.5), f(f(-0.5) * aspect), f(1))) * \
        _T4.translate((f(-1), f(f(-1) / aspect), f(0))) * _T4.perspective(fov, near, far)
    return c2s.inverse().to_float16(), _T4.lookat(origin, target, up).to_float16()


# ----------------------------------------------------------------------------- meshes
class MeshSpec:
    """One <shape type="obj"> of the scene: faces as 3- or 4-tuples of 3D points."""

    def __init__(self, name, faces, reflectance, radiance=None, translate=(0, 0, 0), normals=None, bsdf=None, texcoords=None):
        """bsdf: None = <bsdf type="diffuse"> with `reflectance`; or a dict for a rough conductor
        {"type": "roughconductor", "alpha": a | ("alpha_u","alpha_v"), "eta": rgb, "k": rgb,
         "specular_reflectance": rgb (default 1), "sample_visible": bool, "twosided": bool}, a rough dielectric,
        {"type": "dielectric", "int_ior": 1.49, "ext_ior": 1.00028, "specular_reflectance": rgb | c, "specular_transmittance": rgb | c}
        (the smooth interface; a scalar c = the `uniform` spectrum <spectrum value="c"/>), or
        {"type": "conductor", "eta": rgb | c (default 0), "k": rgb | c (default 1), "specular_reflectance": rgb | c (default 1),
         "twosided": bool} (the smooth conductor: a mirror), or
        {"type": "plastic", "diffuse_reflectance": rgb | c (default 0.5) | a Regular | a checkerboard or bitmap texture as below,
         "specular_reflectance": rgb | c (default 1), "int_ior": 1.49, "ext_ior": 1.00028, "nonlinear": bool (default False),
         "twosided": bool} (a smooth dielectric coat over a diffuse base; the mesh's `reflectance` is not read), or
        {"type": "roughplastic", the plastic's keys, "alpha": a (default 0.1) | (au, av) with au == av, "distribution": "ggx"}
         (the plastic with a GGX coat; "beckmann", unequal alphas and "sample_visible": True are refused), or
        {"type": "diffuse", "twosided": bool, "texture": {"type": "checkerboard", "color0": rgb, "color1": rgb,
         "scale": (sx, sy) | "matrix": 16 floats (the to_uv 4x4, row-major)}} (texture absent = `reflectance`), or the texture
        {"type": "bitmap", "pixels": float32 [H, W, 3] linear RGB (row 0 = texel row 0 = the image's top row),
         "filter": "bilinear" (default) | "nearest", "scale" | "matrix" (default: identity)}; or any of them under a mask,
        {"type": "mask", "opacity": 0.5 (default) | rgb (reduced to its luminance) | a bitmap texture as above with pixels
         float32 [H, W] or [H, W, 3], "bsdf": {...}} (bsdfs/mask.cpp; the nested BSDF may be "twosided", the mask itself may not).
        texcoords: None, or per face a tuple of (u, v) per corner as written in the OBJ `vt` lines (the loader stores 1 - v)."""
        self.name, self.faces, self.reflectance, self.radiance = name, faces, reflectance, radiance
        self.translate, self.normals, self.bsdf, self.texcoords = translate, normals, bsdf, texcoords


def triangulate(mesh):
    """OBJ loader semantics: 8 floats per vertex, quad (v0,v1,v2,v3) -> (v0,v1,v2),(v3,v0,v2)
    (obj.cpp:104-133); `to_world` translate applied to positions at load (obj.cpp:90)."""
    verts, faces = [], []
    tr = np.asarray(mesh.translate, np.float32)
    for fi, f in enumerate(mesh.faces):
        base = len(verts)
        for ci, p in enumerate(f):
            # Transform4f::apply_point with a pure translation: p + t in fp32
            q = np.asarray(p, np.float32) + tr
            uv = mesh.texcoords[fi][ci] if mesh.texcoords is not None else (0, 0)
            verts.append([q[0], q[1], q[2], 0, 0, 0, np.float32(uv[0]),
                          (np.float32(1) - np.float32(uv[1])) if mesh.texcoords is not None else 0])   # flip_tex_coords, obj.cpp:96-97
        if len(f) == 3:
            faces.append([base, base + 1, base + 2])
        else:
            faces.append([base, base + 1, base + 2])
            faces.append([base + 3, base, base + 2])
    return np.array(verts, np.float32).reshape(-1, 8), np.array(faces, np.uint32).reshape(-1, 3)


def write_obj(mesh, path):
    """The same geometry as an OBJ file the reference's loader (and the C++ host) can read."""
    with open(path, "w") as fh:
        fh.write(f"# {mesh.name}: synthetic Cornell-box mesh (classic Cornell data)\n")
        n = 0
        for fi, f in enumerate(mesh.faces):
            for p in f:
                fh.write("v %.9g %.9g %.9g\n" % tuple(float(np.float32(c)) for c in p))
            if mesh.texcoords is not None:
                for uv in mesh.texcoords[fi]:
                    fh.write("vt %.9g %.9g\n" % tuple(float(np.float32(c)) for c in uv))
                fh.write("f " + " ".join("%d/%d" % (n + i + 1, n + i + 1) for i in range(len(f))) + "\n")
            else:
                fh.write("f " + " ".join(str(n + i + 1) for i in range(len(f))) + "\n")
            n += len(f)


def write_pfm(path, pixels, little_endian=True):
    """pixels float32 [H, W, 3] (or [H, W]: one channel), row 0 = the top row -> a PFM file, which stores the bottom row first."""
    a = np.asarray(pixels, np.float32)
    h, w = a.shape[:2]
    with open(path, "wb") as fh:
        fh.write(b"%s\n%d %d\n%s\n" % (b"PF" if a.ndim == 3 else b"Pf", w, h, b"-1.0" if little_endian else b"1.0"))
        fh.write(a[::-1].astype("<f4" if little_endian else ">f4").tobytes())


MASK_TWOSIDED = 'mask: a "twosided" BSDF cannot hold a mask; write mask(twosided(X))'
MASK_NESTED = "mask: a mask cannot be nested in a mask"
MASK_CHILDREN = "mask: exactly one nested BSDF is required"
MASK_UNKNOWN = 'mask: nested object "%s" is neither a BSDF nor the texture "opacity"'


def _mask_nested(spec):
    """The nested BSDF spec of {"type": "mask", "opacity": ..., "bsdf": {...}}, after the refusals both flatteners word alike."""
    if spec.get("twosided"):
        raise ValueError(MASK_TWOSIDED)
    for key, value in spec.items():
        if key not in ("type", "opacity", "bsdf", "twosided") and isinstance(value, dict):
            raise ValueError(MASK_UNKNOWN % key)
    nested = spec.get("bsdf")
    if not isinstance(nested, dict):
        raise ValueError(MASK_CHILDREN)
    if nested.get("type") == "mask":
        raise ValueError(MASK_NESTED)
    return nested


def luminance32(rgb):
    """What both flatteners reduce a coloured opacity to: a grey is its value, any other colour 0.212671 r + 0.715160 g + 0.072169 b
    in fp32, left to right"""
    rgb = np.asarray(rgb, np.float32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    lum = (np.float32(0.212671) * r + np.float32(0.715160) * g) + np.float32(0.072169) * b
    return np.where((r == g) & (g == b), r, lum).astype(np.float32)


def _mask_desc(spec, index, keep):
    """msk_mask_desc of a mask spec on BSDF entry `index` (msk_gpu.h); an image's values are appended to `keep`"""
    k = abi.MaskDesc()
    k.bsdf = index
    op = spec.get("opacity", 0.5)
    if isinstance(op, dict):
        if op.get("type") != "bitmap":
            raise ValueError('mask: "opacity" must be a float, a colour or a bitmap texture')
        px = np.asarray(op["pixels"], np.float32)
        if px.ndim == 3 and px.shape[2] == 3:
            px = luminance32(px)
        if px.ndim != 2 or px.shape[0] < 1 or px.shape[1] < 1:
            raise ValueError("mask: opacity pixels must be float32 [H, W] or [H, W, 3]")
        filt = op.get("filter", "bilinear")
        if filt not in ("bilinear", "nearest"):
            raise ValueError("bitmap filter %r (bilinear or nearest)" % (filt,))
        vals = np.ascontiguousarray(px, np.float32)
        keep.append(vals)
        k.filter = 2 if filt == "bilinear" else 1
        k.height, k.width = vals.shape
        k.values = vals.ctypes.data_as(C.POINTER(C.c_float))
        if "scale" in op:
            m4 = np.diag([op["scale"][0], op["scale"][1], 1.0, 1.0]).astype(np.float32)
        elif "matrix" in op:
            m4 = np.asarray(op["matrix"], np.float32).reshape(4, 4)
        else:
            m4 = np.eye(4, dtype=np.float32)
        k.to_uv[:] = [float(x) for x in (m4[0, 0], m4[0, 1], m4[0, 2], m4[1, 0], m4[1, 1], m4[1, 2])]
    else:
        k.filter = 0
        k.opacity = float(op) if np.isscalar(op) else float(luminance32(op))
    return k


def _to_uv_xml(tex):
    if "scale" in tex:
        return ['    <transform name="to_uv">', '        <scale x="%.9g" y="%.9g"/>' % tuple(tex["scale"]), '    </transform>']
    if "matrix" in tex:
        return ['    <transform name="to_uv">', '        <matrix value="%s"/>' % " ".join("%.9g" % float(np.float32(x)) for x in tex["matrix"]),
                '    </transform>']
    return []


def _bsdf_xml(m, v3, directory=None):
    """The <bsdf> element of one shape (reference plugin parameter names); a bitmap texture's pixels go to
    <directory>/textures/<shape>.pfm."""
    spec = m.bsdf
    if spec is not None and spec.get("type") == "mask":        # bsdfs/mask.cpp: the opacity and exactly one nested BSDF
        nested = _mask_nested(spec)
        inner_mesh = copy.copy(m)
        inner_mesh.bsdf = nested
        op = spec.get("opacity", 0.5)
        if isinstance(op, dict):
            os.makedirs(os.path.join(directory, "textures"), exist_ok=True)
            write_pfm(os.path.join(directory, "textures", m.name + "_opacity.pfm"), np.asarray(op["pixels"], np.float32))
            op_xml = ['<texture name="opacity" type="bitmap">', '    <string name="filename" value="textures/%s_opacity.pfm"/>' % m.name] + \
                     (['    <string name="filter_type" value="%s"/>' % op["filter"]] if "filter" in op else []) + _to_uv_xml(op) + ['</texture>']
        elif np.isscalar(op):
            op_xml = ['<float name="opacity" value="%.9g"/>' % float(np.float32(op))]
        else:
            op_xml = ['<rgb name="opacity" value="%s"/>' % v3(op)]
        inner = [b[8:] for b in _bsdf_xml(inner_mesh, v3, directory)]
        body = (op_xml if "opacity" in spec else []) + inner
        return ['        ' + b for b in ['<bsdf type="mask">'] + ['    ' + b for b in body] + ['</bsdf>']]
    refl_xml = '<spectrum name="reflectance" value="%s"/>' % m.reflectance.text if isinstance(m.reflectance, Regular) else \
               '<spectrum name="reflectance" value="%.9g"/>' % float(m.reflectance) if np.isscalar(m.reflectance) else \
               '<rgb name="reflectance" value="%s"/>' % v3(m.reflectance)
    if spec is None:
        return ['        <bsdf type="diffuse">', '            ' + refl_xml, '        </bsdf>']
    if spec["type"] == "diffuse":
        tex = spec.get("texture")
        if tex is None:
            body = [refl_xml]
        elif tex["type"] == "bitmap":
            os.makedirs(os.path.join(directory, "textures"), exist_ok=True)
            write_pfm(os.path.join(directory, "textures", m.name + ".pfm"), tex["pixels"])
            body = ['<texture name="reflectance" type="bitmap">', '    <string name="filename" value="textures/%s.pfm"/>' % m.name] + \
                   (['    <string name="filter_type" value="%s"/>' % tex["filter"]] if "filter" in tex else []) + _to_uv_xml(tex) + ['</texture>']
        else:     # textures/checkerboard.cpp:11-15 parameter names, as in results/Figure_2_RoughConductor/roughconductor.xml:35-41
            xf = '<scale x="%.9g" y="%.9g"/>' % tuple(tex["scale"]) if "scale" in tex else \
                 '<matrix value="%s"/>' % " ".join("%.9g" % float(np.float32(x)) for x in tex["matrix"])
            body = ['<texture name="reflectance" type="%s">' % tex["type"], '    <rgb name="color0" value="%s"/>' % v3(tex["color0"]),
                    '    <rgb name="color1" value="%s"/>' % v3(tex["color1"]), '    <transform name="to_uv">', '        ' + xf,
                    '    </transform>', '</texture>']
        inner = ['<bsdf type="diffuse">'] + ['    ' + b for b in body] + ['</bsdf>']
        if spec.get("twosided"):
            inner = ['<bsdf type="twosided">'] + ['    ' + b for b in inner] + ['</bsdf>']
        return ['        ' + b for b in inner]
    if spec["type"] in ("plastic", "roughplastic"):
        return _plastic_xml(m, spec, v3, directory)
    body = []
    if spec["type"] not in ("dielectric", "conductor"):          # (the smooth BSDFs read no microfacet parameters)
        a = spec.get("alpha", 0.1)
        if np.isscalar(a):
            body.append('<float name="alpha" value="%r"/>' % float(a))
        else:
            body += ['<float name="alpha_u" value="%r"/>' % float(a[0]), '<float name="alpha_v" value="%r"/>' % float(a[1])]
        body.append('<string name="distribution" value="ggx"/>')
        if spec.get("sample_visible"):
            body.append('<boolean name="sample_visible" value="true"/>')
    keys = {"roughconductor": ("eta", "k", "specular_reflectance"),
            "roughdielectric": ("specular_reflectance", "specular_transmittance"),
            "dielectric": ("specular_reflectance", "specular_transmittance"),
            "conductor": ("eta", "k", "specular_reflectance")}[spec["type"]]
    for k in keys:
        if k in spec:
            body.append('<spectrum name="%s" value="%s"/>' % (k, spec[k].text) if isinstance(spec[k], Regular) else
                        '<spectrum name="%s" value="%.9g"/>' % (k, float(spec[k])) if np.isscalar(spec[k]) else
                        '<rgb name="%s" value="%s"/>' % (k, v3(spec[k])))
    for k in ("int_ior", "ext_ior"):
        if k in spec:
            body.append('<float name="%s" value="%r"/>' % (k, float(spec[k])))
    inner = ['<bsdf type="%s">' % spec["type"]] + ['    ' + b for b in body] + ['</bsdf>']
    if spec.get("twosided"):
        inner = ['<bsdf type="twosided">'] + ['    ' + b for b in inner] + ['</bsdf>']
    return ['        ' + b for b in inner]


def _texture_xml(name, tex, shape, v3, directory):
    """A <texture name=...> element: a bitmap (its pixels go to <directory>/textures/<shape>.pfm) or a checkerboard"""
    if tex["type"] == "bitmap":
        os.makedirs(os.path.join(directory, "textures"), exist_ok=True)
        write_pfm(os.path.join(directory, "textures", shape + ".pfm"), tex["pixels"])
        return ['<texture name="%s" type="bitmap">' % name, '    <string name="filename" value="textures/%s.pfm"/>' % shape] + \
               (['    <string name="filter_type" value="%s"/>' % tex["filter"]] if "filter" in tex else []) + _to_uv_xml(tex) + ['</texture>']
    xf = '<scale x="%.9g" y="%.9g"/>' % tuple(tex["scale"]) if "scale" in tex else \
         '<matrix value="%s"/>' % " ".join("%.9g" % float(np.float32(x)) for x in tex["matrix"])
    return ['<texture name="%s" type="%s">' % (name, tex["type"]), '    <rgb name="color0" value="%s"/>' % v3(tex["color0"]),
            '    <rgb name="color1" value="%s"/>' % v3(tex["color1"]), '    <transform name="to_uv">', '        ' + xf, '    </transform>', '</texture>']


PLASTIC_SPECULAR = 'plastic: "specular_reflectance" must be a constant spectrum or an rgb (a texture that varies over the surface is not supported)'
# the `roughplastic` plugin's refusals, in the C++ host's words (host/src/render.cpp: RoughPlastic)
ROUGHPLASTIC_SPECULAR = "rough" + PLASTIC_SPECULAR
ROUGHPLASTIC_BECKMANN = 'roughplastic: the "beckmann" distribution is not implemented (use "ggx")'
ROUGHPLASTIC_DISTRIBUTION = 'Specified an invalid distribution "%s", must be "beckmann" or "ggx"!'
ROUGHPLASTIC_ANISOTROPIC = 'roughplastic: "alpha_u" and "alpha_v" differ: anisotropic coats are not supported (give "alpha", or two equal values)'
ROUGHPLASTIC_VISIBLE = ('roughplastic: "sample_visible" = true is not supported: the reference draws the coat\'s normal from D(m) cos(theta_m) whatever the '
                        'flag and returns the visible-normal density under it, which biases sample = eval / pdf')


def _plastic_xml(m, spec, v3, directory):
    """<bsdf type="plastic"> or <bsdf type="roughplastic"> with the properties the spec names (an absent one takes the plugin's default)"""
    body = []
    if "diffuse_reflectance" in spec:
        d = spec["diffuse_reflectance"]
        if isinstance(d, dict):
            body += _texture_xml("diffuse_reflectance", d, m.name, v3, directory)
        else:
            body.append('<spectrum name="diffuse_reflectance" value="%s"/>' % d.text if isinstance(d, Regular) else
                        '<spectrum name="diffuse_reflectance" value="%.9g"/>' % float(d) if np.isscalar(d) else
                        '<rgb name="diffuse_reflectance" value="%s"/>' % v3(d))
    if "specular_reflectance" in spec:
        sr = spec["specular_reflectance"]
        if isinstance(sr, dict):
            body += _texture_xml("specular_reflectance", sr, m.name + "_specular", v3, directory)
        else:
            body.append('<spectrum name="specular_reflectance" value="%.9g"/>' % float(sr) if np.isscalar(sr) else
                        '<rgb name="specular_reflectance" value="%s"/>' % v3(sr))
    for k in ("int_ior", "ext_ior"):
        if k in spec:
            body.append('<float name="%s" value="%r"/>' % (k, float(spec[k])))
    if "nonlinear" in spec:
        body.append('<boolean name="nonlinear" value="%s"/>' % ("true" if spec["nonlinear"] else "false"))
    if spec["type"] == "roughplastic":
        if "alpha" in spec:
            a = spec["alpha"]
            body += ['<float name="alpha" value="%r"/>' % float(a)] if np.isscalar(a) else \
                    ['<float name="alpha_u" value="%r"/>' % float(a[0]), '<float name="alpha_v" value="%r"/>' % float(a[1])]
        if "distribution" in spec:
            body.append('<string name="distribution" value="%s"/>' % spec["distribution"])
        if "sample_visible" in spec:
            body.append('<boolean name="sample_visible" value="%s"/>' % ("true" if spec["sample_visible"] else "false"))
    inner = ['<bsdf type="%s">' % spec["type"]] + ['    ' + b for b in body] + ['</bsdf>']
    if spec.get("twosided"):
        inner = ['<bsdf type="twosided">'] + ['    ' + b for b in inner] + ['</bsdf>']
    return ['        ' + b for b in inner]


DIRECT_MAX_SAMPLES = 4096


def direct_integrator(props=None):
    """The constructor of the host library's `"direct"` plugin (host/src/render.cpp: DirectIntegrator), property for property and
    refusal for refusal (the same words): props -> {"light_samples", "bsdf_samples", "gpu_device", "honor_properties",
    "block_size", "hide_emitters"} with the plugin's defaults filled in (a property the plugin does not read is ignored, as the
    plugin ignores it).  Raises ValueError where the plugin throws."""
    props = dict(props or {})
    devices = [t for t in str(props.get("gpu_devices", "")).replace(",", " ").split() if t]
    if len(devices) > 1:
        raise ValueError('"gpu_devices": the "direct" integrator renders on one device (got %d); run one process per GPU and shard the samples' % len(devices))
    n, m = int(props.get("light_samples", 1)), int(props.get("bsdf_samples", 1))
    if n < 0:
        raise ValueError('"light_samples" must be >= 0 (got %d)' % n)
    if m < 0:
        raise ValueError('"bsdf_samples" must be >= 0 (got %d)' % m)
    if n > DIRECT_MAX_SAMPLES:
        raise ValueError('"light_samples" must be at most 4096 (got %d)' % n)
    if m > DIRECT_MAX_SAMPLES:
        raise ValueError('"bsdf_samples" must be at most 4096 (got %d)' % m)
    if n == 0 and m == 0:
        raise ValueError('"light_samples" and "bsdf_samples" must not both be 0')
    as_bool = lambda v: v if isinstance(v, bool) else str(v).lower() == "true"
    return {"light_samples": n, "bsdf_samples": m, "gpu_device": int(devices[0]) if devices else int(props.get("gpu_device", 0)),
            "honor_properties": as_bool(props.get("honor_properties", False)), "block_size": int(props.get("block_size", 32)),
            "hide_emitters": as_bool(props.get("hide_emitters", False))}


def read_integrator(xml_path):
    """The <integrator> element of a scene XML -> (plugin name, its properties as the plugin's constructor settles them).  "direct"
    goes through direct_integrator (and its refusals); any other integrator's properties are returned as written."""
    import xml.etree.ElementTree as ET
    node = ET.parse(str(xml_path)).getroot().find("integrator")
    if node is None:
        raise ValueError("the scene has no integrator")
    conv = {"integer": int, "boolean": lambda v: v.lower() == "true", "string": str, "float": float}
    props = {c.get("name"): conv[c.tag](c.get("value")) for c in node if c.tag in conv}
    kind = node.get("type")
    return kind, (direct_integrator(props) if kind == "direct" else props)


def write_scene_xml(meshes, directory, width, height, spp, camera=None, integrator_props=None, film_type="hdrfilm",
                    filename="scene.xml", env=None, film_props=None, points=(), integrator_type="path", lights=()):
    """Writes <directory>/meshes/*.obj and a Mitsuba-style scene XML the C++ host (and the reference's
    loader) understands; same structure as results/Figure_1_Pathtrace/scene.xml, $-parameters for spp/size."""
    camera = camera or CBOX_CAMERA
    os.makedirs(os.path.join(directory, "meshes"), exist_ok=True)
    v3 = lambda v: ", ".join("%.9g" % float(x) for x in v)
    out = ['<scene>', '    <default name="spp" value="%d"/>' % spp, '    <default name="width" value="%d"/>' % width,
           '    <default name="height" value="%d"/>' % height, '    <integrator type="%s">' % integrator_type]
    for k, val in (integrator_props or {}).items():
        tag = "boolean" if isinstance(val, bool) else "string" if isinstance(val, str) else "integer"
        out.append('        <%s name="%s" value="%s"/>' % (tag, k, str(val).lower()))
    # a camera with "aperture_radius" is a `thinlens` sensor ("focus_distance" is written when given: the plugin's default is far_clip)
    lens = ['        <float name="%s" value="%.9g"/>' % (k, float(np.float32(camera[k]))) for k in ("aperture_radius", "focus_distance") if k in camera]
    out += ['    </integrator>', '    <sensor type="%s">' % ("thinlens" if "aperture_radius" in camera else "perspective")] + lens + [
            '        <float name="near_clip" value="%.9g"/>' % camera["near"], '        <float name="far_clip" value="%.9g"/>' % camera["far"],
            '        <float name="fov" value="%.9g"/>' % camera["fov"], '        <transform name="to_world">',
            '            <lookat origin="%s" target="%s" up="%s"/>' % (v3(camera["origin"]), v3(camera["target"]), v3(camera["up"])),
            '        </transform>', '        <sampler type="independent">', '            <integer name="sample_count" value="$spp"/>',
            '        </sampler>', '        <film type="%s">' % film_type, '            <integer name="width" value="$width"/>',
            '            <integer name="height" value="$height"/>'] + \
           ['            <integer name="%s" value="%d"/>' % (k, int(v)) for k, v in (film_props or {}).items()] + ['        </film>', '    </sensor>']

    def env_xml():
        if env.get("type") == "envmap":       # the image goes to <directory>/textures/envmap.pfm
            os.makedirs(os.path.join(directory, "textures"), exist_ok=True)
            write_pfm(os.path.join(directory, "textures", "envmap.pfm"), env["pixels"])
            body = ['        <string name="filename" value="textures/envmap.pfm"/>']
            if "scale" in env:
                body.append('        <float name="scale" value="%.9g"/>' % float(np.float32(env["scale"])))
            if "to_world" in env:
                body += ['        <transform name="to_world">', '            <matrix value="%s"/>' % " ".join("%.9g" % float(x) for x in _env_to_world4(env).reshape(-1)),
                         '        </transform>']
            return ['    <emitter type="envmap">'] + body + ['    </emitter>']
        rad = env.get("radiance")
        body = ['        <spectrum name="radiance" value="%s"/>' % rad.text] if isinstance(rad, Regular) else \
               ['        <rgb name="radiance" value="%s"/>' % v3(rad)] if rad is not None else \
               (['        <spectrum name="radiance" value="%r"/>' % float(env["scale"])] if "scale" in env else [])   # D65 * scale
        return ['    <emitter type="constant">'] + body + ['    </emitter>']
    def point_xml(pt):
        inten = _point_intensity(pt)
        body = ['        <point name="position" x="%.9g" y="%.9g" z="%.9g"/>' % tuple(float(np.float32(x)) for x in pt["position"])] if "position" in pt else []
        if "to_world" in pt:
            body += ['        <transform name="to_world">', '            <matrix value="%s"/>' % " ".join("%.9g" % float(np.float32(x)) for x in np.asarray(pt["to_world"]).reshape(-1)),
                     '        </transform>']
        body += ['        <spectrum name="intensity" value="%s"/>' % inten.text] if isinstance(inten, Regular) else \
                ['        <spectrum name="intensity" value="%.9g"/>' % float(inten)] if np.isscalar(inten) else \
                ['        <rgb name="intensity" value="%s"/>' % v3(inten)]
        return ['    <emitter type="point">'] + body + ['    </emitter>']
    def light_xml(lt):
        spec = _light_spectrum(lt)
        name = "intensity" if lt["type"] == "spot" else "irradiance"
        body = []
        for key in ("cutoff_angle", "beam_width"):
            if key in lt:
                body.append('        <float name="%s" value="%.9g"/>' % (key, float(np.float32(lt[key]))))
        if "direction" in lt:
            body.append('        <vector name="direction" x="%.9g" y="%.9g" z="%.9g"/>' % tuple(float(np.float32(x)) for x in lt["direction"]))
        if "lookat" in lt:
            la = lt["lookat"]
            body += ['        <transform name="to_world">',
                     '            <lookat origin="%s" target="%s" up="%s"/>' % tuple(v3([np.float32(x) for x in la[k]]) for k in ("origin", "target", "up")),
                     '        </transform>']
        elif "to_world" in lt:
            body += ['        <transform name="to_world">', '            <matrix value="%s"/>' % " ".join("%.9g" % float(np.float32(x)) for x in np.asarray(lt["to_world"]).reshape(-1)),
                     '        </transform>']
        body += ['        <spectrum name="%s" value="%s"/>' % (name, spec.text)] if isinstance(spec, Regular) else \
                ['        <spectrum name="%s" value="%.9g"/>' % (name, float(spec))] if np.isscalar(spec) else \
                ['        <rgb name="%s" value="%s"/>' % (name, v3(spec))]
        return ['    <emitter type="%s">' % lt["type"]] + body + ['    </emitter>']
    if env is not None and env.get("first"):
        out += env_xml()
    for pt in points:
        if pt.get("first"):
            out += point_xml(pt)
    for lt in lights:
        if lt.get("first"):
            out += light_xml(lt)
    for m in meshes:
        write_obj(m, os.path.join(directory, "meshes", m.name + ".obj"))
        out += ['    <shape type="obj">', '        <string name="filename" value="meshes/%s.obj"/>' % m.name]
        if any(float(t) != 0 for t in m.translate):
            out += ['        <transform name="to_world">', '            <translate x="%.9g" y="%.9g" z="%.9g"/>' % tuple(m.translate),
                    '        </transform>']
        out += _bsdf_xml(m, v3, directory)
        if m.radiance is not None:
            out += ['        <emitter type="area">', '            <spectrum name="radiance" value="%s"/>' % m.radiance.text if isinstance(m.radiance, Regular)
                    else '            <rgb name="radiance" value="%s"/>' % v3(m.radiance), '        </emitter>']
        out.append('    </shape>')
    if env is not None and not env.get("first"):
        out += env_xml()
    for pt in points:
        if not pt.get("first"):
            out += point_xml(pt)
    for lt in lights:
        if not lt.get("first"):
            out += light_xml(lt)
    out.append('</scene>')
    path = os.path.join(directory, filename)
    open(path, "w").write("\n".join(out) + "\n")
    return path


WHITE = (0.885809, 0.698859, 0.666422)
GREEN = (0.105421, 0.37798, 0.076425)
RED = (0.570068, 0.0430135, 0.0443706)
BOX = (0.45, 0.30, 0.90)
LUMINAIRE = (0.936461, 0.740433, 0.705267)


def cbox_meshes():
    """The 8 shapes of results/Figure_1_Pathtrace/scene.xml:33-103 in XML order (= geomID order),
    geometry from the classic Cornell measurements."""
    q = lambda *p: tuple(p)
    return [
        MeshSpec("cbox_luminaire", [q((343, 548.8, 227), (343, 548.8, 332), (213, 548.8, 332), (213, 548.8, 227))],
                 LUMINAIRE, radiance=(40, 40, 40), translate=(0, -0.5, 0)),
        MeshSpec("cbox_floor", [q((552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2))], WHITE),
        MeshSpec("cbox_ceiling", [q((556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0))], WHITE),
        MeshSpec("cbox_back", [q((549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2))], WHITE),
        MeshSpec("cbox_greenwall", [q((0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2))], GREEN),
        MeshSpec("cbox_redwall", [q((552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0))], RED),
        MeshSpec("cbox_smallbox", [
            q((130, 165, 65), (82, 165, 225), (240, 165, 272), (290, 165, 114)),
            q((290, 0, 114), (290, 165, 114), (240, 165, 272), (240, 0, 272)),
            q((130, 0, 65), (130, 165, 65), (290, 165, 114), (290, 0, 114)),
            q((82, 0, 225), (82, 165, 225), (130, 165, 65), (130, 0, 65)),
            q((240, 0, 272), (240, 165, 272), (82, 165, 225), (82, 0, 225))], BOX),
        MeshSpec("cbox_largebox", [
            q((423, 330, 247), (265, 330, 296), (314, 330, 456), (472, 330, 406)),
            q((423, 0, 247), (423, 330, 247), (472, 330, 406), (472, 0, 406)),
            q((472, 0, 406), (472, 330, 406), (314, 330, 456), (314, 0, 456)),
            q((314, 0, 456), (314, 330, 456), (265, 330, 296), (265, 0, 296)),
            q((265, 0, 296), (265, 330, 296), (423, 330, 247), (423, 0, 247))], BOX),
    ]


CBOX_CAMERA = dict(fov=49.3077, near=10.0, far=2800.0, origin=(278, 273, -800), target=(278, 273, -799),
                   up=(0, 1, 0))


def blob_mesh(name, center, radius, n_theta, n_phi, reflectance, seed=1, bump=0.15):
    """A closed, bumpy, outward-wound triangle mesh (bunny/teapot-class stand-in):
    a UV sphere displaced by a few low-frequency sinusoids.  ~2*n_theta*n_phi triangles."""
    rng = np.random.RandomState(seed)
    k = rng.uniform(1, 4, (4, 2)).round()
    ph = rng.uniform(0, 2 * np.pi, 4)

    def point(i, j):
        th = np.pi * i / n_theta
        p = 2 * np.pi * (j % n_phi) / n_phi
        r = 1.0
        if 0 < i < n_theta:
            for a in range(4):
                r += bump / 4 * np.sin(k[a, 0] * th * 2 + ph[a]) * np.cos(k[a, 1] * p + ph[a])
        d = np.array([np.sin(th) * np.cos(p), np.cos(th), np.sin(th) * np.sin(p)])
        return tuple(np.asarray(center, np.float64) + radius * r * d)

    faces = []
    for i in range(n_theta):
        for j in range(n_phi):
            a, b, c, d = point(i, j), point(i + 1, j), point(i + 1, j + 1), point(i, j + 1)
            if i == 0:
                faces.append((a, c, b))
            elif i == n_theta - 1:
                faces.append((a, d, b))
            else:
                faces.append((a, d, c))
                faces.append((a, c, b))
    return MeshSpec(name, faces, reflectance)


MSK_CIE_Y_NORMALIZATION = np.float32(1.0 / 106.7502593994140625)       # include/misaki/core/spectrum.h:75


class Regular:
    """A tabulated spectrum on a regular grid = the reference's `regular` texture (spectra/regular.cpp:27-91): what
    <spectrum value="l0:v0, l1:v1, ..."/> with equidistant wavelengths makes (xml.cpp:300-341).  Accepted wherever the mirror takes
    an rgb: MeshSpec.reflectance, MeshSpec.radiance, a BSDF's eta / k / specular_*, the environment's radiance."""

    def __init__(self, lambda_min, lambda_max, values, text=None):
        self.lambda_min, self.lambda_max = float(np.float32(lambda_min)), float(np.float32(lambda_max))
        self.values = np.asarray(values, np.float32).copy()
        self.text = text          # the "l:v, l:v, ..." it was parsed from (write_scene_xml writes it back)

    @staticmethod
    def from_pairs(text, within_emitter=False):
        """create_texture_from_spectrum (xml.cpp:279-341) for "l:v, l:v, ...": values x MSK_CIE_Y_NORMALIZATION inside an
        <emitter>; the steps must agree within math::Epsilon (else the reference makes an `irregular` spectrum, which the back
        end does not take)."""
        pairs = [t.split(":") for t in text.replace(",", " ").split()]
        wl = np.array([np.float32(a) for a, _ in pairs], np.float32)
        v = np.array([np.float32(b) for _, b in pairs], np.float32)
        if within_emitter:
            v = v * MSK_CIE_Y_NORMALIZATION
        step = np.diff(wl)
        if (step < 0).any():
            raise ValueError("Wavelengths must be specified in increasing order!")
        if len(wl) > 2 and (np.abs(step[1:] - step[0]) > np.float32(2.0 ** -24)).any():
            raise ValueError("irregular spectrum (unequal wavelength steps): not supported by the GPU path integrator")
        return Regular(wl[0], wl[-1], v, text=text)


class _RegularPool:
    """The scene's regular_spectra / regular_values arrays while a scene is flattened."""

    def __init__(self):
        self.descs, self.values = [], []

    def add(self, r):
        n = len(r.values)
        if not (2 <= n <= abi.MSK_REGULAR_MAX):
            raise ValueError("a regular spectrum needs 2..%d values (got %d)" % (abi.MSK_REGULAR_MAX, n))
        self.descs.append(abi.RegularSpectrumDesc(r.lambda_min, r.lambda_max, n, len(self.values)))
        self.values += [float(x) for x in r.values]
        return len(self.descs)


def spectrum_desc(rgb, fetch, pool=None):
    """rgb -> msk_spectrum_desc.  In-gamut colours: S(fetch(rgb)); values above 1 (conductor eta/k) use the
    normalisation of spectra/srgb_d65.cpp:18-22 without the D65 factor: scale = 2 max, fetch(rgb / scale).
    A Regular: the tabulated form (its index in the scene's pool)."""
    if isinstance(rgb, Regular):
        return abi.SpectrumDesc((C.c_float * 3)(0.0, 0.0, 0.0), 1.0, pool.add(rgb))
    if np.isscalar(rgb):                    # <spectrum value="c"/>: the `uniform` plugin (spectra/uniform.cpp:16-27)
        return abi.SpectrumDesc((C.c_float * 3)(0.0, 0.0, float("inf")), float(np.float32(rgb)))
    rgb = np.asarray(rgb, np.float32)
    if rgb.max() <= 1.0:
        return abi.SpectrumDesc((C.c_float * 3)(*fetch(tuple(float(x) for x in rgb))), 1.0)
    scale = np.float32(rgb.max() * np.float32(2.0))
    return abi.SpectrumDesc((C.c_float * 3)(*fetch(tuple(float(x) for x in rgb / scale))), float(scale))


def _texture_desc(tex, fetch, texels=None):
    """textures/checkerboard.cpp:11-15: m_transform = the top-left 3x3 of the to_uv 4x4 (transform.h:142-148).  A bitmap
    (msk_gpu.h, msk_texture_desc): its texels' coefficients are appended to `texels`, the scene's pool (a list of float32 [n, 3]
    arrays) — components clamped to [0, 1], fetched once per distinct colour."""
    t = abi.TextureDesc()
    if tex["type"] == "bitmap":
        px = np.asarray(tex["pixels"], np.float32)
        if px.ndim != 3 or px.shape[2] != 3 or px.shape[0] < 1 or px.shape[1] < 1:
            raise ValueError("bitmap pixels must be float32 [H, W, 3]")
        filt = tex.get("filter", "bilinear")
        if filt not in ("bilinear", "nearest"):
            raise ValueError("bitmap filter %r (bilinear or nearest)" % (filt,))
        t.type = abi.MSK_TEXTURE_BITMAP if filt == "bilinear" else abi.MSK_TEXTURE_BITMAP_NEAREST
        t.height, t.width, t.first_texel = px.shape[0], px.shape[1], sum(len(c) for c in texels)
        flat = np.where(px >= 0, np.minimum(px, np.float32(1)), np.float32(0)).astype(np.float32).reshape(-1, 3) + np.float32(0)   # (NaN -> 0, -0 -> +0)
        colours, inverse = np.unique(flat, axis=0, return_inverse=True)
        coeffs = np.array([fetch(tuple(float(x) for x in rgb)) for rgb in colours], np.float32).reshape(-1, 3)
        texels.append(coeffs[inverse.reshape(-1)])
    elif tex["type"] == "checkerboard":
        t.type = abi.MSK_TEXTURE_CHECKERBOARD
        t.color0[:] = fetch(tuple(tex["color0"]))
        t.color1[:] = fetch(tuple(tex["color1"]))
    else:
        raise ValueError(tex["type"])
    if "scale" in tex:
        m4 = np.diag([tex["scale"][0], tex["scale"][1], 1.0, 1.0]).astype(np.float32)
    elif "matrix" in tex:
        m4 = np.asarray(tex["matrix"], np.float32).reshape(4, 4)
    else:
        m4 = np.eye(4, dtype=np.float32)
    t.to_uv[:] = [float(x) for x in (m4[0, 0], m4[0, 1], m4[0, 2], m4[1, 0], m4[1, 1], m4[1, 2])]
    return t


def _bsdf_desc(m, fetch, index, textures=None, pool=None, texels=None):
    b = abi.BsdfDesc()
    b.back_bsdf = -1
    one = abi.SpectrumDesc((C.c_float * 3)(0.0, 0.0, float("inf")), 1.0)
    b.eta, b.k, b.specular_reflectance, b.specular_transmittance = one, one, one, one
    b.ior_eta = b.ior_inv_eta = 1.0
    b.reflectance_scale = 1.0
    spec = m.bsdf or {"type": "diffuse"}
    if spec["type"] == "diffuse":
        b.type = abi.MSK_BSDF_DIFFUSE
        if isinstance(m.reflectance, Regular):
            b.reflectance_regular = pool.add(m.reflectance)
        elif np.isscalar(m.reflectance):        # <spectrum name="reflectance" value="c"/>: the `uniform` plugin (spectra/uniform.cpp)
            b.reflectance[:] = (0.0, 0.0, float("inf"))
            b.reflectance_scale = float(m.reflectance)
        else:
            b.reflectance[:] = fetch(tuple(m.reflectance))
            b.reflectance_scale = 1.0
        if spec.get("texture") is not None:
            textures.append(_texture_desc(spec["texture"], fetch, texels))
            b.reflectance_texture = len(textures)
    elif spec["type"] == "roughconductor":
        b.type = abi.MSK_BSDF_ROUGHCONDUCTOR
        a = spec.get("alpha", 0.1)
        b.alpha_u, b.alpha_v = (a, a) if np.isscalar(a) else a
        b.sample_visible = int(bool(spec.get("sample_visible", False)))
        b.eta, b.k = spectrum_desc(spec["eta"], fetch, pool), spectrum_desc(spec["k"], fetch, pool)
        b.specular_reflectance = spectrum_desc(spec.get("specular_reflectance", (1.0, 1.0, 1.0)), fetch, pool)
    elif spec["type"] == "roughdielectric":
        # bsdfs/roughdielectric.cpp:14-24: m_eta = int_ior / ext_ior in fp32
        b.type = abi.MSK_BSDF_ROUGHDIELECTRIC
        a = spec.get("alpha", 0.1)
        b.alpha_u, b.alpha_v = (a, a) if np.isscalar(a) else a
        b.sample_visible = int(bool(spec.get("sample_visible", False)))
        int_ior, ext_ior = np.float32(spec.get("int_ior", 1.5046)), np.float32(spec.get("ext_ior", 1.00028))
        b.ior_eta, b.ior_inv_eta = float(int_ior / ext_ior), float(ext_ior / int_ior)
        b.specular_reflectance = spectrum_desc(spec.get("specular_reflectance", (1.0, 1.0, 1.0)), fetch, pool)
        b.specular_transmittance = spectrum_desc(spec.get("specular_transmittance", (1.0, 1.0, 1.0)), fetch, pool)
    elif spec["type"] == "conductor":
        # the smooth conductor (msk_gpu.h, MSK_BSDF_CONDUCTOR): defaults eta = 0, k = 1, specular_reflectance = 1 as `uniform` spectra
        b.type = abi.MSK_BSDF_CONDUCTOR
        for key, default in (("eta", 0.0), ("k", 1.0), ("specular_reflectance", 1.0)):
            v = spec.get(key, default)
            if isinstance(v, dict):
                raise ValueError('conductor: "%s" must be a constant spectrum or an rgb (a texture that varies over the surface is not supported)' % key)
            setattr(b, key, spectrum_desc(v, fetch, pool))
    elif spec["type"] in ("plastic", "roughplastic"):
        # msk_gpu.h, MSK_BSDF_PLASTIC: the base's reflectance where the diffuse BSDF keeps its own; defaults 0.5 and 1 as `uniform` spectra
        # MSK_BSDF_ROUGHPLASTIC: the same and one alpha; the checks in the order of the C++ plugin's constructor
        rough = spec["type"] == "roughplastic"
        b.type = abi.MSK_BSDF_ROUGHPLASTIC if rough else abi.MSK_BSDF_PLASTIC
        sr = spec.get("specular_reflectance", 1.0)
        if isinstance(sr, dict):
            raise ValueError(ROUGHPLASTIC_SPECULAR if rough else PLASTIC_SPECULAR)
        if rough:
            distr = spec.get("distribution", "ggx")
            if distr != "ggx":
                raise ValueError(ROUGHPLASTIC_BECKMANN if distr == "beckmann" else ROUGHPLASTIC_DISTRIBUTION % distr)
            if spec.get("sample_visible", False):
                raise ValueError(ROUGHPLASTIC_VISIBLE)
            a = spec.get("alpha", 0.1)
            au, av = (a, a) if np.isscalar(a) else a
            if np.float32(au) != np.float32(av):
                raise ValueError(ROUGHPLASTIC_ANISOTROPIC)
            b.alpha_u = b.alpha_v = float(np.float32(au))
        d = spec.get("diffuse_reflectance", 0.5)
        if isinstance(d, dict):
            b.reflectance[:] = (0.0, 0.0, float("inf"))
            b.reflectance_scale = 0.5
            textures.append(_texture_desc(d, fetch, texels))
            b.reflectance_texture = len(textures)
        elif isinstance(d, Regular):
            b.reflectance_regular = pool.add(d)
        elif np.isscalar(d):
            b.reflectance[:] = (0.0, 0.0, float("inf"))
            b.reflectance_scale = float(np.float32(d))
        else:
            b.reflectance[:] = fetch(tuple(d))
        b.specular_reflectance = spectrum_desc(sr, fetch, pool)
        int_ior, ext_ior = np.float32(spec.get("int_ior", 1.49)), np.float32(spec.get("ext_ior", 1.00028))
        b.ior_eta, b.ior_inv_eta = float(int_ior / ext_ior), float(ext_ior / int_ior)
        b.sample_visible = int(bool(spec.get("nonlinear", False)))
    elif spec["type"] == "dielectric":
        # bsdfs/dielectric.cpp:14-20: m_eta = int_ior / ext_ior in fp32, defaults 1.49 / 1.00028; no microfacet parameters
        if spec.get("twosided"):
            raise ValueError("Only materials without a transmission component can be nested!")      # twosided.cpp:33-35
        b.type = abi.MSK_BSDF_DIELECTRIC
        int_ior, ext_ior = np.float32(spec.get("int_ior", 1.49)), np.float32(spec.get("ext_ior", 1.00028))
        b.ior_eta, b.ior_inv_eta = float(int_ior / ext_ior), float(ext_ior / int_ior)
        b.specular_reflectance = spectrum_desc(spec.get("specular_reflectance", (1.0, 1.0, 1.0)), fetch, pool)
        b.specular_transmittance = spectrum_desc(spec.get("specular_transmittance", (1.0, 1.0, 1.0)), fetch, pool)
    else:
        raise ValueError(spec["type"])
    if spec.get("twosided"):
        b.back_bsdf = index            # twosided(A): the same BSDF on both sides (twosided.cpp:23-24)
    return b


# ----------------------------------------------------------------------------- flatten
class FlatScene:
    """Owns the numpy arrays an msk_scene_desc points into."""

    def __init__(self):
        self.desc = abi.SceneDesc()
        self.keep = []
        self.envmap = None            # abi.EnvmapDesc of the scene's `envmap` emitter, if it has one
        self.points = None            # (abi.PointDesc * n) of the scene's `point` emitters, if it has any (abi.Scene: msk_scene_ext)
        self.masks = None             # (abi.MaskDesc * n) of the scene's `mask` BSDFs, if it has any (abi.Scene: msk_scene_masks)
        self.lens = None              # abi.LensDesc of the scene's `thinlens` sensor, if that is its sensor (abi.Scene: msk_scene_lens)
        self.lights = None            # (abi.LightDesc * n) of the scene's `spot` / `directional` emitters, if it has any (msk_scene_lights)


def _radiance_desc(radiance, fetch, scale_in=1.0):
    """srgb_d65 (spectra/srgb_d65.cpp:13-31): scale = 2*max(rgb); color /= scale; d65 scale *= scale;
    d65.cpp:33-34: m_scale *= 1/10568.  radiance None = Texture::D65(scale_in) (constant.cpp:16)."""
    if radiance is None:
        return (0.0, 0.0, float("inf")), float(np.float32(scale_in) * (np.float32(1.0) / np.float32(10568.0)))
    rad = np.asarray(radiance, np.float32)
    scale = np.float32(rad.max() * np.float32(2.0))
    col = rad / scale if scale != 0 else rad
    ce = fetch(tuple(float(x) for x in col))
    return ce, float(np.float32(np.float32(scale_in) * scale) * (np.float32(1.0) / np.float32(10568.0)))


def _point_intensity(pt):
    """The intensity of a point spec with its "scale" folded in (float32): an rgb triple, a scalar c (= D65 * c, what
    <spectrum value="c"/> is inside an emitter) or a Regular (scale must then be 1)."""
    inten, scale = pt.get("intensity", 1.0), np.float32(pt.get("scale", 1.0))
    if isinstance(inten, Regular):
        if scale != 1:
            raise ValueError("point: a tabulated intensity takes no scale")
        return inten
    if np.isscalar(inten):
        return float(np.float32(inten) * scale)
    return tuple(float(x) for x in np.asarray(inten, np.float32) * scale)


def _point_position(pt):
    """emitters/point.cpp: `position`, or the translation of `to_world` (4x4, applied to the origin in fp32); not both"""
    if "position" in pt and "to_world" in pt:
        raise ValueError('point: only one of the parameters "position" and "to_world" can be specified at the same time!')
    if "position" in pt:
        return tuple(float(np.float32(x)) for x in pt["position"])
    m = np.asarray(pt.get("to_world", np.eye(4)), np.float32).reshape(4, 4)
    # Transform4f::apply_point on (0, 0, 0): the last column divided by w
    w = m[3, 3]
    col = m[:3, 3]
    return tuple(float(x) for x in (col if w == 1 else (col / w).astype(np.float32)))


def _light_spectrum(lt):
    """A light spec's spectrum with its "scale" folded in, as _point_intensity: a spot's "intensity", a sun's "irradiance"."""
    key = "intensity" if lt["type"] == "spot" else "irradiance"
    return _point_intensity({"intensity": lt.get(key, 1.0), "scale": lt.get("scale", 1.0)})


def _light_to_world(lt):
    """A light spec's to_world as float32 [4, 4]: "to_world" (4x4) or "lookat" ({"origin", "target", "up"}); neither = identity"""
    if "lookat" in lt:
        la = lt["lookat"]
        return _T4.lookat(la["origin"], la["target"], la.get("up", (0, 1, 0))).to_float16().reshape(4, 4)
    return np.asarray(lt.get("to_world", np.eye(4)), np.float32).reshape(4, 4)


def _unit3(v, what):
    """v / sqrt(x x + (y y + z z)) in fp32, as the C++ host does; a zero vector is refused"""
    f = np.float32
    x, y, z = (f(c) for c in v)
    l = f(np.sqrt(f(f(x * x) + f(f(y * y) + f(z * z)))))
    if not l > 0:
        raise ValueError("%s: the direction must not be the zero vector" % what)
    return tuple(float(f(c / l)) for c in (x, y, z))


def _light_axis(m, what):
    """to_world applied to the vector (0, 0, 1) in fp32 (Transform4f::apply_vector), then normalised"""
    f = np.float32
    return _unit3([f(m[r, 0] * f(0)) + f(f(m[r, 1] * f(0)) + f(m[r, 2] * f(1))) for r in range(3)], what)


def _light_geometry(lt):
    """A {"type": "spot" | "directional", ...} spec -> (position, direction, cos_cutoff, cos_beam), what abi.LightDesc holds (the C++
    plugins' arithmetic, host/src/render.cpp: SpotLight, DirectionalLight).  The cosines: math.cos of the angle in double (libm, as
    the C++ side), rounded to float."""
    f = np.float32
    kind = lt.get("type")
    if kind == "spot":
        cutoff = float(f(lt.get("cutoff_angle", 20.0)))
        if not (cutoff > 0 and cutoff <= 180):
            raise ValueError("spot: cutoff_angle must be in (0, 180] degrees")
        beam = float(f(lt["beam_width"])) if "beam_width" in lt else float(f(f(cutoff) * f(0.75)))
        if not (beam > 0 and beam <= cutoff):
            raise ValueError("spot: beam_width must be in (0, cutoff_angle] degrees")
        m = _light_to_world(lt)
        r = [f(f(f(m[i, 0] * f(0)) + f(m[i, 1] * f(0))) + f(m[i, 2] * f(0))) + f(m[i, 3] * f(1)) for i in range(4)]   # Transform4f::apply_point on the origin
        pos = tuple(float(f(r[i] / r[3])) for i in range(3))
        cc, cb = float(f(math.cos(cutoff * (math.pi / 180.0)))), float(f(math.cos(beam * (math.pi / 180.0))))
        return pos, _light_axis(m, "spot"), cc, cb
    if kind == "directional":
        if ("direction" in lt) == ("to_world" in lt or "lookat" in lt):
            raise ValueError('directional: exactly one of the parameters "direction" and "to_world" must be specified!')
        d = _unit3(lt["direction"], "directional") if "direction" in lt else _light_axis(_light_to_world(lt), "directional")
        return (0.0, 0.0, 0.0), d, 0.0, 0.0
    raise ValueError("lights: type %r is neither \"spot\" nor \"directional\"" % (kind,))


def lens_desc(camera):
    """The abi.LensDesc of a camera spec, or None for a pinhole: a camera with "aperture_radius" is the `thinlens` sensor
    (host/src/render.cpp: ThinLensCamera), whose "focus_distance" defaults to the far clip distance, as ProjectiveCamera's does.  A
    "focus_distance" without an "aperture_radius" is refused: the plugin needs the radius."""
    if "aperture_radius" not in camera:
        if "focus_distance" in camera:
            raise ValueError('thinlens: the parameter "aperture_radius" must be specified!')
        return None
    return abi.LensDesc(float(np.float32(camera["aperture_radius"])), float(np.float32(camera.get("focus_distance", camera["far"]))))


def _env_to_world4(env):
    """env["to_world"] (3x3 or 4x4, a rotation) -> float32 [4, 4]"""
    m = np.asarray(env.get("to_world", np.eye(3)), np.float32)
    if m.shape == (3, 3):
        m4 = np.eye(4, dtype=np.float32)
        m4[:3, :3] = m
        m = m4
    if m.shape != (4, 4):
        raise ValueError("envmap to_world must be 3x3 or 4x4")
    # a rotation and nothing else (csrc/msk_envmap.h, is_rotation: R R^T within 1e-4 of 1 per entry, in double, and det > 0), with no
    # translation or projective row beside it: refused here as at scene creation
    r = m[:3, :3].astype(np.float64)
    ok = bool(np.all(np.abs(r @ r.T - np.eye(3)) <= 1e-4)) and float(np.linalg.det(r)) > 0
    if not ok or np.any(m[:3, 3] != 0) or np.any(m[3] != (0, 0, 0, 1)):
        raise ValueError("envmap: to_world must be a rotation")
    return m


def envmap_desc(env, fetch):
    """{"type": "envmap", "pixels": float32 [H, W, 3] linear RGB (row 0 = the top row = theta 0), "scale": 1.0, "to_world": rotation}
    -> (abi.EnvmapDesc, [arrays to keep alive]): the texels {c0, c1, c2, w} and the sampling weights, by the arithmetic of the C++
    plugin (host/src/render.cpp, EnvironmentMapEmitter): w = 2 max(rgb), coefficients fetch(rgb / w) once per distinct colour,
    negative components and NaNs 0, a black texel all zeros; weight = (luminance of the 3x3 neighbourhood, u wrapped, v clamped,
    summed in double, rows outer) * sin(pi (j + .5) / H), rounded to float."""
    px = np.asarray(env["pixels"], np.float32)
    if px.ndim != 3 or px.shape[2] != 3 or px.shape[0] < 1 or px.shape[1] < 1:
        raise ValueError("envmap pixels must be float32 [H, W, 3]")
    H, W = px.shape[:2]
    px = np.where(px >= 0, px, np.float32(0)).astype(np.float32)
    flat = px.reshape(-1, 3)
    colours, inverse = np.unique(flat, axis=0, return_inverse=True)
    tex = np.zeros((len(colours), 4), np.float32)
    for k, rgb in enumerate(colours):
        w = np.float32(rgb.max() * np.float32(2.0))
        if w != 0:
            tex[k, :3] = fetch(tuple(float(x) for x in (rgb / w)))
            tex[k, 3] = w
    texels = np.ascontiguousarray(tex[inverse.reshape(-1)], np.float32)
    p64 = px.astype(np.float64)
    lum = (0.212671 * p64[..., 0] + 0.715160 * p64[..., 1]) + 0.072169 * p64[..., 2]
    acc = np.zeros((H, W), np.float64)
    rows, cols = np.arange(H), np.arange(W)
    for dj in (-1, 0, 1):
        rj = np.clip(rows + dj, 0, H - 1)
        for di in (-1, 0, 1):
            acc = acc + lum[rj][:, (cols + di + W) % W]
    sin_theta = np.array([math.sin(math.pi * (j + 0.5) / H) for j in range(H)], np.float64)
    weights = np.ascontiguousarray((acc * sin_theta[:, None]).astype(np.float32).reshape(-1))
    e = abi.EnvmapDesc()
    e.width, e.height = W, H
    e.texels = texels.ctypes.data_as(C.POINTER(C.c_float))
    e.weights = weights.ctypes.data_as(C.POINTER(C.c_float))
    e.to_world[:] = [float(x) for x in _env_to_world4(env)[:3, :3].reshape(-1)]
    return e, [texels, weights]


def flatten(meshes, width, height, camera=None, filter_stddev=0.5, coeff_lookup=None, env=None, crop=None, extra_textures=(), points=(), lights=()):
    """Scene -> msk_scene_desc, the step the `"path"` plugin's render() performs before calling
    the C ABI.  coeff_lookup(rgb)->(c0,c1,c2) overrides the spectral upsampling
    (tests pass the reference's own rgb2spec_fetch results); default = this package's rgb2spec.
    env: None, or {"radiance": rgb | None (= D65), "scale": 1.0, "first": False} = a top-level
    <emitter type="constant"> placed after (or, with first=True, before) the shapes in the XML; or
    {"type": "envmap", "pixels": float32 [H, W, 3], "scale": 1.0, "to_world": rotation, "first": False} = an <emitter type="envmap">
    (envmap_desc above; the result's .envmap is its abi.EnvmapDesc).
    crop: None, or (offset_x, offset_y, width, height) = the film's crop_offset_x/_y, crop_width/_height (film.cpp:12-21).
    points: [{"position": (x, y, z) | "to_world": 4x4, "intensity": rgb | c | Regular, "scale": 1.0, "first": False}] = top-level
    <emitter type="point"> elements, placed like env: those with first=True before the shapes (behind a first env), the others after
    them (behind env), each group in list order; the result's .points is their abi.PointDesc array.
    lights: [{"type": "spot", "intensity": rgb | c | Regular, "scale": 1.0, "cutoff_angle": 20, "beam_width": 3/4 of the cutoff (degrees),
    "to_world": 4x4 | "lookat": {"origin", "target", "up"}, "first": False} | {"type": "directional", "irradiance": ..., "scale": 1.0,
    "direction": (x, y, z) | "to_world" | "lookat", "first": False}] = top-level <emitter type="spot" / "directional"> elements, placed
    like points and behind them in either group; the result's .lights is their abi.LightDesc array.
    camera: {"fov", "near", "far", "origin", "target", "up"} and, for a `thinlens` sensor, "aperture_radius" (then required) and
    "focus_distance" (default: "far"); the result's .lens is then its abi.LensDesc.
    extra_textures: texture specs (as MeshSpec.bsdf["texture"]) appended to the scene's textures after those the BSDFs name:
    no surface shows them, Scene.eval_texture evaluates them."""
    from . import rgb2spec
    fetch = coeff_lookup or rgb2spec.srgb_model_fetch
    camera = camera or CBOX_CAMERA
    fs = FlatScene()
    all_v, all_f, md, bd, ed, td = [], [], [], [], [], []
    texels = []                # the bitmap textures' texel pool: float32 [n, 3] arrays of coefficients, in order
    pool = _RegularPool()
    nv = nf = 0

    def emitter_desc(kind, mesh_id, radiance, scale_in=1.0):
        if isinstance(radiance, Regular):        # a `regular` radiance as it stands (no D65 factor, no sigmoid)
            return abi.EmitterDesc(kind, mesh_id, (C.c_float * 3)(0.0, 0.0, 0.0), 0.0, pool.add(radiance))
        ce, sc = _radiance_desc(radiance, fetch, scale_in)
        return abi.EmitterDesc(kind, mesh_id, (C.c_float * 3)(*ce), float(sc), 0)

    def env_desc():
        if env.get("type") == "envmap":           # the image itself: fs.envmap (abi.Scene hands it to msk_gpu_scene_create_env)
            fs.envmap, keep = envmap_desc(env, fetch)
            fs.keep += keep
            fs.env_texels, fs.env_weights = keep
            return abi.EmitterDesc(abi.MSK_EMITTER_ENVMAP, -1, (C.c_float * 3)(0.0, 0.0, float("inf")), _radiance_desc(None, fetch, env.get("scale", 1.0))[1], 0)
        return emitter_desc(abi.MSK_EMITTER_CONSTANT, -1, env.get("radiance"), env.get("scale", 1.0))
    pd, kd = [], []

    def point_desc(pt):
        pos = _point_position(pt)
        inten = _point_intensity(pt)
        pd.append(abi.PointDesc(len(ed), (C.c_float * 3)(*pos)))
        if np.isscalar(inten):
            return emitter_desc(abi.MSK_EMITTER_POINT, -1, None, inten)
        return emitter_desc(abi.MSK_EMITTER_POINT, -1, inten)
    ld = []

    def light_desc(lt):
        pos, direction, cc, cb = _light_geometry(lt)
        spec = _light_spectrum(lt)
        ld.append(abi.LightDesc(len(ed), (C.c_float * 3)(*pos), (C.c_float * 3)(*direction), cc, cb))
        kind = abi.MSK_EMITTER_SPOT if lt["type"] == "spot" else abi.MSK_EMITTER_DIRECTIONAL
        if np.isscalar(spec):
            return emitter_desc(kind, -1, None, spec)
        return emitter_desc(kind, -1, spec)
    if env is not None and env.get("first"):
        ed.append(env_desc())
    for pt in points:
        if pt.get("first"):
            ed.append(point_desc(pt))
    for lt in lights:
        if lt.get("first"):
            ed.append(light_desc(lt))
    for i, m in enumerate(meshes):
        v, f = triangulate(m)
        if m.bsdf is not None and m.bsdf.get("type") == "mask":      # a mask decorates the entry of its nested BSDF
            inner_mesh = copy.copy(m)
            inner_mesh.bsdf = _mask_nested(m.bsdf)
            kd.append(_mask_desc(m.bsdf, len(bd), fs.keep))
            m = inner_mesh
        bd.append(_bsdf_desc(m, fetch, len(bd), td, pool, texels))
        eid = -1
        if m.radiance is not None:
            ed.append(emitter_desc(abi.MSK_EMITTER_AREA, i, m.radiance))
            eid = len(ed) - 1
        md.append(abi.MeshDesc(nv, len(v), nf, len(f), i, eid, 0, 1 if m.texcoords is not None else 0))
        all_v.append(v)
        all_f.append(f)
        nv += len(v)
        nf += len(f)
    if env is not None and not env.get("first"):
        ed.append(env_desc())
    for pt in points:
        if not pt.get("first"):
            ed.append(point_desc(pt))
    for lt in lights:
        if not lt.get("first"):
            ed.append(light_desc(lt))
    if ld:
        fs.lights = (abi.LightDesc * len(ld))(*ld)
    if pd:
        fs.points = (abi.PointDesc * len(pd))(*pd)
    if kd:
        fs.masks = (abi.MaskDesc * len(kd))(*kd)
    for tex in extra_textures:
        td.append(_texture_desc(tex, fetch, texels))
    verts = np.ascontiguousarray(np.concatenate(all_v + [np.zeros((0, 8), np.float32)]), np.float32).reshape(-1, 8)
    faces = np.ascontiguousarray(np.concatenate(all_f + [np.zeros((0, 3), np.uint32)]), np.uint32).reshape(-1, 3)
    cie, d65 = cie_tables()
    meshes_a = (abi.MeshDesc * max(1, len(md)))(*md)
    bsdfs_a = (abi.BsdfDesc * max(1, len(bd)))(*bd)
    emit_a = (abi.EmitterDesc * max(1, len(ed)))(*ed)
    tex_a = (abi.TextureDesc * max(1, len(td)))(*td)
    reg_a = (abi.RegularSpectrumDesc * max(1, len(pool.descs)))(*pool.descs)
    reg_v = np.ascontiguousarray(np.array(pool.values + ([] if pool.values else [0.0]), np.float32))
    tex_v = np.ascontiguousarray(np.concatenate(texels + [np.zeros((0 if texels else 1, 3), np.float32)]), np.float32).reshape(-1, 3)
    fs.keep += [verts, faces, cie, d65, meshes_a, bsdfs_a, emit_a, tex_a, reg_a, reg_v, tex_v]
    d = fs.desc
    d.abi_version = abi.MSK_ABI_VERSION
    d.n_meshes, d.n_bsdfs, d.n_emitters = len(md), len(bd), len(ed)
    d.meshes, d.bsdfs, d.emitters = meshes_a, bsdfs_a, emit_a
    d.n_textures, d.textures = len(td), tex_a
    d.n_regular_spectra, d.n_regular_values = len(pool.descs), len(pool.values)
    d.regular_spectra = reg_a
    d.regular_values = reg_v.ctypes.data_as(C.POINTER(C.c_float))
    d.n_texels = len(tex_v) if texels else 0
    d.texels = tex_v.ctypes.data_as(C.POINTER(C.c_float)) if texels else None
    fs.texels = tex_v
    d.vertices = verts.ctypes.data_as(C.POINTER(C.c_float))
    d.faces = faces.ctypes.data_as(C.POINTER(C.c_uint32))
    d.n_vertices, d.n_faces = nv, nf
    s2c, tw = perspective_camera(camera["fov"], camera["near"], camera["far"], width, height,
                                 camera["origin"], camera["target"], camera["up"])
    d.camera.sample_to_camera[:] = s2c.tolist()
    d.camera.to_world[:] = tw.tolist()
    d.camera.near_clip, d.camera.far_clip = camera["near"], camera["far"]
    fs.lens = lens_desc(camera)
    radius, lut = gaussian_filter(filter_stddev)
    d.film.width, d.film.height, d.film.filter_radius = width, height, radius
    d.film.filter_lut[:] = lut.tolist()
    if crop is not None:
        d.film.crop_offset[:] = [int(crop[0]), int(crop[1])]
        d.film.crop_size[:] = [int(crop[2]), int(crop[3])]
    d.cie1931_xyz = cie.ctypes.data_as(C.POINTER(C.c_float))
    d.d65 = d65.ctypes.data_as(C.POINTER(C.c_float))
    fs.vertices, fs.faces = verts, faces
    return fs


def cbox_scene(width, height, coeff_lookup=None, extra_meshes=(), crop=None):
    return flatten(cbox_meshes() + list(extra_meshes), width, height, coeff_lookup=coeff_lookup, crop=crop)


# BASELINE configs 3 and 5 name assets/bunny and assets/teapot-full, whose meshes the reference does not ship
# (SURVEY F3): the stand-ins are closed bumpy meshes of the same triangle class inside the Cornell room.
def bunny_class_scene(size, res=187, crop=None):
    """Config-3 class: ~70 k-triangle rough-conductor mesh (two-sided), room + luminaire, no boxes."""
    blob = blob_mesh("bunny_class", (278, 200, 280), 160, res, res, WHITE, seed=7, bump=0.25)
    blob.bsdf = {"type": "roughconductor", "alpha": 0.15, "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14), "twosided": True}
    return flatten(cbox_meshes()[:6] + [blob], size, size, crop=crop)


def teapot_class_scene(size, res=270, diffuse=False, crop=None):
    """Config-5 class: ~146 k-triangle rough-dielectric mesh, room + luminaire, no boxes (diffuse=True: the same geometry,
    white diffuse — measurements of the shading variants on one scene)."""
    blob = blob_mesh("teapot_class", (278, 200, 280), 160, res, res, WHITE, seed=7, bump=0.25)
    if not diffuse:
        blob.bsdf = {"type": "roughdielectric", "alpha": 0.1, "int_ior": 1.5, "ext_ior": 1.0}
    return flatten(cbox_meshes()[:6] + [blob], size, size, crop=crop)


# ----------------------------------------------------------------------------- develop
_XYZ_TO_SRGB = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556],
                         [0.055648, -0.204043, 1.057311]], np.float32)


def develop(film_xyzaw):
    """HDRFilm::image() (hdrfilm.cpp:48-90): rgb = xyz_to_srgb(XYZ) / W, alpha = A / W -> float32[H,W,4]."""
    f = np.asarray(film_xyzaw, np.float32)
    xyz = f[..., :3]
    # Eigen 3x3 * vec3 row reduction, a0 + (a1 + a2)
    rgb = np.stack([_XYZ_TO_SRGB[r, 0] * xyz[..., 0] + (_XYZ_TO_SRGB[r, 1] * xyz[..., 1] +
                                                        _XYZ_TO_SRGB[r, 2] * xyz[..., 2]) for r in range(3)], -1)
    w = f[..., 4]
    inv = np.where(w != 0, np.float32(1.0) / np.where(w != 0, w, 1), np.float32(0)).astype(np.float32)
    return np.concatenate([rgb * inv[..., None], (f[..., 3] * inv)[..., None]], -1).astype(np.float32)
