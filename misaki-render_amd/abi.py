"""ctypes mirror of include/msk_gpu.h (the C ABI of the MI355X back end).

This is the Python-side binding a maintainer would use from a scripting host;
the structs below must stay field-for-field identical to the header.  The
library is loaded from misaki-render_amd/lib/libmsk_gpu.so and there is NO
fallback: if the HIP extension is missing, loading raises.
"""
import ctypes as C
import operator
import os

import numpy as np

MSK_ABI_VERSION = 8
MSK_REGULAR_MAX = 95
MSK_OK = 0
MSK_ERR_INVALID_ARG, MSK_ERR_NO_DEVICE, MSK_ERR_HIP, MSK_ERR_OOM, MSK_ERR_UNSUPPORTED = -1, -2, -3, -4, -5
MSK_BSDF_DIFFUSE, MSK_BSDF_ROUGHCONDUCTOR, MSK_BSDF_ROUGHDIELECTRIC = 0, 1, 2
MSK_BSDF_DIELECTRIC = 3       # "dielectric" (bsdfs/dielectric.cpp): smooth interface, two delta lobes
MSK_BSDF_CONDUCTOR = 4        # "conductor": smooth metal, one delta reflection lobe
MSK_BSDF_PLASTIC = 6          # "plastic": a delta dielectric coat over a diffuse base (type 5 is unassigned)
MSK_BSDF_ROUGHPLASTIC = 7     # "roughplastic": the plastic with a GGX coat in the delta one's place
MSK_EMITTER_AREA, MSK_EMITTER_CONSTANT = 0, 1
MSK_EMITTER_ENVMAP = 2        # "envmap": a lat-long radiance image, importance-sampled (EnvmapDesc, msk_gpu_scene_create_env)
MSK_EMITTER_POINT = 3         # "point": an isotropic delta light (PointDesc + SceneExt, msk_gpu_scene_create_ext)
MSK_EMITTER_SPOT = 4          # "spot": a point light times a cone factor (LightDesc + SceneLights, msk_gpu_scene_create_lights)
MSK_EMITTER_DIRECTIONAL = 5   # "directional": a sun (LightDesc, likewise)
MSK_TEXTURE_CHECKERBOARD = 1
MSK_TEXTURE_BITMAP, MSK_TEXTURE_BITMAP_NEAREST = 2, 3       # "bitmap": bilinear / nearest (ABI v8)
MSK_EMITTER_AREA = 0
MSK_RNG_PCG_BLOCK, MSK_RNG_COUNTER = 0, 1
MSK_CIE_SAMPLES = 95
MSK_FILTER_RESOLUTION = 32


class MeshDesc(C.Structure):
    _fields_ = [("first_vertex", C.c_uint32), ("vertex_count", C.c_uint32),
                ("first_face", C.c_uint32), ("face_count", C.c_uint32),
                ("bsdf_id", C.c_int32), ("emitter_id", C.c_int32),
                ("has_normals", C.c_uint32), ("has_texcoords", C.c_uint32)]


class RegularSpectrumDesc(C.Structure):
    _fields_ = [("lambda_min", C.c_float), ("lambda_max", C.c_float), ("size", C.c_uint32), ("first_value", C.c_uint32)]


class SpectrumDesc(C.Structure):
    _fields_ = [("coeff", C.c_float * 3), ("scale", C.c_float), ("regular", C.c_uint32)]


class BsdfDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("back_bsdf", C.c_int32), ("reflectance", C.c_float * 3),
                ("alpha_u", C.c_float), ("alpha_v", C.c_float), ("sample_visible", C.c_int32),
                ("eta", SpectrumDesc), ("k", SpectrumDesc), ("specular_reflectance", SpectrumDesc),
                ("specular_transmittance", SpectrumDesc), ("ior_eta", C.c_float), ("ior_inv_eta", C.c_float),
                ("reflectance_texture", C.c_uint32), ("reflectance_scale", C.c_float), ("reflectance_regular", C.c_uint32)]


class TextureDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("color0", C.c_float * 3), ("color1", C.c_float * 3), ("to_uv", C.c_float * 6),
                ("width", C.c_uint32), ("height", C.c_uint32), ("first_texel", C.c_uint32)]      # a bitmap's place in SceneDesc.texels


class EmitterDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("mesh_id", C.c_int32), ("radiance", C.c_float * 3),
                ("d65_scale", C.c_float), ("radiance_regular", C.c_uint32)]


class EnvmapDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("texels", C.POINTER(C.c_float)),      # width * height * 4: c0 c1 c2 w
                ("weights", C.POINTER(C.c_float)), ("to_world", C.c_float * 9)]                       # width * height; row-major rotation


class PointDesc(C.Structure):
    _fields_ = [("emitter", C.c_uint32), ("position", C.c_float * 3)]      # index into SceneDesc.emitters; world space


class SceneExt(C.Structure):
    _fields_ = [("envmap", C.POINTER(EnvmapDesc)), ("n_points", C.c_uint32), ("points", C.POINTER(PointDesc))]


class MaskDesc(C.Structure):
    """msk_mask_desc: the `mask` decoration of one BSDF entry.  filter 0: the constant `opacity`; 1 / 2: a nearest / bilinear image"""
    _fields_ = [("bsdf", C.c_uint32), ("opacity", C.c_float), ("filter", C.c_int32), ("to_uv", C.c_float * 6),
                ("width", C.c_uint32), ("height", C.c_uint32), ("values", C.POINTER(C.c_float))]      # width * height scalars in [0, 1]


class SceneMasks(C.Structure):
    _fields_ = [("ext", SceneExt), ("n_masks", C.c_uint32), ("masks", C.POINTER(MaskDesc))]


class LightDesc(C.Structure):
    """msk_light_desc: the geometry of a spot or directional emitter.  direction: the way the light travels, unit length"""
    _fields_ = [("emitter", C.c_uint32), ("position", C.c_float * 3), ("direction", C.c_float * 3),
                ("cos_cutoff", C.c_float), ("cos_beam", C.c_float)]


class SceneLights(C.Structure):
    _fields_ = [("masks", SceneMasks), ("n_lights", C.c_uint32), ("lights", C.POINTER(LightDesc))]


class LensDesc(C.Structure):
    """msk_lens_desc: the `thinlens` sensor's aperture radius (>= 0) and focus distance (> 0), in camera-space units"""
    _fields_ = [("aperture_radius", C.c_float), ("focus_distance", C.c_float)]


class SceneLens(C.Structure):
    _fields_ = [("lights", SceneLights), ("lens", C.POINTER(LensDesc))]


class CameraDesc(C.Structure):
    _fields_ = [("sample_to_camera", C.c_float * 16), ("to_world", C.c_float * 16),
                ("near_clip", C.c_float), ("far_clip", C.c_float)]


class FilmDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("filter_radius", C.c_float),
                ("filter_lut", C.c_float * (MSK_FILTER_RESOLUTION + 1)),
                ("crop_offset", C.c_int32 * 2), ("crop_size", C.c_int32 * 2)]     # {0, 0} size = the whole film


class SceneDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_meshes", C.c_uint32), ("n_bsdfs", C.c_uint32),
                ("n_emitters", C.c_uint32),
                ("meshes", C.POINTER(MeshDesc)), ("bsdfs", C.POINTER(BsdfDesc)),
                ("emitters", C.POINTER(EmitterDesc)),
                ("vertices", C.POINTER(C.c_float)), ("faces", C.POINTER(C.c_uint32)),
                ("n_vertices", C.c_uint32), ("n_faces", C.c_uint32),
                ("camera", CameraDesc), ("film", FilmDesc),
                ("cie1931_xyz", C.POINTER(C.c_float)), ("d65", C.POINTER(C.c_float)),
                ("n_textures", C.c_uint32), ("textures", C.POINTER(TextureDesc)),
                ("n_regular_spectra", C.c_uint32), ("n_regular_values", C.c_uint32),
                ("regular_spectra", C.POINTER(RegularSpectrumDesc)), ("regular_values", C.POINTER(C.c_float)),
                ("n_texels", C.c_uint32), ("texels", C.POINTER(C.c_float))]      # ABI v8: 3 coefficients per texel


class RenderParams(C.Structure):
    _fields_ = [("spp", C.c_uint32), ("seed", C.c_uint64), ("rng_mode", C.c_int32),
                ("rr_depth", C.c_int32), ("max_depth", C.c_int32), ("hide_emitters", C.c_int32),
                ("block_size", C.c_int32), ("block_first", C.c_uint32), ("block_stride", C.c_uint32),
                ("sample_first", C.c_uint32), ("sample_stride", C.c_uint32)]


class DirectParams(C.Structure):
    """msk_direct_params: the "direct" integrator's sample counts per camera sample (each 0 .. 4096, not both 0)."""
    _fields_ = [("light_samples", C.c_uint32), ("bsdf_samples", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("iterations", C.c_uint32), ("passes", C.c_uint32), ("ms_total", C.c_float),
                ("ms_generate", C.c_float), ("ms_trace", C.c_float), ("ms_shade", C.c_float),
                ("ms_resolve", C.c_float), ("n_trace_launches", C.c_uint32),
                ("n_shade_launches", C.c_uint32), ("launches_trace", C.c_uint32), ("launches_shade", C.c_uint32),
                ("launches_wavefront", C.c_uint32), ("invalid_samples", C.c_uint64),
                ("bytes_shade", C.c_uint64), ("bytes_trace", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def render_params(spp, seed=0, rng_mode=MSK_RNG_COUNTER, rr_depth=5, max_depth=-1, hide_emitters=0,
                  block_size=32, block_first=0, block_stride=1, sample_first=0, sample_stride=1):
    """Defaults = the reference's effective integrator settings."""
    return RenderParams(spp, seed, rng_mode, rr_depth, max_depth, hide_emitters, block_size,
                        block_first, block_stride, sample_first, sample_stride)


class MskError(RuntimeError):
    """A non-zero status from the C ABI (the plugin side turns it into the reference's Throw)."""

    def __init__(self, code, text):
        super().__init__(f"msk_gpu error {code}: {text}")
        self.code = code


_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSK_GPU_LIB") or os.path.join(_PKG_DIR, "lib", "libmsk_gpu.so")   # override: A/B experiments

# every symbol include/msk_gpu.h declares
EXPORTS = ["msk_gpu_init", "msk_gpu_shutdown", "msk_gpu_last_error", "msk_gpu_scene_create",
           "msk_gpu_scene_destroy", "msk_gpu_render", "msk_gpu_render_device", "msk_gpu_trace_closest",
           "msk_gpu_trace_any", "msk_gpu_sample_pixels", "msk_gpu_describe", "msk_gpu_render_aov", "msk_gpu_aov_channels",
           "msk_gpu_eval_texture", "msk_gpu_scene_create_env", "msk_gpu_env_eval", "msk_gpu_env_sample",
           "msk_gpu_scene_create_ext", "msk_gpu_point_sample", "msk_gpu_conductor_sample",
           "msk_gpu_scene_create_masks", "msk_gpu_mask_sample", "msk_gpu_mask_eval",
           "msk_gpu_scene_create_lights", "msk_gpu_light_sample",
           "msk_gpu_scene_create_lens", "msk_gpu_camera_sample",
           "msk_gpu_plastic_sample", "msk_gpu_plastic_eval", "msk_gpu_plastic_constants",
           "msk_gpu_roughplastic_sample", "msk_gpu_roughplastic_eval",
           "msk_gpu_render_direct", "msk_gpu_render_direct_device", "msk_gpu_sample_pixels_direct"]

# integrators/aov.cpp:21-28
MSK_AOV_DEPTH, MSK_AOV_POSITION, MSK_AOV_UV, MSK_AOV_GEO_NORMAL, MSK_AOV_SH_NORMAL, MSK_AOV_PATH_RGBA = range(6)
AOV_WIDTH = (1, 3, 2, 3, 3, 4)

_lib = None


def load_library(path=None):
    """dlopen libmsk_gpu.so and type its entry points.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: the HIP back end is not built (run `python -c 'import __graft_entry__ as g; "
            f"g.build()'`).  There is no CPU fallback.")
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    vp, u64 = C.c_void_p, C.c_uint64
    lib.msk_gpu_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    lib.msk_gpu_init.restype = C.c_int
    lib.msk_gpu_shutdown.argtypes = [vp]
    lib.msk_gpu_shutdown.restype = None
    lib.msk_gpu_last_error.argtypes = [vp]
    lib.msk_gpu_last_error.restype = C.c_char_p
    lib.msk_gpu_scene_create.argtypes = [vp, C.POINTER(SceneDesc), C.POINTER(vp)]
    lib.msk_gpu_scene_create.restype = C.c_int
    lib.msk_gpu_scene_destroy.argtypes = [vp]
    lib.msk_gpu_scene_destroy.restype = None
    lib.msk_gpu_render.argtypes = [vp, C.POINTER(RenderParams), vp, C.POINTER(Stats)]
    lib.msk_gpu_render.restype = C.c_int
    lib.msk_gpu_render_device.argtypes = [vp, C.POINTER(RenderParams), vp, vp, C.POINTER(Stats)]
    lib.msk_gpu_render_device.restype = C.c_int
    lib.msk_gpu_trace_closest.argtypes = [vp, u64, vp, vp]
    lib.msk_gpu_trace_closest.restype = C.c_int
    lib.msk_gpu_trace_any.argtypes = [vp, u64, vp, vp]
    lib.msk_gpu_trace_any.restype = C.c_int
    lib.msk_gpu_sample_pixels.argtypes = [vp, C.POINTER(RenderParams), u64, vp, vp, vp]
    lib.msk_gpu_sample_pixels.restype = C.c_int
    lib.msk_gpu_render_aov.argtypes = [vp, C.POINTER(RenderParams), vp, C.c_uint32, vp, C.POINTER(Stats)]
    lib.msk_gpu_render_aov.restype = C.c_int
    lib.msk_gpu_aov_channels.argtypes = [vp, C.c_uint32]
    lib.msk_gpu_aov_channels.restype = C.c_uint32
    lib.msk_gpu_eval_texture.argtypes = [vp, C.c_uint32, u64, vp, vp, vp]
    lib.msk_gpu_eval_texture.restype = C.c_int
    lib.msk_gpu_scene_create_env.argtypes = [vp, C.POINTER(SceneDesc), C.POINTER(EnvmapDesc), C.POINTER(vp)]
    lib.msk_gpu_scene_create_env.restype = C.c_int
    lib.msk_gpu_env_eval.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.msk_gpu_env_eval.restype = C.c_int
    lib.msk_gpu_env_sample.argtypes = [vp, u64, vp, vp, vp, vp]
    lib.msk_gpu_env_sample.restype = C.c_int
    lib.msk_gpu_scene_create_ext.argtypes = [vp, C.POINTER(SceneDesc), C.POINTER(SceneExt), C.POINTER(vp)]
    lib.msk_gpu_scene_create_ext.restype = C.c_int
    lib.msk_gpu_point_sample.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, vp]
    lib.msk_gpu_point_sample.restype = C.c_int
    lib.msk_gpu_conductor_sample.argtypes = [vp, C.c_uint32, u64, vp, vp, vp]
    lib.msk_gpu_conductor_sample.restype = C.c_int
    lib.msk_gpu_scene_create_masks.argtypes = [vp, C.POINTER(SceneDesc), C.POINTER(SceneMasks), C.POINTER(vp)]
    lib.msk_gpu_scene_create_masks.restype = C.c_int
    # (the parent build's library, loaded through MSK_GPU_LIB for an A/B (tools/delta_bench.py), has neither: a scene with lights then
    # fails on the missing symbol; build() holds the tree's own library to EXPORTS)
    if path is None and not os.environ.get("MSK_GPU_LIB") or hasattr(lib, "msk_gpu_scene_create_lights"):
        lib.msk_gpu_scene_create_lights.argtypes = [vp, C.POINTER(SceneDesc), C.POINTER(SceneLights), C.POINTER(vp)]
        lib.msk_gpu_scene_create_lights.restype = C.c_int
        lib.msk_gpu_light_sample.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, vp]
        lib.msk_gpu_light_sample.restype = C.c_int
    if path is None and not os.environ.get("MSK_GPU_LIB") or hasattr(lib, "msk_gpu_scene_create_lens"):       # (likewise: tools/lens_bench.py)
        lib.msk_gpu_scene_create_lens.argtypes = [vp, C.POINTER(SceneDesc), C.POINTER(SceneLens), C.POINTER(vp)]
        lib.msk_gpu_scene_create_lens.restype = C.c_int
        lib.msk_gpu_camera_sample.argtypes = [vp, u64, vp, vp, vp]
        lib.msk_gpu_camera_sample.restype = C.c_int
    lib.msk_gpu_mask_sample.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, vp, vp, vp, vp]
    lib.msk_gpu_mask_sample.restype = C.c_int
    lib.msk_gpu_mask_eval.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, vp, vp, vp]
    lib.msk_gpu_mask_eval.restype = C.c_int
    lib.msk_gpu_plastic_sample.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, vp, vp, vp, vp]
    lib.msk_gpu_plastic_sample.restype = C.c_int
    lib.msk_gpu_plastic_eval.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, vp, vp, vp]
    lib.msk_gpu_plastic_eval.restype = C.c_int
    lib.msk_gpu_roughplastic_sample.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, vp, vp, vp, vp]
    lib.msk_gpu_roughplastic_sample.restype = C.c_int
    lib.msk_gpu_roughplastic_eval.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, vp, vp, vp]
    lib.msk_gpu_roughplastic_eval.restype = C.c_int
    lib.msk_gpu_plastic_constants.argtypes = [vp, C.c_uint32, C.POINTER(C.c_float * 2)]
    lib.msk_gpu_plastic_constants.restype = C.c_int
    lib.msk_gpu_render_direct.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(DirectParams), vp, C.POINTER(Stats)]
    lib.msk_gpu_render_direct.restype = C.c_int
    lib.msk_gpu_render_direct_device.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(DirectParams), vp, vp, C.POINTER(Stats)]
    lib.msk_gpu_render_direct_device.restype = C.c_int
    lib.msk_gpu_sample_pixels_direct.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(DirectParams), u64, vp, vp, vp]
    lib.msk_gpu_sample_pixels_direct.restype = C.c_int
    lib.msk_gpu_describe.argtypes = [vp, C.c_char_p, u64]
    lib.msk_gpu_describe.restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """msk_ctx: one per process.  `device` is a HIP ordinal, or a sequence of ordinals for a GROUP context (msk_gpu_init with
    n > 1: renders are sample-sharded over the members and the films summed on the first device; an ordinal may repeat)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.handle = C.c_void_p()
        try:
            devs = [operator.index(device)]               # any integer type (a numpy rank value included)
        except TypeError:
            devs = [operator.index(d) for d in device]
        self.devices = devs
        ids = (C.c_int * len(devs))(*devs)
        rc = self.lib.msk_gpu_init(ids, len(devs), C.byref(self.handle))
        if rc != MSK_OK:
            raise MskError(rc, (self.lib.msk_gpu_last_error(None) or b"").decode())

    def check(self, rc):
        if rc != MSK_OK:
            raise MskError(rc, (self.lib.msk_gpu_last_error(self.handle) or b"").decode())

    def describe(self):
        buf = C.create_string_buffer(1024)
        self.check(self.lib.msk_gpu_describe(self.handle, buf, 1024))
        return buf.value.decode()

    def close(self):
        if self.handle:
            self.lib.msk_gpu_shutdown(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Scene:
    """msk_scene: geometry + BVH + light tables resident in HBM."""

    def __init__(self, ctx, flat, envmap=None, points=None, masks=None, lights=None, lens=None):
        """flat: hostmirror.FlatScene (keeps the numpy arrays the desc points into alive).  envmap: the EnvmapDesc of the scene's
        MSK_EMITTER_ENVMAP emitter; by default the one the flattener made (flat.envmap), if any.  points: the PointDesc array of
        its MSK_EMITTER_POINT emitters (a ctypes array or a list); by default flat.points.  A scene with points is created
        through msk_gpu_scene_create_ext, one with an image alone through _create_env, any other through msk_gpu_scene_create.
        masks: the MaskDesc array of its `mask` BSDFs (a ctypes array or a list); by default flat.masks.  A scene with masks is
        created through msk_gpu_scene_create_masks.  lights: the LightDesc array of its spot and directional emitters (a ctypes
        array or a list); by default flat.lights.  A scene with lights is created through msk_gpu_scene_create_lights.  lens: the LensDesc of
        its `thinlens` sensor; by default flat.lens.  A scene with a lens is created through msk_gpu_scene_create_lens."""
        self.ctx, self.flat = ctx, flat
        self.handle = C.c_void_p()
        self.envmap = envmap if envmap is not None else getattr(flat, "envmap", None)
        pts = points if points is not None else getattr(flat, "points", None)
        if pts is not None and not isinstance(pts, C.Array):
            pts = (PointDesc * max(1, len(pts)))(*pts) if len(pts) else None
        self.points = pts if (pts is not None and len(pts)) else None
        mk = masks if masks is not None else getattr(flat, "masks", None)
        if mk is not None and not isinstance(mk, C.Array):
            mk = (MaskDesc * max(1, len(mk)))(*mk) if len(mk) else None
        self.masks = mk if (mk is not None and len(mk)) else None
        lt = lights if lights is not None else getattr(flat, "lights", None)
        if lt is not None and not isinstance(lt, C.Array):
            lt = (LightDesc * max(1, len(lt)))(*lt) if len(lt) else None
        self.lights = lt if (lt is not None and len(lt)) else None
        self.lens = lens if lens is not None else getattr(flat, "lens", None)
        if self.lens is not None:
            ext = SceneExt(C.pointer(self.envmap) if self.envmap is not None else None, len(self.points) if self.points is not None else 0, self.points)
            em = SceneMasks(ext, len(self.masks) if self.masks is not None else 0, self.masks)
            el = SceneLights(em, len(self.lights) if self.lights is not None else 0, self.lights)
            self.eln = SceneLens(el, C.pointer(self.lens))
            ctx.check(ctx.lib.msk_gpu_scene_create_lens(ctx.handle, C.byref(flat.desc), C.byref(self.eln), C.byref(self.handle)))
        elif self.lights is not None:
            ext = SceneExt(C.pointer(self.envmap) if self.envmap is not None else None, len(self.points) if self.points is not None else 0, self.points)
            em = SceneMasks(ext, len(self.masks) if self.masks is not None else 0, self.masks)
            self.el = SceneLights(em, len(self.lights), self.lights)
            ctx.check(ctx.lib.msk_gpu_scene_create_lights(ctx.handle, C.byref(flat.desc), C.byref(self.el), C.byref(self.handle)))
        elif self.masks is not None:
            ext = SceneExt(C.pointer(self.envmap) if self.envmap is not None else None, len(self.points) if self.points is not None else 0, self.points)
            self.em = SceneMasks(ext, len(self.masks), self.masks)
            ctx.check(ctx.lib.msk_gpu_scene_create_masks(ctx.handle, C.byref(flat.desc), C.byref(self.em), C.byref(self.handle)))
        elif self.points is not None:
            self.ext = SceneExt(C.pointer(self.envmap) if self.envmap is not None else None, len(self.points), self.points)
            ctx.check(ctx.lib.msk_gpu_scene_create_ext(ctx.handle, C.byref(flat.desc), C.byref(self.ext), C.byref(self.handle)))
        elif self.envmap is not None:
            ctx.check(ctx.lib.msk_gpu_scene_create_env(ctx.handle, C.byref(flat.desc), C.byref(self.envmap), C.byref(self.handle)))
        else:
            ctx.check(ctx.lib.msk_gpu_scene_create(ctx.handle, C.byref(flat.desc), C.byref(self.handle)))

    @property
    def width(self):
        """of the film the render calls write: the crop window (the whole film by default)"""
        f = self.flat.desc.film
        return f.crop_size[0] if (f.crop_size[0] or f.crop_size[1]) else f.width

    @property
    def height(self):
        f = self.flat.desc.film
        return f.crop_size[1] if (f.crop_size[0] or f.crop_size[1]) else f.height

    def render(self, params, out=None):
        """-> (film float32[H,W,5] of weighted sums {X,Y,Z,A,W}, Stats).  out: an array to fill instead of a new one (a
        caller that renders repeatedly keeps its pages mapped: a fresh 5 MB array costs more in page faults than the copy)."""
        film = out if out is not None else np.empty((self.height, self.width, 5), np.float32)
        if not (isinstance(film, np.ndarray) and film.dtype == np.float32 and film.flags.c_contiguous and film.shape == (self.height, self.width, 5)):
            raise ValueError(f"out must be a C-contiguous float32 array of shape {(self.height, self.width, 5)}")      # the library writes that many bytes
        st = Stats()
        self.ctx.check(self.ctx.lib.msk_gpu_render(self.handle, C.byref(params), _ptr(film), C.byref(st)))
        return film, st

    def render_aov(self, params, aov_types):
        """The "aov" integrator: -> (film float32[H,W,5+C] of weighted sums {X,Y,Z,A,W, aov channels...}, Stats)."""
        types = np.ascontiguousarray(aov_types, np.int32)
        n_ch = self.ctx.lib.msk_gpu_aov_channels(_ptr(types), len(types)) if len(types) else 0
        film = np.empty((self.height, self.width, 5 + n_ch), np.float32)
        st = Stats()
        self.ctx.check(self.ctx.lib.msk_gpu_render_aov(self.handle, C.byref(params), _ptr(types), len(types), _ptr(film), C.byref(st)))
        return film, st

    def render_device(self, params, device_ptr, stream=None):
        st = Stats()
        self.ctx.check(self.ctx.lib.msk_gpu_render_device(self.handle, C.byref(params), C.c_void_p(device_ptr),
                                                           C.c_void_p(stream or 0), C.byref(st)))
        return st

    def trace_closest(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.empty((rays.shape[0], 4), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_trace_closest(self.handle, rays.shape[0], _ptr(rays), _ptr(out)))
        return out

    def trace_any(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.empty(rays.shape[0], np.uint8)
        self.ctx.check(self.ctx.lib.msk_gpu_trace_any(self.handle, rays.shape[0], _ptr(rays), _ptr(out)))
        return out

    def sample_pixels(self, params, pixels):
        pixels = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
        n = pixels.shape[0]
        xyz = np.empty((n, params.spp, 3), np.float32)
        pos = np.empty((n, params.spp, 2), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_sample_pixels(self.handle, C.byref(params), n, _ptr(pixels),
                                                           _ptr(xyz), _ptr(pos)))
        return xyz, pos

    def render_direct(self, params, light_samples=1, bsdf_samples=1, out=None):
        """The "direct" integrator (msk_gpu_render_direct): -> (film float32[H,W,5], Stats).  rr_depth / max_depth of params are ignored."""
        film = out if out is not None else np.empty((self.height, self.width, 5), np.float32)
        if not (isinstance(film, np.ndarray) and film.dtype == np.float32 and film.flags.c_contiguous and film.shape == (self.height, self.width, 5)):
            raise ValueError(f"out must be a C-contiguous float32 array of shape {(self.height, self.width, 5)}")
        st, dp = Stats(), DirectParams(light_samples, bsdf_samples)
        self.ctx.check(self.ctx.lib.msk_gpu_render_direct(self.handle, C.byref(params), C.byref(dp), _ptr(film), C.byref(st)))
        return film, st

    def render_direct_device(self, params, device_ptr, light_samples=1, bsdf_samples=1, stream=None):
        st, dp = Stats(), DirectParams(light_samples, bsdf_samples)
        self.ctx.check(self.ctx.lib.msk_gpu_render_direct_device(self.handle, C.byref(params), C.byref(dp), C.c_void_p(device_ptr),
                                                                  C.c_void_p(stream or 0), C.byref(st)))
        return st

    def sample_pixels_direct(self, params, pixels, light_samples=1, bsdf_samples=1):
        """msk_gpu_sample_pixels_direct: per listed pixel the samples this call OWNS (s = sample_first + k sample_stride < spp), in
        order -> (xyz float32[n, owned, 3], pos float32[n, owned, 2])."""
        pixels = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
        n = pixels.shape[0]
        stride = params.sample_stride or 1
        owned = (params.spp - params.sample_first + stride - 1) // stride if params.sample_first < params.spp else 0
        xyz = np.empty((n, owned, 3), np.float32)
        pos = np.empty((n, owned, 2), np.float32)
        dp = DirectParams(light_samples, bsdf_samples)
        self.ctx.check(self.ctx.lib.msk_gpu_sample_pixels_direct(self.handle, C.byref(params), C.byref(dp), n, _ptr(pixels),
                                                                  _ptr(xyz), _ptr(pos)))
        return xyz, pos

    def eval_texture(self, texture, uv, wavelengths):
        """The value of texture `texture` (1-based, as BsdfDesc.reflectance_texture) at uv float32[n, 2] and wavelengths
        float32[n, 4] -> float32[n, 4]: what the shading kernels evaluate at a hit with that si.uv."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        wl = np.ascontiguousarray(wavelengths, np.float32).reshape(-1, 4)
        if len(uv) != len(wl):
            raise ValueError("uv and wavelengths must name the same number of points")
        out = np.empty((len(uv), 4), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_eval_texture(self.handle, int(texture), len(uv), _ptr(uv), _ptr(wl), _ptr(out)))
        return out

    def env_eval(self, dirs, wavelengths):
        """The envmap emitter at unit directions float32[n, 3] and wavelengths float32[n, 4] -> (radiance float32[n, 4], solid-angle
        density float32[n]): what the shading kernels evaluate for a ray that leaves the scene in that direction."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        wl = np.ascontiguousarray(wavelengths, np.float32).reshape(-1, 4)
        if len(d) != len(wl):
            raise ValueError("dirs and wavelengths must name the same number of points")
        rad, pdf = np.empty((len(d), 4), np.float32), np.empty(len(d), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_env_eval(self.handle, len(d), _ptr(d), _ptr(wl), _ptr(rad), _ptr(pdf)))
        return rad, pdf

    def env_sample(self, u):
        """The light direction next-event estimation draws from the envmap emitter for the random numbers u float32[n, 2]
        -> (direction float32[n, 3], uv float32[n, 2], solid-angle density float32[n])."""
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        d, uv, pdf = np.empty((len(u), 3), np.float32), np.empty((len(u), 2), np.float32), np.empty(len(u), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_env_sample(self.handle, len(u), _ptr(u), _ptr(d), _ptr(uv), _ptr(pdf)))
        return d, uv, pdf

    def camera_sample(self, film_pos, aperture_u=None):
        """The camera ray of the film positions (n, 2), in pixels, and — for a scene with a lens — the aperture samples (n, 2):
        -> rays float32[n, 8] = {o, tnear, d, tfar}, what trace_closest reads (msk_gpu_camera_sample)."""
        p = np.ascontiguousarray(film_pos, np.float32).reshape(-1, 2)
        u = None
        if aperture_u is not None:
            u = np.ascontiguousarray(aperture_u, np.float32).reshape(-1, 2)
            if len(u) != len(p):
                raise ValueError("film_pos and aperture_u must name the same number of rays")
        rays = np.empty((len(p), 8), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_camera_sample(self.handle, len(p), _ptr(p), _ptr(u) if u is not None else None, _ptr(rays)))
        return rays

    def light_sample(self, emitter, ref_points, wavelengths):
        """The next-event sample of the spot or directional emitter `emitter` from the reference points (n, 3) at the wavelengths
        (n, 4): -> (d_dist float32[n, 4] = {d, dist}, value float32[n, 4]), as point_sample (msk_gpu_light_sample)."""
        p = np.ascontiguousarray(ref_points, np.float32).reshape(-1, 3)
        wl = np.ascontiguousarray(wavelengths, np.float32).reshape(-1, 4)
        if len(p) != len(wl):
            raise ValueError("ref_points and wavelengths must name the same number of points")
        dd = np.empty((len(p), 4), np.float32)
        val = np.empty((len(p), 4), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_light_sample(self.handle, int(emitter), len(p), _ptr(p), _ptr(wl), _ptr(dd), _ptr(val)))
        return dd, val

    def point_sample(self, emitter, ref_points, wavelengths):
        """The next-event sample of point emitter `emitter` (index into the scene's emitters) from the reference points
        float32[n, 3] at wavelengths float32[n, 4] -> ({d.x, d.y, d.z, dist} float32[n, 4], value float32[n, 4])."""
        p = np.ascontiguousarray(ref_points, np.float32).reshape(-1, 3)
        wl = np.ascontiguousarray(wavelengths, np.float32).reshape(-1, 4)
        if len(p) != len(wl):
            raise ValueError("ref_points and wavelengths must name the same number of points")
        dd, val = np.empty((len(p), 4), np.float32), np.empty((len(p), 4), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_point_sample(self.handle, int(emitter), len(p), _ptr(p), _ptr(wl), _ptr(dd), _ptr(val)))
        return dd, val

    def conductor_sample(self, bsdf, cos_theta_i, wavelengths):
        """The value of the delta lobe of conductor `bsdf` (index into the scene's bsdfs) for cos_theta_i float32[n] at
        wavelengths float32[n, 4] -> float32[n, 4], zeros for cos_theta_i <= 0."""
        c = np.ascontiguousarray(cos_theta_i, np.float32).reshape(-1)
        wl = np.ascontiguousarray(wavelengths, np.float32).reshape(-1, 4)
        if len(c) != len(wl):
            raise ValueError("cos_theta_i and wavelengths must name the same number of points")
        val = np.empty((len(c), 4), np.float32)
        self.ctx.check(self.ctx.lib.msk_gpu_conductor_sample(self.handle, int(bsdf), len(c), _ptr(c), _ptr(wl), _ptr(val)))
        return val

    def mask_sample(self, bsdf, uv, wi, sample1_u, wavelengths, _entry="msk_gpu_mask_sample"):
        """sample() of the decorated BSDF entry `bsdf` of a scene that holds a mask: uv float32[n, 2], wi float32[n, 3] (local),
        sample1_u float32[n, 3] = {sample1, u.x, u.y}, wavelengths float32[n, 4] -> ({wo, pdf} float32[n, 4], value float32[n, 4],
        {eta, delta, null lobe, ok} float32[n, 4])."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        su = np.ascontiguousarray(sample1_u, np.float32).reshape(-1, 3)
        wl = np.ascontiguousarray(wavelengths, np.float32).reshape(-1, 4)
        if not (len(uv) == len(wi) == len(su) == len(wl)):
            raise ValueError("uv, wi, sample1_u and wavelengths must name the same number of points")
        a, b, c = (np.empty((len(uv), 4), np.float32) for _ in range(3))
        self.ctx.check(getattr(self.ctx.lib, _entry)(self.handle, int(bsdf), len(uv), _ptr(uv), _ptr(wi), _ptr(su), _ptr(wl), _ptr(a), _ptr(b), _ptr(c)))
        return a, b, c

    def mask_eval(self, bsdf, uv, wi, wo, wavelengths, _entry="msk_gpu_mask_eval"):
        """The opacity, eval() and pdf() of the decorated BSDF entry `bsdf`: uv float32[n, 2], wi / wo float32[n, 3] (local),
        wavelengths float32[n, 4] -> ({a, pdf} float32[n, 2], eval float32[n, 4])."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        wi = np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        wl = np.ascontiguousarray(wavelengths, np.float32).reshape(-1, 4)
        if not (len(uv) == len(wi) == len(wo) == len(wl)):
            raise ValueError("uv, wi, wo and wavelengths must name the same number of points")
        a, v = np.empty((len(uv), 2), np.float32), np.empty((len(uv), 4), np.float32)
        self.ctx.check(getattr(self.ctx.lib, _entry)(self.handle, int(bsdf), len(uv), _ptr(uv), _ptr(wi), _ptr(wo), _ptr(wl), _ptr(a), _ptr(v)))
        return a, v

    def plastic_sample(self, bsdf, uv, wi, sample1_u, wavelengths):
        """mask_sample on a `plastic` entry, in a scene with or without a mask; the flags' second word says that the sampled lobe was
        delta (the coat, or a mask's null lobe)."""
        return self.mask_sample(bsdf, uv, wi, sample1_u, wavelengths, _entry="msk_gpu_plastic_sample")

    def plastic_eval(self, bsdf, uv, wi, wo, wavelengths):
        """mask_eval on a `plastic` entry, in a scene with or without a mask."""
        return self.mask_eval(bsdf, uv, wi, wo, wavelengths, _entry="msk_gpu_plastic_eval")

    def roughplastic_sample(self, bsdf, uv, wi, sample1_u, wavelengths):
        """mask_sample on a `roughplastic` entry, in a scene with or without a mask."""
        return self.mask_sample(bsdf, uv, wi, sample1_u, wavelengths, _entry="msk_gpu_roughplastic_sample")

    def roughplastic_eval(self, bsdf, uv, wi, wo, wavelengths):
        """mask_eval on a `roughplastic` entry, in a scene with or without a mask."""
        return self.mask_eval(bsdf, uv, wi, wo, wavelengths, _entry="msk_gpu_roughplastic_eval")

    def plastic_constants(self, bsdf):
        """(fdr_int, ssw) of the `plastic` or `roughplastic` entry `bsdf` as the packer computed them, float32."""
        out = (C.c_float * 2)()
        self.ctx.check(self.ctx.lib.msk_gpu_plastic_constants(self.handle, int(bsdf), C.byref(out)))
        return np.float32(out[0]), np.float32(out[1])

    def close(self):
        if self.handle:
            self.ctx.lib.msk_gpu_scene_destroy(self.handle)
            self.handle = C.c_void_p()
