"""The `spot` and `directional` emitters (include/msk_gpu.h at msk_light_desc): the two other delta lights.

CPU: the restatement checks itself (light_ref.py); the packer as a stand-alone native program, plain and sanitized; the two
flatteners; layout and exports; the launch plan; the float64 expectations' own convergence, each spot case with its crop wholly in
one zone of the cone.  GPU: the probe equals the fp32 restatement bit for bit; a spot that covers the sphere is the point light to
the bit; rendered radiance meets float64 closed forms under "path" and under "direct"; direct (1, 1) is path at max_depth = 2;
every execution variant makes the same film; a mask over a spot; a group context; bad descriptors are refused; black where it
must be.

The closed forms' criterion is test_delta_light_mirror's: spp doubles from 4096 until the standard error is at most 0.5 % of the
expectation, then |mean - E| <= 6 se + 1e-3 E per channel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import delta_ref as D
import light_ref as L
import radiometry_ref as R
import test_delta_light_mirror as DM
import test_direct_integrator as DI
import test_envmap as EV
import test_launch_plan as LP
import test_table_placement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CAM = EV.PLANE_CAMERA
W48, CROP = EV.W48, EV.CROP
UP = (0, 1, 0)
POS = DM.POINT                                    # (0.7, 2.5, 0.4): the lamp of the plane scenes
INTENSITY = DM.INTENSITY
SUN_W = (0.3, -1.0, 0.2)                          # the way the sun's light travels (normalised by the flatteners)
SUN_E = (3.0, 2.4, 1.8)
RIGHT = (36, 28)                                  # a second 8 x 8 block of pixels, right of the crop: case (d)'s lit one
DIRECT_NM = [(1, 1), (4, 0), (0, 4), (3, 2)]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def spot_spec(target, cutoff, beam, origin=POS, intensity=INTENSITY, up=UP, **kw):
    return dict({"type": "spot", "intensity": intensity, "cutoff_angle": cutoff, "beam_width": beam, "lookat": {"origin": origin, "target": target, "up": up}}, **kw)


def sun_spec(direction=SUN_W, irradiance=SUN_E, **kw):
    return dict({"type": "directional", "irradiance": irradiance, "direction": direction}, **kw)


def block_pixels(first):
    return np.array([(x, y) for y in range(first[1], first[1] + 8) for x in range(first[0], first[0] + 8)], np.int32)


# ===================================================================================================== CPU 1: the restatement
def test_restatement_checks_itself():
    """(1) the three zones, monotone in c, the hard edge, fp32 within a few 2^-24 of float64"""
    cc, cb = F(0.25), F(0.75)
    assert L.falloff32(np.array([0.75, 0.8, 1.0], F), cc, cb).tolist() == [1.0, 1.0, 1.0]
    assert L.falloff32(np.array([0.25, 0.2, -1.0], F), cc, cb).tolist() == [0.0, 0.0, 0.0]
    assert L.falloff32(np.array([0.5, 0.375, 0.625], F), cc, cb).tolist() == [0.5, 0.15625, 0.84375]       # t = 1/2, 1/4, 3/4: exact in fp32
    c = np.linspace(-1, 1, 20001).astype(F)
    for cc, cb in ((0.25, 0.75), (-1.0, 1.0), (0.9396926, 0.9659258), (-1.0, -1.0), (0.5, 0.5), (0.5, np.nextafter(F(0.5), F(1)))):
        f32, f64 = L.falloff32(c, cc, cb), L.falloff64(c.astype(np.float64), F(cc), F(cb))
        assert np.all(np.diff(f32) >= 0) and f32.min() >= 0 and f32.max() <= 1
        assert np.all(f32[c >= F(cb)] == 1) and np.all(f32[(c <= F(cc)) & (c < F(cb))] == 0)      # the tests' order: the beam first
        # t carries the rounding of c - cos_cutoff (exact here: Sterbenz or small) and one division; the polynomial four more operations
        assert np.all(np.abs(f32 - f64) <= 6 * 2.0 ** -24), (cc, cb, float(np.abs(f32 - f64).max()))
    hard = L.falloff32(np.array([0.5, np.nextafter(F(0.5), F(0)), np.nextafter(F(0.5), F(1))], F), 0.5, 0.5)
    assert hard.tolist() == [1.0, 0.0, 1.0]                            # cos_beam == cos_cutoff: a hard edge, the edge itself lit
    # the sample: straight below the lamp on its axis, distance 2: d = (0, 1, 0), c = 1, value = I / 4
    d, v, pdf = L.spot_sample32((1.0, 3.0, -2.0), (0.0, -1.0, 0.0), 0.5, 0.75, np.array([(1.0, 1.0, -2.0), (1.0, 3.0, -2.0), (1.0, 5.0, -2.0)], F), np.array([(8.0, 3.0, 0.5, 1e-3)] * 3, F))
    assert d.tolist() == [[0.0, 1.0, 0.0, 2.0], [0.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 2.0]]
    assert v.tolist() == [[2.0, 0.75, 0.125, float(F(1e-3) / F(4))], [0.0] * 4, [0.0] * 4] and pdf.tolist() == [1.0, 0.0, 0.0]
    d, v = L.sun_sample32((0.0, -0.6, 0.8), 2.5, np.array([(1.0, 2.0, 3.0, 4.0)] * 2, F))
    assert d.tolist() == [[-0.0, float(F(0.6)), float(F(-0.8)), 5.0]] * 2 and v.tolist() == [[1.0, 2.0, 3.0, 4.0]] * 2
    assert bits(d[0, :1]).tolist() == [0x80000000]                      # the exact negation: -0 for +0


# ===================================================================================================== CPU 2: the packer, native
@pytest.fixture(scope="module")
def native_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("light_tables")
    src = os.path.join(ROOT, "tests", "native", "light_tables_check.cpp")
    plain, san = str(d / "light_tables_check"), str(d / "light_tables_check_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    return plain, san


def test_native_packer_check(native_exe):
    """(2) every refusal with its text, the bytes of the two records, a sun's radius, a scene without the new lights packing to the
    same bytes through the old and the new entry: plain and sanitized, each its own executable"""
    for exe in native_exe:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 100, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("knobs", LP.KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_plan_picks_the_delta_kernels(native_exe, knobs):
    """(5) a spot-only and a sun-only scene, facts as the packer states them: SHADE_DELTA under every knob set"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs)
    r = subprocess.run([native_exe[0], "plan"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.split() == ["cases", str(2 * 7 * 4 * 4 * len(LP.REGION_SIZES) * len(LP.LDS))]


# ===================================================================================================== CPU 3: the two flatteners
def flattener_lights(firsts):
    tw = np.eye(4)
    tw[:3, :3] = EV.skew_rotation()
    return [spot_spec((0.3, 0.0, 0.1), 35.0, 20.0, origin=(1.5, 4.0, -2.0), first=firsts[0]),
            sun_spec((0.3, -1.0, 0.2), 2.5, scale=2.0, first=firsts[1]),
            {"type": "directional", "irradiance": (3.0, 2.0, 1.0), "to_world": tw, "first": firsts[2]},
            {"type": "spot", "lookat": {"origin": (0, 5, 0), "target": (1, 0, 2), "up": (0, 0, 1)}, "first": firsts[3]}]


def flattener_meshes(hm):
    return [DM.plane(hm), hm.MeshSpec("lamp", [tuple(DM.LAMP)], hm.LUMINAIRE, radiance=(40, 30, 20))]


def test_the_two_flatteners_agree(hostmirror, abi, tmp_path):
    """(3) a spot (lookat), a sun by `direction`, a sun by `to_world`, a spot with every default, a point and an area light, in both
    placements: the same descriptors byte for byte, emitter indices in XML order; bad properties refused in the same words"""
    hostlib = EV.host_library()
    for order, firsts in (("behind", (False, False, False, False)), ("mixed", (True, False, True, False))):
        lights = flattener_lights(firsts)
        pts = [DM.point_spec((1.5, 2.0, -3.0), (3.0, 2.0, 1.0), first=firsts[0])]
        xml = hostmirror.write_scene_xml(flattener_meshes(hostmirror), str(tmp_path / order), 16, 16, 1, camera=CAM, points=pts, lights=lights)
        text = open(xml).read()
        assert text.count('<emitter type="spot">') == 2 and text.count('<emitter type="directional">') == 2 and text.count('<emitter type="point">') == 1
        h = hostlib.HostScene(xml).flatten()
        m = hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, points=pts, lights=lights, coeff_lookup=hostlib.srgb_model_fetch)
        assert h.desc.n_emitters == m.desc.n_emitters == 6
        types = [m.desc.emitters[i].type for i in range(6)]
        assert types == ([3, 4, 5, 0, 5, 4] if firsts[0] else [0, 3, 4, 5, 5, 4])
        for i in range(6):
            assert bytes(h.desc.emitters[i]) == bytes(m.desc.emitters[i]), (order, i)
            assert m.desc.emitters[i].mesh_id == (-1 if types[i] else 1)
        assert h.lights is not None and len(h.lights) == len(m.lights) == 4 and bytes(h.lights) == bytes(m.lights)
        assert bytes(h.points) == bytes(m.points)
        assert sorted(l.emitter for l in m.lights) == ([1, 2, 4, 5] if firsts[0] else [2, 3, 4, 5])
        by = {l.emitter: l for l in m.lights}
        s0 = by[1 if firsts[0] else 2]
        assert list(s0.position) == [1.5, 4.0, -2.0]
        assert s0.cos_cutoff == F(np.cos(np.deg2rad(35.0))) and s0.cos_beam == F(np.cos(np.deg2rad(20.0)))
        axis = np.array([0.3 - 1.5, 0.0 - 4.0, 0.1 + 2.0])
        assert np.allclose(list(s0.direction), axis / np.linalg.norm(axis), atol=2e-7)
        s3 = by[5]
        assert list(s3.position) == [0.0, 5.0, 0.0] and s3.cos_cutoff == F(np.cos(np.deg2rad(20.0))) and s3.cos_beam == F(np.cos(np.deg2rad(15.0)))
        for l in m.lights:
            n2 = sum(float(x) ** 2 for x in l.direction)
            assert abs(n2 - 1) < 3e-7
        sun_tw = by[2 if firsts[2] else 4]
        assert np.allclose(list(sun_tw.direction), EV.skew_rotation()[:, 2], atol=2e-7) and list(sun_tw.position) == [0.0, 0.0, 0.0]
    # refusals: the same words on both sides
    cases = [(spot_spec((0, 0, 0), 0.0, 10.0), "spot: cutoff_angle must be in (0, 180] degrees"),
             (spot_spec((0, 0, 0), 181.0, 10.0), "spot: cutoff_angle must be in (0, 180] degrees"),
             (spot_spec((0, 0, 0), 30.0, 31.0), "spot: beam_width must be in (0, cutoff_angle] degrees"),
             (spot_spec((0, 0, 0), 30.0, 0.0), "spot: beam_width must be in (0, cutoff_angle] degrees"),
             (sun_spec((0.0, 0.0, 0.0)), "directional: the direction must not be the zero vector"),
             ({"type": "directional"}, 'directional: exactly one of the parameters "direction" and "to_world" must be specified!'),
             (dict(sun_spec(), to_world=np.eye(4)), 'directional: exactly one of the parameters "direction" and "to_world" must be specified!')]
    for k, (spec, words) in enumerate(cases):
        with pytest.raises(ValueError) as e:
            hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, lights=[spec])
        assert words in str(e.value), (k, str(e.value))
        xml = hostmirror.write_scene_xml(flattener_meshes(hostmirror), str(tmp_path / ("bad%d" % k)), 16, 16, 1, camera=CAM, lights=[spec])
        with pytest.raises(hostlib.HostError) as e:
            hostlib.HostScene(xml).flatten()
        assert words in str(e.value), (k, str(e.value))
    # the limits themselves are taken: 180 degrees is cos = -1 exactly, beam == cutoff a hard edge
    full = hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, lights=[spot_spec((0, 0, 0), 180.0, 180.0)])
    assert full.lights[0].cos_cutoff == -1.0 and full.lights[0].cos_beam == -1.0


# ===================================================================================================== CPU 4: layout and exports
def test_layout_and_exports(abi, tmp_path):
    """(4)"""
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msk_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %zu\\n",'
                   'sizeof(msk_light_desc),offsetof(msk_light_desc,emitter),offsetof(msk_light_desc,position),offsetof(msk_light_desc,direction),'
                   'offsetof(msk_light_desc,cos_cutoff),offsetof(msk_light_desc,cos_beam),sizeof(msk_scene_lights),offsetof(msk_scene_lights,masks),'
                   'offsetof(msk_scene_lights,n_lights),offsetof(msk_scene_lights,lights),MSK_EMITTER_SPOT,MSK_EMITTER_DIRECTIONAL,MSK_ABI_VERSION,'
                   'sizeof(msk_scene_masks));return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    l, s = abi.LightDesc, abi.SceneLights
    assert got == [C.sizeof(l), l.emitter.offset, l.position.offset, l.direction.offset, l.cos_cutoff.offset, l.cos_beam.offset, C.sizeof(s), s.masks.offset,
                   s.n_lights.offset, s.lights.offset, abi.MSK_EMITTER_SPOT, abi.MSK_EMITTER_DIRECTIONAL, abi.MSK_ABI_VERSION, C.sizeof(abi.SceneMasks)]
    assert got[:6] == [36, 0, 4, 16, 28, 32] and got[10:13] == [4, 5, 8] and got[6] == got[13] + 16
    import __graft_entry__ as ge
    ge.build_gpu_library()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("msk_gpu_scene_create_lights", "msk_gpu_light_sample"):
        assert name in abi.EXPORTS and getattr(lib, name) is not None
    hostlib = EV.host_library()
    assert hostlib.load().msk_host_lights is not None


# ===================================================================================================== float64 expectations
def block_rays(desc, m=4, first=CROP):
    t, w = R.gauss_legendre(m)
    yy, xx = np.meshgrid(first[1] + 8 * t, first[0] + 8 * t, indexing="ij")
    o, d = R.camera_ray(desc, xx, yy)
    return o, d, w[:, None] * w[None, :]


def block_corners(desc, first=CROP):
    yy, xx = np.meshgrid(first[1] + 8.0 * np.arange(2), first[0] + 8.0 * np.arange(2), indexing="ij")
    return R.camera_ray(desc, xx, yy)


def light_of(flat, e):
    (l,) = [x for x in flat.lights if x.emitter == e]
    return np.array(l.position[:], np.float64), np.array(l.direction[:], np.float64), float(l.cos_cutoff), float(l.cos_beam)


def zone_of(c, cc, cb):
    return "beam" if np.all(c >= cb) else "dark" if np.all(c <= cc) else "transition" if np.all((c > cc) & (c < cb)) else "mixed"


def spot_on_plane(flat, e, m, zone):
    """the mean over the crop of cos(theta) / d^2 f at the plane through the origin; the crop lies wholly in `zone`: asserted from the
    float64 cosines at its corners (and at the rule's nodes), so that the rule does not straddle a kink"""
    pos, axis, cc, cb = light_of(flat, e)
    o, d = block_corners(flat.desc)
    assert zone_of(L.spot_cosine64(R.hit_plane(o, d, (0, 0, 0), UP), pos, axis), cc, cb) == zone
    o, d, w = block_rays(flat.desc, m)
    x = R.hit_plane(o, d, (0, 0, 0), UP)
    assert zone_of(L.spot_cosine64(x, pos, axis), cc, cb) == zone
    return float((w * L.spot_geometry(x, UP, pos, axis, cc, cb)).sum())


SPOT_CASES = {"a_beam": ((0.0, 0.0, 1.4), 40.0, 30.0, "beam"), "a_transition": ((0.0, 0.0, -3.0), 100.0, 50.0, "transition"), "a_dark": ((0.0, 0.0, -3.0), 40.0, 30.0, "dark")}
SKEW_N = DM.SKEW_N
OCCLUDER_Y = 1.0
OCCLUDER = [(-1.2, OCCLUDER_Y, -0.5), (-1.2, OCCLUDER_Y, 2.7), (0.15, OCCLUDER_Y, 2.7), (0.15, OCCLUDER_Y, -0.5)]
WALL_SPOT = dict(target=(-1.0, 6.0, DM.WALL_Z), cutoff=70.0, beam=20.0)


def in_occluder_shadow(x, w):
    """does the way from the plane points x towards the sun cross the occluder's rectangle?"""
    w = np.asarray(w, np.float64)
    q = x - w * ((OCCLUDER_Y - x[..., 1]) / -w[1])[..., None]
    lo, hi = np.min(OCCLUDER, 0), np.max(OCCLUDER, 0)
    return (q[..., 0] > lo[0]) & (q[..., 0] < hi[0]) & (q[..., 2] > lo[2]) & (q[..., 2] < hi[2])


def mirror_spot_expected(flat, m):
    """(e) F(cos_i) spec rho / pi I cos(theta) / d^2 f at the wall point the mirror shows; the wall points lie in the transition"""
    desc = flat.desc
    pos, axis, cc, cb = light_of(flat, 0)
    o, d, w = block_rays(desc, m)
    x0 = R.hit_plane(o, d, (0, 0, 0), UP)
    d1 = D.reflect(d, UP)
    t = (DM.WALL_Z - x0[..., 2]) / d1[..., 2]
    x1 = x0 + d1 * t[..., None]
    assert np.all(t > 0) and np.all(x1[..., 1] > 0) and np.all(x1[..., 1] < 30) and np.all(np.abs(x1[..., 0]) < 30)
    assert zone_of(L.spot_cosine64(x1, pos, axis), cc, cb) == "transition"
    bd = desc.bsdfs[0]
    f = R.fresnel_conductor(-d[..., 1], float(bd.eta.scale), float(bd.k.scale)) * float(bd.specular_reflectance.scale)
    g = float((w * f * L.spot_geometry(x1, (0, 0, 1), pos, axis, cc, cb)).sum())
    return R.expected_xyz(D.emitter_spectrum(desc, 0) * DM.rho_over_pi(desc, 1), DM.cie_of(desc)) * g


def closed_form_case(hm, name):
    """-> (flat, expectation at 4 x 4 nodes, the same at 8 x 8, the expectation under "direct" at (0, 4) or None where it is the same)"""
    zero = np.zeros(3)
    if name in SPOT_CASES:
        target, cutoff, beam, zone = SPOT_CASES[name]
        flat = hm.flatten([DM.plane(hm)], W48, W48, camera=CAM, lights=[spot_spec(target, cutoff, beam)])
        unit = R.expected_xyz(D.emitter_spectrum(flat.desc, 0) * DM.rho_over_pi(flat.desc), DM.cie_of(flat.desc))
        return flat, unit * spot_on_plane(flat, 0, 4, zone), unit * spot_on_plane(flat, 0, 8, zone), zero
    if name == "b_sun_tilted":
        # wound so that the camera sees its BACK: the twosided adapter flips wi and wo
        flat = hm.flatten([DM.plane(hm, {"type": "diffuse", "twosided": True}, flip=True, rot=EV.skew_rotation())], W48, W48, camera=CAM, lights=[sun_spec()])
        _, w, _, _ = light_of(flat, 0)
        assert np.array(CAM["origin"]) @ SKEW_N > 0 and -w @ SKEW_N > 0.5      # the sun stands on the camera's side of the plane
        e = R.expected_xyz(D.emitter_spectrum(flat.desc, 0) * DM.rho_over_pi(flat.desc), DM.cie_of(flat.desc)) * L.sun_geometry(SKEW_N, w)
        return flat, e, e, zero
    if name == "c_sun_sky_lamp":
        lamp = hm.MeshSpec("lamp", [tuple(DM.LAMP)], hm.LUMINAIRE, radiance=(40, 30, 20))
        flat = hm.flatten([DM.plane(hm), lamp], W48, W48, camera=CAM, env=DM.SKY, lights=[sun_spec(first=True)])
        assert [flat.desc.emitters[i].type for i in range(3)] == [5, 0, 1]
        _, w, _, _ = light_of(flat, 0)
        out = []
        for m in (4, 8):
            o, d, wt = block_rays(flat.desc, m)
            lamp_g = float((wt * R.polygon_irradiance(R.hit_plane(o, d, (0, 0, 0), UP), UP, np.array(DM.LAMP, np.float64))).sum())
            s_s, l_s, k_s = (D.emitter_spectrum(flat.desc, i) for i in range(3))
            for sun_g in (L.sun_geometry(UP, w), 0.0):
                s = R.Spectrum(lambda lam, sun_g=sun_g, lamp_g=lamp_g: s_s(lam) * sun_g + l_s(lam) * lamp_g + k_s(lam) * np.pi, s_s.breaks) * DM.rho_over_pi(flat.desc)
                out.append(R.expected_xyz(s, DM.cie_of(flat.desc)))
        return flat, out[0], out[2], out[1]
    if name in ("d_sun_shadow", "d_sun_beside_shadow"):
        occ = hm.MeshSpec("occluder", [tuple(OCCLUDER)], (0.5, 0.5, 0.5), bsdf={"type": "diffuse", "twosided": True})
        flat = hm.flatten([DM.plane(hm), occ], W48, W48, camera=CAM, lights=[sun_spec()])
        _, w, _, _ = light_of(flat, 0)
        first = CROP if name == "d_sun_shadow" else RIGHT
        for o, d in (block_corners(flat.desc, first), block_rays(flat.desc, 8, first)[:2]):
            x = R.hit_plane(o, d, (0, 0, 0), UP)
            assert np.all(np.abs(x[..., [0, 2]]) < 25)
            assert np.all(in_occluder_shadow(x, w) == (name == "d_sun_shadow"))
            # the camera sees the plane, not the occluder: its ray is at the occluder's height outside the rectangle
            q = o + d * ((OCCLUDER_Y - o[..., 1]) / d[..., 1])[..., None]
            assert np.all((q[..., 2] > 2.7 + 0.1) | (q[..., 0] > 0.15 + 0.1))
        e = R.expected_xyz(D.emitter_spectrum(flat.desc, 0) * DM.rho_over_pi(flat.desc), DM.cie_of(flat.desc)) * L.sun_geometry(UP, w)
        return (flat, zero, zero, zero) if name == "d_sun_shadow" else (flat, e, e, zero)
    if name == "e_mirror_then_spot":
        flat = hm.flatten(DM.mirror_lamp_meshes(hm), W48, W48, camera=CAM,
                          lights=[spot_spec(WALL_SPOT["target"], WALL_SPOT["cutoff"], WALL_SPOT["beam"], origin=DM.LAMP_E, intensity=(300.0, 240.0, 180.0))])
        return flat, mirror_spot_expected(flat, 4), mirror_spot_expected(flat, 8), zero
    raise KeyError(name)


def dark_film_flat(hm):
    """the lamp of the plane scenes turned sideways: its cone meets the plane beyond x = 3, the camera sees |x| < 3.  Every film
    position (the filter's border included) looks at the plane outside the cone: asserted from the float64 cosines"""
    flat = hm.flatten([DM.plane(hm)], W48, W48, camera=CAM, lights=[spot_spec((30.0, 0.0, 0.4), 40.0, 30.0)])
    pos, axis, cc, cb = light_of(flat, 0)
    yy, xx = np.meshgrid(np.linspace(-2.0, W48 + 2.0, 53), np.linspace(-2.0, W48 + 2.0, 53), indexing="ij")
    o, d = R.camera_ray(flat.desc, xx, yy)
    x = R.hit_plane(o, d, (0, 0, 0), UP)
    assert np.all(d[..., 1] < 0) and np.all(np.abs(x[..., [0, 2]]) < 25)
    c = L.spot_cosine64(x, pos, axis)
    assert np.all(c <= cc - 0.05), float(c.max())
    return flat


CASES = ["a_beam", "a_transition", "a_dark", "b_sun_tilted", "c_sun_sky_lamp", "d_sun_shadow", "d_sun_beside_shadow", "e_mirror_then_spot"]
BLACK = ("a_dark", "d_sun_shadow")


@pytest.mark.parametrize("name", CASES)
def test_expectations_have_converged(hostmirror, name):
    """(6) the 4 x 4 Gauss-Legendre rule over the crop against 8 x 8, to 1e-5 relative; the zones are asserted inside closed_form_case"""
    _, e4, e8, e04 = closed_form_case(hostmirror, name)
    print("LIGHT %s: expectation %s (8 x 8 nodes: %s; direct (0, 4): %s)" % (name, e4, e8, e04))
    if name in BLACK:
        assert not e4.any() and not e8.any()
        dark_film_flat(hostmirror)
    else:
        assert np.all(e4 > 0) and np.all(np.abs(e4 - e8) <= 1e-5 * e8)
    assert np.all(e04 >= 0) and (e04.any() == (name == "c_sun_sky_lamp")) and np.all(e04 <= e4)


# ===================================================================================================== GPU 7: the probe
PROBE_SPOT = dict(origin=(0.75, 2.5, -1.25), target=(0.25, 0.0, -0.5))


def probe_flat(hm, cos=None):
    """the probe's scene: a plane, a lamp (emitter 0), a point light (1), a spot with an rgb intensity (2), a sun (3) and a spot
    with a `regular` intensity (4).  cos = (cos_cutoff, cos_beam) overwrites the first spot's cosines"""
    lamp = hm.MeshSpec("lamp", [tuple(DM.LAMP)], hm.LUMINAIRE, radiance=(40, 30, 20))
    reg = hm.Regular(400.0, 700.0, [0.5, 2.0, 1.0, 3.0, 0.25, 1.5, 2.5])
    lights = [spot_spec(PROBE_SPOT["target"], 50.0, 25.0, origin=PROBE_SPOT["origin"]), sun_spec((0.3, -1.0, 0.2), (3.0, 2.0, 1.0)),
              spot_spec((0.75, 0.0, -1.25), 80.0, 30.0, origin=(0.5, 3.5, -1.0), intensity=reg, up=(0, 0, 1))]
    flat = hm.flatten([DM.plane(hm), lamp], 16, 16, camera=CAM, lights=lights, points=[DM.point_spec((1.0, 2.0, 3.0), 2.0)])
    assert [flat.desc.emitters[i].type for i in range(5)] == [0, 3, 4, 5, 4]
    if cos is not None:
        flat.lights[0].cos_cutoff, flat.lights[0].cos_beam = float(cos[0]), float(cos[1])
    return flat


def probe_points():
    """reference points around the first spot: random ones (beam, transition and dark), along 13 directions at distances 2^-10 ..
    2^10, and the position itself"""
    rng = np.random.RandomState(29)
    pos = np.array(PROBE_SPOT["origin"], F)
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 1), (-1, 1, 1), (1, 1, 1), (-1, -1, -1), (0, 1, -1), (3, -2, 1)]
    far = [pos.astype(np.float64) + np.array(d, np.float64) / np.linalg.norm(d) * 2.0 ** k for k in range(-10, 11) for d in dirs][:255]
    p = np.concatenate([pos + rng.uniform(-2, 2, (3840, 3)), far, [pos]]).astype(F)
    wl = rng.uniform(360, 830, (4096, 4)).astype(F)
    return pos, p, wl


def emitter_value32(hm, oracle, flat, e, wl):
    d = flat.desc
    ed = d.emitters[e]
    if ed.radiance_regular:
        r = d.regular_spectra[ed.radiance_regular - 1]
        table = np.array([d.regular_values[r.first_value + i] for i in range(r.size)], F)
        return R_regular32(table, r.lambda_min, r.lambda_max, wl)
    _, d65 = hm.cie_tables()
    return D.intensity32(oracle, ed.radiance[:], (d65 * F(ed.d65_scale)).astype(F), wl)


def R_regular32(table, lambda_min, lambda_max, wl):
    """a `regular` radiance on its own grid (msk_gpu.h, msk_regular_spectrum_desc), in fp32 as the device evaluates an emitter's table"""
    wl = np.asarray(wl, F).reshape(-1, 4)
    inv = F(1.0 / ((float(lambda_max) - float(lambda_min)) / (len(table) - 1)))
    x = ((wl - F(lambda_min)).astype(F) * inv).astype(F)
    i = np.minimum(np.maximum(x, 0).astype(np.int64), len(table) - 2)
    w1 = (x - i.astype(F)).astype(F)
    w0 = (F(1) - w1).astype(F)
    return ((w0 * table[i]).astype(F) + (w1 * table[i + 1]).astype(F)).astype(F)


@pytest.mark.gpu
def test_probe_equals_the_restatement_bit_for_bit(gpu_ctx, hostmirror, oracle, abi):
    """(7) msk_gpu_light_sample runs the device function the shading kernels call; no case excluded"""
    pos, p, wl = probe_points()
    flat = probe_flat(hostmirror)
    sp_pos, sp_axis, cc, cb = light_of(flat, 2)
    c = L.spot_cosine32(sp_pos, sp_axis, p)
    f = L.falloff32(c, cc, cb)
    assert (f == 1).sum() > 100 and (f == 0).sum() > 100 and ((f > 0) & (f < 1)).sum() > 100      # beam, dark, transition
    k = int(np.argmax((f > 0.3) & (f < 0.7)))
    scenes = [("as flattened", flat), ("cos_beam = c of point %d" % k, probe_flat(hostmirror, (cc, c[k]))), ("cos_cutoff = c of point %d" % k, probe_flat(hostmirror, (c[k], cb)))]
    for what, fl in scenes:
        g = abi.Scene(gpu_ctx, fl)
        try:
            for e in (2, 4):
                lp, la, lc, lb = light_of(fl, e)
                gd, gv = g.light_sample(e, p, wl)
                rd, rv, pdf = L.spot_sample32(lp, la, lc, lb, p, emitter_value32(hostmirror, oracle, fl, e, wl))
                for name, a, b in (("d, dist", gd, rd), ("value", gv, rv)):
                    bad = (bits(a) != bits(b)).reshape(len(a), -1).any(-1)
                    assert not bad.any(), (what, e, name, int(bad.sum()), a[bad][:3], b[bad][:3], p[bad][:3])
                assert np.all(np.isfinite(gd)) and np.all(np.isfinite(gv))
                if e == 2:
                    assert not gd[-1].any() and not gv[-1].any()             # the position itself: zeros
                    assert not gv[pdf == 0].any() and gd[:-1][pdf[:-1] == 0].any()      # in the dark: d and dist, no value
                    if fl is not flat:       # on the boundary: c >= cos_beam gives 1, c <= cos_cutoff gives 0
                        want = rv[k] if "beam" in what else np.zeros(4, F)
                        assert np.array_equal(gv[k], want) and (pdf[k] == (1 if "beam" in what else 0))
                        one = L.spot_sample32(lp, la, -1.0, -1.0, p[k:k + 1], emitter_value32(hostmirror, oracle, fl, e, wl[k:k + 1]))[1][0]
                        assert ("beam" not in what) or np.array_equal(gv[k], one)
            # the sun: the exact negation, 2 env_radius, E, from every point
            _, w, _, _ = light_of(fl, 3)
            gd, gv = g.light_sample(3, p, wl)
            rd, rv = L.sun_sample32(w, L.env_radius32(fl.vertices), emitter_value32(hostmirror, oracle, fl, 3, wl))
            assert np.array_equal(bits(gd), bits(rd)) and np.array_equal(bits(gv), bits(rv)) and rd[0, 3] > 0
            for call, text in ((lambda: g.light_sample(0, p[:1], wl[:1]), "emitter 0 is neither a spot nor a directional emitter"),
                               (lambda: g.light_sample(1, p[:1], wl[:1]), "emitter 1 is neither a spot nor a directional emitter"),
                               (lambda: g.light_sample(5, p[:1], wl[:1]), "emitter 5 is neither a spot nor a directional emitter"),
                               (lambda: g.point_sample(2, p[:1], wl[:1]), "emitter 2 is not a point emitter")):
                with pytest.raises(abi.MskError) as err:
                    call()
                assert text in str(err.value) and err.value.code == abi.MSK_ERR_INVALID_ARG
        finally:
            g.close()


# ===================================================================================================== GPU 8: the spot that is a point light
def wall_and_floor(hm):
    wall = hm.MeshSpec("wall", [((-30.0, 0.0, DM.WALL_Z), (30.0, 0.0, DM.WALL_Z), (30.0, 30.0, DM.WALL_Z), (-30.0, 30.0, DM.WALL_Z))], (0.6, 0.5, 0.4))      # faces +z
    return [DM.plane(hm), wall]


@pytest.mark.gpu
def test_a_spot_that_covers_the_sphere_is_the_point_light(gpu_ctx, hostmirror, abi):
    """(8) cutoff_angle = beam_width = 180 (cos = -1): the first branch is taken everywhere.  The lamp stands above the floor and in
    front of the wall and looks down at the wall's foot: every surface point has c > 0.  Samples and films equal those of the point
    scene, bit for bit"""
    lamp, inten = (0.7, 2.5, 0.4), (300.0, 240.0, 180.0)
    spot = hostmirror.flatten(wall_and_floor(hostmirror), W48, W48, camera=CAM, lights=[spot_spec((0.0, 0.0, DM.WALL_Z), 180.0, 180.0, origin=lamp, intensity=inten)])
    point = hostmirror.flatten(wall_and_floor(hostmirror), W48, W48, camera=CAM, points=[DM.point_spec(lamp, inten)])
    pos, axis, cc, cb = light_of(spot, 0)
    assert cc == cb == -1.0 and list(pos) == list(point.points[0].position) and bytes(spot.desc.emitters[0])[4:] == bytes(point.desc.emitters[0])[4:]
    assert axis[1] < 0 and axis[2] < 0      # down and towards the wall: the floor (y = 0 < 2.5) and the wall (z = -6 < 0.4) lie ahead or beside, never straight behind
    gs, gp = abi.Scene(gpu_ctx, spot), abi.Scene(gpu_ctx, point)
    try:
        px = np.array([(x, y) for y in range(0, 48, 3) for x in range(0, 48, 3)], np.int32)
        for depth in (2, -1):
            prm = abi.render_params(spp=16, seed=5, max_depth=depth)
            a, apos = gs.sample_pixels(prm, px)
            b, bpos = gp.sample_pixels(prm, px)
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(apos), bits(bpos)) and a.max() > 0, depth
            fa, sa = gs.render(abi.render_params(spp=8, seed=5, max_depth=depth))
            fb, sb = gp.render(abi.render_params(spp=8, seed=5, max_depth=depth))
            assert np.array_equal(bits(fa), bits(fb)) and (sa.segments, sa.shadow_rays) == (sb.segments, sb.shadow_rays) and sa.shadow_rays > 0
            sa2, _ = gs.render(EV.pcg(abi, spp=2, seed=5, max_depth=depth))
            sb2, _ = gp.render(EV.pcg(abi, spp=2, seed=5, max_depth=depth))
            assert np.array_equal(bits(sa2), bits(sb2)) and sa2[..., :3].max() > 0
        prm = abi.render_params(spp=8, seed=5)
        a, _ = gs.sample_pixels_direct(prm, px, 4, 2)
        b, _ = gp.sample_pixels_direct(prm, px, 4, 2)
        assert np.array_equal(bits(a), bits(b)) and a.max() > 0
        fa, _ = gs.render_direct(prm, 4, 2)
        fb, _ = gp.render_direct(prm, 4, 2)
        assert np.array_equal(bits(fa), bits(fb))
    finally:
        gs.close(); gp.close()


# ===================================================================================================== GPU 9: closed forms
def sampled_mean(sample, what, expected, pixels):
    """test_delta_light_mirror's procedure over any sampler: spp doubles from 4096 until the standard error is at most 0.5 % of the
    expectation, four doublings at the most"""
    spp = 4096
    for _ in range(5):
        xyz = sample(spp, pixels)
        v = xyz.reshape(-1, 3).astype(np.float64)
        mean, se = v.mean(0), v.std(0, ddof=1) / np.sqrt(len(v))
        print("LIGHT %s spp %d: expected %s mean %s se/|E| %s dev/|E| %s" % (what, spp, expected, mean, se / expected, (mean - expected) / expected))
        if np.all(se <= 5e-3 * expected):
            return mean, se
        spp *= 2
    raise AssertionError("the standard error stays above 0.5 %% of the expectation: %s" % (se / expected,))


def case_pixels(name):
    return block_pixels(RIGHT if name == "d_sun_beside_shadow" else CROP)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_rendered_radiance_meets_the_closed_form(gpu_ctx, hostmirror, abi, name):
    """(9 a-e) "path", counter RNG through msk_gpu_sample_pixels: |mean - E| <= 6 standard errors + 1e-3 E per channel; in the dark
    and in the shadow exactly 0, and in the dark no shadow ray is traced"""
    flat, expected, _, _ = closed_form_case(hostmirror, name)
    depth = 3 if name == "e_mirror_then_spot" else 2
    g = abi.Scene(gpu_ctx, flat)
    try:
        sample = lambda spp, px: g.sample_pixels(abi.render_params(spp=spp, seed=7, max_depth=depth), px)[0]
        if name in BLACK:
            xyz = sample(256, case_pixels(name))
            assert np.isfinite(xyz).all() and not xyz.any()
            film, st = g.render(abi.render_params(spp=8, seed=7, max_depth=depth))
            assert np.isfinite(film).all()
            if name == "a_dark":      # f == 0 is pdf 0: no shadow ray.  msk_stats counts a whole render's, so: a film that lies in the dark everywhere
                assert not film[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, :3].any() and film[..., :3].max() > 0 and st.shadow_rays > 0
                g.close()
                g = abi.Scene(gpu_ctx, dark_film_flat(hostmirror))
                film, st = g.render(abi.render_params(spp=8, seed=7, max_depth=depth))
                assert st.samples == W48 * W48 * 8 and st.shadow_rays == 0 and not film[..., :3].any() and np.isfinite(film).all()
            else:
                assert st.shadow_rays > 0 and not film[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, :3].any() and film[..., :3].max() > 0
            return
        mean, se = sampled_mean(sample, "%s path" % name, expected, case_pixels(name))
        if name == "e_mirror_then_spot":
            xyz, _ = g.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=2), case_pixels(name))
            assert not xyz.any()                                         # at max_depth = 2 the path ends on the wall, before its next-event sample
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", DIRECT_NM)
@pytest.mark.parametrize("name", CASES)
def test_direct_meets_the_closed_form(gpu_ctx, hostmirror, abi, name, n, m):
    """(9) the same cases under "direct".  A delta light is reached by light samples alone: at (0, 4) it adds nothing, and a scene
    lit by a spot or a sun alone is exactly 0.  The mirror of case (e) has no smooth lobe and its BSDF sample ends on the wall, which
    does not emit: exactly 0 at every (N, M)"""
    flat, expected, _, e04 = closed_form_case(hostmirror, name)
    if n == 0:
        expected = e04
    if name == "e_mirror_then_spot":
        expected = np.zeros(3)
    g = abi.Scene(gpu_ctx, flat)
    try:
        sample = lambda spp, px: g.sample_pixels_direct(abi.render_params(spp=spp, seed=7), px, n, m)[0]
        if not expected.any():
            xyz = sample(256, case_pixels(name))
            assert np.isfinite(xyz).all() and not xyz.any()
            return
        mean, se = sampled_mean(sample, "%s direct (%d, %d)" % (name, n, m), expected, case_pixels(name))
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


# ===================================================================================================== GPU 10, 11: variants
BOX_SPOT = spot_spec((278.0, 0.0, 279.6), 50.0, 30.0, origin=(120.0, 420.0, 200.0), intensity=(4e5, 3e5, 2e5))
BOX_SUN = sun_spec((0.25, -1.0, 0.35), (6.0, 5.0, 4.0))


def box_meshes(hm, pads=()):
    """test_delta_light_mirror's variant box (open Cornell box, area light, bitmap floor, glass ball, mirror ball).  The mirror ball
    has 5 x 5 rings instead of 6 x 6: with one emitter more than that test's scene, tree and tables still fit the fused kernels' LDS"""
    ball = hm.blob_mesh("mirror", (170, 100, 330), 90, 5, 5, hm.WHITE, seed=4)
    ball.bsdf = dict(DM.GOLD_RGB)
    return EV.variant_meshes(hm, [ball] + list(pads))


def box_flat(hm, which, sky, size=(48, 48)):
    """the variant box under a spot and a sun"""
    env = EV.env_spec(EV.lit_image(), EV.skew_rotation(), scale=40.0) if sky == "envmap" else None
    lights = [BOX_SPOT, BOX_SUN]
    if which == "lds":
        return hm.flatten(box_meshes(hm), size[0], size[1], env=env, lights=lights)
    filler = hm.blob_mesh("filler", (150, 420, 400), 60, 16, 16, hm.WHITE, seed=9)
    base = hm.flatten(box_meshes(hm, [filler]), size[0], size[1], env=env, lights=lights)
    pads = T.faceless_pads(hm, T.SMALL_TABLES_F4 + 1 - T.table_plan(base)["small_f4"])
    return hm.flatten(box_meshes(hm, [filler] + pads), size[0], size[1], env=env, lights=lights)


def test_variant_scenes_sit_where_the_tests_say(hostmirror, abi):
    """test_table_placement.table_plan counts the area emitters' CDFs; a spot adds its five floats to that pool, at most two float4:
    the LDS scene stays far below the limits, the HBM scene above the small tables' limit"""
    for sky in ("none", "envmap"):
        lds, hbm = box_flat(hostmirror, "lds", sky), box_flat(hostmirror, "hbm", sky)
        pl, ph = T.table_plan(lds), T.table_plan(hbm)
        assert pl["table_f4"] + 2 <= T.LDS_TABLES_F4 and pl["small_f4"] + 2 <= T.SMALL_TABLES_F4
        assert not ph["lds_tables"] and not ph["small_staged"] and ph["small_f4"] == T.SMALL_TABLES_F4 + 1
        d = lds.desc
        assert sorted(d.emitters[i].type for i in range(d.n_emitters)) == ([0, 2, 4, 5] if sky == "envmap" else [0, 4, 5])


@pytest.mark.gpu
@pytest.mark.parametrize("hide", [0, 1])
def test_direct_one_one_is_path_at_depth_two(gpu_ctx, hostmirror, abi, hide):
    """(10) spot, sun, area and envmap in one scene: samples, film positions and films as bits"""
    g = abi.Scene(gpu_ctx, box_flat(hostmirror, "lds", "envmap", size=(DI.FW, DI.FH)))
    try:
        prm = abi.render_params(spp=6, seed=11, max_depth=2, rr_depth=5, hide_emitters=hide, block_size=DI.BS)
        want, wpos = g.sample_pixels(prm, DI.all_pixels())
        got, gpos = g.sample_pixels_direct(prm, DI.all_pixels(), 1, 1)
        assert np.array_equal(bits(gpos), bits(wpos))
        bad = (bits(got) != bits(want)).any(-1)
        assert not bad.any(), (hide, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:3], want[bad][:3])
        assert np.isfinite(want).all() and want.max() > 0
        film_p, st_p = g.render(prm)
        film_d, st_d = g.render_direct(prm, 1, 1)
        assert np.array_equal(bits(film_d), bits(film_p)), (hide, float(np.abs(film_d - film_p).max()))
        assert st_d.samples == st_p.samples == DI.FW * DI.FH * 6
    finally:
        g.close()


@pytest.fixture(scope="module")
def variant_reference(gpu_ctx, hostmirror, abi):
    """the default variant's samples and films of the four scenes (no knob set): computed once, never changed"""
    saved = {k: os.environ.pop(k) for k in DM.KNOBS if k in os.environ}
    out = {}
    try:
        for sky in ("none", "envmap"):
            for which in ("lds", "hbm"):
                flat = box_flat(hostmirror, which, sky)
                g = abi.Scene(gpu_ctx, flat)
                xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
                film, st = g.render(abi.render_params(spp=8, seed=5))
                serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
                g.close()
                for a in (xyz, pos, film, serial):
                    a.setflags(write=False)
                assert np.isfinite(film).all() and film[..., :3].max() > 0 and np.isfinite(serial).all()
                out[sky, which] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, samples=st.samples)
    finally:
        os.environ.update(saved)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sky", ["none", "envmap"])
@pytest.mark.parametrize("which,env,expect", [("lds", e, x) for e, x in DM.LDS_VARIANTS] + [("hbm", e, x) for e, x in DM.HBM_VARIANTS],
                         ids=lambda v: EV.variant_id(v) if isinstance(v, dict) else str(v).replace(" ", "_"))
def test_every_execution_variant(gpu_ctx, abi, variant_reference, monkeypatch, which, env, expect, sky):
    """(11) films and samples byte-equal to the default variant's (the anchor is the closed forms, not this test); the serial kernel
    against itself; msk_stats says which kernels made the film"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = variant_reference[sky, which]
    g = abi.Scene(gpu_ctx, want["flat"])
    gx, gp = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
    film, st = g.render(abi.render_params(spp=8, seed=5))
    serial, _ = g.render(EV.pcg(abi, spp=2, seed=5))
    g.close()
    got = "trace %d shade %d wavefront %d" % (st.launches_trace, st.launches_shade, st.launches_wavefront)
    print("LIGHT variant %s %s %s: %s" % (sky, which, EV.variant_id(env), got))
    assert np.array_equal(bits(gp), bits(want["pos"]))
    assert np.array_equal(bits(gx), bits(want["xyz"])), env
    assert np.array_equal(bits(film), bits(want["film"])), (env, float(np.abs(film - want["film"]).max()))
    assert np.array_equal(bits(serial), bits(want["serial"])), env
    assert st.samples == want["samples"]
    if expect == EV.SPLIT:
        assert st.launches_wavefront == 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == EV.FUSED_PART:
        assert st.launches_wavefront > 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == EV.FUSED_ALL:
        assert st.launches_wavefront > 0 and st.launches_shade == 0 and st.launches_trace == 0, got
    else:
        assert st.launches_shade > 0 and st.launches_trace > 0, got


# ===================================================================================================== GPU 12: mask over spot
@pytest.mark.gpu
def test_mask_over_spot(gpu_ctx, hostmirror, abi):
    """(12) a mask(diffuse) floor under a spot and a sun takes the _m kernels; at opacity 1 it is the unmasked scene, bit for bit"""
    lights = [spot_spec((0.0, 0.0, 1.4), 40.0, 30.0), sun_spec()]
    plain = hostmirror.flatten(wall_and_floor(hostmirror), W48, W48, camera=CAM, lights=lights)
    meshes = wall_and_floor(hostmirror)
    meshes[0].bsdf = {"type": "mask", "opacity": 1.0, "bsdf": {"type": "diffuse"}}
    masked = hostmirror.flatten(meshes, W48, W48, camera=CAM, lights=lights)
    assert masked.masks is not None and len(masked.masks) == 1 and plain.masks is None
    assert bytes(masked.desc.bsdfs[0]) == bytes(plain.desc.bsdfs[0])
    gm, gp = abi.Scene(gpu_ctx, masked), abi.Scene(gpu_ctx, plain)
    try:
        a0, _ = gm.mask_eval(0, np.array([[0.5, 0.5]], F), np.array([[0, 0, 1]], F), np.array([[0, 0, 1]], F), np.full((1, 4), 550, F))
        assert a0[0, 0] == 1.0                                            # the mask probe answers: the scene holds a mask
        for depth in (2, -1):
            a, apos = gm.sample_pixels(abi.render_params(spp=16, seed=5, max_depth=depth), EV.crop_pixels())
            b, bpos = gp.sample_pixels(abi.render_params(spp=16, seed=5, max_depth=depth), EV.crop_pixels())
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(apos), bits(bpos)) and a.max() > 0
            fa, _ = gm.render(abi.render_params(spp=4, seed=5, max_depth=depth))
            fb, _ = gp.render(abi.render_params(spp=4, seed=5, max_depth=depth))
            assert np.array_equal(bits(fa), bits(fb)) and fa[..., :3].max() > 0
            sa, _ = gm.render(EV.pcg(abi, spp=2, seed=5, max_depth=depth))
            sb, _ = gp.render(EV.pcg(abi, spp=2, seed=5, max_depth=depth))
            assert np.array_equal(bits(sa), bits(sb))
    finally:
        gm.close(); gp.close()


# ===================================================================================================== GPU 13: group, refusals
@pytest.mark.gpu
def test_two_members_behind_one_context(abi, hostmirror):
    """(13) msk_gpu_init with n = 2 renders a spot + sun scene to the single-device film bit for bit (MSK_RNG_PCG_BLOCK on a 64 x 32
    film: two blocks, one per member); the extension reaches every member, and the probe answers through the group"""
    n_dev = C.c_int(0)
    assert abi.load_library().hipGetDeviceCount(C.byref(n_dev)) == 0
    lamp = hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))
    flat = hostmirror.flatten([DM.plane(hostmirror), lamp], 64, 32, camera=CAM, lights=[spot_spec((0.0, 0.0, 1.4), 60.0, 30.0, first=True), sun_spec()])
    prm = EV.pcg(abi, spp=8, seed=5)
    probe = (np.array([[0.1, 0.0, 1.2]], F), np.full((1, 4), 550, F))
    with abi.Context(0) as one:
        s1 = abi.Scene(one, flat)
        ref, st1 = s1.render(prm)
        p1 = [s1.light_sample(e, *probe) for e in (0, 2)]
        s1.close()
    assert st1.samples == 64 * 32 * 8 and ref[..., :3].max() > 0 and p1[0][1].max() > 0
    for members in [(0, 0)] + ([(0, 1)] if n_dev.value >= 2 else []):
        with abi.Context(members) as grp:
            s2 = abi.Scene(grp, flat)
            film, st2 = s2.render(prm)
            p2 = [s2.light_sample(e, *probe) for e in (0, 2)]
            s2.close()
        assert st2.samples == st1.samples
        assert np.array_equal(bits(film), bits(ref)), (members, float(np.abs(film - ref).max()))
        for a, b in zip(p1, p2):
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.gpu
def test_gpu_rejects_bad_light_descriptors(gpu_ctx, hostmirror, abi):
    """(13) msk_gpu_scene_create_lights through the C ABI refuses each bad descriptor with the packer's words"""
    lamp = hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))

    def fresh():
        return hostmirror.flatten([DM.plane(hostmirror), lamp], 16, 16, camera=CAM, lights=[spot_spec((0.0, 0.0, 1.4), 40.0, 30.0), sun_spec()])

    def copy(l, **kw):
        c = abi.LightDesc.from_buffer_copy(bytes(l))
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    def refused(flat, text, lights=None, entry=None):
        with pytest.raises(abi.MskError) as e:
            if entry is not None:
                h = C.c_void_p()
                gpu_ctx.check(entry(gpu_ctx.handle, C.byref(flat.desc), C.byref(h)))
            else:
                abi.Scene(gpu_ctx, flat, lights=lights)
        assert text in str(e.value), str(e.value)
        assert e.value.code == abi.MSK_ERR_INVALID_ARG
    flat = fresh()
    assert [flat.desc.emitters[i].type for i in range(3)] == [0, 4, 5] and [l.emitter for l in flat.lights] == [1, 2]
    sp, su = flat.lights[0], flat.lights[1]
    abi.Scene(gpu_ctx, flat).close()                                   # the scene itself is fine
    abi.Scene(gpu_ctx, flat, lights=[su, sp]).close()                  # ... in any order
    refused(fresh(), "emitter 1: a spot emitter needs its geometry", entry=gpu_ctx.lib.msk_gpu_scene_create)      # the older entries: refused, not defaulted
    refused(flat, "emitter 2: a directional emitter needs its geometry", lights=[sp])
    refused(flat, "emitter 1: a spot emitter needs its geometry", lights=[su])
    refused(flat, "emitter 1: a spot emitter with two descriptors (msk_light_desc 2 is its second)", lights=[sp, su, sp])
    refused(flat, "emitter 2: a directional emitter with two descriptors", lights=[sp, su, su])
    refused(flat, "msk_light_desc 2: emitter 0 is of type 0, neither a spot", lights=[sp, su, copy(sp, emitter=0)])
    refused(flat, "msk_light_desc 2: emitter 7 out of range", lights=[sp, su, copy(sp, emitter=7)])
    for bad in (np.inf, -np.inf, np.nan):
        refused(flat, "emitter 1: a spot emitter's position must be finite", lights=[copy(sp, position=(1, bad)), su])
        refused(flat, "emitter 1: a spot emitter's direction must be finite", lights=[copy(sp, direction=(0, bad)), su])
        refused(flat, "emitter 2: a directional emitter's direction must be finite", lights=[sp, copy(su, direction=(2, bad))])
    refused(flat, "emitter 1: a spot emitter's direction must have unit length", lights=[copy(sp, direction=(1, float(sp.direction[1]) * 1.01)), su])
    refused(flat, "emitter 2: a directional emitter's direction must have unit length", lights=[sp, copy(su, direction=(1, 0.0))])
    refused(flat, "emitter 1: a spot emitter's cos_cutoff 1 is outside [-1, 1)", lights=[copy(sp, cos_cutoff=1.0, cos_beam=1.0), su])
    refused(flat, "emitter 1: a spot emitter's cos_cutoff -1.5 is outside [-1, 1)", lights=[copy(sp, cos_cutoff=-1.5), su])
    refused(flat, "is outside [cos_cutoff, 1]", lights=[copy(sp, cos_beam=float(np.nextafter(F(sp.cos_cutoff), F(-1)))), su])
    refused(flat, "is outside [cos_cutoff, 1]", lights=[copy(sp, cos_beam=1.25), su])
    # n_lights without lights
    el = abi.SceneLights(abi.SceneMasks(abi.SceneExt(None, 0, None), 0, None), 2, None)
    h = C.c_void_p()
    with pytest.raises(abi.MskError) as e:
        gpu_ctx.check(gpu_ctx.lib.msk_gpu_scene_create_lights(gpu_ctx.handle, C.byref(flat.desc), C.byref(el), C.byref(h)))
    assert "msk_scene_lights: n_lights 2 without lights" in str(e.value) and e.value.code == abi.MSK_ERR_INVALID_ARG
    for e_id, what in ((1, "spot"), (2, "directional")):
        f2 = fresh()
        f2.desc.emitters[e_id].mesh_id = 0
        refused(f2, "emitter %d: a %s emitter has no mesh" % (e_id, what))
    # a scene without the new lights takes no msk_light_desc; an unknown type keeps its words
    none = hostmirror.flatten([DM.plane(hostmirror), lamp], 16, 16, camera=CAM)
    refused(none, "msk_light_desc 0: emitter 0 is of type 0, neither a spot", lights=[copy(sp, emitter=0)])
    f9 = fresh()
    f9.desc.emitters[1].type = 9
    with pytest.raises(abi.MskError) as e:
        abi.Scene(gpu_ctx, f9)
    assert "emitter 1: type 9 is not supported (area, constant, envmap, point)" in str(e.value) and e.value.code == abi.MSK_ERR_UNSUPPORTED


# ===================================================================================================== GPU 14: black where it must be
@pytest.mark.gpu
def test_black_from_below_and_from_behind(gpu_ctx, hostmirror, abi):
    """(14) a spot below a one-sided plane and a sun that shines on its back: exactly 0 in both RNG modes; the lit counterparts are
    not; the films are finite everywhere"""
    below = hostmirror.flatten([DM.plane(hostmirror)], W48, W48, camera=CAM, lights=[spot_spec((0.0, 0.0, 1.4), 180.0, 180.0, origin=(0.7, -2.5, 0.4))])
    behind = hostmirror.flatten([DM.plane(hostmirror)], W48, W48, camera=CAM, lights=[sun_spec((0.3, 1.0, 0.2))])
    above = hostmirror.flatten([DM.plane(hostmirror)], W48, W48, camera=CAM, lights=[spot_spec((0.0, 0.0, 1.4), 180.0, 180.0)])
    front = hostmirror.flatten([DM.plane(hostmirror)], W48, W48, camera=CAM, lights=[sun_spec()])
    for flat, black in ((below, True), (behind, True), (above, False), (front, False)):
        g = abi.Scene(gpu_ctx, flat)
        xyz, _ = g.sample_pixels(abi.render_params(spp=64, seed=7), EV.crop_pixels())
        film, _ = g.render(EV.pcg(abi, spp=2, seed=7))
        full, _ = g.render(abi.render_params(spp=4, seed=7))
        g.close()
        rows = film[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, :3]
        assert np.isfinite(xyz).all() and np.isfinite(film).all() and np.isfinite(full).all()
        assert (not xyz.any() and not film[..., :3].any() and not full[..., :3].any()) if black else (xyz.min() > 0 and rows.min() > 0)
