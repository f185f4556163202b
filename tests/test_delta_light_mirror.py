"""The `point` emitter and the smooth `conductor` (include/msk_gpu.h at msk_point_desc and MSK_BSDF_CONDUCTOR):
a delta light and a delta BSDF.

CPU: the restatement checks itself (delta_ref.py), layout and exports, the two flatteners, the launch plan as a stand-alone native
program, the float64 expectations' own convergence.  GPU: the probes equal the fp32 restatement bit for bit; a scene that merely
CARRIES a conductor entry renders the oracle's film through the new kernels; rendered radiance meets float64 closed forms (a point
light over a diffuse plane, beside an area light, beside a `constant` sky; a mirror under the sky; a lamp seen in a mirror); every
execution variant makes the same film; bad descriptors are refused; a group context; the "aov" integrator.

The miss-branch density (closed form c).  With a point light beside a `constant` sky the older kernels' rule — the MIS weight of a
BSDF sample that leaves the scene uses the density of the bounce's NEXT-EVENT RECORD (path.cpp:90-95) — no longer adds up: when the
bounce's next-event sample went to the point light that record holds no sky density, the BSDF sample counts in full, and the sky
sample of the other half of the bounces still counts with its own weight.  On a diffuse surface under a uniform sky, two emitters:
sky term = rho L (1 + A / 2) with A = integral of (cos / pi) p_l^2 / (p_l^2 + p_b^2), p_l = 1 / (8 pi), p_b = cos / pi, which is
ln(65) / 64 = 0.0652: +3.26 % on the sky's part (test_stale_record_would_be_off_by_per_cents computes it by quadrature).  The
kernels of this family use the density of the ray's own direction, and the weights sum to 1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import delta_ref as D
import radiometry_ref as R
import test_envmap as EV
import test_launch_plan as LP
import test_table_placement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CAM = EV.PLANE_CAMERA
W48, CROP = EV.W48, EV.CROP
GOLD = {"type": "conductor", "eta": 0.2, "k": 3.9, "specular_reflectance": 0.9}          # `uniform` spectra: constants over the wavelengths
GOLD_RGB = {"type": "conductor", "eta": (0.2, 0.92, 1.1), "k": (3.9, 2.45, 2.14), "specular_reflectance": (0.9, 0.8, 0.7)}
POINT = (0.7, 2.5, 0.4)
INTENSITY = (30.0, 24.0, 18.0)
SKY = {"radiance": (0.5, 0.6, 0.8)}
LAMP = [(0.5, 10, -0.5), (0.5, 10, 0.5), (-0.5, 10, 0.5), (-0.5, 10, -0.5)]                   # test_envmap's: wound to face down


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def point_spec(position=POINT, intensity=INTENSITY, **kw):
    return dict({"position": position, "intensity": intensity}, **kw)


def plane(hm, bsdf=None, flip=False, rot=None, name="plane"):
    """test_envmap's plane (50 x 50 through the origin, facing +y), optionally wound the other way round and / or rotated"""
    m = EV.plane_meshes(hm, bsdf)[0]
    m.name = name
    quad = [tuple(float(x) for x in (np.asarray(rot, np.float64) @ np.asarray(v, np.float64) if rot is not None else v)) for v in m.faces[0]]
    m.faces = [tuple(reversed(quad)) if flip else tuple(quad)]
    return m


# ===================================================================================================== CPU
def test_restatement_checks_itself():
    """(1) fp32 against float64 on random inputs, and the hand-checked values"""
    rng = np.random.RandomState(11)
    pos = np.array([0.5, -1.25, 2.0])
    p = (pos + rng.uniform(-2, 2, (4096, 3))).astype(F)
    inten = rng.uniform(0.1, 50, (4096, 4)).astype(F)
    d32, v32 = D.point_sample32(pos, p, inten)
    d64, v64 = D.point_sample64(pos.astype(F), p, inten)
    # d = position - p cancels: its absolute error is one rounding of the operands' size (|coordinates| <= 4), the rest is relative
    dist = d64[:, 3]
    assert np.all(np.abs(d32[:, 3] - dist) <= 2.0 ** -22 * 4 + 2.0 ** -22 * dist)
    rel = (2.0 ** -22 * 4) / dist + 2.0 ** -21
    assert np.all(np.abs(d32[:, :3] - d64[:, :3]) <= 2 * rel[:, None])
    assert np.all(np.abs(v32 - v64) <= 4 * rel[:, None] * v64)
    # straight above at distance 2: d = (0, 1, 0) and value = I / 4, exactly
    d, v = D.point_sample32((1.0, 3.0, -2.0), np.array([(1.0, 1.0, -2.0)], F), np.array([(8.0, 3.0, 0.5, 1e-3)], F))
    assert d.tolist() == [[0.0, 1.0, 0.0, 2.0]] and v.tolist() == [[2.0, 0.75, 0.125, float(F(1e-3) / F(4))]]
    d, v = D.point_sample32((1.0, 3.0, -2.0), np.array([(1.0, 3.0, -2.0)], F), np.ones((1, 4), F))
    assert not d.any() and not v.any()                                  # the position itself
    # the conductor: the defaults are a perfect mirror, exactly
    one, zero = np.ones((3, 4), F), np.zeros((3, 4), F)
    c = np.array([1.0, 0.5, 2.0 ** -12], F)
    assert np.array_equal(D.conductor_sample32(c, zero, one, one), one)
    assert not D.conductor_sample32(np.array([0.0, -0.5, -1.0], F), zero, one, one).any()
    cs = np.concatenate([rng.uniform(0, 1, 4093), [1.0, 0.5, 2.0 ** -12]]).astype(F)
    assert np.all(D.conductor_sample32(cs, np.zeros((4096, 4), F), np.ones((4096, 4), F), np.ones((4096, 4), F)) == 1.0)
    # gold-like constants against radiometry_ref.fresnel_conductor
    eta, k, spec = np.full((4096, 4), 0.2, F), np.full((4096, 4), 3.9, F), np.full((4096, 4), 0.9, F)
    got = D.conductor_sample32(cs, eta, k, spec).astype(np.float64)
    want = float(F(0.9)) * R.fresnel_conductor(cs.astype(np.float64), float(F(0.2)), float(F(3.9)))
    assert np.all(np.abs(got[:, 0] - want) <= 2e-6 * want)
    assert np.allclose(D.conductor_sample64(cs, eta, k, spec)[:, 0], want, rtol=1e-12)
    eta, k = rng.uniform(0.1, 3, (4096, 4)).astype(F), rng.uniform(0.5, 5, (4096, 4)).astype(F)
    got, want = D.conductor_sample32(cs, eta, k, spec).astype(np.float64), D.conductor_sample64(cs, eta, k, spec)
    assert np.all(np.abs(got - want) <= 1e-5 * want + 1e-7)             # (random constants: cancellation in a^2 + b^2 +- t at grazing angles)


def test_layout_and_exports(abi, tmp_path):
    """(2)"""
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msk_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d %d %zu %zu %d\\n",'
                   'sizeof(msk_point_desc),offsetof(msk_point_desc,emitter),offsetof(msk_point_desc,position),'
                   'sizeof(msk_scene_ext),offsetof(msk_scene_ext,n_points),offsetof(msk_scene_ext,points),MSK_BSDF_CONDUCTOR,MSK_EMITTER_POINT,'
                   'sizeof(msk_emitter_desc),sizeof(msk_bsdf_desc),MSK_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    p, e = abi.PointDesc, abi.SceneExt
    assert got == [C.sizeof(p), p.emitter.offset, p.position.offset, C.sizeof(e), e.n_points.offset, e.points.offset, abi.MSK_BSDF_CONDUCTOR,
                   abi.MSK_EMITTER_POINT, C.sizeof(abi.EmitterDesc), C.sizeof(abi.BsdfDesc), abi.MSK_ABI_VERSION]
    assert got[:8] == [16, 0, 4, 24, 8, 16, 4, 3]
    assert got[8:] == [28, 132, 8]                                      # what they were before this feature
    import __graft_entry__ as ge
    ge.build_gpu_library()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("msk_gpu_scene_create_ext", "msk_gpu_point_sample", "msk_gpu_conductor_sample"):
        assert name in abi.EXPORTS and getattr(lib, name) is not None
    blob = open(abi.LIB_PATH, "rb").read()
    for k in (b"k_shade_gen_p", b"k_wavefront_p", b"k_wavefront_h_p", b"k_path_serial_p", b"k_delta_probe"):
        assert k in blob, k


def flattener_meshes(hm):
    lamp = hm.MeshSpec("lamp", [tuple(LAMP)], hm.LUMINAIRE, radiance=(40, 30, 20))
    return [plane(hm, dict(GOLD_RGB, twosided=True), name="mirror2"), lamp, plane(hm, GOLD, rot=np.diag([1.0, 1.0, 1.0]), name="mirror1"),
            plane(hm, {"type": "conductor"}, name="defaults")]


def test_the_two_flatteners_agree(hostmirror, abi, tmp_path):
    """(3) two point lights, an area light, a `twosided` conductor, a one-sided one and one with every default, the point lights
    before and behind the shapes: the same descriptors byte for byte, emitter indices in XML order"""
    hostlib = EV.host_library()
    for order, firsts in (("behind", (False, False)), ("mixed", (True, False))):
        pts = [point_spec((1.5, 2.0, -3.0), (3.0, 2.0, 1.0), first=firsts[0]), point_spec((-4.0, 6.0, 0.25), 2.5, scale=2.0, first=firsts[1])]
        d = tmp_path / order
        xml = hostmirror.write_scene_xml(flattener_meshes(hostmirror), str(d), 16, 16, 1, camera=CAM, points=pts)
        text = open(xml).read()
        assert text.count('<emitter type="point">') == 2 and text.count('<bsdf type="conductor">') == 3 and text.count('<bsdf type="twosided">') == 1
        h = hostlib.HostScene(xml).flatten()
        m = hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, points=pts, coeff_lookup=hostlib.srgb_model_fetch)
        assert h.desc.n_emitters == m.desc.n_emitters == 3 and h.desc.n_bsdfs == m.desc.n_bsdfs == 4
        types = [m.desc.emitters[i].type for i in range(3)]
        assert types == ([abi.MSK_EMITTER_POINT, abi.MSK_EMITTER_AREA, abi.MSK_EMITTER_POINT] if firsts[0] else [abi.MSK_EMITTER_AREA, abi.MSK_EMITTER_POINT, abi.MSK_EMITTER_POINT])
        for i in range(3):
            assert bytes(h.desc.emitters[i]) == bytes(m.desc.emitters[i]), (order, i)
        for i in range(4):
            assert bytes(h.desc.bsdfs[i]) == bytes(m.desc.bsdfs[i]), (order, i)
        assert h.points is not None and len(h.points) == len(m.points) == 2
        assert bytes(h.points) == bytes(m.points)
        assert [p.emitter for p in m.points] == ([0, 2] if firsts[0] else [1, 2])
        assert [list(p.position) for p in m.points] == [[1.5, 2.0, -3.0], [-4.0, 6.0, 0.25]]
        b = m.desc.bsdfs
        assert [b[i].type for i in range(4)] == [abi.MSK_BSDF_CONDUCTOR, abi.MSK_BSDF_DIFFUSE, abi.MSK_BSDF_CONDUCTOR, abi.MSK_BSDF_CONDUCTOR]
        assert [b[i].back_bsdf for i in range(4)] == [0, -1, -1, -1]
        assert list(b[3].eta.coeff) == [0, 0, np.inf] and (b[3].eta.scale, b[3].k.scale, b[3].specular_reflectance.scale) == (0.0, 1.0, 1.0)
        assert b[0].eta.scale == F(2.2) and b[2].k.scale == F(3.9)      # an rgb above 1: 2 max; a uniform spectrum: its value
        # the second light: <spectrum value="5"/> inside an emitter is D65 * 5
        e2 = m.desc.emitters[2]
        assert list(e2.radiance) == [0, 0, np.inf] and e2.d65_scale == F(F(5) * (F(1) / F(10568))) and e2.mesh_id == -1
    # to_world instead of position: its translation
    tw = np.eye(4)
    tw[:3, 3] = (1.5, 2.0, -3.0)
    pts = [{"to_world": tw, "intensity": (3.0, 2.0, 1.0)}]
    xml = hostmirror.write_scene_xml(flattener_meshes(hostmirror), str(tmp_path / "tw"), 16, 16, 1, camera=CAM, points=pts)
    h = hostlib.HostScene(xml).flatten()
    m = hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, points=pts, coeff_lookup=hostlib.srgb_model_fetch)
    assert bytes(h.points) == bytes(m.points) and list(m.points[0].position) == [1.5, 2.0, -3.0]
    # both: refused by both
    both = [dict(pts[0], position=(0, 1, 0))]
    with pytest.raises(ValueError) as e:
        hostmirror.flatten(flattener_meshes(hostmirror), 16, 16, camera=CAM, points=both)
    assert '"position" and "to_world"' in str(e.value)
    xml = hostmirror.write_scene_xml(flattener_meshes(hostmirror), str(tmp_path / "both"), 16, 16, 1, camera=CAM, points=both)
    with pytest.raises(hostlib.HostError) as e:
        hostlib.HostScene(xml).flatten()
    assert '"position" and "to_world"' in str(e.value)
    # a texture that varies over the surface under the conductor: refused loudly
    text = open(xml).read().replace('<point name="position" x="0" y="1" z="0"/>', "")
    tex = '<texture name="eta" type="checkerboard"><rgb name="color0" value="0.1"/><rgb name="color1" value="0.2"/></texture>'
    head, tail = text.rsplit('<bsdf type="conductor">', 1)            # the last conductor: the one that names no parameter
    (tmp_path / "both" / "tex.xml").write_text(head + '<bsdf type="conductor">' + tex + tail)
    with pytest.raises(hostlib.HostError) as e:
        hostlib.HostScene(str(tmp_path / "both" / "tex.xml")).flatten()
    assert "conductor" in str(e.value) and "eta" in str(e.value)
    with pytest.raises(ValueError):
        hostmirror.flatten([plane(hostmirror, {"type": "conductor", "eta": {"type": "checkerboard"}})], 16, 16, camera=CAM)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("launch_plan_delta") / "launch_plan_delta_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out, os.path.join(ROOT, "tests", "native", "launch_plan_delta_check.cpp")])
    return out


@pytest.mark.parametrize("knobs", LP.KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_plan_with_a_delta_light_or_mirror(plan_exe, knobs):
    """(4) has_delta selects SHADE_DELTA everywhere and changes nothing else; without it the plan is what it was"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs)
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.split() == ["cases", str(7 * 128 * 4 * len(LP.REGION_SIZES) * len(LP.LDS))]


def test_stale_record_would_be_off_by_per_cents():
    """closed form (c), from the float64 side: what path.cpp's stale next-event record would make of the sky's part (module docstring)"""
    c, w = R.gauss_legendre(64)
    p_l, p_b = 1.0 / (8.0 * np.pi), c / np.pi
    a = float((w * 2.0 * c * p_l ** 2 / (p_l ** 2 + p_b ** 2)).sum())          # integral over the hemisphere of cos / pi * w_l = integral of 2 c w_l dc
    assert abs(a - np.log(65.0) / 64.0) < 1e-9
    assert 0.03 < a / 2 < 0.035                                           # +3.26 % on rho L, against a bound of 6 standard errors (at most 3 %) + 0.1 %


# ----------------------------------------------------------------------------- float64 expectations
def crop_rays(desc, m=4):
    t, w = R.gauss_legendre(m)
    yy, xx = np.meshgrid(CROP[1] + 8 * t, CROP[0] + 8 * t, indexing="ij")
    o, d = R.camera_ray(desc, xx, yy)
    return o, d, w[:, None] * w[None, :]


def rho_over_pi(desc, b=0):
    bd = desc.bsdfs[b]
    return D.sigmoid_spectrum(bd.reflectance[:], bd.reflectance_scale / np.pi)


def cie_of(desc):
    return np.array(desc.cie1931_xyz[:285], np.float64)


def point_on_plane(desc, position, normal=(0, 1, 0), m=4):
    """the mean over the crop of cos(theta) / d^2 at the plane through the origin"""
    o, d, w = crop_rays(desc, m)
    n = np.asarray(normal, np.float64)
    if o @ n < 0:
        n = -n                                                           # the face the camera sees
    return float((w * D.point_geometry(R.hit_plane(o, d, (0, 0, 0), n), n, position)).sum())


def mirror_fresnel(desc, m=4, b=0):
    o, d, w = crop_rays(desc, m)
    bd = desc.bsdfs[b]
    return float((w * R.fresnel_conductor(-d[..., 1], float(bd.eta.scale), float(bd.k.scale))).sum()) * float(bd.specular_reflectance.scale)


WALL_Z, LAMP_E = -6.0, (1.0, 4.0, -2.0)


def mirror_lamp_meshes(hm):
    wall = hm.MeshSpec("wall", [((-30.0, 0.0, WALL_Z), (30.0, 0.0, WALL_Z), (30.0, 30.0, WALL_Z), (-30.0, 30.0, WALL_Z))], (0.6, 0.5, 0.4))      # faces +z
    return [plane(hm, GOLD), wall]


def mirror_lamp_expected(desc, m=4):
    """(e) F(cos_i) * spec * rho / pi * I * cos(theta) / d^2 at the wall point the mirror shows"""
    o, d, w = crop_rays(desc, m)
    x0 = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
    d1 = D.reflect(d, (0, 1, 0))
    t = (WALL_Z - x0[..., 2]) / d1[..., 2]
    x1 = x0 + d1 * t[..., None]
    assert np.all(t > 0) and np.all(x1[..., 1] > 0) and np.all(x1[..., 1] < 30) and np.all(np.abs(x1[..., 0]) < 30)
    bd = desc.bsdfs[0]
    f = R.fresnel_conductor(-d[..., 1], float(bd.eta.scale), float(bd.k.scale)) * float(bd.specular_reflectance.scale)
    g = float((w * f * D.point_geometry(x1, (0, 0, 1), LAMP_E)).sum())
    return R.expected_xyz(D.emitter_spectrum(desc, 0) * rho_over_pi(desc, 1), cie_of(desc)) * g


SKEW_N = EV.skew_rotation().astype(np.float64) @ np.array([0.0, 1.0, 0.0])


def closed_form_case(hm, name):
    """-> (flat, expectation at 4 x 4 nodes, the same at 8 x 8)"""
    if name in ("a_plane", "a_twosided_rotated"):
        if name == "a_plane":
            meshes, n, pos = [plane(hm)], (0, 1, 0), POINT
        else:       # wound so that the camera sees its BACK: the twosided adapter flips wi and wo
            meshes, n = [plane(hm, {"type": "diffuse", "twosided": True}, flip=True, rot=EV.skew_rotation())], SKEW_N
            pos = tuple(float(x) for x in 2.5 * SKEW_N + np.array([0.6, 0.0, 0.3]))
            assert np.array(CAM["origin"]) @ SKEW_N > 0 and np.array(pos) @ SKEW_N > 0
        flat = hm.flatten(meshes, W48, W48, camera=CAM, points=[point_spec(pos)])
        s = D.emitter_spectrum(flat.desc, 0) * rho_over_pi(flat.desc)
        return flat, *(R.expected_xyz(s, cie_of(flat.desc)) * point_on_plane(flat.desc, pos, n, m) for m in (4, 8))
    if name in ("b_point_first", "b_point_last"):
        first = name == "b_point_first"
        lamp = hm.MeshSpec("lamp", [tuple(LAMP)], hm.LUMINAIRE, radiance=(40, 30, 20))
        flat = hm.flatten([plane(hm), lamp], W48, W48, camera=CAM, points=[point_spec(first=first)])
        ip, ia = (0, 1) if first else (1, 0)
        assert flat.desc.n_emitters == 2 and flat.desc.emitters[ip].type == 3 and flat.points[0].emitter == ip
        out = []
        for m in (4, 8):
            o, d, w = crop_rays(flat.desc, m)
            lamp_g = float((w * R.polygon_irradiance(R.hit_plane(o, d, (0, 0, 0), (0, 1, 0)), (0, 1, 0), np.array(LAMP, np.float64))).sum())
            pg = point_on_plane(flat.desc, POINT, m=m)
            i_s, l_s = D.emitter_spectrum(flat.desc, ip), D.emitter_spectrum(flat.desc, ia)
            s = R.Spectrum(lambda lam, pg=pg, lamp_g=lamp_g: i_s(lam) * pg + l_s(lam) * lamp_g, i_s.breaks) * rho_over_pi(flat.desc)
            out.append(R.expected_xyz(s, cie_of(flat.desc)))
        return flat, out[0], out[1]
    if name == "c_point_and_sky":
        flat = hm.flatten([plane(hm)], W48, W48, camera=CAM, env=SKY, points=[point_spec()])
        assert flat.desc.emitters[0].type == 1 and flat.desc.emitters[1].type == 3
        out = []
        for m in (4, 8):
            pg = point_on_plane(flat.desc, POINT, m=m)
            i_s, l_s = D.emitter_spectrum(flat.desc, 1), D.emitter_spectrum(flat.desc, 0)
            s = R.Spectrum(lambda lam, pg=pg: i_s(lam) * pg + l_s(lam) * np.pi, i_s.breaks) * rho_over_pi(flat.desc)
            out.append(R.expected_xyz(s, cie_of(flat.desc)))
        return flat, out[0], out[1]
    if name == "d_mirror_under_sky":
        flat = hm.flatten([plane(hm, GOLD)], W48, W48, camera=CAM, env=SKY)
        sky = R.expected_xyz(D.emitter_spectrum(flat.desc, 0), cie_of(flat.desc))
        return flat, sky * mirror_fresnel(flat.desc, 4), sky * mirror_fresnel(flat.desc, 8)
    if name == "e_mirror_then_lamp":
        flat = hm.flatten(mirror_lamp_meshes(hm), W48, W48, camera=CAM, points=[point_spec(LAMP_E, (300.0, 240.0, 180.0))])
        return flat, mirror_lamp_expected(flat.desc, 4), mirror_lamp_expected(flat.desc, 8)
    raise KeyError(name)


CASES = ["a_plane", "a_twosided_rotated", "b_point_first", "b_point_last", "c_point_and_sky", "d_mirror_under_sky", "e_mirror_then_lamp"]


@pytest.mark.parametrize("name", CASES)
def test_expectations_have_converged(hostmirror, name):
    """the 4 x 4 Gauss-Legendre rule over the crop against 8 x 8: far inside the 1e-3 the bound allows"""
    _, e4, e8 = closed_form_case(hostmirror, name)
    print("DELTA %s: expectation %s (8 x 8 nodes: %s)" % (name, e4, e8))
    assert np.all(e4 > 0) and np.all(np.abs(e4 - e8) <= 1e-5 * e8)


def film_weights(desc, size, m):
    """test_envmap.expected_film_xyz's weighting: the filter weight a sample at a film position leaves inside the film, against the
    polynomial through an m x m Gauss-Legendre grid -> (nodes, weights a with sum_jk a_j a_k v(t_j, t_k) = the film's expectation, effective
    samples / samples)"""
    x, wx = EV.film_row_weights(desc, size)
    n_eff = (wx.mean() ** 2 / (wx * wx).mean()) ** 2
    t, _ = R.gauss_legendre(m, 0.0, float(size))
    return t, (wx @ EV.lagrange(t, x)) / wx.sum(), n_eff


FILM_POINT = (0.5, 7.0, -1.0)          # higher than POINT: cos / d^2 stays a low-order polynomial over the WHOLE film


def film_case(hm, name, m=10):
    """(8) the 32 x 32 film: (flat, expectation of sum XYZ / sum W, effective samples / samples)"""
    if name == "a_plane":
        flat = hm.flatten([plane(hm)], 32, 32, camera=CAM, points=[point_spec(FILM_POINT, (200.0, 160.0, 120.0))])
        unit = R.expected_xyz(D.emitter_spectrum(flat.desc, 0) * rho_over_pi(flat.desc), cie_of(flat.desc))
        value = lambda o, d: D.point_geometry(R.hit_plane(o, d, (0, 0, 0), (0, 1, 0)), (0, 1, 0), FILM_POINT)
    else:
        flat = hm.flatten([plane(hm, GOLD)], 32, 32, camera=CAM, env=SKY)
        bd = flat.desc.bsdfs[0]
        unit = R.expected_xyz(D.emitter_spectrum(flat.desc, 0), cie_of(flat.desc)) * float(bd.specular_reflectance.scale)
        value = lambda o, d: R.fresnel_conductor(-d[..., 1], float(bd.eta.scale), float(bd.k.scale))
    t, a, n_eff = film_weights(flat.desc, 32, m)
    yy, xx = np.meshgrid(t, t, indexing="ij")
    o, d = R.camera_ray(flat.desc, xx, yy)
    return flat, unit * float(np.einsum("j,k,jk->", a, a, value(o, d))), n_eff


@pytest.mark.parametrize("name", ["a_plane", "d_mirror_under_sky"])
def test_film_expectations_have_converged(hostmirror, name):
    _, fine, n_eff = film_case(hostmirror, name, 14)
    _, coarse, _ = film_case(hostmirror, name, 10)
    print("DELTA film %s: fine %s coarse %s effective samples / samples %.4f" % (name, fine, coarse, n_eff))
    assert np.all(np.abs(coarse - fine) <= 2e-4 * fine) and 0.8 < n_eff < 1.0


# ===================================================================================================== GPU: the probes
def conductor_probe_meshes(hm):
    return [plane(hm, {"type": "conductor"}, name="c0"), plane(hm, GOLD, name="c1"), plane(hm, dict(GOLD_RGB, twosided=True), name="c2")]


def probe_inputs():
    """-> (the first point light's position, reference points float32[4096, 3]: around it, along 13 directions at distances
    2^-10 .. 2^10 and the position itself; wavelengths float32[4096, 4]; cos_theta_i float32[4096] over [-1, 1] with the edges)"""
    rng = np.random.RandomState(23)
    pos = np.array([0.75, 2.5, -1.25], F)
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 1), (-1, 1, 1), (1, 1, 1), (-1, -1, -1), (0, 1, -1), (3, -2, 1)]
    far = [pos.astype(np.float64) + np.array(d, np.float64) / np.linalg.norm(d) * 2.0 ** k for k in range(-10, 11) for d in dirs][:255]
    p = np.concatenate([pos + rng.uniform(-2, 2, (3840, 3)), far, [pos]]).astype(F)
    assert p.shape == (4096, 3) and np.array_equal(p[-1], pos)
    wl = rng.uniform(360, 830, (4096, 4)).astype(F)
    cos = np.concatenate([np.linspace(-1, 1, 4089), [0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0, 2.0 ** -12, 0.5]]).astype(F)
    return pos, p, wl, cos


PROBE_POINT_2 = (5.0, 1.0, 1.0)


def probe_flat(hostmirror, pos):
    """the probes' scene: three conductor planes, a lamp (emitter 0) and two point lights (emitters 1 and 2)"""
    lamp = hostmirror.MeshSpec("lamp", [tuple(LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))
    pts = [point_spec(tuple(pos), INTENSITY), point_spec(PROBE_POINT_2, 3.0)]
    return hostmirror.flatten(conductor_probe_meshes(hostmirror) + [lamp], 16, 16, camera=CAM, points=pts)


@pytest.mark.gpu
def test_probes_equal_the_restatement_bit_for_bit(gpu_ctx, hostmirror, oracle, abi):
    """(5) msk_gpu_point_sample and msk_gpu_conductor_sample run the device functions the shading kernels call; no case excluded"""
    pos, p, wl, cos = probe_inputs()
    flat = probe_flat(hostmirror, pos)
    d = flat.desc
    assert [d.emitters[i].type for i in range(3)] == [0, 3, 3]
    _, d65 = hostmirror.cie_tables()
    g = abi.Scene(gpu_ctx, flat)
    try:
        for e, position in ((1, pos), (2, np.array(PROBE_POINT_2, F))):
            gd, gv = g.point_sample(e, p, wl)
            ed = d.emitters[e]
            inten = D.intensity32(oracle, ed.radiance[:], (d65 * F(ed.d65_scale)).astype(F), wl)
            rd, rv = D.point_sample32(position, p, inten)
            for what, a, b in (("d, dist", gd, rd), ("value", gv, rv)):
                bad = (bits(a) != bits(b)).reshape(len(a), -1).any(-1)
                assert not bad.any(), (e, what, int(bad.sum()), a[bad][:3], b[bad][:3], p[bad][:3])
            assert np.all(np.isfinite(gd)) and np.all(np.isfinite(gv))
        assert not gpu_zero_row(g.point_sample(1, p[-1:], wl[-1:]))      # the position itself: zeros
        for b in range(3):
            gv = g.conductor_sample(b, cos, wl)
            bd = d.bsdfs[b]
            rv = D.conductor_sample32(cos, D.spectrum32(oracle, bd.eta, wl), D.spectrum32(oracle, bd.k, wl), D.spectrum32(oracle, bd.specular_reflectance, wl))
            bad = (bits(gv) != bits(rv)).any(-1)
            assert not bad.any(), (b, int(bad.sum()), cos[bad][:4], gv[bad][:2], rv[bad][:2])
            assert not gv[~(cos > 0)].any() and np.all(gv[cos > 0] > 0)
        assert np.all(g.conductor_sample(0, cos, wl)[cos > 0] == 1.0)     # the defaults: a perfect mirror
        for call, text in ((lambda: g.point_sample(0, p[:1], wl[:1]), "emitter 0 is not a point emitter"), (lambda: g.point_sample(3, p[:1], wl[:1]), "emitter 3 is not a point emitter"),
                           (lambda: g.conductor_sample(3, cos[:1], wl[:1]), "bsdf 3 is not a conductor"), (lambda: g.conductor_sample(4, cos[:1], wl[:1]), "bsdf 4 is not a conductor")):
            with pytest.raises(abi.MskError) as err:
                call()
            assert text in str(err.value) and err.value.code == abi.MSK_ERR_INVALID_ARG
    finally:
        g.close()


def gpu_zero_row(out):
    return bool(np.asarray(out[0]).any() or np.asarray(out[1]).any())


# ===================================================================================================== GPU: the old kernels in the new family
def with_trailing_conductor(hm, abi, flat):
    """the same scene with one more entry in `bsdfs` that no mesh names: a default conductor"""
    d = flat.desc
    extra = hm._bsdf_desc(hm.MeshSpec("unused", [], 0.5, bsdf={"type": "conductor"}), None, d.n_bsdfs)
    arr = (abi.BsdfDesc * (d.n_bsdfs + 1))(*([d.bsdfs[i] for i in range(d.n_bsdfs)] + [extra]))
    flat.keep.append(arr)
    d.bsdfs, d.n_bsdfs = arr, d.n_bsdfs + 1
    return flat


def parity_scenes(hm):
    import test_dielectric_parity as DP
    return {"cbox": lambda: hm.cbox_scene(48, 48), "glass": lambda: DP.blob_room(hm, 1.5, 48)}


@pytest.mark.gpu
@pytest.mark.parametrize("hide", [0, 1])
@pytest.mark.parametrize("scene", ["cbox", "glass"])
def test_new_kernels_are_the_old_ones_where_the_oracle_can_follow(gpu_ctx, oracle, hostmirror, abi, scene, hide):
    """(6) the Cornell box (and the glass-blob room of test_dielectric_parity) plus one unreferenced conductor entry runs
    k_shade_gen_p / k_wavefront_p / k_path_serial_p; its film is the oracle's film of the scene without the entry, bit for bit.
    That the new family ran is confirmed INDIRECTLY: msk_stats has no field that names a kernel family.  What is checked: the probe
    answers, and it answers only for a scene whose `has_delta` is set — the field scene_facts() hands to the plan, which then names
    SHADE_DELTA under every knob (test_plan_with_a_delta_light_or_mirror); and, for the Cornell box, bytes_shade is the general
    variant's.  A build that dropped has_delta between the scene and the plan would pass here (the old kernels make the oracle's
    film too) and fail the closed forms, whose scenes the old kernels cannot render."""
    plain = parity_scenes(hostmirror)[scene]()
    carrying = with_trailing_conductor(hostmirror, abi, parity_scenes(hostmirror)[scene]())
    o, g, g0 = oracle.scene(plain), abi.Scene(gpu_ctx, carrying), abi.Scene(gpu_ctx, plain)
    try:
        assert np.all(g.conductor_sample(carrying.desc.n_bsdfs - 1, np.array([0.5], F), np.full((1, 4), 550, F)) == 1.0)
        with pytest.raises(abi.MskError):
            g0.conductor_sample(0, np.array([0.5], F), np.full((1, 4), 550, F))
        for prm in (abi.render_params(spp=4, seed=3, hide_emitters=hide), EV.pcg(abi, spp=4, seed=3, hide_emitters=hide)):
            film, st = g.render(prm)
            ref, rst = o.render(prm, threads=8)
            _, st0 = g0.render(prm)
            assert st.samples == rst.samples == 48 * 48 * 4
            assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), (scene, hide, prm.rng_mode, float(np.abs(film - ref).max()))
            assert film[..., :3].max() > 0
            if prm.rng_mode == abi.MSK_RNG_COUNTER:
                assert (st.segments, st.shadow_rays) == (st0.segments, st0.shadow_rays)
                if scene == "cbox":      # msk_stats::bytes_shade: 16 B more per segment in the general variant than in the diffuse one the plain box runs
                    assert st.bytes_shade > st0.bytes_shade
    finally:
        g.close(); g0.close(); o.close()


# ===================================================================================================== GPU: closed forms
def sampled_mean_at(g, abi, what, expected, max_depth):
    """test_envmap.sampled_mean's procedure at another max_depth: spp doubles from 4096 until the standard error (from the per-sample
    values) is at most 0.5 % of the expectation, four doublings at the most"""
    spp = 4096
    for _ in range(5):
        xyz, _ = g.sample_pixels(abi.render_params(spp=spp, seed=7, max_depth=max_depth), EV.crop_pixels())
        v = xyz.reshape(-1, 3).astype(np.float64)
        mean, se = v.mean(0), v.std(0, ddof=1) / np.sqrt(len(v))
        print("DELTA %s max_depth %d spp %d: expected %s mean %s se/|E| %s dev/|E| %s" % (what, max_depth, spp, expected, mean, se / expected, (mean - expected) / expected))
        if np.all(se <= 5e-3 * expected):
            return mean, se
        spp *= 2
    raise AssertionError("the standard error stays above 0.5 %% of the expectation: %s" % (se / expected,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_rendered_radiance_meets_the_closed_form(gpu_ctx, hostmirror, abi, name):
    """(7 a-e) counter RNG through msk_gpu_sample_pixels: |mean - E| <= 6 standard errors + 1e-3 E per channel."""
    flat, expected, _ = closed_form_case(hostmirror, name)
    g = abi.Scene(gpu_ctx, flat)
    try:
        if name == "e_mirror_then_lamp":
            mean, se = sampled_mean_at(g, abi, name, expected, 3)
            xyz, _ = g.sample_pixels(abi.render_params(spp=64, seed=7, max_depth=2), EV.crop_pixels())
            assert not xyz.any()                                         # at max_depth = 2 the path ends on the wall, before its next-event sample
            assert np.all(mean > 0)                                      # next-event estimation resumes after the delta bounce
        else:
            mean, se, _ = EV.sampled_mean(g, abi, "DELTA " + name, expected)
        if name == "d_mirror_under_sky":     # a mirror plane under an open sky ends there: the same samples at any depth limit
            a, _ = g.sample_pixels(abi.render_params(spp=256, seed=7, max_depth=2), EV.crop_pixels())
            b, _ = g.sample_pixels(abi.render_params(spp=256, seed=7, max_depth=-1), EV.crop_pixels())
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and a.max() > 0
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)


@pytest.mark.gpu
def test_black_from_behind_and_from_below(gpu_ctx, hostmirror, abi):
    """(7 f) a one-sided conductor seen from behind, under a sky, and a point light below a one-sided diffuse plane: exactly 0, in
    both RNG modes"""
    behind = hostmirror.flatten([plane(hostmirror, GOLD, flip=True)], W48, W48, camera=CAM, env=SKY)
    below = hostmirror.flatten([plane(hostmirror)], W48, W48, camera=CAM, points=[point_spec((0.7, -2.5, 0.4))])
    front = hostmirror.flatten([plane(hostmirror, GOLD)], W48, W48, camera=CAM, env=SKY)
    for flat, black in ((behind, True), (below, True), (front, False)):
        g = abi.Scene(gpu_ctx, flat)
        xyz, _ = g.sample_pixels(abi.render_params(spp=64, seed=7), EV.crop_pixels())
        film, _ = g.render(EV.pcg(abi, spp=2, seed=7))
        g.close()
        rows = film[CROP[1]:CROP[1] + 8, CROP[0]:CROP[0] + 8, :3]
        assert np.isfinite(xyz).all() and np.isfinite(film).all()
        assert (not xyz.any() and not rows.any()) if black else (xyz.min() > 0 and rows.min() > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a_plane", "d_mirror_under_sky"])
def test_film_in_pcg_block_mode_meets_the_closed_form(gpu_ctx, hostmirror, abi, name):
    """(8) MSK_RNG_PCG_BLOCK (k_path_serial_p) through a 32 x 32 film, the bound and the standard error of
    test_envmap.test_film_in_pcg_block_mode_meets_the_quadrature"""
    flat, expected, n_eff = film_case(hostmirror, name)
    g = abi.Scene(gpu_ctx, flat)
    px = np.array([(x, y) for y in range(32) for x in range(32)], np.int32)
    xyz, _ = g.sample_pixels(abi.render_params(spp=64, seed=9, max_depth=2), px)
    sigma = np.sqrt(xyz.astype(np.float64).var(1, ddof=1).mean(0))
    spp = 256
    film, st = g.render(EV.pcg(abi, spp=spp, seed=7, max_depth=2))
    g.close()
    assert st.samples == 32 * 32 * spp
    f = film.astype(np.float64)
    mean = f[..., :3].sum((0, 1)) / f[..., 4].sum()
    se = sigma / np.sqrt(n_eff * st.samples)
    print("DELTA film %s: expected %s mean %s se/|E| %s dev/|E| %s effective samples / samples %.4f" % (name, expected, mean, se / expected, (mean - expected) / expected, n_eff))
    assert np.all(se <= 5e-3 * expected)
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected)


# ===================================================================================================== GPU: execution variants
KNOBS = EV.KNOBS + ("MSK_CAMERA_CULL", "MSK_TRACE_QUEUE")
LDS_VARIANTS = EV.LDS_VARIANTS + [({"MSK_CAMERA_CULL": "0"}, EV.ANY), ({"MSK_TRACE_QUEUE": "0"}, EV.ANY)]
HBM_VARIANTS = EV.HBM_VARIANTS + [({"MSK_LDS_SCENE_KB": "0", "MSK_CAMERA_CULL": "0"}, EV.ANY)]
BOX_POINT = point_spec((120.0, 420.0, 200.0), (4e5, 3e5, 2e5))


def box_meshes(hm, pads=(), mirror=True):
    """test_envmap's variant box (open Cornell box, area light, bitmap floor, glass ball) with a mirror ball"""
    ball = hm.blob_mesh("mirror", (170, 100, 330), 90, 6, 6, hm.WHITE, seed=4)
    if mirror:
        ball.bsdf = dict(GOLD_RGB)
    return EV.variant_meshes(hm, [ball] + list(pads))


def box_flat(hm, which, sky, mirror=True, light=True):
    env = EV.env_spec(EV.lit_image(), EV.skew_rotation(), scale=40.0) if sky == "envmap" else None
    pts = [BOX_POINT] if light else []
    if which == "lds":
        return hm.flatten(box_meshes(hm, mirror=mirror), 48, 48, env=env, points=pts)
    filler = hm.blob_mesh("filler", (150, 420, 400), 60, 16, 16, hm.WHITE, seed=9)
    base = hm.flatten(box_meshes(hm, [filler], mirror), 48, 48, env=env, points=pts)
    pads = T.faceless_pads(hm, T.SMALL_TABLES_F4 + 1 - T.table_plan(base)["small_f4"])
    return hm.flatten(box_meshes(hm, [filler] + pads, mirror), 48, 48, env=env, points=pts)


def test_variant_scenes_sit_where_the_tests_say(hostmirror, abi):
    for sky in ("none", "envmap"):
        lds, hbm = box_flat(hostmirror, "lds", sky), box_flat(hostmirror, "hbm", sky)
        pl, ph = T.table_plan(lds), T.table_plan(hbm)
        assert pl["lds_tables"] and pl["small_staged"]
        assert not ph["lds_tables"] and not ph["small_staged"] and ph["small_f4"] == T.SMALL_TABLES_F4 + 1
        d = lds.desc
        kinds = {d.bsdfs[i].type for i in range(d.n_bsdfs)}
        assert {abi.MSK_BSDF_CONDUCTOR, abi.MSK_BSDF_DIELECTRIC, abi.MSK_BSDF_DIFFUSE} <= kinds and d.n_textures == 1
        assert sorted(d.emitters[i].type for i in range(d.n_emitters)) == ([0, 2, 3] if sky == "envmap" else [0, 3])


@pytest.fixture(scope="module")
def variant_reference(gpu_ctx, hostmirror, abi):
    """the default variant's samples and films of the four scenes (no knob set): computed once, never changed"""
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
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
                assert np.isfinite(film).all() and film[..., :3].max() > 0
                out[sky, which] = dict(flat=flat, xyz=xyz, pos=pos, film=film, serial=serial, samples=st.samples)
    finally:
        os.environ.update(saved)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sky", ["none", "envmap"])
@pytest.mark.parametrize("which,env,expect", [("lds", e, x) for e, x in LDS_VARIANTS] + [("hbm", e, x) for e, x in HBM_VARIANTS],
                         ids=lambda v: EV.variant_id(v) if isinstance(v, dict) else str(v).replace(" ", "_"))
def test_every_execution_variant(gpu_ctx, abi, variant_reference, monkeypatch, which, env, expect, sky):
    """(9) films and samples byte-equal to the default variant's; msk_stats says which kernels made the film."""
    for k in KNOBS:
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
    print("DELTA variant %s %s %s: %s" % (sky, which, EV.variant_id(env), got))
    assert np.array_equal(gp.view(np.uint32), want["pos"].view(np.uint32))
    assert np.array_equal(gx.view(np.uint32), want["xyz"].view(np.uint32)), env
    assert np.array_equal(film.view(np.uint32), want["film"].view(np.uint32)), (env, float(np.abs(film - want["film"]).max()))
    assert np.array_equal(serial.view(np.uint32), want["serial"].view(np.uint32)), env
    assert st.samples == want["samples"]
    if expect == EV.SPLIT:
        assert st.launches_wavefront == 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == EV.FUSED_PART:
        assert st.launches_wavefront > 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == EV.FUSED_ALL:
        assert st.launches_wavefront > 0 and st.launches_shade == 0 and st.launches_trace == 0, got
    else:
        assert st.launches_shade > 0 and st.launches_trace > 0, got


# ===================================================================================================== GPU: refusals, group, aov
@pytest.mark.gpu
def test_gpu_rejects_bad_point_descriptors(gpu_ctx, hostmirror, abi):
    """(10) each MSK_ERR_INVALID_ARG case by its message, which names the emitter"""
    lamp = hostmirror.MeshSpec("lamp", [tuple(LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))

    def fresh():
        return hostmirror.flatten([plane(hostmirror), lamp], 16, 16, camera=CAM, points=[point_spec(), point_spec((1.0, 2.0, 3.0), 2.0)])

    def refused(flat, text, points=None, plain=False):
        with pytest.raises(abi.MskError) as e:
            if plain:
                h = C.c_void_p()
                gpu_ctx.check(gpu_ctx.lib.msk_gpu_scene_create(gpu_ctx.handle, C.byref(flat.desc), C.byref(h)))
            else:
                abi.Scene(gpu_ctx, flat, points=points)
        assert text in str(e.value), str(e.value)
        assert e.value.code == abi.MSK_ERR_INVALID_ARG
    flat = fresh()
    assert [flat.desc.emitters[i].type for i in range(3)] == [0, 3, 3] and [p.emitter for p in flat.points] == [1, 2]
    abi.Scene(gpu_ctx, flat).close()                                   # the scene itself is fine
    abi.Scene(gpu_ctx, flat, points=[flat.points[1], flat.points[0]]).close()      # ... in any order
    refused(fresh(), "emitter 1: a point emitter needs its position", plain=True)      # through plain msk_gpu_scene_create: refused, not defaulted
    refused(flat, "emitter 2: a point emitter needs its position", points=[flat.points[0]])      # a missing entry
    refused(flat, "emitter 1: a point emitter with two positions", points=[flat.points[0], flat.points[1], flat.points[0]])      # a doubled entry
    refused(flat, "emitter 0 is of type 0, not a point emitter", points=[flat.points[0], flat.points[1], abi.PointDesc(0, (C.c_float * 3)(0, 1, 0))])
    refused(flat, "emitter 7 out of range", points=[flat.points[0], flat.points[1], abi.PointDesc(7, (C.c_float * 3)(0, 1, 0))])
    for bad in (np.inf, -np.inf, np.nan):
        refused(flat, "emitter 2: a point emitter's position must be finite", points=[flat.points[0], abi.PointDesc(2, (C.c_float * 3)(0, bad, 0))])
    flat = fresh()
    flat.desc.emitters[1].mesh_id = 0
    refused(flat, "emitter 1: a point emitter has no mesh")
    # a conductor carries the neutral index of refraction: a descriptor of another kind with its type overwritten is refused
    flat = hostmirror.flatten([plane(hostmirror, GOLD)], 16, 16, camera=CAM)
    abi.Scene(gpu_ctx, flat).close()
    flat.desc.bsdfs[0].ior_eta = 1.5
    with pytest.raises(abi.MskError) as e:
        abi.Scene(gpu_ctx, flat)
    assert "bsdf 0: type 4 is not supported for a descriptor with a relative index of refraction" in str(e.value) and e.value.code == abi.MSK_ERR_INVALID_ARG
    flat.desc.bsdfs[0].ior_eta = flat.desc.bsdfs[0].ior_inv_eta = 0.0     # a zero-filled descriptor with the documented fields set: accepted
    abi.Scene(gpu_ctx, flat).close()
    # a scene without a point emitter takes no msk_point_desc
    none = hostmirror.flatten([plane(hostmirror), lamp], 16, 16, camera=CAM)
    refused(none, "emitter 0 is of type 0, not a point emitter", points=[abi.PointDesc(0, (C.c_float * 3)(0, 1, 0))])


@pytest.mark.gpu
def test_two_members_behind_one_context(abi, hostmirror):
    """(11) msk_gpu_init with n = 2 renders scene (b) to the single-device film bit for bit.  MSK_RNG_PCG_BLOCK on a 64 x 32 film:
    two blocks, one per member, and a pixel receives at most two blocks' contributions, whose sum does not depend on the
    order.  (A counter-mode call shards samples, and the members' partial sums re-associate: test_gpu_parity's criterion.)  The two
    members are devices 0 and 1 where there are two, and in any case device 0 twice (an ordinal may repeat)."""
    n_dev = C.c_int(0)
    assert abi.load_library().hipGetDeviceCount(C.byref(n_dev)) == 0
    lamp = hostmirror.MeshSpec("lamp", [tuple(LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))
    flat = hostmirror.flatten([plane(hostmirror), lamp], 64, 32, camera=CAM, points=[point_spec(first=True)])
    prm = EV.pcg(abi, spp=8, seed=5)
    with abi.Context(0) as one:
        s1 = abi.Scene(one, flat)
        ref, st1 = s1.render(prm)
        p1 = s1.point_sample(0, np.zeros((1, 3), F), np.full((1, 4), 550, F))
        s1.close()
    assert st1.samples == 64 * 32 * 8 and ref[..., :3].max() > 0
    for members in [(0, 0)] + ([(0, 1)] if n_dev.value >= 2 else []):
        with abi.Context(members) as grp:
            s2 = abi.Scene(grp, flat)
            film, st2 = s2.render(prm)
            p2 = s2.point_sample(0, np.zeros((1, 3), F), np.full((1, 4), 550, F))
            s2.close()
        assert st2.samples == st1.samples
        assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), (members, float(np.abs(film - ref).max()))
        assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])


@pytest.mark.gpu
def test_aov_geometric_channels(gpu_ctx, hostmirror, abi):
    """(12) msk_gpu_render_aov on the variant box: the geometric channels (and alpha, weight) are those of the same box with the
    conductor swapped for `diffuse` and the point light removed, bit for bit"""
    types = [abi.MSK_AOV_DEPTH, abi.MSK_AOV_POSITION, abi.MSK_AOV_UV, abi.MSK_AOV_GEO_NORMAL, abi.MSK_AOV_SH_NORMAL]
    prm = abi.render_params(spp=4, seed=5)
    films = []
    for mirror, light in ((True, True), (False, False)):
        g = abi.Scene(gpu_ctx, box_flat(hostmirror, "lds", "none", mirror=mirror, light=light))
        film, st = g.render_aov(prm, types)
        g.close()
        assert st.samples == 48 * 48 * 4 and film.shape == (48, 48, 5 + 12)
        films.append(film)
    assert np.array_equal(films[0][..., 3:].view(np.uint32), films[1][..., 3:].view(np.uint32))
    assert films[0][..., 5].max() > 0 and not films[0][..., :3].any()   # depth; without a nested path integrator XYZ is 0
