"""The `thinlens` sensor (include/msk_gpu.h at msk_lens_desc): depth of field from the aperture sample.

Correctness rests on three things here: the contract restated in numpy fp32 (lens_ref.py), which the probe must equal bit for bit;
per-sample float64 expectations (an in-focus edge is sharp, an out-of-focus edge blurs by the circular segment of the lens that sees
past it); and identities between kernels.  The oracle restates the lens too (oracle.cpp, D24): test_lens_light_oracle_parity.py holds
its twin to this file's restatement and float64 expectations (check_sharp, check_blur, run_lens_radiance and mix_expected take either
side) and the device to the twin bit for bit, on the very scenes and parameters of `variant_reference` below, so the anchor of
test_every_execution_variant is a film of the oracle's.

CPU: the restatement against float64; validation, layout and exports as a stand-alone native program, plain and sanitized; the two
flatteners; the launch plan.  GPU: probe = restatement; the sharp edge; the blurred edge; closed-form radiance through a lens under
"path" and "direct"; direct (1, 1) = path at max_depth 2; every execution variant makes the same film; shards; the position AOV of
the focus plane; a mask, a spot and an envmap under a lens; a group context; the plugin; refusals.
"""
import ctypes as C
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import delta_ref as D
import lens_ref as L
import light_ref as LR
import radiometry_ref as R
import test_delta_light_mirror as DM
import test_direct_integrator as DI
import test_envmap as EV
import test_launch_plan as LP
import test_radiometry_closed_form as RC
import test_spot_directional as SD
import test_table_placement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
bits = SD.bits

# the camera of the edge tests: at the origin, looking down +z
FOCUS, RADIUS = 5.0, 0.4
Z_CAM = dict(fov=40.0, near=0.01, far=100.0, origin=(0, 0, 0), target=(0, 0, 1), up=(0, 1, 0))
EDGE_COLUMN = 32.7                       # where the edge projects through the lens centre, in pixels of the 64 x 64 film
EDGE_PIXELS = np.array([(x, y) for y in range(64) for x in (31, 32, 33, 34)], np.int32)     # the four columns around it
MARGIN = 2.0 ** -17 * FOCUS              # see test_in_focus_it_is_sharp
# a camera in general position (the probe): no coordinate of its origin is zero
SKEW_CAM = dict(fov=35.0, near=0.05, far=500.0, origin=(1.5, 2.25, -6.5), target=(0.25, 0.5, 1.0), up=(0.1, 1.0, 0.05))


def lens_cam(cam, radius=None, focus=None):
    c = dict(cam)
    if radius is not None:
        c["aperture_radius"] = radius
    if focus is not None:
        c["focus_distance"] = focus
    return c


def with_lens(abi, flat, radius, focus):
    """the same flattened scene seen through a lens (abi.Scene picks flat.lens up)"""
    flat.lens = abi.LensDesc(float(F(radius)), float(F(focus)))
    return flat


def to_world64(desc):
    return np.array(desc.camera.to_world[:], np.float64).reshape(4, 4)


def focus_world64(desc, pos, focus):
    """float64: the world-space focus points of the film positions pos [..., 2]"""
    fp = L.focus_point64(desc, pos[..., 0], pos[..., 1], focus)
    m = to_world64(desc)
    return fp @ m[:3, :3].T + m[:3, 3]


def emitting_quad(hm, lo_x, hi_x, z, name="screen"):
    """an emitter of uniform radiance in the plane z, facing -z (the camera), over lo_x .. hi_x and |y| <= 20"""
    c, u, v = ((lo_x + hi_x) / 2, 0.0, z), (0.0, 20.0, 0.0), ((hi_x - lo_x) / 2, 0.0, 0.0)
    return hm.MeshSpec(name, [RC.quad(c, u, v)], 0.0, radiance=hm.Regular(360, 830, [1.0, 1.0]))


def edge_setup(hm, abi, z_e, radius=RADIUS):
    """-> (the scene whose screen fills the lit side of the edge in the plane z_e, the scene whose screen fills the view, x0 in that
    plane, +1 / -1 = the side of x the screen is on).  The edge's position in the focus plane, x0 f / z_e, is the focus point of
    column EDGE_COLUMN; the screen lies on the side of growing column numbers."""
    probe = hm.flatten([], 64, 64, camera=Z_CAM)
    fx = focus_world64(probe.desc, np.array([[EDGE_COLUMN, 32.0], [EDGE_COLUMN + 1.0, 32.0]]), FOCUS)[:, 0]
    side = 1.0 if fx[1] > fx[0] else -1.0
    x0 = float(F(fx[0] * z_e / FOCUS))                       # the mesh holds it as a float
    lo, hi = (x0, x0 + 20.0) if side > 0 else (x0 - 20.0, x0)
    edge = with_lens(abi, hm.flatten([emitting_quad(hm, lo, hi, z_e)], 64, 64, camera=Z_CAM), radius, FOCUS)
    full = with_lens(abi, hm.flatten([emitting_quad(hm, -20.0, 20.0, z_e)], 64, 64, camera=Z_CAM), radius, FOCUS)
    assert float(F(lo if side > 0 else hi)) == x0
    return edge, full, x0, side


# ===================================================================================================== CPU 1: the restatement
def test_restatement_against_float64(hostmirror, oracle):
    """(1) fp32 against float64: every ray passes through near_p f / near_p.z; lens points lie in the disk; the disk map preserves
    area on a grid of u; the pinhole's ray is the float64 camera ray of radiometry_ref"""
    rng = np.random.RandomState(3)
    n = 2048
    pos = rng.uniform(-2, 66, (n, 2)).astype(F)
    u = rng.uniform(0, 1, (n, 2)).astype(F)
    u[:8] = [(0.5, 0.5), (0, 0), (1 - 2.0 ** -24, 0), (0.25, 0.25), (0.25, 0.75), (0.5, 0.1), (0.9, 0.5), (0, 1 - 2.0 ** -24)]
    for cam, radius, focus in ((Z_CAM, 0.4, 5.0), (SKEW_CAM, 0.75, 9.0), (SKEW_CAM, 0.0, 3.0)):
        desc = hostmirror.flatten([], 64, 64, camera=cam).desc
        rays = L.camera_ray32(oracle, desc, pos, u, (radius, focus)).astype(np.float64)
        o, d = rays[:, :3], rays[:, 4:7]
        m = to_world64(desc)
        # the lens point: the origin in camera space lies in the disk of `radius` in the plane z = 0, at disk64(u) * radius
        oc = (o - m[:3, 3]) @ m[:3, :3]
        a = L.disk64(u.astype(np.float64)) * radius
        scale = np.abs(m[:3, 3]).max() + radius + 1
        assert np.all(np.abs(oc[:, 2]) <= 8 * 2.0 ** -24 * scale) and np.all(np.hypot(oc[:, 0], oc[:, 1]) <= radius * (1 + 2.0 ** -20) + 8 * 2.0 ** -24 * scale)
        assert np.all(np.abs(oc[:, :2] - a) <= 2.0 ** -20 * radius + 8 * 2.0 ** -24 * scale), float(np.abs(oc[:, :2] - a).max())
        # the ray passes through the focus point: the distance from it to the line o + t d
        fw = focus_world64(desc, pos.astype(np.float64), focus)
        v = fw - o
        dist = np.linalg.norm(v - d * (v * d).sum(-1, keepdims=True) / (d * d).sum(-1, keepdims=True), axis=-1)
        assert np.all(dist <= 32 * 2.0 ** -24 * (np.linalg.norm(fw, axis=-1) + scale)), float(dist.max())
        assert np.all(np.abs(np.linalg.norm(d, axis=-1) - 1) <= 4 * 2.0 ** -24)
        # tnear / tfar: the clip distances along the axis
        dz = d @ m[:3, 2]
        assert np.allclose(rays[:, 3] * dz, cam["near"], rtol=1e-6) and np.allclose(rays[:, 7] * dz, cam["far"], rtol=1e-6)
    # the pinhole
    desc = hostmirror.flatten([], 64, 64, camera=SKEW_CAM).desc
    rays = L.camera_ray32(oracle, desc, pos).astype(np.float64)
    o64, d64 = R.camera_ray(desc, pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64))
    assert np.all(np.abs(rays[:, :3] - o64) <= 2.0 ** -22 * np.abs(o64).max()) and np.all(np.abs(rays[:, 4:7] - d64) <= 8 * 2.0 ** -24)
    # the disk map preserves area: the image of every cell of a 32 x 32 grid of u has the area pi / 1024.  A cell's image is bounded
    # by arcs and radii; its outline is followed through 8 points per side, whose chords cut off at most (theta / 8)^2 / 6 of an arc's
    # sector, theta <= pi / 4 the widest angle a cell spans (the four cells at the centre): 1.6e-3.  The whole disk to 1e-3.
    n_c, sub = 32, 8
    g = np.arange(n_c * sub + 1) / (n_c * sub)
    uu = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    uu = np.minimum(uu, 1 - 2.0 ** -24).astype(F)
    p = L.disk32(oracle, uu).astype(np.float64).reshape(n_c * sub + 1, n_c * sub + 1, 2)
    assert np.all(np.hypot(p[..., 0], p[..., 1]) <= 1 + 2.0 ** -22)
    k = np.arange(sub)
    ring_i = np.concatenate([k, np.full(sub, sub), sub - k, np.zeros(sub, int)])          # a cell's outline, counter-clockwise in u
    ring_j = np.concatenate([np.zeros(sub, int), k, np.full(sub, sub), sub - k])
    ci, cj = np.meshgrid(np.arange(n_c) * sub, np.arange(n_c) * sub, indexing="ij")
    poly = p[ci[..., None] + ring_i, cj[..., None] + ring_j]                                # [32, 32, 32, 2]
    nxt = np.roll(poly, -1, axis=2)
    shoelace = 0.5 * np.abs((poly[..., 0] * nxt[..., 1] - nxt[..., 0] * poly[..., 1]).sum(-1))
    print("LENS disk map: cell areas / (pi / 1024) in [%.6f, %.6f], sum / pi %.6f" % (shoelace.min() / (np.pi / 1024), shoelace.max() / (np.pi / 1024), shoelace.sum() / np.pi))
    assert abs(shoelace.sum() / np.pi - 1) < 1e-3 and np.all(np.abs(shoelace / (np.pi / 1024) - 1) < 2e-3), (shoelace.sum(), shoelace.min(), shoelace.max())
    assert np.allclose(p, L.disk64(uu.astype(np.float64)).reshape(p.shape), atol=4 * 2.0 ** -24)
    # the circular segment: 1, 1/2, 0 and symmetric
    assert L.segment_fraction(np.array([-1.0, 0.0, 1.0])).tolist() == [1.0, 0.5, 0.0]
    h = np.linspace(-1, 1, 101)
    assert np.allclose(L.segment_fraction(h) + L.segment_fraction(-h), 1.0, atol=1e-15)
    # ... against the disk map itself: the share of a fine grid of u whose lens point has x > h
    fine = (np.stack(np.meshgrid(np.arange(512), np.arange(512), indexing="ij"), -1).reshape(-1, 2) + 0.5) / 512
    ax = L.disk64(fine)[:, 0]
    for hh in (-0.7, -0.2, 0.0, 0.35, 0.9):
        assert abs((ax > hh).mean() - L.segment_fraction(hh)) < 3e-3


# ===================================================================================================== CPU 2: the native program
@pytest.fixture(scope="module")
def native_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("lens_check")
    src = os.path.join(ROOT, "tests", "native", "lens_check.cpp")
    plain, san = str(d / "lens_check"), str(d / "lens_check_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src, "-ldl"])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src, "-ldl"])
    return plain, san


def test_native_validation_layout_exports(native_exe, abi):
    """(2) every bad descriptor is refused with its field's name and the tables of a scene with a lens, plain and sanitized; sizes and
    offsets against abi.py; the library exports the two new symbols (the plain executable: it loads the library)"""
    for exe in native_exe:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) > 50, r.stdout[-2000:] + r.stderr[-2000:]
        r = subprocess.run([exe, "layout"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        l, s = abi.LensDesc, abi.SceneLens
        assert [int(x) for x in r.stdout.split()] == [C.sizeof(l), l.aperture_radius.offset, l.focus_distance.offset, C.sizeof(s), s.lights.offset, s.lens.offset,
                                                      C.sizeof(abi.SceneLights), abi.MSK_ABI_VERSION]
    assert abi.MSK_ABI_VERSION == 8
    import __graft_entry__ as ge
    ge.build_gpu_library()
    r = subprocess.run([native_exe[0], "exports", abi.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["exports", "2"], r.stdout + r.stderr
    for name in ("msk_gpu_scene_create_lens", "msk_gpu_camera_sample"):
        assert name in abi.EXPORTS
    assert EV.host_library().load().msk_host_lens is not None


# ===================================================================================================== CPU 3: the two flatteners
def test_the_two_flatteners_agree(hostmirror, abi, tmp_path):
    """(3) an XML scene with a `thinlens` sensor: the same camera and lens descriptors byte for byte; focus_distance defaults to the
    far clip distance; a thinlens without aperture_radius is refused in the same words; a perspective sensor has no lens"""
    hostlib = EV.host_library()
    meshes = lambda: [DM.plane(hostmirror)]
    for k, cam in enumerate((lens_cam(SKEW_CAM, 0.125, 7.5), lens_cam(SKEW_CAM, 0.3), lens_cam(SKEW_CAM, 0.0, 2.0), SKEW_CAM)):
        xml = hostmirror.write_scene_xml(meshes(), str(tmp_path / ("s%d" % k)), 24, 16, 1, camera=cam)
        text = open(xml).read()
        assert ('<sensor type="thinlens">' in text) == ("aperture_radius" in cam) and ('<sensor type="perspective">' in text) != ("aperture_radius" in cam)
        assert ('name="focus_distance"' in text) == ("focus_distance" in cam)
        h = hostlib.HostScene(xml).flatten()
        m = hostmirror.flatten(meshes(), 24, 16, camera=cam, coeff_lookup=hostlib.srgb_model_fetch)
        assert bytes(h.desc.camera) == bytes(m.desc.camera)
        if "aperture_radius" not in cam:
            assert h.lens is None and m.lens is None
            continue
        assert h.lens is not None and m.lens is not None and bytes(h.lens) == bytes(m.lens)
        assert m.lens.aperture_radius == F(cam["aperture_radius"]) and m.lens.focus_distance == F(cam.get("focus_distance", cam["far"]))
    words = 'thinlens: the parameter "aperture_radius" must be specified!'
    with pytest.raises(ValueError) as e:
        hostmirror.flatten(meshes(), 24, 16, camera=lens_cam(SKEW_CAM, None, 4.0))
    assert words in str(e.value)
    xml = hostmirror.write_scene_xml(meshes(), str(tmp_path / "bad"), 24, 16, 1, camera=lens_cam(SKEW_CAM, 0.25, 4.0))
    text = open(xml).read()
    line = [l for l in text.splitlines() if 'name="aperture_radius"' in l]
    assert len(line) == 1
    open(xml, "w").write(text.replace(line[0] + "\n", ""))
    with pytest.raises(hostlib.HostError) as e:
        hostlib.HostScene(xml).flatten()
    assert words in str(e.value), str(e.value)


# ===================================================================================================== CPU 4: the plan
@pytest.mark.parametrize("knobs", LP.KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_plan_with_a_lens(native_exe, knobs):
    """(4) has_lens selects SHADE_LENS over every other family and changes nothing else; without it the plan is what it was"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs)
    r = subprocess.run([native_exe[0], "plan"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.split() == ["cases", str(7 * 512 * 4 * len(LP.REGION_SIZES) * len(LP.LDS))]


# ===================================================================================================== GPU 5: the probe
def probe_inputs():
    """4096 (film position, u) pairs: u on the diagonals, on the axes and at the centre of the square (the branches of the concentric
    map and its creases), at the square's corners and edges; the film's corners; random ones"""
    rng = np.random.RandomState(17)
    pos = rng.uniform(-2, 66, (4096, 2)).astype(F)
    u = rng.uniform(0, 1, (4096, 2)).astype(F)
    t = rng.uniform(0, 1, 256).astype(F)
    top = F(1 - 2.0 ** -24)
    u[0:256] = np.stack([t, t], -1)                                   # x == y
    u[256:512] = np.stack([t, (F(1) - t).astype(F)], -1)              # x == -y (where 1 - t is exact)
    u[512:768] = np.stack([t, np.full(256, 0.5, F)], -1)              # y == 0
    u[768:1024] = np.stack([np.full(256, 0.5, F), t], -1)             # x == 0
    u[1024:1034] = [(0.5, 0.5), (0, 0), (0, top), (top, 0), (top, top), (0, 0.5), (0.5, 0), (top, 0.5), (0.5, top), (0.25, 0.75)]
    pos[1034:1038] = [(0, 0), (64, 0), (0, 64), (64, 64)]
    pos[1038:1042] = [(32, 32), (0.5, 63.5), (-2, -2), (66, 66)]
    return pos, u


@pytest.mark.gpu
@pytest.mark.parametrize("cam", ["z", "skew"])
def test_probe_equals_the_restatement(gpu_ctx, hostmirror, oracle, abi, cam):
    """(5) bit for bit: a lens, R = 0, and the pinhole (which ignores u); with R = 0 the origin is the pinhole's"""
    camera = Z_CAM if cam == "z" else SKEW_CAM
    pos, u = probe_inputs()
    mesh = lambda: [emitting_quad(hostmirror, -1.0, 1.0, 4.0)]
    pin = hostmirror.flatten(mesh(), 64, 64, camera=camera)
    g = abi.Scene(gpu_ctx, pin)
    got_pin = g.camera_sample(pos)
    got_pin_u = g.camera_sample(pos, u)
    g.close()
    want_pin = L.camera_ray32(oracle, pin.desc, pos)
    assert np.array_equal(bits(got_pin), bits(want_pin)), int((bits(got_pin) != bits(want_pin)).any(-1).sum())
    assert np.array_equal(bits(got_pin_u), bits(got_pin))
    for radius, focus in ((0.4, 5.0), (2.5, 0.75), (0.0, 5.0)):
        flat = hostmirror.flatten(mesh(), 64, 64, camera=lens_cam(camera, radius, focus))
        g = abi.Scene(gpu_ctx, flat)
        got = g.camera_sample(pos, u)
        with pytest.raises(abi.MskError) as e:
            g.camera_sample(pos)
        assert e.value.code == abi.MSK_ERR_INVALID_ARG and "aperture_u" in str(e.value)
        g.close()
        want = L.camera_ray32(oracle, flat.desc, pos, u, (radius, focus))
        bad = (bits(got) != bits(want)).any(-1)
        assert not bad.any(), (radius, focus, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2], want[bad][:2])
        assert np.isfinite(got).all()
        if radius == 0.0:
            if cam == "skew":
                assert np.array_equal(bits(got[:, :3]), bits(got_pin[:, :3]))          # bit for bit: no coordinate of the origin is zero
            assert np.array_equal(got[:, :3], got_pin[:, :3])                          # as numbers, always
            assert np.all(np.abs(got[:, 4:7].astype(np.float64) - got_pin[:, 4:7]) <= 4 * 2.0 ** -24)
        else:
            assert not np.array_equal(got[:, :3], got_pin[:, :3])


# ===================================================================================================== GPU 6: in focus it is sharp
def check_sharp(make_scene, hostmirror, abi):
    """(6) An emitting screen fills the side x > x0 of the focus plane z = f; x0 projects to column 32.7.  max_depth = 1: emission
    only.  The same seed on a screen that fills the view gives every sample's lit value W_i (the radiance is uniform, the value is a
    function of the sample's wavelengths alone).  Every sample is all zeros or W_i, bit for bit, and it is lit exactly when the focus
    point of its film position is on the lit side.

    Left out: samples whose focus point lies within m = 2^-17 f of x0.  The ray meets the plane z = f at o.x + t d.x: about thirty
    rounded operations on values of magnitude at most f (the contract's steps 2-6 and the triangle test), each with a relative error
    of 2^-24, so an absolute error below 30 * 2^-24 * f = 2^-19 f: m is four times that.  The cap on what is left out, 0.5 %, is
    asserted first, from the film positions alone (m is 7e-4 of a pixel's width: 0.03 % of four columns)."""
    edge, full, x0, side = edge_setup(hostmirror, abi, FOCUS)
    prm = abi.render_params(spp=64, seed=21, max_depth=1)
    ge, gf = make_scene(edge), make_scene(full)
    try:
        xyz, pos = ge.sample_pixels(prm, EDGE_PIXELS)
        w, wpos = gf.sample_pixels(prm, EDGE_PIXELS)
    finally:
        ge.close(); gf.close()
    assert np.array_equal(bits(pos), bits(wpos)) and np.all(w > 0)
    fx = focus_world64(edge.desc, pos.astype(np.float64), FOCUS)[..., 0]
    out = np.abs(fx - x0) < MARGIN
    print("LENS sharp: %d samples, %d left out (%.4f %%)" % (out.size, int(out.sum()), 100.0 * out.mean()))
    assert out.mean() <= 5e-3
    lit = xyz.any(-1)
    same = (bits(xyz) == bits(w)).all(-1)
    assert np.all(lit == same) and np.all(lit | (bits(xyz) == 0).all(-1)), "a sample is neither all zeros nor its lit value"
    want = side * (fx - x0) > 0
    wrong = (lit != want) & ~out
    assert not wrong.any(), (int(wrong.sum()), fx[wrong][:4], x0)
    assert 0.3 < lit.mean() < 0.7                                  # the edge runs through the four columns


@pytest.mark.gpu
def test_in_focus_it_is_sharp(gpu_ctx, hostmirror, abi):
    """(6) check_sharp on the device"""
    check_sharp(lambda flat: abi.Scene(gpu_ctx, flat), hostmirror, abi)


# ===================================================================================================== GPU 7: out of focus it blurs
BLUR_DEPTHS = [0.6, 1.6]


def check_blur(make_scene, hostmirror, abi, depth):
    """(7) the screen at z_e = 0.6 f and 1.6 f.  Sample i is lit with probability p_i, the share of the lens disk whose ray towards the
    focus point F passes the edge: a.x (1 - z_e / f) + F.x z_e / f > x0, a circular segment (lens_ref.lit_fraction, float64).
    |sum(lit_i) - sum(p_i)| <= 5 sqrt(sum p_i (1 - p_i)) + the change of sum(p_i) when x0 moves by +- m (test 6's m).  2^16 samples."""
    z_e = depth * FOCUS
    edge, full, x0, side = edge_setup(hostmirror, abi, z_e)
    prm = abi.render_params(spp=256, seed=23, max_depth=1)
    ge, gf = make_scene(edge), make_scene(full)
    try:
        xyz, pos = ge.sample_pixels(prm, EDGE_PIXELS)
        w, _ = gf.sample_pixels(prm, EDGE_PIXELS)
    finally:
        ge.close(); gf.close()
    lit = xyz.any(-1)
    assert lit.size == 1 << 16
    assert np.all((bits(xyz) == bits(w)).all(-1) == lit) and np.all(lit | (bits(xyz) == 0).all(-1))
    fx = focus_world64(edge.desc, pos.astype(np.float64), FOCUS)[..., 0]
    p = lambda edge_x: L.lit_fraction(side * fx, side * edge_x, RADIUS, z_e, FOCUS)      # (mirrored when the screen is on the side of falling x)
    p0 = p(x0)
    partly = ((p0 > 0) & (p0 < 1)).mean()
    spread = 5.0 * np.sqrt((p0 * (1 - p0)).sum())
    shift = abs(p(x0 + MARGIN).sum() - p(x0 - MARGIN).sum())
    dev = abs(float(lit.sum()) - p0.sum())
    print("LENS blur z_e = %.1f f: lit %d expected %.1f dev %.1f (%.2f sigma) tol %.1f + %.3f; partly covered lens: %.1f %% of the samples"
          % (depth, int(lit.sum()), p0.sum(), dev, dev / (spread / 5), spread, shift, 100 * partly))
    assert partly > 0.5, "most samples must see a partly covered lens"
    assert dev <= spread + shift
    # and the blur is there: column by column the lit share follows the mean of p, where a sharp edge would give 0 or 1
    share = lit.reshape(64, 4, -1).mean((0, 2))
    want = p0.reshape(64, 4, -1).mean((0, 2))
    assert np.all(np.abs(share - want) < 0.02) and np.all((want > 0.02) & (want < 0.98)), (share, want)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", BLUR_DEPTHS)
def test_out_of_focus_it_blurs_by_the_right_amount(gpu_ctx, hostmirror, abi, depth):
    """(7) check_blur on the device"""
    check_blur(lambda flat: abi.Scene(gpu_ctx, flat), hostmirror, abi, depth)


# ===================================================================================================== GPU 8: radiance
LENS_SIGMA = os.path.join(HERE, "golden", "lens_sigma.json")
# (case of test_radiometry_closed_form, aperture radius, focus distance): scenes whose radiance towards the camera is the same from
# every point of the lens.  The plate fills the pixels' view from every lens point (asserted); the furnace's radiance is the same
# everywhere inside the cube (the lens, radius 0.1 around (0.3, -0.2, -0.6), is inside).
RADIANCE_CASES = {"S4_diffuse_uniform": (0.05, 20.0), "S3_cube_rho0.5_depth3_rr5": (0.1, 1.2)}


def run_lens_radiance(name, side, hm, abi, direct):
    """test_radiometry_closed_form.run_sampled with a lens over the scene and, for `direct`, msk_gpu_sample_pixels_direct at (1, 1).
    The same expectation, sigma, sample counts, tolerance and cap (1e-3 |E| in Y) — except the furnace under "direct", which is "path"
    at max_depth 2: its expectation is the same closed form at that depth, R.furnace(le, rho, 2), and its sigma is measured on the
    oracle's `direct` (tests/golden/make_lens_sigma.py -> lens_sigma.json), as radiometry_sigma.json was.  The plate's path never goes
    beyond depth 2 (a convex scene: the bounce ray leaves it), so its `direct` is its "path"."""
    case = RC.CASES[name](hm)
    radius, focus = RADIANCE_CASES[name]
    with_lens(abi, case.flat, radius, focus)
    sigma = RC.load_sigma(name)
    e, q = RC.expectation(case)
    if direct and name.startswith("S3_"):
        entry = json.load(open(LENS_SIGMA))[name + "_direct"]
        assert entry["samples"] >= 1 << 20
        sigma = np.asarray(entry["sigma"], np.float64)
        cie, _ = RC.tables(case.flat.desc)
        radiance = R.regular(*RC.ONE) * R.constant(0.5).map(lambda r: R.furnace(1.0, r, 2))
        e, e1 = R.expected_xyz(radiance, cie, 16)[None], R.expected_xyz(radiance, cie, 8)[None]
        q = np.abs(e - e1)
        assert np.all(q <= RC.Q_MAX * np.abs(e))
    if name.startswith("S4_"):
        # every ray of the pixels, from every point of the lens' rim, meets the plate
        desc = case.flat.desc
        px = np.array([(x + dx, y + dy) for x, y in RC.S4_PIXELS for dx in (0.0, 1.0) for dy in (0.0, 1.0)])
        fw = focus_world64(desc, px, focus)
        m = to_world64(desc)
        for ang in np.linspace(0, 2 * np.pi, 16, endpoint=False):
            o = m[:3, 3] + radius * (np.cos(ang) * m[:3, 0] + np.sin(ang) * m[:3, 1])
            d = fw - o
            x = R.hit_plane(o, d / np.linalg.norm(d, axis=-1, keepdims=True), (0, 0, 0), (0, 1, 0))
            assert np.abs(x).max() < 1.0
    per_pixel = max(-(-RC.samples_needed(sigma[g], e[g], q[g], side.caps) // len(idx)) for g, idx in enumerate(case.groups))
    spp = side.max_spp
    if side.max_records:                                                 # (as run_sampled: the CPU side has no such limit)
        spp = min(spp, 1 << int(np.log2(side.max_records // len(case.pixels))))
    spp = min(spp, 1 << int(np.ceil(np.log2(per_pixel))))
    n_seeds = -(-per_pixel // spp)
    seed0 = zlib.crc32((name + ("direct" if direct else "lens")).encode()) << 8
    sc = side.scene(case.flat)
    try:
        assert sc.lens is not None
        sums = np.zeros((len(case.pixels), 3))
        for k in range(n_seeds):
            prm = abi.render_params(spp, seed=seed0 + k, **case.params)
            xyz = sc.sample_pixels_direct(prm, case.pixels, 1, 1)[0] if direct else sc.sample_pixels(prm, case.pixels)[0]
            sums += np.add.reduce(xyz, axis=1, dtype=np.float64)
    finally:
        sc.close()
    n = np.array([len(idx) * n_seeds * spp for idx in case.groups])
    mean = np.stack([sums[idx].sum(0) / n[g] for g, idx in enumerate(case.groups)])
    RC.compare(name + (" lens direct" if direct else " lens path"), side, mean, n, sigma, e, q)


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True], ids=["path", "direct"])
@pytest.mark.parametrize("name", sorted(RADIANCE_CASES))
def test_a_lens_does_not_change_radiance(gpu_ctx, hostmirror, abi, name, direct):
    """(8) a plate in a constant environment and a furnace (bounces), through a lens with R > 0"""
    run_lens_radiance(name, RC.GpuSide(gpu_ctx, abi), hostmirror, abi, direct)


def test_lens_sigma_is_what_the_generator_measures():
    """the recorded sigma of the furnace under `direct` lies below the furnace's at max_depth 3 and above (1 + rho) / (1 + rho +
    rho^2) = 6 / 7 of it less 10 %: one bounce fewer"""
    d = np.asarray(json.load(open(LENS_SIGMA))["S3_cube_rho0.5_depth3_rr5_direct"]["sigma"])
    p = RC.load_sigma("S3_cube_rho0.5_depth3_rr5")
    assert d.shape == p.shape and np.all(d < p) and np.all(d > 0.9 * 6 / 7 * p), (d, p)


# ===================================================================================================== GPU 9: kernels agree
BOX_LENS = (25.0, 1100.0)                # in the Cornell box's units: the lens, and the distance of the box's middle


def box_flat(hm, abi, which, sky, size=(48, 48), camera=None, lens=BOX_LENS):
    """test_spot_directional's variant box (open Cornell box: area light, spot, sun, bitmap floor, glass and mirror balls) through
    a lens; `camera` replaces the Cornell camera"""
    env = EV.env_spec(EV.lit_image(), EV.skew_rotation(), scale=40.0) if sky == "envmap" else None
    lights = [SD.BOX_SPOT, SD.BOX_SUN]
    kw = dict(env=env, lights=lights, camera=camera)
    if which == "lds":
        flat = hm.flatten(SD.box_meshes(hm), size[0], size[1], **kw)
    else:
        filler = hm.blob_mesh("filler", (150, 420, 400), 60, 16, 16, hm.WHITE, seed=9)
        base = hm.flatten(SD.box_meshes(hm, [filler]), size[0], size[1], **kw)
        pads = T.faceless_pads(hm, T.SMALL_TABLES_F4 + 1 - T.table_plan(base)["small_f4"])
        flat = hm.flatten(SD.box_meshes(hm, [filler] + pads), size[0], size[1], **kw)
    return with_lens(abi, flat, *lens) if lens else flat


@pytest.mark.gpu
@pytest.mark.parametrize("hide", [0, 1])
def test_direct_one_one_is_path_at_depth_two(gpu_ctx, hostmirror, abi, hide):
    """(9) spot, sun, area light and envmap through a lens: samples, film positions and films as bits"""
    g = abi.Scene(gpu_ctx, box_flat(hostmirror, abi, "lds", "envmap", size=(DI.FW, DI.FH)))
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
    # and the lens is in it: the pinhole's samples are others
    g = abi.Scene(gpu_ctx, box_flat(hostmirror, abi, "lds", "envmap", size=(DI.FW, DI.FH), lens=None))
    pin, ppos = g.sample_pixels(prm, DI.all_pixels())
    g.close()
    assert np.array_equal(bits(ppos), bits(wpos)) and not np.array_equal(bits(pin), bits(want))


WIDE_CAMERA = dict(fov=75.0, near=10.0, far=2800.0, origin=(278, 273, -800), target=(278, 273, -799), up=(0, 1, 0))      # sees past the box


@pytest.fixture(scope="module")
def variant_reference(gpu_ctx, hostmirror, abi):
    """the default variant's samples and films of the two scenes (no knob set): computed once, never changed.  The camera sees past
    the box: part of the camera rays miss the scene's bounds (asserted on the probe's rays), so the camera cull has work"""
    saved = {k: os.environ.pop(k) for k in DM.KNOBS if k in os.environ}
    out = {}
    try:
        for which in ("lds", "hbm"):
            flat = box_flat(hostmirror, abi, which, "none", camera=WIDE_CAMERA)
            g = abi.Scene(gpu_ctx, flat)
            rng = np.random.RandomState(5)
            rays = g.camera_sample(rng.uniform(0, 48, (4096, 2)).astype(F), rng.uniform(0, 1, (4096, 2)).astype(F)).astype(np.float64)
            lo, hi = flat.vertices[:, :3].min(0).astype(np.float64), flat.vertices[:, :3].max(0).astype(np.float64)
            pad = 1e-3 * np.linalg.norm(hi - lo)
            with np.errstate(divide="ignore"):
                t0, t1 = (lo - pad - rays[:, :3]) / rays[:, 4:7], (hi + pad - rays[:, :3]) / rays[:, 4:7]
            miss = np.minimum(t0, t1).max(-1) > np.maximum(t0, t1).min(-1)
            assert 0.1 < miss.mean() < 0.8, miss.mean()
            xyz, pos = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
            film, st = g.render(abi.render_params(spp=8, seed=5))
            g.close()
            for a in (xyz, pos, film):
                a.setflags(write=False)
            assert np.isfinite(film).all() and film[..., :3].max() > 0 and (film[..., 4] > 0).all() and (film[..., :3].sum(-1) == 0).any()
            out[which] = dict(flat=flat, xyz=xyz, pos=pos, film=film, samples=st.samples)
    finally:
        os.environ.update(saved)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which,env,expect", [("lds", e, x) for e, x in DM.LDS_VARIANTS] + [("hbm", e, x) for e, x in DM.HBM_VARIANTS],
                         ids=lambda v: EV.variant_id(v) if isinstance(v, dict) else str(v).replace(" ", "_"))
def test_every_execution_variant(gpu_ctx, abi, variant_reference, monkeypatch, which, env, expect):
    """(9) films and samples byte-equal to the default variant's (the anchors are the tests above, not this one); msk_stats says which
    kernels made the film"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = variant_reference[which]
    g = abi.Scene(gpu_ctx, want["flat"])
    gx, gp = g.sample_pixels(abi.render_params(spp=16, seed=5), EV.crop_pixels())
    film, st = g.render(abi.render_params(spp=8, seed=5))
    g.close()
    got = "trace %d shade %d wavefront %d" % (st.launches_trace, st.launches_shade, st.launches_wavefront)
    print("LENS variant %s %s: %s" % (which, EV.variant_id(env), got))
    assert np.array_equal(bits(gp), bits(want["pos"]))
    assert np.array_equal(bits(gx), bits(want["xyz"])), env
    assert np.array_equal(bits(film), bits(want["film"])), (env, float(np.abs(film - want["film"]).max()))
    assert st.samples == want["samples"]
    if expect == EV.SPLIT:
        assert st.launches_wavefront == 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == EV.FUSED_PART:
        assert st.launches_wavefront > 0 and st.launches_shade > 0 and st.launches_trace > 0, got
    elif expect == EV.FUSED_ALL:
        assert st.launches_wavefront > 0 and st.launches_shade == 0 and st.launches_trace == 0, got
    else:
        assert st.launches_shade > 0 and st.launches_trace > 0, got


def film_sum_bound(film, spp, border=2):
    """Two fp32 sums of the same positive addends in different orders: each is within n 2^-24 of the exact sum, n the number of addends
    of a film pixel, at most spp (2 border + 1)^2; |X|, |Y|, |Z| are bounded by their own sums since every addend is >= 0"""
    return 2.0 * spp * (2 * border + 1) ** 2 * 2.0 ** -24 * np.abs(film)


@pytest.mark.gpu
def test_the_film_is_the_sum_of_two_sample_shards(gpu_ctx, abi, variant_reference, monkeypatch):
    """(9) shards (0, 2) and (1, 2) of the samples: another order of summation, so not bits; the bound is film_sum_bound's"""
    for k in DM.KNOBS:
        monkeypatch.delenv(k, raising=False)
    want = variant_reference["lds"]
    g = abi.Scene(gpu_ctx, want["flat"])
    half = [g.render(abi.render_params(spp=8, seed=5, sample_first=r, sample_stride=2)) for r in (0, 1)]
    g.close()
    assert half[0][1].samples == half[1][1].samples == 48 * 48 * 4
    total = half[0][0].astype(np.float64) + half[1][0]
    assert np.all(np.abs(total - want["film"]) <= film_sum_bound(want["film"], 8) + 1e-30)
    assert not np.array_equal(bits(half[0][0]), bits(half[1][0]))


# ===================================================================================================== GPU 10: aov
@pytest.mark.gpu
def test_position_aov_of_the_focus_plane(gpu_ctx, hostmirror, abi):
    """(10) a plane at z = f: every lens ray of a film position meets it at that position's focus point, so the position AOV's film
    through the lens is the pinhole's.  Bound per sample and coordinate: both rays reach the point through at most 64 rounded operations
    (the contract's steps, the triangle test, the interaction's point from the barycentrics) on values of magnitude at most
    M = |focus point| + R <= 6.5, so each is within 64 * 2^-24 * M of the exact point and they differ by at most 2^-17 M.  A film
    value is the sum of w_i p_i over the same weights on both sides: the difference is at most W * 2^-17 M, W the pixel's weight sum,
    plus film_sum_bound's rounding of the two sums (|p| <= M).  The depth AOV likewise, with the ray's length in M's place."""
    pin = hostmirror.flatten([emitting_quad(hostmirror, -20.0, 20.0, FOCUS)], 48, 48, camera=Z_CAM)
    lens = with_lens(abi, hostmirror.flatten([emitting_quad(hostmirror, -20.0, 20.0, FOCUS)], 48, 48, camera=Z_CAM), RADIUS, FOCUS)
    prm = abi.render_params(spp=16, seed=9)
    films = []
    for flat in (pin, lens):
        g = abi.Scene(gpu_ctx, flat)
        films.append(g.render_aov(prm, [abi.MSK_AOV_POSITION, abi.MSK_AOV_DEPTH])[0].astype(np.float64))
        g.close()
    a, b = films
    assert a.shape == (48, 48, 9) and np.array_equal(a[..., 4], b[..., 4]) and (a[..., 4] > 0).all()
    m = 6.5
    w = a[..., 4:5]
    tol = w * 2.0 ** -17 * m + 2.0 * 16 * 25 * 2.0 ** -24 * w * m
    assert np.all(np.abs(a[..., 5:8] - b[..., 5:8]) <= tol), float((np.abs(a[..., 5:8] - b[..., 5:8]) / tol).max())
    assert np.all(np.abs(a[..., 7] / a[..., 4] - FOCUS) <= 2.0 ** -17 * m)                        # z = f everywhere
    # the depth is NOT the pinhole's: a lens ray starts off the axis.  It lies between f and the length from the rim
    depth_l, depth_p = b[..., 8] / b[..., 4], a[..., 8] / a[..., 4]
    assert np.all(depth_p >= FOCUS * (1 - 1e-6)) and np.all(depth_l >= FOCUS * (1 - 1e-6)) and np.all(depth_l <= np.hypot(FOCUS, np.hypot(2.2, 2.2) + RADIUS))
    assert np.abs(depth_l - depth_p).max() > 1e-4


# ===================================================================================================== GPU 11: everything else
MIX_CAM = dict(fov=30.0, near=0.1, far=1000.0, origin=(0, 6, 0), target=(0, 0, 0), up=(0, 0, 1))      # straight down on the plane y = 0
MIX_LENS = (0.5, 6.0)                    # focused on the plane
MIX_ALPHA = 0.75
MIX_SKY = (0.5, 0.4, 0.3)
MIX_SPOT = SD.spot_spec((3.0, 0.0, 0.25), 60.0, 25.0, origin=(1.0, 3.0, -0.5), intensity=(30.0, 24.0, 18.0))
MIX_BLOCK = (20, 20)


def mix_flats(hm):
    """a diffuse plane under a constant mask of opacity 0.75, a spot and an envmap of one colour (the image emitter's code with the
    constant sky's radiance: test_envmap.test_uniform_image_is_the_constant_sky), seen straight from above through a lens focused on
    it; and the same scene with the `constant` emitter of that colour, whose descriptor the float64 expectation reads"""
    def meshes():
        p = DM.plane(hm)
        p.bsdf = {"type": "mask", "opacity": MIX_ALPHA, "bsdf": {"type": "diffuse"}}
        return [p]
    img = np.broadcast_to(np.array(MIX_SKY, F), (3, 4, 3))
    fe = hm.flatten(meshes(), 48, 48, camera=lens_cam(MIX_CAM, *MIX_LENS), env=EV.env_spec(img, EV.skew_rotation()), lights=[MIX_SPOT])
    fc = hm.flatten(meshes(), 48, 48, camera=MIX_CAM, env={"radiance": MIX_SKY}, lights=[MIX_SPOT])
    return fe, fc


def mix_expected(fe, fc, m):
    """The plane is the focus plane: every lens ray of a film position meets it at the pinhole ray's point x, and everything it sees
    there is the same from every direction: a (rho / pi) (I G(x) + pi c) + (1 - a) c per wavelength, G the spot's cos / d^2 times its
    cone factor, c the sky (in front of the plane for the diffuse lobe, behind it for the null lobe).  G's mean over the block by an
    m x m Gauss-Legendre rule."""
    types = [fc.desc.emitters[i].type for i in range(fc.desc.n_emitters)]
    spot_e, sky_e = types.index(4), types.index(1)
    pos, axis, cc, cb = SD.light_of(fc, spot_e)
    t, w = R.gauss_legendre(m)
    yy, xx = np.meshgrid(MIX_BLOCK[1] + 8 * t, MIX_BLOCK[0] + 8 * t, indexing="ij")
    o, d = R.camera_ray(fc.desc, xx, yy)
    x = R.hit_plane(o, d, (0, 0, 0), (0, 1, 0))
    c = LR.spot_cosine64(x, pos, axis)
    assert np.all((c > cc) & (c < cb)), "the block lies in the cone's transition zone"
    g = float(((w[:, None] * w[None, :]) * LR.spot_geometry(x, (0, 1, 0), pos, axis, cc, cb)).sum())
    spot, sky, rho = D.emitter_spectrum(fc.desc, spot_e), D.emitter_spectrum(fc.desc, sky_e), DM.rho_over_pi(fc.desc)
    s = R.Spectrum(lambda lam: MIX_ALPHA * rho(lam) * (spot(lam) * g + sky(lam) * np.pi) + (1 - MIX_ALPHA) * sky(lam), spot.breaks)
    return R.expected_xyz(s, DM.cie_of(fc.desc))


def test_mix_expectation_has_converged(hostmirror):
    fe, fc = mix_flats(hostmirror)
    assert fe.lens is not None and fe.masks is not None and fe.lights is not None and fe.envmap is not None and fc.lens is None
    assert abs(np.linalg.norm(np.array(MIX_CAM["origin"])) - MIX_LENS[1]) == 0
    e4, e8 = mix_expected(fe, fc, 4), mix_expected(fe, fc, 8)
    print("LENS mix: expectation %s (8 x 8 nodes: %s)" % (e4, e8))
    assert np.all(e4 > 0) and np.all(np.abs(e4 - e8) <= 1e-5 * e8)


@pytest.mark.gpu
def test_a_lens_over_mask_spot_and_envmap(gpu_ctx, hostmirror, abi):
    """(11) the top tier carries the rest: test_spot_directional's criterion (spp doubles from 4096 until the standard error is at most
    0.5 % of the expectation; |mean - E| <= 6 se + 1e-3 E per channel)"""
    fe, fc = mix_flats(hostmirror)
    expected = mix_expected(fe, fc, 4)
    g = abi.Scene(gpu_ctx, fe)
    try:
        sample = lambda spp, px: g.sample_pixels(abi.render_params(spp=spp, seed=7), px)[0]
        mean, se = SD.sampled_mean(sample, "lens over mask, spot, envmap", expected, SD.block_pixels(MIX_BLOCK))
        film, st = g.render(abi.render_params(spp=4, seed=7))
    finally:
        g.close()
    assert np.all(np.abs(mean - expected) <= 6 * se + 1e-3 * expected), ((mean - expected) / expected, se / expected)
    assert np.isfinite(film).all() and st.samples == 48 * 48 * 4


@pytest.mark.gpu
def test_two_members_behind_one_context(abi, hostmirror):
    """(11) msk_gpu_init with n = 2: the lens reaches every member (the members shard the samples: the film is the single-device film
    up to the order of summation, film_sum_bound), and the probe answers through the group"""
    n_dev = C.c_int(0)
    assert abi.load_library().hipGetDeviceCount(C.byref(n_dev)) == 0
    lamp = hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))
    flat = hostmirror.flatten([DM.plane(hostmirror), lamp], 64, 32, camera=lens_cam(EV.PLANE_CAMERA, 0.3, 8.5))
    pin = hostmirror.flatten([DM.plane(hostmirror), lamp], 64, 32, camera=EV.PLANE_CAMERA)
    prm = abi.render_params(spp=8, seed=5)
    pos, u = probe_inputs()
    with abi.Context(0) as one:
        s1 = abi.Scene(one, flat)
        ref, st1 = s1.render(prm)
        r1 = s1.camera_sample(pos, u)
        s1.close()
        s0 = abi.Scene(one, pin)
        ref_pin, _ = s0.render(prm)
        s0.close()
    assert st1.samples == 64 * 32 * 8 and ref[..., :3].max() > 0
    blur = np.abs(ref.astype(np.float64) - ref_pin)
    assert (blur > 4 * film_sum_bound(ref, 8)).any()                                   # the lens changes the film by more than the bound below
    for members in [(0, 0)] + ([(0, 1)] if n_dev.value >= 2 else []):
        with abi.Context(members) as grp:
            s2 = abi.Scene(grp, flat)
            film, st2 = s2.render(prm)
            r2 = s2.camera_sample(pos, u)
            s2.close()
        assert st2.samples == st1.samples
        assert np.all(np.abs(film.astype(np.float64) - ref) <= film_sum_bound(ref, 8) + 1e-30), members
        assert np.array_equal(bits(r1), bits(r2))


@pytest.mark.gpu
def test_the_plugin_renders_a_thinlens_sensor(gpu_ctx, hostmirror, abi, tmp_path):
    """(11) <sensor type="thinlens"> through the C++ plugin: the film msk_gpu_render makes of the plugin's own flattened scene, bit for bit"""
    hostlib = EV.host_library()
    lamp = hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))
    xml = hostmirror.write_scene_xml([DM.plane(hostmirror), lamp], str(tmp_path / "lens"), 32, 24, 4, camera=lens_cam(EV.PLANE_CAMERA, 0.3, 8.5))
    hs = hostlib.HostScene(xml)
    film, _, st = hs.render()
    flat = hs.flatten()
    assert flat.lens is not None and flat.lens.aperture_radius == F(0.3)
    g = abi.Scene(gpu_ctx, flat)
    ref, rst = g.render(flat.params)
    g.close()
    hs.close()
    assert st.samples == rst.samples == 32 * 24 * 4 and ref[..., :3].max() > 0
    assert np.array_equal(bits(film), bits(ref))


@pytest.mark.gpu
def test_gpu_refusals(gpu_ctx, hostmirror, abi):
    """(11) bad descriptors are refused on the device path, with the field's name; MSK_RNG_PCG_BLOCK is refused with its message; the
    older entry points make a pinhole scene"""
    lamp = hostmirror.MeshSpec("lamp", [tuple(DM.LAMP)], hostmirror.LUMINAIRE, radiance=(40, 30, 20))
    flat = hostmirror.flatten([DM.plane(hostmirror), lamp], 16, 16, camera=EV.PLANE_CAMERA)
    for radius, focus, field in ((-1.0, 5.0, "aperture_radius"), (np.nan, 5.0, "aperture_radius"), (np.inf, 5.0, "aperture_radius"), (-np.inf, 5.0, "aperture_radius"),
                                 (0.5, 0.0, "focus_distance"), (0.5, -2.0, "focus_distance"), (0.5, np.inf, "focus_distance"), (0.5, np.nan, "focus_distance")):
        with pytest.raises(abi.MskError) as e:
            abi.Scene(gpu_ctx, flat, lens=abi.LensDesc(radius, focus))
        assert e.value.code == abi.MSK_ERR_INVALID_ARG and field in str(e.value) and "msk_lens_desc" in str(e.value), str(e.value)
    g = abi.Scene(gpu_ctx, flat, lens=abi.LensDesc(0.0, 5.0))                         # R = 0 is valid
    for prm in (EV.pcg(abi, spp=2, seed=5),):
        with pytest.raises(abi.MskError) as e:
            g.render(prm)
        assert e.value.code == abi.MSK_ERR_UNSUPPORTED and "thinlens" in str(e.value) and "MSK_RNG_PCG_BLOCK" in str(e.value), str(e.value)
    film, st = g.render(abi.render_params(spp=2, seed=5))
    g.close()
    assert np.isfinite(film).all() and st.samples == 16 * 16 * 2
    # a NULL lens through the new entry is the older entry: the same film as bits, and MSK_RNG_PCG_BLOCK renders
    eln = abi.SceneLens(abi.SceneLights(abi.SceneMasks(abi.SceneExt(None, 0, None), 0, None), 0, None), None)
    h = C.c_void_p()
    gpu_ctx.check(gpu_ctx.lib.msk_gpu_scene_create_lens(gpu_ctx.handle, C.byref(flat.desc), C.byref(eln), C.byref(h)))
    a = np.empty((16, 16, 5), F)
    st = abi.Stats()
    prm = EV.pcg(abi, spp=2, seed=5)
    gpu_ctx.check(gpu_ctx.lib.msk_gpu_render(h, C.byref(prm), a.ctypes.data_as(C.c_void_p), C.byref(st)))
    gpu_ctx.lib.msk_gpu_scene_destroy(h)
    g = abi.Scene(gpu_ctx, flat)
    b, _ = g.render(prm)
    g.close()
    assert np.array_equal(bits(a), bits(b))
