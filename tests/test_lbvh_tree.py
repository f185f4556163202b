"""The tree the device-side BVH builder makes (csrc/msk_lbvh.hip, MSK_BVH_BUILD=gpu), pinned to a scalar CPU twin
(tests/native/lbvh_ref.h): structure, boxes, depth.  Film and trace_closest parity cannot see the tree — hit selection is by
(t, prim) — so a refit that reads a stale box, a triangle in two leaves, swapped Morton axes or a wrong `depth` pass them all.

CPU (any box): the twin passes the checks that do not rest on it (every node once, the leaves tile [0, n), child boxes EQUAL to the
padded union of their triangles, records equal to the host builder's by prim, depth, class bits), its hierarchy is that of a
literal transcription of k_hierarchy's loops, and its trees go through collapse4 / collapse8 like the host builder's.
GPU: msklbvh::build equals the twin bit for bit on every input, writes nothing behind its records, and builds the same bytes
twice (tests/native/lbvh_tree_check.hip); a staircase scene whose Karras tree is over thirty levels deep gives the oracle's
brute-force hits and film through every placement, the overflow stack at MSK_STACK_CAP=4 included."""
import importlib.util
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
KNOBS = ("MSK_BVH_BUILD", "MSK_BVH_LEAF", "MSK_BVH_SWEEP", "MSK_LDS_SCENE_KB", "MSK_STACK_CAP", "MSK_WIDE_BVH", "MSK_QUANT_BVH", "MSK_WIDE_LDS",
         "MSK_COLLAPSE_OPTIMAL", "MSK_PAD_SCALE", "MSK_FUSED", "MSK_SORT", "MSK_STREAMS", "MSK_FUSED_HBM", "MSK_FUSED_TAIL_PCT", "MSK_TRACE_REFILL")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lbvh") / "lbvh_tree_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(NATIVE, "lbvh_tree_check.cpp")])
    return exe


def _run(cmd, timeout):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "all ok" in p.stdout and "FAIL" not in p.stdout, "\n".join(l for l in p.stdout.splitlines() if "ok  " not in l)[-3000:] + p.stderr[-1000:]
    return p.stdout


def test_the_twin_passes_the_tree_checks_and_is_karras_hierarchy(checker):
    """Every input (sizes 0 … 70001 around the wave, block, sort tile and scan tile; soups at three scales, equal codes, runs of
    duplicates, the staircase in four boxes, planar and one-ulp extents, Morton boxes too small and too large; leaf sizes 1 … 8; class
    bits): the tree checks on the twin, first / last / left / right of every inner node against k_hierarchy's loops, depth = the
    height of the uncollapsed hierarchy, and a staircase of at least 30 levels from 65 triangles on."""
    out = _run([checker, "twin"], 120)
    deep = [int(l.split("depth")[1].split()[0]) for l in out.splitlines() if l.startswith("ok   d") and int(l.split(" n ")[1].split()[0]) >= 65]
    assert len(deep) >= 4 * 10 and min(deep) >= 30


def test_the_twins_trees_collapse_like_the_host_builders(checker):
    """Twin trees (Karras numbering: children not above their parent; chains of 30 levels) and host-built trees of the same triangles
    through collapse4 (optimal, greedy) and collapse8: the quantised forms contain the padded boxes wherever they exist (a refusal is
    printed, not failed), the wide tree's leaves are the binary tree's, each once, and max_depth4 / max_depth8 cover the walked depth.
    The mean area ratios are printed and not bounded: nobody has measured one for Karras trees."""
    _run([checker, "collapse"], 120)


# ------------------------------------------------------------------------------------------ the deep tree through the library
def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


S = 100.0          # the staircase's box: [0, S]^3


def _staircase_faces(rng, n):
    """Family d of lbvh_ref.h: cluster r = i % 31 in the middle of cell (1023 >> ((r+2)/3), 1023 >> ((r+1)/3), 1023 >> (r/3)), every
    triangle a tenth of a cell wide."""
    cell = S / 1024.0
    faces = []
    for i in range(n):
        r = i % 31
        q = np.array([1023 >> ((r + 2) // 3), 1023 >> ((r + 1) // 3), 1023 >> (r // 3)], np.float64)
        faces.append(tuple(tuple(float(np.float32(v)) for v in (q + 0.5) * cell + rng.uniform(-0.05, 0.05, 3) * cell) for _ in range(3)))
    return faces


@pytest.fixture(scope="module")
def deep(hostmirror, oracle, abi, checker, tmp_path_factory):
    """The scene, its rays, the twin's height of its triangles and the oracle's brute-force answers, made once."""
    hm = hostmirror
    rng = np.random.RandomState(31)
    soup = hm.MeshSpec("staircase", _staircase_faces(rng, 257), (0.5, 0.5, 0.5), radiance=(8, 8, 8))
    # one tiny triangle at each nominal corner: the scene's bounds (min / max of the vertices) are the nominal box
    corners = []
    for k in range(8):
        c = np.array([S * ((k >> a) & 1) for a in range(3)])
        inward = np.where(c > 0, -1.0, 1.0) * 1e-3 * S
        corners.append(tuple(tuple(float(np.float32(v)) for v in p) for p in (c, c + inward * [1, 0, 0.5], c + inward * [0, 1, 0.5])))
    corner_mesh = hm.MeshSpec("corners", corners, (0.7, 0.3, 0.2))
    camera = dict(fov=40.0, near=1.0, far=1e4, origin=(S + 60.0, S + 45.0, S + 30.0), target=(0.0, 0.0, 0.0), up=(0, 1, 0))
    flat = hm.flatten([soup, corner_mesh], 16, 16, camera=camera)
    d = flat.desc
    tris = np.array([[flat.vertices[d.meshes[m].first_vertex + i, :3] for i in flat.faces[f]] for m in range(d.n_meshes)
                     for f in range(d.meshes[m].first_face, d.meshes[m].first_face + d.meshes[m].face_count)], np.float32)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    assert len(tris) == 265 and np.array_equal(lo, np.zeros(3, np.float32)) and np.array_equal(hi, np.full(3, S, np.float32))
    path = str(tmp_path_factory.mktemp("deep") / "tris.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I6f", len(tris), *lo, *hi) + tris.astype("<f4").tobytes())
    r = subprocess.run([checker, "height", path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    height = int(r.stdout.split("height")[1].split()[0])
    # rays: half from outside towards random points of the clusters, half adversarial (from / towards vertices, edges, planes)
    n = 2048
    t = tris[rng.randint(0, 257, n)].astype(np.float64)
    b = rng.dirichlet([1, 1, 1], n)
    target = np.einsum("nk,nkc->nc", b, t) + rng.normal(size=(n, 3)) * 0.002 * (rng.uniform(size=(n, 1)) < 0.5)
    dirs = rng.normal(size=(n, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    origin = np.full(3, S / 2) + dirs * 2 * S
    dd = target - origin; dist = np.linalg.norm(dd, axis=1, keepdims=True); dd /= dist
    outside = np.concatenate([origin, np.zeros((n, 1)), dd, np.where(rng.uniform(size=(n, 1)) < 0.5, np.inf, dist * 1.001)], 1).astype(np.float32)
    rays = np.concatenate([outside, _load("fuzz_rays").adversarial_rays(rng, tris, n)]).astype(np.float32)
    assert rays.shape == (4096, 8)
    orc = oracle.scene(flat)
    orc.set_bvh(0)                                   # the brute force
    closest, occluded = orc.trace_closest(rays).copy(), orc.trace_any(rays).copy()
    prm = abi.render_params(spp=4, seed=3)
    film, _ = orc.render(prm, threads=4)
    orc.close()
    closest.setflags(write=False); occluded.setflags(write=False); film.setflags(write=False)
    return dict(flat=flat, rays=rays, height=height, closest=closest, occluded=occluded, film=film, prm=prm, stdout=r.stdout)


def test_the_staircase_scene_makes_a_tree_of_thirty_levels(deep):
    """The precondition of the GPU test below, on the CPU: the twin, run on the flattened triangles with the scene's bounds, reports
    a hierarchy at least 30 levels high (every parity scene of the suite makes 15 to 20), and the rays do hit the clusters."""
    print(deep["stdout"])
    assert deep["height"] >= 30
    hit = np.isfinite(deep["closest"][:, 0]) & (deep["closest"].view(np.uint32)[:, 3] != 0xffffffff)
    assert deep["occluded"][:2048].mean() > 0.25 and hit.any()


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_device_built_tree_equals_the_twin_bit_for_bit(tmp_path):
    """tests/native/lbvh_tree_check.hip, compiled with the library's own flags (the builder under test is the library's): every input,
    guards and sentinel, two builds."""
    import __graft_entry__ as entry
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = str(tmp_path / "lbvh_tree_check_gpu")
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["-o", exe, os.path.join(NATIVE, "lbvh_tree_check.hip")], check=True, capture_output=True)
    _run(["timeout", "-k", "10", "120", exe], 150)


KNOB_SETS = [{}, {"MSK_BVH_LEAF": "1"},
             {"MSK_LDS_SCENE_KB": "0"}, {"MSK_LDS_SCENE_KB": "0", "MSK_BVH_LEAF": "1"},
             {"MSK_LDS_SCENE_KB": "0", "MSK_STACK_CAP": "4"},
             {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "0", "MSK_STACK_CAP": "4"},
             {"MSK_LDS_SCENE_KB": "0", "MSK_WIDE_BVH": "8"},
             {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "1"},
             {"MSK_LDS_SCENE_KB": "0", "MSK_QUANT_BVH": "0"}]


@pytest.mark.gpu
def test_a_tree_of_thirty_levels_gives_the_brute_force_hits_in_every_placement(deep, request, abi, monkeypatch):
    """The staircase scene with MSK_BVH_BUILD=gpu: trace_closest bit for bit and trace_any against the oracle's brute force under
    every knob set, and a 16 x 16, 4 spp render against the oracle's film with the default knobs and with the tree in HBM and four
    stack entries in LDS (the overflow stack under k_trace_r<6>).  A refusal by msk_gpu_scene_create fails the test: a placement
    that cannot hold the stack has to fall back, not refuse.  The library does not expose the trace mode; the renders print their
    launch counts.  Measured: 8 trace and 8 shade launches, no k_wavefront* launch under either knob set — the fused tail of a
    tree in HBM (k_wavefront_h) needs shading tables that do not fit LDS (msk_plan.h: fused_h), and this scene's 265 triangles do."""
    assert deep["height"] >= 30                      # on the CPU, before the GPU is used
    gpu_ctx = request.getfixturevalue("gpu_ctx")
    for knobs in KNOB_SETS:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("MSK_BVH_BUILD", "gpu")
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        g = abi.Scene(gpu_ctx, deep["flat"])
        try:
            closest, occluded = g.trace_closest(deep["rays"]), g.trace_any(deep["rays"])
            assert np.array_equal(closest.view(np.uint32), deep["closest"].view(np.uint32)), knobs
            assert np.array_equal(occluded, deep["occluded"]), knobs
            if knobs in ({}, {"MSK_LDS_SCENE_KB": "0", "MSK_STACK_CAP": "4"}):
                film, st = g.render(deep["prm"])
                print("knobs %s: render launches trace %u shade %u wavefront %u, iterations %u" % (knobs, st.launches_trace, st.launches_shade, st.launches_wavefront, st.iterations))
                assert np.array_equal(film.view(np.uint32), deep["film"].view(np.uint32)), knobs
        finally:
            g.close()
