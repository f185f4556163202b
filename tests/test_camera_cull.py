"""Camera samples that miss the scene's bounds are finished where they are made (msk_kernels.h: shade_region's regeneration,
PassParams::cull; msk_bvh.h: cull_bounds).  The cull must change no bit of any film and no counter: every GPU case compares the
film with the CPU oracle's bit for bit and `samples` exactly.  `segments` is compared twice: with the oracle's within the bound
test_gpu_parity.py documents for this pair (the GPU drops a zero-throughput path one ray earlier than the scalar loop: <= 1e-5
of the segments, whatever the cull does), and EXACTLY with the same render under MSK_CAMERA_CULL=0 — a culled sample counts
exactly one segment, as it did when it went through the pool; where every sample is culled the oracle's count is met exactly
too.  The last test is CPU-only: the bounds themselves."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W1, H1, SPP1 = 96, 64, 70            # 70 spp: not a multiple of 64, so a batch of 64 samples straddles pixels — culled and kept lanes together
SEEDS1 = (1, 7)


def bits(a):
    return a.view(np.uint32)


def same_counters(st, rst, g=None, prm=None):
    """`samples` and `segments` against the oracle's; with (g, prm) also against the same render without the cull, exactly."""
    if g is not None:
        before = os.environ.get("MSK_CAMERA_CULL")
        os.environ["MSK_CAMERA_CULL"] = "0"               # read per call by the library
        try:
            _, off = g.render(prm)
        finally:
            if before is None:
                del os.environ["MSK_CAMERA_CULL"]
            else:
                os.environ["MSK_CAMERA_CULL"] = before
        print(f"[counters] without the cull: segments {off.segments} iterations {off.iterations}")
        if (st.samples, st.segments, st.shadow_rays) != (off.samples, off.segments, off.shadow_rays):
            return False
    print(f"[counters] gpu samples {st.samples} segments {st.segments} iterations {st.iterations} | oracle samples {rst.samples} segments {rst.segments}")
    return st.samples == rst.samples and abs(int(st.segments) - int(rst.segments)) <= 1e-5 * rst.segments


@pytest.fixture(scope="module")
def case1(gpu_ctx, abi, hostmirror, oracle, golden_lookup):
    """Case 1's scene, its oracle films (computed once) and its GPU renders with the default pool."""
    flat = hostmirror.cbox_scene(W1, H1, coeff_lookup=golden_lookup)
    g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
    ref = {s: o.render(abi.render_params(spp=SPP1, seed=s), threads=8) for s in SEEDS1}
    yield g, o, ref
    g.close()
    o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS1)
def test_mixed_batches(case1, abi, seed):
    g, _, ref = case1
    prm = abi.render_params(spp=SPP1, seed=seed)
    film, st = g.render(prm)
    want, rst = ref[seed]
    assert same_counters(st, rst, g, prm) and st.samples == W1 * H1 * SPP1
    assert np.array_equal(bits(film), bits(want))
    assert (want[..., :3].max(-1) == 0).any() and (want[..., 1] > 0).any()       # background and box are both in the picture


@pytest.mark.gpu
def test_tiny_pool(case1, abi, monkeypatch):
    """64 regions of 128 slots: the free tail is smaller than a batch (batches are cut at the first sample without a slot), regions
    refill over culled batches, and a sweep over background rows stops at the cap on the samples it may examine (2 x 128)."""
    g, _, ref = case1
    monkeypatch.setenv("MSK_REGIONS", "64")
    monkeypatch.setenv("MSK_REGION_SIZE", "128")
    for seed in SEEDS1:
        prm = abi.render_params(spp=SPP1, seed=seed)
        film, st = g.render(prm)
        want, rst = ref[seed]
        assert same_counters(st, rst, g, prm)
        assert np.array_equal(bits(film), bits(want)), seed


@pytest.mark.gpu
def test_everything_culled(gpu_ctx, abi, hostmirror, oracle, golden_lookup):
    """One block of background: no sample ever takes a slot.  The render must end (the regeneration loop, the fused loop's
    "region is empty" exit and the watchdog's "counters stand still" test all see sweeps that leave no live path).
    The Cornell camera's field of view (49.3 degrees) puts the box's edge at pixel 31.08 of a 256-pixel film, inside the corner
    block; at 52 degrees it is at 36.8 (278 / (800 tan 26) of the half width), and the 32 x 32 corner crop is all background.
    A crop window is fed by every block whose 2-pixel filter border reaches it — four here, three of which see the box — so the
    render is the first of four tile shards: over a crop the shards count the blocks that feed it, and the first is the corner."""
    cam = dict(hostmirror.CBOX_CAMERA, fov=52.0)
    flat = hostmirror.flatten(hostmirror.cbox_meshes(), 256, 256, camera=cam, coeff_lookup=golden_lookup, crop=(0, 0, 32, 32))
    g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
    prm = abi.render_params(spp=64, seed=2, block_first=0, block_stride=4)
    film, st = g.render(prm)
    ref, rst = o.render(prm, threads=8)
    g.close()
    o.close()
    print(f"[all culled] samples {st.samples} segments {st.segments} iterations {st.iterations}; oracle {rst.samples} {rst.segments}")
    assert st.samples == 32 * 32 * 64 == rst.samples
    assert st.segments == st.samples == rst.segments and st.shadow_rays == 0
    assert np.array_equal(bits(film[..., 4]), bits(ref[..., 4])) and np.array_equal(bits(film), bits(ref))
    assert not film[..., :3].any() and film[..., 4].min() > 0
    assert st.bytes_shade == 20 * st.samples and st.bytes_trace == 0              # the records, and nothing else


@pytest.mark.gpu
def test_silhouette(gpu_ctx, abi, hostmirror, oracle, golden_lookup):
    """A 64 x 8 window over the right edge of the box's opening (pixel 449.8 of 512; the window is x 416..479, rows 248..255,
    inside two blocks): 2048 spp, so about a million camera rays pass within a pixel of the bounds, on both sides."""
    flat = hostmirror.cbox_scene(512, 512, coeff_lookup=golden_lookup, crop=(416, 248, 64, 8))
    g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
    prm = abi.render_params(spp=2048, seed=5)
    film, st = g.render(prm)
    ref, rst = o.render(prm, threads=16)
    ok = same_counters(st, rst, g, prm)
    g.close()
    o.close()
    assert ok
    assert np.array_equal(bits(film), bits(ref))
    lit = ref[..., 1] > 0
    assert lit[:, :30].all() and not lit[:, 38:].any()                            # box on the left of the window, background on the right


@pytest.mark.gpu
def test_far_clip_before_the_box(gpu_ctx, abi, hostmirror, oracle, golden_lookup):
    """The camera stands at z = -800 and the box begins at z = 0: with far = 700 every ray ends before it, and is culled by tfar."""
    cam = dict(hostmirror.CBOX_CAMERA, far=700.0)
    flat = hostmirror.flatten(hostmirror.cbox_meshes(), 64, 64, camera=cam, coeff_lookup=golden_lookup)
    g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
    prm = abi.render_params(spp=8, seed=3)
    film, st = g.render(prm)
    ref, rst = o.render(prm, threads=8)
    g.close()
    o.close()
    assert st.samples == rst.samples == 64 * 64 * 8 and st.segments == rst.segments == st.samples
    assert np.array_equal(bits(film), bits(ref)) and not film[..., :3].any()
    assert st.bytes_shade == 20 * st.samples                                      # every sample was culled


@pytest.mark.gpu
def test_culling_is_off_where_a_miss_is_not_a_zero_record(gpu_ctx, abi, hostmirror, oracle, golden_lookup, monkeypatch):
    """An environment emitter (a ray that leaves the scene carries radiance) and an "aov" render (record groups and the nested
    RGB record are written per sample by other code): MSK_CAMERA_CULL changes nothing — the same film, and the same bytes of
    state counted (a culled sample would take 160 of them off)."""
    from test_environment import sphere_scene
    env = abi.Scene(gpu_ctx, sphere_scene(hostmirror, 64, 64, {"radiance": None}))
    box = abi.Scene(gpu_ctx, hostmirror.cbox_scene(64, 64, coeff_lookup=golden_lookup))
    prm = abi.render_params(spp=8, seed=6)
    types = [abi.MSK_AOV_DEPTH, abi.MSK_AOV_PATH_RGBA]
    runs = {}
    for cull in ("1", "0"):
        monkeypatch.setenv("MSK_CAMERA_CULL", cull)
        runs[cull] = (env.render(prm), box.render_aov(prm, types), box.render_aov(prm, [abi.MSK_AOV_SH_NORMAL]), box.render(prm))
    env.close()
    box.close()
    for k in range(3):
        (f1, s1), (f0, s0) = runs["1"][k], runs["0"][k]
        assert np.array_equal(bits(f1), bits(f0)), k
        assert (s1.bytes_shade, s1.bytes_trace, s1.segments, s1.samples) == (s0.bytes_shade, s0.bytes_trace, s0.segments, s0.samples), k
    (_, s1), (_, s0) = runs["1"][3], runs["0"][3]
    assert s1.bytes_shade < s0.bytes_shade                                        # (the knob does reach the plain render of the same box)


@pytest.mark.gpu
def test_shards(case1, abi):
    """Case 1 as two sample shards (each bit-equal to the oracle's shard) and as two tile shards (each bit-equal to the oracle's;
    their sum bit-equal to the whole film away from the tiles' 2-pixel filter borders, where one shard contributes)."""
    g, o, ref = case1
    seed = SEEDS1[0]
    full = ref[seed][0]
    for r in range(2):
        prm = abi.render_params(spp=SPP1, seed=seed, sample_first=r, sample_stride=2)
        film, st = g.render(prm)
        want, rst = o.render(prm, threads=8)
        assert same_counters(st, rst, g, prm) and np.array_equal(bits(film), bits(want)), r
    parts = []
    for r in range(2):
        prm = abi.render_params(spp=SPP1, seed=seed, block_first=r, block_stride=2)
        film, st = g.render(prm)
        want, rst = o.render(prm, threads=8)
        assert same_counters(st, rst, g, prm) and np.array_equal(bits(film), bits(want)), r
        parts.append(film)
    interior = np.ones((H1, W1), bool)
    for k in range(0, max(W1, H1), 32):
        interior[max(0, k - 2):k + 2, :] = False
        interior[:, max(0, k - 2):k + 2] = False
    s = parts[0] + parts[1]
    assert np.array_equal(bits(s[interior]), bits(full[interior]))


@pytest.mark.gpu
def test_on_against_off(gpu_ctx, abi, hostmirror, golden_lookup, monkeypatch):
    g = abi.Scene(gpu_ctx, hostmirror.cbox_scene(128, 128, coeff_lookup=golden_lookup))
    prm = abi.render_params(spp=16, seed=4)
    monkeypatch.setenv("MSK_CAMERA_CULL", "0")
    f0, s0 = g.render(prm)
    monkeypatch.setenv("MSK_CAMERA_CULL", "1")
    f1, s1 = g.render(prm)
    g.close()
    print(f"[on/off] iterations {s0.iterations} -> {s1.iterations}; bytes {s0.bytes_shade + s0.bytes_trace} -> {s1.bytes_shade + s1.bytes_trace}")
    assert np.array_equal(bits(f1), bits(f0))
    assert (s1.samples, s1.segments, s1.shadow_rays) == (s0.samples, s0.segments, s0.shadow_rays)
    assert s1.iterations <= s0.iterations
    # the culled count: the samples whose record is all zeros are the ones that hit nothing; of those the cull takes the ones
    # that miss the BOUNDS.  It is not exposed by the ABI; the byte counts pin it: 160 bytes each, 112 of shading and 48 of traversal
    saved = (s0.bytes_shade + s0.bytes_trace) - (s1.bytes_shade + s1.bytes_trace)
    assert saved > 0 and saved % 160 == 0
    culled = saved // 160
    assert s0.bytes_shade - s1.bytes_shade == 112 * culled and s0.bytes_trace - s1.bytes_trace == 48 * culled
    assert 0.38 * s1.samples < culled < 0.46 * s1.samples                         # 43.3 % of this camera's rays miss the box's bounds


# ---- CPU: the bounds themselves
def triangle_positions(flat):
    """9 floats per triangle, as msk_gpu_scene_create gathers them (faces index their mesh's vertices)."""
    d = flat.desc
    out = []
    for i in range(d.n_meshes):
        m = d.meshes[i]
        f = flat.faces[m.first_face:m.first_face + m.face_count].astype(np.int64) + m.first_vertex
        out.append(flat.vertices[f, :3].reshape(-1, 9))
    return np.ascontiguousarray(np.concatenate(out + [np.zeros((0, 9), np.float32)]), np.float32)


def run_check(exe, path, pos, pad):
    pos.tofile(path)
    r = subprocess.run([exe, path, repr(pad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines()}
    head = dict(zip(rows["tris"][1::2], rows["tris"][2::2]))
    fl = lambda v: np.array([float.fromhex(x) for x in v], np.float32)
    return int(rows["tris"][0]), int(head["root_ref"]), int(head["on"]), fl(rows["node"]) if "node" in rows else None, fl(rows["lo"]), fl(rows["hi"])


def test_bounds_are_the_union_of_the_roots_child_boxes(hostmirror, tmp_path):
    exe = str(tmp_path / "cull_bounds_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "native", "cull_bounds_check.cpp")])
    path = str(tmp_path / "tris.f32")
    blob = hostmirror.blob_mesh("blob", (370, 420, 250), 70, 40, 40, hostmirror.WHITE, seed=2)
    for flat in (hostmirror.cbox_scene(16, 16), hostmirror.flatten([blob], 16, 16)):
        pos = triangle_positions(flat)
        pad = 0.5e-5 * float(np.linalg.norm(pos.reshape(-1, 3).max(0) - pos.reshape(-1, 3).min(0)))
        n, root, on, node, lo, hi = run_check(exe, path, pos, pad)
        assert n == len(pos) and on == 1 and root < 0x80000000
        # node: [lo0.x lo1.x lo0.y lo1.y] [lo0.z lo1.z hi0.x hi1.x] [hi0.y hi1.y hi0.z hi1.z]
        assert np.array_equal(lo, np.minimum(node[0:6:2], node[1:6:2])) and np.array_equal(hi, np.maximum(node[6:12:2], node[7:12:2]))
        # ... which hold every vertex, and no more than the boxes' padding (2 tri_pad, rounded) around them
        v = pos.reshape(-1, 3)
        assert (lo < v.min(0)).all() and (hi > v.max(0)).all()
        assert np.allclose(lo, v.min(0) - 2 * pad, rtol=0, atol=1e-3 * pad + 1e-4) and np.allclose(hi, v.max(0) + 2 * pad, rtol=0, atol=1e-3 * pad + 1e-4)
    # no pair of child boxes, no cull: a tree that is one leaf (two triangles), and no triangles at all
    two = triangle_positions(hostmirror.cbox_scene(16, 16))[:2]
    n, root, on, node, _, _ = run_check(exe, path, two, 1e-3)
    assert n == 2 and root >= 0x80000000 and on == 0 and node is None
    n, _, on, _, _, _ = run_check(exe, path, np.zeros((0, 9), np.float32), 1e-3)
    assert n == 0 and on == 0
