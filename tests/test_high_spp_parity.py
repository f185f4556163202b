"""Film parity at the sample counts the project benchmarks: BASELINE config 4 (cbox 1920x1080 @ 4096 spp, 8,493,465,600 samples
in one record pass, past 2^32), the config-5 class at its 1024 spp, and the top of the path state's 20-bit sample field.

A whole film at these counts is out of the oracle's reach, so single film pixels are checked against OracleScene.film_pixels
(tests/oracle_binding.py: only the samples that can reach a pixel, same order, same sums; tests/test_oracle_film_pixels.py
proves it equal to OracleScene.render), and crops against OracleScene.render of the blocks they touch.  Need an MI355X."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W4, H4, SPP4 = 1920, 1080, 4096
ORACLE_THREADS = 16


def cbox(hostmirror, golden_lookup, w, h, crop=None):
    return hostmirror.cbox_scene(w, h, coeff_lookup=golden_lookup, crop=crop)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pass_pixels(oracle, w, h, bs=32):
    """film (x, y) of every pass pixel index j of a whole-film one-pass render: spiral block order, raster order inside a block"""
    xs, ys = [], []
    for ox, oy, sx, sy in oracle.spiral_blocks(w, h, bs):
        yy, xx = np.mgrid[oy:oy + sy, ox:ox + sx]
        xs.append(xx.ravel())
        ys.append(yy.ravel())
    return np.concatenate(xs), np.concatenate(ys)


def block_cover(oracle, w, h, border=2, bs=32):
    """-> (how many blocks' bordered areas hold each pixel, spiral id of the one block where that count is 1)"""
    cover = np.zeros((h, w), np.int32)
    owner = np.full((h, w), -1, np.int64)
    for bid, (ox, oy, sx, sy) in enumerate(oracle.spiral_blocks(w, h, bs)):
        sl = np.s_[max(0, oy - border):oy + sy + border, max(0, ox - border):ox + sx + border]
        cover[sl] += 1
        owner[sl] = bid
    return cover, owner


def config4_anchors(oracle):
    """>= 24 film pixels, named by their pass pixel index j (the k_shade_gen split of sample j * 4096 + si)"""
    jx, jy = pass_pixels(oracle, W4, H4)
    n = len(jx)
    assert n == W4 * H4
    lim = (1 << 32) // SPP4                                       # 1,048,576: the first j whose samples are all >= 2^32
    js = {0, 1, 1000, 523_777, lim - 2, lim - 1, lim, lim + 1, 1_500_000, n - 2, n - 1}
    pts = {(int(jx[j]), int(jy[j])) for j in js}
    # 2-block and 4-block edge pixels of the blocks on both sides of the boundary, of an early and of a late block
    for j in (lim - 1, lim, 30_000, 1_900_000):
        bx, by = int(jx[j]) // 32 * 32, int(jy[j]) // 32 * 32
        for p in ((bx, by), (bx - 1, by - 1), (bx + 31, by + 32), (bx + 32, by + 31), (bx + 15, by), (bx + 16, by - 1),
                  (bx, by + 17), (bx - 2, by + 18), (bx + 33, by + 5)):
            if 0 <= p[0] < W4 and 0 <= p[1] < H4:
                pts.add(p)
    # the 24-px ragged bottom block row, and the four film corners
    pts |= {(0, 0), (W4 - 1, 0), (0, H4 - 1), (W4 - 1, H4 - 1), (700, 1056), (701, 1055), (959, 1079), (1280, 1066), (1279, 1057)}
    pts = sorted(pts)
    j_of = {(int(x), int(y)): j for j, (x, y) in enumerate(zip(jx, jy))}
    return pts, np.array([j_of[p] for p in pts])


def test_config4_one_pass_past_2_32_samples(gpu_ctx, abi, hostmirror, oracle, golden_lookup, monkeypatch):
    """BASELINE config 4 in one call and one record pass: the linear sample index passes 2^32, so k_shade_gen splits it with
    its 64-bit division.  Anchors on both sides of j * 4096 = 2^32 against the oracle; the whole film against the 8 tile
    shards, whose ~1.06e9 samples each stay on the 32-bit division."""
    import torch
    monkeypatch.setenv("MSK_RECORD_BUDGET_MB", "163000")         # 8,493,465,600 x 20 B = 162,000 MiB of records: one pass
    flat = cbox(hostmirror, golden_lookup, W4, H4)
    free0, _ = torch.cuda.mem_get_info(0)
    g = abi.Scene(gpu_ctx, flat)
    o = oracle.scene(flat)
    try:
        prm = abi.render_params(spp=SPP4, seed=3)
        t0 = time.time()
        film, st = g.render(prm)
        t_whole = time.time() - t0
        held, _ = torch.cuda.mem_get_info(0)
        assert st.samples == 8_493_465_600 and st.passes == 1 and st.invalid_samples == 0
        assert free0 - held > 160_000 << 20                       # the one pass's records are resident
        assert np.isfinite(film).all() and (film >= 0).all() and (film[..., 4] > 0).all()

        pts, js = config4_anchors(oracle)
        lim = (1 << 32) // SPP4
        assert len(pts) >= 24 and (js < lim).sum() >= 6 and (js >= lim).sum() >= 6
        assert {lim - 1, lim, W4 * H4 - 1} <= set(js.tolist())
        t0 = time.time()
        want = o.film_pixels(prm, pts, threads=ORACLE_THREADS)
        t_oracle = time.time() - t0
        got = np.stack([film[y, x] for x, y in pts])
        bad = [(p, int(j), gv.tolist(), wv.tolist()) for p, j, gv, wv in zip(pts, js, got, want) if not np.array_equal(bits(gv), bits(wv))]
        assert not bad, bad[:6]

        # the 8 tile shards: every block exactly once, each shard on the 32-bit split
        cover, owner = block_cover(oracle, W4, H4)
        acc = np.zeros_like(film)
        n = 0
        t0 = time.time()
        for r in range(8):
            sh, sst = g.render(abi.render_params(spp=SPP4, seed=3, block_first=r, block_stride=8))
            assert sst.samples < 1 << 32 and sst.passes == 1
            n += sst.samples
            one = cover == 1
            assert np.array_equal(bits(sh[one]), bits(np.where((owner[one] % 8 == r)[:, None], film[one], np.float32(0)))), r
            acc += sh                                             # rank order, fp32
        t_shards = time.time() - t0
        assert n == st.samples
        le2 = cover <= 2                                          # one term, or two: a + b == b + a
        assert np.array_equal(bits(acc[le2]), bits(film[le2]))
        # 3 or 4 blocks: the same fp32 terms (all >= 0) summed in another order, <= 3 roundings of the total each way
        assert np.allclose(acc[~le2], film[~le2], rtol=2e-6, atol=0)
        print(f"\n[timing] config 4 whole {t_whole:.1f} s ({st.ms_total:.0f} ms device), 8 tile shards {t_shards:.1f} s, "
              f"oracle {len(pts)} anchors {t_oracle:.1f} s")
    finally:
        g.close()
        o.close()
    free1, _ = torch.cuda.mem_get_info(0)
    assert free1 >= free0 - (1 << 30), (free0, free1)              # the ~170 GB workspace went back


# ---- config 4, 64x64 crops: long k_resolve_rows chains, pass planning and the render variants against OracleScene.render
CROPS = {"grid3x3": (944, 520, 64, 64),                             # off the block grid: blocks 29..31 x 16..18
         "corner": (1856, 1016, 64, 64)}                            # blocks 57..59 x 31..33: the 24-px last row
CROP_SAMPLES = {"grid3x3": 9 * 32 * 32 * SPP4, "corner": 3 * (32 * 32 * 2 + 32 * 24) * SPP4}


@pytest.fixture(scope="module")
def config4_crops(gpu_ctx, abi, hostmirror, oracle, golden_lookup):
    out = {}
    for name, c in CROPS.items():
        flat = cbox(hostmirror, golden_lookup, W4, H4, crop=c)
        o = oracle.scene(flat)
        t0 = time.time()
        ref, rst = o.render(abi.render_params(spp=SPP4, seed=5), threads=ORACLE_THREADS)
        print(f"\n[timing] oracle crop {name} {time.time() - t0:.1f} s")
        assert rst.samples == CROP_SAMPLES[name]
        out[name] = (abi.Scene(gpu_ctx, flat), o, ref)
    yield out
    for g, o, _ in out.values():
        g.close()
        o.close()


@pytest.mark.parametrize("env", [{}, {"MSK_STREAMS": "1"}, {"MSK_RESOLVE_GENERIC": "1"}, {"MSK_RECORD_BUDGET_MB": "200"},
                                 {"MSK_FUSED_TAIL_PCT": "0"}], ids=["default", "streams1", "resolve_generic", "passes", "no_fused_tail"])
@pytest.mark.parametrize("name", list(CROPS))
def test_config4_crop_bit_exact(config4_crops, abi, monkeypatch, name, env):
    g, _, ref = config4_crops[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    film, st = g.render(abi.render_params(spp=SPP4, seed=5))
    assert st.samples == CROP_SAMPLES[name] and st.invalid_samples == 0
    if "MSK_RECORD_BUDGET_MB" in env:                             # 80 MiB of records per block: two blocks per pass
        assert st.passes >= 3
    assert np.array_equal(bits(film), bits(ref)), float(np.abs(film - ref).max())


@pytest.mark.parametrize("name", list(CROPS))
def test_config4_crop_tile_shards_bit_exact(config4_crops, abi, name):
    g, o, ref = config4_crops[name]
    acc, n = np.zeros_like(ref), 0
    for r in range(8):
        prm = abi.render_params(spp=SPP4, seed=5, block_first=r, block_stride=8)
        film, st = g.render(prm)
        want, wst = o.render(prm, threads=ORACLE_THREADS)
        assert st.samples == wst.samples
        assert np.array_equal(bits(film), bits(want)), r
        acc += film
        n += st.samples
    assert n == CROP_SAMPLES[name] and np.allclose(acc, ref, rtol=2e-6, atol=0)


# ---- config-5 class at its real sample count
TEAPOT_CROP = (516, 516, 56, 56)       # inside [514, 574)^2: the bordered areas of exactly 2 x 2 blocks (16..17 x 16..17)


def test_config5_class_at_1024_spp(gpu_ctx, abi, hostmirror, oracle):
    """The rough-dielectric config-5 class at 1024 spp (the suite's other tests render it at 128): one whole call and the
    8 sample shards, each bit-exact vs the oracle.  The window touches 2 x 2 blocks: 4,194,304 dielectric samples, which
    the oracle needs about half a minute for on 16 threads (a 64 x 64 window would touch 3 x 3)."""
    flat = hostmirror.teapot_class_scene(1024, crop=TEAPOT_CROP)
    g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
    try:
        prm = abi.render_params(spp=1024, seed=8)
        film, st = g.render(prm)
        t0 = time.time()
        ref, rst = o.render(prm, threads=ORACLE_THREADS)
        t_whole = time.time() - t0
        assert st.samples == rst.samples == 4 * 32 * 32 * 1024
        assert np.array_equal(bits(film), bits(ref)), float(np.abs(film - ref).max())
        acc = np.zeros_like(film)
        t0 = time.time()
        for r in range(8):
            sp = abi.render_params(spp=1024, seed=8, sample_first=r, sample_stride=8)
            sh, sst = g.render(sp)
            want, wst = o.render(sp, threads=ORACLE_THREADS)
            assert sst.samples == wst.samples == 4 * 32 * 32 * 128
            assert np.array_equal(bits(sh), bits(want)), r
            acc += sh
        t_shards = time.time() - t0
        # 8 partial sums of ~128 x 25 fp32 terms each against one sum of ~1024 x 25: re-association only
        assert np.allclose(acc, film, rtol=1e-4, atol=1e-6), float(np.abs(acc - film).max())
        print(f"\n[timing] config-5 class oracle: whole {t_whole:.1f} s, 8 sample shards {t_shards:.1f} s (with the GPU renders)")
    finally:
        g.close()
        o.close()


# ---- the top of the 20-bit sample field
ONE_BLOCK_CROP = (48, 48, 2, 2)        # 16 px inside block (1, 1) of a 128 x 128 film: no other block's border reaches it


def test_2_20_spp_fills_the_sample_field(gpu_ctx, abi, hostmirror, oracle, golden_lookup):
    """spp = 2^20: owned sample indices up to 0xFFFFF, the whole 20-bit field of PathState::id.y, and a 2^20-long replay chain
    per pixel.  Exactly one block is rendered; the crop's pixels are bit-exact vs the oracle, and max_depth = 1 leaves the
    filter-weight channels (which only the sample positions decide) bit for bit as they are."""
    flat = cbox(hostmirror, golden_lookup, 128, 128, crop=ONE_BLOCK_CROP)
    g, o = abi.Scene(gpu_ctx, flat), oracle.scene(flat)
    try:
        spp = 1 << 20
        prm = abi.render_params(spp=spp, seed=13)
        film, st = g.render(prm)
        assert st.samples == 32 * 32 * spp and st.invalid_samples == 0
        cx, cy = ONE_BLOCK_CROP[:2]
        pts = [(cx + dx, cy + dy) for dy in range(2) for dx in range(2)]
        t0 = time.time()
        want = o.film_pixels(prm, pts, threads=ORACLE_THREADS)
        t_oracle = time.time() - t0
        got = np.stack([film[y - cy, x - cx] for x, y in pts])
        assert np.array_equal(bits(got), bits(want)), (got, want)
        d1, st1 = g.render(abi.render_params(spp=spp, seed=13, max_depth=1))
        assert st1.samples == st.samples
        assert np.array_equal(bits(d1[..., 3:]), bits(film[..., 3:]))
        assert not np.array_equal(bits(d1[..., :3]), bits(film[..., :3]))        # (and the radiance did change)
        print(f"\n[timing] 2^20 spp: oracle 4 pixels {t_oracle:.1f} s")
    finally:
        g.close()
        o.close()
