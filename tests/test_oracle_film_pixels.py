"""OracleScene.film_pixels (tests/oracle_binding.py) against OracleScene.render, on the CPU: the oracle side of the high-spp
parity tests (tests/test_high_spp_parity.py) reads single film pixels at sample counts a whole render cannot reach, from only
the samples that can touch them.  Leaving the others out must not change a single bit."""
import numpy as np
import pytest


def probe_pixels(w, h, bs=32):
    """~40 pixels: block interiors, both sides of 2-block edges, 4-block corners, film corners, the ragged last row / column"""
    pts = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (16, 16), (48, 40), (5, 20)}
    for e in range(bs, w, bs):                                   # vertical block edges: 2-block pixels on both sides
        pts |= {(e - 3, 10), (e - 2, 10), (e - 1, 10), (e, 10), (e + 1, 11), (e + 2, 12)}
    for e in range(bs, h, bs):
        pts |= {(20, e - 2), (21, e - 1), (22, e), (23, e + 1)}
    for ex in range(bs, w, bs):                                  # 4-block corners
        for ey in range(bs, h, bs):
            pts |= {(ex - 1, ey - 1), (ex, ey), (ex - 2, ey + 1), (ex + 1, ey - 2)}
    last = (h - 1) // bs * bs
    pts |= {(x, y) for x in (3, w // 2, w - 2) for y in (last, h - 2)}
    return sorted(p for p in pts if p[0] < w and p[1] < h)


@pytest.mark.parametrize("crop", [None, (27, 19, 50, 45)])
def test_film_pixels_equal_the_whole_render(abi, hostmirror, oracle, golden_lookup, crop):
    w, h = 100, 72                                               # 4 x 3 blocks, a 4-px last column and an 8-px last row
    flat = hostmirror.cbox_scene(w, h, coeff_lookup=golden_lookup, crop=crop)
    o = oracle.scene(flat)
    try:
        prm = abi.render_params(spp=16, seed=11)
        ref, _ = o.render(prm, threads=8)
        cx, cy, cw, ch = crop or (0, 0, w, h)
        pts = [p for p in probe_pixels(w, h) if cx <= p[0] < cx + cw and cy <= p[1] < cy + ch]
        if crop:
            pts += [(cx, cy), (cx + cw - 1, cy), (cx, cy + ch - 1), (cx + cw - 1, cy + ch - 1)]       # the window's corners
            pts += [(cx, y) for y in (31, 32)] + [(cx + cw - 1, y) for y in (31, 32)] + \
                   [(x, y) for x in (31, 32, 63, 64) for y in (cy, cy + ch - 1)]                  # its edges at block edges
        assert len(pts) >= (20 if crop else 40)
        got = o.film_pixels(prm, pts, threads=4)
        want = np.stack([ref[y - cy, x - cx] for x, y in pts])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            [(p, g, r) for p, g, r in zip(pts, got, want) if not np.array_equal(g, r)][:4]
        assert (want[:, 4] > 0).all()                            # every probe has samples: the comparison is not of zeros
        # a block shard: only that shard's blocks are summed
        sh = abi.render_params(spp=16, seed=11, block_first=1, block_stride=3)
        ref1, _ = o.render(sh, threads=8)
        got1 = o.film_pixels(sh, pts, threads=4)
        assert np.array_equal(got1.view(np.uint32), np.stack([ref1[y - cy, x - cx] for x, y in pts]).view(np.uint32))
    finally:
        o.close()
