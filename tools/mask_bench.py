#!/usr/bin/env python3
"""Times the `mask` kernels against the family a scene without masks runs (EXPERIMENTS.md, "The mask BSDF").

    python tools/mask_bench.py [--size 512] [--spp 64] [--steps 5] [--warmup 2]

The Cornell box with a constant mask of opacity 1 on every BSDF entry (k_shade_gen_m / k_wavefront_m: the nested BSDF to the bit)
against the same scene without masks (the diffuse-only family), in one process, alternated: device time of msk_gpu_render
(msk_stats::ms_total), the median of --steps renders after --warmup.  Checks that the two films are the same bits.  One JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    abi = importlib.import_module("misaki-render_amd.abi")
    hm = importlib.import_module("misaki-render_amd.hostmirror")
    plain = hm.cbox_scene(args.size, args.size)
    masked = hm.cbox_scene(args.size, args.size)
    n = masked.desc.n_bsdfs
    masked.masks = (abi.MaskDesc * n)()
    for b in range(n):
        masked.masks[b].bsdf, masked.masks[b].opacity, masked.masks[b].filter = b, 1.0, 0
    ctx = abi.Context(0)
    g0, g1 = abi.Scene(ctx, plain), abi.Scene(ctx, masked)
    prm = abi.render_params(spp=args.spp, seed=1)
    runs = {"plain": [], "masked": []}
    films = {}
    for step in range(args.warmup + args.steps):
        for name, g in (("plain", g0), ("masked", g1)):
            film, st = g.render(prm)
            films[name] = film
            if step >= args.warmup:
                runs[name].append(st.ms_total)
    g0.close()
    g1.close()
    ctx.close()
    ms0, ms1 = statistics.median(runs["plain"]), statistics.median(runs["masked"])
    print(json.dumps({"scene": "cbox", "size": args.size, "spp": args.spp, "ms_without_masks": round(ms0, 3), "ms_with_opacity_one_masks": round(ms1, 3),
                      "ratio": round(ms1 / ms0, 4), "runs_without": [round(x, 3) for x in runs["plain"]], "runs_with": [round(x, 3) for x in runs["masked"]],
                      "same_film_bits": bool(np.array_equal(films["plain"].view(np.uint32), films["masked"].view(np.uint32)))}), flush=True)


if __name__ == "__main__":
    main()
