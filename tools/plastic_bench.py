#!/usr/bin/env python3
"""Times a `plastic` scene against the same scene diffuse (EXPERIMENTS.md, "The plastic BSDF").

    python tools/plastic_bench.py [--size 512] [--spp 64] [--steps 5] [--warmup 2]

The Cornell box with plastic boxes and walls (every shape but the luminaire: its own colour as the diffuse base under a coat of
1.49 / 1.00028, nonlinear; k_shade_gen_m / k_wavefront_m) against the box as it is (the diffuse-only family), in one process,
alternated: device time of msk_gpu_render (msk_stats::ms_total), the median of --steps renders after --warmup.  One JSON line."""
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
    meshes = hm.cbox_meshes()
    for m in meshes:
        if m.radiance is None:
            m.bsdf = {"type": "plastic", "diffuse_reflectance": tuple(m.reflectance), "nonlinear": True}
    plain, coated = hm.cbox_scene(args.size, args.size), hm.flatten(meshes, args.size, args.size)
    ctx = abi.Context(0)
    g0, g1 = abi.Scene(ctx, plain), abi.Scene(ctx, coated)
    prm = abi.render_params(spp=args.spp, seed=1)
    runs = {"diffuse": [], "plastic": []}
    stats = {}
    for step in range(args.warmup + args.steps):
        for name, g in (("diffuse", g0), ("plastic", g1)):
            film, st = g.render(prm)
            stats[name] = (st, bool(np.isfinite(film).all()), float(film[..., 1].sum() / film[..., 4].sum()))
            if step >= args.warmup:
                runs[name].append(st.ms_total)
    g0.close()
    g1.close()
    ctx.close()
    ms0, ms1 = statistics.median(runs["diffuse"]), statistics.median(runs["plastic"])
    print(json.dumps({"scene": "cbox", "size": args.size, "spp": args.spp, "ms_diffuse": round(ms0, 3), "ms_plastic": round(ms1, 3), "ratio": round(ms1 / ms0, 4),
                      "runs_diffuse": [round(x, 3) for x in runs["diffuse"]], "runs_plastic": [round(x, 3) for x in runs["plastic"]],
                      "segments_diffuse": int(stats["diffuse"][0].segments), "segments_plastic": int(stats["plastic"][0].segments),
                      "ms_per_msegment_diffuse": round(ms0 / (stats["diffuse"][0].segments / 1e6), 4),
                      "ms_per_msegment_plastic": round(ms1 / (stats["plastic"][0].segments / 1e6), 4),
                      "finite": stats["plastic"][1], "mean_y_diffuse": round(stats["diffuse"][2], 5), "mean_y_plastic": round(stats["plastic"][2], 5)}), flush=True)


if __name__ == "__main__":
    main()
