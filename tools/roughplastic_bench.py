#!/usr/bin/env python3
"""Times a `roughplastic` scene against the same scene `plastic` and diffuse (EXPERIMENTS.md, "The roughplastic BSDF").

    python tools/roughplastic_bench.py [--size 512] [--spp 64] [--steps 5] [--warmup 2] [--alpha 0.1]

The Cornell box with every shape but the luminaire roughplastic (its own colour as the diffuse base under a GGX coat of 1.49 /
1.00028, nonlinear; k_shade_gen_m / k_wavefront_m) against the same box plastic (the delta coat, the same kernels) and the box as
it is (the diffuse-only family), in one process, alternated: device time of msk_gpu_render (msk_stats::ms_total), the median of
--steps renders after --warmup, and the same per million path segments.  One JSON line."""
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
    ap.add_argument("--alpha", type=float, default=0.1)
    args = ap.parse_args()
    abi = importlib.import_module("misaki-render_amd.abi")
    hm = importlib.import_module("misaki-render_amd.hostmirror")

    def coated(kind, **kw):
        meshes = hm.cbox_meshes()
        for m in meshes:
            if m.radiance is None:
                m.bsdf = dict({"type": kind, "diffuse_reflectance": tuple(m.reflectance), "nonlinear": True}, **kw)
        return hm.flatten(meshes, args.size, args.size)

    flats = {"diffuse": hm.cbox_scene(args.size, args.size), "plastic": coated("plastic"), "roughplastic": coated("roughplastic", alpha=args.alpha)}
    ctx = abi.Context(0)
    scenes = {name: abi.Scene(ctx, flat) for name, flat in flats.items()}
    prm = abi.render_params(spp=args.spp, seed=1)
    runs = {name: [] for name in scenes}
    stats = {}
    for step in range(args.warmup + args.steps):
        for name, g in scenes.items():
            film, st = g.render(prm)
            stats[name] = (st, bool(np.isfinite(film).all()), float(film[..., 1].sum() / film[..., 4].sum()))
            if step >= args.warmup:
                runs[name].append(st.ms_total)
    for g in scenes.values():
        g.close()
    ctx.close()
    ms = {name: statistics.median(r) for name, r in runs.items()}
    out = {"scene": "cbox", "size": args.size, "spp": args.spp, "alpha": args.alpha}
    for name in scenes:
        seg = int(stats[name][0].segments)
        out.update({"ms_" + name: round(ms[name], 3), "runs_" + name: [round(x, 3) for x in runs[name]], "segments_" + name: seg,
                    "ms_per_msegment_" + name: round(ms[name] / (seg / 1e6), 4), "mean_y_" + name: round(stats[name][2], 5)})
    out.update({"ratio_to_plastic": round(ms["roughplastic"] / ms["plastic"], 4), "ratio_to_diffuse": round(ms["roughplastic"] / ms["diffuse"], 4),
                "finite": stats["roughplastic"][1]})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
