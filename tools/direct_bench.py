#!/usr/bin/env python3
"""Times the "direct" integrator against "path" at max_depth = 2 (EXPERIMENTS.md, "The direct integrator").

    python tools/direct_bench.py [--size 512] [--spp 512] [--steps 3] [--scene cbox|mesh]

For each of (1, 1), (4, 4) and (16, 1): device time of msk_gpu_render_direct (msk_stats::ms_total, the median of --steps renders
after one warm-up), the rays it traced, and the time per BUDGETED ray ms / (samples (1 + N + M)); heavier settings render
spp / (1 + N + M) * 3 samples per pixel so that every row traces about the same number of rays.  First row: "path" with max_depth = 2
on the same scene and spp.  One JSON line per row."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--scene", choices=("cbox", "mesh"), default="cbox", help="mesh: the 70 k-triangle config-3-class scene (tree in HBM)")
    args = ap.parse_args()
    abi = importlib.import_module("misaki-render_amd.abi")
    hm = importlib.import_module("misaki-render_amd.hostmirror")
    flat = hm.cbox_scene(args.size, args.size) if args.scene == "cbox" else hm.bunny_class_scene(args.size)
    ctx = abi.Context(0)
    g = abi.Scene(ctx, flat)

    def timed(call):
        call()
        stats = [call()[1] for _ in range(args.steps)]
        return statistics.median(s.ms_total for s in stats), [round(s.ms_total, 2) for s in stats], stats[-1]

    prm = abi.render_params(spp=args.spp, seed=1, max_depth=2)
    ms, runs, st = timed(lambda: g.render(prm))
    print(json.dumps({"scene": args.scene, "integrator": "path max_depth=2", "spp": args.spp, "ms": round(ms, 2), "runs": runs, "samples": st.samples,
                      "rays": st.segments + st.shadow_rays, "ns_per_budgeted_ray": round(ms * 1e6 / (st.samples * 3), 4)}), flush=True)
    for n, m in ((1, 1), (4, 4), (16, 1)):
        spp = max(1, args.spp * 3 // (1 + n + m))
        p = abi.render_params(spp=spp, seed=1)
        ms, runs, st = timed(lambda: g.render_direct(p, n, m))
        print(json.dumps({"scene": args.scene, "integrator": "direct (%d, %d)" % (n, m), "spp": spp, "ms": round(ms, 2), "runs": runs, "samples": st.samples,
                          "rays": st.segments + st.shadow_rays, "launches": st.iterations,
                          "ns_per_budgeted_ray": round(ms * 1e6 / (st.samples * (1 + n + m)), 4)}), flush=True)
    g.close()
    ctx.close()


if __name__ == "__main__":
    main()
