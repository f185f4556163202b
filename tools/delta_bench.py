#!/usr/bin/env python3
"""Times the point-light closed-form scene under two builds of the GPU library (EXPERIMENTS.md, "Spot and directional").

    python tools/delta_bench.py --ab "MSK_GPU_LIB=path/to/parent/libmsk_gpu.so" "" [--size 1024] [--spp 256] [--steps 5] [--warmup 2] [--reps 5]

The scene of tests/test_delta_light_mirror.py's closed form (a): one large diffuse plane under one point light, the camera of the
plane tests, `path` at max_depth = 2.  Every quoted group of K=V (an empty one: this build) is one configuration, run as its own
process, interleaved --reps times; a process renders --warmup + --steps times and reports msk_stats::ms_total of the timed ones.
Prints per configuration the median over all timed renders, the medians of its processes and their spread, and whether all films
were the same bits, with the medians of the per-kernel device times (msk_stats::ms_trace / ms_shade / ms_resolve; MSK_TIMING_EVERY is 1 by default)."""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAMERA = dict(fov=20.0, near=0.1, far=1000.0, origin=(0, 3, 8), target=(0, 0, 0), up=(0, 1, 0))


def run_once(a):
    import numpy as np
    abi = importlib.import_module("misaki-render_amd.abi")
    hm = importlib.import_module("misaki-render_amd.hostmirror")
    s = 50.0
    plane = hm.MeshSpec("plane", [((-s, 0, s), (s, 0, s), (s, 0, -s), (-s, 0, -s))], (0.6, 0.5, 0.4))
    flat = hm.flatten([plane], a.size, a.size, camera=CAMERA, points=[{"position": (0.7, 2.5, 0.4), "intensity": (30.0, 24.0, 18.0)}])
    ctx = abi.Context(0)
    g = abi.Scene(ctx, flat)
    prm = abi.render_params(spp=a.spp, seed=1, max_depth=2)
    runs = []
    for step in range(a.warmup + a.steps):
        film, st = g.render(prm)
        if step >= a.warmup:
            runs.append({"ms_total": st.ms_total, "ms_trace": st.ms_trace, "ms_shade": st.ms_shade, "ms_resolve": st.ms_resolve})
    g.close()
    ctx.close()
    print(json.dumps({"lib": abi.LIB_PATH, "runs": runs, "samples": int(st.samples), "shadow_rays": int(st.shadow_rays),
                      "film": hashlib.sha256(np.ascontiguousarray(film).tobytes()).hexdigest()[:16]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ab", nargs="+", default=None)
    a = ap.parse_args()
    if not a.ab:
        return run_once(a)
    res = {c: [] for c in a.ab}
    for _ in range(a.reps):
        for c in a.ab:
            env = dict(os.environ)
            for kv in c.split():
                k, v = kv.split("=", 1)
                env[k] = v
            cmd = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--spp", str(a.spp), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode:
                print("FAILED: %r rc %d %s" % (c, p.returncode, p.stderr[-400:]), flush=True)
                return 1
            res[c].append(json.loads(p.stdout.strip().split("\n")[-1]))
    films = {d["film"] for c in a.ab for d in res[c]}
    for c in a.ab:
        meds = [statistics.median(r["ms_total"] for r in d["runs"]) for d in res[c]]
        every = [r["ms_total"] for d in res[c] for r in d["runs"]]
        out = {"config": c or "(this build)", "lib": res[c][0]["lib"], "size": a.size, "spp": a.spp, "median_ms": round(statistics.median(every), 3),
               "process_medians_ms": [round(x, 3) for x in meds], "spread_ms": round(max(meds) - min(meds), 3), "min_ms": round(min(every), 3),
               "max_ms": round(max(every), 3), "shadow_rays": res[c][0]["shadow_rays"], "one_film": len(films) == 1}
        for k in ("ms_trace", "ms_shade", "ms_resolve"):
            out[k] = round(statistics.median(r[k] for d in res[c] for r in d["runs"]), 3)
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
