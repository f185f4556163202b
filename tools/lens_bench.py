#!/usr/bin/env python3
"""What a `thinlens` sensor costs (EXPERIMENTS.md, "The thinlens sensor"; GPU box).

    python tools/lens_bench.py [--steps 5] [--warmup 2] [--reps 3] [--mesh-size 1024] [--mesh-spp 128]

Two scenes — the Cornell box at 512 x 512 and 512 spp (bench.py's workload: diffuse only, so without a lens it runs its specialised
kernels and with one the top tier's) and the config-3-class mesh scene (a 70 k-triangle rough conductor) — each through the pinhole
and through a lens focused on the room's middle, under `path` and under `direct` at (1, 1): eight configurations, one scene object
each in one process, rendered --warmup + --steps times per repetition, the repetitions interleaved.  Prints one JSON line per
configuration: the median of msk_stats::ms_total over all timed renders, the repetitions' medians and their spread, the medians of
the per-kernel device times, and the lens' cost against the same build's pinhole render of the same scene."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LENS = (25.0, 1080.0)        # the Cornell box's units: the camera stands 800 in front of the box, whose middle is 280 inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mesh-size", type=int, default=1024)
    ap.add_argument("--mesh-spp", type=int, default=128)
    a = ap.parse_args()
    abi = importlib.import_module("misaki-render_amd.abi")
    hm = importlib.import_module("misaki-render_amd.hostmirror")
    ctx = abi.Context(0)
    scenes = {"cbox_512_512spp": (lambda: hm.cbox_scene(512, 512), 512), "mesh_c3_%d_%dspp" % (a.mesh_size, a.mesh_spp): (lambda: hm.bunny_class_scene(a.mesh_size), a.mesh_spp)}
    configs = []
    for name, (make, spp) in scenes.items():
        for lens in (False, True):
            flat = make()
            if lens:
                flat.lens = abi.LensDesc(*LENS)
            g = abi.Scene(ctx, flat)
            for integrator in ("path", "direct"):
                configs.append(dict(scene=name, lens=lens, integrator=integrator, g=g, prm=abi.render_params(spp=spp, seed=1), runs=[], rep_medians=[]))
    for _ in range(a.reps):
        for c in configs:
            timed = []
            for step in range(a.warmup + a.steps):
                film, st = c["g"].render(c["prm"]) if c["integrator"] == "path" else c["g"].render_direct(c["prm"], 1, 1)
                if step >= a.warmup:
                    timed.append({k: getattr(st, k) for k in ("ms_total", "ms_trace", "ms_shade", "ms_resolve")})
            c["runs"] += timed
            c["rep_medians"].append(statistics.median(r["ms_total"] for r in timed))
            c["samples"], c["segments"] = int(st.samples), int(st.segments)
    base = {(c["scene"], c["integrator"]): statistics.median(r["ms_total"] for r in c["runs"]) for c in configs if not c["lens"]}
    for c in configs:
        med = statistics.median(r["ms_total"] for r in c["runs"])
        out = {"scene": c["scene"], "integrator": c["integrator"], "lens": c["lens"], "median_ms": round(med, 3),
               "rep_medians_ms": [round(x, 3) for x in c["rep_medians"]], "spread_ms": round(max(c["rep_medians"]) - min(c["rep_medians"]), 3),
               "samples": c["samples"], "segments": c["segments"]}
        for k in ("ms_trace", "ms_shade", "ms_resolve"):
            out[k] = round(statistics.median(r[k] for r in c["runs"]), 3)
        if c["lens"]:
            out["against_pinhole"] = round(med / base[c["scene"], c["integrator"]], 4)
        print(json.dumps(out), flush=True)
    for c in configs:
        if c["integrator"] == "direct":
            c["g"].close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
