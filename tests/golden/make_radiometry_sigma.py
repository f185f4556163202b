#!/usr/bin/env python3
"""Writes tests/golden/radiometry_sigma.json: the per-sample standard deviation of X, Y, Z of every scenario of
tests/test_radiometry_closed_form.py, per group of pixels that share an expectation, measured on the CPU oracle with at least
2^20 samples per group.  It is the one measured input of that module's tolerance (sigma / sqrt(N)); the means are recorded
for orientation only, no test reads them.  Seeds differ from the tests' own."""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SAMPLES = 1 << 20


def main():
    abi = importlib.import_module("misaki-render_amd.abi")
    hm = importlib.import_module("misaki-render_amd.hostmirror")
    import oracle_binding
    import test_radiometry_closed_form as T
    side = T.CpuSide(oracle_binding.load(), abi)
    out = {}
    for name in sorted(T.CASES):
        case = T.CASES[name](hm)
        sc = side.scene(case.flat)
        largest = max(len(g) for g in case.groups)
        smallest = min(len(g) for g in case.groups)
        spp = 1 << 12
        seeds = [977 + k for k in range(-(-SAMPLES // (spp * smallest)))]

        def one(job):
            i, seed = job
            xyz, _ = sc.sample_pixels(abi.render_params(spp, seed=seed, **case.params), case.pixels[i][None])
            x = xyz[0].astype(np.float64)
            return i, x.sum(0), (x * x).sum(0)
        s1, s2 = np.zeros((len(case.pixels), 3)), np.zeros((len(case.pixels), 3))
        for i, a, b in side.pool.map(one, [(i, seed) for seed in seeds for i in range(len(case.pixels))]):
            s1[i] += a
            s2[i] += b
        sc.close()
        sigma, mean = [], []
        for g in case.groups:
            n = len(g) * len(seeds) * spp
            m = s1[g].sum(0) / n
            sigma.append(np.sqrt(np.maximum(s2[g].sum(0) / n - m * m, 0.0) * n / (n - 1)).tolist())
            mean.append(m.tolist())
        out[name] = {"samples": smallest * len(seeds) * spp, "sigma": sigma, "mean": mean}
        print(name, largest * len(seeds) * spp, np.round(np.array(sigma) / np.array(mean), 3).tolist(), flush=True)
    json.dump(out, open(os.path.join(HERE, "radiometry_sigma.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
