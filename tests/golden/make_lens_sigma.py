#!/usr/bin/env python3
"""Writes tests/golden/lens_sigma.json: the per-sample standard deviation of X, Y, Z of the furnace of
tests/test_thinlens.py::test_a_lens_does_not_change_radiance under the "direct" integrator at (1, 1), measured on the CPU oracle's
`direct` with 2^20 samples, as make_radiometry_sigma.py measures the "path" scenarios.  It is measured through the
pinhole: the furnace's radiance is the same from every point and in every direction, so the pinhole's samples have the distribution
the lens' have.  The
mean is recorded for orientation only; no test reads it.  Seeds differ from the tests' own."""
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
NAME = "S3_cube_rho0.5_depth3_rr5"


def main():
    abi = importlib.import_module("misaki-render_amd.abi")
    hm = importlib.import_module("misaki-render_amd.hostmirror")
    import oracle_binding
    import test_radiometry_closed_form as T
    case = T.CASES[NAME](hm)
    sc = oracle_binding.load().scene(case.flat)
    spp = 1 << 12
    n_seeds = -(-SAMPLES // (spp * len(case.pixels)))
    s1, s2 = np.zeros(3), np.zeros(3)
    for seed in range(977, 977 + n_seeds):
        xyz, _ = sc.sample_pixels_direct(abi.render_params(spp, seed=seed, **case.params), case.pixels, 1, 1)
        x = xyz.reshape(-1, 3).astype(np.float64)
        s1 += x.sum(0)
        s2 += (x * x).sum(0)
    sc.close()
    n = n_seeds * spp * len(case.pixels)
    m = s1 / n
    sigma = np.sqrt(np.maximum(s2 / n - m * m, 0.0) * n / (n - 1))
    out = {NAME + "_direct": {"samples": n, "sigma": [sigma.tolist()], "mean": [m.tolist()]}}
    print(out)
    json.dump(out, open(os.path.join(HERE, "lens_sigma.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
