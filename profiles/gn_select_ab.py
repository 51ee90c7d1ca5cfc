"""One build's side of profiles/gn_select_ab.txt: the full-key selection alone and behind an overflowed short pipeline,
and bench.py's reference-sized pair.  Run once per build and round, alternating, with ICP_MI355X_LIB naming the build's
library; prints one JSON line.

    ICP_MI355X_LIB=<libicp_mi355x.so of the build> python profiles/gn_select_ab.py <label>
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import icp_rust_amd as I  # noqa: E402


def run_at_the_median(n):
    """tests/test_gpu_parity.py: 30 % of the x residuals are one exact value on the median"""
    rng = np.random.default_rng(n)
    a = rng.normal(size=(n, 2)) * 10
    r = rng.normal(size=(n, 2)) * 0.2
    k = int(0.3 * n)
    r[:k, 0] = 0.0
    r[k:k + (n - k) // 2, 0] = -np.abs(r[k:k + (n - k) // 2, 0]) - 1e-3
    r[k + (n - k) // 2:, 0] = np.abs(r[k + (n - k) // 2:, 0]) + 1e-3
    return a, a - r


def timed(f, reps, warm=5):
    for _ in range(warm):
        f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    out = {"label": sys.argv[1] if len(sys.argv) > 1 else "", "lib": I._lib.LIB_PATH}
    T = I.Transform()
    for n in (10_000, 200_001):
        a, b = run_at_the_median(n)
        c0 = I.gn_path_counters()
        out[f"weighted_update_{n}"] = timed(lambda: I.weighted_gauss_newton_update(T, a, b), 40)
        c1 = I.gn_path_counters()
        out[f"weighted_update_{n}"]["full_key_evaluations"] = c1[3] - c0[3]  # (45: every call ends in one)
        out[f"residual_stddevs_{n}"] = timed(lambda: I.residual_stddevs(T, a, b), 40)
    import bench

    out["reference_sized"] = bench.reference_sized()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
