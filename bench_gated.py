"""Gated registration (Icp{2,3}d.estimate(..., max_correspondence_distance=r): include/icp_mi355x.h section 10) next
to the plain estimate on the same handle and source cloud: estimate, the gated call with r = +inf (the same bits, the
general path and no bet), the gated call with a finite r.  Not the headline benchmark (bench.py); a tool for the
extension.  Median of --reps calls (default five), device-resident source.

    python bench_gated.py [--reps R] [--iters K] [--only NAME]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import numpy as np

import icp_rust_amd as I
from icp_rust_amd import synth
from icp_rust_amd.scans import load_scan2d

G = os.path.join(ROOT, "tests", "golden", "scans2d")
INF = float("inf")


def timed(fn, reps):
    fn()  # (first use: buffers, window predictions)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def compare(label, icp, src, r, iters, reps, out):
    import torch

    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    T0 = I.Transform()
    _, inner, inl = icp.estimate(d_src, T0, iters, return_info="inner", max_correspondence_distance=r)
    row = {"points": [len(src), icp.m], "iters": iters, "r": r, "inliers_first_last": [int(inl[0]), int(inl[-1])],
           "inner": inner.tolist(),
           "estimate_ms": timed(lambda: icp.estimate(d_src, T0, iters), reps),
           "gated_inf_ms": timed(lambda: icp.estimate(d_src, T0, iters, max_correspondence_distance=INF), reps),
           "gated_r_ms": timed(lambda: icp.estimate(d_src, T0, iters, max_correspondence_distance=r), reps)}
    for k in ("estimate_ms", "gated_inf_ms", "gated_r_ms"):
        row[k.replace("_ms", "_ms_per_iter")] = row[k] / iters
    out[label] = row
    print(f"{label}: estimate {row['estimate_ms']:.3f} ms, gated inf {row['gated_inf_ms']:.3f} ms, gated r={r} "
          f"{row['gated_r_ms']:.3f} ms for {iters} iterations; inliers {row['inliers_first_last']}", flush=True)


def blob_scene(n_total, share=0.4, seed=5):
    """the room outline with a blob the target does not hold (tests/test_gpu_gated.py), scaled up"""
    rng = np.random.default_rng(seed)

    def walls(n):
        t = rng.random(n)
        side = rng.integers(0, 4, n)
        x = np.where(side == 0, t * 10, np.where(side == 1, 10.0, np.where(side == 2, t * 10, 0.0)))
        y = np.where(side == 0, 0.0, np.where(side == 1, t * 6, np.where(side == 2, 6.0, t * 6)))
        return np.stack([x, y], 1)

    k = int(n_total * share)
    dst = walls(n_total) + rng.normal(size=(n_total, 2)) * 0.005
    world = np.concatenate([walls(n_total - k) + rng.normal(size=(n_total - k, 2)) * 0.005,
                            np.array([4.0, 3.0]) + rng.normal(size=(k, 2)) * 0.4])
    inv = I.Transform([0.25, -0.15, 0.04]).inverse()
    p = inv.pose
    src = np.stack([(p.r00 * world[:, 0] + p.r01 * world[:, 1]) + p.tx,
                    (p.r10 * world[:, 0] + p.r11 * world[:, 1]) + p.ty], 1)
    return np.ascontiguousarray(rng.permutation(src)), np.ascontiguousarray(dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    out = {}

    def want(name):
        return a.only is None or a.only == name

    if want("pair_1M_x_1M_3d"):
        src, dst = synth.synthetic_pair(1_000_000, 1_000_000)  # bench.py's pair
        icp = I.Icp3d(dst)
        compare("pair_1M_x_1M_3d", icp, src, 0.5, a.iters, a.reps, out)
        icp.close()
    if want("frame_28k_3d"):
        pk = synth.synthetic_scan3d_packets(150)  # bench.py's 28.8k-point frame
        s3, d3 = synth.remove_invalid_values(pk[:75]), synth.remove_invalid_values(pk[75:150])
        icp = I.Icp3d(d3)
        compare("frame_28k_3d", icp, s3, 0.2, a.iters, a.reps, out)
        icp.close()
    if want("golden_2d"):
        icp = I.Icp2d(load_scan2d(f"{G}/002.txt"))  # (estimate: one launch; gated: the general path)
        compare("golden_2d", icp, load_scan2d(f"{G}/001.txt"), 500.0, a.iters, a.reps, out)
        icp.close()
    if want("blob_1M_2d"):
        src, dst = blob_scene(1_000_000)
        icp = I.Icp2d(dst)
        compare("blob_1M_2d", icp, src, 0.5, a.iters, a.reps, out)
        truth = I.Transform([0.25, -0.15, 0.04]).as_array()
        row = out["blob_1M_2d"]
        row["error_estimate"] = float(np.abs(icp.estimate(src, I.Transform(), a.iters).as_array() - truth).max())
        row["error_gated"] = float(np.abs(icp.estimate(src, I.Transform(), a.iters,
                                                       max_correspondence_distance=0.5).as_array() - truth).max())
        print(f"blob_1M_2d: error of estimate {row['error_estimate']:.4f}, gated {row['error_gated']:.4f}", flush=True)
        icp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
