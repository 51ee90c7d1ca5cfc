"""Point-to-plane pose evaluation (Icp3d.evaluate_point_to_plane: include/icp_mi355x.h section 13) next to its
yardstick, Icp3d.evaluate on the same handle in the same process, and next to what a caller ran before it,
estimate_point_to_plane(..., 1) from the same pose.  Each with a device source and with a host source, median of five.
Not the headline benchmark (bench.py); a tool for the extension.

    python bench_quality_plane.py [--reps R]
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

NORMALS_K = 8


def timed(fn, reps):
    fn()  # (first use: buffers)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def single(label, icp, src, T, r, reps, out):
    """both evaluations at T and one outer point-to-plane iteration from T, device and host source"""
    import torch

    d_src = torch.from_numpy(src).cuda()
    row = {"points": [len(src), icp.m]}
    for name, fn in (("evaluate_point_to_plane", lambda s: icp.evaluate_point_to_plane(s, T, r)),
                     ("evaluate", lambda s: icp.evaluate(s, T, r)),
                     ("estimate_point_to_plane1", lambda s: icp.estimate_point_to_plane(s, T, 1))):
        row[name + "_device_ms"] = timed(lambda: fn(d_src), reps)
        row[name + "_host_ms"] = timed(lambda: fn(src), reps)
    row["plane_over_point_device"] = row["evaluate_point_to_plane_device_ms"] / row["evaluate_device_ms"]
    row["plane_over_point_host"] = row["evaluate_point_to_plane_host_ms"] / row["evaluate_host_ms"]
    q = icp.evaluate_point_to_plane(d_src, T, r)
    row["fitness"], row["plane_rmse"], row["translation_eig"] = q.fitness, q.plane_rmse, q.translation_eig.tolist()
    out[label] = row
    print(f"{label}: evaluate_point_to_plane {row['evaluate_point_to_plane_device_ms']:.3f} ms (host src "
          f"{row['evaluate_point_to_plane_host_ms']:.3f}), evaluate {row['evaluate_device_ms']:.3f} ms (host src "
          f"{row['evaluate_host_ms']:.3f}), ratio {row['plane_over_point_device']:.3f} (host src "
          f"{row['plane_over_point_host']:.3f}), estimate_point_to_plane(.., 1) "
          f"{row['estimate_point_to_plane1_device_ms']:.3f} ms (host src {row['estimate_point_to_plane1_host_ms']:.3f})",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    out = {}
    pk = synth.synthetic_scan3d_packets(150)  # bench.py's 28.8k-point frame against its neighbour
    s3, d3 = synth.remove_invalid_values(pk[:75]), synth.remove_invalid_values(pk[75:150])
    icp = I.Icp3d(d3)
    icp.compute_normals(NORMALS_K)
    T = icp.estimate_point_to_plane(s3, I.Transform(), 20)
    single("frame_28k_3d", icp, s3, T, 0.1, a.reps, out)
    icp.close()
    src, dst = synth.synthetic_pair(1_000_000, 1_000_000)  # bench.py's pair
    icp = I.Icp3d(dst)
    icp.compute_normals(NORMALS_K)
    T = icp.estimate_point_to_plane(src, I.Transform(), 20)
    single("pair_1M_x_1M_3d", icp, src, T, 0.1, a.reps, out)
    icp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
