"""Gated point-to-plane registration (Icp3d.estimate_point_to_plane(..., max_correspondence_distance=r):
include/icp_mi355x.h section 12) next to the ungated call on the same handle, source cloud and start pose:
estimate_point_to_plane, the gated call with r = +inf (the same bits: the cost of the gate's two launches and its wait),
the gated call with a finite r.  Two settings: the 28.8k-point synthetic frame against its neighbour frame, and a
scan-to-map loop of its own against bench_map.py's map (every frame registered with the gated call, appended, the new
targets given normals) in which each frame is also timed the three ways from the pose the loop had reached.  Not the
headline benchmark (bench.py); a tool for the extension.  Median of --reps calls, device-resident
source.  The gate's own two launches are read from a kernel trace of a run of this script (k_plgate_stage,
k_plgate_place), e.g. with --only frame_28k.

    python bench_gated_plane.py [--reps R] [--iters K] [--only NAME] [--map-points M] [--frames F] [--k K]
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

INF = float("inf")


def timed(fn, reps):
    fn()  # (first use: buffers, window predictions)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def three_ways(icp, d_src, T0, r, iters, reps):
    _, _, inner, inl = icp.estimate_point_to_plane(d_src, T0, iters, return_info=True, max_correspondence_distance=r)
    row = {"points": [int(d_src.shape[0]), icp.target_count], "iters": iters, "r": r,
           "inliers_first_last": [int(inl[0]), int(inl[-1])], "inner": inner.tolist()}
    for key, fn in (("ungated", lambda: icp.estimate_point_to_plane(d_src, T0, iters)),
                    ("gated_inf", lambda: icp.estimate_point_to_plane(d_src, T0, iters, max_correspondence_distance=INF)),
                    ("gated_r", lambda: icp.estimate_point_to_plane(d_src, T0, iters, max_correspondence_distance=r))):
        med, lo, hi = timed(fn, reps)
        row[key + "_ms_per_iter"] = med / iters
        row[key + "_ms_per_iter_min_max"] = [lo / iters, hi / iters]
    return row


def show(label, row):
    print(f"{label}: per outer iteration: ungated {row['ungated_ms_per_iter']:.3f} ms, gated inf "
          f"{row['gated_inf_ms_per_iter']:.3f} ms, gated r={row['r']} {row['gated_r_ms_per_iter']:.3f} ms; inliers "
          f"{row['inliers_first_last']} of {row['points'][0]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, choices=[None, "frame_28k", "map"])
    ap.add_argument("--map-points", type=int, default=10_000_000)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--k", type=int, default=8, help="neighbours of a normal")
    ap.add_argument("--r", type=float, default=0.2)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_gated_plane.py needs a GPU: the product path has no CPU fallback")
    I.build()
    out = {}
    if a.only in (None, "frame_28k"):
        pk = synth.synthetic_scan3d_packets(150)  # bench.py's 28.8k-point frame and its neighbour
        s3, d3 = synth.remove_invalid_values(pk[:75]), synth.remove_invalid_values(pk[75:150])
        icp = I.Icp3d(d3)
        icp.compute_normals(a.k)
        d_src = torch.from_numpy(np.ascontiguousarray(s3)).cuda()
        out["frame_28k"] = three_ways(icp, d_src, I.Transform(), a.r, a.iters, a.reps)
        show("frame_28k", out["frame_28k"])
        icp.close()
    if a.only in (None, "map"):
        m0, chunk, frame_points = a.map_points, 1 << 20, 75 * 384
        d_map = torch.empty((m0, 3), dtype=torch.float64, device="cuda")
        for first in range(0, m0, chunk):  # bench_map.py's map
            cnt = min(chunk, m0 - first)
            d_map[first:first + cnt] = torch.from_numpy(synth.box_cloud(synth.SEED + 200, cnt, first=first)).cuda()
        motion = np.array([0.02, -0.01, 0.001])
        world = I.Icp3d(d_map)
        world.reserve(m0 + (a.frames + 1) * frame_points)
        del d_map
        world.compute_normals(a.k)
        rows, err = [], []
        T = I.Transform()
        for k in range(1, a.frames + 1):
            s, _ = synth.synthetic_pair(frame_points, 1, seed=synth.SEED + 300 + 2 * k, param=tuple(k * motion))
            d_scan = torch.from_numpy(s).cuda()
            rows.append(three_ways(world, d_scan, T, a.r, a.iters, a.reps))
            T = world.estimate_point_to_plane(d_scan, T, a.iters, max_correspondence_distance=a.r)
            err.append(float(np.max(np.abs(T.as_array() - I.Transform(tuple(k * motion)).as_array()))))
            world.append(d_scan, T)
            world.update_normals(a.k)
        row = {"frames": a.frames, "map_points_start": m0, "map_points_end": world.target_count, "iters": a.iters, "r": a.r,
               "points": rows[-1]["points"], "inliers_first_last": rows[-1]["inliers_first_last"],
               "pose_abs_err_vs_truth_per_frame": err}
        for key in ("ungated", "gated_inf", "gated_r"):
            per = [x[key + "_ms_per_iter"] for x in rows]
            row[key + "_ms_per_iter"] = float(np.median(per))
            row[key + "_ms_per_iter_min_max"] = [float(np.min(per)), float(np.max(per))]
        out["map"] = row
        show("map", row)
        world.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
