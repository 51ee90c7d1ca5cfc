"""Point-to-line registration for 2-D handles (Icp2d.estimate_point_to_line: include/icp_mi355x.h section 14) next to the
point-to-point estimate (Icp2d.estimate) on the same handle, source cloud and start pose.  Two settings: the golden scan
pair 001 -> 002 (650 x 668 points, the reference's own workload) and two independent samples of a synthetic room
outline at 100k x 100k.  Per setting: ms per call of both estimates (median of --reps, device-resident source), their
inner counts, the time of compute_line_normals, and the time of the CPU statement of the same registration (the numpy
restatement of the normals is not timed: the CPU statement is fed the device's normals).  Not the headline benchmark
(bench.py); a tool for the extension.  Prints one JSON line.

    python bench_line.py [--reps R] [--iters K] [--only NAME] [--points N] [--k K] [--no-cpu]
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
from icp_rust_amd.scans import load_scan2d


def timed(fn, reps):
    fn()  # (first use: buffers, window predictions)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def outline(rng, m, noise=2e-3):
    """m samples of the walls of a room ([-3, 3] x [-2, 2] and a partition), N(0, noise) off the wall"""
    segs = np.array([[-3, -2, 3, -2], [3, -2, 3, 2], [3, 2, -3, 2], [-3, 2, -3, -2], [0, -2, 0, 0.5]], dtype=np.float64)
    d = segs[:, 2:] - segs[:, :2]
    length = np.hypot(d[:, 0], d[:, 1])
    which = rng.choice(len(segs), size=m, p=length / length.sum())
    nrm = np.stack([-d[:, 1], d[:, 0]], axis=1) / length[:, None]
    p = segs[which, :2] + rng.random(m)[:, None] * d[which] + rng.normal(0.0, noise, m)[:, None] * nrm[which]
    return np.ascontiguousarray(p)


def cpu_statement_ms(dst, normals, src, iters):
    """the oracle's point-to-plane estimate on lifted clouds (tests/oracle_ffi.py), all cores for the search"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ffi as O

    lift = lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), 1))], axis=1))
    O.set_threads(os.cpu_count() if (os.cpu_count() or 1) < 16 else 16)
    try:
        tree = O.KdTree(lift(dst))
        n3, s3 = lift(normals), lift(src)
        t0 = time.perf_counter()
        rc, T, _, inner = O.p2pl_estimate(tree, n3, s3, O.transform_identity(), iters)
        ms = 1e3 * (time.perf_counter() - t0)
    finally:
        O.set_threads(1)
    assert rc == O.OK
    return ms, T.as_array(), inner.tolist()


def one_setting(dst, src, k, iters, reps, cpu, truth=None):
    import torch

    icp = I.Icp2d(dst)
    row = {"points": [len(src), len(dst)], "iters": iters, "k": k}
    med, lo, hi = timed(lambda: icp.compute_line_normals(k), reps)
    row["compute_line_normals_ms"], row["compute_line_normals_ms_min_max"] = med, [lo, hi]
    d_src = torch.from_numpy(src).cuda()
    T0 = I.Transform()
    Tl, _, inner_l = icp.estimate_point_to_line(d_src, T0, iters, return_info=True)
    Tp, inner_p = icp.estimate(d_src, T0, iters, return_info="inner")
    row["point_to_line_inner"], row["point_to_point_inner"] = inner_l.tolist(), inner_p.tolist()
    for key, fn in (("point_to_line", lambda: icp.estimate_point_to_line(d_src, T0, iters)),
                    ("point_to_point", lambda: icp.estimate(d_src, T0, iters))):
        med, lo, hi = timed(fn, reps)
        row[key + "_ms_per_call"], row[key + "_ms_per_call_min_max"] = med, [lo, hi]
    if truth is not None:
        row["point_to_line_abs_err_vs_truth"] = float(np.max(np.abs(Tl.as_array() - truth.as_array())))
        row["point_to_point_abs_err_vs_truth"] = float(np.max(np.abs(Tp.as_array() - truth.as_array())))
    if cpu:
        ms, oT, oinner = cpu_statement_ms(dst, icp.read_line_normals(), src, iters)
        row["cpu_statement_ms_per_call"] = ms
        row["cpu_statement_inner"] = oinner
        row["pose_abs_diff_vs_cpu_statement"] = float(np.max(np.abs(Tl.as_array() - oT)))
    icp.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, choices=[None, "golden_001_002", "outline"])
    ap.add_argument("--points", type=int, default=100_000, help="outline: points of the scan and of the target")
    ap.add_argument("--k", type=int, default=8, help="neighbours of a line normal")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU statement")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_line.py needs a GPU: the product path has no CPU fallback")
    I.build()
    out = {}
    if a.only in (None, "golden_001_002"):
        g = os.path.join(ROOT, "tests", "golden", "scans2d")
        src, dst = load_scan2d(os.path.join(g, "001.txt")), load_scan2d(os.path.join(g, "002.txt"))
        out["golden_001_002"] = one_setting(np.ascontiguousarray(dst), np.ascontiguousarray(src), a.k, a.iters, a.reps,
                                            not a.no_cpu)
    if a.only in (None, "outline"):
        Tt = I.Transform([0.03, -0.02, 0.01])
        dst = outline(np.random.default_rng(5), a.points)
        scan = outline(np.random.default_rng(1005), a.points)
        r00, r10, r01, r11, tx, ty = Tt.inverse().pose.as_tuple()
        src = np.ascontiguousarray(np.stack([(r00 * scan[:, 0] + r01 * scan[:, 1]) + tx,
                                             (r10 * scan[:, 0] + r11 * scan[:, 1]) + ty], axis=1))
        out["outline"] = one_setting(dst, src, a.k, a.iters, a.reps, not a.no_cpu, truth=Tt)
    for name, row in out.items():
        print(f"{name}: point-to-line {row['point_to_line_ms_per_call']:.3f} ms per call, point-to-point "
              f"{row['point_to_point_ms_per_call']:.3f} ms, normals {row['compute_line_normals_ms']:.3f} ms"
              + (f", CPU statement {row['cpu_statement_ms_per_call']:.1f} ms" if "cpu_statement_ms_per_call" in row else ""),
              file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
