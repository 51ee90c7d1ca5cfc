"""Point-to-line pose quality (include/icp_mi355x.h section 16), single and batched.
Single call: Icp2d.evaluate_point_to_line next to Icp2d.evaluate on the same handle, device-resident source, at the pose
a point-to-line registration returns -- on golden scans 001 -> 002 and on a 100 000 x 100 000 room outline.
Batch: IcpBatch.evaluate_point_to_line_packed on the golden pairs k -> k + 1, cycled, at batch sizes 1, 64 and 256, next
to IcpBatch.evaluate_packed on the same items (the point residual: no normals) and to serial single calls -- on handles
whose normals exist, and everything a batch item equals: a fresh handle, its normals, the score.
Median of --reps calls after a first one, as bench_line_batch.py.  Not the headline benchmark (bench.py); a tool for the
extension.  Prints one JSON line.

    python bench_line_quality.py [--reps R] [--k K] [--sizes 1,64,256] [--bound R]
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
    fn()  # (first use: buffers, the LDS grant, code objects)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def outline(rng, m, noise=2e-3):
    """m samples of the outline of a room with a partition, 2 mm off the walls (the scene of tests/test_line_abi.py)"""
    segs = np.array([[-3, -2, 3, -2], [3, -2, 3, 2], [3, 2, -3, 2], [-3, 2, -3, -2], [0, -2, 0, 0.5]], dtype=np.float64)
    d = segs[:, 2:] - segs[:, :2]
    length = np.hypot(d[:, 0], d[:, 1])
    which = rng.choice(len(segs), size=m, p=length / length.sum())
    t, off = rng.random(m), rng.normal(0.0, noise, m)
    nrm = np.stack([-d[:, 1], d[:, 0]], axis=1) / length[:, None]
    return np.ascontiguousarray(segs[which, :2] + t[:, None] * d[which] + off[:, None] * nrm[which])


def single_row(name, dst, src, k, bound, reps, iters):
    import torch

    icp = I.Icp2d(dst)
    icp.compute_line_normals(k)
    d_src = torch.from_numpy(src).cuda()
    T = icp.estimate_point_to_line(d_src, I.Transform(), iters)
    q, p = icp.evaluate_point_to_line(d_src, T, bound), icp.evaluate(d_src, T, bound)
    row = {"n": len(src), "m": len(dst), "fitness": q.fitness, "line_rmse": q.line_rmse, "point_rmse": p.inlier_rmse,
           "translation_eig": q.translation_eig.tolist()}
    med, lo, hi = timed(lambda: icp.evaluate_point_to_line(d_src, T, bound), reps)
    row["line_ms"], row["line_ms_min_max"] = med, [lo, hi]
    med, lo, hi = timed(lambda: icp.evaluate(d_src, T, bound), reps)
    row["point_ms"], row["point_ms_min_max"] = med, [lo, hi]
    row["line_over_point"] = row["line_ms"] / med
    icp.close()
    print(f"{name}: evaluate_point_to_line {row['line_ms']:.3f} ms, evaluate {row['point_ms']:.3f} ms "
          f"(x{row['line_over_point']:.2f}); line_rmse {q.line_rmse:.3g}, point rmse {p.inlier_rmse:.3g}",
          file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--k", type=int, default=8, help="neighbours of a line normal")
    ap.add_argument("--sizes", default="1,64,256")
    ap.add_argument("--bound", type=float, default=100.0, help="max correspondence distance on the golden scans (mm)")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_line_quality.py needs a GPU: the product path has no CPU fallback")
    I.build()
    g = os.path.join(ROOT, "tests", "golden", "scans2d")
    names = sorted(f for f in os.listdir(g) if f.endswith(".txt"))
    scans = [np.ascontiguousarray(load_scan2d(os.path.join(g, f))) for f in names]
    out = {"k": a.k, "reps": a.reps, "bound": a.bound, "scans": len(scans), "single": {}, "sizes": {}}

    out["single"]["golden_001_002"] = single_row("golden 001 -> 002", scans[1], scans[0], a.k, a.bound, a.reps, 20)
    Tt = I.Transform([0.03, -0.02, 0.01])
    big_dst = outline(np.random.default_rng(5), 100_000)
    big_src = outline(np.random.default_rng(1005), 100_000)
    r00, r10, r01, r11, tx, ty = Tt.inverse().pose.as_tuple()
    big_src = np.ascontiguousarray(np.stack([r00 * big_src[:, 0] + r01 * big_src[:, 1] + tx,
                                             r10 * big_src[:, 0] + r11 * big_src[:, 1] + ty], axis=1))
    out["single"]["outline_100k"] = single_row("outline 100k x 100k", big_dst, big_src, a.k, 0.05, a.reps, 6)

    pairs = len(scans) - 1
    first = np.cumsum([0] + [len(s) for s in scans])
    d_packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans))).cuda()
    d_scans = [torch.from_numpy(s).cuda() for s in scans]
    B = I.IcpBatch(2)
    # the poses scored: what the batched point-to-line registration returns for each pair
    reg = B.estimate_point_to_line_packed(
        d_packed, d_packed, [(int(first[i]), len(scans[i]), int(first[i + 1]), len(scans[i + 1]), I.Transform())
                             for i in range(pairs)], 20, a.k)

    def items_of(count):  # item i: scan i -> scan i + 1 (src, dst) at its registered pose, cycled over the pairs
        return [(int(first[i % pairs]), len(scans[i % pairs]), int(first[i % pairs + 1]), len(scans[i % pairs + 1]),
                 reg[i % pairs]) for i in range(count)]

    for count in [int(x) for x in a.sizes.split(",")]:
        items = items_of(count)
        row = {"points_first_item": [items[0][1], items[0][3]]}
        before = B.line_quality_counters()
        qs = B.evaluate_point_to_line_packed(d_packed, d_packed, items, a.k, a.bound)
        after = B.line_quality_counters()
        row["served_in_launch"], row["one_by_one"] = after[0] - before[0], after[1] - before[1]
        med, lo, hi = timed(lambda: B.evaluate_point_to_line_packed(d_packed, d_packed, items, a.k, a.bound), a.reps)
        row["line_batch_ms_per_call"], row["line_batch_ms_min_max"] = med, [lo, hi]
        row["line_batch_items_per_s"] = 1e3 * count / med
        med, lo, hi = timed(lambda: B.evaluate_packed(d_packed, d_packed, items, a.bound), a.reps)
        row["point_batch_ms_per_call"], row["point_batch_ms_min_max"] = med, [lo, hi]
        row["line_over_point_batch"] = row["line_batch_ms_per_call"] / med
        handles = {}
        for i in range(min(count, pairs)):
            handles[i] = I.Icp2d(scans[i + 1])
            handles[i].compute_line_normals(a.k)

        def serial_scores():
            for i in range(count):
                handles[i % pairs].evaluate_point_to_line(d_scans[i % pairs], reg[i % pairs], a.bound)

        med, lo, hi = timed(serial_scores, a.reps)
        row["serial_ms_per_call"], row["serial_ms_min_max"], row["serial_ms_per_item"] = med, [lo, hi], med / count
        single = handles[0].evaluate_point_to_line(d_scans[0], reg[0], a.bound)
        row["first_item_equals_single_call"] = bool(np.array_equal(qs[0].as_array(), single.as_array())
                                                    and qs[0].inliers == single.inliers)
        for h in handles.values():
            h.close()

        def serial_fresh():
            for i in range(count):
                h = I.Icp2d(d_scans[i % pairs + 1])
                h.compute_line_normals(a.k)
                h.evaluate_point_to_line(d_scans[i % pairs], reg[i % pairs], a.bound)
                h.close()

        if count <= 64:
            med, lo, hi = timed(serial_fresh, a.reps)
            row["serial_fresh_handle_ms_per_call"], row["serial_fresh_handle_ms_min_max"] = med, [lo, hi]
            row["serial_fresh_handle_ms_per_item"] = med / count
        out["sizes"][str(count)] = row
        print(f"B = {count}: line batch {row['line_batch_ms_per_call']:.3f} ms ({row['line_batch_items_per_s']:.0f} items/s), "
              f"point batch {row['point_batch_ms_per_call']:.3f} ms, serial single scores {row['serial_ms_per_call']:.3f} ms "
              f"({row['serial_ms_per_item']:.3f} per item)"
              + (f", with a fresh handle and its normals {row['serial_fresh_handle_ms_per_item']:.3f} per item"
                 if "serial_fresh_handle_ms_per_item" in row else ""), file=sys.stderr, flush=True)

    # one workgroup at the largest target count it serves (2048 targets: consecutive scans, concatenated)
    big = [(0, len(scans[0]), int(first[1]), 2048, I.Transform())]
    med, lo, hi = timed(lambda: B.evaluate_point_to_line_packed(d_packed, d_packed, big, a.k, a.bound), a.reps)
    med_p, lo_p, hi_p = timed(lambda: B.evaluate_packed(d_packed, d_packed, big, a.bound), a.reps)
    out["one_item_2048_targets"] = {"line_batch_ms": med, "line_batch_ms_min_max": [lo, hi], "point_batch_ms": med_p,
                                    "point_batch_ms_min_max": [lo_p, hi_p]}
    print(f"one item, m = 2048: line batch {med:.4f} ms, point batch {med_p:.4f} ms", file=sys.stderr, flush=True)
    out["line_quality_counters"] = list(B.line_quality_counters())
    B.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
