"""Batched point-to-line registration (IcpBatch.estimate_point_to_line_packed: include/icp_mi355x.h section 15) on the
golden 2-D scans: consecutive pairs k -> k + 1, cycled, from the identity, k = 8 neighbours, 20 outer iterations, at batch
sizes 1, 64 and 256.  In the same process, on the same items: serial single calls (Icp2d.estimate_point_to_line on a
handle whose normals exist, device-resident source -- bench_line.py's figure -- and the whole of what a batch item equals:
a fresh handle, its normals, the estimate) and the point-residual batch (IcpBatch.estimate_packed).  The cost of the
in-kernel normals: a batch of one whose source is a single point and that runs one outer iteration (box, target sort,
normals, one search; no inner loop), next to the point-residual batch of the same item (box, target sort, one search),
at the first pair's target count and at 2048 targets.
Median of --reps calls after a first one, as bench_line.py.  Not the headline benchmark (bench.py); a tool for the
extension.  Prints one JSON line.

    python bench_line_batch.py [--reps R] [--iters K] [--k K] [--sizes 1,64,256]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--k", type=int, default=8, help="neighbours of a line normal")
    ap.add_argument("--sizes", default="1,64,256")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_line_batch.py needs a GPU: the product path has no CPU fallback")
    I.build()
    g = os.path.join(ROOT, "tests", "golden", "scans2d")
    names = sorted(f for f in os.listdir(g) if f.endswith(".txt"))
    scans = [np.ascontiguousarray(load_scan2d(os.path.join(g, f))) for f in names]
    pairs = len(scans) - 1
    first = np.cumsum([0] + [len(s) for s in scans])
    packed = np.ascontiguousarray(np.concatenate(scans))
    d_packed = torch.from_numpy(packed).cuda()
    d_scans = [torch.from_numpy(s).cuda() for s in scans]
    T0 = I.Transform()
    B = I.IcpBatch(2)
    out = {"iters": a.iters, "k": a.k, "reps": a.reps, "scans": len(scans), "sizes": {}}

    def items_of(count):  # item i: scan i -> scan i + 1 (src, dst), cycled over the pairs
        return [(int(first[i % pairs]), len(scans[i % pairs]), int(first[i % pairs + 1]), len(scans[i % pairs + 1]), T0)
                for i in range(count)]

    for count in [int(x) for x in a.sizes.split(",")]:
        items = items_of(count)
        row = {"points_first_item": [items[0][1], items[0][3]]}
        before = B.line_counters()
        Ts, _, inner, _ = B.estimate_point_to_line_packed(d_packed, d_packed, items, a.iters, a.k, return_info=True)
        after = B.line_counters()
        row["served_in_launch"], row["one_by_one"] = after[0] - before[0], after[1] - before[1]
        row["inner_first_item"] = inner[0].tolist()
        med, lo, hi = timed(lambda: B.estimate_point_to_line_packed(d_packed, d_packed, items, a.iters, a.k), a.reps)
        row["line_batch_ms_per_call"], row["line_batch_ms_min_max"] = med, [lo, hi]
        row["line_batch_pairs_per_s"] = 1e3 * count / med
        med, lo, hi = timed(lambda: B.estimate_packed(d_packed, d_packed, items, a.iters), a.reps)
        row["point_batch_ms_per_call"], row["point_batch_ms_min_max"] = med, [lo, hi]
        row["line_over_point_batch"] = row["line_batch_ms_per_call"] / med
        # serial single calls on the same items: handles with their normals ready (bench_line.py's figure) ...
        handles = {}
        for i in range(min(count, pairs)):
            handles[i] = I.Icp2d(scans[i + 1])
            handles[i].compute_line_normals(a.k)

        def serial_estimates():
            for i in range(count):
                handles[i % pairs].estimate_point_to_line(d_scans[i % pairs], T0, a.iters)

        med, lo, hi = timed(serial_estimates, a.reps)
        row["serial_estimate_ms_per_call"], row["serial_estimate_ms_min_max"] = med, [lo, hi]
        row["serial_estimate_ms_per_pair"] = med / count
        Tsingle = handles[0].estimate_point_to_line(d_scans[0], T0, a.iters)
        row["first_item_equals_single_call"] = bool(np.array_equal(Ts[0].as_array(), Tsingle.as_array()))
        for h in handles.values():
            h.close()

        # ... and everything a batch item equals: a fresh handle, its normals, the estimate
        def serial_fresh():
            for i in range(count):
                h = I.Icp2d(d_scans[i % pairs + 1])
                h.compute_line_normals(a.k)
                h.estimate_point_to_line(d_scans[i % pairs], T0, a.iters)
                h.close()

        if count <= 64:
            med, lo, hi = timed(serial_fresh, a.reps)
            row["serial_fresh_handle_ms_per_call"], row["serial_fresh_handle_ms_min_max"] = med, [lo, hi]
            row["serial_fresh_handle_ms_per_pair"] = med / count
        out["sizes"][str(count)] = row
        print(f"B = {count}: line batch {row['line_batch_ms_per_call']:.3f} ms ({row['line_batch_pairs_per_s']:.0f} pairs/s), "
              f"point batch {row['point_batch_ms_per_call']:.3f} ms, serial single estimates "
              f"{row['serial_estimate_ms_per_call']:.3f} ms ({row['serial_estimate_ms_per_pair']:.3f} per pair)"
              + (f", with a fresh handle and its normals {row['serial_fresh_handle_ms_per_pair']:.3f} per pair"
                 if "serial_fresh_handle_ms_per_pair" in row else ""), file=sys.stderr, flush=True)

    # the in-kernel normals at the first pair's target count: one source point, one outer iteration
    one = [(0, 1, int(first[1]), len(scans[1]), T0)]
    med_l, lo, hi = timed(lambda: B.estimate_point_to_line_packed(d_packed, d_packed, one, 1, a.k), a.reps)
    med_p, lo_p, hi_p = timed(lambda: B.estimate_packed(d_packed, d_packed, one, 1), a.reps)
    out["normals_probe"] = {"targets": len(scans[1]), "line_batch_ms": med_l, "line_batch_ms_min_max": [lo, hi],
                            "point_batch_ms": med_p, "point_batch_ms_min_max": [lo_p, hi_p],
                            "in_kernel_normals_ms": med_l - med_p}
    print(f"normals probe (m = {len(scans[1])}, one source point, one iteration): line batch {med_l:.4f} ms, point batch "
          f"{med_p:.4f} ms, difference {med_l - med_p:.4f} ms", file=sys.stderr, flush=True)
    # ... and at the largest target count a workgroup serves (2048 targets: consecutive scans, concatenated), where the
    # lists of only 320 targets fit beside the targets and the normals take seven rounds
    big = [(0, 1, int(first[1]), 2048, T0)]
    med_l, lo, hi = timed(lambda: B.estimate_point_to_line_packed(d_packed, d_packed, big, 1, a.k), a.reps)
    med_p, lo_p, hi_p = timed(lambda: B.estimate_packed(d_packed, d_packed, big, 1), a.reps)
    out["normals_probe_2048"] = {"targets": 2048, "line_batch_ms": med_l, "line_batch_ms_min_max": [lo, hi],
                                 "point_batch_ms": med_p, "point_batch_ms_min_max": [lo_p, hi_p],
                                 "in_kernel_normals_ms": med_l - med_p}
    print(f"normals probe (m = 2048, one source point, one iteration): line batch {med_l:.4f} ms, point batch "
          f"{med_p:.4f} ms, difference {med_l - med_p:.4f} ms", file=sys.stderr, flush=True)
    out["line_counters"] = list(B.line_counters())
    B.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
