"""Batched point-to-plane registration (IcpBatch.estimate_point_to_plane_packed: include/icp_mi355x.h section 18) on small
3-D items: one synthetic frame (icp_rust_amd/synth.py) thinned to items of at most 1024 source and 2048 target points --
item i takes every STRIDE-th point from offset i -- from the identity, k = 8 neighbours, 20 outer iterations, at batch
sizes 1, 64 and 256, the clouds device-resident.  In the same process, on the same items: the point-residual batch
(IcpBatch.estimate_packed) and serial single calls (Icp3d.estimate_point_to_plane on a handle whose normals exist, and
the whole of what a batch item equals: a fresh handle, its normals, the estimate).  The relation to read is a batch of
one against the single call of the same item; the single call is the reference.  The cost of the in-kernel normals: a
batch of one whose source is a single point and that runs one outer iteration (box, target sort, normals, one search; no
inner loop), next to the point-residual batch of the same item (box, target sort, one search), at 668 and at 2048
targets (2048: the lists of only 128 targets fit beside the targets, sixteen rounds).
Median of --reps calls after a first one.  Not the headline benchmark (bench.py); a tool for the extension (DESIGN.md
section 9m).  Prints one JSON line.

    python bench_plane_batch.py [--reps R] [--iters K] [--k K] [--sizes 1,64,256]
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

STRIDE = 128
N_ITEM, M_ITEM = 1024, 2048


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
    ap.add_argument("--k", type=int, default=8, help="neighbours of a plane normal")
    ap.add_argument("--sizes", default="1,64,256")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_plane_batch.py needs a GPU: the product path has no CPU fallback")
    I.build()
    frame_src, frame_dst = synth.synthetic_pair(N_ITEM * STRIDE, M_ITEM * STRIDE)
    srcs = [np.ascontiguousarray(frame_src[i::STRIDE][:N_ITEM]) for i in range(STRIDE)]
    dsts = [np.ascontiguousarray(frame_dst[i::STRIDE][:M_ITEM]) for i in range(STRIDE)]
    src_packed, dst_packed = np.ascontiguousarray(np.concatenate(srcs)), np.ascontiguousarray(np.concatenate(dsts))
    d_src, d_dst = torch.from_numpy(src_packed).cuda(), torch.from_numpy(dst_packed).cuda()
    d_srcs = [torch.from_numpy(s).cuda() for s in srcs]
    d_dsts = [torch.from_numpy(d).cuda() for d in dsts]
    T0 = I.Transform()
    B = I.IcpBatch(3)
    out = {"iters": a.iters, "k": a.k, "reps": a.reps, "distinct_items": STRIDE, "sizes": {}}

    def items_of(count):  # item i: thinning i of the frame, cycled
        return [((i % STRIDE) * N_ITEM, N_ITEM, (i % STRIDE) * M_ITEM, M_ITEM, T0) for i in range(count)]

    for count in [int(x) for x in a.sizes.split(",")]:
        items = items_of(count)
        row = {"points_first_item": [items[0][1], items[0][3]]}
        before = B.plane_counters()
        Ts, _, inner, _ = B.estimate_point_to_plane_packed(d_src, d_dst, items, a.iters, a.k, return_info=True)
        after = B.plane_counters()
        row["served_in_launch"], row["one_by_one"] = after[0] - before[0], after[1] - before[1]
        row["inner_first_item"] = inner[0].tolist()
        med, lo, hi = timed(lambda: B.estimate_point_to_plane_packed(d_src, d_dst, items, a.iters, a.k), a.reps)
        row["plane_batch_ms_per_call"], row["plane_batch_ms_min_max"] = med, [lo, hi]
        row["plane_batch_items_per_s"] = 1e3 * count / med
        med, lo, hi = timed(lambda: B.estimate_packed(d_src, d_dst, items, a.iters), a.reps)
        row["point_batch_ms_per_call"], row["point_batch_ms_min_max"] = med, [lo, hi]
        row["plane_over_point_batch"] = row["plane_batch_ms_per_call"] / med
        # serial single calls on the same items: handles with their normals ready ...
        handles = {}
        for i in range(min(count, STRIDE)):
            handles[i] = I.Icp3d(dsts[i])
            handles[i].compute_normals(a.k)

        def serial_estimates():
            for i in range(count):
                handles[i % STRIDE].estimate_point_to_plane(d_srcs[i % STRIDE], T0, a.iters)

        med, lo, hi = timed(serial_estimates, a.reps)
        row["serial_estimate_ms_per_call"], row["serial_estimate_ms_min_max"] = med, [lo, hi]
        row["serial_estimate_ms_per_item"] = med / count
        Tsingle = handles[0].estimate_point_to_plane(d_srcs[0], T0, a.iters)
        row["first_item_equals_single_call"] = bool(np.array_equal(Ts[0].as_array(), Tsingle.as_array()))
        for h in handles.values():
            h.close()

        # ... and everything a batch item equals: a fresh handle, its normals, the estimate
        def serial_fresh():
            for i in range(count):
                h = I.Icp3d(d_dsts[i % STRIDE])
                h.compute_normals(a.k)
                h.estimate_point_to_plane(d_srcs[i % STRIDE], T0, a.iters)
                h.close()

        if count <= 64:
            med, lo, hi = timed(serial_fresh, a.reps)
            row["serial_fresh_handle_ms_per_call"], row["serial_fresh_handle_ms_min_max"] = med, [lo, hi]
            row["serial_fresh_handle_ms_per_item"] = med / count
        out["sizes"][str(count)] = row
        print(f"B = {count}: plane batch {row['plane_batch_ms_per_call']:.3f} ms ({row['plane_batch_items_per_s']:.0f} items/s), "
              f"point batch {row['point_batch_ms_per_call']:.3f} ms, serial single estimates "
              f"{row['serial_estimate_ms_per_call']:.3f} ms ({row['serial_estimate_ms_per_item']:.3f} per item)"
              + (f", with a fresh handle and its normals {row['serial_fresh_handle_ms_per_item']:.3f} per item"
                 if "serial_fresh_handle_ms_per_item" in row else ""), file=sys.stderr, flush=True)

    # the in-kernel normals: one source point, one outer iteration, at 668 targets and at the largest count a workgroup
    # serves
    for m in (668, M_ITEM):
        one = [(0, 1, 0, m, T0)]
        med_l, lo, hi = timed(lambda: B.estimate_point_to_plane_packed(d_src, d_dst, one, 1, a.k), a.reps)
        med_p, lo_p, hi_p = timed(lambda: B.estimate_packed(d_src, d_dst, one, 1), a.reps)
        out[f"normals_probe_{m}"] = {"targets": m, "plane_batch_ms": med_l, "plane_batch_ms_min_max": [lo, hi],
                                     "point_batch_ms": med_p, "point_batch_ms_min_max": [lo_p, hi_p],
                                     "in_kernel_normals_ms": med_l - med_p}
        print(f"normals probe (m = {m}, one source point, one iteration): plane batch {med_l:.4f} ms, point batch "
              f"{med_p:.4f} ms, difference {med_l - med_p:.4f} ms", file=sys.stderr, flush=True)
    out["plane_counters"] = list(B.plane_counters())
    B.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
