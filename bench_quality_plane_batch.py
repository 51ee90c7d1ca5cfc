"""Batched point-to-plane pose quality (include/icp_mi355x.h section 20): IcpBatch.evaluate_point_to_plane_packed at batch
sizes 1, 64 and 256 on two classes of 3-D items thinned from one synthetic frame (icp_rust_amd/synth.py) -- the largest
item a workgroup serves (1024 source x 2048 target points: sixteen rounds of normals) and a patch of a few hundred
targets (512 x 300: one round) -- scored at the pose a batched point-to-plane registration returns.  Next to it, on the
same items: IcpBatch.evaluate_packed (the point residual: no normals), serial Icp3d.evaluate_point_to_plane on handles
whose normals are ready, and the serial sequence a batch item is defined by: a fresh handle, its normals, the score.
Median of --reps calls after a first one, with min and max, as bench_line_quality.py.  Not the headline benchmark
(bench.py); a tool for the extension.  Prints one JSON line.

    python bench_quality_plane_batch.py [--reps R] [--k K] [--sizes 1,64,256] [--bound R] [--iters I]
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
CLASSES = (("1024x2048", 1024, 2048), ("512x300", 512, 300))


def timed(fn, reps):
    fn()  # (first use: buffers, the LDS grant, code objects)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def bench_class(name, n_item, m_item, frame_src, frame_dst, a, sizes):
    import torch

    srcs = [np.ascontiguousarray(frame_src[i::STRIDE][:n_item]) for i in range(STRIDE)]
    dsts = [np.ascontiguousarray(frame_dst[i::STRIDE][:m_item]) for i in range(STRIDE)]
    d_src = torch.from_numpy(np.ascontiguousarray(np.concatenate(srcs))).cuda()
    d_dst = torch.from_numpy(np.ascontiguousarray(np.concatenate(dsts))).cuda()
    d_srcs = [torch.from_numpy(s).cuda() for s in srcs]
    d_dsts = [torch.from_numpy(d).cuda() for d in dsts]
    B = I.IcpBatch(3)
    # the poses scored: what the batched point-to-plane registration returns for each thinning
    reg = B.estimate_point_to_plane_packed(d_src, d_dst, [(i * n_item, n_item, i * m_item, m_item, I.Transform())
                                                          for i in range(STRIDE)], a.iters, a.k)

    def items_of(count):  # item i: thinning i of the frame at its registered pose, cycled
        return [((i % STRIDE) * n_item, n_item, (i % STRIDE) * m_item, m_item, reg[i % STRIDE]) for i in range(count)]

    out = {}
    for count in sizes:
        items = items_of(count)
        row = {"points_first_item": [n_item, m_item]}
        before = B.plane_quality_counters()
        qs = B.evaluate_point_to_plane_packed(d_src, d_dst, items, a.k, a.bound)
        after = B.plane_quality_counters()
        row["served_in_launch"], row["one_by_one"] = after[0] - before[0], after[1] - before[1]
        row["first_item"] = {"fitness": qs[0].fitness, "plane_rmse": qs[0].plane_rmse, "point_rmse": qs[0].inlier_rmse,
                             "translation_eig": qs[0].translation_eig.tolist()}
        med, lo, hi = timed(lambda: B.evaluate_point_to_plane_packed(d_src, d_dst, items, a.k, a.bound), a.reps)
        row["plane_batch_ms_per_call"], row["plane_batch_ms_min_max"] = med, [lo, hi]
        row["plane_batch_items_per_s"] = 1e3 * count / med
        med, lo, hi = timed(lambda: B.evaluate_packed(d_src, d_dst, items, a.bound), a.reps)
        row["point_batch_ms_per_call"], row["point_batch_ms_min_max"] = med, [lo, hi]
        row["plane_over_point_batch"] = row["plane_batch_ms_per_call"] / med
        # serial single calls on the same items: handles with their normals ready ...
        handles = {}
        for i in range(min(count, STRIDE)):
            handles[i] = I.Icp3d(dsts[i])
            handles[i].compute_normals(a.k)

        def serial_scores():
            for i in range(count):
                handles[i % STRIDE].evaluate_point_to_plane(d_srcs[i % STRIDE], reg[i % STRIDE], a.bound)

        med, lo, hi = timed(serial_scores, a.reps)
        row["serial_ms_per_call"], row["serial_ms_min_max"], row["serial_ms_per_item"] = med, [lo, hi], med / count
        single = handles[0].evaluate_point_to_plane(d_srcs[0], reg[0], a.bound)
        row["first_item_equals_single_call"] = bool(np.array_equal(qs[0].as_array(), single.as_array())
                                                    and qs[0].inliers == single.inliers)
        for h in handles.values():
            h.close()

        # ... and the sequence a batch item is defined by: a fresh handle, its normals, the score
        def serial_fresh():
            for i in range(count):
                h = I.Icp3d(d_dsts[i % STRIDE])
                h.compute_normals(a.k)
                h.evaluate_point_to_plane(d_srcs[i % STRIDE], reg[i % STRIDE], a.bound)
                h.close()

        med, lo, hi = timed(serial_fresh, a.reps)
        row["serial_fresh_handle_ms_per_call"], row["serial_fresh_handle_ms_min_max"] = med, [lo, hi]
        row["serial_fresh_handle_ms_per_item"] = med / count
        row["fresh_over_batch"] = med / row["plane_batch_ms_per_call"]
        out[str(count)] = row
        print(f"{name}, B = {count}: plane batch {row['plane_batch_ms_per_call']:.3f} ms "
              f"[{row['plane_batch_ms_min_max'][0]:.3f}, {row['plane_batch_ms_min_max'][1]:.3f}] "
              f"({row['plane_batch_items_per_s']:.0f} items/s), point batch {row['point_batch_ms_per_call']:.3f} ms, "
              f"serial scores on ready handles {row['serial_ms_per_call']:.3f} ms "
              f"({row['serial_ms_per_item']:.3f} per item), "
              f"serial fresh handles with normals {row['serial_fresh_handle_ms_per_call']:.3f} ms "
              f"({row['serial_fresh_handle_ms_per_item']:.3f} per item, x{row['fresh_over_batch']:.2f} the batch); "
              f"first item equals its single call: {row['first_item_equals_single_call']}", file=sys.stderr, flush=True)
    counters = list(B.plane_quality_counters())
    B.close()
    return out, counters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--k", type=int, default=8, help="neighbours of a plane normal")
    ap.add_argument("--sizes", default="1,64,256")
    ap.add_argument("--bound", type=float, default=0.5, help="max correspondence distance")
    ap.add_argument("--iters", type=int, default=20, help="outer iterations of the registration whose poses are scored")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_quality_plane_batch.py needs a GPU: the product path has no CPU fallback")
    I.build()
    frame_src, frame_dst = synth.synthetic_pair(1024 * STRIDE, 2048 * STRIDE)
    sizes = [int(x) for x in a.sizes.split(",")]
    out = {"k": a.k, "reps": a.reps, "bound": a.bound, "iters": a.iters, "distinct_items": STRIDE, "classes": {}}
    for name, n_item, m_item in CLASSES:
        rows, counters = bench_class(name, n_item, m_item, frame_src, frame_dst, a, sizes)
        out["classes"][name] = {"sizes": rows, "plane_quality_counters": counters}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
