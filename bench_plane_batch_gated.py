"""Gated batched point-to-plane registration (IcpBatch.estimate_point_to_plane_packed(...,
max_correspondence_distance=r): include/icp_mi355x.h section 19) on bench_plane_batch.py's items -- one synthetic frame
thinned to items of 1024 source and 2048 target points, item i every STRIDE-th point from offset i -- with a share of each
source lifted out of the targets' box (points the targets do not hold), from the identity, k = 8 neighbours, 20 outer
iterations, at batch sizes 1, 64 and 256, the clouds device-resident.  In the same process, on the same items: the gated
batch at a bound that bites (default: the third quartile of item 0's nearest-neighbour distances at the identity among
the points left in place) and at +inf, the ungated batch (section 18), and serial single gated calls
(Icp3d.estimate_point_to_plane with the same bound) on handles whose normals exist and on fresh handles (a fresh handle,
its normals, the estimate: everything a batch item equals).  The single calls are the reference.  With each size the
mean kept fraction per outer iteration, over the items.
Median of --reps calls after a first one, with min and max.  Not the headline benchmark (bench.py); a tool for the
extension.  Prints one JSON line.

    python bench_plane_batch_gated.py [--reps R] [--iters K] [--k K] [--bound R] [--share S] [--sizes 1,64,256]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import numpy as np

import icp_rust_amd as I
from bench_plane_batch import M_ITEM, N_ITEM, STRIDE, timed
from icp_rust_amd import synth

INF = float("inf")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--k", type=int, default=8, help="neighbours of a plane normal")
    ap.add_argument("--bound", type=float, default=None, help="maximum correspondence distance (default: see above)")
    ap.add_argument("--share", type=float, default=0.3, help="share of each source lifted out of the targets' box")
    ap.add_argument("--sizes", default="1,64,256")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_plane_batch_gated.py needs a GPU: the product path has no CPU fallback")
    I.build()
    frame_src, frame_dst = synth.synthetic_pair(N_ITEM * STRIDE, M_ITEM * STRIDE)
    rng = np.random.default_rng(19)
    lift = 1.5 * float(frame_dst[:, 2].max() - frame_dst[:, 2].min())
    srcs, kept_rows = [], None
    for i in range(STRIDE):
        s = np.ascontiguousarray(frame_src[i::STRIDE][:N_ITEM]).copy()
        moved = rng.permutation(N_ITEM)[:int(a.share * N_ITEM)]
        s[moved, 2] += lift
        if i == 0:
            kept_rows = np.setdiff1d(np.arange(N_ITEM), moved)
        srcs.append(s)
    dsts = [np.ascontiguousarray(frame_dst[i::STRIDE][:M_ITEM]) for i in range(STRIDE)]
    r = a.bound
    if r is None:
        d = srcs[0][kept_rows][:, None, :] - dsts[0][None, :, :]
        r = float(np.sqrt(np.quantile((d * d).sum(axis=2).min(axis=1), 0.75)))
    src_packed, dst_packed = np.ascontiguousarray(np.concatenate(srcs)), np.ascontiguousarray(np.concatenate(dsts))
    d_src, d_dst = torch.from_numpy(src_packed).cuda(), torch.from_numpy(dst_packed).cuda()
    d_srcs = [torch.from_numpy(s).cuda() for s in srcs]
    d_dsts = [torch.from_numpy(d).cuda() for d in dsts]
    T0 = I.Transform()
    B = I.IcpBatch(3)
    out = {"iters": a.iters, "k": a.k, "reps": a.reps, "bound": r, "lifted_share": a.share, "distinct_items": STRIDE,
           "sizes": {}}

    def items_of(count):  # item i: thinning i of the frame, cycled
        return [((i % STRIDE) * N_ITEM, N_ITEM, (i % STRIDE) * M_ITEM, M_ITEM, T0) for i in range(count)]

    def batch(items, bound, **kw):
        return B.estimate_point_to_plane_packed(d_src, d_dst, items, a.iters, a.k, max_correspondence_distance=bound, **kw)

    for count in [int(x) for x in a.sizes.split(",")]:
        items = items_of(count)
        row = {"points_first_item": [items[0][1], items[0][3]]}
        before = B.plane_gated_counters()
        Ts, _, inner, _, inl = batch(items, r, return_info=True)
        after = B.plane_gated_counters()
        row["served_in_launch"], row["one_by_one"] = after[0] - before[0], after[1] - before[1]
        row["inner_first_item"], row["inliers_first_item"] = inner[0].tolist(), inl[0].tolist()
        row["mean_kept_fraction_per_iteration"] = [round(float(x), 4) for x in (inl / float(N_ITEM)).mean(axis=0)]
        row["mean_kept_fraction"] = float((inl / float(N_ITEM)).mean())
        row["items_with_at_most_512_kept"] = int((inl.max(axis=1) <= 512).sum())
        med, lo, hi = timed(lambda: batch(items, r), a.reps)
        row["gated_batch_ms_per_call"], row["gated_batch_ms_min_max"] = med, [lo, hi]
        row["gated_batch_items_per_s"] = 1e3 * count / med
        med, lo, hi = timed(lambda: batch(items, INF), a.reps)
        row["gated_inf_batch_ms_per_call"], row["gated_inf_batch_ms_min_max"] = med, [lo, hi]
        med, lo, hi = timed(lambda: batch(items, None), a.reps)
        row["ungated_batch_ms_per_call"], row["ungated_batch_ms_min_max"] = med, [lo, hi]
        row["gated_over_ungated_batch"] = row["gated_batch_ms_per_call"] / med
        row["gated_inf_over_ungated_batch"] = row["gated_inf_batch_ms_per_call"] / med
        # serial single gated calls on the same items: handles with their normals ready ...
        handles = {}
        for i in range(min(count, STRIDE)):
            handles[i] = I.Icp3d(dsts[i])
            handles[i].compute_normals(a.k)

        def serial_gated():
            for i in range(count):
                handles[i % STRIDE].estimate_point_to_plane(d_srcs[i % STRIDE], T0, a.iters, max_correspondence_distance=r)

        med, lo, hi = timed(serial_gated, a.reps)
        row["serial_gated_ms_per_call"], row["serial_gated_ms_min_max"] = med, [lo, hi]
        row["serial_gated_ms_per_item"] = med / count
        row["serial_over_gated_batch"] = med / row["gated_batch_ms_per_call"]
        Tsingle = handles[0].estimate_point_to_plane(d_srcs[0], T0, a.iters, max_correspondence_distance=r)
        row["first_item_equals_single_call"] = bool(np.array_equal(Ts[0].as_array(), Tsingle.as_array()))
        for h in handles.values():
            h.close()

        # ... and everything a batch item equals: a fresh handle, its normals, the gated estimate
        def serial_fresh():
            for i in range(count):
                h = I.Icp3d(d_dsts[i % STRIDE])
                h.compute_normals(a.k)
                h.estimate_point_to_plane(d_srcs[i % STRIDE], T0, a.iters, max_correspondence_distance=r)
                h.close()

        med, lo, hi = timed(serial_fresh, a.reps)
        row["serial_fresh_handle_ms_per_call"], row["serial_fresh_handle_ms_min_max"] = med, [lo, hi]
        row["serial_fresh_handle_ms_per_item"] = med / count
        row["serial_fresh_over_gated_batch"] = med / row["gated_batch_ms_per_call"]
        out["sizes"][str(count)] = row
        print(f"B = {count}: gated batch {row['gated_batch_ms_per_call']:.3f} ms ({row['gated_batch_items_per_s']:.0f} "
              f"items/s), at +inf {row['gated_inf_batch_ms_per_call']:.3f} ms, ungated batch "
              f"{row['ungated_batch_ms_per_call']:.3f} ms, serial single gated calls {row['serial_gated_ms_per_call']:.3f} ms "
              f"({row['serial_gated_ms_per_item']:.3f} per item), on fresh handles "
              f"{row['serial_fresh_handle_ms_per_item']:.3f} per item; kept fraction {row['mean_kept_fraction']:.3f}",
              file=sys.stderr, flush=True)
    out["plane_gated_counters"] = list(B.plane_gated_counters())
    out["plane_counters"] = list(B.plane_counters())
    B.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
