"""Gated batched point-to-point registration (IcpBatch.estimate_packed(..., max_correspondence_distance=r):
include/icp_mi355x.h section 21) on the golden 2-D scans: the 39 consecutive pairs k -> k + 1, cycled, from the identity,
20 outer iterations, device-resident clouds, at batch sizes 1, 64 and 256.  In the same process, on the same items: the
ungated batch (section 8) and serial single gated calls (Icp2d.estimate with the same bound on a handle that exists,
device-resident source).  With each size the mean kept fraction per outer iteration, over the items.
Median of --reps calls after a first one, as bench_line_batch_gated.py.  Not the headline benchmark (bench.py); a tool for
the extension.  Prints one JSON line.

    python bench_batch_gated.py [--reps R] [--iters K] [--bound R | --bound inf] [--sizes 1,64,256]
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
    ap.add_argument("--bound", type=float, default=4.0,
                    help="maximum correspondence distance, in the scans' unit (4: about the median nearest-neighbour "
                         "distance of a consecutive pair at the identity -- the bound bites)")
    ap.add_argument("--sizes", default="1,64,256")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_gated.py needs a GPU: the product path has no CPU fallback")
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
    r = a.bound
    out = {"iters": a.iters, "reps": a.reps, "bound": r, "scans": len(scans), "pairs": pairs, "sizes": {}}

    def items_of(count):  # item i: scan i -> scan i + 1 (src, dst), cycled over the pairs
        return [(int(first[i % pairs]), len(scans[i % pairs]), int(first[i % pairs + 1]), len(scans[i % pairs + 1]), T0)
                for i in range(count)]

    def gated(items):
        return B.estimate_packed(d_packed, d_packed, items, a.iters, max_correspondence_distance=r)

    for count in [int(x) for x in a.sizes.split(",")]:
        items = items_of(count)
        row = {"points_first_item": [items[0][1], items[0][3]]}
        before = B.gated_counters()
        Ts, _, inner, _, inl = B.estimate_packed(d_packed, d_packed, items, a.iters, return_info=True,
                                                 max_correspondence_distance=r)
        after = B.gated_counters()
        row["served_in_launch"], row["one_by_one"] = after[0] - before[0], after[1] - before[1]
        row["inner_first_item"], row["inliers_first_item"] = inner[0].tolist(), inl[0].tolist()
        n_of = np.array([it[1] for it in items], dtype=np.float64)
        row["mean_kept_fraction_per_iteration"] = [round(float(x), 4) for x in (inl / n_of[:, None]).mean(axis=0)]
        row["mean_kept_fraction"] = float((inl / n_of[:, None]).mean())
        row["items_with_at_most_512_kept"] = int((inl.max(axis=1) <= 512).sum())
        med, lo, hi = timed(lambda: gated(items), a.reps)
        row["gated_batch_ms_per_call"], row["gated_batch_ms_min_max"] = med, [lo, hi]
        row["gated_batch_pairs_per_s"] = 1e3 * count / med
        med, lo, hi = timed(lambda: B.estimate_packed(d_packed, d_packed, items, a.iters), a.reps)
        row["ungated_batch_ms_per_call"], row["ungated_batch_ms_min_max"] = med, [lo, hi]
        row["gated_over_ungated_batch"] = row["gated_batch_ms_per_call"] / med
        # serial single gated calls on the same items: handles that exist
        handles = {i: I.Icp2d(scans[i + 1]) for i in range(min(count, pairs))}

        def serial_gated():
            for i in range(count):
                handles[i % pairs].estimate(d_scans[i % pairs], T0, a.iters, max_correspondence_distance=r)

        med, lo, hi = timed(serial_gated, a.reps)
        row["serial_gated_ms_per_call"], row["serial_gated_ms_min_max"] = med, [lo, hi]
        row["serial_gated_ms_per_pair"] = med / count
        row["serial_over_gated_batch"] = med / row["gated_batch_ms_per_call"]
        Tsingle = handles[0].estimate(d_scans[0], T0, a.iters, max_correspondence_distance=r)
        row["first_item_equals_single_call"] = bool(np.array_equal(Ts[0].as_array(), Tsingle.as_array()))
        for h in handles.values():
            h.close()
        out["sizes"][str(count)] = row
        print(f"B = {count}: gated batch {row['gated_batch_ms_per_call']:.3f} ms ({row['gated_batch_pairs_per_s']:.0f} "
              f"pairs/s), ungated batch {row['ungated_batch_ms_per_call']:.3f} ms, serial single gated calls "
              f"{row['serial_gated_ms_per_call']:.3f} ms ({row['serial_gated_ms_per_pair']:.3f} per pair); kept fraction "
              f"{row['mean_kept_fraction']:.3f}", file=sys.stderr, flush=True)
    out["gated_counters"] = list(B.gated_counters())
    B.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
