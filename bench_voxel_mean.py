"""Voxel centroids (icp.voxel_centroids: include/icp_mi355x.h section 25) next to the floor it cannot beat and to what
a caller could write without it.  Every arm of a row in one process, alternating, median of --reps (default five) after a
dropped warm-up round; every arm ends in a wait for the device before its clock stops.
  spread  a 3-D cloud of 28.8k, 1M and 10M points (bench_voxel.py: uniform_cloud, 2.82 points per voxel) through
          (a) voxel_centroids, device entry, means + counts;
          (b) voxel_downsample, device entry: the floor -- the centroids run the same table, marks and compaction, and more;
          (c) a torch statement on the same GPU: floor-divide, the cells packed into an int64 key,
              torch.unique(return_inverse), index_add_ of the points, bincount, divide (float atomics: its bits vary);
  heavy   2^23 points in ONE voxel beside 2^23 points spread as above: a voxel far too large must be folded by the
          whole machine, not by one workgroup.
Not the headline benchmark (bench.py); a tool for the extension.

    python bench_voxel_mean.py [--reps R] [--sizes 28800,1000000,10000000] [--heavy 8388608]
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
from bench_voxel import VOXEL, uniform_cloud
from icp_rust_amd import synth


def by_torch(d_p, v):
    """finite points whose cells fit an int64 key: what a user's own statement would assume; the voxels come in key
    order, not in the order of their first points"""
    import torch

    c = torch.floor(d_p / v).to(torch.int64)
    c -= c.min(dim=0).values
    span = c.max(dim=0).values + 1
    key = (c[:, 0] * span[1] + c[:, 1]) * span[2] + c[:, 2]
    uniq, inverse = torch.unique(key, return_inverse=True)
    sums = torch.zeros((uniq.shape[0], d_p.shape[1]), dtype=d_p.dtype, device=d_p.device)
    sums.index_add_(0, inverse, d_p)
    counts = torch.bincount(inverse, minlength=uniq.shape[0])
    return sums / counts[:, None].to(d_p.dtype), counts


def timed(fn):
    import torch

    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def row_of(name, d_p, v, reps, out, with_torch=True):
    import torch

    n = d_p.shape[0]
    arms = {"centroids": lambda: I.voxel_centroids(d_p, v, return_counts=True),
            "downsample": lambda: I.voxel_downsample(d_p, v)}
    if with_torch:
        arms["torch"] = lambda: by_torch(d_p, v)
    t = {k: [] for k in arms}
    row = {"points": int(n), "voxel": v}
    for rep in range(reps + 1):  # (the first round warms the workspace and torch's allocator and is dropped)
        res = {}
        for k, fn in arms.items():
            dt, res[k] = timed(fn)
            t[k].append(dt)
        if rep == 0:
            mean, count = res["centroids"]
            row["voxels"] = int(mean.shape[0])
            row["largest_voxel"] = int(count.max().item())
            assert res["downsample"].shape[0] == mean.shape[0] and int(count.long().sum().item()) == n
            if with_torch:  # the same voxels; aligned by the cell of the mean, the two agree to rounding
                t_mean, t_count = res["torch"]
                assert t_mean.shape[0] == mean.shape[0]

                def keyed(m):
                    c = torch.floor(m / v).to(torch.int64)
                    return torch.argsort((c[:, 0] * (1 << 40)) + (c[:, 1] * (1 << 20)) + c[:, 2])

                row["max_abs_difference_to_torch"] = float((mean[keyed(mean)] - t_mean[keyed(t_mean)]).abs().max().item())
        del res
    for k, v_ in t.items():
        row[k + "_ms"] = 1e3 * float(np.median(v_[1:]))
        row[k + "_ms_all"] = [round(1e3 * x, 4) for x in v_[1:]]
    row["centroids_over_downsample"] = row["centroids_ms"] / row["downsample_ms"]
    out[name] = row
    line = (f"{name}: {n} points, {row['voxels']} voxels (largest {row['largest_voxel']}): centroids "
            f"{row['centroids_ms']:.3f} ms, voxel_downsample {row['downsample_ms']:.3f} ms "
            f"(x {row['centroids_over_downsample']:.2f})")
    if with_torch:
        line += (f", torch statement {row['torch_ms']:.3f} ms (centroids / torch {row['centroids_ms'] / row['torch_ms']:.2f}; "
                 f"max |difference| {row['max_abs_difference_to_torch']:.2e})")
    print(line, flush=True)
    I.lib().icp_trim_pool()
    torch.cuda.empty_cache()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="28800,1000000,10000000")
    ap.add_argument("--heavy", type=int, default=1 << 23)
    a = ap.parse_args()
    out = {}
    for n in (int(x) for x in a.sizes.split(",")):
        d_p = torch.from_numpy(uniform_cloud(synth.SEED + 91, n, 2.82)).cuda()
        row_of(f"spread_{n}", d_p, VOXEL, a.reps, out)
        del d_p
    if a.heavy:
        n = a.heavy
        d_p = torch.from_numpy(uniform_cloud(synth.SEED + 94, n, 2.82)).cuda()
        row_of(f"spread_{n}", d_p, VOXEL, a.reps, out, with_torch=False)
        side = float(d_p.max().item())
        row_of(f"one_voxel_{n}", d_p, 2.0 * side, a.reps, out, with_torch=False)  # the same points, a v far too large
        del d_p
        ratio = out[f"one_voxel_{n}"]["centroids_ms"] / out[f"spread_{n}"]["centroids_ms"]
        out["one_voxel_over_spread"] = ratio
        print(f"one voxel of {n} points / the same points spread: x {ratio:.2f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
