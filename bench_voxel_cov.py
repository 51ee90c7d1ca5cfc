"""Voxel covariances (icp.voxel_covariances: include/icp_mi355x.h section 26) next to the floor they cannot beat and to
what a caller could write without them.  Every arm of a row in one process, alternating, median of --reps (default five)
after a dropped warm-up round; every arm ends in a wait for the device before its clock stops.
  spread  a 3-D cloud of 28.8k, 1M and 10M points (bench_voxel.py: uniform_cloud, 2.82 points per voxel) through
          (a) voxel_covariances, device entry, packed covariances + means + counts;
          (b) voxel_centroids, device entry, means + counts: the floor -- the covariances run the same chain, and the
              second moments on top;
          (c) a torch statement on the same GPU: bench_voxel_mean.py's means (torch.unique + index_add_), then the
              deviations from them, their six products, a second index_add_ and the division (float atomics: its bits vary);
  heavy   2^23 points in ONE voxel beside 2^23 points spread as above: the second pass over the work lists.
Not the headline benchmark (bench.py); a tool for the extension.

    python bench_voxel_cov.py [--reps R] [--sizes 28800,1000000,10000000] [--heavy 8388608] [--ddof 1]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import numpy as np

import icp_rust_amd as I
from bench_voxel import VOXEL, uniform_cloud
from bench_voxel_mean import timed
from icp_rust_amd import synth

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def by_torch(d_p, v, ddof):
    """finite points whose cells fit an int64 key: what a user's own statement would assume; two passes, as the rule's;
    the voxels come in key order, not in the order of their first points"""
    import torch

    c = torch.floor(d_p / v).to(torch.int64)
    c -= c.min(dim=0).values
    span = c.max(dim=0).values + 1
    key = (c[:, 0] * span[1] + c[:, 1]) * span[2] + c[:, 2]
    uniq, inverse = torch.unique(key, return_inverse=True)
    k = uniq.shape[0]
    counts = torch.bincount(inverse, minlength=k)
    mean = torch.zeros((k, 3), dtype=d_p.dtype, device=d_p.device).index_add_(0, inverse, d_p) / counts[:, None].to(d_p.dtype)
    d = d_p - mean[inverse]
    prods = torch.stack([d[:, a] * d[:, b] for a, b in PAIRS], dim=1)
    sums = torch.zeros((k, 6), dtype=d_p.dtype, device=d_p.device).index_add_(0, inverse, prods)
    cov = sums / (counts - ddof).clamp(min=1)[:, None].to(d_p.dtype)
    return cov, mean, counts


def row_of(name, d_p, v, ddof, reps, out, with_torch=True):
    import torch

    n = d_p.shape[0]
    arms = {"covariances": lambda: I.voxel_covariances(d_p, v, ddof, return_counts=True, packed=True),
            "centroids": lambda: I.voxel_centroids(d_p, v, return_counts=True)}
    if with_torch:
        arms["torch"] = lambda: by_torch(d_p, v, ddof)
    t = {k: [] for k in arms}
    row = {"points": int(n), "voxel": v, "ddof": ddof}
    for rep in range(reps + 1):  # (the first round warms the workspace and torch's allocator and is dropped)
        res = {}
        for k, fn in arms.items():
            dt, res[k] = timed(fn)
            t[k].append(dt)
        if rep == 0:
            cov, mean, count = res["covariances"]
            row["voxels"] = int(mean.shape[0])
            row["largest_voxel"] = int(count.max().item())
            assert torch.equal(mean, res["centroids"][0]) and torch.equal(count, res["centroids"][1])
            if with_torch:  # the same voxels; aligned by the cell of the mean, the two agree to rounding
                t_cov, t_mean, _ = res["torch"]
                assert t_mean.shape[0] == mean.shape[0]

                def keyed(m):
                    c = torch.floor(m / v).to(torch.int64)
                    return torch.argsort((c[:, 0] * (1 << 40)) + (c[:, 1] * (1 << 20)) + c[:, 2])

                row["max_abs_difference_to_torch"] = float((cov[keyed(mean)] - t_cov[keyed(t_mean)]).abs().max().item())
        del res
    for k, v_ in t.items():
        row[k + "_ms"] = 1e3 * float(np.median(v_[1:]))
        row[k + "_ms_all"] = [round(1e3 * x, 4) for x in v_[1:]]
    row["covariances_over_centroids"] = row["covariances_ms"] / row["centroids_ms"]
    out[name] = row
    line = (f"{name}: {n} points, {row['voxels']} voxels (largest {row['largest_voxel']}): covariances "
            f"{row['covariances_ms']:.3f} ms, voxel_centroids {row['centroids_ms']:.3f} ms "
            f"(x {row['covariances_over_centroids']:.2f})")
    if with_torch:
        line += (f", torch statement {row['torch_ms']:.3f} ms (covariances / torch "
                 f"{row['covariances_ms'] / row['torch_ms']:.2f}; max |difference| {row['max_abs_difference_to_torch']:.2e})")
    print(line, flush=True)
    I.lib().icp_trim_pool()
    torch.cuda.empty_cache()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="28800,1000000,10000000")
    ap.add_argument("--heavy", type=int, default=1 << 23)
    ap.add_argument("--ddof", type=int, default=1, choices=(0, 1))
    a = ap.parse_args()
    out = {}
    for n in (int(x) for x in a.sizes.split(",")):
        d_p = torch.from_numpy(uniform_cloud(synth.SEED + 91, n, 2.82)).cuda()
        row_of(f"spread_{n}", d_p, VOXEL, a.ddof, a.reps, out)
        del d_p
    if a.heavy:
        n = a.heavy
        d_p = torch.from_numpy(uniform_cloud(synth.SEED + 94, n, 2.82)).cuda()
        row_of(f"spread_{n}", d_p, VOXEL, a.ddof, a.reps, out, with_torch=False)
        side = float(d_p.max().item())
        row_of(f"one_voxel_{n}", d_p, 2.0 * side, a.ddof, a.reps, out, with_torch=False)  # the same points, a v far too large
        del d_p
        ratio = out[f"one_voxel_{n}"]["covariances_ms"] / out[f"spread_{n}"]["covariances_ms"]
        out["one_voxel_over_spread"] = ratio
        print(f"one voxel of {n} points / the same points spread: x {ratio:.2f}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
