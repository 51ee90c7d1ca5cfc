"""The neighbour lists and the two outlier filters (Icp3d.neighbours / icp_target_neighbours_device,
remove_radius_outliers, remove_statistical_outliers: include/icp_mi355x.h section 23) next to what a caller can write
today.  Every arm of a size in one process, alternating, median of --reps (default five) after a dropped round:
  lists16 / lists32   the device entry at k = 16 (KMAX = 16) and k = 32 (KMAX = 32), all targets, record order
  radius / statistical the two filters on a fresh handle (its creation is not timed)
  torch               cdist + topk on the same GPU, where the m x m matrix fits (--torch-max points)
  ckdtree             scipy.spatial.cKDTree build + query(k = 17) on the host, if scipy imports (--tree-max points)
  order               at --order-size points: the list kernel over all targets (lanes in the order of the grid's sorted
                      records) against the same kernel over targets [1, m) (lanes in index order), a recorded A/B
The cloud: uniform, one point per 0.1^3 on average, so that a radius of 0.1 holds about five targets whatever the size.
Not the headline benchmark (bench.py); a tool for the extension.

    python bench_outlier.py [--reps R] [--sizes 28800,120000,1000000,10000000] [--torch-max N] [--tree-max N]
                            [--order-size N]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import numpy as np

import icp_rust_amd as I
from icp_rust_amd import synth

RADIUS, MIN_NEIGHBOURS, K, RATIO = 0.1, 4, 16, 2.0


def uniform_cloud(seed, n):
    side = 0.1 * n ** (1.0 / 3.0)
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(0.0, side, (n, 3)))


def lists_device(icp, k, first, count, d_idx, d_d2):
    rc = I.lib().icp_target_neighbours_device(icp._h, k, first, count, C.c_void_p(d_idx.data_ptr()),
                                              C.c_void_p(d_d2.data_ptr()))
    assert rc == 0, rc
    icp.synchronize()


def summary(t):
    row = {}
    for k, v in t.items():
        if len(v) > 1:
            row[k + "_ms"] = 1e3 * float(np.median(v[1:]))
            row[k + "_ms_all"] = [round(1e3 * x, 4) for x in v[1:]]
        elif v:
            row[k + "_ms"] = 1e3 * float(v[0])  # (a host arm measured once)
    return row


def size_rows(n, reps, torch_max, tree_max, out):
    import torch

    p = uniform_cloud(synth.SEED + 95, n)
    d_p = torch.from_numpy(p).cuda()
    d_idx = torch.empty((n, 32), dtype=torch.int32, device="cuda")
    d_d2 = torch.empty((n, 32), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    icp = I.Icp3d(d_p)
    t = {"lists16": [], "lists32": [], "radius": [], "statistical": [], "torch": [], "ckdtree": []}
    removed = {}
    for rep in range(reps + 1):
        for k in (16, 32):
            t0 = time.perf_counter()
            lists_device(icp, k, 0, n, d_idx, d_d2)
            t[f"lists{k}"].append(time.perf_counter() - t0)
            if rep == 0 and k == 16:
                first_rows = d_idx.view(-1)[:4 * 16].view(4, 16).cpu().numpy().copy()  # (rows of k entries)
        for name in ("radius", "statistical"):
            fresh = I.Icp3d(d_p)
            fresh.synchronize()
            t0 = time.perf_counter()
            removed[name] = fresh.remove_radius_outliers(RADIUS, MIN_NEIGHBOURS) if name == "radius" else \
                fresh.remove_statistical_outliers(K, RATIO)
            t[name].append(time.perf_counter() - t0)
            fresh.close()
        if n <= torch_max:
            t0 = time.perf_counter()
            d2t, idxt = torch.topk(torch.cdist(d_p, d_p), 17, dim=1, largest=False)
            torch.cuda.synchronize()
            t["torch"].append(time.perf_counter() - t0)
            del d2t, idxt
        if n <= tree_max and (rep == 0 or n <= 120_000):
            try:
                from scipy.spatial import cKDTree
            except ImportError:
                cKDTree = None
            if cKDTree is not None:
                t0 = time.perf_counter()
                dist, nb = cKDTree(p).query(p, k=17, workers=16)
                t["ckdtree"].append(time.perf_counter() - t0)
                if rep == 0:  # the same neighbourhoods wherever the tree's distances have no ties
                    assert np.mean(np.sort(nb[:4, :16], axis=1) == np.sort(first_rows.astype(np.int64), axis=1)) > 0.9
    icp.close()
    row = {"points": n, "radius": RADIUS, "min_neighbours": MIN_NEIGHBOURS, "k": K, "std_ratio": RATIO, "removed": removed}
    row.update(summary(t))
    out[f"size_{n}"] = row
    print(f"{n}: lists k=16 {row['lists16_ms']:.3f} ms, k=32 {row['lists32_ms']:.3f} ms, radius filter "
          f"{row['radius_ms']:.3f} ms (removed {removed['radius']}), statistical {row['statistical_ms']:.3f} ms (removed "
          f"{removed['statistical']}), torch cdist+topk {row.get('torch_ms', float('nan')):.3f} ms, cKDTree "
          f"{row.get('ckdtree_ms', float('nan')):.1f} ms", flush=True)
    del d_p, d_idx, d_d2
    I.lib().icp_trim_pool()
    torch.cuda.empty_cache()


def order_rows(n, reps, out):
    import torch

    d_p = torch.from_numpy(uniform_cloud(synth.SEED + 96, n)).cuda()
    d_idx = torch.empty((n, 32), dtype=torch.int32, device="cuda")
    d_d2 = torch.empty((n, 32), dtype=torch.float64, device="cuda")
    icp = I.Icp3d(d_p)
    t = {"record16": [], "index16": [], "record32": [], "index32": []}
    for rep in range(reps + 1):
        for k in (16, 32):
            for name, first in (("record", 0), ("index", 1)):
                t0 = time.perf_counter()
                lists_device(icp, k, first, n - first, d_idx, d_d2)
                t[f"{name}{k}"].append(time.perf_counter() - t0)
    icp.close()
    row = {"points": n}
    row.update(summary(t))
    out["order"] = row
    print(f"order at {n}: k=16 record {row['record16_ms']:.3f} ms / index {row['index16_ms']:.3f} ms; k=32 record "
          f"{row['record32_ms']:.3f} ms / index {row['index32_ms']:.3f} ms", flush=True)
    del d_p, d_idx, d_d2
    I.lib().icp_trim_pool()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="28800,120000,1000000,10000000")
    ap.add_argument("--torch-max", type=int, default=28_800)  # (the m x m matrix: 6.6 GB at 28.8k, 115 GB at 120k)
    ap.add_argument("--tree-max", type=int, default=1_000_000)
    ap.add_argument("--order-size", type=int, default=1_000_000)
    a = ap.parse_args()
    out = {}
    for n in (int(x) for x in a.sizes.split(",") if x):
        size_rows(n, a.reps, a.torch_max, a.tree_max, out)
    if a.order_size:
        order_rows(a.order_size, a.reps, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
