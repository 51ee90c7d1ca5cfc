"""Neighbour queries of arbitrary points, radius counts and removal by mask (Icp3d.query / count_within / remove:
include/icp_mi355x.h section 24) next to what exists.  Every arm of a size in one process, alternating, median of --reps
(default five) after a dropped round.  One handle on --targets (default 1M) uniform 3-D points, one point per 0.1^3 on
average (bench_outlier.py's cloud); the queries are an independent uniform sample of the same box.
  lists    per query size and k in (8, 16): the device entry with its lanes in cell order (the per-call sort), in the
           caller's order, Icp3d.neighbours(k) over ALL targets on the same handle (the ideal: lanes in record order, no
           sort; its size is the target count, not the query size) and scipy's cKDTree.query with 16 workers, if scipy
           imports (the tree is built once, outside the timed region)
  counts   count_within(r = 0.1) with cap = 4 and with the full count, both orders; beside them the radius filter
           (remove_radius_outliers(0.1, 4)) on a fresh handle of the targets
  removal  remove(mask) of a random 10 % against crop() of a disc that removes the same share, each on a fresh handle
The handle's sort keeps the caller's order up to 65 536 points: below that only the caller-order arm exists.
Not the headline benchmark (bench.py); a tool for the extension.  Writes --out.

    python bench_query.py [--reps R] [--targets M] [--sizes 28800,120000,250000,500000,1000000] [--tree-max N] [--out FILE]
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
from bench_outlier import summary, uniform_cloud
from icp_rust_amd import synth

RADIUS, CAP, KS = 0.1, 4, (8, 16)
FULL = 0xFFFFFFFF
SORT_FROM = 65_537  # the handle's per-call sort orders nothing smaller
ORDERS = (("cell", 1), ("caller", -1))


def timed(icp, call):
    t0 = time.perf_counter()
    rc = call()
    assert rc == 0, rc
    icp.synchronize()
    return time.perf_counter() - t0


def query_rows(icp, p, n, reps, tree, out):
    import torch

    m = len(p)
    side = 0.1 * m ** (1.0 / 3.0)
    q = np.ascontiguousarray(np.random.default_rng(synth.SEED + 97 + n).uniform(0.0, side, (n, 3)))
    d_q = torch.from_numpy(q).cuda()
    d_idx = torch.empty((max(n, m), 16), dtype=torch.int32, device="cuda")
    d_d2 = torch.empty((max(n, m), 16), dtype=torch.float64, device="cuda")
    d_counts = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = I.lib()
    qp, ip, dp, cp = (C.c_void_p(x.data_ptr()) for x in (d_q, d_idx, d_d2, d_counts))
    orders = [o for o in ORDERS if o[0] == "caller" or n >= SORT_FROM]
    t = {}
    before = icp.query_counters()
    for rep in range(reps + 1):
        for k in KS:
            for name, force in orders:
                L.icp_query_force_order(icp._h, force)
                t.setdefault(f"lists{k}_{name}", []).append(
                    timed(icp, lambda: L.icp_query_neighbours_device(icp._h, qp, n, None, k, ip, dp)))
            t.setdefault(f"neighbours{k}_all_targets", []).append(
                timed(icp, lambda: L.icp_target_neighbours_device(icp._h, k, 0, m, ip, dp)))
            if tree is not None and (rep == 0 or n <= 120_000):
                t0 = time.perf_counter()
                tree.query(q, k=k, workers=16)
                t.setdefault(f"ckdtree{k}", []).append(time.perf_counter() - t0)
        for cap_name, cap in (("cap4", CAP), ("full", FULL)):
            for name, force in orders:
                L.icp_query_force_order(icp._h, force)
                t.setdefault(f"count_{cap_name}_{name}", []).append(
                    timed(icp, lambda: L.icp_count_within_device(icp._h, qp, n, None, RADIUS, cap, cp)))
    L.icp_query_force_order(icp._h, 0)
    after = icp.query_counters()
    row = {"targets": m, "queries": n, "radius": RADIUS, "cap": CAP,
           "calls_cell_order": after[0] - before[0], "calls_caller_order": after[1] - before[1],
           "mean_count": float(d_counts.cpu().numpy().view(np.uint32).mean())}
    row.update(summary(t))
    out[f"queries_{n}"] = row
    print(f"{n} queries against {m}: " + ", ".join(f"{k[:-3]} {v:.3f}" for k, v in row.items() if k.endswith("_ms")),
          flush=True)
    del d_q, d_idx, d_d2, d_counts
    torch.cuda.empty_cache()


def removal_rows(p, reps, out):
    import torch

    m = len(p)
    rng = np.random.default_rng(synth.SEED + 98)
    mask = rng.uniform(size=m) >= 0.1
    centre = p[:, :2].mean(0)
    crop_radius = float(np.quantile(np.hypot(p[:, 0] - centre[0], p[:, 1] - centre[1]), 0.9))
    d_p = torch.from_numpy(p).cuda()
    d_mask = torch.from_numpy(mask).cuda()
    torch.cuda.synchronize()
    t = {"remove_mask_host": [], "remove_mask_device": [], "crop": [], "radius_filter": []}
    removed = {}
    for rep in range(reps + 1):
        for name in t:
            fresh = I.Icp3d(d_p)
            fresh.synchronize()
            t0 = time.perf_counter()
            if name == "remove_mask_host":
                removed[name] = fresh.remove(mask)
            elif name == "remove_mask_device":
                removed[name] = fresh.remove(d_mask)
            elif name == "crop":
                removed[name] = fresh.crop(centre, crop_radius)
            else:
                removed[name] = fresh.remove_radius_outliers(RADIUS, CAP)
            t[name].append(time.perf_counter() - t0)
            if rep == 0:
                removed[name + "_counters"] = list(fresh.remove_counters() if name.startswith("remove") else
                                                   fresh.crop_counters() if name == "crop" else fresh.outlier_counters())
            fresh.close()
    row = {"targets": m, "removed": removed}
    row.update(summary(t))
    out["removal"] = row
    print(f"removal at {m}: " + ", ".join(f"{k[:-3]} {v:.3f}" for k, v in row.items() if k.endswith("_ms")) +
          f" (removed {removed})", flush=True)
    del d_p, d_mask
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--targets", type=int, default=1_000_000)
    ap.add_argument("--sizes", default="28800,120000,250000,500000,1000000")
    ap.add_argument("--tree-max", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    a = ap.parse_args()
    import torch

    out = {}
    p = uniform_cloud(synth.SEED + 95, a.targets)
    tree = None
    if a.targets <= a.tree_max:
        try:
            from scipy.spatial import cKDTree

            t0 = time.perf_counter()
            tree = cKDTree(p)
            out["ckdtree_build_ms"] = 1e3 * (time.perf_counter() - t0)
        except ImportError:
            pass
    d_p = torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    icp = I.Icp3d(d_p)
    for n in (int(x) for x in a.sizes.split(",") if x):
        query_rows(icp, p, n, a.reps, tree, out)
    icp.close()
    del d_p
    I.lib().icp_trim_pool()
    torch.cuda.empty_cache()
    removal_rows(p, a.reps, out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
