"""Voxel thinning (icp.voxel_downsample, Icp3d.thin: include/icp_mi355x.h section 22) next to what a caller could do
before it existed.  Three parts, every arm of a part in one process, alternating, median of --reps (default five):
  call  the stand-alone device entry on a 3-D cloud of 28.8k, 120k, 1M and 10M points at a voxel size that keeps about
        a third, against (a) the numpy restatement of the rule on the host and (b) a torch-on-GPU statement a user could
        write (floor-divide, pack the cells into an int64 key, torch.unique + a scatter of the minimum index);
  thin  Icp3d.thin on a map of about 1M and 10M targets (one per voxel already) after an append of 28.8k points, against
        a fresh Icp3d on the kept tensor;
  loop  the scan-to-map loop with and without map_voxel: map size, ms per frame, and how far the paths part.
Not the headline benchmark (bench.py); a tool for the extension.

    python bench_voxel.py [--reps R] [--sizes 28800,120000,1000000,10000000] [--maps 1000000,10000000] [--frames F]
                          [--map-voxel V] [--only call|thin|loop]
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
from icp_rust_amd import harness, synth

VOXEL = 0.1


def uniform_cloud(seed, n, per_voxel):
    """n points uniform in a cube of n / per_voxel voxels of size VOXEL: the share of first points is
    (1 - exp(-per_voxel)) / per_voxel whatever n is (2.82 per voxel: about a third)"""
    side = VOXEL * (n / per_voxel) ** (1.0 / 3.0)
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(0.0, side, (n, 3)))


def by_numpy(p, v):
    ok = np.isfinite(p).all(axis=1)
    c = np.floor(p / v) + 0.0
    _, first = np.unique(c[ok], axis=0, return_index=True)
    return np.sort(np.flatnonzero(ok)[first])


def by_torch(d_p, v):
    """finite points whose cells fit an int64 key: what a user's own statement would assume"""
    import torch

    c = torch.floor(d_p / v).to(torch.int64)
    c -= c.min(dim=0).values
    span = c.max(dim=0).values + 1
    key = (c[:, 0] * span[1] + c[:, 1]) * span[2] + c[:, 2]
    uniq, inverse = torch.unique(key, return_inverse=True)
    first = torch.full((uniq.shape[0],), d_p.shape[0], dtype=torch.int64, device=d_p.device)
    first.scatter_reduce_(0, inverse, torch.arange(d_p.shape[0], device=d_p.device), reduce="amin")
    kept = first.sort().values
    return d_p[kept], kept


def call_rows(n, reps, out):
    import torch

    p = uniform_cloud(synth.SEED + 91, n, 2.82)
    d_p = torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    numpy_once = n >= 1_000_000  # (host only, nothing to warm, tens of seconds at 10M: one sample)
    t = {"device": [], "numpy": [], "torch": []}
    want = None
    for rep in range(reps + 1):  # (the first round warms the workspace and torch's allocator and is dropped)
        t0 = time.perf_counter()
        out_d, idx_d = I.voxel_downsample(d_p, VOXEL, return_index=True)  # (the entry waits for its stream)
        t["device"].append(time.perf_counter() - t0)
        if rep == 0 or not numpy_once:
            t0 = time.perf_counter()
            want = by_numpy(p, VOXEL)
            t["numpy"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        out_t, idx_t = by_torch(d_p, VOXEL)
        torch.cuda.synchronize()
        t["torch"].append(time.perf_counter() - t0)
        if rep == 0:
            assert np.array_equal(idx_d.cpu().numpy().view(np.uint32), want)
            assert torch.equal(idx_t, idx_d.long()) and torch.equal(out_t, out_d)
        del out_d, idx_d, out_t, idx_t
    row = {"points": n, "voxel": VOXEL, "kept": int(len(want))}
    for k, v in t.items():
        v = v if k == "numpy" and numpy_once else v[1:]
        row[k + "_ms"] = 1e3 * float(np.median(v))
        row[k + "_ms_all"] = [round(1e3 * x, 4) for x in v]
    out[f"call_{n}"] = row
    print(f"call {n}: kept {row['kept']} ({row['kept'] / n:.3f}), device entry {row['device_ms']:.3f} ms, numpy "
          f"{row['numpy_ms']:.1f} ms, torch statement {row['torch_ms']:.3f} ms", flush=True)
    del d_p
    I.lib().icp_trim_pool()
    torch.cuda.empty_cache()


def thin_rows(m, reps, out):
    import torch

    d_raw = torch.from_numpy(uniform_cloud(synth.SEED + 92, (3 * m) // 2, 0.8)).cuda()
    d_map = I.voxel_downsample(d_raw, VOXEL).clone()  # one per voxel already: about 1.03 m targets
    side = float(d_raw.max().item())
    del d_raw
    frame = np.ascontiguousarray(np.random.default_rng(synth.SEED + 93).uniform(0.0, side, (28_800, 3)))
    d_frame = torch.from_numpy(frame).cuda()
    d_kept = I.voxel_downsample(torch.cat([d_map, d_frame]), VOXEL).clone()
    torch.cuda.synchronize()
    t = {"thin": [], "fresh": []}
    paths = None
    for rep in range(reps + 1):
        icp = I.Icp3d(d_map)
        icp.append(d_frame)
        t0 = time.perf_counter()
        removed = icp.thin(VOXEL)
        t["thin"].append(time.perf_counter() - t0)
        paths = icp.thin_counters()
        assert icp.target_count == d_kept.shape[0] and removed == d_map.shape[0] + 28_800 - d_kept.shape[0]
        if rep == 0 and m <= 1_000_000:
            assert np.array_equal(icp.read_targets(), d_kept.cpu().numpy())
        icp.close()
        t0 = time.perf_counter()
        icp = I.Icp3d(d_kept)
        icp.synchronize()
        t["fresh"].append(time.perf_counter() - t0)
        icp.close()
    row = {"map": int(d_map.shape[0]), "appended": 28_800, "removed": int(removed),
           "thin_path": "moved" if paths == (1, 0) else "rebuilt"}
    for k, v in t.items():
        row[k + "_ms"] = 1e3 * float(np.median(v[1:]))
        row[k + "_ms_all"] = [round(1e3 * x, 4) for x in v[1:]]
    out[f"thin_{m}"] = row
    print(f"thin {row['map']} + 28800: removed {row['removed']}, thin ({row['thin_path']}) {row['thin_ms']:.3f} ms, fresh "
          f"Icp3d on the kept tensor {row['fresh_ms']:.3f} ms", flush=True)
    del d_map, d_kept, d_frame
    I.lib().icp_trim_pool()
    torch.cuda.empty_cache()


def loop_rows(frames, map_voxel, reps, out):
    pk = synth.synthetic_scan3d_packets(synth.PACKETS_PER_FRAME * (frames + 1))
    t = {"grow": [], "thinned": []}
    size, path = {}, {}
    for rep in range(reps + 1):
        for name, v in (("grow", None), ("thinned", map_voxel)):
            t0 = time.perf_counter()
            Ts, path[name], world = harness.run_scan_to_map(pk, max_iter=20, map_voxel=v)
            t[name].append(time.perf_counter() - t0)
            size[name] = world.target_count
            if v is not None:
                size["thins_moved_rebuilt"] = world.thin_counters()
            world.close()
    row = {"frames": frames, "map_voxel": map_voxel, "final_map": size,
           "path_max_abs_difference": float(np.max(np.abs(path["grow"] - path["thinned"])))}
    for k, v in t.items():
        row[k + "_ms_per_frame"] = 1e3 * float(np.median(v[1:])) / frames
    out["scan_to_map"] = row
    print(f"scan-to-map, {frames} frames: growing map {row['grow_ms_per_frame']:.2f} ms/frame ({size['grow']} points), "
          f"map_voxel {map_voxel} {row['thinned_ms_per_frame']:.2f} ms/frame ({size['thinned']} points; thins moved / "
          f"rebuilt {size['thins_moved_rebuilt']}); paths differ by at most {row['path_max_abs_difference']:.3e}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="28800,120000,1000000,10000000")
    ap.add_argument("--maps", default="1000000,10000000")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--map-voxel", type=float, default=0.05)
    ap.add_argument("--only", default=None, choices=[None, "call", "thin", "loop"])
    a = ap.parse_args()
    out = {}
    if a.only in (None, "call"):
        for n in (int(x) for x in a.sizes.split(",")):
            call_rows(n, a.reps, out)
    if a.only in (None, "thin"):
        for m in (int(x) for x in a.maps.split(",")):
            thin_rows(m, a.reps, out)
    if a.only in (None, "loop"):
        loop_rows(a.frames, a.map_voxel, a.reps, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
