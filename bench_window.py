"""The sliding-window map (Icp3d.crop: include/icp_mi355x.h section 11) next to the two things a caller could do
before it existed, on the same cloud: (a) a fresh Icp3d on the kept points (a device tensor: create + full build of the
grid), (b) compaction followed by a full build_grid -- the crop's own rebuild path, forced by a handle whose grid was
chosen for 1.4 x as many points (built with a far-away block that a first crop removed by moving the records).  A thin
crop (about 7 % removed) and a deep one (half removed; always a rebuild), at 1M and 10M targets, 3-D.  All arms in one
process, alternating, median of --reps (default five).  Then the scan-to-map loop with and without map_radius.
Not the headline benchmark (bench.py); a tool for the extension.

    python bench_window.py [--reps R] [--sizes 1000000,10000000] [--frames F] [--only crop|loop]
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


def crop_rows(m, reps, out):
    import torch

    cloud = synth.box_cloud(synth.SEED + 71, m)
    d2 = cloud[:, 0] * cloud[:, 0] + cloud[:, 1] * cloud[:, 1]
    extra = synth.box_cloud(synth.SEED + 72, (2 * m) // 5) + np.array([500.0, 0.0, 0.0])
    d_cloud = torch.from_numpy(cloud).cuda()
    d_both = torch.from_numpy(np.ascontiguousarray(np.concatenate([cloud, extra]))).cuda()
    del extra
    center = (0.0, 0.0)
    for case, share in (("thin", 0.93), ("deep", 0.5)):
        radius = float(np.sqrt(np.quantile(d2, share)))
        mask = d2 <= radius * radius
        d_kept = torch.from_numpy(np.ascontiguousarray(cloud[mask])).cuda()
        torch.cuda.synchronize()
        t = {"crop": [], "fresh": [], "rebuild": []}
        paths = {}
        for rep in range(reps + 1):  # (the first round warms the pool's buffers and is dropped)
            # the crop as shipped
            icp = I.Icp3d(d_cloud)
            t0 = time.perf_counter()
            removed = icp.crop(center, radius)
            t["crop"].append(time.perf_counter() - t0)
            paths["crop"] = icp.crop_counters()
            assert removed == m - int(mask.sum())
            if rep == 0:
                assert np.array_equal(icp.read_targets(), cloud[mask])
            icp.close()
            # (a) what a caller did before: a fresh handle on the kept points
            t0 = time.perf_counter()
            icp = I.Icp3d(d_kept)
            t["fresh"].append(time.perf_counter() - t0)
            icp.close()
            # (b) compaction + build_grid: the same cloud in a handle whose cell size is due for a re-tune
            icp = I.Icp3d(d_both)
            assert icp.crop(center, 200.0) == (2 * m) // 5 and icp.crop_counters() == (1, 0)
            t0 = time.perf_counter()
            icp.crop(center, radius)
            t["rebuild"].append(time.perf_counter() - t0)
            paths["rebuild"] = icp.crop_counters()
            assert paths["rebuild"] == (1, 1)
            icp.close()
        row = {"targets": m, "radius": radius, "removed": m - int(mask.sum()),
               "crop_path": "moved" if paths["crop"] == (1, 0) else "rebuilt"}
        for k, v in t.items():
            row[k + "_ms"] = 1e3 * float(np.median(v[1:]))
            row[k + "_ms_all"] = [round(1e3 * x, 4) for x in v[1:]]
        out[f"{case}_{m}"] = row
        print(f"{case} {m}: removed {row['removed']}, crop ({row['crop_path']}) {row['crop_ms']:.3f} ms, "
              f"(a) fresh Icp3d {row['fresh_ms']:.3f} ms, (b) compaction + build_grid {row['rebuild_ms']:.3f} ms",
              flush=True)
        del d_kept
    I.lib().icp_trim_pool()


def loop_rows(frames, radius, reps, out):
    pk = synth.synthetic_scan3d_packets(synth.PACKETS_PER_FRAME * (frames + 1))
    t = {"grow": [], "window": []}
    size = {}
    for rep in range(reps + 1):
        for name, r in (("grow", None), ("window", radius)):
            t0 = time.perf_counter()
            Ts, _, world = harness.run_scan_to_map(pk, max_iter=20, map_radius=r)
            t[name].append(time.perf_counter() - t0)
            size[name] = world.target_count
            if r is not None:
                size["crops_moved_rebuilt"] = world.crop_counters()
            world.close()
    row = {"frames": frames, "map_radius": radius, "final_map": size}
    for k, v in t.items():
        row[k + "_frames_per_s"] = frames / float(np.median(v[1:]))
    out["scan_to_map"] = row
    print(f"scan-to-map, {frames} frames: growing map {row['grow_frames_per_s']:.1f} frames/s ({size['grow']} points), "
          f"map_radius {radius} {row['window_frames_per_s']:.1f} frames/s ({size['window']} points; crops moved / rebuilt "
          f"{size['crops_moved_rebuilt']})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--map-radius", type=float, default=4.0)
    ap.add_argument("--only", default=None, choices=[None, "crop", "loop"])
    a = ap.parse_args()
    out = {}
    if a.only in (None, "crop"):
        for m in (int(x) for x in a.sizes.split(",")):
            crop_rows(m, a.reps, out)
    if a.only in (None, "loop"):
        loop_rows(a.frames, a.map_radius, a.reps, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
