"""A/B of voxel centroids between two builds of the library (profiles/voxel_cov_ab.txt): voxel_centroids' device entry,
means + counts, at 1M and 10M points (bench_voxel.py's cloud, 2.82 points per voxel) and at 2^23 points in ONE voxel.  The
bodies of its three folding kernels moved into voxel_fold_device.hpp, where voxel_cov.hip instantiates them with the
second moments switched on; profiles/voxel_mean_ab.py covers the thinning beside it.

    python profiles/voxel_cov_ab.py ROUNDS parent.so new.so     (paths relative to the repo root)

The method is profiles/voxel_mean_ab.py's, whose table it prints: the builds alternate, every sample is its own process,
a sample's figure is the median of five calls after a warm-up, each call timed around its own wait for the device.
Without arguments: one sample, as one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import voxel_mean_ab as ab


def sample():
    import numpy as np
    import torch

    import icp_rust_amd as I
    from bench_voxel import VOXEL, uniform_cloud
    from icp_rust_amd import synth

    def median_of(fn):
        ts = []
        for _ in range(6):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts[1:]))

    out = {}
    for n in (1_000_000, 10_000_000):
        d_p = torch.from_numpy(uniform_cloud(synth.SEED + 91, n, 2.82)).cuda()
        torch.cuda.synchronize()
        out[f"voxel_centroids, {n} points"] = median_of(lambda: I.voxel_centroids(d_p, VOXEL, return_counts=True))
        del d_p
    d_p = torch.from_numpy(uniform_cloud(synth.SEED + 94, 1 << 23, 2.82)).cuda()
    side = float(d_p.max().item())
    out["voxel_centroids, 8388608 points in one voxel"] = median_of(lambda: I.voxel_centroids(d_p, 2.0 * side, return_counts=True))
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        ab.__file__ = os.path.abspath(__file__)  # (its run() starts this file's sample)
        ab.main()
    else:
        ab.bind_what_the_library_has()
        sample()
