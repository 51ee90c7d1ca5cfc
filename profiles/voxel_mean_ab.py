"""A/B of voxel thinning between two builds of the library (profiles/voxel_mean_ab.txt): voxel_downsample's device entry
at 1M and 10M points (bench_voxel.py's cloud, 2.82 points per voxel) and at 2^23 points in ONE voxel, and Icp3d.thin on maps
of 1M and 10M targets after a 28 800-point append.  The device helpers of voxel.hip moved into voxel_device.hpp and its
insert kernel now sends one lane per cell and wave to the table.

    python profiles/voxel_mean_ab.py ROUNDS parent.so new.so     (paths relative to the repo root)

The builds alternate -- parent, new, parent, new, ... -- and every sample is its own process (the library is chosen at
import, ICP_MI355X_LIB); a sample's figure is the median of five calls after a warm-up, each call timed around its own
wait for the device.  Per line: the parent's min / median / max over its samples, the new build's, and whether the new
median lies inside the parent's range or below it.  An older build lacks the newest entries: every child binds only what
its library has (both builds alike).  Without arguments: one sample, as one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bind_what_the_library_has():
    import ctypes

    try:
        import torch  # noqa: F401  (its HIP runtime first, as icp_rust_amd._lib loads it)
    except ImportError:
        pass
    from icp_rust_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(L, n)]:
        del _lib.SIGNATURES[name]


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
        out[f"voxel_downsample, {n} points"] = median_of(lambda: I.voxel_downsample(d_p, VOXEL, return_index=True))
        del d_p
    d_p = torch.from_numpy(uniform_cloud(synth.SEED + 94, 1 << 23, 2.82)).cuda()
    side = float(d_p.max().item())
    out["voxel_downsample, 8388608 points in one voxel"] = median_of(lambda: I.voxel_downsample(d_p, 2.0 * side, return_index=True))
    del d_p
    for m in (1_000_000, 10_000_000):
        d_raw = torch.from_numpy(uniform_cloud(synth.SEED + 92, (3 * m) // 2, 0.8)).cuda()
        d_map = I.voxel_downsample(d_raw, VOXEL).clone()
        side = float(d_raw.max().item())
        del d_raw
        frame = np.ascontiguousarray(np.random.default_rng(synth.SEED + 93).uniform(0.0, side, (28_800, 3)))
        d_frame = torch.from_numpy(frame).cuda()
        torch.cuda.synchronize()
        ts = []
        for _ in range(6):
            icp = I.Icp3d(d_map)
            icp.append(d_frame)
            t0 = time.perf_counter()
            icp.thin(VOXEL)
            ts.append(time.perf_counter() - t0)
            icp.close()
        out[f"thin, map of {m} + 28800"] = 1e3 * float(np.median(ts[1:]))
        del d_map, d_frame
    print(json.dumps(out))


def run(lib, what):
    env = dict(os.environ, ICP_MI355X_LIB=os.path.join(ROOT, lib))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    if p.returncode != 0:  # (no further process on a device that may have faulted)
        raise SystemExit(f"{what} {lib}: exit {p.returncode}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    rounds, libs = int(sys.argv[1]), sys.argv[2:4]
    got = {lib: [] for lib in libs}
    for r in range(rounds):
        for lib in libs:
            s = run(lib, f"round {r}")
            got[lib].append(s)
            print(f"round {r} {lib}: " + ", ".join(f"{v:.4f}" for v in s.values()), flush=True)
    parent, new = libs
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print(f"\nms; parent = {parent}, new = {new}; {rounds} alternating samples each")
    print(f"{'line':48s} {'parent min':>10s} {'median':>9s} {'max':>9s} | {'new min':>9s} {'median':>9s} {'max':>9s} | new median")
    for line in got[parent][0]:
        a, b = [s[line] for s in got[parent]], [s[line] for s in got[new]]
        verdict = "below the range" if med(b) < min(a) else ("inside the range" if med(b) <= max(a) else "ABOVE THE RANGE")
        print(f"{line:48s} {min(a):10.4f} {med(a):9.4f} {max(a):9.4f} | {min(b):9.4f} {med(b):9.4f} {max(b):9.4f} | {verdict}")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main()
    else:
        bind_what_the_library_has()
        sample()
