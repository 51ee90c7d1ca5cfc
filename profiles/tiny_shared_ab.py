"""A/B of the one-workgroup estimators between two builds of the library (profiles/tiny_shared_ab.txt): the lines of
bench_small.py (the 2-D scan pair, the 3-D frame), bench_batch.py (B = 256, identity start, both dimensions) and
bench_line_batch.py (a batch of one and of 256), each timed by the statements of its script.

    python profiles/tiny_shared_ab.py ROUNDS parent.so new.so     (paths relative to the repo root)

The builds alternate -- parent, new, parent, new, ... -- and every sample is its own process (the library is chosen at
import, ICP_MI355X_LIB).  Per line: the parent's min / median / max over its samples, the new build's, and whether the
new median lies inside the parent's range or below it.  Without arguments: one sample, as one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sample():
    import numpy as np
    import torch

    import icp_rust_amd as I
    from icp_rust_amd import synth
    from icp_rust_amd.scans import load_scan2d

    def median_of(fn, reps):  # bench_batch.py / bench_line_batch.py: a first call, then the median of `reps`
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts))

    out = {}
    g = os.path.join(ROOT, "tests", "golden", "scans2d")
    scans = [np.ascontiguousarray(load_scan2d(f"{g}/{k:03d}.txt")) for k in range(1, 41)]
    # bench_small.py: the scan pair 001 -> 002 and the 28.8k-point frame, mean of 20 / 10 calls after a first one
    icp = I.Icp2d(scans[1])
    icp.estimate(scans[0], I.Transform(), 20)
    t0 = time.perf_counter()
    for _ in range(20):
        icp.estimate(scans[0], I.Transform(), 20, return_info=True)
    out["small 2-D scan pair, estimate(20)"] = 1e3 * (time.perf_counter() - t0) / 20
    icp.close()
    pk = synth.synthetic_scan3d_packets(150)
    s3, d3 = synth.remove_invalid_values(pk[:75]), synth.remove_invalid_values(pk[75:150])
    icp = I.Icp3d(d3)
    icp.estimate(s3, I.Transform(), 20)
    t0 = time.perf_counter()
    for _ in range(10):
        icp.estimate(s3, I.Transform(), 20, return_info=True)
    out["small 3-D frame, estimate(20)"] = 1e3 * (time.perf_counter() - t0) / 10
    icp.close()
    # bench_batch.py: B = 256 from the identity; 2-D the consecutive golden pairs, 3-D eight synthetic 1000 x 2000 pairs
    pairs2 = list(zip(scans[:-1], scans[1:]))
    pairs3 = [synth.synthetic_pair(1000, 2000, seed=synth.SEED + k) for k in range(8)]
    for dim, pairs in ((2, pairs2), (3, pairs3)):
        B = I.IcpBatch(dim)
        sel = [k % len(pairs) for k in range(256)]
        srcs, dsts, inits = [pairs[k][0] for k in sel], [pairs[k][1] for k in sel], [I.Transform() for _ in sel]
        out[f"point batch {dim}-D, B = 256, identity"] = median_of(lambda: B.estimate(srcs, dsts, inits, 20), 5)
        B.close()
    # bench_line_batch.py: device-resident packed scans, k = 8, 20 iterations, median of 7
    first = np.cumsum([0] + [len(s) for s in scans])
    d_packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans))).cuda()
    npairs = len(scans) - 1
    B = I.IcpBatch(2)
    for count in (1, 256):
        items = [(int(first[i % npairs]), len(scans[i % npairs]), int(first[i % npairs + 1]), len(scans[i % npairs + 1]),
                  I.Transform()) for i in range(count)]
        out[f"line batch, B = {count}"] = median_of(
            lambda: B.estimate_point_to_line_packed(d_packed, d_packed, items, 20, 8), 7)
    B.close()
    print(json.dumps(out))


def main():
    rounds, libs = int(sys.argv[1]), sys.argv[2:4]
    got = {lib: [] for lib in libs}
    for r in range(rounds):
        for lib in libs:
            env = dict(os.environ, ICP_MI355X_LIB=os.path.join(ROOT, lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:  # (no further process on a device that may have faulted)
                raise SystemExit(f"round {r} {lib}: exit {p.returncode}\n{p.stderr[-2000:]}")
            got[lib].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"round {r} {lib}: " + ", ".join(f"{v:.4f}" for v in got[lib][-1].values()), flush=True)
    parent, new = libs
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print(f"\nms per call; parent = {parent}, new = {new}; {rounds} alternating samples each")
    print(f"{'line':42s} {'parent min':>10s} {'median':>9s} {'max':>9s} | {'new min':>9s} {'median':>9s} {'max':>9s} | new median")
    for line in got[parent][0]:
        a, b = [s[line] for s in got[parent]], [s[line] for s in got[new]]
        verdict = "below the range" if med(b) < min(a) else ("inside the range" if med(b) <= max(a) else "ABOVE THE RANGE")
        print(f"{line:42s} {min(a):10.4f} {med(a):9.4f} {max(a):9.4f} | {min(b):9.4f} {med(b):9.4f} {max(b):9.4f} | {verdict}")


if __name__ == "__main__":
    main() if len(sys.argv) > 1 else sample()
