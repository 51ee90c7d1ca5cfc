"""Throughput of the batch call (IcpBatch: many small registrations in one launch) in problems per second, next to the
same problems as serial Icp2d / Icp3d calls and the single-thread CPU oracle.  Not the headline benchmark (bench.py) and
not bench_small.py's single-pair latency; a tool for the batched extension ("Batched small registrations").

    python bench_batch.py [--reps R] [--sizes 1,64,256,1024,4096]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import synth
from icp_rust_amd.scans import load_scan2d

G = os.path.join(ROOT, "tests", "golden", "scans2d")


def timed(fn, reps):
    fn()  # (first use: buffers, LDS grant)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,64,256,1024,4096")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    out = {}
    scans = [load_scan2d(f"{G}/{k:03d}.txt") for k in range(1, 41)]
    pairs2 = list(zip(scans[:-1], scans[1:]))  # consecutive golden pairs, cycled
    pairs3 = [synth.synthetic_pair(1000, 2000, seed=synth.SEED + k) for k in range(8)]  # 3-D, <= 2048 targets
    for dim, pairs, label in ((2, pairs2, "2d_scans"), (3, pairs3, "3d_synth")):
        B = I.IcpBatch(dim)
        cold = [I.Transform() for _ in pairs]
        warm = B.estimate([p[0] for p in pairs], [p[1] for p in pairs], cold, 20)  # a converged pose per pair
        for start, inits0 in (("identity", cold), ("warm", warm)):
            for b in sizes:
                sel = [k % len(pairs) for k in range(b)]
                srcs, dsts, inits = [pairs[k][0] for k in sel], [pairs[k][1] for k in sel], [inits0[k] for k in sel]
                t = timed(lambda: B.estimate(srcs, dsts, inits, 20), a.reps)
                out[f"{label}_{start}_B{b}_per_s"] = b / t
                print(f"{label} {start:8s} B={b:5d}: {t * 1e3:9.3f} ms per batch, {b / t:10.0f} problems/s", flush=True)
        served, one, launches, refused = B.counters()
        print(f"   {label} counters: in-kernel {served}, one by one {one}, launches {launches}, LDS refused {refused}")
        # the same problems as serial single calls (a handle per pair, as the reference builds one per frame)
        cls = I.Icp2d if dim == 2 else I.Icp3d
        nser = 16

        def serial():
            for k in range(nser):
                h = cls(pairs[k % len(pairs)][1])
                h.estimate(pairs[k % len(pairs)][0], I.Transform(), 20)
                h.close()

        t = timed(serial, 2) / nser
        out[f"{label}_serial_per_s"] = 1 / t
        print(f"{label} serial {cls.__name__}(dst).estimate(20): {t * 1e3:.3f} ms per problem, {1 / t:.0f} problems/s")
        trees = [O.KdTree(p[1]) for p in pairs[:8]] if dim == 2 else None
        t0 = time.perf_counter()
        for k in range(8):
            if dim == 2:
                trees[k].estimate(pairs[k][0], O.transform_identity(), 20)
            else:
                O.icp_estimate(3, pairs[k][1], pairs[k][0], O.transform_identity(), 20, use_kdtree=True)
        t = (time.perf_counter() - t0) / 8
        out[f"{label}_cpu_oracle_1core_per_s"] = 1 / t
        print(f"{label} CPU oracle, one core: {t * 1e3:.3f} ms per problem, {1 / t:.0f} problems/s", flush=True)
        B.close()
    # K = 256 hypotheses of one scan pair (one shared src / dst range)
    B = I.IcpBatch(2)
    rng = np.random.default_rng(3)
    hyp = [I.Transform([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.4, 0.4)]) for _ in range(256)]
    src, dst = pairs2[0]
    items = [(0, len(src), 0, len(dst), T) for T in hyp]
    t = timed(lambda: B.estimate_packed(src, dst, items, 20), a.reps)
    out["hypotheses_K256_per_s"] = 256 / t
    print(f"hypotheses K=256 over one 2-D pair: {t * 1e3:.3f} ms per batch, {256 / t:.0f} problems/s")
    print(json.dumps({k: round(v, 1) for k, v in out.items()}))


if __name__ == "__main__":
    main()
