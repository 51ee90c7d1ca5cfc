"""Pose evaluation (Icp{2,3}d.evaluate, IcpBatch.evaluate: include/icp_mi355x.h section 9) next to what a caller ran
before it: estimate(..., 1) on the same handle, and the host scoring loop of IcpBatch.estimate_hypotheses (one
huber_error call per item).  Not the headline benchmark (bench.py); a tool for the extension.

    python bench_quality.py [--reps R]
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
from icp_rust_amd import synth
from icp_rust_amd.scans import load_scan2d

G = os.path.join(ROOT, "tests", "golden", "scans2d")


def timed(fn, reps):
    fn()  # (first use: buffers)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def single(label, icp, src, T, r, reps, out):
    """evaluate at T vs one outer iteration of estimate from T, host and device source"""
    import torch

    d_src = torch.from_numpy(src).cuda()
    row = {"points": [len(src), icp.m],
           "evaluate_host_ms": timed(lambda: icp.evaluate(src, T, r), reps),
           "evaluate_device_ms": timed(lambda: icp.evaluate(d_src, T, r), reps),
           "estimate1_host_ms": timed(lambda: icp.estimate(src, T, 1), reps),
           "estimate1_device_ms": timed(lambda: icp.estimate(d_src, T, 1), reps)}
    out[label] = row
    print(f"{label}: evaluate {row['evaluate_device_ms']:.3f} ms (host src {row['evaluate_host_ms']:.3f}), "
          f"estimate(.., 1) {row['estimate1_device_ms']:.3f} ms (host src {row['estimate1_host_ms']:.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    out = {}
    src, dst = synth.synthetic_pair(1_000_000, 1_000_000)  # bench.py's pair
    icp = I.Icp3d(dst)
    T = icp.estimate(src, I.Transform(), 20)
    single("pair_1M_x_1M_3d", icp, src, T, 0.1, a.reps, out)
    icp.close()
    pk = synth.synthetic_scan3d_packets(150)  # bench.py's 28.8k-point frame
    s3, d3 = synth.remove_invalid_values(pk[:75]), synth.remove_invalid_values(pk[75:150])
    icp = I.Icp3d(d3)
    T = icp.estimate(s3, I.Transform(), 20)
    single("frame_28k_3d", icp, s3, T, 0.1, a.reps, out)
    icp.close()
    # 256 golden 2-D scan pairs (the 39 consecutive ones, cycled) at their estimated poses
    scans = [load_scan2d(f"{G}/{k:03d}.txt") for k in range(1, 41)]
    pairs = list(zip(scans[:-1], scans[1:]))
    sel = [k % len(pairs) for k in range(256)]
    srcs, dsts = [pairs[k][0] for k in sel], [pairs[k][1] for k in sel]
    B = I.IcpBatch(2)
    Ts, idxs, _, _ = B.estimate(srcs, dsts, None, 20, return_info=True)
    t_batch = timed(lambda: B.evaluate(srcs, dsts, Ts, 0.2), a.reps)

    def host_scoring():  # IcpBatch.estimate_hypotheses' loop: one huber_error per item on its last correspondences
        return [I.huber_error(T, s, d[ix.astype(np.int64)]) for T, s, d, ix in zip(Ts, srcs, dsts, idxs)]

    t_host = timed(host_scoring, max(1, a.reps // 2))
    out["batch_256_golden_2d"] = {"evaluate_ms": t_batch, "host_huber_loop_ms": t_host,
                                  "counters": list(B.evaluate_counters())}
    print(f"256 golden 2-D pairs: batch evaluate {t_batch:.3f} ms, host scoring loop {t_host:.3f} ms", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
