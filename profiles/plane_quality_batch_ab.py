"""A/B of what the batched plane quality touches in what exists, between two builds of the library
(profiles/plane_quality_batch_bench.txt), in the manner of profiles/plane_batch_gated_ab.py: the plane estimate batch
(its normals' rounds moved to p2plane_device.hpp), the line quality batch (its driver in api_batch.hip now serves both
residuals) -- a batch of one and of 256 each, timed by their benches' statements -- and the headline bench.py.

    python profiles/plane_quality_batch_ab.py ROUNDS parent.so new.so     (paths relative to the repo root)

The builds alternate -- parent, new, parent, new, ... -- and every sample is its own process (the library is chosen at
import, ICP_MI355X_LIB).  Per line: the parent's min / median / max over its samples, the new build's, and whether the
new median lies inside the parent's range or below it, with the new median over the parent's.  An older build lacks the
newest entries: every child binds only what its library has (both builds alike).  Without arguments: one sample of the
two batches, as one JSON line; `--run script args...`: that script, so bound."""
import json
import os
import runpy
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from line_batch_gated_ab import HEADLINE, bind_what_the_library_has  # noqa: E402


def sample():
    import numpy as np
    import torch

    import icp_rust_amd as I
    from bench_plane_batch import M_ITEM, N_ITEM, STRIDE
    from icp_rust_amd import synth
    from icp_rust_amd.scans import load_scan2d

    def median_of(fn, reps):  # the benches' own statement: a first call, then the median of `reps`
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts))

    out = {}
    frame_src, frame_dst = synth.synthetic_pair(N_ITEM * STRIDE, M_ITEM * STRIDE)
    d_src = torch.from_numpy(np.ascontiguousarray(np.concatenate([frame_src[i::STRIDE][:N_ITEM] for i in range(STRIDE)]))).cuda()
    d_dst = torch.from_numpy(np.ascontiguousarray(np.concatenate([frame_dst[i::STRIDE][:M_ITEM] for i in range(STRIDE)]))).cuda()
    B = I.IcpBatch(3)
    for count in (1, 256):
        items = [((i % STRIDE) * N_ITEM, N_ITEM, (i % STRIDE) * M_ITEM, M_ITEM, I.Transform()) for i in range(count)]
        out[f"plane batch, B = {count}"] = median_of(lambda: B.estimate_point_to_plane_packed(d_src, d_dst, items, 20, 8), 7)
    B.close()
    g = os.path.join(ROOT, "tests", "golden", "scans2d")
    scans = [np.ascontiguousarray(load_scan2d(f"{g}/{k:03d}.txt")) for k in range(1, 41)]
    first = np.cumsum([0] + [len(s) for s in scans])
    d_packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans))).cuda()
    npairs = len(scans) - 1
    B = I.IcpBatch(2)
    for count in (1, 256):
        items = [(int(first[i % npairs]), len(scans[i % npairs]), int(first[i % npairs + 1]), len(scans[i % npairs + 1]),
                  I.Transform()) for i in range(count)]
        out[f"line quality batch, B = {count}"] = median_of(
            lambda: B.evaluate_point_to_line_packed(d_packed, d_packed, items, 8, 100.0), 7)
    B.close()
    print(json.dumps(out))


def run(args, lib, what):
    env = dict(os.environ, ICP_MI355X_LIB=os.path.join(ROOT, lib))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    if p.returncode != 0:  # (no further process on a device that may have faulted)
        raise SystemExit(f"{what} {lib}: exit {p.returncode}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    rounds, libs = int(sys.argv[1]), sys.argv[2:4]
    got = {lib: [] for lib in libs}
    for r in range(rounds):
        for lib in libs:
            s = run([], lib, f"round {r}")
            head = run(["--run", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], lib,
                       f"round {r} bench.py")
            assert head["unit"] == "iterations/s", head["unit"]
            s[HEADLINE] = 1e3 / head["value"]
            got[lib].append(s)
            print(f"round {r} {lib}: " + ", ".join(f"{v:.4f}" for v in s.values()), flush=True)
    parent, new = libs
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print(f"\nms; parent = {parent}, new = {new}; {rounds} alternating samples each")
    print(f"{'line':58s} {'parent min':>10s} {'median':>9s} {'max':>9s} | {'new min':>9s} {'median':>9s} {'max':>9s} | new median")
    for line in got[parent][0]:
        a, b = [s[line] for s in got[parent]], [s[line] for s in got[new]]
        verdict = "below the range" if med(b) < min(a) else ("inside the range" if med(b) <= max(a) else "ABOVE THE RANGE")
        verdict += f"; new / parent median {med(b) / med(a):.4f}"
        print(f"{line:58s} {min(a):10.4f} {med(a):9.4f} {max(a):9.4f} | {min(b):9.4f} {med(b):9.4f} {max(b):9.4f} | {verdict}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--run":
        bind_what_the_library_has()
        sys.argv = sys.argv[2:]
        runpy.run_path(sys.argv[0], run_name="__main__")
    elif len(sys.argv) > 1:
        main()
    else:
        bind_what_the_library_has()
        sample()
