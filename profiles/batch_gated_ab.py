"""A/B of what the gated point batch kernel shares its body with, between two builds of the library
(profiles/batch_gated_ab.txt): the lines of bench_batch.py (a batch of one and of 256 from the identity, both dimensions,
timed by its statements), bench_small.py's 2-D scan pair and the headline bench.py.

    python profiles/batch_gated_ab.py ROUNDS parent.so new.so     (paths relative to the repo root)

The builds alternate -- parent, new, parent, new, ... -- and every sample is its own process (the library is chosen at
import, ICP_MI355X_LIB).  Per line: the parent's min / median / max over its samples, the new build's, and whether the
new median lies inside the parent's range or below it; for bench.py also the new median over the parent's.  An older
build lacks the newest entries: every child binds only what its library has (both builds alike).  Without arguments: one
sample of the batches and the scan pair, as one JSON line; `--run script args...`: that script, so bound."""
import json
import os
import runpy
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADLINE = "bench.py --gpus 1 --steps 20 --warmup 5, ms per iteration"


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

    import icp_rust_amd as I
    from icp_rust_amd import synth
    from icp_rust_amd.scans import load_scan2d

    def median_of(fn, reps):  # bench_batch.py: a first call, then the median of `reps`
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
    # bench_small.py: the scan pair 001 -> 002, mean of 20 calls after a first one
    icp = I.Icp2d(scans[1])
    icp.estimate(scans[0], I.Transform(), 20)
    t0 = time.perf_counter()
    for _ in range(20):
        icp.estimate(scans[0], I.Transform(), 20, return_info=True)
    out["small 2-D scan pair, estimate(20)"] = 1e3 * (time.perf_counter() - t0) / 20
    icp.close()
    # bench_batch.py: from the identity; 2-D the consecutive golden pairs, 3-D eight synthetic 1000 x 2000 pairs
    pairs2 = list(zip(scans[:-1], scans[1:]))
    pairs3 = [synth.synthetic_pair(1000, 2000, seed=synth.SEED + k) for k in range(8)]
    for dim, pairs in ((2, pairs2), (3, pairs3)):
        B = I.IcpBatch(dim)
        for count in (1, 256):
            sel = [k % len(pairs) for k in range(count)]
            srcs, dsts, inits = [pairs[k][0] for k in sel], [pairs[k][1] for k in sel], [I.Transform() for _ in sel]
            out[f"point batch {dim}-D, B = {count}, identity"] = median_of(lambda: B.estimate(srcs, dsts, inits, 20), 5)
        B.close()
    print(json.dumps(out))


def run(args, lib, what):
    env = dict(os.environ, ICP_MI355X_LIB=os.path.join(ROOT, lib))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    if p.returncode != 0:  # (no further process on a device that may have faulted)
        raise SystemExit(f"{what} {lib}: exit {p.returncode}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    rounds, libs = int(sys.argv[1]), sys.argv[2:4]
    got = {lib: [] for lib in libs}
    for r in range(rounds):
        for lib in libs:
            s = run([], lib, f"round {r}")
            head = run(["--run", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], lib, f"round {r} bench.py")
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
        if line == HEADLINE:
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
