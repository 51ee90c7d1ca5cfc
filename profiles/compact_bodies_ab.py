"""A/B of the extension benchmarks around the shared mark and place bodies (compact_device.hpp), by the method of
profiles/shared_core_ab.txt: two builds of the library loaded by the same benchmark scripts, alternating, every run a
process of its own (the library is chosen at import through ICP_MI355X_LIB).
    python3 profiles/compact_bodies_ab.py run PARENT.so THIS.so ROUNDS OUTDIR [job ...]
    python3 profiles/compact_bodies_ab.py table OUTDIR
A run that fails or outlives its limit ends the whole script: nothing more is started on the card."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# job -> (arguments, seconds allowed per run, the figures whose kernels are the same in both builds: the controls)
JOBS = {
    "window": (["bench_window.py", "--only", "crop", "--sizes", "1000000"], 240, r"fresh_ms$"),
    "voxel": (["bench_voxel.py", "--only", "call", "--sizes", "28800,1000000"], 240, r"torch_ms$"),
    "voxel_thin": (["bench_voxel.py", "--only", "thin", "--maps", "1000000"], 240, r"fresh_ms$"),
    "voxel_mean": (["bench_voxel_mean.py", "--sizes", "28800,1000000", "--heavy", "0"], 240, r"torch_ms$"),
    "query": (["bench_query.py", "--sizes", "28800", "--tree-max", "0", "--out", os.devnull], 300,
              r"(lists|neighbours|count_)"),
    "outlier": (["bench_outlier.py", "--sizes", "120000,1000000", "--torch-max", "0", "--tree-max", "0",
                 "--order-size", "0"], 300, r"lists\d+_ms$"),
}


def figures(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from figures(v, prefix + k + ".")
        elif k.endswith("_ms") and isinstance(v, (int, float)) and "numpy" not in k:  # (numpy: a host arm, no library)
            yield prefix + k, float(v)


def run(parent, this, rounds, outdir, jobs):
    os.makedirs(outdir, exist_ok=True)
    for job in jobs:
        args, limit, _ = JOBS[job]
        with open(os.path.join(outdir, job + ".jsonl"), "a") as f:
            for r in range(rounds):
                for name, lib in (("parent", parent), ("this", this)):
                    env = dict(os.environ, ICP_MI355X_LIB=os.path.abspath(lib))
                    p = subprocess.run([sys.executable, os.path.join(ROOT, args[0])] + args[1:], env=env, cwd=ROOT,
                                       capture_output=True, text=True, timeout=limit)
                    if p.returncode != 0:
                        print(f"{job} round {r} {name}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
                        sys.exit(1)
                    f.write(json.dumps({"build": name, "round": r, "out": json.loads(p.stdout.strip().splitlines()[-1])}) + "\n")
                    f.flush()
                    print(f"{job} round {r} {name} ok", flush=True)


def table(outdir):
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    rows, worst = [], 0.0
    for job, (_, _, control) in JOBS.items():
        path = os.path.join(outdir, job + ".jsonl")
        if not os.path.exists(path):
            continue
        runs = {"parent": {}, "this": {}}
        for line in open(path):
            rec = json.loads(line)
            for k, v in figures(rec["out"]):
                runs[rec["build"]].setdefault(k, []).append(v)
        for k in runs["parent"]:
            a, b = runs["parent"][k], runs["this"][k]
            lo, hi, m = min(a), max(a), med(b)
            out = 0.0 if lo <= m <= hi else (m - hi) / hi if m > hi else (m - lo) / lo
            is_control = re.search(control, k) is not None
            if is_control:
                worst = max(worst, abs(out))
            rows.append((job, k, is_control, a, b, lo, hi, m, out))
    print(f"controls leave their parent spread by at most {100 * worst:.2f} %")
    print(f"{'figure':58s} {'parent runs':>{9 * 5}s}   {'this commit runs':>{9 * 5}s}   parent spread          median  verdict")
    for job, k, is_control, a, b, lo, hi, m, out in rows:
        verdict = "inside" if out == 0.0 else f"{100 * out:+.2f} % " + ("(within the controls')" if abs(out) <= worst else "OUTSIDE")
        print(f"{(job + ':' + k)[:57]:58s} {''.join(f'{x:9.3f}' for x in a)}   {''.join(f'{x:9.3f}' for x in b)}   "
              f"[{lo:9.3f},{hi:9.3f}] {m:9.3f}  {'control, ' if is_control else ''}{verdict}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5], sys.argv[6:] or list(JOBS))
    else:
        table(sys.argv[2])
