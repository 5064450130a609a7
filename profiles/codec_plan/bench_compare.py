"""What run.sh compares between the parent commit's build and this tree.

    bench_compare.py outputs <dump dir> <log dir>   sha256 of every array the six `bench.py --dump-outputs` runs left, their ms_per_step
    bench_compare.py kernels <log dir>              kernel names and launch counts of the two `bench.py --full` runs, side by side
"""
import glob
import hashlib
import json
import os
import statistics
import sys


def result_line(path):
    for line in open(path):
        if line.startswith('{"metric"'):
            return json.loads(line)
    raise SystemExit(f"{path}: no result line")


def outputs(dumps, logs):
    seen = {}
    for run in sorted(os.listdir(dumps)):
        row = {os.path.basename(f): hashlib.sha256(open(f, "rb").read()).hexdigest()[:16] for f in sorted(glob.glob(f"{dumps}/{run}/*.npy"))}
        seen[run] = row
        print(run, row)
    first = next(iter(seen.values()))
    print("every dumped array bitwise equal across the runs:", bool(first) and all(row == first for row in seen.values()))
    ms = {"parent": [], "tree": []}
    for log in sorted(glob.glob(f"{logs}/bench_[1-6]_*.log")):
        r = result_line(log)
        side = "parent" if log.endswith("_parent.log") else "tree"
        ms[side].append(r["ms_per_step"])
        print(os.path.basename(log), "ms_per_step", r["ms_per_step"], "value", r["value"])
    p, t = ms["parent"], ms["tree"]
    med = statistics.median(t)
    print(f"parent ms_per_step {p}: min {min(p)} max {max(p)} median {statistics.median(p)}")
    print(f"tree   ms_per_step {t}: median {med} -> inside the parent's range: {min(p) <= med <= max(p)}; "
          f"above the parent's max by {max(0.0, med - max(p)):.2f} ms (the parent's own spread: {max(p) - min(p):.2f} ms)")


def kernels(logs):
    rows = {}
    for side in ("parent", "tree"):
        for k in result_line(f"{logs}/bench_full_{side}.log")["kernels"]:
            rows.setdefault(k["kernel"], {})[side] = k["launches"]
    differ = 0
    for name in sorted(rows):
        a, b = rows[name].get("parent"), rows[name].get("tree")
        differ += a != b
        print(f"{name:48s} parent {a!s:>6} tree {b!s:>6}{'' if a == b else '   DIFFERS'}")
    print(f"{len(rows)} kernel records, differing: {differ}")


if __name__ == "__main__":
    outputs(sys.argv[2], sys.argv[3]) if sys.argv[1] == "outputs" else kernels(sys.argv[2])
