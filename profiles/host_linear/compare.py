"""Diffs what launch_cases.py wrote for the parent commit's build and for this tree's:  compare.py <parent dir> <tree dir>
The launch logs line by line, per case; results.json (return codes, error texts, output hashes, profile records, sentinel figures,
workspace sizes) key by key.  Prints the summary that is kept as launch_compare.txt."""
import json
import sys
from collections import OrderedDict


def cases(path):
    out, cur = OrderedDict(), None
    for line in open(path):
        if line.startswith("## "):
            cur = out.setdefault(line[3:].strip(), [])
        else:
            cur.append(line)
    return out


pa, tr = sys.argv[1], sys.argv[2]
lp, lt = cases(pa + "/launches.log"), cases(tr + "/launches.log")
rp, rt = json.load(open(pa + "/results.json")), json.load(open(tr + "/results.json"))
assert list(lp) == list(lt) and sorted(rp) == sorted(rt), "the two sides ran different cases"
total = rows = keys = 0
print(f"{'case':58s} {'launches':>8s} {'rows differing':>14s} {'outputs':>8s} {'profile records':>15s} {'calls (rc, text)':>16s}")
for case in lp:
    a, b = lp[case], lt[case]
    d = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    ra, rb = rp[case], rt[case]
    bad = [k for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
    total += len(b); rows += d; keys += len(bad)
    print(f"{case:58s} {len(b):8d} {d:14d} {len(rb['sha']):8d} {len(rb.get('profile', [])):15d} {len(rb['calls']):16d}"
          + (f"  DIFFERENT: {bad}" if bad else ""))
print(f"\ncases: {len(lp)}   launches compared: {total}   rows differing: {rows}   result entries differing: {keys}")
sys.exit(1 if rows or keys else 0)
