"""probes_compare.py DIR: the fp16x3 times of probe_vit_<i>_<side>.log / probe_tower_<i>_<side>.log (run.sh probes), per figure the three
values of each side and whether each of the tree's lies inside the parent's span (min .. max)."""
import glob
import json
import os
import re
import sys

d = sys.argv[1]
vals = {}   # figure -> side -> [ms]
for path in sorted(glob.glob(os.path.join(d, "probe_*_*_*.log"))):
    kind, _, side = re.match(r"probe_(\w+?)_(\d)_(\w+)\.log", os.path.basename(path)).groups()
    text = open(path).read()
    if kind == "vit":
        m = re.search(r"fp16x3: ([\d.]+) ms per", text)
        figs = {"vision tower 250 frames": float(m.group(1))} if m else {}
    else:
        r = json.loads(text.strip().splitlines()[-1])
        figs = {f"{k} (median)": v["fp16x3"]["ms_median"] for k, v in r.items() if not k.endswith("_bytes")}
    for k, v in figs.items():
        vals.setdefault(k, {}).setdefault(side, []).append(v)
for k, s in sorted(vals.items()):
    p, t = s.get("parent", []), s.get("tree", [])
    inside = [min(p) <= v <= max(p) for v in t] if p else []
    print(f"{k} fp16x3 ms: parent {p} (span {min(p):.3f} .. {max(p):.3f}), tree {t}: inside the parent's span {inside}")
