"""compare_json.py PARENT.json TREE.json: the entries of towers_simt.py of both sides, one line each, and the count that differ."""
import json
import sys

a, b = (json.load(open(p)) for p in sys.argv[1:3])
differing = 0
for key in sorted(set(a) | set(b)):
    same = a.get(key) == b.get(key)
    differing += not same
    e = b.get(key) or {}
    print(f"{key}: out {e.get('out', '-')} workspace {e.get('workspace', '-')} codes/texts {len(e.get('log', []))} {'same' if same else 'DIFFERENT'}")
    if not same:
        print(f"   parent {a.get(key)}\n   tree   {b.get(key)}")
print(f"# {len(set(a) | set(b))} entries, differing: {differing}")
