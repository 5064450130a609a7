#!/bin/bash
# The selection-layer cleanup (GemmVariant / GEMM_FLAG_* / DebugFlag names, ablation build removed) on one MI355X box, prebuilt
# libraries: smoke(), the whole GPU suite, then bench.py on the parent commit's build ($PARENT = a checkout of it, built) and on this
# tree, alternating, three runs each, with the dumped outputs compared bit for bit.  Every step under a time limit of its own; the
# chain ends at the first step that fails.
set -o pipefail
ROOT=$PWD
PARENT=${PARENT:?directory of the parent commit, built}
D=$(mktemp -d)
ARGS="--gpus 1 --steps 5 --warmup 2"
timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > smoke.log 2>&1 &&
timeout -k 10 1000 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > gpu_tests.log 2>&1 || exit 1
for i in 1 2 3; do
  (cd $PARENT && timeout -k 10 400 python bench.py $ARGS --dump-outputs $D/parent_$i) > bench_parent_$i.log 2>&1 || exit 1
  (cd $ROOT && timeout -k 10 400 python bench.py $ARGS --dump-outputs $D/branch_$i) > bench_branch_$i.log 2>&1 || exit 1
done
# bench_compare.txt: sha256 of every dumped array of the six runs, the six ms_per_step values.
# bench_compare_balanced.txt: a second call with the six runs in the order parent, tree, tree, parent, parent, tree (ms_per_step rises
# through a call on these boxes: with the parent first in every pair the rise falls on the tree's side).
