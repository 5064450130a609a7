#!/bin/bash
# The engine refactor (one codec workspace plan, GemmKind / Phase, fold_plan) on one MI355X box, prebuilt libraries.  No kernel
# changed, so everything here compares this tree with the parent commit's build ($PARENT = a checkout of it, built):
#   run.sh tests   smoke(), tests/test_codec_workspace_gpu.py with its figures, the whole GPU suite
#   run.sh bench   bench.py --steps 5 --warmup 2 --dump-outputs, order parent tree tree parent parent tree (ms_per_step rises
#                  through a call on these boxes), every dumped array compared bit for bit -> bench_compare.txt
#   run.sh full    bench.py --full once per side (no CPU baseline / other precisions / other configs: the kernel table is what is
#                  compared), kernel names and launch counts of prep, dit and codec side by side -> kernels_compare.txt
#   run.sh sizes   (no GPU) workspace_compare.py on the parent's and this tree's CPU emulation library -> workspace_compare.txt
# Every GPU step under a time limit of its own; the chain ends at the first step that fails.  Logs go to $OUT (default: here).
set -o pipefail
ROOT=$PWD
HERE=profiles/codec_plan
OUT=${OUT:-$ROOT/$HERE}
PARENT=${PARENT:?directory of the parent commit, built}
mkdir -p $OUT
export PYTHONUNBUFFERED=1
case "$1" in
tests)
  timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $OUT/smoke.log 2>&1 &&
  timeout -k 10 300 python -m pytest tests/test_codec_workspace_gpu.py -m gpu -s -q -p no:cacheprovider > $OUT/codec_workspace_gpu.log 2>&1 &&
  timeout -k 10 1000 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > $OUT/gpu_tests.log 2>&1
  ;;
bench)
  D=$(mktemp -d)
  i=0
  for side in parent tree tree parent parent tree; do
    i=$((i + 1)); dir=$ROOT; [ $side = parent ] && dir=$PARENT
    (cd $dir && timeout -k 10 400 python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs $D/${i}_$side) > $OUT/bench_${i}_$side.log 2>&1 || exit 1
  done
  python $HERE/bench_compare.py outputs $D $OUT > $OUT/bench_compare.txt
  ;;
full)
  for side in parent tree; do
    dir=$ROOT; [ $side = parent ] && dir=$PARENT
    (cd $dir && timeout -k 10 500 python bench.py --gpus 1 --steps 3 --warmup 1 --full --no-cpu-baseline --no-parity-mode --no-hostile --no-other-configs) > $OUT/bench_full_$side.log 2>&1 || exit 1
  done
  python $HERE/bench_compare.py kernels $OUT > $OUT/kernels_compare.txt
  ;;
sizes)
  T=$(mktemp -d)
  for side in parent tree; do
    lib=$ROOT/oracle/_emu/libsamaudio_emu.so; [ $side = parent ] && lib=$PARENT/oracle/_emu/libsamaudio_emu.so
    python $HERE/workspace_compare.py $lib sizes > $T/$side.txt || exit 1
    for mode in fp32 fp32+x3codec bf16; do python $HERE/workspace_compare.py $lib passes $mode >> $T/$side.txt || exit 1; done
  done
  { echo "# workspace_compare.py on the parent's and on this tree's emulation library: rows of this tree; differing rows: $(diff $T/parent.txt $T/tree.txt | grep -c '^[<>]')"
    diff $T/parent.txt $T/tree.txt; cat $T/tree.txt; } > $OUT/workspace_compare.txt
  ;;
esac
