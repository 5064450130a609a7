#!/bin/bash
# The host refactor (one weight record, one launch path for native and x3 GEMMs) against the parent commit.  No kernel changed, so
# every step compares this tree with the parent's build ($PARENT = a checkout of the parent commit, built with __graft_entry__.build()):
#   run.sh objects   (no GPU) sha256 of every kernel file's object, both libraries, side by side -> kernel_object_hashes.txt
#   run.sh launches  (no GPU) the logging build of the launcher emulation of both sides (build_log_emu.sh), launch_cases.py on each,
#                    compare.py -> launch_compare.txt
#   run.sh sizes     (no GPU) profiles/codec_plan/workspace_compare.py on both emulation libraries -> workspace_compare.txt (the Judge's
#                    and the span predictor's workspace sizes are part of `launches`: results.json "workspace_bytes")
#   run.sh tests     smoke(), then the GPU suite, on $SIDE (tree | parent): pass counts to compare -> gpu_tests_$SIDE.log
#   run.sh bench     bench.py --steps 5 --warmup 2 --dump-outputs, order parent tree tree parent parent tree, every dumped array compared
#                    bit for bit, the six ms_per_step -> bench_compare.txt
#   run.sh full      bench.py --full once per side, kernel names and launch counts of prep / dit / codec -> kernels_compare.txt
# Every GPU step under a time limit of its own; the chain ends at the first step that fails.  Logs go to $OUT (default: here).
set -o pipefail
ROOT=$PWD
HERE=profiles/host_linear
CMP=profiles/codec_plan/bench_compare.py
OUT=${OUT:-$ROOT/$HERE}
PARENT=${PARENT:?directory of the parent commit, built}
mkdir -p $OUT
export PYTHONUNBUFFERED=1
case "$1" in
objects)
  for d in build build_f16; do for f in gemm gemm2 gemm8 attention kernels peav_kernels vit_kernels t5_kernels; do
    a=$(sha256sum $PARENT/sam_audio_amd/csrc/$d/$f.o | cut -c1-16); b=$(sha256sum sam_audio_amd/csrc/$d/$f.o | cut -c1-16)
    echo "$d/$f.o parent $a tree $b $([ $a = $b ] && echo same || echo DIFFERENT)"
  done; done > $OUT/kernel_object_hashes.txt
  ;;
launches)
  T=$(mktemp -d)
  for side in parent tree; do
    dir=$ROOT; [ $side = parent ] && dir=$PARENT
    bash $HERE/build_log_emu.sh $dir $T/lib_$side > $T/build_$side.log 2>&1 || { cat $T/build_$side.log; exit 1; }
    python $HERE/launch_cases.py $T/lib_$side/libsamaudio_emu_log.so $T/$side || exit 1
  done
  python $HERE/compare.py $T/parent $T/tree > $OUT/launch_compare.txt
  ;;
sizes)
  T=$(mktemp -d)
  for side in parent tree; do
    lib=$ROOT/oracle/_emu/libsamaudio_emu.so; [ $side = parent ] && lib=$PARENT/oracle/_emu/libsamaudio_emu.so
    python profiles/codec_plan/workspace_compare.py $lib sizes > $T/$side.txt || exit 1
    for mode in fp32 fp32+x3codec bf16; do python profiles/codec_plan/workspace_compare.py $lib passes $mode >> $T/$side.txt || exit 1; done
  done
  { echo "# workspace_compare.py on the parent's and on this tree's emulation library: $(wc -l < $T/tree.txt) rows; differing rows: $(diff $T/parent.txt $T/tree.txt | grep -c '^[<>]')"
    diff $T/parent.txt $T/tree.txt; } > $OUT/workspace_compare.txt
  ;;
tests)
  SIDE=${SIDE:-tree}; dir=$ROOT; [ $SIDE = parent ] && dir=$PARENT
  cd $dir &&
  timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $OUT/smoke_$SIDE.log 2>&1 &&
  timeout -k 10 1100 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > $OUT/gpu_tests_$SIDE.log 2>&1
  ;;
bench)
  D=$(mktemp -d)
  i=0
  for side in parent tree tree parent parent tree; do
    i=$((i + 1)); dir=$ROOT; [ $side = parent ] && dir=$PARENT
    (cd $dir && timeout -k 10 400 python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs $D/${i}_$side) > $OUT/bench_${i}_$side.log 2>&1 || exit 1
  done
  python $CMP outputs $D $OUT > $OUT/bench_compare.txt
  ;;
full)
  for side in parent tree; do
    dir=$ROOT; [ $side = parent ] && dir=$PARENT
    (cd $dir && timeout -k 10 500 python bench.py --gpus 1 --steps 3 --warmup 1 --full --no-cpu-baseline --no-parity-mode --no-hostile --no-other-configs) > $OUT/bench_full_$side.log 2>&1 || exit 1
  done
  python $CMP kernels $OUT > $OUT/kernels_compare.txt
  ;;
esac
