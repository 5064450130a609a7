#!/bin/bash
# One x3 launch path for the towers (host.h) and one hi/lo split primitive for the kernels (common.h), against the parent commit
# ($PARENT = a checkout of the parent commit, built with __graft_entry__.build()).  Nothing may change a number or a launch:
#   run.sh objects   (no GPU) untouched kernel files: sha256 of their objects, both libraries; touched ones (kernels, peav_kernels,
#                    attention, gemm8): the gfx950 instruction text per kernel symbol (disasm_compare.py) -> kernel_code_compare.txt
#   run.sh launches | sizes | tests | bench     the steps of profiles/host_linear/run.sh, with their results written here
#   run.sh simt      (no GPU) vision tower, T5, ModernBERT on the functional simulator library of both sides (towers_simt.py):
#                    output bytes, return codes, error texts, samaudio_vit_workspace_bytes -> simt_compare.txt.  It builds nothing:
#                    oracle/_simt/libsamaudio_simt.so of BOTH sides must exist (oracle/simt/build.sh, or build())
#   run.sh probes    tools/vit_probe.py and tools/tower_probe.py in fp16x3, parent and tree interleaved, three runs each -> probe_*.log,
#                    probes_compare.txt
# Every GPU step under a time limit of its own; the chain ends at the first step that fails.  Logs go to $OUT (default: here).
set -o pipefail
ROOT=$PWD
HERE=profiles/x3_one_path
export OUT=${OUT:-$ROOT/$HERE}
PARENT=${PARENT:?directory of the parent commit, built}
mkdir -p $OUT
export PYTHONUNBUFFERED=1
case "$1" in
objects)
  { for d in build build_f16; do for f in gemm gemm2 vit_kernels t5_kernels; do
      a=$(sha256sum $PARENT/sam_audio_amd/csrc/$d/$f.o | cut -c1-16); b=$(sha256sum sam_audio_amd/csrc/$d/$f.o | cut -c1-16)
      echo "$d/$f.o parent $a tree $b $([ $a = $b ] && echo same || echo DIFFERENT)"
    done; done
    python $HERE/disasm_compare.py $PARENT/sam_audio_amd/csrc sam_audio_amd/csrc kernels peav_kernels attention gemm8
  } > $OUT/kernel_code_compare.txt
  ;;
launches|sizes|tests|bench)
  PARENT=$PARENT bash profiles/host_linear/run.sh $1
  ;;
simt)
  T=$(mktemp -d)
  for side in parent tree; do
    dir=$ROOT; [ $side = parent ] && dir=$PARENT
    SAMAUDIO_EMU_DRYRUN=simt SAMAUDIO_EMU_NOBUILD=1 python $HERE/towers_simt.py $dir $T/$side.json || exit 1
  done
  python $HERE/compare_json.py $T/parent.json $T/tree.json > $OUT/simt_compare.txt
  ;;
probes)
  i=0
  for side in parent tree tree parent parent tree; do
    i=$((i + 1)); dir=$ROOT; [ $side = parent ] && dir=$PARENT
    (cd $dir && timeout -k 10 200 python tools/vit_probe.py 250 fp16x3) > $OUT/probe_vit_${i}_$side.log 2>&1 &&
    (cd $dir && timeout -k 10 300 python tools/tower_probe.py 10) > $OUT/probe_tower_${i}_$side.log 2>&1 || exit 1
  done
  python $HERE/probes_compare.py $OUT > $OUT/probes_compare.txt
  ;;
esac
