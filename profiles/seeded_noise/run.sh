#!/bin/bash
# The measurement behind DESIGN.md section 10.10, as it was run: `tests` = the new GPU tests with every figure; `suite` = the whole
# GPU suite once, then smoke(); `bench` = the op's timing beside torch.randn, then bench.py on this tree and on a checkout of the
# parent commit (second argument: its directory, libraries built), alternating twice.  One MI355X, prebuilt libraries.  Each step
# under its own time limit; a step that fails ends the script.
set -o pipefail
out=$PWD/profiles/seeded_noise/out
mkdir -p $out
case "$1" in
tests)
  timeout -k 10 400 python -m pytest tests/test_noise_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=12 > $out/gpu_tests.log 2>&1 ;;
suite)
  timeout -k 10 1000 python -m pytest tests -m gpu -q -p no:cacheprovider -rs > $out/gpu_suite.log 2>&1 \
   && timeout -k 10 150 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1 ;;
bench)
  parent=${2:?directory of a checkout of the parent commit}
  timeout -k 10 200 python tools/noise_probe.py > $out/probe.log 2>&1 || exit 1
  : > $out/bench_ab.txt
  for round in 1 2; do
    for which in new parent; do
      dir=.; [ $which = parent ] && dir=$parent
      (cd $dir && timeout -k 10 200 python bench.py --gpus 1 --steps 5 --warmup 2) > $out/bench_${which}_$round.log 2>&1 || exit 1
      echo "$which $round: $(tail -1 $out/bench_${which}_$round.log)" >> $out/bench_ab.txt
    done
  done ;;
*) echo "usage: $0 tests | suite | bench <parent checkout>"; exit 2 ;;
esac
