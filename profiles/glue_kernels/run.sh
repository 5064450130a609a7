#!/bin/bash
# The measurement behind profiles/glue_kernels/README.md: the new GPU tests with every figure; `suite` as the second argument runs the
# whole GPU suite instead, `bench` smoke() and the benchmark.  One MI355X, prebuilt libraries.  Each step under its own time limit; a
# step that fails ends the script.
set -o pipefail
out=${1:-profiles/glue_kernels/out}
mkdir -p $out
if [ "$2" = "suite" ]; then
  timeout -k 10 1100 python -m pytest tests -m gpu -q -p no:cacheprovider -rs --durations=15 2>&1 | tee $out/gpu_suite.log | tail -40
  exit $?
fi
if [ "$2" = "bench" ]; then   # $3: a checkout of the parent commit with its libraries built
  out=$(realpath $out)
  timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1 || exit $?
  n=0
  for side in parent tree tree parent; do
    n=$((n + 1))
    dir=$PWD
    [ $side = parent ] && dir=$3
    (cd $dir && timeout -k 10 240 python bench.py --gpus 1 --steps 5 --warmup 2) > $out/bench_${n}_${side}.log 2>&1 || exit $?
  done
  exit 0
fi
timeout -k 10 300 python -m pytest tests/test_glue_kernels_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=10 > $out/gpu_tests.log 2>&1
