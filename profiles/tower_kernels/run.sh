#!/bin/bash
# The measurement behind profiles/tower_kernels/README.md: the new GPU tests with every figure; `suite` as the second argument runs the
# whole GPU suite instead, `bench` smoke() and the benchmark.  One MI355X, prebuilt libraries.  Each step under its own time limit; a
# step that fails ends the script.
set -o pipefail
out=${1:-profiles/tower_kernels/out}
mkdir -p $out
if [ "$2" = "suite" ]; then
  timeout -k 10 1100 python -m pytest tests -m gpu -q -p no:cacheprovider -rs --durations=15 2>&1 | tee $out/gpu_suite.log | tail -40
  exit $?
fi
if [ "$2" = "bench" ]; then
  timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1 \
   && timeout -k 10 240 python bench.py --gpus 1 --steps 5 --warmup 2 > $out/bench.log 2>&1
  exit $?
fi
timeout -k 10 300 python -m pytest tests/test_tower_kernels_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=10 > $out/gpu_tests.log 2>&1
