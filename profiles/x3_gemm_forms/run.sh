#!/bin/bash
# The GPU runs behind profiles/x3_gemm_forms/README.md.  One MI355X, prebuilt libraries.  Each step under its own time limit; a step that
# fails ends the script.
#   run.sh OUT new   : the new file alone with every figure it prints
#   run.sh OUT tests : the new file, then the whole GPU suite
#   run.sh OUT bench : smoke() and the benchmark
set -o pipefail
out=${1:-profiles/x3_gemm_forms/out}
mkdir -p $out
if [ "$2" = "bench" ]; then
  timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1 \
   && timeout -k 10 400 python bench.py --gpus 1 --steps 5 --warmup 2 > $out/bench.log 2>&1
  exit $?
fi
timeout -k 10 300 python -m pytest tests/test_x3_gemm_forms_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=10 > $out/gpu_tests.log 2>&1 || exit $?
[ "$2" = "new" ] && exit 0
timeout -k 10 900 python -m pytest tests -m gpu -q -p no:cacheprovider -rs --durations=15 > $out/gpu_suite.log 2>&1
