#!/bin/bash
# The measurement behind DESIGN.md section 10.8: the new GPU tests with every figure, smoke(), the ranker's timings at the real dims, a
# kernel trace of one forward (per-kernel durations), the benchmark; `suite` as the second argument runs the whole GPU suite instead.
# One MI355X, prebuilt libraries.  Each step under its own time limit; a step that fails ends the script.
set -o pipefail
out=${1:-profiles/clap/out}
mkdir -p $out
if [ "$2" = "suite" ]; then
  timeout -k 10 1100 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > $out/gpu_suite.log 2>&1
  exit $?
fi
if [ "$2" = "probe" ]; then
  timeout -k 10 300 python tools/clap_probe.py 8 8 10 10 > $out/probe.log 2>&1 \
   && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- python tools/clap_probe.py kernels > $out/trace.log 2>&1 \
   && cp $out/trace/*/*kernel_stats.csv $out/kernel_stats.csv \
   && timeout -k 10 240 python bench.py --gpus 1 --steps 5 --warmup 2 > $out/bench.log 2>&1
  exit $?
fi
timeout -k 10 420 python -m pytest tests/test_clap_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=10 > $out/gpu_tests.log 2>&1 \
 && timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1
