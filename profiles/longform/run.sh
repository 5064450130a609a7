#!/bin/bash
# The measurement behind DESIGN.md section 10.7: the new GPU tests with every figure, smoke(), the long-clip probe (one 60 s clip as one
# row and as 10 s windows with 1 s overlap, large*, fp16x3), a kernel trace of the blend launches alone, the benchmark; `suite` as the
# second argument runs the whole GPU suite instead.  One MI355X, prebuilt libraries.  Each step under its own time limit; a step that
# fails ends the script.
set -o pipefail
out=${1:-profiles/longform/out}
mkdir -p $out
if [ "$2" = "suite" ]; then
  timeout -k 10 1000 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > $out/gpu_suite.log 2>&1
  exit $?
fi
timeout -k 10 400 python -m pytest tests/test_longform_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=20 > $out/gpu_tests.log 2>&1 \
 && timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1 \
 && timeout -k 10 400 python tools/longform_probe.py 'large*' 60 10 1 3 fp16x3 > $out/probe.log 2>&1 \
 && timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- python tools/longform_probe.py kernels 60 10 1 200 > $out/trace_probe.log 2>&1 \
 && cp $out/trace/*/*kernel_stats.csv $out/kernel_stats.csv \
 && timeout -k 10 300 python bench.py --gpus 1 --steps 5 --warmup 2 > $out/bench.log 2>&1
