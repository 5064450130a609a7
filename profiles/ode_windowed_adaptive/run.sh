#!/bin/bash
# The measurement behind DESIGN.md section 10.11.  One MI355X, prebuilt libraries.  Every step under its own time limit; a step that
# fails ends the script.
#   run.sh OUT tests             the new GPU tests with every figure, then smoke()
#   run.sh OUT suite             the whole GPU suite
#   run.sh OUT measure [PARENT]  tools/ode_windowed_adaptive_probe.py (one 60 s clip, large*, fp16x3, 10 s windows with 1 s overlap: windowed
#                                midpoint against dopri5 / bosh3 per clip at 1e-2 / 1e-3 / 1e-4, 8 alternated rounds), a kernel trace of
#                                grouped dopri5 solves on their own, and - with PARENT, a built checkout of the parent commit - the
#                                parent's windowed midpoint (its tools/longform_probe.py) and the benchmark alternating parent / tree
set -o pipefail
out=${1:-profiles/ode_windowed_adaptive/out}
mode=${2:-tests}
parent=$3
mkdir -p $out
root=$(pwd)
case $mode in
tests)
  timeout -k 10 500 python -m pytest tests/test_ode_windowed_adaptive_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=25 > $out/gpu_tests.log 2>&1 \
   && timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1
  ;;
suite)
  timeout -k 10 1150 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > $out/gpu_suite.log 2>&1
  ;;
measure)
  timeout -k 10 420 python tools/ode_windowed_adaptive_probe.py 'large*' 60 10 1 8 fp16x3 > $out/probe.log 2>&1 \
   && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- python tools/ode_windowed_adaptive_probe.py trace dopri5 1e-3 2 > $out/trace_probe.log 2>&1 \
   && cp $out/trace/*/*kernel_stats.csv $out/kernel_stats.csv || exit $?
  if [ -n "$parent" ]; then
    (cd $parent && timeout -k 10 300 python tools/longform_probe.py 'large*' 60 10 1 8 fp16x3) > $out/parent_midpoint.log 2>&1 || exit $?
    : > $out/bench_ab.txt
    for i in 1 2; do
      (cd $parent && timeout -k 10 300 python bench.py --gpus 1 --steps 3 --warmup 1 2>&1 | tail -1 | sed 's/^/parent /') >> $out/bench_ab.txt || exit $?
      (cd $root && timeout -k 10 300 python bench.py --gpus 1 --steps 3 --warmup 1 2>&1 | tail -1 | sed 's/^/tree   /') >> $out/bench_ab.txt || exit $?
    done
  fi
  ;;
esac
