#!/bin/bash
# The measurement behind profiles/x3_invariance/README.md, one MI355X, prebuilt libraries.  $1: output directory; $2: `new` (default) =
# the new file with every printed name list, `edited` = the two files that gained fp16x3 cases (with the printed errors), `suite` = the
# whole GPU suite, `bench` = smoke() and one benchmark run.  gpu_tests.log is the `new` log followed by the `edited` one.  Each step
# under its own time limit; a step that fails ends the script.
set -o pipefail
out=${1:-profiles/x3_invariance/out}
mkdir -p $out
case "${2:-new}" in
  new)
    timeout -k 10 400 python -m pytest tests/test_x3_invariance_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=0 > $out/gpu_tests_new.log 2>&1
    ;;
  edited)
    timeout -k 10 1000 python -m pytest tests/test_large_gpu.py tests/test_configs_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=0 > $out/gpu_tests_edited.log 2>&1
    ;;
  suite)
    timeout -k 10 1150 python -m pytest tests -m gpu -q -p no:cacheprovider -rs --durations=25 2>&1 | tee $out/gpu_suite.log | tail -45
    ;;
  bench)
    timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1 || exit $?
    timeout -k 10 300 python bench.py --gpus 1 --steps 5 --warmup 2 > $out/bench_tree.log 2>&1
    ;;
esac
