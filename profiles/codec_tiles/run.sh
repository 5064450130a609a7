#!/bin/bash
# The measurement behind DESIGN.md section 10.12: the new GPU tests with every figure, smoke(), the tile probe (large*, fp16x3), the
# benchmark; `suite` as the second argument runs the whole GPU suite instead.  One MI355X, prebuilt libraries.  Each step under its own
# time limit; a step that fails ends the script.
set -o pipefail
out=${1:-profiles/codec_tiles/out}
mkdir -p $out
if [ "$2" = "suite" ]; then
  timeout -k 10 1000 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > $out/gpu_suite.log 2>&1
  exit $?
fi
timeout -k 10 400 python -m pytest tests/test_codec_tiles_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=15 > $out/gpu_tests.log 2>&1 \
 && timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1 \
 && timeout -k 10 840 python tools/codec_tiles_probe.py 'large*' fp16x3 3 > $out/probe.log 2>&1 \
 && timeout -k 10 300 python bench.py --gpus 1 --steps 5 --warmup 2 > $out/bench.log 2>&1
