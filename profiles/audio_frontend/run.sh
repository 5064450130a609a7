#!/bin/bash
# The measurement behind DESIGN.md section 10.5: the new GPU tests with every figure, smoke(), the processor / kernel timings and the
# memory figures; then the whole GPU suite and the benchmark.  One MI355X, prebuilt libraries.  Each step under its own time limit;
# a step that fails ends the script.
set -o pipefail
out=${1:-profiles/audio_frontend/out}
mkdir -p $out
timeout -k 10 300 python -m pytest tests/test_audio_frontend_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=10 > $out/gpu_tests.log 2>&1 \
 && timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1 \
 && timeout -k 10 420 python tools/audio_frontend_probe.py 32 10 44100 7 > $out/probe.log 2>&1 \
 && timeout -k 10 800 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > $out/gpu_suite.log 2>&1 \
 && timeout -k 10 240 python bench.py --gpus 1 --steps 5 --warmup 2 > $out/bench.log 2>&1 \
 && timeout -k 10 120 python tools/audio_frontend_probe.py memory all all 32 10 44100 > $out/memory.log 2>&1
