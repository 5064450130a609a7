#!/bin/bash
# tests/test_layer_kernels_gpu.py with every figure printed, smoke(), then the whole GPU suite - one MI355X box, prebuilt libraries.
# Every step under a time limit of its own; the chain ends at the first step that fails.
set -o pipefail
timeout -k 10 600 python -m pytest tests/test_layer_kernels_gpu.py -m gpu -s -q -p no:cacheprovider > layer_kernels_gpu.log 2>&1 &&
timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > smoke.log 2>&1 &&
timeout -k 10 1100 python -m pytest tests -m gpu -x -q -p no:cacheprovider -rs > gpu_tests.log 2>&1
