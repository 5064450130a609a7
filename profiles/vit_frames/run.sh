#!/bin/bash
# The measurement behind DESIGN.md section 10.2 "uint8 frames": device events + memory, then a kernel trace in a run of its own.
# Each step under its own time limit; a step that fails ends the script.
set -o pipefail
out=${1:-profiles/vit_frames/out}
mkdir -p $out
timeout -k 10 420 python tools/vit_frames_probe.py 250 720 1280 fp16 11 2>&1 | tee $out/probe.log \
 && timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -o trace -- python tools/vit_frames_probe.py 250 720 1280 fp16 11 trace
