#!/bin/bash
# The measurement behind DESIGN.md section 10.2 "video": the new GPU tests with every figure, then tools/vit_video_probe.py - the
# masked, picked launch against the plain launch (and against the plain launch of the parent commit's build of the library, if its
# path is given), the tower with and without the de-duplication, and one fresh process per end-to-end path for the memory peaks.
# One MI355X, prebuilt libraries.  Each step under its own time limit; a step that fails ends the script.
# With a parent library also the A/B of the plain launch over 15 rounds, and the same against a byte copy of this tree's own library
# in the parent's place (what the slot of the second library is worth).
# usage: profiles/vit_video/run.sh [output directory] [libsamaudio_hip.so of the parent commit]
set -o pipefail
out=${1:-profiles/vit_video/out}
parent=$2
mkdir -p $out
timeout -k 10 300 python -m pytest tests/test_vit_video_gpu.py -m gpu -s -q -p no:cacheprovider -rs --durations=10 > $out/gpu_tests.log 2>&1 \
 && timeout -k 10 300 python tools/vit_video_probe.py kernel 300 250 720 1280 fp16 7 $parent > $out/probe_300.log 2>&1 \
 && timeout -k 10 300 python tools/vit_video_probe.py kernel 80 250 720 1280 fp16 7 $parent > $out/probe_80.log 2>&1 \
 && timeout -k 10 240 python tools/vit_video_probe.py e2e torch 300 250 720 1280 fp16 > $out/e2e_torch_300.log 2>&1 \
 && timeout -k 10 240 python tools/vit_video_probe.py e2e hip 300 250 720 1280 fp16 > $out/e2e_hip_300.log 2>&1 \
 && timeout -k 10 240 python tools/vit_video_probe.py e2e torch 80 250 720 1280 fp16 > $out/e2e_torch_80.log 2>&1 \
 && timeout -k 10 240 python tools/vit_video_probe.py e2e hip 80 250 720 1280 fp16 > $out/e2e_hip_80.log 2>&1 \
 && if [ -n "$parent" ]; then
      cp sam_audio_amd/libsamaudio_hip.so $out/libsamaudio_hip_tree_copy.so \
       && timeout -k 10 300 python tools/vit_video_probe.py kernel 300 250 720 1280 fp16 15 $parent > $out/ab_parent.log 2>&1 \
       && timeout -k 10 300 python tools/vit_video_probe.py kernel 300 250 720 1280 fp16 15 $out/libsamaudio_hip_tree_copy.so > $out/ab_null.log 2>&1
    fi
