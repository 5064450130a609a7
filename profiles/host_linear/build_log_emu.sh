#!/bin/bash
# Builds the LOGGING variant of the launcher emulation for one source tree:  build_log_emu.sh <tree root> <out dir>
# The tree's own engine.hip / peav.hip / api.hip and oracle/emu sources, with every launch routed through the generated shim
# (gen_log_shim.py, always THIS directory's: both sides of a comparison log in the same format).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
TREE="$(cd "$1" && pwd)"; OUT="$2"
mkdir -p "$OUT"; OUT="$(cd "$OUT" && pwd)"
SRC=$TREE/sam_audio_amd/csrc
python "$HERE/gen_log_shim.py" "$TREE" "$OUT/log_shim.cpp" "$OUT/log_defines.txt"
REN=""
for f in hipMemsetAsync hipMemcpyAsync hipMemcpy hipStreamSynchronize hipEventCreate hipEventDestroy hipEventRecord \
         hipEventSynchronize hipEventElapsedTime hipStreamBeginCapture hipStreamCreateWithFlags; do
  REN="$REN -D$f=emu_$f"
done
FLAGS="--offload-host-only --offload-arch=gfx950 -O2 -std=c++17 -fPIC -fopenmp -Wno-unused-result -Wno-macro-redefined"
pids=()
for f in engine peav api; do
  hipcc $FLAGS $REN $(cat "$OUT/log_defines.txt") -c $SRC/$f.hip -o $OUT/$f.o & pids+=($!)
done
hipcc $FLAGS $REN -x hip -c $TREE/oracle/emu/emu_kernels.cpp -o $OUT/emu_kernels.o & pids+=($!)
hipcc $FLAGS $REN -x hip -c $TREE/oracle/emu/emu_hip.cpp -o $OUT/emu_hip.o & pids+=($!)
hipcc $FLAGS $REN -I$SRC -x hip -c $OUT/log_shim.cpp -o $OUT/log_shim.o & pids+=($!)
for p in "${pids[@]}"; do wait $p; done
hipcc -shared -fPIC -fopenmp $OUT/engine.o $OUT/peav.o $OUT/api.o $OUT/emu_kernels.o $OUT/emu_hip.o $OUT/log_shim.o -o $OUT/libsamaudio_emu_log.so
echo "built $OUT/libsamaudio_emu_log.so"
