#!/usr/bin/env python
"""The uint8 frame path of the visual prompt on one video (PE-Core-L14-336, random-init weights): PerceptionEncoder with
frame_transform="torch" (float copy of the video -> F.interpolate -> round / clamp -> normalise, then patchify in the tower) against
frame_transform="hip" (resize_frames_kernel writes the patch embedding's operand from the uint8 frames) - DESIGN.md section 10.2.
usage: python tools/vit_frames_probe.py [frames] [height] [width] [precision] [reps] [trace]

Default: device events, `reps` (default 11) rounds alternating the two paths in one process after a warm-up of each -
  transform()                      the torch ops alone (patchify, the rest of what the kernel replaces, is a kernel of the tower: see trace)
  samaudio_op_resize_frames        the kernel in its planar fp32 form, with its achieved bytes/s (u8 read + fp32 written)
  PerceptionEncoder.__call__       end to end in both modes, and torch.cuda.max_memory_allocated around it
`trace`: a warm-up and three encodes of each mode and nothing else - the form `rocprofv3 --kernel-trace --stats` is run on
(patchify_kernel against resize_frames_kernel in its fused form)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd import hip, preset_config  # noqa: E402
from sam_audio_amd.config import PE_VISION_CONFIGS  # noqa: E402
from sam_audio_amd.synthetic import init_vision_state_dict  # noqa: E402
from sam_audio_amd.vision_encoder import PerceptionEncoder  # noqa: E402

argv = sys.argv[1:]
trace = "trace" in argv
argv = [a for a in argv if a != "trace"]
n, H, W = (int(argv[i]) if len(argv) > i else d for i, d in enumerate((250, 720, 1280)))
prec = argv[3] if len(argv) > 3 else "fp16"
reps = int(argv[4]) if len(argv) > 4 else 11
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12   # bytes/s: the spec figure and what a streaming kernel reaches on MI355X

dev = torch.device("cuda:0")
cfg = preset_config("large*")
pe = PE_VISION_CONFIGS[cfg.vision_encoder.name]
S = pe.image_size
sd = {"model.visual." + k: v for k, v in init_vision_state_dict(pe, seed=5, device=dev).items()}
encs = {}
for ft in ("torch", "hip"):
    encs[ft] = PerceptionEncoder(cfg.vision_encoder, device=dev, precision=prec, frame_transform=ft)
    encs[ft].load_state_dict(sd)
video = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(1))


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


if trace:
    for ft in ("torch", "hip", "torch", "hip", "torch", "hip", "torch", "hip"):
        encs[ft]([video])
    torch.cuda.synchronize()
    encs.clear()
    sys.exit(0)

lib = hip.lib(hip.operands_for(prec))
planar = torch.empty(n, 3, S, S, device=dev)
mode = hip.RESIZE_MODES[encs["hip"].mode]


def kernel():
    hip.check(lib.samaudio_op_resize_frames(hip.ptr(video), n, H, W, S, mode, hip.ptr(planar), hip.current_stream_ptr()))


steps = {"transform (torch)": lambda: encs["torch"].transform(video), "resize_frames (planar fp32)": kernel,
         "encoder, torch": lambda: encs["torch"]([video]), "encoder, hip": lambda: encs["hip"]([video])}
outs = {k: events(f)[1] for k, f in steps.items()}   # warm-up: code objects, workspaces, the side context, the allocator's blocks
times = {k: [] for k in steps}
for _ in range(reps):
    for k, f in steps.items():
        times[k].append(events(f)[0])
med = {k: statistics.median(v) for k, v in times.items()}
print(f"{cfg.vision_encoder.name} {prec}, {n} frames of {H} x {W} uint8 -> {S}, {encs['hip'].mode}; {reps} rounds alternating in one "
      f"process after a warm-up (device events, ms)")
for k in steps:
    print(f"  {k:28s} median {med[k]:9.3f}   min {min(times[k]):9.3f}   max {max(times[k]):9.3f}")
moved = video.numel() + planar.numel() * 4
rate = moved / (med["resize_frames (planar fp32)"] * 1e-3)
print(f"  resize_frames: {moved / 1e9:.3f} GB (u8 read + fp32 written) -> {rate / 1e12:.3f} TB/s = {rate / HBM_PEAK:.3f} of the 8 TB/s HBM "
      f"peak ({rate / HBM_ACHIEVABLE:.3f} of the 6.3 TB/s a streaming kernel reaches)")
print(f"  kernel / transform: {med['resize_frames (planar fp32)'] / med['transform (torch)']:.3f};  encoder hip / torch: "
      f"{med['encoder, hip'] / med['encoder, torch']:.3f}")
x = (outs["encoder, hip"] - outs["encoder, torch"]).abs().max().item()
lv = (((planar * 0.5 + 0.5) * 255).round() - ((outs["transform (torch)"] * 0.5 + 0.5) * 255).round()).abs()
print(f"  features hip against torch: max-abs {x:.3e};  levels that differ from torch's: {int((lv != 0).sum())} of {lv.numel()} "
      f"(largest {lv.max().item():.0f})")
del outs, planar
for ft in ("torch", "hip"):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    encs[ft]([video])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"  memory, frame_transform={ft!r}: {base / 2 ** 30:.2f} GiB allocated before the call (weights, workspaces, the "
          f"{video.numel() / 2 ** 30:.2f} GiB video), peak {peak / 2 ** 30:.2f} GiB, + {(peak - base) / 2 ** 30:.2f} GiB")
encs.clear()   # destroy the contexts before the interpreter takes the library module apart
