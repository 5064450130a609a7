#!/usr/bin/env python
"""The PE-Core-L14-336 tower alone on one 250-frame video (random-init weights).
usage: python tools/vit_probe.py [frames] [precision[,precision...]] [rounds]

One precision (default fp16; "fp16x3" / "bf16x3" = the compensated mode): a warm-up encode, then three timed
ones - the form `rocprofv3 --kernel-trace --stats` is run on.
Several precisions: every tower is built and warmed up first, then `rounds` (default 5) rounds alternate one encode of each in the
same process, each between device events; per precision the per-round times, their median, the algorithmic rate and the workspace
of its contexts are printed (profiles/vit_x3/)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd import preset_config  # noqa: E402
from sam_audio_amd.config import PE_VISION_CONFIGS  # noqa: E402
from sam_audio_amd.synthetic import init_vision_state_dict  # noqa: E402
from sam_audio_amd.vision_encoder import PerceptionEncoder  # noqa: E402
from sam_audio_amd.vision_tower import tower_flops  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 250
precs = (sys.argv[2] if len(sys.argv) > 2 else "fp16").split(",")
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
cfg = preset_config("large*")
pe = PE_VISION_CONFIGS[cfg.vision_encoder.name]
sd = {"model.visual." + k: v for k, v in init_vision_state_dict(pe, seed=5, device=dev).items()}
fl = tower_flops(pe, n)


def build(prec):
    enc = PerceptionEncoder(cfg.vision_encoder, device=dev, precision=prec)
    enc.load_state_dict(sd)
    return enc


def timed(enc, frames, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = enc.encode(frames)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def rate(ms):
    return f"{fl / ms / 1e9:.1f} TFLOP/s algorithmic ({fl / ms / 1e9 / 2500:.3f} of the 16-bit MFMA peak)"


video = torch.rand(n, 3, 360, 640, device=dev)
if len(precs) == 1:
    enc = build(precs[0])
    frames = enc.transform(video)
    enc.encode(frames)
    ms, _ = timed(enc, frames, 3)
    print(f"{cfg.vision_encoder.name} {precs[0]}: {ms:.2f} ms per {n} frames, {rate(ms)}")
    sys.exit(0)

encs = {p: build(p) for p in precs}
frames = encs[precs[0]].transform(video)
outs = {p: encs[p].encode(frames) for p in precs}   # warm-up: code objects, workspaces, the side context
torch.cuda.synchronize()
times = {p: [] for p in precs}
for _ in range(rounds):
    for p in precs:
        ms, _ = timed(encs[p], frames)
        times[p].append(ms)
print(f"{cfg.vision_encoder.name}, {n} frames, {rounds} rounds alternating {' / '.join(precs)} in one process (device events, ms per encode)")
for p in precs:
    t = encs[p].tower
    ctx = [t._workspace] + ([t._side[0]._workspace] if t._side else [])
    ws = " + ".join(f"{w.numel() / 2 ** 30:.2f}" for w in ctx if w is not None)
    med = statistics.median(times[p])
    print(f"  {p:7s} {' '.join(f'{x:8.2f}' for x in times[p])}   median {med:8.2f} ms, {rate(med)}; workspace {ws} GiB "
          f"({len(ctx)} context{'s' if len(ctx) > 1 else ''})")
ref = precs[0]
for p in precs[1:]:
    d = (outs[p] - outs[ref]).abs().max().item()
    print(f"  {p} against {ref}: median time ratio {statistics.median(times[p]) / statistics.median(times[ref]):.3f}, features max-abs "
          f"difference {d:.3e} (seeded init weights: benign)")
encs.clear()   # destroy the contexts before the interpreter takes the library module apart
