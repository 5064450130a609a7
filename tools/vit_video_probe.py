#!/usr/bin/env python
"""The visual prompt of one clip without its two host passes (PE-Core-L14-336, random-init weights; DESIGN.md section 10.2 "video"):
`SAMAudioProcessor(video_transform="hip")` hands the raw uint8 video, its mask and the picked indices to the frame kernel
(samaudio_vit_encode_video), which masks and picks while it reads and encodes every distinct frame once - against
`video_transform="torch"`, which multiplies the whole video by the mask and gathers one frame per latent step on the CPU.  Both on a
PerceptionEncoder with frame_transform="hip".
usage: python tools/vit_video_probe.py kernel [src_frames] [picked] [height] [width] [precision] [rounds] [parent library]
       python tools/vit_video_probe.py e2e torch|hip [src_frames] [picked] [height] [width] [precision]

kernel: device events in one process, after a warm-up of every step -
  the masked, picked launch (samaudio_op_resize_video, 3-channel mask) against samaudio_op_resize_frames on the materialised frames,
      alternating in rotating order, `rounds` (default 7) rounds of 21 launches each: the median of every round, the requested bytes
      and the rate;
  samaudio_op_resize_frames of this build against the same entry of another build of the library (`parent library`: the .so of the
      parent commit), alternating launch by launch in the same rounds: both medians per round and the spread of the parent's own;
  PerceptionEncoder.__call__ on the MaskedVideo (distinct frames through the tower) against the materialised tensor (every picked
      frame through the tower): what the de-duplication saves when the video has fewer frames than the clip has latent steps.
e2e: ONE path in a fresh process (the resident-set peak of a process never goes down): a warm-up on an 8-frame video, then four
  times mask_videos -> __call__ -> Batch.to(device) -> PerceptionEncoder, host clock to a device synchronise, with the peak resident
  set (VmHWM) and torch.cuda.max_memory_allocated."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd import MaskedVideo, SAMAudioProcessor, hip, preset_config  # noqa: E402
from sam_audio_amd.config import PE_VISION_CONFIGS  # noqa: E402
from sam_audio_amd.synthetic import init_vision_state_dict  # noqa: E402
from sam_audio_amd.vision_encoder import PerceptionEncoder  # noqa: E402

argv = sys.argv[1:]
what = argv.pop(0) if argv else "kernel"
path = argv.pop(0) if what == "e2e" else None
src, n, H, W = (int(argv[i]) if len(argv) > i else d for i, d in enumerate((300, 250, 720, 1280)))
prec = argv[4] if len(argv) > 4 else "fp16"
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12   # bytes/s: the spec figure and what a streaming kernel reaches on MI355X
MC = 3

dev = torch.device("cuda:0")
cfg = preset_config("large*")
pe = PE_VISION_CONFIGS[cfg.vision_encoder.name]
S = pe.image_size
enc = PerceptionEncoder(cfg.vision_encoder, device=dev, precision=prec, frame_transform="hip")
enc.load_state_dict({"model.visual." + k: v for k, v in init_vision_state_dict(pe, seed=5, device=dev).items()})


def host_video(frames, seed):
    """uint8 video and a 3-channel u8 mask (blocks of 16 x 16 pixels, about 40 % masked, non-zero bytes 255) on the host"""
    g = torch.Generator().manual_seed(seed)
    video = torch.randint(0, 256, (frames, 3, H, W), generator=g, dtype=torch.uint8)
    field = torch.rand(frames, MC, (H + 15) // 16, (W + 15) // 16, generator=g) < 0.4
    mask = field.repeat_interleave(16, 2).repeat_interleave(16, 3)[:, :, :H, :W].to(torch.uint8) * 255
    return video, mask.contiguous()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def vm(key):
    with open("/proc/self/status") as f:
        return next(int(line.split()[1]) for line in f if line.startswith(key)) / 2 ** 20   # GiB


if what == "e2e":
    hop = cfg.audio_codec.hop_length
    proc = SAMAudioProcessor.from_config(cfg, video_transform=path)

    def run(video, mask, steps):
        t0 = time.perf_counter()
        masked = proc.mask_videos([video], [mask])
        batch = proc(descriptions=["a"], audios=[torch.zeros(1, steps * hop)], masked_videos=masked)
        t1 = time.perf_counter()
        batch = batch.to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        feats = enc(batch.masked_video)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert feats.shape[1] == steps
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3

    run(*host_video(8, 2), 8)   # code objects, the library's first calls
    video, mask = host_video(src, 1)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base_rss, base_dev = vm("VmRSS"), torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    print(f"{cfg.vision_encoder.name} {prec}, video_transform={path!r}: {src} source frames of {H} x {W} uint8 + a {MC}-channel mask "
          f"({(video.numel() + mask.numel()) / 2 ** 30:.2f} GiB on the host), {n} picked frames -> {S}; host clock, ms")
    for i in range(4):   # (call 0 also sizes the tower's workspace for its chunks and builds the second stream's context)
        t = run(video, mask, n)
        print(f"  call {i}: processor {t[0]:9.2f}   Batch.to {t[1]:9.2f}   encoder {t[2]:9.2f}   total {t[3]:9.2f}")
    print(f"  host: resident set {base_rss:.2f} GiB before the calls (video, mask, torch, the library), peak {vm('VmHWM'):.2f} GiB")
    print(f"  device: {base_dev / 2 ** 30:.2f} GiB allocated before the calls (weights), peak "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB, + {(torch.cuda.max_memory_allocated() - base_dev) / 2 ** 30:.2f} GiB")
    del enc
    sys.exit(0)

rounds = int(argv[5]) if len(argv) > 5 else 7
parent_path = argv[6] if len(argv) > 6 else None
PER_ROUND = 21
lib = hip.lib()
mode = hip.RESIZE_MODES[enc.mode]
g = torch.Generator(device=dev).manual_seed(1)
video = torch.randint(0, 256, (src, 3, H, W), dtype=torch.uint8, device=dev, generator=g)
field = torch.rand(src, MC, (H + 15) // 16, (W + 15) // 16, device=dev, generator=g) < 0.4
mask = (field.repeat_interleave(16, 2).repeat_interleave(16, 3)[:, :, :H, :W].to(torch.uint8) * 255).contiguous()
index = torch.linspace(0, src - 1, n).round().long()
pick = index.to(torch.int32).to(dev)
distinct = index.unique().numel()
mat = (video * mask.eq(0))[index.to(dev)].contiguous()
out_a, out_b = torch.empty(n, 3, S, S, device=dev), torch.empty(n, 3, S, S, device=dev)
st = hip.current_stream_ptr()


def k_video():
    hip.check(lib.samaudio_op_resize_video(hip.ptr(video), src, H, W, hip.ptr(mask), MC, hip.ptr(pick), n, S, mode, hip.ptr(out_a), st))


def k_frames():
    hip.check(lib.samaudio_op_resize_frames(hip.ptr(mat), n, H, W, S, mode, hip.ptr(out_b), st))


steps = {"resize_video (mask + pick)": k_video, "resize_frames (materialised)": k_frames}
if parent_path:
    parent = C.CDLL(os.path.abspath(parent_path))
    parent.samaudio_op_resize_frames.restype, parent.samaudio_op_resize_frames.argtypes = hip._PROTOS["samaudio_op_resize_frames"]

    def k_parent():
        assert parent.samaudio_op_resize_frames(hip.ptr(mat), n, H, W, S, mode, hip.ptr(out_b), st) == 0
    steps["resize_frames (parent build)"] = k_parent

for f in steps.values():
    events(f)
    events(f)
assert torch.equal(out_a, out_b), "the masked, picked launch must equal the plain launch on the materialised frames"
medians = {k: [] for k in steps}
order = list(steps)
for _ in range(rounds):
    times = {k: [] for k in steps}
    for _ in range(PER_ROUND):
        order = order[1:] + order[:1]   # every step follows every other one equally often (what the one before left in the caches)
        for k in order:
            times[k].append(events(steps[k])[0])
    for k in steps:
        medians[k].append(statistics.median(times[k]))
print(f"{src} source frames of {H} x {W} uint8, {MC}-channel mask, {n} picked ({distinct} distinct) -> {S}, {enc.mode}; {rounds} rounds of "
      f"{PER_ROUND} launches per step, the steps alternating launch by launch in rotating order (device events, ms)")
for k in steps:
    m = medians[k]
    print(f"  {k:30s} median of the round medians {statistics.median(m):7.4f}   round medians {min(m):7.4f} .. {max(m):7.4f}   "
          + " ".join(f"{v:.4f}" for v in m))
med = {k: statistics.median(v) for k, v in medians.items()}
frame_bytes = 3 * H * W
req_v = n * frame_bytes * (1 + MC / 3) + out_a.numel() * 4
req_f = n * frame_bytes + out_b.numel() * 4
for k, b in (("resize_video (mask + pick)", req_v), ("resize_frames (materialised)", req_f)):
    r = b / (med[k] * 1e-3)
    print(f"  {k}: {b / 1e9:.3f} GB requested (u8 frames{' + u8 mask' if b == req_v else ''} read per picked frame + fp32 written) -> "
          f"{r / 1e12:.3f} TB/s = {r / HBM_PEAK:.3f} of the 8 TB/s HBM peak ({r / HBM_ACHIEVABLE:.3f} of 6.3 TB/s)")
print(f"  resize_video / resize_frames: {med['resize_video (mask + pick)'] / med['resize_frames (materialised)']:.3f} "
      f"(bytes requested: {req_v / req_f:.3f})")
if parent_path:
    p = medians["resize_frames (parent build)"]
    print(f"  resize_frames, this build / parent build: {med['resize_frames (materialised)'] / med['resize_frames (parent build)']:.4f}; "
          f"the parent's own round medians spread {min(p):.4f} .. {max(p):.4f} ({(max(p) - min(p)) / statistics.median(p) * 100:.2f} %)")

# the tower with and without the de-duplication
item = MaskedVideo(video, mask, index)
tower_steps = {"encoder, MaskedVideo": lambda: enc([item]), "encoder, materialised": lambda: enc([mat])}
outs = {k: events(f)[1] for k, f in tower_steps.items()}
same = torch.equal(outs["encoder, MaskedVideo"], outs["encoder, materialised"])
err = (outs["encoder, MaskedVideo"] - outs["encoder, materialised"]).abs().max().item()
tt = {k: [] for k in tower_steps}
for _ in range(rounds):
    for k, f in tower_steps.items():
        tt[k].append(events(f)[0])
print(f"  PerceptionEncoder.__call__, {rounds} rounds alternating: {distinct} distinct frames through the tower against all {n}")
for k in tower_steps:
    print(f"  {k:30s} median {statistics.median(tt[k]):9.3f}   min {min(tt[k]):9.3f}   max {max(tt[k]):9.3f}")
print(f"  MaskedVideo / materialised: {statistics.median(tt['encoder, MaskedVideo']) / statistics.median(tt['encoder, materialised']):.3f}; "
      f"features bit-equal: {same}, max-abs difference {err:.3e} (the same frames in chunks of other sizes where frames repeat)")
del enc, item
