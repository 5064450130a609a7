#!/usr/bin/env python
"""The DAC-VAE in time tiles: what it does to peak memory and to time.
usage: python tools/codec_tiles_probe.py [size] [precision] [reps]        (default large* fp16x3 3)

  longform   one 60 s clip, 10 s windows with 1 s overlap: peak device memory and ms per separate(), untiled against
             codec_tile_seconds 10 and 2 (median of `reps` after a warm-up, device events)
  codec      the benchmarked shape, 32 clips x 10 s: encode + decode-pairs time for tiles of 10 s (one tile: the untiled call), 5, 2, 1
             and 0.5 s, the order of the runs alternating; beside each the cost of the halo alone, (L + 2h) / L
  ten-min    one 10-minute clip through separate() with 10 s windows and 2 s codec tiles: peak memory and time; the untiled call is
             attempted only if the size query says its codec workspace fits the free memory - otherwise the query's figure is printed

One model serves every run: between runs its workspaces are dropped and the allocator's peak is reset, so a peak is that run's own."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd import SAMAudio, SAMAudioProcessor, longform, preset_config  # noqa: E402
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features  # noqa: E402

dev = torch.device("cuda:0")
argv = sys.argv[1:]
size = argv[0] if argv else "large*"
precision = argv[1] if len(argv) > 1 else "fp16x3"
reps = int(argv[2]) if len(argv) > 2 else 3
GiB = 2.0 ** 30

cfg = preset_config(size)
codec = cfg.audio_codec
hop, rate = codec.hop_length, codec.sample_rate
base = torch.cuda.memory_allocated()
model = SAMAudio(cfg, precision=precision, device=str(dev))
model.load_state_dict(init_state_dict(cfg, seed=0, device=dev), strict=False)
torch.cuda.synchronize()
torch.cuda.empty_cache()
weights = torch.cuda.memory_allocated() - base
h_enc, h_dec = (model._lib.samaudio_codec_halo_frames(model._ctx, d) for d in (0, 1))
print(f"{size} {precision}: model tensors {weights / GiB:.2f} GiB; codec reach {h_enc} frames (encode), {h_dec} frames (decode); "
      f"{rate / hop:.0f} frames per second")


def fresh():
    """drop every workspace and the allocator's cache and peak: the next run's peak is its own"""
    for own in [model] + list(model._lanes):
        own._workspace = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def clip_batch(seconds, n=1):
    samples = int(round(seconds * rate))
    text, tmask = synthetic_text_features(n, 8)
    return SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * n, audios=[synthetic_clip(i, samples) for i in range(n)],
                                              text_features=text, text_mask=tmask).to(dev)


def frames_of(seconds):
    return longform.seconds_to_frames(seconds, rate, hop)


# ---------------------------------------------------------------------------------------------- 1. the longform probe's shape
batch = clip_batch(60.0)
T = batch.sizes_host[0]
noise = synthetic_noise(1, T).to(dev)
print(f"\nlongform: one clip of 60 s = {T} frames, 10 s windows with 1 s overlap; median of {reps} separate() calls after a warm-up")
ref = None
for tile in (None, 10.0, 2.0):
    fresh()
    call = lambda: model.separate(batch, noise=noise, window_seconds=10.0, window_overlap_seconds=1.0, codec_tile_seconds=tile)  # noqa: E731
    call()
    ms = [timed(call)[0] for _ in range(reps)]
    res = call()
    peak = torch.cuda.max_memory_allocated() - base
    if ref is None:
        ref = (statistics.median(ms), peak, res)
    same = all(torch.equal(a, b) for a, b in zip(res.target + res.residual, ref[2].target + ref[2].residual))
    print(f"  codec_tile_seconds={tile!s:5}: median {statistics.median(ms):8.1f} ms (min {min(ms):.1f}, max {max(ms):.1f}) = "
          f"{statistics.median(ms) / ref[0]:.3f} x untiled; peak device memory {peak / GiB:6.2f} GiB = {peak / ref[1]:.3f} x untiled "
          f"(model tensors {weights / GiB:.2f} GiB); waveforms bit-equal to untiled: {same}; tiles {model.last_codec_tiles}")
del ref, res

# ---------------------------------------------------------------------------------------------- 2. the benchmarked shape
B, seconds = 32, 10.0
batch = clip_batch(seconds, B)
T = batch.sizes_host[0]
state = torch.randn(B, T, 2 * codec.codebook_dim, device=dev)
tiles = [10.0, 5.0, 2.0, 1.0, 0.5]
print(f"\ncodec: {B} clips x {seconds:g} s = {T} frames each; encode + decode-pairs (2 x {B} waveforms) per run; {2 * reps} runs per tile, "
      f"the order of the tiles alternating")


def codec_run(L):
    """each call in a workspace of its own size (the engine takes as many items per pass as the workspace holds): SAMAUDIO_CODEC_CHUNK
    items x the longest segment"""
    model._workspace = None
    model.encode_audio(batch.audios, tile_frames=L)
    model._workspace = None
    model.decode_audio(state, pairs=True, tile_frames=L)


for chunk in ("16", "2"):   # items per pass: the default, and one pair - the smallest working set a pass can have
    os.environ["SAMAUDIO_CODEC_CHUNK"] = chunk
    ms = {t: [] for t in tiles}
    fresh()
    for t in tiles:
        codec_run(frames_of(t))   # warm-up
    torch.cuda.synchronize()
    for rep in range(2 * reps):
        for t in (tiles if rep % 2 == 0 else tiles[::-1]):
            ms[t].append(timed(lambda: codec_run(frames_of(t)))[0])
    one = statistics.median(ms[tiles[0]])
    print(f"  SAMAUDIO_CODEC_CHUNK={chunk}:")
    for t in tiles:
        L = frames_of(t)
        halo = ((L + 2 * h_enc) / L + (L + 2 * h_dec) / L) / 2 if L < T else 1.0
        m = statistics.median(ms[t])
        ws = model._lib.samaudio_workspace_bytes(model._ctx, 0, 0, 0, int(chunk), model._codec_segment(T, L, True))
        print(f"    tile {t:4g} s = {L:3d} frames: median {m:7.1f} ms (min {min(ms[t]):.1f}, max {max(ms[t]):.1f}) = {m / one:.3f} x one tile; "
              f"the halo alone would cost {halo:.3f} x (mean of encode's and decode's (L + 2h) / L); decode workspace {ws / GiB:.2f} GiB")
os.environ.pop("SAMAUDIO_CODEC_CHUNK")
del state

# ---------------------------------------------------------------------------------------------- 3. ten minutes
seconds = 600.0
batch = clip_batch(seconds)
T = batch.sizes_host[0]
noise = synthetic_noise(1, T).to(dev)
fresh()
untiled = model._lib.samaudio_workspace_bytes(model._ctx, 0, 0, 0, 2, T * hop)
free = torch.cuda.mem_get_info()[0]
print(f"\nten-min: one clip of {seconds:g} s = {T} frames, 10 s windows with 1 s overlap, codec tiles of 2 s")
print(f"  untiled: the size query asks {untiled / GiB:.1f} GiB of codec workspace for one (target, residual) pair; {free / GiB:.1f} GiB are free: "
      + ("it fits" if untiled < free else "not attempted"))
call = lambda tile: model.separate(batch, noise=noise, window_seconds=10.0, window_overlap_seconds=1.0, codec_tile_seconds=tile)  # noqa: E731
call(2.0)
t_ms, _ = timed(lambda: call(2.0))
peak = torch.cuda.max_memory_allocated() - base
print(f"  tiled: {t_ms:.1f} ms per separate(); peak device memory {peak / GiB:.2f} GiB (model tensors {weights / GiB:.2f} GiB); "
      f"tiles {model.last_codec_tiles}")
if untiled < free:
    fresh()
    call(None)
    t_ms, _ = timed(lambda: call(None))
    print(f"  untiled: {t_ms:.1f} ms per separate(); peak device memory {(torch.cuda.max_memory_allocated() - base) / GiB:.2f} GiB")

del model
