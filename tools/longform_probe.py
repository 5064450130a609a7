#!/usr/bin/env python
"""A long clip through separate() as one row and as overlapping windows.
usage: python tools/longform_probe.py [size] [seconds] [window_s] [overlap_s] [reps] [precision]
                                      (default large* 60 10 1 3 fp16x3: one 60 s clip, 10 s windows with 1 s overlap)
       python tools/longform_probe.py kernels [seconds] [window_s] [overlap_s] [launches]
                                      (window_blend_kernel alone on that plan's rows, for a kernel trace)

  whole      separate() of the clip as one row of T frames: the code path without the window arguments
  windowed   separate(window_seconds=, window_overlap_seconds=) of the same clip on the same noise
each on a fresh model: time per call between device events (median of `reps` after a warm-up) and the peak of torch's allocator over
the calls (weights, workspace, tensors).  Then one profiled windowed call: the share of window_blend_kernel in the kernel time of the
call.  The default ODE (midpoint, 16 steps = 32 evaluations of the field)."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd import SAMAudio, SAMAudioProcessor, hip, longform, preset_config  # noqa: E402
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features  # noqa: E402

HBM_PEAK = 8.0e12
dev = torch.device("cuda:0")
argv = sys.argv[1:]


def events(fn, n):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


if argv[:1] == ["kernels"]:
    seconds, window_s, overlap_s = (float(argv[i]) if len(argv) > i else d for i, d in enumerate((60.0, 10.0, 1.0), start=1))
    launches = int(argv[4]) if len(argv) > 4 else 200
    codec = preset_config("large*").audio_codec
    fps = codec.sample_rate / codec.hop_length
    T = longform.seconds_to_frames(seconds, codec.sample_rate, codec.hop_length)
    W, O = (longform.seconds_to_frames(s, codec.sample_rate, codec.hop_length) for s in (window_s, overlap_s))
    plan = longform.plan_windows([T], W, O, batch_frames=T)
    C2 = 256
    out = torch.randn(plan.rows, plan.row_frames, C2, device=dev)
    table = torch.tensor(plan.next_row, dtype=torch.int32, device=dev)
    lib = hip.lib()

    def blend():
        hip.check(lib.samaudio_op_window_blend(hip.ptr(out), hip.ptr(table), plan.rows, plan.row_frames, O, C2, hip.current_stream_ptr()))

    links = sum(s >= 0 for s in plan.next_row)
    moved = links * O * C2 * 4 * 4   # two reads and two writes per pair
    ms = events(lambda: [blend() for _ in range(launches)], 5)
    per = statistics.median(ms) / launches
    print(f"window_blend_kernel on [{plan.rows}, {plan.row_frames}, {C2}] ({T} frames at {fps:.0f} per second, W = {W}, O = {O}, {links} links): "
          f"{moved / 1e3:.1f} kB moved per launch; {launches} back-to-back launches between device events: {per * 1e3:.2f} us per launch "
          f"(launch gaps included) = {moved / (per * 1e-3) / 1e9:.1f} GB/s = {moved / (per * 1e-3) / HBM_PEAK:.5f} of the "
          f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    sys.exit(0)

size = argv[0] if argv else "large*"
seconds, window_s, overlap_s = (float(argv[i]) if len(argv) > i else d for i, d in enumerate((60.0, 10.0, 1.0), start=1))
reps = int(argv[4]) if len(argv) > 4 else 3
precision = argv[5] if len(argv) > 5 else "fp16x3"

cfg = preset_config(size)
codec = cfg.audio_codec
sd = init_state_dict(cfg, seed=0, device=dev)
samples = int(round(seconds * codec.sample_rate))
text, tmask = synthetic_text_features(1, 8)
batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"], audios=[synthetic_clip(0, samples)], text_features=text,
                                           text_mask=tmask).to(dev)
T = batch.sizes_host[0]
noise = synthetic_noise(1, T).to(dev)
W, O = (longform.seconds_to_frames(s, codec.sample_rate, codec.hop_length) for s in (window_s, overlap_s))
plan = longform.plan_windows([T], W, O, batch_frames=T)
print(f"{size} {precision}, one clip of {seconds:g} s = {T} frames; windows of {window_s:g} s with {overlap_s:g} s overlap: W = {W}, O = {O}, "
      f"S = {plan.stride}, n = {plan.counts[0]} rows of {plan.row_frames} frames = {plan.rows * plan.row_frames / T:.3f} x the frames of the "
      f"whole clip; {reps} calls after a warm-up")

results = {}
for name, kw in (("whole", {}), ("windowed", dict(window_seconds=window_s, window_overlap_seconds=overlap_s))):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    model = SAMAudio(cfg, precision=precision, device=str(dev))
    model.load_state_dict(sd, strict=False)
    weights = torch.cuda.memory_allocated() - base
    ms = events(lambda: model.separate(batch, noise=noise, **kw), reps)
    peak = torch.cuda.max_memory_allocated() - base
    results[name] = (statistics.median(ms), peak, model.last_latent.clone())
    print(f"  {name:9s} separate(): median {statistics.median(ms):.1f} ms (min {min(ms):.1f}, max {max(ms):.1f}); peak device memory "
          f"{peak / 2**30:.2f} GiB of which the model's tensors {weights / 2**30:.2f} GiB")
    if name == "windowed":
        model.profile_begin()
        model.separate(batch, noise=noise, **kw)
        recs = model.profile_end()
        total = sum(r["ms"] for r in recs)
        blend = [r for r in recs if r["name"].endswith("window_blend")]
        b_ms, b_n = sum(r["ms"] for r in blend), sum(r["launches"] for r in blend)
        print(f"  profiled windowed call: window_blend_kernel {b_n} launches, {b_ms:.3f} ms of {total:.1f} ms of kernel time = "
              f"{100 * b_ms / total:.3f} %")
    del model
w, x = results["whole"], results["windowed"]
diff = (w[2] - x[2]).abs().max().item()
print(f"  windowed / whole: time {x[0] / w[0]:.3f}, peak memory {x[1] / w[1]:.3f}; the two latents differ by up to {diff:.2f} (two different "
      f"computations by definition; nothing is claimed about either's quality)")
