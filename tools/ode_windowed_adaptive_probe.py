#!/usr/bin/env python
"""A long clip through the windowed separate() with the adaptive solvers stepped per clip against the
windowed default midpoint solve.
usage: python tools/ode_windowed_adaptive_probe.py [size] [seconds] [window_s] [overlap_s] [reps] [precision]
                                      (default large* 60 10 1 8 fp16x3: one 60 s clip, 10 s windows with 1 s overlap)
       python tools/ode_windowed_adaptive_probe.py trace [method] [tol] [calls]
                                      (that clip, `calls` grouped solves and nothing else timed: for a kernel trace)

  midpoint   separate(window_seconds=, window_overlap_seconds=) at step 1/16: 32 evaluations of the field
  dopri5 / bosh3 at rtol = atol = 1e-2 / 1e-3 / 1e-4 with step_control="clip" on the same noise
one model, the configurations ALTERNATED (one call of each per round, `reps` rounds after a warm-up round): time per call between
device events, median over the rounds; evaluations, accepted / rejected steps of the clip, distance of the latent to midpoint's.
Nothing here is a gate."""
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
trace = argv[:1] == ["trace"]
if trace:
    method, tol, calls = (argv[1] if len(argv) > 1 else "dopri5"), float(argv[2]) if len(argv) > 2 else 1e-3, int(argv[3]) if len(argv) > 3 else 2
    argv = []
size = argv[0] if argv else "large*"
seconds, window_s, overlap_s = (float(argv[i]) if len(argv) > i else d for i, d in enumerate((60.0, 10.0, 1.0), start=1))
reps = int(argv[4]) if len(argv) > 4 else 8
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
win = dict(window_seconds=window_s, window_overlap_seconds=overlap_s)
model = SAMAudio(cfg, precision=precision, device=str(dev))
model.load_state_dict(sd, strict=False)
print(f"{size} {precision}, one clip of {seconds:g} s = {T} frames; windows of {window_s:g} s with {overlap_s:g} s overlap: W = {W}, O = {O}, "
      f"n = {plan.counts[0]} rows of {plan.row_frames} frames, one group")

if trace:
    opt = {"method": method, "rtol": tol, "atol": tol}
    for _ in range(calls):
        model.separate(batch, noise=noise, ode_opt=opt, step_control="clip", **win)
    torch.cuda.synchronize()
    st = model.last_ode_stats
    print(f"{calls} calls of {method} at {tol:g}: {st['evaluations']} evaluations, {st['rows']}")
    del model
    sys.exit(0)

configs = [("midpoint 1/16", {}, {})]
for m in ("dopri5", "bosh3"):
    for tol_ in (1e-2, 1e-3, 1e-4):
        configs.append((f"{m} {tol_:g}", {"ode_opt": {"method": m, "rtol": tol_, "atol": tol_}}, {"step_control": "clip"}))
times = {name: [] for name, _, _ in configs}
info = {}
for rnd in range(reps + 1):   # round 0 warms up
    for name, a, b in configs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.separate(batch, noise=noise, **a, **b, **win)
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            times[name].append(e0.elapsed_time(e1))
        else:
            info[name] = (model.last_latent.clone(), dict(model.last_ode_stats) if a else None)
mid_ms, mid_lat = statistics.median(times["midpoint 1/16"]), info["midpoint 1/16"][0]
print(f"  {'midpoint 1/16':12s}: 32 evaluations; separate() median {mid_ms:.1f} ms (min {min(times['midpoint 1/16']):.1f}, max "
      f"{max(times['midpoint 1/16']):.1f}); |latent| <= {mid_lat.abs().max().item():.2f}")
for name, a, _ in configs[1:]:
    lat, st = info[name]
    ms = statistics.median(times[name])
    r = st["rows"][0]
    print(f"  {name:12s}: {st['evaluations']} evaluations ({st['evaluations'] / 32:.3f} x midpoint), accepted {r['accepted']}, rejected "
          f"{r['rejected']}, windows {st['windows']}; separate() median {ms:.1f} ms (min {min(times[name]):.1f}, max {max(times[name]):.1f}) = "
          f"{ms / mid_ms:.3f} x midpoint; max-abs to midpoint's latent {(lat - mid_lat).abs().max().item():.3e}")
