#!/usr/bin/env python
"""The adaptive ODE solvers (dopri5 / bosh3, per-row step control: DESIGN.md section 10.9) measured on separate()'s solve.
usage: python tools/ode_adaptive_probe.py [size] [seconds] [precision] [clips ...]     (default large* 10 fp16x3 4 32)

For every clip count, on prepared conditioning of synthetic clips with ragged lengths (the last frames of every second clip are padding):
  evaluations   per solve for rtol = atol in {1e-2, 1e-3, 1e-4}, both methods, against midpoint's 32; accepted / rejected per row,
                minimum and maximum over the rows; the distance of the latent to the default midpoint solve's
  overhead      one profiled solve at 1e-3: the kernel time of ode_error + ode_control + ode_commit (+ ode_stage_rows) as a share of the
                kernel time of the solve.  The host read of a trial step cannot be bracketed by events; it shows as the gap between a
                solve's wall-time ratio to midpoint and its evaluation ratio (first table)
  spread        the trial step at which each row finished: rows that finish early ride along until the last one - the wasted share
                is 1 - mean(finish) / max(finish)
Nothing here is a gate."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd import SAMAudio, preset_config  # noqa: E402
from sam_audio_amd.model import DFLT_ODE_OPT  # noqa: E402
from sam_audio_amd.synthetic import init_state_dict, synthetic_noise  # noqa: E402

argv = sys.argv[1:]
size = argv[0] if argv else "large*"
seconds = float(argv[1]) if len(argv) > 1 else 10.0
precision = argv[2] if len(argv) > 2 else "fp16x3"
clip_counts = [int(a) for a in argv[3:]] or [4, 32]
dev = torch.device("cuda:0")

cfg = preset_config(size)
codec = cfg.audio_codec
T = int(round(seconds * codec.sample_rate / codec.hop_length))
sd = init_state_dict(cfg, seed=0, device=dev, with_codec=False)
model = SAMAudio(cfg, precision=precision, device=str(dev))
model.load_state_dict(sd, strict=False)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


for B in clip_counts:
    g = torch.Generator().manual_seed(B)
    z = torch.randn(B, T, 128, generator=g)
    feats, text = torch.cat([z, z], 2), torch.randn(B, 8, 768, generator=g)
    lengths = torch.tensor([T if b % 2 == 0 else T - 1 - 7 * (b % 5) for b in range(B)])
    pad = torch.arange(T)[None, :] < lengths[:, None]
    noise = synthetic_noise(B, T).to(dev)
    model._prepare(feats, text, None, None, None, None, pad)
    model.solve(noise, DFLT_ODE_OPT)
    mid, mid_ms = wall(lambda: model.solve(noise, DFLT_ODE_OPT))
    print(f"== {size} {precision}, {B} clips x {seconds:g} s ({T} frames, valid {int(lengths.min())} .. {T}); midpoint 1/16: 32 evaluations, "
          f"{mid_ms:.1f} ms, |latent| <= {mid.abs().max().item():.2f}")
    for method in ("dopri5", "bosh3"):
        for tol in (1e-2, 1e-3, 1e-4):
            opt = {"method": method, "rtol": tol, "atol": tol}
            model.solve(noise, opt)
            out, ms = wall(lambda: model.solve(noise, opt))
            st = model.last_ode_stats
            acc = [r["accepted"] for r in st["rows"]]
            rej = [r["rejected"] for r in st["rows"]]
            finish = [a + r for a, r in zip(acc, rej)]
            waste = 1 - sum(finish) / (len(finish) * max(finish))
            print(f"{method} tol {tol:g}: {st['evaluations']} evaluations ({st['evaluations'] / 32:.2f} x midpoint), {ms:.1f} ms "
                  f"({ms / mid_ms:.2f} x); accepted {min(acc)} .. {max(acc)}, rejected {min(rej)} .. {max(rej)} per row; rows finish at trial "
                  f"step {min(finish)} .. {max(finish)}: wasted share {waste:.3f}; max-abs to midpoint {(out - mid).abs().max().item():.3e}")
        opt = {"method": method, "rtol": 1e-3, "atol": 1e-3}
        model.profile_begin()
        _, ms = wall(lambda: model.solve(noise, opt))
        recs = {r["name"]: r for r in model.profile_end()}
        trials = max(r["accepted"] + r["rejected"] for r in model.last_ode_stats["rows"])
        total = sum(r["ms"] for r in recs.values())
        glue = {k: recs[f"dit/{k}"]["ms"] for k in ("ode_stage_rows", "ode_error", "ode_control", "ode_commit")}
        tail = glue["ode_error"] + glue["ode_control"] + glue["ode_commit"]
        print(f"{method} 1e-3 profiled: {trials} trial steps, kernels {total:.2f} ms, wall {ms:.2f} ms (event-bracketed launches); "
              + ", ".join(f"{k} {v:.3f} ms" for k, v in glue.items())
              + f"; error + control + commit = {tail / total:.4f} of the kernel time = {tail / trials * 1e3:.1f} us per trial step of "
              f"{total / trials:.2f} ms; with ode_stage_rows {(tail + glue['ode_stage_rows']) / total:.4f}")
