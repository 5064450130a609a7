#!/usr/bin/env python
"""The Judge and the span predictor alone, in the exact-fp32 mode, the plain 16-bit mode and the compensated mode (fp16x3) of the
fp16 library: ms per call and the error of each mode against the fp32 mode, on benign and on hostile (make_hostile_peav) weights.

Shapes of bench.py's configs[3]: Judge 8 clips x 8 candidates x 250 frames at pe-av-large, span predictor 8 x 250.  The codec and
the text tower are left out (latents and pooled text rows are the inputs): what is timed is samaudio_judge_score /
samaudio_frame_logits.  The three modes alternate inside one process after a warm-up; device events, medians of REPS >= 8.

usage: python tools/tower_probe.py [reps] [--once MODE]     (--once: three calls of one mode, for rocprofv3 --kernel-trace --stats)
The reference of the error columns is the library's fp32 mode (itself held to the CPU oracle by tests/test_zz_next_rows_gpu.py):
the CPU oracle at these dims is minutes of work per weight set."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd.config import PEAudioFrameConfig, SAMAudioJudgeConfig  # noqa: E402
from sam_audio_amd.judge import PEAudioFrame, SAMAudioJudgeModel  # noqa: E402
from sam_audio_amd.synthetic import init_frame_state_dict, init_judge_state_dict, make_hostile_peav  # noqa: E402

MODES = ("fp32", "fp16", "fp16x3")
TEXT = dict(hidden_size=1024, intermediate_size=2624, num_hidden_layers=2, num_attention_heads=16, vocab_size=128,
            pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2, global_attn_every_n_layers=2,
            local_attention=8, max_position_embeddings=64)
CLIPS, CAND, FRAMES = 8, 8, 250
dev = torch.device("cuda:0")


def text_tower():
    import transformers
    torch.manual_seed(1)
    return transformers.ModernBertModel(transformers.ModernBertConfig(**TEXT)).eval()


def judges(hostile, modes):
    cfg = SAMAudioJudgeConfig(text_model=TEXT, nth_text_layer=None)
    sd = init_judge_state_dict(cfg, seed=9, device="cpu", with_codec=False)
    if hostile:
        sd = make_hostile_peav(sd, "transformer.", cfg.transformer, seed=1, in_proj="data_proj")
        sd = make_hostile_peav(sd, "finetune_transformer.", cfg.finetune_transformer, seed=2, in_proj="finetune_data_proj")
    out = {}
    for p in modes:
        m = SAMAudioJudgeModel(cfg, precision=p, device=str(dev), text_model=text_tower())
        m.load_state_dict(sd, strict=False)
        out[p] = m
    g = torch.Generator().manual_seed(3)
    args = (torch.randn(CLIPS, FRAMES, cfg.audio_codec.codebook_dim, generator=g).to(dev),
            torch.randn(CLIPS * CAND, FRAMES, cfg.audio_codec.codebook_dim, generator=g).to(dev), CAND,
            torch.randn(CLIPS * CAND, cfg.text_hidden, generator=g).to(dev),
            (torch.arange(FRAMES)[None] < torch.tensor([250, 250, 231, 250, 198, 250, 250, 127])[:, None]).to(dev))
    return {p: (lambda m=m: m._score(*args)) for p, m in out.items()}, out


def frames(hostile, modes):
    cfg = PEAudioFrameConfig(text_model=TEXT)
    sd = init_frame_state_dict(cfg, seed=2)
    if hostile:
        sd = make_hostile_peav(sd, "audio_encoder.", cfg.audio, seed=3, in_proj="audio_encoder.embedder.data_proj")
    out = {}
    for p in modes:
        f = PEAudioFrame(cfg, precision=p, device=str(dev), text_model=text_tower())
        f.load_state_dict(sd, strict=False)
        out[p] = f
    g = torch.Generator().manual_seed(4)
    args = (torch.randn(CLIPS, FRAMES, cfg.codebook_dim, generator=g).to(dev), torch.randn(CLIPS, cfg.text_hidden, generator=g).to(dev),
            (torch.arange(FRAMES)[None] < torch.tensor([250, 250, 231, 250, 198, 250, 250, 127])[:, None]).to(dev))
    return {p: (lambda f=f: f.frame_logits(*args) * args[2]) for p, f in out.items()}, out


def measure(name, calls, reps):
    res = {}
    outs = {p: fn().float().cpu() for p, fn in calls.items()}   # (first call: workspace allocation)
    for p in calls:
        calls[p]()
    torch.cuda.synchronize()
    ms = {p: [] for p in calls}
    for _ in range(reps):   # the modes alternate: clock and neighbour effects hit all of them alike
        for p, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[p].append(e0.elapsed_time(e1))
    ref = outs["fp32"]
    for p in calls:
        res[p] = dict(ms_median=statistics.median(ms[p]), ms_min=min(ms[p]), ms_max=max(ms[p]),
                      max_abs_err_vs_fp32=(outs[p] - ref).abs().max().item(), ref_absmax=ref.abs().max().item())
        print(f"{name:28s} {p:7s} {res[p]['ms_median']:9.3f} ms (min {res[p]['ms_min']:.3f}, max {res[p]['ms_max']:.3f}; {reps} reps)   "
              f"max-abs err vs fp32 {res[p]['max_abs_err_vs_fp32']:.3e} on |ref| <= {res[p]['ref_absmax']:.3f}", flush=True)
    return res


def main():
    if "--once" in sys.argv:
        mode = sys.argv[sys.argv.index("--once") + 1]
        for build in (judges, frames):
            calls, keep = build(False, (mode,))
            for _ in range(3):
                calls[mode]()
            torch.cuda.synchronize()
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    result = {}
    for hostile in (False, True):
        tag = "hostile" if hostile else "benign"
        calls, keep = judges(hostile, MODES)
        result[f"judge_{tag}"] = measure(f"judge 8x8x250 ({tag})", calls, reps)
        if not hostile:
            ws = {p: m._lib.samaudio_judge_workspace_bytes(m._h, CLIPS, CAND, FRAMES) for p, m in keep.items()}
            result["judge_workspace_bytes"] = ws
            print("judge workspace bytes:", ws, flush=True)
        del calls, keep
        torch.cuda.empty_cache()
        calls, keep = frames(hostile, MODES)
        result[f"frame_{tag}"] = measure(f"span predictor 8x250 ({tag})", calls, reps)
        if not hostile:
            ws = {p: f._lib.samaudio_frame_workspace_bytes(f._h, CLIPS, FRAMES) for p, f in keep.items()}
            result["frame_workspace_bytes"] = ws
            print("span predictor workspace bytes:", ws, flush=True)
        del calls, keep
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
