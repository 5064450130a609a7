"""Compensated 16-bit operands for the PE-AV towers: `SAMAudioJudgeModel` / `PEAudioFrame` with precision "fp16x3" / "bf16x3"
(include/samaudio.h samaudio_judge_set_option).

fp32 storage; the four GEMMs of every transformer layer, the two k3 convolutions of the ResNet block, the self-attention, the
output projection and the Judge's cat_audio_proj multiply hi/lo-split 16-bit operands.  The bound of every parity check here is the
project's bar - 1e-3 max-abs, times max(1, |reference|max) where values exceed 1 - for BOTH half formats; the measured errors are
printed through util.report.  On the CPU simulator (SAMAUDIO_EMU_DRYRUN: the bfloat16 library only) the bf16x3 form exercises the
same kernels, layouts and plumbing.
"""
import ctypes as C
import json
import os

import pytest
import torch

from oracle import gen_golden_judge as G
from oracle import judge_oracle as J
from oracle import samaudio_oracle as O
from sam_audio_amd import hip
from sam_audio_amd.config import PEAudioFrameConfig, PEAVTransformerConfig
from sam_audio_amd.synthetic import (init_frame_state_dict, init_judge_state_dict, init_peav_state_dict, make_hostile_peav,
                                     synthetic_clip)
from tests import util
from tests.test_zz_next_rows_gpu import TINY_TEXT, _cfg, _judge, _judge_case

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
X3 = ["bf16x3"] if SIM else ["fp16x3", "bf16x3"]
HALF = {"fp16x3": torch.float16, "bf16x3": torch.bfloat16}
PLAIN = {"fp16x3": "fp16", "bf16x3": "bf16"}   # the plain 16-bit mode of the same library
BAR = 1e-3                                     # the project's parity bar


def _bar(want):
    return BAR * max(1.0, want.abs().max().item())


# ---------------------------------------------------------------------------------------------------- 1: the new kernel
@pytest.mark.parametrize("prec", X3)
def test_masked_groupnorm_silu_split3(gpu, prec):
    """Split-form output of the masked GroupNorm + SiLU against the fp32 kernel of the same library: hi + lo is its value to the
    split's own bound (2^-21 relative for IEEE half - half a quantum 2^-25 where lo is subnormal -, 2^-15 for bfloat16), both hi
    thirds are the same bits, masked rows are zeros in all three thirds, halo rows are not touched."""
    lib = hip.lib(hip.operands_for(prec))
    B, S, Cc, halo = 3, 37, 256, 1
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, S, Cc, generator=g) * 1.5 + 0.3
    w, b = torch.randn(Cc, generator=g) * 0.2 + 1, torch.randn(Cc, generator=g) * 0.1
    mask = torch.arange(S)[None] < torch.tensor([37, 20, 1])[:, None]
    want = torch.nn.functional.silu(J.masked_group_norm_1(x, mask, w, b))
    xd, wd, bd, md = x.to(gpu), w.to(gpu), b.to(gpu), mask.to(gpu).to(torch.uint8)   # kept alive across the launches
    part = torch.empty(B * 64 * 3, dtype=torch.float64, device=gpu)
    ref = torch.full((B, S + 2 * halo, Cc), float("nan"), device=gpu)
    hip.check(lib.samaudio_op_masked_groupnorm_silu(hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(md), hip.ptr(part), hip.ptr(ref),
                                                    hip.F32, B, S, Cc, halo, 1e-5, util.stream()))
    out = torch.full((B, S + 2 * halo, 3 * Cc), float("nan"), dtype=HALF[prec], device=gpu)
    hip.check(lib.samaudio_op_masked_groupnorm_silu_split3(hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(md), hip.ptr(part),
                                                           hip.ptr(out), B, S, Cc, halo, 1e-5, util.stream()))
    out, ref = out.cpu(), ref.cpu()[:, halo:halo + S]
    assert torch.isnan(out[:, 0].float()).all() and torch.isnan(out[:, -1].float()).all(), "halo rows were touched"
    body = out[:, halo:halo + S]
    lo, hi, hi2 = body[..., :Cc].float(), body[..., Cc:2 * Cc].float(), body[..., 2 * Cc:].float()
    assert torch.equal(hi, hi2), "the two hi thirds differ"
    assert (body[~mask].float() == 0).all(), "masked rows are not zero in all three thirds"
    util.report(f"masked groupnorm (fp32 kernel) {prec}", ref, want, 1e-4)
    rel, floor = (2.0 ** -21, 2.0 ** -25) if prec == "fp16x3" else (2.0 ** -15, 0.0)
    err, bound = (hi + lo - ref).abs(), (ref.abs() * rel).clamp_min(floor)
    print(f"masked groupnorm split3 {prec}: max |hi + lo - fp32| / bound = {(err / bound.clamp_min(1e-45)).max().item():.3f}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------- 2, 3: one transformer
def _encode(m, z, mask, gpu):
    rows, T, _ = z.shape
    D = m.config.transformer.hidden_size
    hidden = torch.empty(rows, T + 1, D, device=gpu)
    pm = mask.to(gpu).to(torch.uint8).contiguous() if mask is not None else None
    m.ensure_workspace(rows, 1, T)
    zd = z.to(gpu).contiguous()
    hip.check(m._lib.samaudio_judge_encode(m._h, 0, hip.ptr(zd), hip.ptr(pm), rows, T, hip.ptr(hidden), util.stream()))
    return hidden.cpu()


def _transformer_case(tc, rows, T, lengths, seed=5):
    g = torch.Generator().manual_seed(seed)
    psd = init_peav_state_dict(tc, "transformer.", g, torch.device("cpu"))
    mask = torch.arange(T)[None] < torch.tensor(lengths)[:, None]
    cfg = _cfg(codec=dict(codebook_dim=64))
    cfg.transformer = tc
    sd = init_judge_state_dict(cfg, seed=9, with_codec=False)
    sd.update(psd)
    z = torch.randn(rows, T, 64, generator=g)
    return cfg, sd, z, mask


def _oracle_transformer(sd, tc, z, mask):
    xin = torch.nn.functional.linear(z, sd["data_proj.weight"], sd["data_proj.bias"])
    with torch.inference_mode():
        return J.peav_transformer(sd, "transformer.", xin, mask, n_heads=tc.num_attention_heads, n_layers=tc.num_hidden_layers,
                                  eps=tc.rms_norm_eps, rope_theta=tc.rope_theta)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("masked", [True, False])
def test_peav_transformer_x3_matches_oracle(gpu, prec, masked):
    """One PE-AV transformer through samaudio_judge_encode at the tiny config (B=3, T=21, lengths 21/13/6): few rows, i.e. the
    128x128 walk of the 8-phase family, N = 2 * 448 = 896 a half tile."""
    tc = PEAVTransformerConfig(**G.TINY_TC)
    cfg, sd, z, mask = _transformer_case(tc, 3, 21, [21, 13, 6])
    last, pooled = _oracle_transformer(sd, tc, z, mask if masked else None)
    hidden = _encode(_judge(cfg, sd, prec, gpu), z, mask if masked else None, gpu)
    valid = (mask if masked else torch.ones_like(mask))[..., None]
    util.report(f"peav x3 pooled {prec}", hidden[:, 0], pooled, _bar(pooled))
    util.report(f"peav x3 last_hidden {prec}", hidden[:, 1:] * valid, last * valid, _bar(last * valid))


TOWER_BITS = ("qkv", "wo", "w13", "w2", "patch")


@pytest.mark.parametrize("prec", X3)
def test_peav_x3_per_class_masks(gpu, prec):
    """Every class bit of SAMAUDIO_CLS_X3_TOWER alone, and all of them but wo, on one transformer through samaudio_judge_encode
    (2 rows, T = 50 with lengths 50 / 9: S = 51 is no multiple of 64 and the second row has a masked tail).  Only the twins of the
    classes that are switched on are registered; finalize takes that, and the result is inside the bound of the full-mask test above
    (the classes left in fp32 are exact, so a subset cannot need a wider one)."""
    from sam_audio_amd.judge import convert_judge, convert_judge_x3
    tc = PEAVTransformerConfig(**G.TINY_TC)
    cfg, sd, z, mask = _transformer_case(tc, 2, 50, [50, 9])
    last, pooled = _oracle_transformer(sd, tc, z, mask)
    valid = mask[..., None]
    single = [hip.CLS[b] for b in TOWER_BITS] + [hip.X3_ATTENTION]
    assert sum(single) == hip.CLS_X3_TOWER
    for classes in single + [hip.CLS_X3_TOWER & ~hip.CLS["wo"]]:
        m = _judge_unloaded(cfg, prec, gpu)
        hip.check(m._lib.samaudio_judge_set_option(m._h, hip.OPT_X3_CLASSES, classes))
        tensors = convert_judge(sd, cfg, torch.float32, gpu)
        tensors.update(convert_judge_x3(tensors, cfg, HALF[prec], classes))
        m.register(tensors)
        hip.check(m._lib.samaudio_judge_finalize(m._h))
        hidden = _encode(m, z, mask, gpu)
        util.report(f"peav x3 classes {classes:#x} pooled {prec}", hidden[:, 0], pooled, _bar(pooled))
        util.report(f"peav x3 classes {classes:#x} last_hidden {prec}", hidden[:, 1:] * valid, last * valid, _bar(last * valid))


def _judge_unloaded(cfg, prec, gpu):
    from sam_audio_amd.judge import SAMAudioJudgeModel
    return SAMAudioJudgeModel(cfg, precision=prec, device=str(gpu), text_model=G.text_tower(cfg))


@pytest.mark.skipif(SIM, reason="the 256x256 sharing walk at pe-av-large width: MI355X only (hours on the simulator)")
@pytest.mark.parametrize("prec", X3)
def test_peav_layer_at_large_width_on_the_sharing_walk(gpu, prec):
    """One layer at pe-av-large width (hidden 1792, 14 heads, intermediate 4800), 20 items x 240 frames = 4 820 rows = 19 row tiles
    with 212 rows in the last, N = 9 600 = 37.5 column tiles: the smallest shape at which gemm_variant sends all four layer classes
    to the 256x256 kernel (operand-sharing walk) with partial tiles in both directions.  Ragged lengths, same oracle."""
    tc = PEAVTransformerConfig(hidden_size=1792, intermediate_size=4800, num_hidden_layers=1, num_attention_heads=14)
    lengths = [240 - 11 * i for i in range(20)]
    cfg, sd, z, mask = _transformer_case(tc, 20, 240, lengths, seed=6)
    last, pooled = _oracle_transformer(sd, tc, z, mask)
    hidden = _encode(_judge(cfg, sd, prec, gpu), z, mask, gpu)
    valid = mask[..., None]
    util.report(f"peav x3 large pooled {prec}", hidden[:, 0], pooled, _bar(pooled))
    util.report(f"peav x3 large last_hidden {prec}", hidden[:, 1:] * valid, last * valid, _bar(last * valid))


# ---------------------------------------------------------------------------------------------------- 4: Judge
@pytest.mark.parametrize("prec", X3)
def test_judge_x3_forward_matches_oracle(gpu, prec):
    cfg = _cfg()
    sd = init_judge_state_dict(cfg, seed=9)
    inp = _judge_case(cfg)
    tm = G.text_tower(cfg)
    pooled = G.text_pooled(tm, cfg, inp["input_ids"], inp["attention_mask"])
    with torch.inference_mode():
        want = J.judge_forward(sd, cfg, pooled, inp["input_values"], inp["separated_values"], inp["padding_mask"])
    m = _judge(cfg, sd, prec, gpu, text_model=tm)
    out = m(**{k: v.to(gpu) for k, v in inp.items()})
    got = torch.cat([out.overall, out.recall, out.precision, out.faithfulness], dim=1)
    util.report(f"judge x3 scores {prec}", got, want, _bar(want))
    assert out.overall.shape == (2, 1)


@pytest.mark.parametrize("prec", X3)
def test_judge_x3_candidate_dedup_equals_the_expanded_batch(gpu, prec):
    cfg = _cfg()
    sd = init_judge_state_dict(cfg, seed=9)
    cand = 3
    inp = _judge_case(cfg, B=2, T=5, cand=cand)
    tm = G.text_tower(cfg)
    pooled = G.text_pooled(tm, cfg, inp["input_ids"], inp["attention_mask"]).repeat_interleave(cand, 0)
    m = _judge(cfg, sd, prec, gpu, text_model=tm)
    scores = m.score_candidates(inp["input_ids"].to(gpu), inp["input_values"].to(gpu), inp["separated_values"].to(gpu),
                                cand, attention_mask=inp["attention_mask"].to(gpu), padding_mask=inp["padding_mask"].to(gpu))
    expanded = m(input_ids=inp["input_ids"].repeat_interleave(cand, 0).to(gpu),
                 attention_mask=inp["attention_mask"].repeat_interleave(cand, 0).to(gpu),
                 input_values=inp["input_values"].repeat_interleave(cand, 0).to(gpu),
                 separated_values=inp["separated_values"].to(gpu),
                 padding_mask=inp["padding_mask"].repeat_interleave(cand, 0).to(gpu))
    assert scores.shape == (2, cand)
    util.report(f"x3 dedup vs expanded {prec}", scores.reshape(-1, 1), expanded.overall.cpu(), 1e-5)
    with torch.inference_mode():
        want = J.judge_forward(sd, cfg, pooled, inp["input_values"].repeat_interleave(cand, 0), inp["separated_values"],
                               inp["padding_mask"].repeat_interleave(cand, 0))
    util.report(f"x3 dedup vs oracle {prec}", scores.reshape(-1), want[:, 0], _bar(want[:, 0]))


# ---------------------------------------------------------------------------------------------------- 5: PE-A-Frame
def _frame_case():
    cfg = PEAudioFrameConfig(audio=G.TINY_TC, text_model=dict(TINY_TEXT, hidden_size=64), codebook_dim=128)
    g = torch.Generator().manual_seed(6)
    B, T = 3, 50
    feats = torch.randn(B, T, 128, generator=g)
    pooled = torch.randn(B, cfg.text_hidden, generator=g)
    pad = torch.arange(T)[None] < torch.tensor([50, 31, 9])[:, None]
    return cfg, feats, pooled, pad


def _frame(cfg, sd, prec, gpu):
    import transformers
    from sam_audio_amd.judge import PEAudioFrame
    torch.manual_seed(1)
    tm = transformers.ModernBertModel(transformers.ModernBertConfig(**cfg.text_model)).eval()
    fp = PEAudioFrame(cfg, precision=prec, device=str(gpu), text_model=tm)
    fp.load_state_dict(sd, strict=False)
    return fp


@pytest.mark.parametrize("prec", X3)
def test_frame_x3_logits_and_spans_match_oracle(gpu, prec):
    cfg, feats, pooled, pad = _frame_case()
    sd = init_frame_state_dict(cfg, seed=2)
    with torch.inference_mode():
        want = J.frame_logits(sd, cfg, pooled, feats, pad)
    out = _frame(cfg, sd, prec, gpu)(input_features=feats.to(gpu), padding_mask=pad.to(gpu), return_spans=True,
                                     text_pooled=pooled.to(gpu))
    util.report(f"frame x3 logits {prec}", out.logits.cpu() * pad, want * pad, _bar(want * pad))
    margin = (want.abs() > 1e-2) | ~pad                                     # frames not sitting on the threshold
    ids_w, al_w = O.anchors_to_ids([[("+", s, e) for s, e in r] for r in J.spans_from_logits(want, pad, 1920, 48000)],
                                   pad, 1920, 48000)
    ids_g, al_g = O.anchors_to_ids([[("+", s, e) for s, e in r] for r in out.spans], pad, 1920, 48000)
    assert torch.equal((al_w >= 2) & margin, (al_g >= 2) & margin), "span frames differ away from the threshold"


# ---------------------------------------------------------------------------------------------------- 6: hostile weights
def _err(got, want):
    return (got.float().cpu() - want).abs().max().item()


@pytest.mark.parametrize("prec", X3)
def test_hostile_tower_weights_stay_inside_the_bar(gpu, prec):
    """Trained-like statistics (synthetic.make_hostile_peav: outlier channels, log-normal norm gains, GroupNorm gains over a decade)
    on the tiny dims: Judge scores and frame logits in the x3 mode are inside the bar; the plain 16-bit mode of the same library
    runs beside it and its error is printed, not asserted."""
    cfg = _cfg()
    sd = init_judge_state_dict(cfg, seed=9)
    sd = make_hostile_peav(sd, "transformer.", cfg.transformer, seed=1, in_proj="data_proj")
    sd = make_hostile_peav(sd, "finetune_transformer.", cfg.finetune_transformer, seed=2, in_proj="finetune_data_proj")
    inp = _judge_case(cfg)
    tm = G.text_tower(cfg)
    pooled = G.text_pooled(tm, cfg, inp["input_ids"], inp["attention_mask"])
    with torch.inference_mode():
        want = J.judge_forward(sd, cfg, pooled, inp["input_values"], inp["separated_values"], inp["padding_mask"])
    got = {}
    for p in (PLAIN[prec], prec):
        out = _judge(cfg, sd, p, gpu, text_model=tm)(**{k: v.to(gpu) for k, v in inp.items()})
        got[p] = torch.cat([out.overall, out.recall, out.precision, out.faithfulness], dim=1)
    print(f"hostile judge scores, plain {PLAIN[prec]}: max-abs err {_err(got[PLAIN[prec]], want):.3e} (printed, not asserted)")
    util.report(f"hostile judge scores {prec}", got[prec], want, _bar(want))

    fcfg, feats, fpooled, pad = _frame_case()
    fsd = init_frame_state_dict(fcfg, seed=2)
    fsd = make_hostile_peav(fsd, "audio_encoder.", fcfg.audio, seed=3, in_proj="audio_encoder.embedder.data_proj")
    with torch.inference_mode():
        fwant = J.frame_logits(fsd, fcfg, fpooled, feats, pad) * pad
    logits = {p: _frame(fcfg, fsd, p, gpu).frame_logits(feats.to(gpu), fpooled.to(gpu), pad.to(gpu)).cpu() * pad
              for p in (PLAIN[prec], prec)}
    print(f"hostile frame logits, plain {PLAIN[prec]}: max-abs err {_err(logits[PLAIN[prec]], fwant):.3e} (printed, not asserted)")
    util.report(f"hostile frame logits {prec}", logits[prec], fwant, _bar(fwant))


# ---------------------------------------------------------------------------------------------------- 7: workspace
@pytest.mark.parametrize("prec", X3)
def test_judge_x3_workspace_is_exactly_what_the_plan_takes(gpu, prec):
    """The score of the dedup case in a NaN-poisoned buffer of exactly samaudio_judge_workspace_bytes followed by a canary tail:
    the result is the oracle's, the canary is intact; one plan unit less is refused with SAMAUDIO_ERR_WORKSPACE."""
    cfg = _cfg()
    sd = init_judge_state_dict(cfg, seed=9)
    cand = 3
    inp = _judge_case(cfg, B=2, T=5, cand=cand)
    tm = G.text_tower(cfg)
    pooled = G.text_pooled(tm, cfg, inp["input_ids"], inp["attention_mask"]).repeat_interleave(cand, 0)
    with torch.inference_mode():
        want = J.judge_forward(sd, cfg, pooled, inp["input_values"].repeat_interleave(cand, 0), inp["separated_values"],
                               inp["padding_mask"].repeat_interleave(cand, 0))
    m = _judge(cfg, sd, prec, gpu, text_model=tm)
    lat = m._codec.encode(torch.cat([inp["input_values"], inp["separated_values"]], dim=0).to(gpu))
    in_lat, sep_lat = lat[:2].contiguous(), lat[2:].contiguous()
    frames = in_lat.shape[1]
    mask = m._frame_mask(inp["padding_mask"]).to(gpu).to(torch.uint8).contiguous()
    pd = pooled.to(gpu).float().contiguous()
    need = m._lib.samaudio_judge_workspace_bytes(m._h, 2, cand, frames)
    canary = 1 << 20
    buf = torch.full((need + 256 + canary,), 255, dtype=torch.uint8, device=gpu)   # 0xFF bytes: NaN as fp32 and as 16-bit
    off = (-buf.data_ptr()) % 256
    scores = torch.empty(2 * cand, 4, device=gpu)

    def score(nbytes):
        hip.check(m._lib.samaudio_judge_set_workspace(m._h, C.c_void_p(buf.data_ptr() + off), nbytes))
        hip.check(m._lib.samaudio_judge_score(m._h, hip.ptr(in_lat), hip.ptr(sep_lat), 2, cand, frames, hip.ptr(pd), hip.ptr(mask),
                                              hip.ptr(scores), util.stream()))

    with pytest.raises(hip.SamAudioHipError, match=r"\[-3\]"):
        score(need - 4096 - 256)   # workspace_bytes = the plan + 4096; the plan is carved in 256-byte units
    score(need)
    util.report(f"x3 judge in an exact workspace {prec}", scores[:, 0], want[:, 0], _bar(want[:, 0]))
    tail = buf[off + need:].cpu()
    assert (tail == 255).all(), f"{int((tail != 255).sum())} canary bytes behind a {need}-byte workspace were written"
    print(f"x3 judge workspace (2 clips x {cand} candidates x {frames} frames, tiny dims): {need} bytes")


# ---------------------------------------------------------------------------------------------------- 8: option errors
def test_tower_x3_option_errors(gpu):
    """No launch: the option on a 16-bit context and a non-tower bit are SAMAUDIO_ERR_ARG; finalize without a twin of a class that is
    switched on is SAMAUDIO_ERR_WEIGHT and names the twin."""
    from sam_audio_amd.judge import SAMAudioJudgeModel, PEAudioFrame, convert_judge
    cfg = _cfg()
    tm = G.text_tower(cfg)
    lib = hip.lib()
    m16 = SAMAudioJudgeModel(cfg, precision="bf16", device=str(gpu), text_model=tm)
    assert lib.samaudio_judge_set_option(m16._h, hip.OPT_X3_CLASSES, hip.CLS["qkv"]) == hip.ERR_ARG
    assert lib.samaudio_judge_set_option(m16._h, hip.OPT_X3_CLASSES, 0) == 0
    m32 = SAMAudioJudgeModel(cfg, precision="fp32", device=str(gpu), text_model=tm)
    for bit in ("cwq", "cwo", "ckv", "codec", "out"):
        assert lib.samaudio_judge_set_option(m32._h, hip.OPT_X3_CLASSES, hip.CLS_X3_TOWER | hip.CLS[bit]) == hip.ERR_ARG, bit
    assert lib.samaudio_judge_set_option(m32._h, hip.OPT_X3_CLASSES + 100, 0) == hip.ERR_ARG
    fcfg = PEAudioFrameConfig(audio=G.TINY_TC, text_model=dict(TINY_TEXT, hidden_size=64), codebook_dim=128)
    f16 = PEAudioFrame(fcfg, precision="bf16", device=str(gpu), text_model=tm)
    assert lib.samaudio_frame_set_option(f16._h, hip.OPT_X3_CLASSES, hip.X3_ATTENTION) == hip.ERR_ARG
    f32 = PEAudioFrame(fcfg, precision="fp32", device=str(gpu), text_model=tm)
    assert lib.samaudio_frame_set_option(f32._h, hip.OPT_X3_CLASSES, hip.CLS["cwq"]) == hip.ERR_ARG
    assert lib.samaudio_frame_set_option(f32._h, hip.OPT_X3_CLASSES, hip.CLS_X3_TOWER) == 0
    # a missing twin
    assert lib.samaudio_judge_set_option(m32._h, hip.OPT_X3_CLASSES, hip.CLS["w2"]) == 0
    sd = init_judge_state_dict(cfg, seed=9, with_codec=False)
    m32.register(convert_judge(sd, cfg, torch.float32, gpu))
    assert lib.samaudio_judge_finalize(m32._h) == hip.ERR_WEIGHT
    assert "t.L0.w2.x3" in lib.samaudio_last_error().decode()
    assert lib.samaudio_judge_set_option(m32._h, hip.OPT_X3_CLASSES, 0) == 0
    assert lib.samaudio_judge_finalize(m32._h) == 0, "with the mask at 0 the fp32 tensors alone finalize"


# ---------------------------------------------------------------------------------------------------- 9: separate() reranking
def test_separate_reranking_with_an_x3_judge_picks_the_oracles_argmax(gpu, tmp_path):
    """separate(reranking_candidates=3) with a Judge loaded from a checkpoint directory through JudgeRanker(tower_precision="fp16x3"
    / "bf16x3"): the returned target is the candidate the CPU oracle of the Judge scores highest."""
    from sam_audio_amd import SAMAudio, SAMAudioProcessor, preset_config
    from sam_audio_amd.config import JudgeRankerConfig
    from sam_audio_amd.processor import SAMAudioJudgeProcessor
    from sam_audio_amd.ranking import JudgeRanker
    from sam_audio_amd.synthetic import init_state_dict, synthetic_noise, synthetic_text_features
    from tests.test_judge_host_cpu import _Tok
    prec = X3[0]
    cand = 3
    cfg = preset_config("tiny")
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 6 * hop) for i in range(2)]
    text, tmask = synthetic_text_features(2, 4)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["dog", "rain"], audios=clips, text_features=text,
                                               text_mask=tmask).to(gpu)
    model = SAMAudio(cfg, precision="fp32", device=str(gpu))
    model.load_state_dict(init_state_dict(cfg, seed=3))
    # the Judge as a local checkpoint directory (config.json + checkpoint.pt, text tower included)
    jcfg = _cfg()
    jsd = init_judge_state_dict(jcfg, seed=9)
    tm = G.text_tower(jcfg)
    ckpt = dict(jsd)
    ckpt.update({"text_model." + k: v for k, v in tm.state_dict().items()})
    with open(tmp_path / "config.json", "w") as f:
        json.dump(dict(transformer=G.TINY_TC, finetune_transformer=G.TINY_FT, text_model=TINY_TEXT, nth_text_layer=2,
                       bottleneck_dim=64), f)
    torch.save(ckpt, tmp_path / "checkpoint.pt")
    jproc = SAMAudioJudgeProcessor(hop, 48000, tokenizer=_Tok())
    ranker = JudgeRanker(JudgeRankerConfig(checkpoint_or_model_id=str(tmp_path)), processor=jproc, tower_precision=prec,
                         device=str(gpu))
    assert ranker.model.precision == prec
    seen = {}

    def spy(**kw):
        seen["kw"] = dict(descriptions=list(kw["descriptions"]), input_audio=[x.cpu() for x in kw["input_audio"]],
                          extracted_audio=[[c.cpu() for c in row] for row in kw["extracted_audio"]])
        seen["scores"] = ranker(**kw)
        return seen["scores"]

    model.text_ranker = spy
    # candidates that the REFERENCE can tell apart: start states of different amplitude (seeded noise alone gives this tiny DiT
    # three near-identical separations, which the fp32 oracle scores within one ulp of each other - no argmax to speak of)
    noise = synthetic_noise(2 * cand, 6) * torch.tensor([0.25, 1.0, 4.0]).repeat(2)[:, None, None]
    res = model.separate(batch, noise=noise.to(gpu), reranking_candidates=cand)
    assert seen["scores"].shape == (2, cand)
    # the oracle on what the ranker was handed
    kw = seen["kw"]
    mixtures = [x[0][None] for x in kw["input_audio"]]
    extracted = [x[None] for cands in kw["extracted_audio"] for x in cands]
    processed = jproc(text=list(kw["descriptions"]), input_audio=mixtures, separated_audio=extracted, sampling_rate=48000)
    pooled = G.text_pooled(tm, jcfg, processed["input_ids"], processed.get("attention_mask")).repeat_interleave(cand, 0)
    with torch.inference_mode():
        want = J.judge_forward(jsd, jcfg, pooled, processed["input_values"].repeat_interleave(cand, 0),
                               processed["separated_values"], processed["padding_mask"].repeat_interleave(cand, 0))[:, 0].view(2, cand)
    util.report(f"reranker scores {prec}", seen["scores"], want, _bar(want))
    top2 = want.topk(2, dim=1).values
    print(f"oracle scores {want.tolist()}, gap between the best two candidates {(top2[:, 0] - top2[:, 1]).tolist()}")
    # the oracle's argmax exists only where its best two scores differ by more than the oracle's own error: the fp32 oracle is held
    # to 1e-4 x max(1, |score|) of its float64 form (tests/test_towers_x3_cpu.py), so a smaller gap means the INPUTS are unfit
    assert (top2[:, 0] - top2[:, 1]).min().item() > 1e-4 * max(1.0, want.abs().max().item()), "the oracle itself cannot rank these candidates"
    pick = want.argmax(dim=1).tolist()
    assert seen["scores"].argmax(dim=1).tolist() == pick, "the x3 Judge ranks another candidate first than its oracle"
    lat = model.last_latent.view(2, cand, 6, -1)
    half = lat.shape[-1] // 2
    for b in range(2):
        wav = model.decode_audio(lat[b, pick[b], :, :half][None].contiguous())[0]
        assert torch.allclose(res.target[b], wav[: res.target[b].numel()], atol=1e-5)
