"""Text-length, clip-length and candidate edges of the DiT (reference transformer.py:382-388, model.py:170-203), every precision.

The other model-level tests feed a short text memory (3-8 tokens) beside a longer clip.  Real prompts are longer (T5 gives 17+ tokens for
a sentence, pad_mode='max_length' 512) and real clips can be short (1 s = 25 frames): here the text memory is as long as or longer than
the clip, around the fold slots of the cross-attention (8 / 16 tokens), with candidates, with ragged clips and masks, under a workspace
guard (tests/util.py workspace_guard) that turns a write past the workspace plan into an assertion.  Each case runs separate() between
its encode and its decode - samaudio_prepare_latent and the euler ODE solve, on the oracle's codec latent - and compares the final
latent with the fp32 oracle on the CPU.  On the simulator (SAMAUDIO_EMU_DRYRUN=simt: bfloat16 library only) the precisions that build
carries run: fp32, bf16 and bf16x3.
"""
import math
import os
import re

import pytest
import torch

from oracle import samaudio_oracle as O
from sam_audio_amd import SAMAudio, SAMAudioProcessor, hip, preset_config
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
from tests import util

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
X3 = ["bf16x3"] if SIM else ["fp16x3", "bf16x3"]
PRECS = ["fp32", "bf16"] + ([] if SIM else ["fp16"]) + X3
# the bounds of the same call elsewhere: fp32 / fp16x3 / bf16x3 tests/test_x3_gpu.py (cross-attention test), fp16
# tests/test_fp16_gpu.py; bf16: 2 x the largest error measured on MI355X over this file's cases (4.11e-3, T=6 Lt=32; the simulator
# gives 4.17e-3 for the same case)
TOL = {"fp32": 1e-3, "fp16x3": 1e-4, "bf16x3": 1e-3, "fp16": 1.5e-3, "bf16": 8.5e-3}
OPT = {"method": "euler", "options": {"step_size": 0.5}}


@pytest.fixture(autouse=True)
def _folds_on(monkeypatch):
    """The cases here are about the folded cross-attention forms too: another test module's SAMAUDIO_NO_FOLD (tests/test_emu_cpu.py sets
    it when it is imported) must not switch them off; the launcher emulation (SAMAUDIO_EMU_DRYRUN=1) has no fold kernels."""
    if os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != "1":
        monkeypatch.delenv("SAMAUDIO_NO_FOLD", raising=False)


_SD = {}


def _state_dict(cfg, key="tiny"):
    if key not in _SD:
        _SD[key] = init_state_dict(cfg, seed=5)
    return _SD[key]


def _model(cfg, sd, prec, gpu, **kw):
    model = SAMAudio(cfg, precision=prec, device=str(gpu), **kw)
    model.load_state_dict(sd, strict=False)
    return model


def _case(cfg, sd, lengths, text_len, cand=1, mask=None):
    """clips of `lengths` frames, a ragged text mask (or `mask`), the oracle's codec latent and final latent"""
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, n * hop) for i, n in enumerate(lengths)]
    text, tmask = synthetic_text_features(len(lengths), text_len, ragged=True)
    if mask is not None:
        tmask = mask
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * len(lengths), audios=clips, text_features=text, text_mask=tmask)
    noise = synthetic_noise(len(lengths) * cand, max(lengths))
    with torch.inference_mode():
        _, _, lat_ref = O.separate(sd, cfg, batch.audios, batch.sizes.long(), text, tmask, noise, candidates=cand, method="euler",
                                   step_size=0.5, decode=False)
        z = O.dac_encode(sd, cfg.audio_codec, batch.audios).transpose(1, 2).contiguous()
    return dict(z=z, text=text, tmask=tmask, ids=batch.anchor_ids, align=batch.anchor_alignment, pad=batch.audio_pad_mask, noise=noise,
                cand=cand), lat_ref


def _prepare(model, c, gpu):
    """samaudio_prepare_latent with the conditioning separate() passes (model.py:756)"""
    model._apply_options(1)
    model._prepare(c["z"].to(gpu), c["text"].to(gpu), c["tmask"].to(gpu), None, c["ids"].to(gpu), c["align"].to(gpu), c["pad"].to(gpu),
                   candidates=c["cand"], latent=True)


def _solve(model, c, gpu, prepared=None, owners=None):
    """separate() without the codec, under the workspace guard: samaudio_prepare_latent + the ODE solve of each row group (model.py:
    759-768; `streams=2` models solve two groups on two engine contexts), or - `prepared` - the caller's prepare and one solve.
    `owners`: a list that receives whom the guard handed workspaces to."""
    with util.workspace_guard(model) as handed, torch.inference_mode(), torch.cuda.device(model.device):
        if prepared is None:
            cond = [c["z"], c["text"], c["tmask"], None, c["ids"], c["align"], c["pad"]]
            cond = [None if t is None else t.to(gpu) for t in cond]
            groups = min(model.streams, c["z"].size(0))
            lat = model._solve_concurrent(c["noise"].to(gpu), OPT, cond, groups, candidates=c["cand"], latent=True)
        else:
            prepared()
            lat = model.solve(c["noise"].to(gpu), OPT)
    if owners is not None:
        owners.extend(handed)
    return lat.cpu()


def _check(name, prec, lat, lat_ref):
    err = (lat - lat_ref).abs().max().item()
    print(f"{name} ({prec}): latent max-abs err {err:.3e} (|ref| <= {lat_ref.abs().max():.2f}, tol {TOL[prec]:.1e})")
    assert err < TOL[prec], f"{name} ({prec}): {err} >= {TOL[prec]}"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("text_len", [1, 8, 9, 16, 17])
def test_text_lengths_at_the_fold_slot_edges(gpu, prec, text_len):
    """8 / 16 tokens are the head slots of the folded cross-attention (bf16 / fp16: cross_attn_probs + fold; x3: the *3 kernels),
    17 the first memory on the unfolded path (cross_attn_kernel + c_wo GEMM)."""
    cfg = preset_config("tiny")
    sd = _state_dict(cfg)
    c, lat_ref = _case(cfg, sd, [6, 6], text_len)
    _check(f"T=6 Lt={text_len}", prec, _solve(_model(cfg, sd, prec, gpu), c, gpu), lat_ref)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T,text_len", [(1, 17), (4, 20), (6, 32), (25, 512)])
def test_text_longer_than_the_clip(gpu, prec, T, text_len):
    """Class CKV of the x3 modes splits the Mt = rows * Lt text rows into the scratch operand the frame rows use (rows * (T + 2) rows):
    (25, 512) is pad_mode='max_length' on a 1 s clip."""
    cfg = preset_config("tiny")
    sd = _state_dict(cfg)
    c, lat_ref = _case(cfg, sd, [T, T], text_len)
    _check(f"T={T} Lt={text_len}", prec, _solve(_model(cfg, sd, prec, gpu), c, gpu), lat_ref)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T,text_len", [(4, 20), (1, 17), (6, 8)])
def test_candidates_with_text_longer_than_the_candidates_frames(gpu, prec, T, text_len):
    """2 clips x 2 candidates: prepare computes the text projection once per clip (B * Lt rows) and repeats it sample-major
    (reference model.py:193-203); Lt > candidates * T must not spill into the repeat's destination.  (6, 8): the control."""
    cfg = preset_config("tiny")
    sd = _state_dict(cfg)
    c, lat_ref = _case(cfg, sd, [T, T], text_len, cand=2)
    _check(f"2 candidates T={T} Lt={text_len}", prec, _solve(_model(cfg, sd, prec, gpu), c, gpu), lat_ref)


@pytest.mark.parametrize("prec", PRECS)
def test_two_stream_lanes_with_text_longer_than_the_clip(gpu, prec):
    """streams=2: the second row group runs on a stream lane with a workspace of its own - which the guard covers too."""
    cfg = preset_config("tiny")
    sd = _state_dict(cfg)
    c, lat_ref = _case(cfg, sd, [4, 4, 4], 20)
    model = _model(cfg, sd, prec, gpu, streams=2)
    owners = []
    lat = _solve(model, c, gpu, owners=owners)
    assert model._lanes and any(o is model._lanes[0] for o in owners), "the lane's workspace went through the guard"
    _check("2 stream lanes, clips of 4 frames, Lt=20", prec, lat, lat_ref)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("classes", ["w2", "qkv,wo,w2"])
def test_w2_on_split_operands_without_w13(gpu, prec, classes):
    """Class W2 without W13: nothing writes w2's split operand in an epilogue, so w2 splits the F-wide SwiGLU hidden itself (into the
    F-wide scratch: with a short text the D-wide one holds rows * (T + 2) rows of 3 D, less than the M rows of 3 F)."""
    cfg = preset_config("tiny")
    sd = _state_dict(cfg)
    c, lat_ref = _case(cfg, sd, [6, 6], 4)
    _check(f"x3_classes={classes!r}, T=6 Lt=4", prec, _solve(_model(cfg, sd, prec, gpu, x3_classes=classes), c, gpu), lat_ref)


@pytest.mark.parametrize("prec", PRECS)
def test_clips_of_different_lengths_with_a_long_text(gpu, prec):
    """A 1-frame clip padded to its neighbours' 5 (audio pad mask), 40 text tokens."""
    cfg = preset_config("tiny")
    sd = _state_dict(cfg)
    c, lat_ref = _case(cfg, sd, [5, 1, 3], 40)
    _check("clips of 5 / 1 / 3 frames, Lt=40", prec, _solve(_model(cfg, sd, prec, gpu), c, gpu), lat_ref)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("text_len", [4, 12, 20])
def test_fully_masked_text_row(gpu, prec, text_len):
    """Clip 0's text mask is all False: the reference's softmax over an all -inf row is NaN (quirk Q18) - the
    clip's latent must be non-finite wherever the oracle's is, never a large finite value; clip 1 stays within its bound.  4 / 12
    tokens take the folds (8 / 16 slots), 20 the unfolded path."""
    cfg = preset_config("tiny")
    sd = _state_dict(cfg)
    _, tmask = synthetic_text_features(2, text_len, ragged=True)
    tmask[0] = False
    c, lat_ref = _case(cfg, sd, [6, 6], text_len, mask=tmask)
    bad_ref = ~torch.isfinite(lat_ref)
    assert bad_ref[0].all() and not bad_ref[1].any(), "the oracle: NaN for the masked clip only"
    lat = _solve(_model(cfg, sd, prec, gpu), c, gpu)
    finite = torch.isfinite(lat)
    print(f"fully masked text row, Lt={text_len} ({prec}): {int(finite[0].sum())} finite values in the masked clip "
          f"(largest {lat[0][finite[0]].abs().max().item() if finite[0].any() else 0.0:.3e})")
    assert not finite[bad_ref].any(), "non-finite wherever the oracle is"
    _check(f"unmasked clip beside a fully masked one, Lt={text_len}", prec, lat[1:], lat_ref[1:])


@pytest.mark.parametrize("prec", X3)
def test_split_attention_operands_beyond_the_16_bit_range(gpu, prec):
    """self_attn_x3_kernel splits Q, K, V^T into hi / lo halves: a hi half beyond the largest finite 16-bit value must be clamped (as
    split3 does) and the rest carried by lo, not turned into inf.  Entries from 6.6e4 up to what a pair of halves holds (IEEE half:
    65504 + 65504; bfloat16: far beyond) against the fp64 softmax attention."""
    B, H, T = 2, 2, 50
    Tp = (T + 63) // 64 * 64
    D = H * 128
    top = 1.3e5 if prec == "fp16x3" else 2e5
    g = torch.Generator().manual_seed(31)
    q, k, v = (torch.randn(B, H, T, 128, generator=g) for _ in range(3))
    for x in (q, v):
        pick = torch.rand(x.shape, generator=g) < 0.02
        big = (6.6e4 + (top - 6.6e4) * torch.rand(x.shape, generator=g)) * torch.sign(torch.randn(x.shape, generator=g))
        x[pick] = big[pick]
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, T - 9:] = False
    pad = lambda z: torch.nn.functional.pad(z, (0, 0, 0, Tp - T))
    qd, kd = pad(q).contiguous().to(gpu), pad(k).contiguous().to(gpu)
    vtd = pad(v).transpose(2, 3).contiguous().to(gpu)
    out = torch.full((B * T, D), float("nan"), device=gpu)
    md = mask.to(gpu).to(torch.uint8)
    hip.check(hip.lib(hip.operands_for(prec)).samaudio_op_self_attention(
        hip.ptr(qd), hip.ptr(kd), hip.ptr(vtd), hip.ptr(md), hip.ptr(out), 2, B, T, Tp, H, util.stream()))
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(128)
    s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    want = (torch.softmax(s, -1) @ v.double()).permute(0, 2, 1, 3).reshape(B * T, D)
    got = out.cpu().double()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} non-finite outputs"
    rel = ((got - want).abs().max() / want.abs().max()).item()
    print(f"self-attention on split operands with entries up to {top:.1e} ({prec}): max-abs err / max |ref| = {rel:.3e}")
    assert rel < 2e-3


@pytest.mark.parametrize("prec", X3)
def test_cwo_switched_off_after_prepare(gpu, prec):
    """A model prepared with the default classes (fold on compensated operands for Lt <= 16) and then switched to a class set without
    CWO must compute what a model built with that class set computes, bit for bit - and run no cross_attn_*3 kernel."""
    cfg = preset_config("tiny")
    sd = _state_dict(cfg)
    c, _ = _case(cfg, sd, [6, 6], 8)
    no_cwo = hip.CLS_X3_DEFAULT & ~hip.CLS["cwo"]
    fresh = _model(cfg, sd, prec, gpu, x3_classes=no_cwo)
    want = _solve(fresh, c, gpu)
    model = _model(cfg, sd, prec, gpu)
    x3_kernels = re.compile(r"cross_attn_\w*3$")

    def profiled_solve(switch):
        def prepare():
            _prepare(model, c, gpu)
            if switch:
                model.x3_classes = no_cwo
                model._set_precision_options(model._ctx)
            model.profile_begin()
        lat = _solve(model, c, gpu, prepared=prepare)
        return lat, sorted(r["name"] for r in model.profile_end() if r["launches"])

    _, names_auto = profiled_solve(False)
    assert any(x3_kernels.search(n) for n in names_auto), "the default classes fold on compensated operands"
    lat, names = profiled_solve(True)
    print(f"CWO switched off after prepare ({prec}): cross-attention kernels {[n for n in names if 'cross_attn' in n]}")
    assert not any(x3_kernels.search(n) for n in names)
    assert torch.equal(lat, want)
