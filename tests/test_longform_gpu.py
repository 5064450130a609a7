"""Windowed separate() of clips longer than one window: window_blend_kernel against the float64 blend of
tests/longform_ref.py, and SAMAudio.separate(window_seconds=, window_overlap_seconds=) against the windowed solve that file builds from
the oracle's field.  'tiny' dims, W = 16 frames, O = 4: clips of 29 and 17 frames give 3 + 2 window rows, the second clip's last window
with the minimum of O + 1 valid frames.  The tests whose docstring starts with "light" make sense on the SIMT simulator as well."""
import functools

import pytest
import torch

from sam_audio_amd import SAMAudio, SAMAudioProcessor, hip, preset_config
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
from tests import longform_ref as R
from tests import util

pytestmark = pytest.mark.gpu

W, OV = 16, 4
MIDPOINT4 = {"method": "midpoint", "options": {"step_size": 1 / 4}}


def _model(cfg, sd, prec, gpu, **kw):
    m = SAMAudio(cfg, precision=prec, device=str(gpu), **kw)
    m.load_state_dict(sd, strict=False)
    return m


def _seconds(cfg, frames):
    return frames * cfg.audio_codec.hop_length / cfg.audio_codec.sample_rate


def _windowed(model, batch, cfg, **kw):
    return model.separate(batch, window_seconds=_seconds(cfg, W), window_overlap_seconds=_seconds(cfg, OV), **kw)


def _batch(cfg, frames, anchors=None):
    """ragged clips of `frames` latent frames each (the shorter ones not a whole number of hops), ragged text"""
    hop = cfg.audio_codec.hop_length
    longest = max(frames)
    clips = [synthetic_clip(i, n * hop if n == longest else (n - 1) * hop + 100) for i, n in enumerate(frames)]
    text, tmask = synthetic_text_features(len(frames), 5, ragged=True)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * len(frames), audios=clips, anchors=anchors, text_features=text,
                                               text_mask=tmask)
    assert batch.sizes_host == list(frames)
    return batch, text, tmask


@functools.lru_cache(maxsize=None)
def _parity_case(with_video: bool):
    """inputs and the reference implementation's result, computed once per session: clips of 29 and 17 frames, text prompt plus
    anchors (one span crossing the first overlap), midpoint with 4 steps"""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=7)
    anchors = [[("+", _seconds(cfg, 10), _seconds(cfg, 20))], [("-", 0.0, _seconds(cfg, 3)), ("+", _seconds(cfg, 11), _seconds(cfg, 15))]]
    batch, text, tmask = _batch(cfg, (29, 17), anchors)
    noise = synthetic_noise(2, 29)
    video = None
    if with_video:
        g = torch.Generator().manual_seed(21)
        video = torch.nn.functional.normalize(torch.randn(2, 29, cfg.vision_encoder.dim, generator=g), dim=-1)   # [B, T, dim]
    with torch.inference_mode():
        ref = R.separate(sd, cfg, batch.audios, batch.sizes.long(), text, tmask, noise, W, OV, anchors=anchors,
                         video=None if video is None else video.transpose(1, 2), method="midpoint", step_size=1 / 4)
    return cfg, sd, anchors, text, tmask, noise, video, ref


def _attach_video(model, batch, video, gpu):
    """the visual-feature stand-in of the tiny configuration: an injected encoder that returns fixed features [B, T, dim]"""
    batch.masked_video = [torch.zeros(1, 3, 2, 2, dtype=torch.uint8) for _ in range(video.size(0))]
    model.vision_encoder = lambda videos: video.to(gpu)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("C2", [4, 256])
@pytest.mark.parametrize("overlap", [1, 4, 8])
def test_window_blend_kernel_matches_float64(gpu, overlap, C2):
    """light.  samaudio_op_window_blend on [5, 16, C2] with the table [2, -1, 4, -1, -1]: a chain of three rows 0 -> 2 -> 4 with the
    non-adjacent successors two candidates give (row 2 is blended at its head AND its tail), rows 1 and 3 without a link.

    Error bound, from the arithmetic (u = 2^-24, fp32 round to nearest): the kernel computes d = fl(q - p), a = fl((j + 1) / (O + 1))
    and v = fma(a, d, p).  |d - (q - p)| <= u |q - p|; the weight is within 2 u relative of a_j (1 u for a correctly rounded divide,
    2 u allowed for one that is not); the fused multiply-add rounds once, <= u |v|.  With 0 < a_j < 1, |q - p| <= |p| + |q| and
    |v| <= max(|p|, |q|): |v_kernel - v| <= (1 + 2 + 1) u (|p| + |q|) plus second-order terms.  A multiply followed by an add in place
    of the fma would add one more u (|p| + |q|).  The bound asserted is 6 u (|p| + |q|) per element: it covers both forms and the
    second-order terms, and was not tuned to a result."""
    rows, frames = 5, W
    table = [2, -1, 4, -1, -1]
    n = rows * frames * C2
    x = (((torch.arange(n, dtype=torch.float64) * 0.6180339887498949) % 1.0 - 0.5) * 8).to(torch.float32).view(rows, frames, C2)
    assert x.unique().numel() == n, "distinct values: a misplaced element cannot hide"
    want = R.blend(x, table, overlap)
    dev = x.to(gpu).contiguous()
    nxt = torch.tensor(table, dtype=torch.int32).to(gpu)
    hip.check(hip.lib().samaudio_op_window_blend(hip.ptr(dev), hip.ptr(nxt), rows, frames, overlap, C2, util.stream()))
    got = dev.cpu()
    touched = torch.zeros(rows, frames, dtype=torch.bool)
    bound = torch.zeros(rows, frames, C2, dtype=torch.float64)
    worst = 0.0
    for r, s in enumerate(table):
        if s < 0:
            continue
        tail, head = slice(frames - overlap, frames), slice(0, overlap)
        assert torch.equal(got[r, tail].view(torch.int32), got[s, head].view(torch.int32)), "both elements of a pair hold the same bits"
        b = 6 * 2.0 ** -24 * (x[r, tail].double().abs() + x[s, head].double().abs())
        bound[r, tail], bound[s, head] = b, b
        touched[r, tail] = touched[s, head] = True
        worst = max(worst, ((got[r, tail].double() - want[r, tail]).abs() / b).max().item())
    print(f"window_blend O={overlap} C2={C2}: worst error / bound = {worst:.3f}")
    assert ((got.double() - want).abs() <= bound).all()
    assert touched.sum().item() == 4 * overlap
    assert torch.equal(got[~touched].view(torch.int32), x[~touched].view(torch.int32)), "everything outside the overlaps is untouched"
    assert torch.equal(got[[1, 3]].view(torch.int32), x[[1, 3]].view(torch.int32)), "rows without a link are untouched"
    assert not torch.equal(got[touched], x[touched])


# ------------------------------------------------------------------------------------------------ 2. consistency of a solve
@pytest.mark.parametrize("method", ["midpoint", "rk4"])
def test_overlaps_hold_the_same_bits_after_a_solve(gpu, method):
    """light.  After a windowed separate() the tail of every window row equals the head of its successor bitwise: the rows received the
    same bits after every evaluation and the stage combinations are elementwise."""
    cfg, sd, anchors, text, tmask, noise, _, _ = _parity_case(False)
    batch, _, _ = _batch(cfg, (29, 17), anchors)
    model = _model(cfg, sd, "fp32", gpu)
    _windowed(model, batch.to(gpu), cfg, noise=noise.to(gpu), ode_opt={"method": method, "options": {"step_size": 1 / 2}})
    rows, plan = model.last_window_latent.cpu(), model.last_window_plan
    assert plan.counts == [3, 2] and plan.next_row == [1, 2, -1, 4, -1] and tuple(rows.shape) == (5, W, 256)
    S = W - OV
    for r, s in enumerate(plan.next_row):
        if s >= 0:
            assert torch.equal(rows[r, S:S + OV].view(torch.int32), rows[s, :OV].view(torch.int32)), f"link {r} -> {s} ({method})"
    assert torch.isfinite(rows).all()


# ------------------------------------------------------------------------------------------------ 3. parity
@pytest.mark.parametrize("with_video", [False, True], ids=["text+anchors", "text+anchors+video"])
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_windowed_separate_matches_the_reference_implementation(gpu, prec, with_video):
    """Latent, window rows and both waveforms of a windowed separate() within 1e-3 of tests/longform_ref.separate - the bar
    tests/test_ode_methods_gpu.py holds the unwindowed solve to, for fp32 and for fp16x3 alike."""
    cfg, sd, anchors, text, tmask, noise, video, ref = _parity_case(with_video)
    t_ref, r_ref, lat_ref, rows_ref = ref
    batch, _, _ = _batch(cfg, (29, 17), anchors)
    model = _model(cfg, sd, prec, gpu)
    if with_video:
        _attach_video(model, batch, video, gpu)
    res = _windowed(model, batch.to(gpu), cfg, noise=noise.to(gpu), ode_opt=MIDPOINT4)
    name = f"windowed separate {prec}{' video' if with_video else ''}"
    if with_video:   # the video term must matter for this case to mean anything
        assert (lat_ref - _parity_case(False)[7][2]).abs().max() > 1e-2
    assert tuple(model.last_latent.shape) == (2, 29, 256)
    util.report(f"{name} window rows", model.last_window_latent, rows_ref, 1e-3)
    util.report(f"{name} latent", model.last_latent, lat_ref, 1e-3)
    assert [t.numel() for t in res.target] == [t.numel() for t in t_ref]
    for got, want in zip(res.target + res.residual, t_ref + r_ref):
        util.report(f"{name} waveform", got, want, 1e-3)


# ------------------------------------------------------------------------------------------------ 4. one window is the plain path
def test_clips_inside_one_window_take_the_plain_path(gpu):
    """light.  Clips with T <= W, windowed: the same bits as separate() without the arguments on the same noise (one row per clip, no
    successor, no table, no blend launch)."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=7)
    batch, _, _ = _batch(cfg, (6, 5))
    batch = batch.to(gpu)
    noise = synthetic_noise(2, 6).to(gpu)
    model = _model(cfg, sd, "fp32", gpu)
    plain = model.separate(batch, noise=noise, ode_opt=MIDPOINT4)
    lat = model.last_latent.clone()
    win = _windowed(model, batch, cfg, noise=noise, ode_opt=MIDPOINT4)
    assert model.last_window_plan.counts == [1, 1] and model.last_window_plan.next_row == [-1, -1]
    assert torch.equal(model.last_latent, lat) and torch.equal(model.last_window_latent, lat)
    for a, b in zip(plain.target + plain.residual, win.target + win.residual):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. candidates
def test_candidates_are_ranked_as_whole_clips(gpu):
    """reranking_candidates = 2 with a ranker that prefers candidate 1: it is handed whole-clip candidates of the full length, the
    chosen target is candidate 1's stitched decode, the successor stride is 2, and every candidate's latent is the reference's."""
    cfg, sd, anchors, text, tmask, _, _, _ = _parity_case(False)
    batch, _, _ = _batch(cfg, (29, 17), anchors)
    hop = cfg.audio_codec.hop_length
    noise = synthetic_noise(4, 29, seed=17)
    with torch.inference_mode():
        _, _, lat_ref, _ = R.separate(sd, cfg, batch.audios, batch.sizes.long(), text, tmask, noise, W, OV, anchors=anchors,
                                      candidates=2, method="midpoint", step_size=1 / 2, decode=False)
    seen = []

    def ranker(extracted_audio, input_audio, descriptions, sample_rate, **kw):
        seen.append([tuple(w.shape) for w in extracted_audio])
        return torch.tensor([[0.0, 1.0]] * len(extracted_audio), device=extracted_audio[0].device)

    model = _model(cfg, sd, "fp32", gpu)
    model.text_ranker = ranker
    res = _windowed(model, batch.to(gpu), cfg, noise=noise.to(gpu), reranking_candidates=2,
                    ode_opt={"method": "midpoint", "options": {"step_size": 1 / 2}})
    assert seen == [[(2, 29 * hop), (2, 17 * hop)]], "whole-clip candidates of the full length"
    plan = model.last_window_plan
    assert plan.candidates == 2 and plan.rows == 10
    assert all(s == r + 2 for r, s in enumerate(plan.next_row) if s >= 0) and sum(s >= 0 for s in plan.next_row) == 6
    assert tuple(model.last_latent.shape) == (4, 29, 256)
    util.report("windowed latent, 2 candidates", model.last_latent, lat_ref, 1e-3)
    wavs = model.decode_audio(model.last_latent, pairs=True).view(4, 2, -1)
    for b, size in enumerate((29 * hop, 17 * hop)):
        assert torch.equal(res.target[b], wavs[2 * b + 1, 0, :size]) and torch.equal(res.residual[b], wavs[2 * b + 1, 1, :size])
    assert not torch.equal(wavs[0, 0], wavs[1, 0])


# ------------------------------------------------------------------------------------------------ 6. switch-off
def test_the_table_does_not_survive_the_next_prepare(gpu):
    """light.  After a windowed call a plain separate() on the same model gives the bits of a fresh model."""
    cfg, sd, anchors, text, tmask, noise, _, _ = _parity_case(False)
    batch, _, _ = _batch(cfg, (29, 17), anchors)
    batch = batch.to(gpu)
    opt = {"method": "midpoint", "options": {"step_size": 1 / 2}}
    used = _model(cfg, sd, "fp32", gpu)
    _windowed(used, batch, cfg, noise=noise.to(gpu), ode_opt=opt)
    windowed = used.last_latent.clone()
    used.separate(batch, noise=noise.to(gpu), ode_opt=opt)
    fresh = _model(cfg, sd, "fp32", gpu)
    fresh.separate(batch, noise=noise.to(gpu), ode_opt=opt)
    assert torch.equal(used.last_latent, fresh.last_latent)
    assert (windowed - fresh.last_latent).abs().max() > 1e-2, "the windows must matter for the parity tests to mean anything"
    # the C ABI itself: a table set after prepare is gone after the next prepare (a forward then equals the unwindowed one)
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, W, 128, generator=g)
    feats, txt = torch.cat([z, z], 2), torch.randn(2, 3, 768, generator=g)
    y, t = synthetic_noise(2, W), torch.tensor([0.25])
    want = fresh.forward(y, feats, txt, t)
    nxt = torch.tensor([1, -1], dtype=torch.int32).to(gpu)
    hip.check(fresh._lib.samaudio_set_windows(fresh._ctx, hip.ptr(nxt), 2, OV))
    out = torch.empty_like(want)
    hip.check(fresh._lib.samaudio_forward(fresh._ctx, hip.ptr(y.to(gpu).contiguous()), hip.ptr(t.to(gpu)), 1, hip.ptr(out), util.stream()))
    assert torch.equal(out[0, W - OV:].view(torch.int32), out[1, :OV].view(torch.int32)) and not torch.equal(out, want)
    assert torch.equal(out[0, :W - OV], want[0, :W - OV]) and torch.equal(out[1, OV:], want[1, OV:])
    util.report("blended forward", out[0, W - OV:], R.blend(want.cpu(), [1, -1], OV)[0, W - OV:].float(), 1e-5)
    assert torch.equal(fresh.forward(y, feats, txt, t), want), "forward() prepares: the table is gone"


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_at_the_c_abi(gpu):
    """light.  samaudio_set_windows: rows that are not the prepared row count, an overlap above frames / 2 or below 1, a context that
    was never prepared.  samaudio_op_window_blend: the same overlap range, channels % 4 != 0.  All before any launch."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=13, with_codec=False)
    model = _model(cfg, sd, "fp32", gpu)
    lib = model._lib
    nxt = torch.tensor([1, -1, -1], dtype=torch.int32).to(gpu)
    with pytest.raises(hip.SamAudioHipError, match="prepare first"):   # SAMAUDIO_ERR_STATE
        hip.check(lib.samaudio_set_windows(model._ctx, hip.ptr(nxt), 2, OV))
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, W, 128, generator=g)
    model._prepare(torch.cat([z, z], 2), torch.randn(2, 3, 768, generator=g), None, None, None, None, None)
    for rows, overlap, why in ((3, OV, "row count"), (1, OV, "row count"), (2, W // 2 + 1, "overlap"), (2, 0, "overlap")):
        with pytest.raises(AssertionError, match=why):   # SAMAUDIO_ERR_ARG
            hip.check(lib.samaudio_set_windows(model._ctx, hip.ptr(nxt), rows, overlap))
    hip.check(lib.samaudio_set_windows(model._ctx, hip.ptr(nxt), 2, W // 2))
    hip.check(lib.samaudio_set_windows(model._ctx, None, 0, 0))   # off
    x = torch.zeros(2, W, 8).to(gpu)
    keep = x.clone()
    for frames, overlap, channels, why in ((W, W // 2 + 1, 8, "overlap"), (W, 0, 8, "overlap"), (W, OV, 6, "channels"),
                                           (W, OV, 2, "channels"), (1, 1, 8, "frames")):
        with pytest.raises(AssertionError, match=why):
            hip.check(lib.samaudio_op_window_blend(hip.ptr(x), hip.ptr(nxt), 2, frames, overlap, channels, util.stream()))
    assert torch.equal(x, keep)


def test_one_argument_alone_is_a_value_error(gpu):
    """light.  window_seconds without window_overlap_seconds (or the reverse), and the plan's refusals through separate()."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=7)
    batch, _, _ = _batch(cfg, (6, 5))
    model = _model(cfg, sd, "fp32", gpu)
    for kw in (dict(window_seconds=1.0), dict(window_overlap_seconds=0.1),
               dict(window_seconds=_seconds(cfg, 16), window_overlap_seconds=_seconds(cfg, 9)),
               dict(window_seconds=_seconds(cfg, 16), window_overlap_seconds=0.0),
               dict(window_seconds=_seconds(cfg, 1), window_overlap_seconds=_seconds(cfg, 1)),
               dict(window_seconds=_seconds(cfg, cfg.transformer.max_positions + 1), window_overlap_seconds=1.0)):
        with pytest.raises(ValueError):
            model.separate(batch, **kw)
