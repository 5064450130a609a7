"""The sound-activity kernels (sam_audio_amd/csrc/kernels.hip activity_cells_kernel / activity_score_kernel; include/samaudio.h
samaudio_op_activity; sam_audio_amd/activity.py; ranking.SoundActivityRanker) against the CPU statement of
tests/activity_ref.py (pinned to CPython's audioop, unpinned vs pydub / torchcodec; tests/test_activity_cpu.py holds its parts
together).

Every comparison is exact: spans, span counts and peaks are equal as integers - behind the quantisation to int16 the kernels do integer
arithmetic only - and the scores are the statement's float32, bit for bit (SCORE_ULPS = 0: the issue allowed one float32 ulp, the
float64 sums, the division and the rounding to float32 came out bit-equal on every case on the MI355X and on the simulator, so the
bound was tightened to equality).  A span edge wrong by one 10 ms step would move a 3 s clip's IoU by more than 1e-3.
"""

import numpy as np
import pytest
import torch

from sam_audio_amd import activity, hip
from sam_audio_amd.config import SoundActivityRankerConfig
from sam_audio_amd.ranking import EnsembleRanker, Ranker, SoundActivityRanker
from tests import activity_ref as A

pytestmark = pytest.mark.gpu
SCORE_ULPS = 0
REF = [(0.25, 0.9), (1.0, 1.5)]                       # one span over the first burst, one that cuts the second
OVERLAPPING = [(0.2, 1.0), (0.5, 1.5), (2.9, 7.0)]    # two that overlap each other, one that leaves the clip


def _ulps(a, b) -> int:
    """distance of two float32 values in units of the last place (both finite and of one sign here)"""
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def _run(gpu, x, rate, ref=None, metric="iou", sil=-40, mode="rel_to_max"):
    """one row -> (score as np.float32, [[start_ms, end_ms], ...], peak)"""
    wav = torch.from_numpy(np.ascontiguousarray(x))[None].to(gpu)
    score, spans, count, peak = activity.activity(wav, rate, ref, metric, sil, mode, return_spans=True)
    assert score.shape == (1,) and score.dtype == torch.float32 and score.device.type == gpu.type
    assert spans.dtype == count.dtype == peak.dtype == torch.int32 and spans.shape[0] == 1 and spans.shape[2] == 2
    n = int(count[0])
    assert 0 <= n <= spans.shape[1]
    return np.float32(score.cpu().numpy()[0]), spans[0, :n].cpu().tolist(), int(peak[0])


def _check(gpu, name, ref=None, metric="iou", sil=-40, mode="rel_to_max"):
    x, rate = A.case(name)
    st = A.expected(name, sil, mode)
    score, spans, peak = _run(gpu, x, rate, ref, metric, sil, mode)
    what = f"{name} ({len(x)} samples at {rate} Hz, L = {st['L']}) {metric} {mode} {sil}"
    want = A.score_of(st, ref or [], metric)
    print(f"{what}: peak {peak} / {st['peak']}, spans {spans}, score {score!r} / {want!r}, {_ulps(score, want)} ulp")
    assert spans == st["ms"], what
    assert peak == st["peak"], what
    assert _ulps(score, want) <= SCORE_ULPS, what
    return score, spans


@pytest.mark.parametrize("name", [s[0] for s in A.SHAPES])
def test_shapes_against_the_statement(gpu, name):
    """every length class and rate ratio x the three metrics; detect_nonsilent returns the statement's spans in seconds"""
    for metric in A.METRICS:
        _check(gpu, name, REF, metric)
    x, rate = A.case(name)
    got = activity.detect_nonsilent(torch.from_numpy(x).to(gpu), rate)
    assert got == [A.expected(name)["spans"]]
    hand = {s[0]: s[3] for s in A.SHAPES}[name]
    if hand is not None:
        assert got == [hand]


def test_value_cases(gpu):
    score, spans = _check(gpu, "zeros", REF)
    assert spans == [] and score == 0
    _, spans = _check(gpu, "full_scale", REF, "recall")
    assert spans == [[0, A.expected("full_scale")["L"]]]
    _check(gpu, "clipping", REF, "precision")                     # values beyond +-1, an infinity and a NaN sample


def test_a_clip_longer_than_one_chunk_of_window_starts(gpu):
    """21 s: the score kernel passes the window starts through LDS 2 000 at a time; activity on both sides of the seam"""
    st = A.expected("two_chunks")
    assert (st["L"] - 250) // 10 + 1 > 2_000 and st["spans"] == [(0.5, 1.0), (19.2, 19.6), (20.1, 20.3), (20.62, 20.7)]
    for metric in A.METRICS:
        _check(gpu, "two_chunks", [(0.4, 1.2), (19.0, 20.2)], metric)


def test_the_table_tie(gpu):
    """peak 300 -> T = 3, and the quiet half has rms 3: silent only because 3 <= 3.0000000000000013, which the host's table carries"""
    _, spans = _check(gpu, "tie", [(0.0, 1.25)])
    assert spans == [[0, 1000]]
    _, spans = _check(gpu, "tie", [(0.0, 1.25)], "recall", A.TIE_ABS_DB, "abs")
    assert spans == [[0, 1000]]
    _, spans = _check(gpu, "tie", [(0.0, 1.25)], "iou", -80.9, "abs")    # a threshold below 3: nothing is silent
    assert spans == [[0, 2000]]


@pytest.mark.parametrize("metric", A.METRICS)
def test_reference_spans(gpu, metric):
    """overlapping reference spans count twice, as in the reference; none at all: spans only, score 0"""
    score, _ = _check(gpu, "3s_48k", OVERLAPPING, metric)
    assert score > 0
    for none in (None, []):
        score, spans = _check(gpu, "3s_48k", none, metric)
        assert score == 0 and spans == A.expected("3s_48k")["ms"]
    _check(gpu, "3s_48k", [(5.0, 6.0)], metric)                    # no overlap
    _check(gpu, "zeros", OVERLAPPING, metric)                      # no hypothesis spans
    _check(gpu, "44k1", [(0.3, 0.85), (1.4, 1.62), (2.2, 2.268)], metric)   # the statement's own spans: 1


def test_candidates_as_a_strided_view(gpu):
    """3 rows narrowed out of a padded [2, 3, n + 777] tensor with NaN behind n: equal to contiguous rows, independent of `rows` and
    of the other rows' content, and two runs are bitwise equal"""
    x, rate = A.case("unaligned_last")
    n = len(x)
    rows = np.stack([x, np.roll(x, 20_000), 0.25 * x[::-1]])
    padded = torch.full((2, 3, n + 777), float("nan"))
    padded[1, :, :n] = torch.from_numpy(rows)
    view = padded.to(gpu)[1, :, :n]
    assert view.stride() == (n + 777, 1) and not view.is_contiguous()
    got = activity.activity(view, rate, REF, "iou", return_spans=True)
    again = activity.activity(view, rate, REF, "iou", return_spans=True)
    contiguous = activity.activity(view.contiguous(), rate, REF, "iou", return_spans=True)
    for a, b, c in zip(got, again, contiguous):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert int(got[2].min()) >= 1
    for r in range(3):
        st = A.statement(rows[r], rate)
        assert got[1][r, : int(got[2][r])].cpu().tolist() == st["ms"] and int(got[3][r]) == st["peak"]
        assert _ulps(got[0][r].cpu().numpy(), A.score_of(st, REF)) <= SCORE_ULPS
        alone = activity.activity(view[r], rate, REF, "iou", return_spans=True)          # one row, [n]
        other = view[r: r + 1].clone() if r else torch.cat([view[:1], torch.zeros_like(view[:1])])
        beside = activity.activity(other, rate, REF, "iou", return_spans=True)            # other rows, other `rows`
        for a, b, c in zip(got, alone, beside):
            assert torch.equal(a[r], b[0]) and torch.equal(a[r], c[0])
    into = torch.full((3,), float("nan"), device=gpu)
    assert activity.activity(view, rate, REF, "iou", out=into) is into and torch.equal(into, got[0])


def _ragged_candidates(gpu):
    """2 ragged clips x 3 candidates, each clip's candidates the rows of one padded tensor as separate() hands them over"""
    (a, rate), (b, _) = A.case("3s_48k"), A.case("unaligned_last")
    clips = [np.stack([a, np.roll(a, 30_000), 0.5 * np.roll(a, -10_000)]), np.stack([np.roll(b, 7_000), b, np.zeros_like(b)])]
    longest = max(c.shape[1] for c in clips)
    padded = torch.zeros(2, 3, longest)
    for i, c in enumerate(clips):
        padded[i, :, : c.shape[1]] = torch.from_numpy(c)
    dev = padded.to(gpu)
    anchors = [[("+", 0.3, 0.85), ("-", 1.3, 1.7)], [("+", 0.2, 0.9)]]
    return clips, [dev[i, :, : c.shape[1]] for i, c in enumerate(clips)], anchors, rate


def _want_scores(clips, anchors, rate, metric):
    return torch.tensor([[float(A.score(c, rate, [(s, e) for _, s, e in spans], metric)) for c in cands]
                         for cands, spans in zip(clips, anchors)])


@pytest.mark.parametrize("metric", ["iou", "precision"])
def test_ranker_forward(gpu, metric):
    """[B, candidates] on the device; the reference spans are (start, end) of EVERY anchor of the clip, whatever its token"""
    clips, wavs, anchors, rate = _ragged_candidates(gpu)
    ranker = SoundActivityRanker(SoundActivityRankerConfig(metric=metric))
    got = ranker(extracted_audio=wavs, spans=anchors, sample_rate=rate, descriptions=["a", "b"], input_audio=wavs)
    assert got.shape == (2, 3) and got.dtype == torch.float32 and got.device.type == gpu.type
    want = _want_scores(clips, anchors, rate, metric)
    print(got.cpu(), want)
    assert torch.equal(got.cpu(), want)
    assert len(set(want[0].tolist())) == 3 and float(want[1, 2]) == 0.0                  # the candidates do differ
    empty = ranker(extracted_audio=wavs, spans=[[], anchors[1]], sample_rate=rate)       # a clip without anchors scores 0
    assert torch.equal(empty.cpu()[0], torch.zeros(3)) and torch.equal(empty.cpu()[1], want[1])
    with pytest.raises(ValueError):
        ranker(extracted_audio=wavs, spans=anchors[:1], sample_rate=rate)


def test_ensemble_with_a_constant_ranker(gpu):
    clips, wavs, anchors, rate = _ragged_candidates(gpu)
    const = torch.tensor([[0.0, 0.5, 1.0], [1.0, 0.0, 0.25]])

    class Const(Ranker):
        def forward(self, **kw):
            assert "spans" in kw
            return const.to(gpu)

    ens = EnsembleRanker([SoundActivityRanker(), Const()], [0.75, 0.25])
    assert ens.needs_spans
    got = ens(extracted_audio=wavs, spans=anchors, sample_rate=rate)
    want = 0.75 * _want_scores(clips, anchors, rate, "iou") + 0.25 * const
    assert torch.equal(got.cpu(), want)


def test_error_returns_reach_python(gpu):
    x = torch.from_numpy(A.case("short")[0]).to(gpu)
    with pytest.raises(ValueError):
        activity.activity(x, 48_000, metric="f1")
    with pytest.raises(ValueError):
        activity.activity(x, 48_000, out=torch.empty(2, device=gpu))
    with pytest.raises(ValueError):
        activity.activity(x[:0], 48_000)
    table = activity.device_table(-40, "rel_to_max", gpu)
    assert activity.device_table(-40, "rel_to_max", gpu) is table and table.dtype == torch.int32 and table.numel() == 32_769
    work, out = torch.empty(200, dtype=torch.int64, device=gpu), torch.empty(1, device=gpu)
    rc = hip.lib().samaudio_op_activity(hip.ptr(x), 1, x.numel(), x.numel(), 2, 1, hip.ptr(table), None, 0, 5, hip.ptr(work), 1600,
                                        hip.ptr(out), None, 0, None, None, hip.current_stream_ptr())
    assert rc == hip.ERR_ARG and b"activity" in hip.lib().samaudio_last_error()


def _separate_setup(gpu, frames=(30, 22)):
    from sam_audio_amd import SAMAudio, SAMAudioProcessor, preset_config
    from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
    cfg = preset_config("tiny")
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, f * hop) for i, f in enumerate(frames)]
    text, tmask = synthetic_text_features(2, 3)
    proc = SAMAudioProcessor.from_config(cfg)
    model = SAMAudio(cfg, precision="fp32", device=str(gpu))
    model.load_state_dict(init_state_dict(cfg, seed=3))
    noise = synthetic_noise(6, max(frames)).to(gpu)

    def batch(anchors=None):
        return proc(descriptions=["a", "b"], audios=clips, text_features=text, text_mask=tmask, anchors=anchors).to(gpu)

    return cfg, model, batch, noise


def _spy(model, ranker, seen):
    def spy(**kw):
        seen.update(kw, scores=ranker(**kw))
        return seen["scores"]

    spy.needs_spans = True
    model.text_ranker = spy


def _check_pick(model, res, seen, anchors, rate, cfg_ranker):
    """the returned target is the candidate the statement picks from the decoded waveforms"""
    cands = [w.cpu().numpy() for w in seen["extracted_audio"]]
    want = torch.tensor([[float(A.score(c, rate, [(s, e) for _, s, e in spans], cfg_ranker.metric, cfg_ranker.sil_threshold,
                                        cfg_ranker.threshold_mode)) for c in clip] for clip, spans in zip(cands, anchors)])
    print("scores", seen["scores"].cpu().tolist(), "statement", want.tolist())
    assert seen["spans"] == anchors and seen["scores"].shape == (2, 3)
    assert torch.equal(seen["scores"].cpu(), want)
    picks = want.argmax(dim=1).tolist()
    for b, pick in enumerate(picks):
        assert torch.equal(res.target[b], seen["extracted_audio"][b][pick])
    return picks


def test_separate_picks_the_statements_candidate(gpu):
    """separate(reranking_candidates=3) on the tiny preset with anchors and the ranker attached; then the same through
    predict_spans=True with a tiny PE-A-Frame span predictor, whose spans reach the ranker as batch.anchors"""
    cfg, model, batch, noise = _separate_setup(gpu)
    rate = cfg.audio_codec.sample_rate
    # An untrained model decodes every candidate to stationary noise whose 250 ms windows stay within 1.2 dB of each other, at an rms of
    # 1 600 - 1 830 (of 32 768) from unit noise; a candidate drawn from 4 x the noise comes out at 5 850 - 6 850, one from 0.25 x at
    # about 1 300.  An absolute threshold of -21 dB (rms 2 920) lies 4 dB above the quiet candidates and 6 dB below the loud one: only
    # the loud candidate of a clip has nonsilent spans, and it is candidate 2 of clip 0 and candidate 1 of clip 1.
    noise = noise * torch.tensor([0.25, 1.0, 4.0, 1.0, 4.0, 0.25], device=noise.device).view(6, 1, 1)
    rc = SoundActivityRankerConfig(threshold_mode="abs", sil_threshold=-21, metric="iou")
    anchors = [[("+", 0.1, 0.6)], [("+", 0.0, 0.3), ("-", 0.5, 0.8)]]
    seen = {}
    _spy(model, SoundActivityRanker(rc), seen)
    res = model.separate(batch(anchors), noise=noise, reranking_candidates=3)
    assert _check_pick(model, res, seen, anchors, rate, rc) == [2, 1]
    # without anchors the ranker cannot score: said before anything is ranked
    with pytest.raises(ValueError, match="predict_spans=True"):
        model.separate(batch(), noise=noise, reranking_candidates=3)
    # predict_spans=True: the tiny span predictor of tests/test_zz_next_rows_gpu.py, from its public helpers
    import transformers
    from oracle import gen_golden_judge as G
    from sam_audio_amd.config import PEAudioFrameConfig
    from sam_audio_amd.judge import PEAudioFrame
    from sam_audio_amd.synthetic import init_frame_state_dict
    fcfg = PEAudioFrameConfig(audio=G.TINY_TC, text_model=dict(G.TINY_TEXT, hidden_size=64), codebook_dim=128)
    torch.manual_seed(1)
    tm = transformers.ModernBertModel(transformers.ModernBertConfig(**fcfg.text_model)).eval()
    predictor = PEAudioFrame(fcfg, precision="fp32", device=str(gpu), text_model=tm)
    predictor.load_state_dict(init_frame_state_dict(fcfg, seed=2), strict=False)
    pooled = torch.randn(2, fcfg.text_hidden, generator=torch.Generator().manual_seed(6)).to(gpu)
    model.span_predictor = predictor
    model.span_predictor_transform = lambda text: {"text_pooled": pooled}
    seen.clear()
    b = batch()
    res = model.separate(b, noise=noise, reranking_candidates=3, predict_spans=True)
    assert b.anchors is not None and len(b.anchors) == 2 and all(tok == "+" for clip in b.anchors for tok, _, _ in clip)
    _check_pick(model, res, seen, b.anchors, rate, rc)
