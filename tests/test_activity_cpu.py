"""The CPU side of the sound-activity ranker (tests/test_activity_gpu.py holds the kernels to tests/activity_ref.py on the GPU): the
closed form of the rate conversion against audioop.ratecv, the integer identities the kernels rest on, the threshold table, the
integer form against the literal statement, the config / ranker / separate() wiring, the C-ABI wiring, the argument refusals of the
real library, and the GPU tests on the SIMT simulator."""
import audioop
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sam_audio_amd import activity, hip
from sam_audio_amd.config import SAMAudioConfig, SoundActivityRankerConfig, parse_ranker_config
from sam_audio_amd.ranking import EnsembleRanker, Ranker, SoundActivityRanker, create_ranker
from tests import activity_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (48_000, 44_100, 32_000, 24_000, 16_000)
LENGTHS = (1, 2, 7, 1_000, 12_345)


@pytest.mark.parametrize("rate", RATES + (47_999,))
def test_closed_form_is_audioop_ratecv(rate):
    rng = np.random.default_rng(rate)
    for samples in LENGTHS:
        s = rng.integers(-32768, 32768, samples).astype(np.int16)
        if samples >= 7:
            s[:3] = (-32768, 32767, -32768)
        want = A.ratecv(s, rate)
        got = A.closed_form(s, rate)
        assert got.shape == want.shape and np.array_equal(got, want), (rate, samples)
        # the kernel's form of it: trunc(65536 w / o) >> 16 = floor(w / o), w in 32 bits
        g = math.gcd(rate, A.RATE)
        i, o = rate // g, A.RATE // g
        j = np.arange(len(want), dtype=np.int64)
        m = -((-i * j) // o)
        d = o * m - i * j
        x = np.concatenate([s.astype(np.int64), [0]])
        w = x[m - 1] * d + x[m] * (o - d)
        assert int(np.abs(w).max()) < 2 ** 31
        assert np.array_equal(w // o, want.astype(np.int64)), (rate, samples)
        # the lengths the library and the Python side report
        step, phases = activity.ratio(rate)
        assert (step, phases) == (i, o)
        assert hip.lib().samaudio_activity_length_ms(samples, step, phases) == A.length_ms(len(want))


def test_length_ms_is_python_round():
    lib = hip.lib()
    for frames in list(range(1, 200)) + [6_000 + k for k in range(-30, 31)] + [48_007, 48_012, 48_013, 48_036, 240_000, 10 ** 9 + 12]:
        assert lib.samaudio_activity_length_ms(frames, 1, 1) == A.length_ms(frames), frames
    assert lib.samaudio_activity_length_ms(12, 1, 1) == 0 and lib.samaudio_activity_length_ms(36, 1, 1) == 2      # ties go to even
    assert lib.samaudio_activity_length_ms(0, 1, 1) == -1 and lib.samaudio_activity_length_ms(5, 0, 1) == -1
    assert lib.samaudio_activity_length_ms(5, 1, 0) == -1 and lib.samaudio_activity_length_ms(5, 1, 7) == -1
    assert lib.samaudio_activity_workspace_bytes(3, 144_000, 2, 1) == 3 * 3_000 * 8
    assert lib.samaudio_activity_workspace_bytes(2, 5, 2, 1) == 2 * 8 and lib.samaudio_activity_workspace_bytes(0, 5, 2, 1) == -1
    for a in range(0, 100_000, 7):     # the kernel's spans in seconds: ms / 1000 in float64 is round(ms / 1000, 3)
        assert round(a / 1000, 3) == a / 1000.0


def test_rms_and_the_comparison_identity():
    rng = np.random.default_rng(0)
    for scale in (1, 50, 3_000, 32_768):
        y = rng.integers(-scale, scale, A.WIN_FRAMES).astype(np.int16) if scale < 32_768 else np.full(A.WIN_FRAMES, -32768, np.int16)
        S = int((y.astype(np.int64) ** 2).sum())
        assert math.isqrt(S // A.WIN_FRAMES) == audioop.rms(y.astype("<i2").tobytes(), 2)
    assert S < 2 ** 43
    # rms <= thresh  <=>  S < (T + 1)^2 6000 with T = floor(thresh): at both sides of the edge, for any thresh in [T, T + 1)
    for T in (0, 1, 3, 99, 327, 32_767):
        edge = (T + 1) ** 2 * A.WIN_FRAMES
        for thresh in (float(T), T + 0.5, math.nextafter(T + 1.0, 0.0)):
            assert math.isqrt((edge - 1) // A.WIN_FRAMES) <= thresh
            assert not math.isqrt(edge // A.WIN_FRAMES) <= thresh


def test_threshold_table():
    t = activity.threshold_table(-40, "rel_to_max")
    assert t.dtype == torch.int32 and t.shape == (32_769,)
    assert [int(t[p]) for p in (0, 100, 300, 32_768)] == [0, 1, 3, 327]
    assert A.threshold(300, -40, "rel_to_max") > 3.0 and A.threshold(100, -40, "rel_to_max") > 1.0     # the ties a device pow could flip
    assert np.array_equal(t.numpy(), A.threshold_table(-40, "rel_to_max"))
    assert activity.threshold_table(-40.0, "rel_to_max") is t                                       # cached
    a = activity.threshold_table(A.TIE_ABS_DB, "abs")
    assert int(a.min()) == int(a.max()) == 3 and np.array_equal(a.numpy(), A.threshold_table(A.TIE_ABS_DB, "abs"))
    assert int(activity.threshold_table(20, "abs")[0]) == 65_535                                    # clamped
    assert bool((t[1:] >= t[:-1]).all())
    with pytest.raises(ValueError):
        activity.threshold_table(-40, "relative")


@pytest.mark.parametrize("name", [s[0] for s in A.SHAPES] + list(A.VALUE_CASES))
def test_integer_form_gives_the_statements_silent_starts_and_peak(name):
    x, rate = A.case(name)
    modes = [(-40, "rel_to_max")] + ([(A.TIE_ABS_DB, "abs")] if name == "tie" else [])
    for sil, mode in modes:
        st = A.expected(name, sil, mode)
        got = A.integer_form(x, rate, sil, mode)
        assert (got["L"], got["peak"], got["silent"]) == (st["L"], st["peak"], st["silent"])
    hand = {s[0]: s[3] for s in A.SHAPES}.get(name)
    if hand is not None:
        assert A.expected(name)["spans"] == hand
    assert len(st["ms"]) <= st["L"] // 250 + 1


def test_the_statement_on_the_value_cases():
    assert A.expected("3s_48k")["peak"] == 11_585
    assert A.expected("zeros")["spans"] == [] and A.expected("zeros")["peak"] == 0
    full = A.expected("full_scale")
    assert full["spans"] == [(0.0, full["L"] / 1000)] and full["peak"] == 32_768
    tie = A.expected("tie")
    assert tie["peak"] == 300 and tie["spans"] == [(0.0, 1.0)] and 1_750 in tie["silent"]
    assert A.expected("tie", A.TIE_ABS_DB, "abs")["spans"] == [(0.0, 1.0)]
    assert A.expected("tie", -80.9, "abs")["spans"] == [(0.0, 2.0)]       # below 3: the quiet half is not silent any more
    assert A.expected("one_window")["L"] == 250 and A.expected("unaligned_last")["L"] == 2_026 and A.expected("rounds_up")["L"] == 2_001
    # overlapping reference spans count twice; no reference spans: 0
    r = A.compute_iou_recall_precision([[0.0, 1.0]], [[0.0, 0.5], [0.25, 0.75]])
    assert r["recall"] == 1.0 and r["precision"] == 1.0 and r["iou"] == 1.0
    assert A.compute_iou_recall_precision([[0.0, 1.0]], []) == {"iou": 0.0, "recall": 0, "precision": 0.0}


def test_config_round_trip_and_refusals():
    cfg = parse_ranker_config({"kind": "sound_activity"})
    assert isinstance(cfg, SoundActivityRankerConfig)
    assert (cfg.threshold_mode, cfg.sil_threshold, cfg.metric, cfg.kind) == ("rel_to_max", -40, "iou", "sound_activity")
    ranker = create_ranker(cfg)
    assert isinstance(ranker, SoundActivityRanker) and ranker.needs_spans and ranker.config is cfg
    cfg = parse_ranker_config({"kind": "sound_activity", "threshold_mode": "abs", "sil_threshold": -55.5, "metric": "recall"})
    assert (cfg.threshold_mode, cfg.sil_threshold, cfg.metric) == ("abs", -55.5, "recall")
    assert isinstance(create_ranker(cfg), SoundActivityRanker)
    for bad in ({"threshold_mode": "relative"}, {"metric": "f1"}):
        with pytest.raises(ValueError):
            parse_ranker_config(dict(bad, kind="sound_activity"))
    with pytest.raises(TypeError):
        parse_ranker_config({"kind": "sound_activity", "window": 3})
    # inside an ensemble, and through SAMAudioConfig
    const = type("Const", (Ranker,), {"forward": lambda self, **kw: torch.zeros(1, 1)})()
    ens = create_ranker({"kind": "ensemble", "rankers": {"activity": ({"kind": "sound_activity", "metric": "recall"}, 0.25),
                                                         "other": (const, 0.75)}})
    assert isinstance(ens, EnsembleRanker) and ens.weights == [0.25, 0.75] and ens.needs_spans
    assert isinstance(ens.rankers[0], SoundActivityRanker) and ens.rankers[0].config.metric == "recall" and ens.rankers[1] is const
    assert not EnsembleRanker([const], [1.0]).needs_spans
    with pytest.raises(ValueError):
        create_ranker({"kind": "ensemble", "rankers": {"a": ({"kind": "sound_activity", "metric": "f1"}, 1.0)}})
    assert isinstance(SAMAudioConfig(text_ranker={"kind": "sound_activity"}).text_ranker, SoundActivityRankerConfig)
    with pytest.raises(NotImplementedError, match="third-party"):      # CLAP / ImageBind: as before
        create_ranker({"kind": "clap"})
    import sam_audio_amd
    assert sam_audio_amd.SoundActivityRanker is SoundActivityRanker and sam_audio_amd.SoundActivityRankerConfig is SoundActivityRankerConfig


def test_attach_rankers_builds_it_from_the_model_config():
    from sam_audio_amd import preset_config
    from sam_audio_amd.model import SAMAudio
    cfg = preset_config("tiny")
    cfg.text_ranker = parse_ranker_config({"kind": "sound_activity", "metric": "precision"})
    m = SAMAudio(cfg, precision="fp32", device="cpu")
    m.attach_rankers()
    assert isinstance(m.text_ranker, SoundActivityRanker) and m.text_ranker.config.metric == "precision"


def test_rerank_hands_spans_to_rankers_that_ask_for_them():
    from sam_audio_amd import preset_config
    from sam_audio_amd.model import SAMAudio
    m = SAMAudio(preset_config("tiny"), precision="fp32", device="cpu")
    calls = []

    class Rk(Ranker):
        def __init__(self, needs):
            if needs is not None:
                self.needs_spans = needs

        def forward(self, **kw):
            calls.append(kw)
            return torch.tensor([[0.1, 0.9, 0.2], [0.5, 0.1, 0.7]])

    class B:
        audios = torch.randn(2, 1, 64)
        descriptions = ["a", "b"]
        masked_video = None
        anchors = [[("+", 0.0, 0.5)], [("-", 0.1, 0.2), ("+", 0.3, 0.4)]]

    tgt = [torch.randn(3, 64), torch.randn(3, 32)]
    sizes = torch.tensor([64, 32])
    plain = ["descriptions", "extracted_audio", "input_audio", "sample_rate"]
    for needs, keys in ((None, plain), (False, plain), (True, sorted(plain + ["spans"]))):
        m.text_ranker = Rk(needs)
        assert m._rerank(B, tgt, sizes, 3).tolist() == [1, 2]
        assert sorted(calls[-1]) == keys
    assert calls[-1]["spans"] is B.anchors and calls[-1]["sample_rate"] == 48_000
    m.text_ranker = EnsembleRanker([Rk(None), Rk(True)], [0.5, 0.5])
    assert m._rerank(B, tgt, sizes, 3).tolist() == [1, 2] and "spans" in calls[-1] and "spans" in calls[-2]
    B.anchors = None
    n = len(calls)
    with pytest.raises(ValueError, match=r"anchors=.*predict_spans=True"):
        m._rerank(B, tgt, sizes, 3)
    assert len(calls) == n
    m.text_ranker = Rk(None)
    assert m._rerank(B, tgt, sizes, 3).tolist() == [1, 2]          # a ranker that does not ask is not held to anchors


def test_header_and_python_wiring():
    header = open(os.path.join(ROOT, "include", "samaudio.h")).read()
    for name in ("samaudio_op_activity", "samaudio_activity_length_ms", "samaudio_activity_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in hip.EXPORTED_SYMBOLS
    assert "sound activity" in header and "rms(i) <= thresh  <=>  S(i) < (T + 1)^2 6000" in header   # the statement the kernels are held to
    assert "pinned to" in header and "unpinned vs pydub / torchcodec" in header
    assert hip.ACTIVITY_METRICS == {"iou": 0, "recall": 1, "precision": 2} and activity.METRICS == A.METRICS
    kernels_h = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "kernels.h")).read()
    assert re.search(r"__attribute__\(\(weak\)\)\s+hipError_t\s+launch_activity\(", kernels_h)
    kernels = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "kernels.hip")).read()
    for name in ("activity_cells_kernel", "activity_score_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % name, kernels)
    x = torch.zeros(2, 800)
    with pytest.raises(hip.SamAudioHipError, match="no CPU fallback"):
        activity.activity(x, 48_000)
    with pytest.raises(hip.SamAudioHipError, match="no CPU fallback"):
        activity.detect_nonsilent(x, 48_000)
    with pytest.raises(hip.SamAudioHipError, match="no CPU fallback"):
        SoundActivityRanker()(extracted_audio=[x], spans=[[("+", 0.0, 0.01)]], sample_rate=48_000)
    with pytest.raises(ValueError):
        activity.activity(x, 48_000, metric="f1")
    with pytest.raises(ValueError):
        activity.activity(x, 48_000, threshold_mode="relative")
    with pytest.raises(ValueError):
        activity.activity(x, 0)


def test_library_refuses_bad_activity_arguments_without_a_gpu():
    """argument validation happens before any launch, so it is checked on the real library here"""
    lib = hip.lib()
    buf = (C.c_double * 4096)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)
    odd = C.c_void_p(C.addressof(buf) + 4)
    samples, step, phases = 30_000, 2, 1                      # 48 kHz: N = 15 000, L = 625, at most 3 spans
    assert lib.samaudio_activity_length_ms(samples, step, phases) == 625
    need = lib.samaudio_activity_workspace_bytes(2, samples, step, phases)
    assert need == 2 * 625 * 8

    def call(wav=p, rows=2, row_stride=samples, samples=samples, step=step, phases=phases, table=p, ref=p, n_ref=1, metric=0,
             workspace=p, workspace_bytes=need, scores=p, spans=p, max_spans=3, count=p, peak=p):
        return lib.samaudio_op_activity(wav, rows, row_stride, samples, step, phases, table, ref, n_ref, metric, workspace,
                                        workspace_bytes, scores, spans, max_spans, count, peak, None)

    for kw in (dict(wav=null), dict(table=null), dict(workspace=null), dict(scores=null), dict(rows=0), dict(samples=0),
               dict(step=0), dict(phases=0), dict(phases=7), dict(row_stride=samples - 1), dict(metric=3), dict(metric=-1),
               dict(n_ref=-1), dict(ref=null), dict(workspace_bytes=need - 1), dict(workspace=odd), dict(max_spans=2)):
        assert call(**kw) == hip.ERR_ARG, kw
        assert b"activity" in lib.samaudio_last_error(), kw


def test_activity_kernels_on_the_simulator():
    """tests/test_activity_gpu.py on the SIMT simulator (the real kernel code compiled for the host, as tests/test_simt_cpu.py runs its
    selections): every shape and value case, the metrics, the strided view, the ranker and the ensemble.  (separate() runs on the GPU
    only.)"""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_activity_gpu.py", "-k", "not separate"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail
