"""The CPU statement of the sound-activity ranker (sam_audio_amd/activity.py, csrc/kernels.hip activity_cells_kernel /
activity_score_kernel, include/samaudio.h "sound activity").

The reference (sam_audio/ranking/sound_activity.py) encodes the waveform to a WAV file with torchcodec, parses it with pydub and runs
pydub.silence.detect_nonsilent on it.  Neither package is part of this environment.  CPython's `audioop` is, and it is what pydub
calls for every number it computes (ratecv in set_frame_rate, rms in AudioSegment.rms), so this file uses audioop.ratecv and
audioop.rms themselves and restates pydub's pure-Python control flow around them (silence.detect_silence / detect_nonsilent,
utils.ratio_to_db / db_to_float, AudioSegment.__len__ / __getitem__).  PINNED TO audioop, UNPINNED vs pydub / torchcodec: the
quantisation to int16 (step 1) is this build's definition of the reference's WAV encode.

`statement` is the literal form; `integer_form` is the numpy restatement the kernels follow (closed-form interpolation, 1 ms cells,
window sums, the threshold table); tests/test_activity_cpu.py holds the two together.
"""
import audioop
import math
from functools import lru_cache

import numpy as np

RATE = 24_000            # detect_nonsilent's SAMPLE_RATE
WIN_MS = 250             # min_sil_ms, and get_peak_rms's window
SEEK_MS = 10             # seek_step
PEAK_HOP_MS = 100        # get_peak_rms's hop
FULL_SCALE = 32768.0     # AudioSegment.max_possible_amplitude of 16-bit samples
FRAMES_PER_MS = RATE // 1000
WIN_FRAMES = WIN_MS * FRAMES_PER_MS
METRICS = ("iou", "recall", "precision")


def quantise(x) -> np.ndarray:
    """step 1: fp32 waveform -> int16, round half to even, clipped, NaN -> 0"""
    v = np.asarray(x, dtype=np.float64) * 32768.0
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def ratecv(s: np.ndarray, sr: int) -> np.ndarray:
    """step 2: audioop.ratecv itself"""
    return np.frombuffer(audioop.ratecv(s.astype("<i2").tobytes(), 2, 1, int(sr), RATE, None)[0], dtype="<i2").astype(np.int16)


def closed_form(s: np.ndarray, sr: int) -> np.ndarray:
    """step 2 in closed form: what audioop.ratecv computes, per output sample, in 64-bit integers"""
    g = math.gcd(int(sr), RATE)
    i, o, M = int(sr) // g, RATE // g, len(s)
    N = (o * (M - 1)) // i + 1
    j = np.arange(N, dtype=np.int64)
    m = -((-i * j) // o)
    d = o * m - i * j
    x = np.concatenate([s.astype(np.int64), [0]])        # x[-1] = 0
    num = 65536 * (x[m - 1] * d + x[m] * (o - d))
    q = np.where(num >= 0, num // o, -((-num) // o))      # trunc: toward zero
    return (q >> 16).astype(np.int16)


def length_ms(n_frames: int) -> int:
    """step 3: AudioSegment.__len__"""
    return round(1000 * n_frames / RATE)


def _window(y: np.ndarray, start_ms: int) -> bytes:
    """AudioSegment[start : start + 250]: frames at or beyond the end count as zero (pydub pads up to 2 ms of missing frames)"""
    w = np.zeros(WIN_FRAMES, dtype="<i2")
    part = y[FRAMES_PER_MS * start_ms: FRAMES_PER_MS * (start_ms + WIN_MS)]
    w[: len(part)] = part
    return w.tobytes()


def ratio_to_db(r: float) -> float:
    return -float("inf") if r == 0 else 20 * math.log(r, 10)


def threshold(peak: int, sil_threshold, threshold_mode: str) -> float:
    """step 7: the rms value at or below which a window is silent"""
    if threshold_mode == "rel_to_max":
        thr_db = sil_threshold + ratio_to_db(peak / FULL_SCALE)
    elif threshold_mode == "abs":
        thr_db = sil_threshold
    else:
        raise ValueError(threshold_mode)
    return 10 ** (thr_db / 20) * FULL_SCALE


def starts(L: int):
    """step 8: detect_silence's slice starts"""
    last = L - WIN_MS
    out = list(range(0, last + 1, SEEK_MS))
    if last % SEEK_MS:
        out.append(last)
    return out


def silent_ranges(silent_starts):
    """step 9: pydub.silence.detect_silence from the silent starts on"""
    if not silent_starts:
        return []
    rest = list(silent_starts)
    ranges = []
    prev = rest.pop(0)
    current = prev
    for s in rest:
        continuous = s == prev + SEEK_MS
        has_gap = s > prev + WIN_MS
        if not continuous and has_gap:
            ranges.append([current, prev + WIN_MS])
            current = s
        prev = s
    ranges.append([current, prev + WIN_MS])
    return ranges


def nonsilent_ranges(silent, L: int):
    """step 10: pydub.silence.detect_nonsilent from the silent ranges on"""
    if not silent:
        return [[0, L]]
    if silent[0][0] == 0 and silent[0][1] == L:
        return []
    prev_end = 0
    out = []
    for a, b in silent:
        out.append([prev_end, a])
        prev_end = b
    if b != L:
        out.append([prev_end, L])
    if out[0] == [0, 0]:
        out.pop(0)
    return out


def compute_iou_recall_precision(hyp_spans, ref_spans):
    """step 11: sound_activity.py:72-93, operation for operation"""
    def span_length(span):
        return span[1] - span[0]

    def intersection_length(a, b):
        return max(0, min(a[1], b[1]) - max(a[0], b[0]))

    total_hyp = sum(span_length(s) for s in hyp_spans)
    total_ref = sum(span_length(s) for s in ref_spans)
    inter = 0
    for h in hyp_spans:
        for r in ref_spans:
            inter += intersection_length(h, r)
    union = sum(span_length(s) for s in list(hyp_spans) + list(ref_spans)) - inter
    return {"iou": inter / union if union > 0 else 0,
            "recall": inter / total_ref if total_ref > 0 else 0,
            "precision": inter / total_hyp if total_hyp > 0 else 0}


def statement(x, sr: int, sil_threshold=-40, threshold_mode="rel_to_max"):
    """One mono waveform -> dict(L, peak, silent (the silent starts), ms (nonsilent spans in ms), spans (in seconds))"""
    y = ratecv(quantise(x), sr)
    L = length_ms(len(y))
    if L < WIN_MS:
        ms = [[0, L]]
        return dict(L=L, peak=0, silent=[], ms=ms, spans=[(round(a / 1000, 3), round(b / 1000, 3)) for a, b in ms])
    peak = max(audioop.rms(_window(y, i), 2) for i in range(0, L - WIN_MS + 1, PEAK_HOP_MS))
    thresh = threshold(peak, sil_threshold, threshold_mode)
    silent = [i for i in starts(L) if audioop.rms(_window(y, i), 2) <= thresh]
    ms = nonsilent_ranges(silent_ranges(silent), L)
    return dict(L=L, peak=peak, silent=silent, ms=ms, spans=[(round(a / 1000, 3), round(b / 1000, 3)) for a, b in ms])


def score(x, sr: int, ref_spans, metric="iou", sil_threshold=-40, threshold_mode="rel_to_max") -> float:
    """the float the reference puts into its score list; ref_spans: [(start_s, end_s), ...]"""
    hyp = [list(s) for s in statement(x, sr, sil_threshold, threshold_mode)["spans"]]
    return compute_iou_recall_precision(hyp, [list(r) for r in ref_spans])[metric]


def score_f32(*args, **kwargs) -> np.float32:
    """... as the float32 `torch.tensor(list_of_floats)` holds"""
    return np.float32(score(*args, **kwargs))


# ---- the integer form the kernels follow ---------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def threshold_table(sil_threshold, threshold_mode: str) -> np.ndarray:
    """T[peak] = floor(thresh(peak)) clamped to 65 535, for peak in [0, 32768]: rms <= thresh <=> S < (T + 1)^2 6000"""
    return np.array([min(int(math.floor(threshold(p, sil_threshold, threshold_mode))), 65535) for p in range(32769)], dtype=np.int32)


def cells(y: np.ndarray, L: int) -> np.ndarray:
    """int64 sum of y^2 over frames [24 c, 24 c + 24) for c < L, frames at or beyond len(y) as zero"""
    sq = np.zeros(FRAMES_PER_MS * L, dtype=np.int64)
    n = min(len(y), len(sq))
    sq[:n] = y[:n].astype(np.int64) ** 2
    return sq.reshape(L, FRAMES_PER_MS).sum(1)


def integer_form(x, sr: int, sil_threshold=-40, threshold_mode="rel_to_max"):
    """steps 1-8 as the kernels do them -> dict(L, peak, silent)"""
    y = closed_form(quantise(x), sr)
    L = length_ms(len(y))
    if L < WIN_MS:
        return dict(L=L, peak=0, silent=[])
    P = np.concatenate([[0], np.cumsum(cells(y, L))])
    S = lambda i: int(P[i + WIN_MS] - P[i])   # noqa: E731
    peak = max(math.isqrt(S(i) // WIN_FRAMES) for i in range(0, L - WIN_MS + 1, PEAK_HOP_MS))
    T = int(threshold_table(sil_threshold, threshold_mode)[peak])
    limit = (T + 1) ** 2 * WIN_FRAMES
    return dict(L=L, peak=peak, silent=[i for i in starts(L) if S(i) < limit])


# ---- the signal of the tests ------------------------------------------------------------------------------------------------------

BURSTS = ((0.30, 0.85), (1.40, 1.62), (2.20, 2.21))


def burst_signal(samples: int, sr: int, seed: int = 0, gain: float = 0.5) -> np.ndarray:
    """noise of amplitude 1e-4 plus 440 Hz bursts over BURSTS, fp32"""
    t = np.arange(samples, dtype=np.float64) / sr
    x = 1e-4 * np.random.default_rng(seed).uniform(-1.0, 1.0, samples)
    for a, b in BURSTS:
        x += np.where((t >= a) & (t < b), gain * np.sin(2 * math.pi * 440.0 * t), 0.0)
    return x.astype(np.float32)


# (id, samples, rate, the spans in seconds where they were worked out by hand) - the smallest shapes at which a kernel can go wrong
SHAPES = (
    ("3s_48k", 144_000, 48_000, [(0.3, 0.85), (1.4, 1.62), (2.2, 2.21)]),
    ("short", 9_600, 48_000, [(0.0, 0.2)]),                            # L = 200: shorter than one window
    ("one_window", 12_007, 48_000, None),                              # L = 250: exactly one window
    ("unaligned_last", 97_234, 48_000, [(0.3, 0.85), (1.4, 1.62)]),    # L = 2 026: (L - 250) % 10 != 0
    ("plus_13", 96_013, 48_000, None),                                 # N = 48 007: frames behind 24 L that no window reads
    ("rounds_up", 96_026, 48_000, None),                               # N = 48 013, L = 2 001: the last slice is zero-padded
    ("44k1", 100_000, 44_100, [(0.3, 0.85), (1.4, 1.62), (2.2, 2.268)]),   # non-integer ratio
    ("16k", 48_000, 16_000, None),                                     # upsampling
    ("24k", 72_000, 24_000, None),                                     # identity
    ("47999", 143_997, 47_999, None),                                  # odd rate: 24 000 phases
    ("tiny", 5, 48_000, [(0.0, 0.0)]),                                 # L = 0
)
TIE_ABS_DB = -80.2   # 10^(-80.2 / 20) 32768 = 3.2023...: the quiet half of `tie` is silent in "abs" mode too


@lru_cache(maxsize=None)
def case(name: str):
    """(waveform fp32, rate) of a shape of SHAPES or of a value case"""
    for n, samples, rate, _ in SHAPES:
        if n == name:
            return burst_signal(samples, rate, seed=len(n)), rate
    rate = 24_000
    if name == "zeros":
        return np.zeros(30_000, dtype=np.float32), rate
    if name == "full_scale":
        return np.full(30_011, -1.0, dtype=np.float32), rate    # -32768 everywhere: peak 32768, the table's last entry
    if name == "clipping":      # values beyond +-1 and a NaN sample inside a burst
        x = burst_signal(72_000, rate, seed=3, gain=1.7)
        x[9_000] = np.nan
        x[9_001] = np.inf
        x[9_002] = -1e30
        return x, rate
    if name == "tie":           # 1 s of alternating +-300 / 32768, then 1 s of +-3 / 32768: peak 300, T = 3, rms of the quiet half 3
        sign = np.where(np.arange(rate) % 2 == 0, 1.0, -1.0)
        return np.concatenate([sign * 300 / 32768, sign * 3 / 32768]).astype(np.float32), rate
    if name == "two_chunks":    # 21 s at 8 kHz: 2 076 regular window starts, more than the score kernel holds in LDS at a time (2 000);
        rate = 8_000            # bursts on both sides of start 2 000 (20.0 s) and silence across it
        t = np.arange(21 * rate, dtype=np.float64) / rate
        x = 1e-4 * np.random.default_rng(5).uniform(-1.0, 1.0, len(t))
        for a, b in ((0.5, 1.0), (19.2, 19.6), (20.1, 20.3), (20.62, 20.7)):
            x += np.where((t >= a) & (t < b), 0.4 * np.sin(2 * math.pi * 330.0 * t), 0.0)
        return x.astype(np.float32), rate
    raise KeyError(name)


VALUE_CASES = ("zeros", "full_scale", "clipping", "tie", "two_chunks")


@lru_cache(maxsize=None)
def expected(name: str, sil_threshold=-40, threshold_mode="rel_to_max"):
    """the statement on a case, computed once"""
    x, rate = case(name)
    return statement(x, rate, sil_threshold, threshold_mode)


def score_of(st, ref_spans, metric="iou") -> np.float32:
    """the reference's score of a `statement` result against ref_spans [(start_s, end_s), ...], as the float32 its score tensor holds"""
    return np.float32(compute_iou_recall_precision([list(s) for s in st["spans"]], [list(r) for r in ref_spans])[metric])
