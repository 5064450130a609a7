"""Sound activity on the GPU: silence detection on separated waveforms and the overlap of their nonsilent spans with reference spans
(csrc/kernels.hip activity_cells_kernel / activity_score_kernel, include/samaudio.h samaudio_op_activity).

The algorithm is the reference's `sam_audio/ranking/sound_activity.py` (pydub.silence.detect_nonsilent at 24 kHz, then
compute_iou_recall_precision); its CPU statement is tests/activity_ref.py, pinned to CPython's audioop and unpinned vs pydub /
torchcodec.  The one number of it that needs a logarithm and a power - the silence threshold as a function of the peak rms - is
evaluated here on the host, with pydub's own Python expressions, for every possible peak, and uploaded as a table.  `activity` reads
nothing back; `detect_nonsilent` does, because the spans are its result.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple, Union

import torch

from . import hip

RATE = 24_000
WINDOW_MS = 250
FULL_SCALE = 32768.0
THRESHOLD_MODES = ("abs", "rel_to_max")
METRICS = tuple(hip.ACTIVITY_METRICS)

_tables: Dict[tuple, torch.Tensor] = {}
_device_tables: Dict[tuple, torch.Tensor] = {}


def _ratio_to_db(ratio: float) -> float:
    """pydub.utils.ratio_to_db (using_amplitude=True): math.log(r, 10), not log10"""
    return -float("inf") if ratio == 0 else 20 * math.log(ratio, 10)


def threshold_table(sil_threshold=-40, threshold_mode: str = "rel_to_max") -> torch.Tensor:
    """T [32769] int32, T[peak] = min(floor(thresh(peak)), 65535): a window of rms r is silent iff r <= thresh(peak) iff r <= T[peak].
    thresh is pydub's db_to_float(silence_thresh) * max_possible_amplitude with the reference's silence_thresh: sil_threshold +
    ratio_to_db(peak / 32768) in "rel_to_max" mode, sil_threshold in "abs" mode.  Cached per (sil_threshold, threshold_mode)."""
    if threshold_mode not in THRESHOLD_MODES:
        raise ValueError(f"threshold_mode must be one of {THRESHOLD_MODES}, got {threshold_mode!r}")
    key = (float(sil_threshold), threshold_mode)
    if key not in _tables:
        values = []
        for peak in range(32769):
            thr_db = sil_threshold + _ratio_to_db(peak / FULL_SCALE) if threshold_mode == "rel_to_max" else sil_threshold
            thresh = 10 ** (thr_db / 20) * FULL_SCALE
            values.append(min(int(math.floor(thresh)), 65535) if thresh < 65536.0 else 65535)
        _tables[key] = torch.tensor(values, dtype=torch.int32)
    return _tables[key]


def device_table(sil_threshold, threshold_mode: str, device) -> torch.Tensor:
    """`threshold_table` on `device`, uploaded once per table and device"""
    key = (float(sil_threshold), threshold_mode, str(device))
    if key not in _device_tables:
        _device_tables[key] = threshold_table(sil_threshold, threshold_mode).to(device)
    return _device_tables[key]


def ratio(sample_rate: int) -> Tuple[int, int]:
    """(step, phases) = (rate / g, 24000 / g)"""
    sample_rate = int(sample_rate)
    if sample_rate <= 0:
        raise ValueError("sample_rate must be positive")
    g = math.gcd(sample_rate, RATE)
    return sample_rate // g, RATE // g


def _rows(wav: torch.Tensor) -> torch.Tensor:
    """[rows, n] fp32 whose rows are contiguous in time and do not overlap; a view is kept where it already is one"""
    if wav.dim() == 1:
        wav = wav[None]
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise ValueError(f"activity needs waveforms [rows, samples] with at least one row and one sample, got {tuple(wav.shape)}")
    if wav.dtype != torch.float32:
        wav = wav.float()
    if wav.stride(1) != 1 or (wav.shape[0] > 1 and wav.stride(0) < wav.shape[1]):
        wav = wav.contiguous()
    return wav


def _ref_tensor(ref_spans, device) -> Optional[torch.Tensor]:
    if ref_spans is None:
        return None
    if isinstance(ref_spans, torch.Tensor):
        if ref_spans.dtype != torch.float64 or ref_spans.dim() != 2 or ref_spans.shape[1] != 2 or not ref_spans.is_contiguous():
            raise ValueError("ref_spans as a tensor must be contiguous float64 [n_ref, 2]")
        return ref_spans if ref_spans.device == device else ref_spans.to(device)
    spans = [[float(a), float(b)] for a, b in ref_spans]
    return torch.tensor(spans, dtype=torch.float64).reshape(len(spans), 2).to(device)


def activity(wav: torch.Tensor, sample_rate: int, ref_spans=None, metric: str = "iou", sil_threshold=-40,
             threshold_mode: str = "rel_to_max", return_spans: bool = False, out: Optional[torch.Tensor] = None
             ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]:
    """Scores [rows] fp32 on the device: `metric` ("iou" | "recall" | "precision") of every row's nonsilent spans against `ref_spans`
    ([(start_s, end_s), ...] or a float64 device tensor [n_ref, 2]; None or empty: zeros).  `wav` is a device tensor [rows, n] (or
    [n]); a strided view whose rows are contiguous in time is read in place.  Every row is one mono clip at `sample_rate`.
    `return_spans`: also (spans [rows, max_spans, 2] int32 ms, span_count [rows] int32, peak [rows] int32), all on the device; only the
    first span_count[r] spans of row r are written.  `out`: a contiguous fp32 [rows] tensor to write the scores into.
    Two launches, nothing is read back."""
    if metric not in hip.ACTIVITY_METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    threshold_table(sil_threshold, threshold_mode)     # (refuses an unknown mode on any device)
    step, phases = ratio(sample_rate)
    hip.require_gpu(wav.device, "activity.activity")
    x = _rows(wav)
    rows, samples = x.shape
    device = x.device
    table = device_table(sil_threshold, threshold_mode, device)
    ref = _ref_tensor(ref_spans, device)
    n_ref = 0 if ref is None else int(ref.shape[0])
    lib = hip.lib()
    L = int(lib.samaudio_activity_length_ms(samples, step, phases))
    need = int(lib.samaudio_activity_workspace_bytes(rows, samples, step, phases))
    if L < 0 or need < 0:
        raise ValueError(f"activity: {samples} samples at {sample_rate} Hz are refused by the library")
    workspace = torch.empty(need // 8, dtype=torch.int64, device=device)
    scores = out if out is not None else torch.empty(rows, dtype=torch.float32, device=device)
    if scores.dtype != torch.float32 or tuple(scores.shape) != (rows,) or not scores.is_contiguous() or scores.device != device:
        raise ValueError("out must be a contiguous fp32 [rows] tensor on the waveforms' device")
    spans = count = peak = None
    max_spans = 0
    if return_spans:
        max_spans = L // WINDOW_MS + 1
        spans = torch.zeros(rows, max_spans, 2, dtype=torch.int32, device=device)
        count = torch.empty(rows, dtype=torch.int32, device=device)
        peak = torch.empty(rows, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        hip.check(lib.samaudio_op_activity(C.c_void_p(x.data_ptr()), rows, x.stride(0) if rows > 1 else samples, samples, step, phases,
                                           hip.ptr(table), hip.ptr(ref) if n_ref else C.c_void_p(0), n_ref,
                                           hip.ACTIVITY_METRICS[metric], hip.ptr(workspace), need, hip.ptr(scores), hip.ptr(spans),
                                           max_spans, hip.ptr(count), hip.ptr(peak), hip.current_stream_ptr()))
    return (scores, spans, count, peak) if return_spans else scores


def detect_nonsilent(wav: torch.Tensor, sample_rate: int, sil_threshold=-40,
                     threshold_mode: str = "rel_to_max") -> List[List[Tuple[float, float]]]:
    """The reference's `detect_nonsilent((wav, sample_rate))` for every row: [(start_s, end_s), ...] per row, rounded to ms as
    there.  Reads the spans back from the device - they are the result."""
    _, spans, count, _ = activity(wav, sample_rate, None, "iou", sil_threshold, threshold_mode, return_spans=True)
    spans, count = spans.cpu().tolist(), count.cpu().tolist()
    return [[(round(a / 1000, 3), round(b / 1000, 3)) for a, b in row[:n]] for row, n in zip(spans, count)]
