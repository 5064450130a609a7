"""Audio front end on the GPU: resample, mix down to mono and right-pad PCM clips with one HIP kernel per clip
(csrc/kernels.hip resample_mix_kernel, include/samaudio.h samaudio_op_resample).

`processor.resample` stays the CPU statement of the algorithm.  This module holds its filter bank in compact form - per output
phase the one run of taps whose fp32 weight is not zero - and the launches: `resample` for device tensors (what
`SAMAudio.separate(output_sampling_rate=...)` uses on its results) and `mix_into` for one clip of a batch (what
`SAMAudioProcessor(audio_transform="hip")` uses).  Nothing here reads device memory back to the host.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, NamedTuple, Tuple

import torch

from . import hip

MAX_BANK_ELEMENTS = 4 << 20     # phases x taps per phase of fp32 (16 MiB) a pair of rates may take
_PHASE_CHUNK = 1 << 16          # phases evaluated at a time: the float64 scratch stays a few MiB for any pair


class FilterBank(NamedTuple):
    o: int                      # input samples per period (orig / gcd): the kernel's `step`
    n: int                      # output samples per period (new / gcd): the kernel's `phases`
    first: torch.Tensor         # [n] int32: the smallest d whose fp32 weight is not zero
    K: int                      # the longest run of a phase
    weights: torch.Tensor       # [n, K] fp32: weights[p, t] = fp32(h(p, first[p] + t)), zeros behind a run


def _phase_runs(o: int, n: int, lw: int, rolloff: float, p0: int, p1: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Phases [p0, p1): (d of the first candidate tap [m], fp32 weights [m, 2 width + 4], taps inside the statement's range).
    h is evaluated with processor.resample's own sequence of float64 operations, on the candidates that can be non-zero only:
    |d / o - p / n| base < lw, i.e. d within width of p o / n."""
    base = min(o, n) * rolloff
    width = math.ceil(lw * o / base)
    p = torch.arange(p0, p1, dtype=torch.int64)
    start = (p * o) // n - width - 1
    d = start[:, None] + torch.arange(2 * width + 4, dtype=torch.int64)[None, :]
    inside = (d >= -width) & (d < width + o)
    t = ((-p.to(torch.float64)[:, None] / n + d.to(torch.float64) / o) * base).clamp_(-lw, lw)
    window = torch.cos(t * math.pi / lw / 2) ** 2
    t = t * math.pi
    h = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / o)
    return start, torch.where(inside, h, torch.zeros_like(h)).to(torch.float32), inside


def _runs(start: torch.Tensor, w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(column of the first non-zero weight, run length up to the last one) per row; an all-zero row is (0, 0)"""
    nz = w != 0
    cols = torch.arange(w.shape[1])
    lo = torch.where(nz, cols, w.shape[1]).amin(1)
    hi = torch.where(nz, cols, -1).amax(1)
    return torch.where(hi >= 0, lo, 0), (hi - lo + 1).clamp_(min=0)


_banks: Dict[tuple, FilterBank] = {}
_device_banks: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def filter_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> FilterBank:
    """The filter bank of `processor.resample(., orig_freq, new_freq)` in compact form; the dense [n, 2 width + o] matrix is never
    formed.  Only taps whose fp32 weight is zero are left out.  A pair whose bank would pass MAX_BANK_ELEMENTS is refused."""
    orig_freq, new_freq, lw = int(orig_freq), int(new_freq), int(lowpass_filter_width)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("sampling rates must be positive")
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    key = (o, n, lw, float(rolloff))
    if key in _banks:
        return _banks[key]
    # phase 0 alone bounds K from below: an oversized pair is refused before its phases are evaluated
    start, w, _ = _phase_runs(o, n, lw, rolloff, 0, 1)
    k0 = int(_runs(start, w)[1][0])
    if n * max(k0, 1) > MAX_BANK_ELEMENTS:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz (reduced ratio {o} -> {n}) needs a filter bank of {n} phases x "
                         f">= {k0} taps, above the limit of {MAX_BANK_ELEMENTS} weights")
    parts = []
    for p0 in range(0, n, _PHASE_CHUNK):
        start, w, _ = _phase_runs(o, n, lw, rolloff, p0, min(n, p0 + _PHASE_CHUNK))
        lo, run = _runs(start, w)
        parts.append((start + lo, lo, run, w))
    K = max(1, max(int(run.max()) for _, _, run, _ in parts))
    if n * K > MAX_BANK_ELEMENTS:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} Hz (reduced ratio {o} -> {n}) needs a filter bank of {n} phases x "
                         f"{K} taps, above the limit of {MAX_BANK_ELEMENTS} weights")
    weights = []
    for _, lo, run, w in parts:
        w = torch.nn.functional.pad(w, (0, K))                                   # room behind a run that starts late
        taken = torch.gather(w, 1, lo[:, None] + torch.arange(K)[None, :])
        weights.append(torch.where(torch.arange(K)[None, :] < run[:, None], taken, torch.zeros_like(taken)))
    bank = FilterBank(o, n, torch.cat([f for f, _, _, _ in parts]).to(torch.int32), K, torch.cat(weights))
    _banks[key] = bank
    return bank


_IDENTITY = FilterBank(1, 1, torch.zeros(1, dtype=torch.int32), 1, torch.ones(1, 1))   # same rate: convert, mix, pad


def device_bank(orig_freq: int, new_freq: int, device, lowpass_filter_width: int = 6,
                rolloff: float = 0.99) -> Tuple[FilterBank, torch.Tensor, torch.Tensor]:
    """(bank, taps [K, n] fp32 tap-major, first [n] int32) with the two tensors on `device`, uploaded once per bank and device.
    Equal rates: the one-phase, one-tap bank of weight 1."""
    if int(orig_freq) == int(new_freq):
        bank, key = _IDENTITY, ("identity",)
    else:
        bank = filter_bank(orig_freq, new_freq, lowpass_filter_width, rolloff)
        key = (bank.o, bank.n, int(lowpass_filter_width), float(rolloff))
    key += (str(device),)
    if key not in _device_banks:
        _device_banks[key] = (bank.weights.t().contiguous().to(device), bank.first.to(device))
    return (bank,) + _device_banks[key]


def resample_length(samples: int, orig_freq: int, new_freq: int) -> int:
    """ceil(n samples / o): the length `processor.resample` returns, by integer arithmetic"""
    g = math.gcd(int(orig_freq), int(new_freq))
    return -(-(int(new_freq) // g) * int(samples) // (int(orig_freq) // g))


def mix_into(out_row: torch.Tensor, pcm: torch.Tensor, channels: int, samples: int, ch_stride: int, s_stride: int,
             orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> int:
    """One launch: `pcm` (a device tensor of int16 or fp32 elements; element (c, i) at c * ch_stride + i * s_stride from its first)
    -> out_row[: length] = the mean over the channels at `new_freq`, out_row[length :] = 0.  `out_row` is a contiguous fp32 row on the
    same device and may be uninitialised.  Returns the length."""
    if pcm.dtype not in (torch.int16, torch.float32):
        raise TypeError(f"PCM must be int16 or float32, got {pcm.dtype}")
    if out_row.dtype != torch.float32 or out_row.dim() != 1 or not out_row.is_contiguous() or out_row.device != pcm.device:
        raise ValueError("out_row must be a contiguous fp32 row on the PCM's device")
    hip.require_gpu(pcm.device, "audio.mix_into")
    bank, taps, first = device_bank(orig_freq, new_freq, pcm.device, lowpass_filter_width, rolloff)
    fmt = hip.PCM_S16 if pcm.dtype == torch.int16 else hip.PCM_F32
    with torch.cuda.device(pcm.device):
        hip.check(hip.lib().samaudio_op_resample(C.c_void_p(pcm.data_ptr()), fmt, int(channels), int(samples), int(ch_stride),
                                                 int(s_stride), hip.ptr(taps), hip.ptr(first), bank.n, bank.o, bank.K,
                                                 hip.ptr(out_row), out_row.numel(), hip.current_stream_ptr()))
    return -(-bank.n * int(samples) // bank.o)


def resample(wav: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """`processor.resample` for a device tensor [..., samples]: one launch per row, fp32 on the device.  Equal rates return the
    argument.  int16 rows are read as PCM (scaled by 1 / 32768), everything else as fp32."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("sampling rates must be positive")
    if orig_freq == new_freq:
        return wav
    hip.require_gpu(wav.device, "audio.resample")
    x = wav.reshape(-1, wav.shape[-1])
    if x.dtype not in (torch.int16, torch.float32):
        x = x.float()
    samples = x.shape[-1]
    length = resample_length(samples, orig_freq, new_freq)
    out = torch.empty(x.shape[0], length, dtype=torch.float32, device=x.device)
    if samples:
        for row, dst in zip(x, out):
            mix_into(dst, row, 1, samples, 0, row.stride(0), orig_freq, new_freq, lowpass_filter_width, rolloff)
    return out.reshape(*wav.shape[:-1], length)
