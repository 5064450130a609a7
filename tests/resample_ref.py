"""float64 direct form of the resampler behind the audio front end (include/samaudio.h samaudio_op_resample),
written from the formula and not from the product's bank code (sam_audio_amd/audio.py), plus input generators and the error bound.

With g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff, width = ceil(lw o / base):
    y[j] = sum_d h(p, d) x[f o + d],  f = j // n,  p = j % n,  d in [-width, width + o),  x = 0 outside [0, samples),
           j < ceil(n samples / o)
    h(p, d) = sinc(pi t) cos^2(pi t / (2 lw)) base / o,  t = clamp((d / o - p / n) base, -lw, lw),  sinc(0) = 1
tests/test_audio_frontend_cpu.py pins it to processor.resample.  These are helpers, not tests.
"""
import math

import torch

PAIRS = [(2, 3), (3, 2), (44100, 48000), (48000, 44100), (16000, 48000), (48000, 16000), (44100, 16000)]
MORE_PAIRS = [(22050, 48000), (8000, 48000), (32000, 48000), (96000, 48000)]   # the CPU statements cover these as well
TILE_MAX = 2048     # most outputs of one workgroup (csrc/kernels.hip kResampleTileMax): 3 * TILE_MAX + 1 outputs span >= 3 tiles


def reduced(orig: int, new: int):
    g = math.gcd(orig, new)
    return orig // g, new // g


def geometry(orig: int, new: int, lw: int = 6, rolloff: float = 0.99):
    """(o, n, base, width)"""
    o, n = reduced(orig, new)
    base = min(o, n) * rolloff
    return o, n, base, math.ceil(lw * o / base)


def out_length(samples: int, orig: int, new: int) -> int:
    o, n = reduced(orig, new)
    return -(-n * samples // o)


def weights64(orig: int, new: int, lw: int = 6, rolloff: float = 0.99, phases=None) -> torch.Tensor:
    """h as float64 [n, 2 width + o] (or the rows `phases` of it): column c is d = c - width.  Equal rates: [[1.]] (width 0)."""
    if orig == new:
        return torch.ones(1, 1, dtype=torch.float64)
    o, n, base, width = geometry(orig, new, lw, rolloff)
    d = torch.arange(-width, width + o, dtype=torch.float64)[None, :]
    p = (torch.arange(n) if phases is None else phases).to(torch.float64)[:, None]
    t = ((d / o - p / n) * base).clamp(-lw, lw)
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(math.pi * t) / (math.pi * t))
    return sinc * torch.cos(math.pi * t / (2 * lw)) ** 2 * (base / o)


def bank_figures(orig: int, new: int):
    """(K, S): the longest run of fp32-non-zero weights of a phase, and max_p sum_d |h(p, d)| of the float64 weights"""
    h = weights64(orig, new)
    nz = h.float() != 0
    cols = torch.arange(h.shape[1])
    lo = torch.where(nz, cols, h.shape[1]).amin(1)
    hi = torch.where(nz, cols, -1).amax(1)
    return int((hi - lo + 1).max()), float(h.abs().sum(1).max())


def to_float64(x: torch.Tensor) -> torch.Tensor:
    """PCM as the kernel reads it: int16 scaled by 1 / 32768, floats as they are"""
    return x.double() / 32768.0 if x.dtype == torch.int16 else x.double()


def direct(x: torch.Tensor, orig: int, new: int, j0: int = 0, j1=None, lw: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """x [channels, samples] (int16 | float) -> y[j0:j1] of the mean over the channels, float64.  Only the input window those outputs
    reach is converted, so a slice of a very long clip is cheap."""
    samples = x.shape[-1]
    total = out_length(samples, orig, new)
    j1 = total if j1 is None else min(j1, total)
    if orig == new:
        return to_float64(x[:, j0:j1]).mean(0)
    o, n, _, width = geometry(orig, new, lw, rolloff)
    h = weights64(orig, new, lw, rolloff)                                  # [n, D]
    D = h.shape[1]
    f0, f1 = j0 // n, (j1 - 1) // n + 1                                      # frames [f0, f1)
    lo, hi = f0 * o - width, (f1 - 1) * o - width + D                        # input window [lo, hi)
    win = torch.zeros(hi - lo, dtype=torch.float64)
    a, b = max(lo, 0), min(hi, samples)
    if b > a:
        win[a - lo: b - lo] = to_float64(x[:, a:b]).mean(0)
    frames = win.unfold(0, D, o)                                             # [f1 - f0, D]: frames[f, c] = x[(f0 + f) o + c - width]
    y = (frames @ h.t()).reshape(-1)                                         # [(f1 - f0) n]
    return y[j0 - f0 * n: j1 - f0 * n]


def tolerance(K: int, C: int, S: float, A: float) -> float:
    """First-order bound of an fp32 dot product of K fp32-rounded weights over inputs that carry a C-term mean, against float64:
    each of the K products and K sums, the weight's rounding and the mean's C roundings cost 2^-24 relative to sum |h| |x| <= S A."""
    return 1.01 * (K + C + 2) * 2.0 ** -24 * S * A


def pcm_int16(channels: int, samples: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, (channels, samples), generator=g, dtype=torch.int16)


def pcm_float(channels: int, samples: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand(channels, samples, generator=g) * 2 - 1


def lengths(orig: int, new: int):
    """1 sample, fewer than width, a multiple of o, that plus 1, and one whose outputs span at least three workgroup tiles"""
    o, n = reduced(orig, new)
    mult = o * max(2, -(-40 // o))
    return [1, 5, mult, mult + 1, -(-(3 * TILE_MAX + 5) * o // n)]
