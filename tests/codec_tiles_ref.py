"""The reach of the DAC-VAE and the plan of its time tiles, restated in plain Python integers from the codec's configuration (the
published DAC architecture: Conv1d / ConvTranspose1d kernel sizes, strides, paddings and dilations), not from the engine.

Indices are those of PyTorch's definitions:
  Conv1d(k, stride s, padding p, dilation d):       out[q] reads in[q s - p + j d],  j = 0 .. k - 1
  ConvTranspose1d(k, stride s, padding p):          in[i] writes out[i s - p + j],   j = 0 .. k - 1

Encoder (rates r0..r3, hop = their product):  Conv1d(k7, p3); per stage: three residual units (Conv1d(k7, dilation d, p 3d), Conv1d(k1))
with d = 1, 3, 9, then Conv1d(k = 2r, stride r, p = ceil(r / 2)); Conv1d(k3, p1); the quantizer's in_proj Conv1d(k1).
Decoder (rates in its own order): out_proj Conv1d(k1); Conv1d(k7, p3); per stage: ConvTranspose1d(k = 2r, stride r, p = ceil(r / 2))
then the three residual units; Conv1d(k7, p3) + tanh.

A range is walked backwards from one latent frame f: `lo` / `hi` are how far the rows a layer reads lie before the first / behind the
last row that belongs to frame f at that layer's rate (`per` rows per frame)."""
from typing import List, NamedTuple, Tuple

DILATIONS = (1, 3, 9)


def _conv(lo: int, hi: int, k: int, stride: int, pad: int, dil: int = 1) -> Tuple[int, int]:
    """the input rows [first * stride - pad, last * stride - pad + (k - 1) dil] of output rows [first, last], relative to a frame whose
    first row is index 0 at both rates: output rows [-lo, n - 1 + hi] with n rows per frame -> input rows [-lo', n stride - 1 + hi']"""
    return lo * stride + pad, hi * stride + (k - 1) * dil - pad - (stride - 1)


def _conv_transpose(lo: int, hi: int, n_out: int, k: int, stride: int, pad: int) -> Tuple[int, int]:
    """output row o gets in[i] for every i with 0 <= o + pad - i stride <= k - 1"""
    first, last = -lo, n_out - 1 + hi                     # output rows, the frame's first row = 0
    i_min = -((-(first + pad - (k - 1))) // stride)       # ceil((first + pad - (k - 1)) / stride)
    i_max = (last + pad) // stride                        # floor
    n_in = n_out // stride
    return -i_min, i_max - (n_in - 1)


def reach_rows(enc_rates, dec_rates, decode: bool) -> Tuple[int, int, int]:
    """(rows before, rows behind, rows per frame) at the direction's INPUT: samples for the encoder, latent frames for the decoder"""
    lo = hi = 0
    if not decode:
        lo, hi = _conv(lo, hi, 1, 1, 0)            # in_proj
        lo, hi = _conv(lo, hi, 3, 1, 1)
        for r in reversed(list(enc_rates)):
            lo, hi = _conv(lo, hi, 2 * r, r, (r + 1) // 2)
            for d in reversed(DILATIONS):
                lo, hi = _conv(lo, hi, 1, 1, 0)
                lo, hi = _conv(lo, hi, 7, 1, 3 * d, d)
        lo, hi = _conv(lo, hi, 7, 1, 3)
        per = 1
        for r in enc_rates:
            per *= r
        return lo, hi, per
    per = 1
    for r in dec_rates:
        per *= r
    lo, hi = _conv(lo, hi, 7, 1, 3)
    for r in reversed(list(dec_rates)):
        for d in reversed(DILATIONS):
            lo, hi = _conv(lo, hi, 1, 1, 0)
            lo, hi = _conv(lo, hi, 7, 1, 3 * d, d)
        lo, hi = _conv_transpose(lo, hi, per, 2 * r, r, (r + 1) // 2)
        per //= r
    lo, hi = _conv(lo, hi, 7, 1, 3)
    lo, hi = _conv(lo, hi, 1, 1, 0)                # out_proj
    assert per == 1
    return lo, hi, 1


def halo_frames(enc_rates, dec_rates, decode: bool) -> int:
    """the reach in whole latent frames, the larger side"""
    lo, hi, per = reach_rows(enc_rates, dec_rates, decode)
    return max(-(-lo // per), -(-hi // per))


class Tile(NamedTuple):
    keep0: int
    keep1: int
    seg0: int
    seg1: int


def tile_plan(T: int, L: int, h: int) -> List[Tile]:
    """tile k keeps [kL, min(T, (k + 1) L)) of a pass over [max(0, kL - h), min(T, (k + 1) L + h))"""
    assert T >= 1 and L >= 1 and h >= 0
    return [Tile(k * L, min(T, (k + 1) * L), max(0, k * L - h), min(T, (k + 1) * L + h)) for k in range(-(-T // L))]


def longest_segment(T: int, L: int, h: int) -> int:
    return max(t.seg1 - t.seg0 for t in tile_plan(T, L, h))
