"""float64 statement of the DAC-VAE convolution forms (reference codec.py:65-89; engine.hip codec_encode / codec_decode launch each
as one generalised GEMM), written with torch's own convolutions and not from the product's index arithmetic.

Tensors arrive in the engine's layout: activations channels-last [n, T, C] (the interior of a buffer with HALO zero rows on either
side, `halo_buffer`), weights [Cout, taps * Cin] with the tap outermost; a transposed convolution's weight regrouped as
tests/test_gemm_gpu.py::test_transposed_conv does it, [s * Cout, 2 * Cin] = [r][Cout] x [j][Cin] with j = 0 the previous input row
(kernel taps s + r) and j = 1 the current one (taps r).  Everything is computed in float64 from the values handed in: pass operands
rounded to a 16-bit format (`rounded`) to state what plain 16-bit operands would give.  These are helpers, not tests.
"""
import math

import torch
import torch.nn.functional as F

HALO = 40   # csrc/kernels.h HALO: zero rows in front of and behind every codec activation buffer


def halo_buffer(x: torch.Tensor) -> torch.Tensor:
    """[n, T, C] -> [n, HALO + T + HALO, C] with zero halos"""
    return F.pad(x, (0, 0, HALO, HALO))


def rounded(t: torch.Tensor, half: torch.dtype) -> torch.Tensor:
    return t.to(half).to(torch.float64)


def _ncl(x):   # channels-last [n, T, C] -> float64 [n, C, T]
    return x.to(torch.float64).transpose(1, 2)


def conv_same(x, w, taps: int, dil: int = 1):
    """'same' convolution: x [n, T, Cin], w [Cout, taps * Cin] -> float64 [n, T, Cout].  Even `taps` (the encoder's input convolution
    as the engine states it: a window of 8 rows from 3 in front) pad taps / 2 - 1 rows in front and taps / 2 behind."""
    cout, cin = w.shape[0], x.shape[2]
    w3 = w.to(torch.float64).reshape(cout, taps, cin).permute(0, 2, 1)
    xt = _ncl(x)
    if taps % 2:
        return F.conv1d(xt, w3, padding=(taps // 2) * dil, dilation=dil).transpose(1, 2)
    return F.conv1d(F.pad(xt, ((taps // 2 - 1) * dil, (taps // 2) * dil)), w3, dilation=dil).transpose(1, 2)


def conv_strided(x, w, s: int):
    """k = 2s, stride s, pad ceil(s / 2): x [n, T, Cin] (T % s == 0), w [Cout, 2s * Cin] -> float64 [n, T / s, Cout]"""
    cout, cin = w.shape[0], x.shape[2]
    w3 = w.to(torch.float64).reshape(cout, 2 * s, cin).permute(0, 2, 1)
    return F.conv1d(_ncl(x), w3, stride=s, padding=math.ceil(s / 2)).transpose(1, 2)


def transposed_weight(wg, s: int):
    """the engine's regrouped [s * Cout, 2 * Cin] -> ConvTranspose1d's [Cin, Cout, 2s]"""
    cout, cin = wg.shape[0] // s, wg.shape[1] // 2
    g = wg.to(torch.float64).reshape(s, cout, 2, cin)   # [r][Cout][j][Cin]
    return torch.cat([g[:, :, 1], g[:, :, 0]], dim=0).permute(2, 1, 0)   # taps r (j = 1), then taps s + r (j = 0)


def conv_transposed(x, wg, s: int):
    """k = 2s, stride s, pad ceil(s / 2): x [n, T, Cin], wg [s * Cout, 2 * Cin] -> float64 [n, T * s, Cout]"""
    return F.conv_transpose1d(_ncl(x), transposed_weight(wg, s), stride=s, padding=math.ceil(s / 2)).transpose(1, 2)


def snake(v, alpha):
    """x + sin^2(alpha x) / (alpha + 1e-9), alpha per channel (last axis)"""
    a = alpha.to(torch.float64)
    v = v.to(torch.float64)
    return v + torch.sin(a * v) ** 2 / (a + 1e-9)


def finish(acc, bias=None, res=None, act: str = "none", alpha=None):
    """(raw, activated): raw = acc + bias + res, activated = act(raw) with act in none | snake | tanh"""
    raw = acc
    if bias is not None:
        raw = raw + bias.to(torch.float64)
    if res is not None:
        raw = raw + res.to(torch.float64)
    if act == "snake":
        return raw, snake(raw, alpha)
    if act == "tanh":
        return raw, torch.tanh(raw)
    assert act == "none"
    return raw, raw
