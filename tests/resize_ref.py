"""float64 restatement of the frame resize of the HIP library (include/samaudio.h samaudio_op_resize_frames):
the yardstick of tests/test_vit_frames_gpu.py, itself pinned to torch's CPU kernels by tests/test_vit_frames_cpu.py.

Per axis with `inp` source pixels and `out` target pixels: scale = inp / out, support = max(scale, 1) * r (r = 2 bicubic, 1 bilinear),
inv = 1 / max(scale, 1); output i: c = scale (i + 0.5), lo = max(0, int(c - support + 0.5)), hi = min(inp, int(c + support + 0.5)),
w_j = f((j + lo - c + 0.5) inv) for j = 0 .. hi - lo - 1, normalised to sum 1; f = the triangle filter | the cubic convolution filter
with a = -0.5.  The 2-D result is the horizontal pass followed by the vertical pass.  This is what
F.interpolate(x.float(), (S, S), mode, antialias=True, align_corners=False) computes.  Nearest: source pixel
min(floor(i * (float)inp / (float)out), inp - 1), formed in fp32 as torch forms it.
"""
import functools
import math

import numpy as np
import torch

MODES = ("nearest", "bilinear", "bicubic")


def _triangle(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def axis_matrix(inp: int, out: int, mode: str) -> torch.Tensor:
    """[out, inp] float64: row i holds the normalised weights of output pixel i."""
    m = torch.zeros(out, inp, dtype=torch.float64)
    if mode == "nearest":
        scale = np.float32(inp) / np.float32(out)
        for i in range(out):
            m[i, min(int(math.floor(np.float32(i) * scale)), inp - 1)] = 1.0
        return m
    f, r = (_cubic, 2.0) if mode == "bicubic" else (_triangle, 1.0)
    scale = inp / out
    support = (scale if scale >= 1.0 else 1.0) * r
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    for i in range(out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - support + 0.5)), min(inp, int(c + support + 0.5))
        w = [f((j + lo - c + 0.5) * inv) for j in range(hi - lo)]
        total = sum(w)
        for j, v in enumerate(w):
            m[i, lo + j] = v / total
    return m


def resize64(frames_u8: torch.Tensor, size: int, mode: str) -> torch.Tensor:
    """uint8 [n, 3, H, W] -> float64 [n, 3, size, size], not rounded."""
    H, W = frames_u8.shape[-2:]
    x = frames_u8.double()
    x = x @ axis_matrix(W, size, mode).t()                            # horizontal pass
    return axis_matrix(H, size, mode) @ x                             # then the vertical pass


def levels(ref64: torch.Tensor) -> torch.Tensor:
    """round half to even, clamp to 0..255 (what the uint8 path of the transform does; bicubic overshoot ends here)"""
    return ref64.round().clamp(0, 255)


def normalise(level: torch.Tensor) -> torch.Tensor:
    """(v / 255 - 0.5) / 0.5 as the two fp32 operations the transform performs"""
    return (level.float() / 255.0 - 0.5) / 0.5


def torch_resize(frames_u8: torch.Tensor, size: int, mode: str) -> torch.Tensor:
    """torch's CPU kernel on the float copy (fp32), not rounded"""
    kw = {"antialias": True, "align_corners": False} if mode != "nearest" else {}
    return torch.nn.functional.interpolate(frames_u8.float(), size=(size, size), mode=mode, **kw)


# (H, W) -> S: down-scaling, up-scaling, one axis the identity, 31 vertical taps (more source rows than one pass through LDS holds),
# 43 horizontal taps, a single row, and a target wider than 64 columns
CASES = [((80, 64), 56), ((45, 61), 56), ((56, 131), 56), ((431, 97), 56), ((23, 600), 56), ((1, 3), 56), ((97, 131), 112)]


def random_frames(n: int, H: int, W: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8)


def checkerboard(n: int = 3, H: int = 45, W: int = 61) -> torch.Tensor:
    """0 / 255 cells 3 px high and 2 px wide: 37 % of its bicubic outputs at 56 x 56 overshoot 0..255, so the clamp is exercised"""
    y, x = torch.arange(H)[:, None], torch.arange(W)[None, :]
    board = (((y // 3 + x // 2) % 2) * 255).to(torch.uint8)
    return board.expand(n, 3, H, W).contiguous()


@functools.lru_cache(maxsize=None)
def case(H: int, W: int, S: int, mode: str, kind: str = "random"):
    """(frames u8 [3,3,H,W], float64 reference, delta): computed once, shared, never modified.  delta = max(1e-3, 2 x the largest
    |torch fp32 - reference|): how close to a half-integer a reference value has to lie for its rounding to be undecided in fp32."""
    u8 = checkerboard(3, H, W) if kind == "checkerboard" else random_frames(3, H, W, seed=H * 1000 + W)
    ref = resize64(u8, S, mode)
    dev = (torch_resize(u8, S, mode).double() - ref).abs().max().item()
    return u8, ref, max(1e-3, 2.0 * dev), dev
