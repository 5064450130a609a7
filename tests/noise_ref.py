"""The statement of separate(seed=...)'s noise: what samaudio_op_noise / noise_rows_kernel are held to.

This build's own definition - torch's device randn hands out Philox offsets by launch geometry and cannot be made invariant to the
batch, torchdiffeq and the reference say nothing about the draw - written in numpy, float64 unless a dtype is asked for.

The value at (seed, clip_id, candidate, frame t, channel c) of a tensor with C channels (C % 4 == 0, Q = C / 4):
  generator  Philox4x32-10 (Random123): multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85
             key     = (seed & 0xffffffff, seed >> 32),                                  0 <= seed < 2^64
             counter = (t * Q + c // 4, candidate, clip_id & 0xffffffff, clip_id >> 32),  0 <= clip_id < 2^63
             one call yields x0..x3, which become channels 4q .. 4q + 3
  uniforms   u_a = ((x >> 8) + 1) * 2^-24 in (0, 1],  u_b = (x >> 8) * 2^-24 in [0, 1): both exact in float32
  normals    (x0, x1): r = sqrt(-2 ln u_a(x0)), th = 2 pi u_b(x1), z0 = r cos th, z1 = r sin th; (x2, x3) -> z2, z3 likewise
             |z| <= sqrt(48 ln 2) ~ 5.768; u_a = 1 gives r = 0, never an infinity
The counter is frame-major inside a (clip, candidate) stream and knows nothing of the frame count, the batch or the number of
candidates: that is what makes a value independent of padding, batch composition and sharding.
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
Z_MAX = math.sqrt(48.0 * math.log(2.0))   # u_a = 2^-24: r = sqrt(2 * 24 ln 2)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays, Random123's philox4x32 with 10 rounds"""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK32) for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    lo32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [w.astype(np.uint32) for w in c]


def _pair(xa, xb, dtype):
    f = np.dtype(dtype).type
    ua = ((xa >> np.uint32(8)).astype(dtype) + f(1)) * f(2.0 ** -24)
    ub = (xb >> np.uint32(8)).astype(dtype) * f(2.0 ** -24)
    r = np.sqrt(f(-2) * np.log(ua))
    th = f(2 * math.pi) * ub
    return r * np.cos(th), r * np.sin(th)


def stream(seed, clip_id, candidate, frames, channels, dtype=np.float64, frame0=0):
    """[frames, channels] of the (seed, clip_id, candidate) stream from frame `frame0` on, every operation in `dtype`"""
    seed, clip_id, candidate = int(seed), int(clip_id), int(candidate)
    assert 0 <= seed < 2 ** 64 and 0 <= clip_id < 2 ** 63 and 0 <= candidate < 2 ** 32
    assert channels >= 4 and channels % 4 == 0
    q = channels // 4
    assert (frame0 + frames) * q <= 2 ** 32
    w0 = np.arange(frame0 * q, (frame0 + frames) * q, dtype=np.uint64)
    x = philox4x32_10((w0, candidate, clip_id & MASK32, clip_id >> 32), (seed & MASK32, seed >> 32))
    z0, z1 = _pair(x[0], x[1], dtype)
    z2, z3 = _pair(x[2], x[3], dtype)
    return np.stack([z0, z1, z2, z3], axis=1).reshape(frames, channels)


def noise(seed, clip_ids, candidates, frames, channels, dtype=np.float64):
    """[len(clip_ids) * candidates, frames, channels]: row b * candidates + c = stream(seed, clip_ids[b], c)"""
    return np.stack([stream(seed, cid, c, frames, channels, dtype) for cid in clip_ids for c in range(candidates)])


def moments(z):
    """(mean, variance, kurtosis, max |z|) of all values, float64"""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    m = z.mean()
    d = z - m
    var = (d * d).mean()
    return m, var, (d ** 4).mean() / var ** 2, np.abs(z).max()


def corr(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def check_statistics(z, others):
    """The 5-sigma conditions on a [frames, channels] draw of n values and on its correlation with the draws `others` (name -> array
    of the same shape).  Returns the figures; raises AssertionError naming the first condition that fails."""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    mean, var, kurt, zmax = moments(z)
    fig = {"mean": mean, "var": var, "kurtosis": kurt, "max_abs": zmax,
           "lag1_channels": corr(z[:, :-1], z[:, 1:]), "lag1_frames": corr(z[:-1], z[1:])}
    for name, other in others.items():
        fig["corr_" + name] = corr(z, other)
    bound = 5 / math.sqrt(n)
    assert abs(mean) < bound, fig
    assert abs(var - 1) < 5 * math.sqrt(2 / n), fig
    assert abs(kurt - 3) < 5 * math.sqrt(24 / n), fig
    assert zmax <= Z_MAX, fig
    for key in fig:
        if key.startswith(("lag1_", "corr_")):
            assert abs(fig[key]) < bound, (key, fig)
    return fig
