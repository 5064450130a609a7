"""Seeded noise for SAMAudio.separate(seed=...): one counter-based stream per (seed, clip id, candidate), in HIP.

`torch.randn` hands a clip whatever the global generator holds when its turn comes: the draw depends on the clip's place in the
batch, the padded length, the number of candidates, everything drawn before, and on several GPUs on the rank that owns the clip.
`seeded_noise` is a function of (seed, clip id, candidate, frame, channel) alone - Philox4x32-10 keyed by the seed and counted by
(frame * channels / 4 + quad, candidate, clip id), two Box-Muller pairs per call (tests/noise_ref.py is the
statement, include/samaudio.h samaudio_op_noise the C entry point).  This build's own definition: pinned to Random123's known
answers and to the float64 statement, unpinned vs torch's randn.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import hip

SEED_LIMIT = 1 << 64      # 0 <= seed < 2^64: the Philox key
CLIP_ID_LIMIT = 1 << 63   # 0 <= clip id < 2^63: counter words 2 and 3


def check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"seed must be an int, got {type(seed).__name__}")
    if not 0 <= seed < SEED_LIMIT:
        raise ValueError(f"seed must be in [0, 2**64), got {seed}")
    return seed


def check_clip_ids(clip_ids: Sequence[int], n: Optional[int] = None, distinct: bool = False) -> list:
    """A host list of clip ids in [0, 2**63); `n`: the required length; `distinct`: no id twice (a batch's ids: two clips that share
    an id would start from the same noise)."""
    raw = list(clip_ids)
    try:
        ids = [int(v) for v in raw]
    except (TypeError, ValueError) as exc:
        raise ValueError(f"clip ids must be integers ({exc})") from exc
    if any(isinstance(v, bool) or i != v for v, i in zip(raw, ids)):
        raise ValueError("clip ids must be integers")
    if n is not None and len(ids) != n:
        raise ValueError(f"clip_ids: {len(ids)} ids for {n} clips")
    if any(not 0 <= v < CLIP_ID_LIMIT for v in ids):
        raise ValueError("clip ids must be in [0, 2**63)")
    if distinct and len(set(ids)) != len(ids):
        raise ValueError("clip ids must be distinct")
    return ids


def seeded_noise(seed: int, clip_ids: Sequence[int], candidates: int, frames: int, channels: int, device,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [len(clip_ids) * candidates, frames, channels] on `device`: row b * candidates + c is the stream of (seed, clip_ids[b],
    candidate c), the reference's sample-major candidate order.  A row's values do not depend on the other rows, on `frames` (a longer
    call extends a shorter one) or on `candidates`.  `out`: a contiguous fp32 tensor of that shape, 16-byte aligned, to fill instead.
    One call of samaudio_op_noise on the current stream (the ids travel as kernel arguments, 64 clips per launch); nothing is read
    back.  ValueError, before anything is launched, for a seed outside [0, 2**64), an id outside [0, 2**63) and shapes the kernel
    does not take."""
    seed = check_seed(seed)
    ids = check_clip_ids(clip_ids)
    candidates, frames, channels = int(candidates), int(frames), int(channels)
    if not ids or candidates < 1 or frames < 1:
        raise ValueError("seeded_noise: clips, candidates and frames must be at least 1")
    if channels < 4 or channels % 4:
        raise ValueError("seeded_noise: channels must be a positive multiple of 4")
    if frames * (channels // 4) > 1 << 32:
        raise ValueError("seeded_noise: frames * channels / 4 must not exceed 2**32")
    device = torch.device(device)
    hip.require_gpu(device, "noise.seeded_noise")
    shape = (len(ids) * candidates, frames, channels)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    elif (out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device.type != device.type
          or device.index not in (None, out.device.index) or out.data_ptr() % 16):
        raise ValueError(f"out must be a contiguous fp32 {list(shape)} tensor on {device}, aligned to 16 bytes")
    host = (C.c_int64 * len(ids))(*ids)
    with torch.cuda.device(device):
        hip.check(hip.lib().samaudio_op_noise(hip.ptr(out), len(ids), candidates, frames, channels, C.c_uint64(seed), host,
                                              hip.current_stream_ptr()))
    return out
