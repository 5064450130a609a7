"""CPU reference implementation of the windowed separate() (sam_audio_amd/longform.py, window_blend_kernel).
The reference project has no answer to clips longer than a window, so this file states the definition, the way tests/activity_ref.py
states the sound-activity ranker: plan arithmetic in plain loops, the blend in float64, a windowed solve built from the oracle's field
(oracle.samaudio_oracle.samaudio_forward on the window rows) with the blend after every evaluation and tests/ode_ref.solve driving it,
and the stitch."""
from typing import List, Optional, Sequence

import torch

from oracle import samaudio_oracle as O
from tests import ode_ref


# ---------------------------------------------------------------------------------------------------------------- plan
def frames_of(seconds: float, sample_rate: int, hop: int) -> int:
    return int(round(seconds * sample_rate / hop))


def refuses(W: int, O_: int, max_positions: int) -> bool:
    return W < 2 or O_ < 1 or O_ > W // 2 or W > max_positions


def windows(T: int, W: int, Ov: int) -> int:
    """n = max(1, ceil((T - O) / S)), counted instead of divided: the smallest n >= 1 whose windows reach frame T"""
    S = W - Ov
    n = 1
    while (n - 1) * S + W < T:
        n += 1
    return n


def successor_table(lengths: Sequence[int], W: int, Ov: int, candidates: int = 1) -> List[int]:
    """engine row (window row g, candidate c) = g * candidates + c, window rows clip by clip; successor = the clip's next window, same
    candidate, or -1"""
    table, g = [], 0
    for T in lengths:
        n = windows(T, W, Ov)
        for w in range(n):
            for c in range(candidates):
                table.append((g + 1) * candidates + c if w < n - 1 else -1)
            g += 1
    return table


# ---------------------------------------------------------------------------------------------------------------- blend
def blend(x: torch.Tensor, next_row: Sequence[int], Ov: int) -> torch.Tensor:
    """x [rows, W, C2] -> float64: for every link r -> s and j < O both x[r, W - O + j] and x[s, j] become p + a_j (q - p),
    a_j = (j + 1) / (O + 1)"""
    out = x.to(torch.float64).clone()
    src = x.to(torch.float64)
    W = x.shape[1]
    for r, s in enumerate(next_row):
        if s < 0:
            continue
        for j in range(Ov):
            a = (j + 1) / (Ov + 1)
            p, q = src[r, W - Ov + j], src[s, j]
            v = p + a * (q - p)
            out[r, W - Ov + j] = v
            out[s, j] = v
    return out


# ---------------------------------------------------------------------------------------------------------------- rows and stitch
def window_rows(x: torch.Tensor, lengths: Sequence[int], W: int, Ov: int, fill=0) -> torch.Tensor:
    """x [B, T, ...] (padded whole clips) -> [window rows, L, ...], L = min(W, T): row (b, w) holds the frames [w S, w S + L) of clip b,
    `fill` where that leaves the padded batch"""
    S, T = W - Ov, x.shape[1]
    L = min(W, T)
    rows = []
    for b, Tb in enumerate(lengths):
        for w in range(windows(Tb, W, Ov)):
            row = torch.full((L,) + tuple(x.shape[2:]), fill, dtype=x.dtype)
            k = max(0, min(L, T - w * S))
            row[:k] = x[b, w * S: w * S + k]
            rows.append(row)
    return torch.stack(rows)


def stitch(rows: torch.Tensor, lengths: Sequence[int], W: int, Ov: int, candidates: int, T: int) -> torch.Tensor:
    """rows [window rows * candidates, L, C] -> [B * candidates, T, C]: frame t of a clip from its window min(t // S, n - 1); a padding
    frame that lies behind that window's row is zero"""
    S, L = W - Ov, rows.shape[1]
    out = torch.zeros((len(lengths) * candidates, T, rows.shape[2]), dtype=rows.dtype)
    g = 0
    for b, Tb in enumerate(lengths):
        n = windows(Tb, W, Ov)
        for c in range(candidates):
            for t in range(T):
                w = min(t // S, n - 1)
                if t - w * S < L:
                    out[b * candidates + c, t] = rows[(g + w) * candidates + c, t - w * S]
        g += n
    return out


# ---------------------------------------------------------------------------------------------------------------- the solve
def separate(sd, cfg, audios, sizes, text, text_mask, noise, W: int, Ov: int, *, anchors=None, video: Optional[torch.Tensor] = None,
             candidates: int = 1, method: str = "midpoint", grid: Optional[Sequence[float]] = None, step_size: float = 2 / 32,
             decode: bool = True):
    """oracle.samaudio_oracle.separate over windows: encode the whole clips, cut everything into window rows, solve the rows as one
    batch with the blend after every evaluation of the field, stitch, decode once.  Returns (targets, residuals, stitched latent,
    window rows); candidate 0 of every clip, as the oracle does."""
    codec = cfg.audio_codec
    z = O.dac_encode(sd, codec, audios).transpose(1, 2)
    feats = torch.cat([z, z], dim=2)
    B, T, _ = feats.shape
    lengths = [int(v) for v in sizes.tolist()]
    pad_mask = torch.arange(T)[None, :] < sizes[:, None]
    ids, align = O.anchors_to_ids(anchors, pad_mask, codec.hop_length, codec.sample_rate)
    if video is None:
        video = feats.new_zeros(B, cfg.vision_encoder.dim, T)
    clip_of = [b for b, Tb in enumerate(lengths) for _ in range(windows(Tb, W, Ov))]

    def rep(x):
        return x if candidates == 1 else x.repeat_interleave(candidates, dim=0)

    feats_r = rep(window_rows(feats, lengths, W, Ov))
    video_r = rep(window_rows(video.transpose(1, 2), lengths, W, Ov).transpose(1, 2))
    align_r = rep(window_rows(align, lengths, W, Ov, fill=1))
    pad_r = rep(window_rows(pad_mask, lengths, W, Ov, fill=False))
    text_r, tmask_r, ids_r = rep(text[clip_of]), rep(text_mask[clip_of]), rep(ids[clip_of])
    # noise: engine row (g, c) reads whole-clip noise row clip(g) * candidates + c
    per_cand = [window_rows(noise[c::candidates], lengths, W, Ov) for c in range(candidates)]
    noise_r = torch.stack(per_cand, dim=1).reshape((-1,) + tuple(per_cand[0].shape[1:]))
    table = successor_table(lengths, W, Ov, candidates)
    linked = any(s >= 0 for s in table)

    def field_fn(t, y):
        f = O.samaudio_forward(sd, cfg, y, feats_r, text_r, t.expand(y.shape[0]), video=video_r, text_mask=tmask_r,
                               anchor_ids=ids_r, anchor_alignment=align_r, pad_mask=pad_r)
        return blend(f, table, Ov).to(f.dtype) if linked else f

    g = list(grid) if grid is not None else ode_ref.step_grid(step_size)
    rows = ode_ref.solve(field_fn, noise_r, method, g)
    latent = stitch(rows, lengths, W, Ov, candidates, T)
    if not decode:
        return None, None, latent, rows
    Bc, C = latent.shape[0], latent.shape[2] // 2
    wavs = O.dac_decode(sd, codec, latent.transpose(1, 2).reshape(2 * Bc, C, T)).view(Bc, 2, -1)
    wav_sizes = (sizes * codec.hop_length).tolist()
    target = [wavs[b * candidates, 0, : wav_sizes[b]] for b in range(B)]
    residual = [wavs[b * candidates, 1, : wav_sizes[b]] for b in range(B)]
    return target, residual, latent, rows

