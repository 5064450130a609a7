"""Window plan of a windowed separate(): pure integer arithmetic on the host, plus the index tensors that
gather whole-clip tensors into window rows and stitch the window rows back.  No arithmetic on values happens here.

A clip of T valid frames is cut into n = max(1, ceil((T - O) / S)) windows of W frames with stride S = W - O; window w covers the
frames [w S, w S + W).  Every window but the last is full; the last holds T - (n - 1) S valid frames (more than O, at most W) and is
padded under the row's pad mask.  With O <= W // 2 a frame lies in at most two windows.

Engine rows are laid out as `window_row * candidates + c` (samaudio_prepare_latent repeats each conditioning item for its candidates),
window rows clip by clip in window order; the successor of a row is therefore `row + candidates`, or -1 for a clip's last window."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Sequence, Tuple


def seconds_to_frames(seconds: float, sample_rate: int, hop: int) -> int:
    return int(round(seconds * sample_rate / hop))


def check_window(window: int, overlap: int, max_positions: int) -> None:
    """ValueError for a window / overlap pair (in frames) the windowed solve refuses."""
    if window < 2:
        raise ValueError(f"window of {window} frames: a window needs at least 2 frames")
    if overlap < 1:
        raise ValueError(f"window overlap of {overlap} frames: neighbouring windows must share at least 1 frame")
    if overlap > window // 2:
        raise ValueError(f"window overlap of {overlap} frames exceeds half the window ({window} frames): a frame may lie in at most "
                         "two windows")
    if window > max_positions:
        raise ValueError(f"window of {window} frames: the transformer has {max_positions} RoPE positions")


def window_count(frames: int, window: int, overlap: int) -> int:
    """n = max(1, ceil((T - O) / S))"""
    stride = window - overlap
    return max(1, -(-(frames - overlap) // stride))


@dataclass
class WindowPlan:
    window: int                 # W
    overlap: int                # O
    candidates: int
    lengths: List[int]          # T of every clip (valid frames)
    batch_frames: int           # frames of the padded whole-clip tensors (>= max(lengths))
    counts: List[int] = field(default_factory=list)     # n of every clip
    first: List[int] = field(default_factory=list)      # window row of every clip's window 0
    next_row: List[int] = field(default_factory=list)   # successor table over the engine rows

    @property
    def stride(self) -> int:
        return self.window - self.overlap

    @property
    def row_frames(self) -> int:
        """frames of a window row: W, or the batch length when every clip fits one window (the rows are then the plain path's)"""
        return min(self.window, self.batch_frames)

    @property
    def window_rows(self) -> int:
        return sum(self.counts)

    @property
    def rows(self) -> int:
        return self.window_rows * self.candidates

    def valid_frames(self, clip: int, w: int) -> int:
        return min(self.window, self.lengths[clip] - w * self.stride)

    def source(self, clip: int, t: int) -> Tuple[int, int]:
        """(window, offset inside it) a stitched frame t of `clip` is read from: window min(t // S, n - 1)"""
        w = min(t // self.stride, self.counts[clip] - 1)
        return w, t - w * self.stride

    # ---------------------------------------------------------------- step control per clip
    def groups(self) -> List[Tuple[int, int, int]]:
        """Per (clip, candidate), in the stitched latent's row order: (first engine row, window count, row stride) of its window
        rows - the rows (first[b] + w) * candidates + c, w < n_b - which an adaptive solve steps as one integration."""
        return [((self.first[b]) * self.candidates + c, n, self.candidates)
                for b, n in enumerate(self.counts) for c in range(self.candidates)]

    def owner_mask(self) -> List[List[bool]]:
        """Per engine row and frame of the row: whether the row OWNS the frame - the frame is valid and lies before the stride, or
        the row is its clip's last window.  That is `source`'s rule, so the owned frames are the ones the stitch reads, and every
        valid frame of a clip is owned by exactly one row: a norm over owned frames counts each frame of the clip once."""
        L, S = self.row_frames, self.stride
        mask = []
        for b, n in enumerate(self.counts):
            for w in range(n):
                valid = self.valid_frames(b, w)
                row = [j < valid and (j < S or w == n - 1) for j in range(L)]
                mask.extend(list(row) for _ in range(self.candidates))
        return mask

    # ---------------------------------------------------------------- index tensors (host lists; the model uploads them once)
    def gather_index(self) -> Tuple[List[int], List[List[int]], List[List[bool]]]:
        """Per window row: the clip it belongs to, the whole-clip frame of each of its `row_frames` frames (clamped into the batch) and
        whether that frame exists in the padded batch (frames past `batch_frames` are filled, not read)."""
        clip_of, frame_of, inside = [], [], []
        L, T = self.row_frames, self.batch_frames
        for b, n in enumerate(self.counts):
            for w in range(n):
                t0 = w * self.stride
                clip_of.append(b)
                frame_of.append([min(t0 + j, T - 1) for j in range(L)])
                inside.append([t0 + j < T for j in range(L)])
        return clip_of, frame_of, inside

    def stitch_index(self) -> Tuple[List[List[int]], List[List[int]], List[List[bool]]]:
        """Per whole-clip output row (clip * candidates + c) and frame t: the engine row and the frame inside it that hold the frame,
        and whether there is one (a padding frame past the last window's row has none and is zero in the stitched latent)."""
        rows, offs, have = [], [], []
        L = self.row_frames
        for b in range(len(self.lengths)):
            src = [self.source(b, t) for t in range(self.batch_frames)]
            for c in range(self.candidates):
                rows.append([(self.first[b] + w) * self.candidates + c for w, _ in src])
                offs.append([min(o, L - 1) for _, o in src])
                have.append([o < L for _, o in src])
        return rows, offs, have


def plan_windows(lengths: Sequence[int], window: int, overlap: int, candidates: int = 1, batch_frames: int = 0,
                 max_positions: int = 1 << 30) -> WindowPlan:
    """The plan for clips of `lengths` valid frames each (W = window, O = overlap, in frames)."""
    check_window(window, overlap, max_positions)
    lengths = [int(t) for t in lengths]
    if not lengths or min(lengths) < 1 or candidates < 1:
        raise ValueError("plan_windows: every clip needs at least one frame, and candidates >= 1")
    plan = WindowPlan(window=window, overlap=overlap, candidates=candidates, lengths=lengths,
                      batch_frames=max(int(batch_frames), max(lengths)))
    row = 0
    for T in lengths:
        n = window_count(T, window, overlap)
        plan.counts.append(n)
        plan.first.append(row)
        for w in range(n):
            for c in range(candidates):
                plan.next_row.append((row + w + 1) * candidates + c if w + 1 < n else -1)
        row += n
    return plan
