"""THE STATEMENT of the adaptive ODE solvers over window rows with step control PER CLIP (samaudio.h samaudio_set_window_groups,
DESIGN.md section 10.11).  It builds on tests/ode_adaptive_ref.py (the controller, pinned to scipy's RK45 / RK23) and on
tests/longform_ref.py (windows, successor table, blend, stitch) and changes neither.

A windowed solve cuts a clip of T valid frames into n window rows of W frames with stride S = W - O; after every evaluation of the
field the O frames two neighbouring rows share are cross-faded, so the rows of a clip describe ONE trajectory of the clip and must
stand at one time: they form a GROUP.

    group (clip b, candidate c)  = the engine rows (first[b] + w) * candidates + c, w < n_b    (a clip inside one window: one row)
    window w OWNS frame j of its row  iff  j is valid (j < min(W, T_b - w S)) and (j < S or w == n_b - 1)
      - longform_ref.stitch reads frame t of a clip from window min(t // S, n - 1): exactly the owned frames, T_b of them per group
    per trial step of a group, with scipy's controller exactly as tests/ode_adaptive_ref.py states it:
      scale = atol + rtol * max(|y|, |y_new|)
      err   = sqrt(sum over the group's OWNED elements of (h K^T E / scale)^2 / (T_b * C2))
    and the three norms of select_initial_step are taken the same way.  All rows of a group receive the same t, h, stage times and
    accept / reject decision; the field they are evaluated with ends with the blend (the caller's `fn` includes it).

Each frame of a clip is therefore counted once, whichever windows hold it: for a field that acts on every frame on its own (the
blend of equal values is the identity) the grouped solve of the window rows IS scipy's solve of the stitched clip vector, which
tests/test_ode_windowed_adaptive_cpu.py checks step for step.  Unpinned vs torchdiffeq, as section 10.9; the windowed solve itself
is this build's own definition, as section 10.7.

`dtype` is the bookkeeping type as in ode_adaptive_ref.solve: torch.float64 is the statement, torch.float32 what the engine does
(whose float32 sum of a group's norm runs over the chunk partials of its rows in window order - tests/test_ode_windowed_adaptive_gpu.py
states that order where it matters).  Groups that have ended ride along, as rows do there."""
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from tests import longform_ref as L
from tests import ode_adaptive_ref as A

METHODS = A.METHODS
STATUS = A.STATUS


# ---------------------------------------------------------------------------------------------------------------- groups and ownership
def groups(lengths: Sequence[int], W: int, Ov: int, candidates: int = 1) -> List[List[int]]:
    """per (clip, candidate), in the stitched latent's row order: the engine rows of its windows, in window order"""
    out, g = [], 0
    for T in lengths:
        n = L.windows(T, W, Ov)
        for c in range(candidates):
            out.append([(g + w) * candidates + c for w in range(n)])
        g += n
    return out


def owner_mask(lengths: Sequence[int], W: int, Ov: int, candidates: int = 1, row_frames: Optional[int] = None) -> torch.Tensor:
    """[engine rows, row_frames] bool (row_frames: W unless the rows are shorter): the frames a row owns"""
    S = W - Ov
    Lr = W if row_frames is None else row_frames
    rows = []
    for T in lengths:
        n = L.windows(T, W, Ov)
        for w in range(n):
            valid = min(W, T - w * S)
            row = [j < valid and (j < S or w == n - 1) for j in range(Lr)]
            for _ in range(candidates):
                rows.append(row)
    return torch.tensor(rows, dtype=torch.bool)


def _norm(x: torch.Tensor, grp: List[List[int]], owner: Optional[torch.Tensor], F):
    """per group the root mean square over its owned elements: the owned frames of its rows in window order, every channel"""
    out = []
    for rows in grp:
        if len(rows) == 1:   # (the expression of ode_adaptive_ref._norm, so that a one-row group is a row of that file bit for bit)
            r = rows[0]
            v = x[r] if owner is None else x[r][owner[r]]
        else:
            v = torch.cat([x[r] if owner is None else x[r][owner[r]] for r in rows])
        out.append(F(torch.sqrt(torch.mean(v * v)).item()) if v.numel() else F(0))
    return out


# ---------------------------------------------------------------------------------------------------------------- the solve
def solve(fn: Callable, y0: torch.Tensor, method: str, rtol: float, atol: float, *, grp: List[List[int]],
          owner: Optional[torch.Tensor] = None, dtype=torch.float64, t0: float = 0.0, t1: float = 1.0,
          first_step: Optional[float] = None, safety: float = 0.9, ifactor: float = 10.0, dfactor: float = 0.2,
          max_num_steps: int = 2 ** 31 - 1):
    """fn(t [rows] tensor of `dtype`, y [rows, frames, C2] of `dtype`) -> dy/dt [rows, frames, C2], the blend included; every row
    of a group is handed the group's time.  `grp`: lists of rows (every row in exactly one); `owner` [rows, frames] bool (None: every
    frame of every row is owned, which is right for one-row groups without padding only).  Returns (y at t1, stats): stats["groups"][g]
    = {accepted, rejected, t, last_h, status, trials: [(t, h, err, accepted)], ts: [accepted t]}, stats["evaluations"]."""
    Am, B, C, E, S, q = A.tableau(method)
    F = np.float32 if dtype == torch.float32 else np.float64
    Am, B, C, E = Am.astype(F), B.astype(F), C.astype(F), E.astype(F)
    y = y0.to(dtype).clone()
    rows = y.shape[0]
    assert sorted(r for g in grp for r in g) == list(range(rows)), "the groups must partition the rows"
    group_of = [0] * rows
    for g, members in enumerate(grp):
        for r in members:
            group_of[r] = g
    shape1 = (rows,) + (1,) * (y.dim() - 1)
    rtol, atol, t0, t1 = F(rtol), F(atol), F(t0), F(t1)

    ctl = A.Controller(method, F, t1, safety, ifactor, dfactor, max_num_steps)
    G = [ctl.new_row(t0) for _ in grp]

    def per_row(values):   # one value per group -> one per row
        return [values[group_of[r]] for r in range(rows)]

    def col(values):
        return torch.tensor(np.array(per_row(values), dtype=F), dtype=dtype, device=y.device).reshape(shape1)

    def field(times, state):
        return fn(torch.tensor(np.array(per_row(times), dtype=F), dtype=dtype, device=y.device), state).to(dtype)

    def combine(coefs, K):
        acc = None
        for j, a in enumerate(coefs):
            if a != 0:
                acc = K[j] * float(a) if acc is None else acc + K[j] * float(a)
        run = torch.tensor(per_row([c.status == 0 for c in G]), device=y.device).reshape(shape1)
        return torch.where(run, y + acc * col([c.h for c in G]), y)

    evaluations = 1
    K = [None] * (S + 1)
    K[0] = field([c.t for c in G], y)
    if first_step is None:   # scipy select_initial_step, per group
        scale = atol + torch.abs(y) * rtol
        d0, d1 = _norm(y / scale, grp, owner, F), _norm(K[0] / scale, grp, owner, F)
        h0 = []
        for a, b in zip(d0, d1):
            h = F(1e-6) if (a < F(1e-5) or b < F(1e-5)) else F(0.01) * a / b
            h0.append(min(h, t1 - t0))
        y1 = y + col(h0) * K[0]
        f1 = field([t0 + h for h in h0], y1)
        evaluations += 1
        d2 = [n / h for n, h in zip(_norm((f1 - K[0]) / scale, grp, owner, F), h0)]
        for c, h, b, d in zip(G, h0, d1, d2):
            if b <= F(1e-15) and d <= F(1e-15):
                h1 = max(F(1e-6), h * F(1e-3))
            else:
                h1 = (F(0.01) / max(b, d)) ** (F(1) / F(q + 1))
            c.h_abs = min(F(100) * h, h1, t1 - t0)
    else:
        for c in G:
            c.h_abs = F(first_step)
    for c in G:
        ctl.begin_trial(c)

    while any(c.status == 0 for c in G):
        for i in range(1, S):
            K[i] = field([c.t + C[i] * c.h if c.status == 0 else c.t for c in G], combine(Am[i][:i], K))
        y_new = combine(B, K)
        K[S] = field([c.t + c.h if c.status == 0 else c.t for c in G], y_new)
        evaluations += S
        est = None
        for j in range(S + 1):
            if E[j] != 0:
                est = K[j] * float(E[j]) if est is None else est + K[j] * float(E[j])
        scale = atol + torch.maximum(torch.abs(y), torch.abs(y_new)) * rtol
        errs = _norm(est * col([c.h for c in G]) / scale, grp, owner, F)
        take = [ctl.decide(c, err) if c.status == 0 else False for c, err in zip(G, errs)]
        sel = torch.tensor(per_row(take), device=y.device).reshape(shape1)
        y = torch.where(sel, y_new, y)
        K[0] = torch.where(sel, K[S], K[0])   # FSAL
    stats = {"evaluations": evaluations,
             "groups": [dict(accepted=c.accepted, rejected=c.rejected, t=float(c.t), last_h=float(c.h_prev), status=STATUS[c.status],
                             trials=c.trials, ts=c.ts) for c in G]}
    return y, stats


# ---------------------------------------------------------------------------------------------------------------- whole separate()
def stepper(lengths: Sequence[int], W: int, Ov: int, candidates: int, method: str, rtol: float, atol: float,
            stats_out: Optional[list] = None, **options) -> Callable:
    """A stand-in for tests.ode_ref.solve inside longform_ref.separate (same signature; its method and grid are ignored) that runs
    the float64-bookkeeping grouped restatement GROUP BY GROUP: longform_ref's field takes one time for all rows, so for a group it
    is evaluated on the batch with the group's rows replaced by the group's state, and the group's rows of the result are kept (the
    field's rows are independent and the blend links rows of one group only)."""
    grp = groups(lengths, W, Ov, candidates)

    def solve_rows(fn, y0, method_=None, grid=None, record=None):
        owner = owner_mask(lengths, W, Ov, candidates, row_frames=y0.shape[1])
        out = y0.clone()
        for members in grp:
            def group_field(t, y_rows, members=members):
                full = y0.clone()
                full[members] = y_rows.to(y0.dtype)
                return fn(t[0].to(torch.float32), full)[members]
            y, stats = solve(group_field, y0[members], method, rtol, atol, grp=[list(range(len(members)))], owner=owner[members],
                             dtype=torch.float64, **options)
            out[members] = y.to(y0.dtype)
            if stats_out is not None:
                stats_out.append(stats)
        return out
    return solve_rows
