"""THE STATEMENT of the adaptive ODE solvers with per-row step control (samaudio.h samaudio_ode_solve_adaptive).

Pinned to scipy's RK45 / RK23; unpinned vs torchdiffeq (not installed).  The tableaux A, B, C, E are read from
scipy.integrate._ivp.rk.RK45 ("dopri5": Dormand-Prince 5(4), 6 evaluations per trial step, error-estimator order 4) and RK23
("bosh3": Bogacki-Shampine 3(2), 3 evaluations, order 2); both are FSAL.  The controller is scipy's RungeKutta._step_impl with
max_step = inf, the first step scipy's select_initial_step; tests/test_ode_adaptive_cpu.py runs this file step for step against scipy.

Every row integrates on its own from t0 to t1.  Per trial step of row r:
    scale = atol + rtol * max(|y|, |y_new|)
    err   = sqrt(mean((h * K^T E / scale)^2))     over the row's VALID frames (mask [rows, frames]; None: all) and all channels
    accept iff err < 1; then factor = min(ifactor, safety * err^(-1/(q+1))), ifactor at err == 0, and at most 1 if a trial of
    the same step was rejected before; on reject factor = max(dfactor, safety * err^(-1/(q+1)))
    a trial that would pass t1 ends at t1 exactly; min_step = 10 ulp(t) in the bookkeeping type: a step proposed below it is raised
    to it at the start of a step, and a REJECTION that drives h below it fails the row ("step_underflow")
    max_num_steps bounds the trial steps (accepted + rejected) of a row ("max_num_steps")
`first_step` replaces select_initial_step (which costs one more evaluation, with the same per-row norm); safety / ifactor / dfactor
are torchdiffeq's names for scipy's SAFETY / MAX_FACTOR / MIN_FACTOR.

Known departures from torchdiffeq's dopri5 / bosh3: (1) norm and step are per row, torchdiffeq's are per call (identical for one
row); (2) the last step is clipped to t1, torchdiffeq steps past t1 and interpolates back; (3) scipy's factor cap after a rejection.
Two correct adaptive solvers of one ODE at one tolerance differ by O(tolerance); no closer claim is made.

`dtype` is the bookkeeping type (t, h, norms, state and combinations): torch.float64 is the statement, torch.float32 what the engine
does.  Rows that have ended ride along: the field is still evaluated on their (unchanged) state at their own time, as the engine does,
so the number of field launches (`evaluations`) is the engine's."""
from typing import Callable, Optional

import numpy as np
import torch

METHODS = ("dopri5", "bosh3")
STATUS = ("running", "finished", "step_underflow", "max_num_steps")


def tableau(method: str):
    """(A, B, C, E, stages, order) of scipy's class, as float64 numpy arrays"""
    from scipy.integrate._ivp import rk
    cls = {"dopri5": rk.RK45, "bosh3": rk.RK23}[method]
    return cls.A, cls.B, cls.C, cls.E, cls.n_stages, cls.error_estimator_order


class Row:
    """a row's control block (the fields of the engine's, kernels.h OdeRowCtl)"""


class Controller:
    """scipy's RungeKutta._step_impl (max_step = inf) for one row, in the scalar type F (np.float32 | np.float64)"""

    def __init__(self, method, F, t1, safety=0.9, ifactor=10.0, dfactor=0.2, max_num_steps=2 ** 31 - 1):
        self.F, self.t1 = F, F(t1)
        self.safety, self.ifactor, self.dfactor = F(safety), F(ifactor), F(dfactor)
        self.expo = F(-1) / F(tableau(method)[5] + 1)
        self.max_num_steps = max_num_steps

    def new_row(self, t0):
        F, c = self.F, Row()
        c.t = c.t_new = F(t0)
        c.h = c.h_abs = c.h_prev = c.err = F(0)
        c.status, c.accepted, c.rejected, c.step_rejected = 0, 0, 0, False
        c.trials, c.ts = [], []
        return c

    def begin_trial(self, c):
        """the next trial step of a running row: h clipped to t1, or the row's failure"""
        F = self.F
        if c.accepted + c.rejected >= self.max_num_steps:
            c.status = 3
            return
        min_step = F(10) * (np.nextafter(c.t, F(np.inf)) - c.t)
        if not c.step_rejected:
            if c.h_abs < min_step:
                c.h_abs = min_step
        elif c.h_abs < min_step:
            c.status = 2
            return
        t_new = c.t + c.h_abs
        if t_new - self.t1 > 0:
            t_new = self.t1
        c.t_new = t_new
        c.h = t_new - c.t

    def decide(self, c, err) -> bool:
        """accept / reject the trial of a running row on its error norm, then begin the next trial; True: accepted"""
        F, ok = self.F, False
        c.err = err
        c.h_abs = c.h
        if err < 1:
            factor = self.ifactor if err == 0 else min(self.ifactor, self.safety * err ** self.expo)
            if c.step_rejected:
                factor = min(F(1), factor)
            c.trials.append((c.t, c.h, err, True))
            c.h_abs = c.h_abs * factor
            c.h_prev = c.h
            c.t = c.t_new
            c.ts.append(c.t)
            c.accepted += 1
            c.step_rejected = False
            ok = True
            if c.t - self.t1 >= 0:
                c.status = 1
        else:
            shrink = self.safety * err ** self.expo
            c.trials.append((c.t, c.h, err, False))
            c.h_abs = c.h_abs * (shrink if shrink > self.dfactor else self.dfactor)   # (a NaN norm shrinks by dfactor)
            c.rejected += 1
            c.step_rejected = True
        if c.status == 0:
            self.begin_trial(c)
        return ok


def _norm(x: torch.Tensor, mask: Optional[torch.Tensor], F):
    """per-row root mean square over the valid frames; x [rows, ...] -> list of F scalars"""
    out = []
    for r in range(x.shape[0]):
        v = x[r] if mask is None else x[r][mask[r]]
        out.append(F(torch.sqrt(torch.mean(v * v)).item()) if v.numel() else F(0))
    return out


def solve(fn: Callable, y0: torch.Tensor, method: str, rtol: float, atol: float, *, dtype=torch.float64,
          mask: Optional[torch.Tensor] = None, t0: float = 0.0, t1: float = 1.0, first_step: Optional[float] = None,
          safety: float = 0.9, ifactor: float = 10.0, dfactor: float = 0.2, max_num_steps: int = 2 ** 31 - 1):
    """fn(t [rows] tensor of `dtype`, y [rows, ...] of `dtype`) -> dy/dt [rows, ...].  Returns (y at t1, stats): stats["rows"][r] =
    {accepted, rejected, t, last_h, status, trials: [(t, h, err, accepted)], ts: [accepted t]}, stats["evaluations"]."""
    A, B, C, E, S, q = tableau(method)
    F = np.float32 if dtype == torch.float32 else np.float64
    A, B, C, E = A.astype(F), B.astype(F), C.astype(F), E.astype(F)
    y = y0.to(dtype).clone()
    rows = y.shape[0]
    shape1 = (rows,) + (1,) * (y.dim() - 1)
    rtol, atol, t0, t1 = F(rtol), F(atol), F(t0), F(t1)

    ctl = Controller(method, F, t1, safety, ifactor, dfactor, max_num_steps)
    R = [ctl.new_row(t0) for _ in range(rows)]
    begin_trial = ctl.begin_trial

    def running():
        return [c.status == 0 for c in R]

    def col(values):   # one value per row -> a tensor that broadcasts over the row
        return torch.tensor(np.array(values, dtype=F), dtype=dtype, device=y.device).reshape(shape1)

    def field(times, state):
        return fn(torch.tensor(np.array(times, dtype=F), dtype=dtype, device=y.device), state).to(dtype)

    def combine(coefs, K):   # y + h * sum_j coefs[j] K[j] on running rows, y on the others (their K is never looked at)
        acc = None
        for j, a in enumerate(coefs):
            if a != 0:
                acc = K[j] * float(a) if acc is None else acc + K[j] * float(a)
        run = torch.tensor(running(), device=y.device).reshape(shape1)
        return torch.where(run, y + acc * col([c.h for c in R]), y)

    evaluations = 1
    K = [None] * (S + 1)
    K[0] = field([c.t for c in R], y)
    if first_step is None:   # scipy select_initial_step, per row
        scale = atol + torch.abs(y) * rtol
        d0, d1 = _norm(y / scale, mask, F), _norm(K[0] / scale, mask, F)
        h0 = []
        for a, b in zip(d0, d1):
            h = F(1e-6) if (a < F(1e-5) or b < F(1e-5)) else F(0.01) * a / b
            h0.append(min(h, t1 - t0))
        y1 = y + col(h0) * K[0]
        f1 = field([t0 + h for h in h0], y1)
        evaluations += 1
        d2 = [n / h for n, h in zip(_norm((f1 - K[0]) / scale, mask, F), h0)]
        for c, h, b, d in zip(R, h0, d1, d2):
            if b <= F(1e-15) and d <= F(1e-15):
                h1 = max(F(1e-6), h * F(1e-3))
            else:
                h1 = (F(0.01) / max(b, d)) ** (F(1) / F(q + 1))
            c.h_abs = min(F(100) * h, h1, t1 - t0)
    else:
        for c in R:
            c.h_abs = F(first_step)
    for c in R:
        begin_trial(c)

    while any(running()):
        for i in range(1, S):
            K[i] = field([c.t + C[i] * c.h if c.status == 0 else c.t for c in R], combine(A[i][:i], K))
        y_new = combine(B, K)
        K[S] = field([c.t + c.h if c.status == 0 else c.t for c in R], y_new)
        evaluations += S
        est = None
        for j in range(S + 1):
            if E[j] != 0:
                est = K[j] * float(E[j]) if est is None else est + K[j] * float(E[j])
        scale = atol + torch.maximum(torch.abs(y), torch.abs(y_new)) * rtol
        errs = _norm(est * col([c.h for c in R]) / scale, mask, F)
        take = []
        for c, err in zip(R, errs):
            ok = ctl.decide(c, err) if c.status == 0 else False
            take.append(ok)
        sel = torch.tensor(take, device=y.device).reshape(shape1)
        y = torch.where(sel, y_new, y)
        K[0] = torch.where(sel, K[S], K[0])   # FSAL
    stats = {"evaluations": evaluations,
             "rows": [dict(accepted=c.accepted, rejected=c.rejected, t=float(c.t), last_h=float(c.h_prev), status=STATUS[c.status],
                           trials=c.trials, ts=c.ts) for c in R]}
    return y, stats


def oracle_stepper(method: str, rtol: float, atol: float, mask: Optional[torch.Tensor] = None, stats_out: Optional[list] = None,
                   **options) -> Callable:
    """A stand-in for oracle.samaudio_oracle.ode_fixed_grid (same signature; its `method` / `step_size` are ignored) that runs the
    float64-bookkeeping restatement ROW BY ROW: the oracle's field takes one time for the whole batch, so for row r it is evaluated on
    the batch with row r replaced by the row's state, and row r of the result is kept (rows of the field are independent)."""
    def ode_fixed_grid(fn, y0, method_=None, step_size=None, t0=0.0, t1=1.0, record=None, **kw):
        out = []
        for r in range(y0.shape[0]):
            def row_field(t, y_row, r=r):
                full = y0.clone()
                full[r] = y_row[0].to(y0.dtype)
                return fn(t[0].to(torch.float32), full)[r:r + 1]
            y, stats = solve(row_field, y0[r:r + 1], method, rtol, atol, dtype=torch.float64,
                             mask=None if mask is None else mask[r:r + 1], t0=t0, t1=t1, **options)
            out.append(y.to(y0.dtype))
            if stats_out is not None:
                stats_out.append(stats)
        return torch.cat(out)
    return ode_fixed_grid
