"""Restatement of torchdiffeq's fixed-grid ODE steppers over an arbitrary time grid: the oracle of the engine's ODE methods
(samaudio.h SAMAUDIO_ODE_*).  torchdiffeq itself is not installed; the formulas follow its
fixed_grid.py / rk_common.py in its grouping: rk4 is rk4_alt_step_func (the 3/8 rule, not classical RK4), heun3 the Heun3
tableau.  Stage times are computed like torchdiffeq computes them on float32 time tensors (t0 + dt * c, the last rk4 stage at t1).

`oracle_stepper` builds a drop-in for oracle.samaudio_oracle.ode_fixed_grid, which oracle.samaudio_oracle.separate calls by its
module-level name: tests monkeypatch it so that encode, field, candidates and decode of the oracle are reused unchanged."""
import math
from typing import Callable, List, Optional, Sequence

import torch

METHODS = ("euler", "midpoint", "rk4", "heun3")
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4, "heun3": 3}


def step_grid(step_size: float, t0: float = 0.0, t1: float = 1.0) -> List[float]:
    """torchdiffeq's grid from step_size: t0 + k h, the last point clamped to t1 (the values sam_audio_amd.model.ode_grid builds)"""
    n = int(math.ceil((t1 - t0) / step_size + 1))
    grid = [min(t0 + k * step_size, t1) for k in range(n)]
    grid[-1] = t1
    return grid


def step(fn: Callable, method: str, ta: float, tb: float, y0: torch.Tensor) -> torch.Tensor:
    """One step ta -> tb of `method`; fn(t, y) with t a float32 scalar tensor."""
    t0, t1 = torch.tensor(ta, dtype=torch.float32), torch.tensor(tb, dtype=torch.float32)
    dt_t = t1 - t0
    dt = float(dt_t)
    k1 = fn(t0, y0)
    if method == "euler":
        return y0 + dt * k1
    if method == "midpoint":
        half = 0.5 * dt
        return y0 + dt * fn(t0 + 0.5 * dt_t, y0 + k1 * half)
    if method == "rk4":
        k2 = fn(t0 + dt_t * (1 / 3), y0 + dt * k1 * (1 / 3))
        k3 = fn(t0 + dt_t * (2 / 3), y0 + dt * (k2 - k1 * (1 / 3)))
        k4 = fn(t1, y0 + dt * (k1 - k2 + k3))
        return y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
    if method == "heun3":
        k2 = fn(t0 + dt_t * (1 / 3), y0 + dt * k1 * (1 / 3))
        k3 = fn(t0 + dt_t * (2 / 3), y0 + dt * (k2 * (2 / 3)))
        return y0 + dt * (k1 * 0.25 + k3 * 0.75)
    raise ValueError(f"unknown method {method!r}")


def solve(fn: Callable, y0: torch.Tensor, method: str, grid: Sequence[float], record: Optional[list] = None) -> torch.Tensor:
    y = y0
    for ta, tb in zip(grid[:-1], grid[1:]):
        y = step(fn, method, float(ta), float(tb), y)
        if record is not None:
            record.append(y)
    return y


def oracle_stepper(grid: Optional[Sequence[float]] = None) -> Callable:
    """A stand-in for oracle.samaudio_oracle.ode_fixed_grid (same signature) that runs every method of METHODS; `grid` replaces the
    step-size grid (a grid_constructor's grid, or [0, 1] for no options)."""
    def ode_fixed_grid(fn, y0, method="midpoint", step_size=2 / 32, t0=0.0, t1=1.0, record=None):
        g = list(grid) if grid is not None else step_grid(step_size, t0, t1)
        return solve(fn, y0, method, g, record)
    return ode_fixed_grid
