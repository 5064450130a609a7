"""ODE options of separate() (sam_audio_amd.model.ode_grid, torchdiffeq's FixedGridODESolver semantics), the restated rk4 / heun3
steppers of tests/ode_ref.py in closed form, and the light cases of tests/test_ode_methods_gpu.py on the SIMT simulator
(ode_stage_kernel, the in-place last combination and the stage-buffer plumbing with the real kernel code)."""
import os
import subprocess
import sys

import pytest
import torch

from sam_audio_amd import hip
from sam_audio_amd.model import ode_grid
from tests import ode_ref
from tests.test_emu_cpu import emu  # noqa: F401  (fixture: the launcher emulation library, built on demand)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ option parsing
@pytest.mark.parametrize("method,code", [("rk4", hip.ODE_RK4), ("heun3", hip.ODE_HEUN3), ("euler", hip.ODE_EULER),
                                         ("midpoint", hip.ODE_MIDPOINT)])
def test_step_size_grids_for_every_method(method, code):
    got = ode_grid({"method": method, "options": {"step_size": 1 / 8}})
    assert got == (code, ode_ref.step_grid(1 / 8)) and len(got[1]) == 9 and got[1][0] == 0.0 and got[1][-1] == 1.0
    assert ode_grid({"method": method, "options": {"step_size": 0.3}})[1] == [0.0, 0.3, 0.6, 0.8999999999999999, 1.0]


def test_no_options_is_one_step():
    for opt in ({"method": "rk4"}, {"method": "euler", "options": {}}, {"method": "heun3", "options": None}):
        assert ode_grid(opt)[1] == [0.0, 1.0]


def test_grid_constructor_is_called_like_torchdiffeq():
    calls = []
    y0 = torch.randn(3, 5, 256)

    def constructor(func, y, t):
        calls.append((func, y, t))
        return torch.tensor([0.0, 0.1, 0.3, 0.6, 1.0])

    method, grid = ode_grid({"method": "rk4", "options": {"grid_constructor": constructor}}, y0=y0)
    assert method == hip.ODE_RK4
    assert grid == torch.tensor([0.0, 0.1, 0.3, 0.6, 1.0]).tolist()
    (func, y, t), = calls
    assert y is y0 and t.tolist() == [0.0, 1.0] and t.device == y0.device
    with pytest.raises(NotImplementedError, match="grid_constructor"):
        func(t[0], y0)
    # a list or a float64 tensor is taken as well
    assert ode_grid({"method": "heun3", "options": {"grid_constructor": lambda f, y, t: [0.0, 0.5, 1.0]}}, y0=y0)[1] == [0, 0.5, 1]
    g64 = ode_grid({"method": "midpoint", "options": {"grid_constructor": lambda f, y, t: torch.tensor([0, 0.25, 1.0],
                                                                                                       dtype=torch.float64)}})
    assert g64 == (hip.ODE_MIDPOINT, [0.0, 0.25, 1.0])


@pytest.mark.parametrize("bad,why", [
    ([0.1, 0.5, 1.0], "start at"),
    ([0.0, 0.5, 0.99], "end at"),
    ([0.0, 0.6, 0.3, 1.0], "strictly increasing"),
    ([0.0, 0.5, 0.5, 1.0], "strictly increasing"),
    ([0.0, 0.5, 0.5 + 1e-12, 1.0], "strictly increasing"),   # distinct in float64, equal in the float32 the engine integrates over
    ([[0.0, 0.5, 1.0]], "1-D"),
    ([0.0], "1-D"),
])
def test_grid_constructor_results_are_validated(bad, why):
    with pytest.raises(ValueError, match=why):
        ode_grid({"method": "rk4", "options": {"grid_constructor": lambda f, y, t: torch.tensor(bad, dtype=torch.float64)}})


def test_rejected_options_and_methods():
    both = {"step_size": 0.25, "grid_constructor": lambda f, y, t: t}
    with pytest.raises(ValueError, match="mutually exclusive"):
        ode_grid({"method": "rk4", "options": both})
    with pytest.raises(ValueError, match="rtol"):
        ode_grid({"method": "rk4", "options": {"step_size": 0.25, "rtol": 1e-3}})
    for method in ("dopri5", "dopri8", "bosh3", "fehlberg2", "adaptive_heun", "explicit_adams", "implicit_adams", "fixed_adams",
                   "scipy_solver", "rk4_classic"):
        with pytest.raises(ValueError, match="euler | midpoint | rk4 | heun3"):
            ode_grid({"method": method, "options": {"step_size": 0.25}})


def test_grids_longer_than_the_engine_time_table_are_refused():
    """rk4 takes 4 evaluation times per step, heun3 3, of the engine's 4096"""
    assert len(ode_grid({"method": "rk4", "options": {"step_size": 1 / 1024}})[1]) == 1025
    with pytest.raises(ValueError, match="time table"):
        ode_grid({"method": "rk4", "options": {"step_size": 1 / 1025}})
    assert len(ode_grid({"method": "heun3", "options": {"step_size": 1 / 1365}})[1]) == 1366
    with pytest.raises(ValueError, match="time table"):
        ode_grid({"method": "heun3", "options": {"step_size": 1 / 1366}})


# ------------------------------------------------------------------------------------------------ the restated steppers
def test_restated_steppers_on_exponential_growth():
    """y' = y, eight steps of 1/8: an s-stage method of order s = s <= 4 reproduces the Taylor polynomial of e^h per step."""
    h = 1 / 8
    y0 = torch.ones(4, dtype=torch.float64)
    field = lambda t, y: y   # noqa: E731
    rk4 = ode_ref.solve(field, y0, "rk4", ode_ref.step_grid(h))
    heun3 = ode_ref.solve(field, y0, "heun3", ode_ref.step_grid(h))
    assert torch.allclose(rk4, torch.full_like(y0, (1 + h + h ** 2 / 2 + h ** 3 / 6 + h ** 4 / 24) ** 8), rtol=1e-14, atol=0)
    assert torch.allclose(heun3, torch.full_like(y0, (1 + h + h ** 2 / 2 + h ** 3 / 6) ** 8), rtol=1e-14, atol=0)


def test_restated_steppers_pin_the_nodes_and_weights():
    """y' = t^4, one step over [0, 1]: torchdiffeq's rk4 (3/8 rule) gives 11/54 where classical RK4 would give 5/24, heun3 gives 4/27."""
    y0 = torch.zeros(2, dtype=torch.float64)
    field = lambda t, y: torch.full_like(y, float(t) ** 4)   # noqa: E731
    rk4 = ode_ref.solve(field, y0, "rk4", [0.0, 1.0])
    heun3 = ode_ref.solve(field, y0, "heun3", [0.0, 1.0])
    assert (rk4 - 11 / 54).abs().max() < 1e-7 and (rk4 - 5 / 24).abs().min() > 1e-3
    assert (heun3 - 4 / 27).abs().max() < 1e-7


def test_restated_stepper_replaces_the_oracle_stepper_for_midpoint_and_euler():
    """The monkeypatched stand-in agrees with oracle.samaudio_oracle.ode_fixed_grid where both are defined."""
    from oracle import samaudio_oracle as O
    g = torch.Generator().manual_seed(0)
    A = torch.randn(6, 6, generator=g) / 3
    y0 = torch.randn(2, 6, generator=g)
    field = lambda t, y: y @ A.T + t   # noqa: E731
    for method in ("midpoint", "euler"):
        want = O.ode_fixed_grid(field, y0, method=method, step_size=0.3)
        got = ode_ref.oracle_stepper()(field, y0, method=method, step_size=0.3)
        assert (got - want).abs().max() < 1e-6


# ------------------------------------------------------------------------------------------------ the launcher emulation build
def test_emulated_build_loads_and_refuses_the_runge_kutta_methods(emu):
    """The launcher emulation (oracle/emu) has no ode_stage launcher: engine.hip references it weakly, so the library still binds every
    entry point (the emu fixture) and a Runge-Kutta solve is refused with SAMAUDIO_ERR_STATE, leaving the state alone; midpoint runs."""
    import ctypes as C

    from sam_audio_amd import preset_config
    from sam_audio_amd.synthetic import init_state_dict, synthetic_noise
    from sam_audio_amd.weights import convert_dit
    from tests.test_emu_cpu import _check, _engine, _set, _ws

    cfg = preset_config("tiny")
    keep = []
    ctx = _engine(emu, cfg, hip.F32, keep)
    _set(emu, emu.samaudio_set_tensor, ctx, convert_dit(init_state_dict(cfg, seed=3, with_codec=False), cfg, torch.float32, "cpu"),
         keep)
    _check(emu, emu.samaudio_finalize(ctx, 0))
    B, T, Lt = 1, 2, 3
    buf, p, n = _ws(emu.samaudio_workspace_bytes(ctx, B, T, Lt, 0, 0))
    _check(emu, emu.samaudio_set_workspace(ctx, p, n))
    g = torch.Generator().manual_seed(2)
    z = torch.randn(B, T, 128, generator=g)
    feats, text = torch.cat([z, z], 2).contiguous(), torch.randn(B, Lt, 768, generator=g)
    _check(emu, emu.samaudio_prepare(ctx, B, T, Lt, hip.ptr(feats), hip.ptr(text), None, None, None, 0, None, None, None))
    stages, sp, sn = _ws(emu.samaudio_ode_stage_bytes(ctx, hip.ODE_RK4, B, T))
    _check(emu, emu.samaudio_set_ode_stages(ctx, sp, sn))
    noise = synthetic_noise(B, T)
    state = noise.clone()
    grid = (C.c_float * 3)(0.0, 0.5, 1.0)
    for method in (hip.ODE_RK4, hip.ODE_HEUN3):
        assert emu.samaudio_ode_solve(ctx, hip.ptr(state), method, grid, 3, None) == hip.ERR_STATE
        assert "not available in this build" in emu.samaudio_last_error().decode()
    assert torch.equal(state, noise)
    _check(emu, emu.samaudio_ode_solve(ctx, hip.ptr(state), hip.ODE_MIDPOINT, grid, 3, None))
    assert torch.isfinite(state).all() and not torch.equal(state, noise)
    emu.samaudio_destroy(ctx)


# ------------------------------------------------------------------------------------------------ the kernel on the simulator
def test_light_ode_method_cases_on_the_simulator():
    """tests/test_ode_methods_gpu.py's light cases with every product source on the SIMT simulator (conftest.py,
    SAMAUDIO_EMU_DRYRUN=simt): rk4 and heun3 against the host-driven field at 'tiny' dims, the time-table and stage-buffer refusals."""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_ode_methods_gpu.py", "-k", "host or time_table or stage_buffer"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    out = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, out
    assert "4 passed" in out and "failed" not in out
