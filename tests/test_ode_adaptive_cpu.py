"""The adaptive ODE solvers without a GPU: the restatement tests/ode_adaptive_ref.py step for step against scipy's RK45 / RK23, its
per-row independence, the options of separate() (sam_audio_amd.model.ode_adaptive), the launcher emulation's refusal, and the light
cases of tests/test_ode_adaptive_gpu.py on the SIMT simulator (the real kernel code of kernels.hip)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sam_audio_amd import hip
from sam_audio_amd.model import ODE_ADAPTIVE_OPTIONS, is_adaptive, ode_adaptive, ode_grid
from tests import ode_adaptive_ref as ref
from tests.test_emu_cpu import emu  # noqa: F401  (fixture: the launcher emulation library, built on demand)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300


def _fields():
    g = np.random.default_rng(0)
    lam = -np.linspace(1.0, 60.0, N)                  # stiff-ish and linear: the explicit pairs are stability-bound and reject
    y_lin = g.standard_normal(N)
    w = g.standard_normal(N)

    def linear(t, y):
        return lam * y + 5.0 * np.sin(12.0 * t) * w

    def nonlinear(t, y):
        return np.sin(3.0 * y) * np.roll(y, 1) + np.cos(7.0 * t) - 0.5 * y ** 3

    return {"linear": (linear, y_lin), "nonlinear": (nonlinear, 1.5 * g.standard_normal(N))}


def _as_rows(f):
    """the numpy field of one row as the restatement's fn(t [1], y [1, N])"""
    return lambda t, y: torch.from_numpy(f(float(t[0]), y[0].numpy()))[None]


@pytest.mark.parametrize("method", ref.METHODS)
@pytest.mark.parametrize("name,rtol,atol", [("linear", 1e-3, 1e-6), ("nonlinear", 1e-5, 1e-8)])
def test_restatement_is_scipy_step_for_step(method, name, rtol, atol):
    """One row, float64 bookkeeping, against scipy.integrate.RK45 / RK23 driven through .step() with max_step = inf: the same accepted
    steps, the same evaluations, the accepted times and the final state to float64 rounding.
    The bound is eps times an operation count, and it is a heuristic, not a proof.  The count: scipy combines the stages with BLAS
    dots, the restatement in index order, so each of the (stages + 1) combinations of a trial step (the stage inputs, the candidate,
    the estimate) may differ by up to (stages + 2) roundings relative to its largest term; over all trial steps that is ops = trials *
    (stages + 1) * (stages + 2) roundings, and the bound is ops * eps * max|y| for the state and ops * eps for the accepted times (sums
    of h, each h a few roundings away from err).  What the count leaves out is how the field carries a difference from one step to
    the next: a factor of up to exp(L h) per step for a field of Lipschitz constant L (60 for the linear field) in general.  It is
    left out because both fields here are contractive on the states the solve visits (the linear one's rates are all negative, the
    nonlinear one is damped by -0.5 y^3) and an accepted step lies inside the pair's stability region, so differences shrink rather
    than grow; a field without that property would need the factor.  The counts are asserted first: the bound means something only
    while no accept / reject decision flips."""
    from scipy.integrate import RK23, RK45
    f, y0 = _fields()[name]
    S = {"dopri5": 6, "bosh3": 3}[method]
    solver = {"dopri5": RK45, "bosh3": RK23}[method](f, 0.0, y0, 1.0, max_step=np.inf, rtol=rtol, atol=atol)
    ts = []
    while solver.status == "running":
        solver.step()
        ts.append(solver.t)
    assert solver.status == "finished"
    got, stats = ref.solve(_as_rows(f), torch.from_numpy(y0)[None], method, rtol, atol)
    row = stats["rows"][0]
    trials = row["accepted"] + row["rejected"]
    print(f"{method} {name}: {row['accepted']} accepted, {row['rejected']} rejected, {stats['evaluations']} evaluations")
    assert row["status"] == "finished" and row["t"] == 1.0 and solver.t == 1.0
    assert row["accepted"] == len(ts)
    assert stats["evaluations"] == solver.nfev == 2 + S * trials
    if name == "linear":
        assert row["rejected"] >= 1, "the stiff-ish field is there to force rejections"
    ops = trials * (S + 1) * (S + 2)
    bound = ops * np.finfo(np.float64).eps
    dt = max(abs(a - b) for a, b in zip(row["ts"], ts))
    dy = np.abs(got[0].numpy() - solver.y).max()
    print(f"  max |dt| {dt:.2e}, max |dy| {dy:.2e}, bound {bound:.2e} x max|y| {np.abs(solver.y).max():.2f}")
    assert dt <= bound
    assert dy <= bound * max(1.0, np.abs(solver.y).max(), np.abs(y0).max())


@pytest.mark.parametrize("method", ref.METHODS)
def test_rows_are_independent_bit_for_bit(method):
    """three rows of very different scale (so their step sequences differ) in one call = the three one-row calls, float64"""
    f, y0 = _fields()["nonlinear"]
    y = torch.from_numpy(np.stack([y0, 0.01 * y0, np.roll(y0, 7) * 2.0]))

    def fn(t, yy):
        return torch.stack([torch.from_numpy(f(float(tt), row.numpy())) for tt, row in zip(t, yy)])

    whole, stats = ref.solve(fn, y, method, 1e-4, 1e-7)
    counts = set()
    for r in range(3):
        alone, s1 = ref.solve(fn, y[r:r + 1], method, 1e-4, 1e-7)
        assert torch.equal(alone[0], whole[r])
        a, b = s1["rows"][0], stats["rows"][r]
        assert (a["accepted"], a["rejected"], a["ts"]) == (b["accepted"], b["rejected"], b["ts"])
        counts.add((a["accepted"], a["rejected"]))
    assert len(counts) > 1, "the rows were meant to take different step sequences"


def test_padding_frames_never_enter_a_norm():
    """mask [rows, frames]: garbage dynamics in the padding frames of a row change nothing for its step sequence"""
    def fn(t, y):   # frames 3.. of every row are 1000 times faster
        rate = torch.ones(y.shape[1], 1, dtype=y.dtype)
        rate[3:] = 1000.0
        return -rate * y * torch.cos(t)[:, None, None]

    y0 = torch.linspace(0.5, 2.0, 5 * 4, dtype=torch.float64).reshape(1, 5, 4)
    mask = torch.tensor([[True, True, True, False, False]])
    _, masked = ref.solve(fn, y0, "dopri5", 1e-6, 1e-9, mask=mask)
    _, short = ref.solve(fn, y0[:, :3], "dopri5", 1e-6, 1e-9)
    _, full = ref.solve(fn, y0, "dopri5", 1e-6, 1e-9)
    assert masked["rows"][0]["ts"] == short["rows"][0]["ts"]
    assert full["rows"][0]["accepted"] > masked["rows"][0]["accepted"]


def test_restatement_options_and_failures():
    f, y0 = _fields()["linear"]
    fn, y = _as_rows(f), torch.from_numpy(y0)[None]
    _, base = ref.solve(fn, y, "bosh3", 1e-3, 1e-6)
    _, first = ref.solve(fn, y, "bosh3", 1e-3, 1e-6, first_step=0.5)
    assert first["evaluations"] == 1 + 3 * (first["rows"][0]["accepted"] + first["rows"][0]["rejected"])
    assert first["rows"][0]["trials"][0][1] == 0.5 and not first["rows"][0]["trials"][0][3]
    _, cautious = ref.solve(fn, y, "bosh3", 1e-3, 1e-6, safety=0.5, ifactor=2.0, dfactor=0.5)
    assert cautious["rows"][0]["accepted"] > base["rows"][0]["accepted"]
    _, capped = ref.solve(fn, y, "bosh3", 1e-3, 1e-6, max_num_steps=2)
    r = capped["rows"][0]
    assert r["status"] == "max_num_steps" and r["accepted"] + r["rejected"] == 2 and r["t"] < 1.0
    _, f32 = ref.solve(fn, y, "bosh3", 1e-3, 1e-6, dtype=torch.float32)
    assert f32["rows"][0]["status"] == "finished" and f32["rows"][0]["t"] == 1.0


# ------------------------------------------------------------------------------------------------ option parsing
def _opt(method="dopri5", **kw):
    return dict({"method": method, "rtol": 1e-3, "atol": 1e-4}, **kw)


def test_accepted_adaptive_options():
    code, p = ode_adaptive(_opt())
    assert code == hip.ODE_DOPRI5 and is_adaptive(_opt()) and not is_adaptive({"method": "rk4"}) and not is_adaptive({})
    assert (p.rtol, p.atol) == (np.float32(1e-3), np.float32(1e-4))
    assert (p.first_step, p.safety, p.ifactor, p.dfactor, p.max_num_steps) == (0.0, np.float32(0.9), 10.0, np.float32(0.2), 2 ** 31 - 1)
    code, p = ode_adaptive(_opt("bosh3", options={"first_step": 0.25, "safety": 0.8, "ifactor": 5, "dfactor": 0.5, "max_num_steps": 40}))
    assert code == hip.ODE_BOSH3
    assert (p.first_step, p.safety, p.ifactor, p.dfactor, p.max_num_steps) == (0.25, np.float32(0.8), 5.0, 0.5, 40)
    assert set(ODE_ADAPTIVE_OPTIONS) == {"first_step", "safety", "ifactor", "dfactor", "max_num_steps"}
    for empty in ({}, None):
        assert ode_adaptive(_opt(options=empty))[1].max_num_steps == 2 ** 31 - 1
    assert ode_adaptive(_opt(options={"first_step": None}))[1].first_step == 0.0


@pytest.mark.parametrize("key", ["step_size", "grid_constructor", "norm", "step_t", "jump_t", "dtype", "max_step"])
def test_refused_adaptive_option_keys(key):
    with pytest.raises(ValueError, match=key):
        ode_adaptive(_opt(options={key: 0.5}))


def test_refused_adaptive_ode_opts():
    for missing in ("rtol", "atol"):
        opt = _opt()
        del opt[missing]
        with pytest.raises(ValueError, match=r"torchdiffeq's defaults \(1e-7 / 1e-9\) lie below what an fp32"):
            ode_adaptive(opt)
    with pytest.raises(ValueError, match="defaults"):
        ode_adaptive({"method": "bosh3"})
    for bad in (dict(rtol=0.0), dict(atol=-1e-3), dict(rtol=float("nan")), dict(atol=float("inf"))):
        with pytest.raises(ValueError, match="positive"):
            ode_adaptive(_opt(**bad))
    for options in ({"first_step": 0.0}, {"first_step": 2.0}, {"safety": 0.0}, {"ifactor": 0.5}, {"dfactor": 1.0}, {"dfactor": 0.0},
                    {"max_num_steps": 0}):
        with pytest.raises(ValueError):
            ode_adaptive(_opt(options=options))
    with pytest.raises(ValueError, match="adjoint"):
        ode_adaptive(_opt(adjoint_params=()))
    for method in ("dopri8", "fehlberg2", "adaptive_heun", "explicit_adams", "rk4"):
        with pytest.raises(ValueError, match="dopri5 . bosh3"):
            ode_adaptive(_opt(method))
    with pytest.raises(ValueError, match="window_seconds"):
        ode_adaptive(_opt(), windowed=True)


def test_fixed_grid_parser_keeps_its_behaviour():
    """ode_grid stays the fixed-grid function: the adaptive methods are not its, and rtol / atol in a fixed-grid method's options
    are refused as before"""
    with pytest.raises(ValueError, match="ode_adaptive"):
        ode_grid(_opt())
    with pytest.raises(ValueError, match="rtol"):
        ode_grid({"method": "rk4", "options": {"step_size": 0.25, "rtol": 1e-3}})
    assert ode_grid({"method": "rk4", "rtol": 1e-3, "atol": 1e-3, "options": {"step_size": 0.5}}) == (hip.ODE_RK4, [0.0, 0.5, 1.0])


def test_separate_refuses_before_anything_runs():
    """separate() checks an adaptive ode_opt first: no model state is needed to be told about missing tolerances or windows"""
    from sam_audio_amd.model import SAMAudio
    fn = getattr(SAMAudio.separate, "__wrapped__", SAMAudio.separate)
    with pytest.raises(ValueError, match="window_seconds"):
        fn(object(), None, ode_opt=_opt(), window_seconds=5.0, window_overlap_seconds=1.0)
    with pytest.raises(ValueError, match="defaults"):
        fn(object(), None, ode_opt={"method": "dopri5"})


# ------------------------------------------------------------------------------------------------ the launcher emulation build
def test_emulated_build_refuses_the_adaptive_methods(emu):
    """The launcher emulation has none of the four launchers: the library binds (the emu fixture), sizes the stage buffer, and refuses
    the solve and every hook with SAMAUDIO_ERR_STATE, leaving the state alone; samaudio_ode_solve refuses the ids with ERR_ARG."""
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
    need = emu.samaudio_ode_stage_bytes(ctx, hip.ODE_DOPRI5, B, T)
    assert need > 8 * B * T * 256 * 4 > emu.samaudio_ode_stage_bytes(ctx, hip.ODE_BOSH3, B, T) > 5 * B * T * 256 * 4
    stages, sp, sn = _ws(need)
    _check(emu, emu.samaudio_set_ode_stages(ctx, sp, sn))
    noise = synthetic_noise(B, T)
    state = noise.clone()
    params = ode_adaptive(_opt())[1]
    stats = (hip.OdeRowStats * B)()
    for method in (hip.ODE_DOPRI5, hip.ODE_BOSH3):
        assert emu.samaudio_ode_solve_adaptive(ctx, hip.ptr(state), method, 0.0, 1.0, C.byref(params), stats, None) == hip.ERR_STATE
        assert "not available in this build" in emu.samaudio_last_error().decode()
        grid = (C.c_float * 2)(0.0, 1.0)
        assert emu.samaudio_ode_solve(ctx, hip.ptr(state), method, grid, 2, None) == hip.ERR_ARG
    assert emu.samaudio_ode_solve_adaptive(ctx, hip.ptr(state), hip.ODE_RK4, 0.0, 1.0, C.byref(params), stats, None) == hip.ERR_ARG
    assert torch.equal(state, noise)
    emu.samaudio_destroy(ctx)


# ------------------------------------------------------------------------------------------------ the kernels on the simulator
def test_light_adaptive_cases_on_the_simulator():
    """tests/test_ode_adaptive_gpu.py's light cases with every product source on the SIMT simulator (conftest.py,
    SAMAUDIO_EMU_DRYRUN=simt): the four kernel hooks against float64, the controller's decision table, the error paths, and the
    engine's loop against the restatement over the host-driven field at 'tiny' dims (bosh3 on the model as initialised: about half a
    minute on the simulator; the other three cases of that test take four more and stay with the hardware)."""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_ode_adaptive_gpu.py", "-k", "light and not pushed and not dopri5-plain"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    out = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, out
    assert "29 passed" in out and "failed" not in out and "skipped" not in out
