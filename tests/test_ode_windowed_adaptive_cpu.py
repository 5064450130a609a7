"""Adaptive solvers over window rows with step control per clip, without a GPU: the plan's groups and
ownership mask (sam_audio_amd/longform.py) against the plain loops of tests/ode_windowed_adaptive_ref.py and against the stitch; the
restatement against tests/ode_adaptive_ref.py for one-row groups and step for step against scipy's RK45 / RK23 on the stitched clip;
the keyword of separate(); the surface; and the controller hook's cases of tests/test_ode_windowed_adaptive_gpu.py on the SIMT
simulator (the real kernel code of kernels.hip)."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sam_audio_amd import hip, longform
from sam_audio_amd.model import ODE_ADAPTIVE_OPTIONS, SAMAudio, check_step_control, ode_adaptive
from tests import longform_ref as L
from tests import ode_adaptive_ref as A
from tests import ode_windowed_adaptive_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("candidates", [1, 2, 3])
@pytest.mark.parametrize("W,Ov", [(12, 3), (16, 4), (8, 4), (5, 1), (2, 1)])
def test_groups_partition_the_rows_and_own_every_valid_frame_once(W, Ov, candidates):
    """For clips shorter than, equal to and longer than a window (a last window with the minimum of O + 1 valid frames included):
    WindowPlan.groups() are the restatement's row lists and partition the engine rows; the frames a group owns number the clip's valid
    length; and the owned (row, frame) pairs are exactly the pairs the stitch reads for the clip's valid frames."""
    S = W - Ov
    lengths = [30, 12, 17, 1, W, W + 1, 2 * S + Ov, 2 * S + Ov + 1, 3 * S + 1]
    plan = longform.plan_windows(lengths, W, Ov, candidates)
    grp = ref.groups(lengths, W, Ov, candidates)
    table = plan.groups()
    assert len(table) == len(lengths) * candidates == len(grp)
    assert [[first + w * stride for w in range(n)] for first, n, stride in table] == grp
    assert sorted(r for g in grp for r in g) == list(range(plan.rows)), "every engine row in exactly one group"
    assert all(stride == candidates for _, _, stride in table) and [n for _, n, _ in table[::candidates]] == plan.counts
    mask = plan.owner_mask()
    assert torch.equal(torch.tensor(mask), ref.owner_mask(lengths, W, Ov, candidates, plan.row_frames))
    assert len(mask) == plan.rows and all(len(m) == plan.row_frames for m in mask)
    rows, offs, have = plan.stitch_index()
    for b, T in enumerate(lengths):
        for c in range(candidates):
            members = grp[b * candidates + c]
            owned = {(r, j) for r in members for j in range(plan.row_frames) if mask[r][j]}
            assert len(owned) == T, (b, c)
            out = b * candidates + c
            assert all(have[out][t] for t in range(T))
            assert owned == {(rows[out][t], offs[out][t]) for t in range(T)}, "owned = what the stitch reads"
            for r in members[:-1]:   # the successor links run inside a group, in its order
                assert plan.next_row[r] == members[members.index(r) + 1]
            assert plan.next_row[members[-1]] == -1


def test_a_plan_of_short_clips_has_one_row_groups():
    plan = longform.plan_windows([6, 5], 16, 4, 2, batch_frames=6)
    assert plan.groups() == [(0, 1, 2), (1, 1, 2), (2, 1, 2), (3, 1, 2)]
    assert plan.owner_mask() == [[True] * 6] * 2 + [[True] * 5 + [False]] * 2


# ------------------------------------------------------------------------------------------------ the restatement
def _rows_field():
    g = np.random.default_rng(5)
    lam = torch.from_numpy(-np.linspace(1.0, 60.0, 4))
    w = torch.from_numpy(g.standard_normal(4))

    def fn(t, y):   # [rows, frames, 4]: every frame on its own
        tt = t[:, None, None]
        return lam * y + 5.0 * torch.sin(12.0 * tt) * w + torch.sin(3.0 * y) * torch.roll(y, 1, dims=2)

    return fn, torch.from_numpy(g.standard_normal((3, 5, 4))) * torch.tensor([1.0, 0.01, 2.0])[:, None, None]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("method", ref.METHODS)
def test_one_row_groups_are_the_per_row_restatement_exactly(method, dtype):
    """Three rows of different scale, one of them padded, as three groups of one row with the pad mask as the ownership mask: every
    trial (t, h, err, decision), the evaluations and the state of tests/ode_adaptive_ref.solve, bit for bit."""
    fn, y0 = _rows_field()
    mask = torch.arange(5)[None, :] < torch.tensor([5, 3, 5])[:, None]
    want, ws = A.solve(fn, y0, method, 1e-4, 1e-7, dtype=dtype, mask=mask)
    got, gs = ref.solve(fn, y0, method, 1e-4, 1e-7, dtype=dtype, grp=[[0], [1], [2]], owner=mask)
    assert torch.equal(got, want) and gs["evaluations"] == ws["evaluations"]
    for a, b in zip(gs["groups"], ws["rows"]):
        assert a == b
    assert len({(r["accepted"], r["rejected"]) for r in ws["rows"]}) > 1, "the rows were meant to step differently"


LENGTHS, W, OV, C2 = (30, 12, 17), 12, 3, 6


def _frame_local_field():
    """every frame's derivative depends on that frame's values and t alone (on the channel, never on the frame's position): two
    copies of a frame in neighbouring windows receive equal derivatives and the blend of equal values is the identity.  Stiff-ish
    and linear plus a forcing, so that the explicit pairs are stability-bound and reject."""
    g = np.random.default_rng(11)
    lam = -np.linspace(1.0, 60.0, C2)
    w = g.standard_normal(C2)

    def f(t, y):   # y [..., C2]
        return lam * y + 5.0 * np.sin(12.0 * t) * w + 0.3 * np.sin(3.0 * y) * np.roll(y, 1, axis=-1)

    clips = [g.standard_normal((T, C2)) * (0.2 + b) for b, T in enumerate(LENGTHS)]
    return f, clips


@pytest.mark.parametrize("method", ref.METHODS)
def test_grouped_restatement_is_scipy_on_the_stitched_clip(method):
    """Clips of 30, 12 and 17 frames, W = 12, O = 3: 3, 1 and 2 windows, the last window of the 17-frame clip with 8 valid frames.
    The grouped solve of the six window rows in ONE call, float64, against scipy.integrate.RK45 / RK23 (max_step = inf) on each
    stitched clip vector of T_b * C2 values: the same accepted steps, rejections and evaluations per clip, the accepted times and the
    stitched state to float64 rounding - the bound and its caveat are tests/test_ode_adaptive_cpu.py's (ops * eps, ops = trials *
    (stages + 1) * (stages + 2); the field is contractive).  The blend adds no rounding: the two copies of a shared frame start
    equal, the field and the stage combinations are elementwise, so they stay equal bit for bit, q - p is exactly 0 and p + a (q - p)
    is p.  A norm that counted the overlap frames twice, or counted padding, would change err and with it every h: the times would
    differ in the first digits, not the last."""
    from scipy.integrate import RK23, RK45
    f, clips = _frame_local_field()
    S = {"dopri5": 6, "bosh3": 3}[method]
    rtol, atol = 1e-3, 1e-6
    T = max(LENGTHS)
    padded = torch.zeros(len(LENGTHS), T, C2, dtype=torch.float64)
    for b, c in enumerate(clips):
        padded[b, :len(c)] = torch.from_numpy(c)
    y0 = L.window_rows(padded, LENGTHS, W, OV)
    table = L.successor_table(LENGTHS, W, OV)
    grp = ref.groups(LENGTHS, W, OV)
    owner = ref.owner_mask(LENGTHS, W, OV)
    assert grp == [[0, 1, 2], [3], [4, 5]] and table == [1, 2, -1, -1, 5, -1] and tuple(y0.shape) == (6, W, C2)
    assert owner.sum(1).tolist() == [9, 9, 12, 12, 9, 8]

    def fn(t, y):
        out = torch.from_numpy(f(t.numpy()[:, None, None], y.numpy()))
        return L.blend(out, table, OV)

    got, stats = ref.solve(fn, y0, method, rtol, atol, grp=grp, owner=owner)
    latent = L.stitch(got, LENGTHS, W, OV, 1, T)
    rejected = 0
    for b, (Tb, clip) in enumerate(zip(LENGTHS, clips)):
        solver = {"dopri5": RK45, "bosh3": RK23}[method](lambda t, v: f(t, v.reshape(Tb, C2)).reshape(-1), 0.0, clip.reshape(-1), 1.0,
                                                         max_step=np.inf, rtol=rtol, atol=atol)
        ts = []
        while solver.status == "running":
            solver.step()
            ts.append(solver.t)
        row = stats["groups"][b]
        trials = row["accepted"] + row["rejected"]
        rejected += row["rejected"]
        print(f"{method} clip {b} ({Tb} frames, {len(grp[b])} windows): {row['accepted']} accepted, {row['rejected']} rejected")
        assert row["status"] == "finished" and row["t"] == 1.0 and solver.status == "finished"
        assert row["accepted"] == len(ts) and solver.nfev == 2 + S * trials
        ops = trials * (S + 1) * (S + 2)
        bound = ops * np.finfo(np.float64).eps
        dt = max(abs(a - c) for a, c in zip(row["ts"], ts))
        dy = np.abs(latent[b, :Tb].numpy().reshape(-1) - solver.y).max()
        print(f"  max |dt| {dt:.2e}, max |dy| {dy:.2e}, bound {bound:.2e} x max|y| {np.abs(solver.y).max():.2f}")
        assert dt <= bound
        assert dy <= bound * max(1.0, np.abs(solver.y).max(), np.abs(clip).max())
    assert rejected >= 1, "the stiff-ish field is there to force rejections"
    assert stats["evaluations"] == 2 + S * max(g["accepted"] + g["rejected"] for g in stats["groups"]), "finished groups ride along"
    assert len({tuple(g["ts"]) for g in stats["groups"]}) == 3, "the clips were meant to step differently"
    for r, s in enumerate(table):   # the rows of a clip stayed one trajectory
        if s >= 0:
            assert torch.equal(got[r, W - OV:], got[s, :OV])


# ------------------------------------------------------------------------------------------------ the keyword and the surface
def _opt(method="dopri5", **kw):
    return dict({"method": method, "rtol": 1e-3, "atol": 1e-4}, **kw)


def test_step_control_keyword():
    assert check_step_control(None, _opt()) is False and check_step_control("row", _opt()) is False
    assert check_step_control("clip", _opt()) is True and check_step_control("clip", _opt("bosh3")) is True
    assert check_step_control(None, {"method": "rk4"}) is False and check_step_control("row", {}) is False
    for bad in ("call", "Clip", 1, True):
        with pytest.raises(ValueError, match="step_control"):
            check_step_control(bad, _opt())
    for fixed in ({"method": "rk4"}, {"method": "midpoint"}, {}, {"method": "euler", "options": {"step_size": 0.5}}):
        with pytest.raises(ValueError, match="step_control='clip'.*fixed-grid"):
            check_step_control("clip", fixed)
    assert inspect.signature(SAMAudio.separate).parameters["step_control"].default is None
    assert set(ODE_ADAPTIVE_OPTIONS) == {"first_step", "safety", "ifactor", "dfactor", "max_num_steps"}


def test_separate_checks_the_keyword_before_anything_runs():
    """no model state is needed to be told; and the two refusals from before the keyword still stand, now pointing to it"""
    fn = getattr(SAMAudio.separate, "__wrapped__", SAMAudio.separate)
    with pytest.raises(ValueError, match="window_seconds.*step_control"):
        ode_adaptive(_opt(), windowed=True)
    for kw in ({}, {"step_control": None}, {"step_control": "row"}):
        with pytest.raises(ValueError, match="window_seconds"):
            fn(object(), None, ode_opt=_opt(), window_seconds=5.0, window_overlap_seconds=1.0, **kw)
    with pytest.raises(ValueError, match="fixed-grid"):
        fn(object(), None, ode_opt={"method": "rk4"}, step_control="clip")
    with pytest.raises(ValueError, match="fixed-grid"):
        fn(object(), None, step_control="clip", window_seconds=5.0, window_overlap_seconds=1.0)
    with pytest.raises(ValueError, match="step_control"):
        fn(object(), None, ode_opt=_opt(), step_control="batch")
    with pytest.raises(ValueError, match="defaults"):   # "clip" lifts the refusal of windows, nothing else
        fn(object(), None, ode_opt={"method": "dopri5"}, step_control="clip", window_seconds=5.0, window_overlap_seconds=1.0)
    with pytest.raises(RuntimeError, match="load_state_dict"):   # past every check: the model itself is asked for

        class Bare:
            _has_dit = _has_codec = False
        fn(Bare(), None, ode_opt=_opt(), step_control="clip", window_seconds=5.0, window_overlap_seconds=1.0)


def test_surface():
    header = open(os.path.join(ROOT, "include", "samaudio.h")).read()
    for name in ("samaudio_set_window_groups", "samaudio_op_ode_control_groups"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in hip.EXPORTED_SYMBOLS
    assert len(hip._PROTOS["samaudio_set_window_groups"][1]) == 4
    assert len(hip._PROTOS["samaudio_op_ode_control_groups"][1]) == len(hip._PROTOS["samaudio_op_ode_control"][1]) + 2
    kernels_h = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "kernels.h")).read()
    assert re.search(r"__attribute__\(\(weak\)\)\s+hipError_t\s+launch_ode_control_groups\(", kernels_h), "oracle/emu must still link"


# ------------------------------------------------------------------------------------------------ the kernel on the simulator
def test_controller_hook_cases_on_the_simulator():
    """tests/test_ode_windowed_adaptive_gpu.py's controller-hook cases with every product source on the SIMT simulator (conftest.py,
    SAMAUDIO_EMU_DRYRUN=simt): ode_control_groups_kernel itself, group sums, 257 groups and the null table included."""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_ode_windowed_adaptive_gpu.py", "-k", "hook"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, out
    assert "passed" in out and "failed" not in out and "skipped" not in out
