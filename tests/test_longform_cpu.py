"""The window plan of the windowed separate() (sam_audio_amd/longform.py) against the plain-loop restatement in
tests/longform_ref.py: pure integer arithmetic, no GPU.  Plus the surface: the C declarations, the ctypes signatures and the keyword
arguments of SAMAudio.separate()."""
import inspect
import math
import os
import re

import pytest

from sam_audio_amd import SAMAudio, hip, longform
from tests import longform_ref as R
from tests.test_emu_cpu import emu  # noqa: F401  (fixture: the launcher emulation library, built on demand)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (T, W, O) -> (n, valid frames of the last window)
CASES = [
    ((16, 16, 4), (1, 16)),    # one window
    ((17, 16, 4), (2, 5)),     # two windows, the last with O + 1 valid frames: the minimum
    ((28, 16, 4), (2, 16)),    # two full windows
    ((29, 16, 4), (3, 5)),     # three windows, last 5
    ((40, 16, 4), (3, 16)),    # three full windows
    ((16, 16, 8), (1, 16)),    # O = W / 2
    ((17, 16, 8), (2, 9)),
    ((24, 16, 8), (2, 16)),
    ((25, 16, 8), (3, 9)),
    ((3, 16, 4), (1, 3)),      # shorter than a window
]


@pytest.mark.parametrize("case,want", CASES)
def test_window_count_and_last_window(case, want):
    T, W, O = case
    n = longform.window_count(T, W, O)
    S = W - O
    assert n == max(1, math.ceil((T - O) / S)) == R.windows(T, W, O) == want[0]
    plan = longform.plan_windows([T], W, O)
    assert plan.counts == [n] and plan.stride == S and plan.window_rows == n
    last = plan.valid_frames(0, n - 1)
    assert last == T - (n - 1) * S == want[1]
    if n > 1:
        assert O < last <= W, "the last window must hold more than the overlap"
        assert all(plan.valid_frames(0, w) == W for w in range(n - 1)), "every window but the last is full"


def test_formula_over_a_sweep():
    """every (T, W, O) with W <= 12: n, coverage of every frame by one or two windows, the source window of the stitch"""
    for W in range(2, 13):
        for O in range(1, W // 2 + 1):
            S = W - O
            for T in range(1, 5 * W):
                n = longform.window_count(T, W, O)
                assert n == R.windows(T, W, O) == max(1, -(-(T - O) // S))
                plan = longform.plan_windows([T], W, O)
                for t in range(T):
                    covering = [w for w in range(n) if w * S <= t < w * S + W]
                    assert 1 <= len(covering) <= 2, (T, W, O, t)
                    w, off = plan.source(0, t)
                    assert w in covering and off == t - w * S and 0 <= off < plan.valid_frames(0, w)
                if n > 1:
                    assert O < T - (n - 1) * S <= W


def test_successor_tables_with_and_without_candidates():
    lengths = [29, 17, 16]   # 3 + 2 + 1 windows
    plan = longform.plan_windows(lengths, 16, 4)
    assert plan.counts == [3, 2, 1] and plan.first == [0, 3, 5] and plan.rows == 6
    assert plan.next_row == [1, 2, -1, 4, -1, -1] == R.successor_table(lengths, 16, 4)
    two = longform.plan_windows(lengths, 16, 4, candidates=2)
    assert two.rows == 12
    assert two.next_row == [2, 3, 4, 5, -1, -1, 8, 9, -1, -1, -1, -1] == R.successor_table(lengths, 16, 4, 2)
    assert all(s == r + 2 for r, s in enumerate(two.next_row) if s >= 0), "the successor stride is the candidate count"


def test_gather_and_stitch_indices_round_trip():
    """window rows gathered from an index ramp and stitched back give the ramp on every valid frame, zeros behind the last row"""
    import torch
    lengths, W, O, cand = [29, 17], 16, 4, 2
    T = max(lengths)
    plan = longform.plan_windows(lengths, W, O, cand, batch_frames=T)
    assert plan.row_frames == W
    clip_of, frame_of, inside = plan.gather_index()
    assert clip_of == [0, 0, 0, 1, 1]
    x = torch.arange(2 * T).view(2, T, 1)
    rows = x[torch.tensor(clip_of)[:, None], torch.tensor(frame_of)].masked_fill(~torch.tensor(inside)[:, :, None], -1)
    assert torch.equal(rows, R.window_rows(x, lengths, W, O, fill=-1))
    rows_c = rows.repeat_interleave(cand, dim=0) * 10 + torch.tensor([0, 1]).repeat(5)[:, None, None]   # mark the candidate
    srow, soff, have = plan.stitch_index()
    got = rows_c[torch.tensor(srow), torch.tensor(soff)].masked_fill(~torch.tensor(have)[:, :, None], 0)
    assert torch.equal(got, R.stitch(rows_c, lengths, W, O, cand, T))
    for b, Tb in enumerate(lengths):
        for c in range(cand):
            assert got[b * cand + c, :Tb, 0].tolist() == [10 * (b * T + t) + c for t in range(Tb)]
    assert got[2, 28, 0] == 0 and not have[2][28], "clip 1 ends at frame 17; frame 28 lies behind its last window's row [12, 28)"
    # every clip inside one window: the rows are the whole clips (the plain path's shapes), nothing is linked
    one = longform.plan_windows([6, 5], 16, 4, batch_frames=6)
    assert one.row_frames == 6 and one.next_row == [-1, -1] and one.gather_index()[1] == [list(range(6))] * 2


@pytest.mark.parametrize("W,O", [(1, 1), (0, 1), (16, 0), (16, -1), (16, 9), (17, 9), (2, 2), (10001, 4)])
def test_refusals(W, O):
    assert R.refuses(W, O, 10000)
    with pytest.raises(ValueError):
        longform.check_window(W, O, 10000)
    with pytest.raises(ValueError):
        longform.plan_windows([100], W, O, max_positions=10000)


def test_accepted_edges():
    for W, O in [(2, 1), (16, 8), (17, 8), (10000, 5000)]:
        assert not R.refuses(W, O, 10000)
        longform.check_window(W, O, 10000)


def test_seconds_become_frames_by_rounding():
    sr, hop = 48000, 1920   # 25 frames per second
    assert longform.seconds_to_frames(10.0, sr, hop) == 250 == R.frames_of(10.0, sr, hop)
    assert longform.seconds_to_frames(1.0, sr, hop) == 25
    assert longform.seconds_to_frames(0.65, sr, hop) == int(round(0.65 * sr / hop)) == 16
    assert longform.seconds_to_frames(0.01, sr, hop) == 0   # ... which check_window then refuses as an overlap


def test_emulated_build_loads_and_refuses_windows(emu):
    """The launcher emulation (oracle/emu) has no window_blend launcher: the product references it weakly, so the library still binds
    both new entry points (the emu fixture) and answers SAMAUDIO_ERR_STATE; a forward without windows runs as before."""
    import torch

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
    B, T, Lt = 2, 4, 3
    buf, p, n = _ws(emu.samaudio_workspace_bytes(ctx, B, T, Lt, 0, 0))
    _check(emu, emu.samaudio_set_workspace(ctx, p, n))
    g = torch.Generator().manual_seed(2)
    z = torch.randn(B, T, 128, generator=g)
    feats, text = torch.cat([z, z], 2).contiguous(), torch.randn(B, Lt, 768, generator=g)
    _check(emu, emu.samaudio_prepare(ctx, B, T, Lt, hip.ptr(feats), hip.ptr(text), None, None, None, 0, None, None, None))
    nxt = torch.tensor([1, -1], dtype=torch.int32)
    assert emu.samaudio_set_windows(ctx, hip.ptr(nxt), B, 2) == hip.ERR_STATE
    assert "window_blend_kernel" in emu.samaudio_last_error().decode()
    y = synthetic_noise(B, T)
    keep_y = y.clone()
    assert emu.samaudio_op_window_blend(hip.ptr(y), hip.ptr(nxt), B, T, 2, 256, None) == hip.ERR_STATE
    assert torch.equal(y, keep_y)
    _check(emu, emu.samaudio_set_windows(ctx, None, 0, 0))
    out, t = torch.empty_like(y), torch.tensor([0.5])
    _check(emu, emu.samaudio_forward(ctx, hip.ptr(y), hip.ptr(t), 1, hip.ptr(out), None))
    assert torch.isfinite(out).all()
    emu.samaudio_destroy(ctx)


def test_kernel_and_refusals_on_the_simulator():
    """tests/test_longform_gpu.py's kernel-level cases with every product source on the SIMT simulator (conftest.py,
    SAMAUDIO_EMU_DRYRUN=simt): window_blend_kernel's indexing against the float64 blend for the six shapes, the C ABI's refusals and
    separate()'s ValueErrors.  (The whole-solve cases run the codec and take minutes there; they run on the GPU.)"""
    import subprocess
    import sys
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_longform_gpu.py", "-k", "kernel or refusals or value_error"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    out = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, out
    assert "8 passed" in out and "failed" not in out


def test_surface():
    """the two C entry points are declared, bound and typed; separate() has the two keyword arguments, None by default"""
    header = open(os.path.join(ROOT, "include", "samaudio.h")).read()
    for name in ("samaudio_set_windows", "samaudio_op_window_blend"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in hip.EXPORTED_SYMBOLS
    assert len(hip._PROTOS["samaudio_set_windows"][1]) == 4 and len(hip._PROTOS["samaudio_op_window_blend"][1]) == 7
    kernels_h = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "kernels.h")).read()
    assert re.search(r"__attribute__\(\(weak\)\)\s+hipError_t\s+launch_window_blend\(", kernels_h), "oracle/emu must still link"
    sig = inspect.signature(SAMAudio.separate).parameters
    assert sig["window_seconds"].default is None and sig["window_overlap_seconds"].default is None
