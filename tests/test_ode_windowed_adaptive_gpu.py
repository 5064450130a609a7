"""dopri5 / bosh3 over window rows with step control PER CLIP (samaudio.h samaudio_set_window_groups) on the
device.  The statement is tests/ode_windowed_adaptive_ref.py (pinned to scipy on the stitched clip by
tests/test_ode_windowed_adaptive_cpu.py).  Here: ode_control_groups_kernel through its hook against the float32 restatement's
decisions, the engine's grouped loop against the restatement over the field driven from the host, the bits the overlaps hold, a batch
against its clips solved alone, candidates, the clip inside one window, whole separate() against the statement, the refusals and the
untouched defaults.  The tests named `light` make sense on the SIMT simulator as well (those named `hook` run there from
tests/test_ode_windowed_adaptive_cpu.py)."""
import contextlib
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from sam_audio_amd import SAMAudioProcessor, hip, longform, preset_config
from sam_audio_amd.model import DFLT_ODE_OPT, ode_adaptive
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
from tests import longform_ref as L
from tests import ode_adaptive_ref as A
from tests import ode_windowed_adaptive_ref as ref
from tests import util
from tests.test_ode_adaptive_gpu import FIN, FW, IW, METHOD, RUN, _ctl, _ulps
from tests.test_ode_methods_gpu import _model, _solve_inputs
from tests.test_tower_kernels_gpu import NAN, _all_nan, _dev, _lib, _nan, _ok, _same_bits

pytestmark = pytest.mark.gpu

F = np.float32
LENGTHS, W, OV = (30, 12, 17), 12, 3            # 3, 1 and 2 windows; the last window of the 17-frame clip holds 8 valid frames
ADAPTIVE = {"method": "dopri5", "rtol": 1e-3, "atol": 1e-3}


def _seconds(cfg, frames):
    return frames * cfg.audio_codec.hop_length / cfg.audio_codec.sample_rate


def _win(cfg, w=W, o=OV):
    return dict(window_seconds=_seconds(cfg, w), window_overlap_seconds=_seconds(cfg, o), step_control="clip")


# ---------------------------------------------------------------------------------------------------------------------
# 1. ode_control_groups through its hook
# ---------------------------------------------------------------------------------------------------------------------
def _members(table, rows):
    return [[first + w * stride for w in range(n) if 0 <= first + w * stride < rows] for first, n, stride in table]


def _ordered_sum(part, members, reverse=False):
    """the stated order in float32: the group's rows in window order, the chunks of a row in order, one accumulator"""
    ss = F(0)
    cells = [(r, k) for r in members for k in range(part.shape[1])]
    for r, k in (reversed(cells) if reverse else cells):
        ss = F(ss + F(part[r, k].item()))
    return ss


def _launch(gpu, hook, ctl, mode, method, opt, part, part_b, chunks, mask, frames, channels, times, active, rows, table=None,
            t0=0.0):
    params = ode_adaptive(dict({"method": method, "rtol": 1e-3, "atol": 1e-3}, options=opt))[1]
    args = [hip.ptr(ctl), mode, METHOD[method], t0, 1.0, C.byref(params), None if part is None else hip.ptr(part),
            None if part_b is None else hip.ptr(part_b), chunks, None if mask is None else hip.ptr(mask), frames, channels,
            hip.ptr(times), hip.ptr(active), rows]
    if hook == "groups":
        tab = None if table is None else _dev(torch.tensor(table, dtype=torch.int32), gpu)
        args += [None if tab is None else hip.ptr(tab), rows if table is None else len(table)]
    fn = getattr(_lib("fp32"), "samaudio_op_ode_control_groups" if hook == "groups" else "samaudio_op_ode_control")
    _ok("fp32", fn(*args, util.stream()))


# group -> (fields of every row of the group before the decision, the err its partials are scaled to)
TABLE = [(0, 1, 2), (1, 1, 2), (2, 2, 2), (3, 2, 2), (6, 3, 2), (7, 3, 2), (17, 2, 2)]   # the last one lies behind the rows: absent
GROUP_CASES = [
    ("1 row, err 0.5: accepted", dict(t=0.125, h=0.0625), 0.5),
    ("1 row, err 4: rejected", dict(t=0.125, h=0.0625), 4.0),
    ("2 rows, accepted after a rejection: factor capped at 1", dict(t=0.25, h=0.03125, step_rejected=1, rejected=1), 0.01),
    ("2 rows, finished: untouched", dict(t=1.0, h=0.03125, status=FIN, accepted=9, rejected=2), 0.5),
    ("3 rows, the next step would pass t1: clipped", dict(t=0.875, h=0.0625), 0.001),
    ("3 rows, err 2: rejected", dict(t=0.25, h=0.0625), 2.0),
]


@pytest.mark.parametrize("frames,overlap", [(17, 3), (4, 1)])
@pytest.mark.parametrize("method", ref.METHODS)
def test_light_control_groups_hook_decision_table(gpu, method, frames, overlap):
    """One launch over groups of 1, 2 and 3 rows with the row stride of two candidates (12 rows; a seventh table entry points behind
    them), rows of `frames` x 256 elements: 17 frames are 4352 elements, two chunks, 4 frames one.  Every group's sum must be the
    float32 sum of its partials in the stated order - the partials of every group of four or more terms (17 frames) are drawn so that
    the reversed order gives another err (on the reference) - and its decision the float32 restatement's Controller's, with
    test_light_control_decision_table's bounds: integers, t and err exact, one ulp where powf enters.  Every row of a group ends with
    the same 64 bytes and the same column of the time table; the partials of a finished group (NaN) are never read; nothing is
    written behind the rows."""
    S = A.tableau(method)[4]
    Cn = [float(np.float32(c)) for c in A.tableau(method)[2]] + [1.0]
    rows, channels = 12, 256
    chunks = -(-frames * channels // 4096)
    members = _members(TABLE, rows)
    assert members[:6] == [[0], [1], [2, 4], [3, 5], [6, 8, 10], [7, 9, 11]] and members[6] == []
    ctl_ref = A.Controller(method, F, 1.0, max_num_steps=1000)
    g = torch.Generator().manual_seed(31 + frames)
    part = torch.zeros(rows, chunks)
    fields = {k: [0.0] * rows for k in FW} | {k: [0] * rows for k in IW}
    want = []
    for (name, f, err), rows_g in zip(GROUP_CASES, members):
        n = ((len(rows_g) - 1) * (frames - overlap) + frames) * channels                  # the owned frames of the group
        for draw in range(64):   # partials of one magnitude, drawn until the reversed order gives the group another err
            p = 0.5 + torch.rand(len(rows_g), chunks, generator=g)
            part[rows_g] = p * (err * err * n / p.double().sum().item())
            ss = _ordered_sum(part, rows_g)
            other = np.sqrt(_ordered_sum(part, rows_g, reverse=True) / F(n))
            # (two terms commute; with three the difference rarely survives the root)
            if len(rows_g) * chunks < 4 or other != np.sqrt(ss / F(n)):
                break
        else:
            raise AssertionError(f"{name}: no draw in which the order of the sum matters")
        c = ctl_ref.new_row(0.0)
        c.t, c.h = F(f["t"]), F(f["h"])
        c.t_new, c.h_abs = F(c.t + c.h), c.h
        c.status, c.accepted, c.rejected = f.get("status", RUN), f.get("accepted", 3), f.get("rejected", 0)
        c.step_rejected = bool(f.get("step_rejected", 0))
        c.n_valid = n
        for r in rows_g:
            for k in FW:
                fields[k][r] = float(getattr(c, k, 0.0))
            for k in IW:
                fields[k][r] = int(getattr(c, k, 0))
        if c.status == RUN:
            c.took = ctl_ref.decide(c, np.sqrt(ss / F(n)))
            assert abs(float(c.err) - err) < 1e-3 * err
        else:
            c.took = False
            part[rows_g] = NAN
        want.append(c)
    before = torch.cat([_ctl(rows, **fields), torch.full((1, hip.ODE_CTL_WORDS), NAN)])
    ctl = _dev(before, gpu)
    times = _nan((S + 2, rows), torch.float32, gpu)
    active = torch.full((2,), -7, dtype=torch.int32, device=gpu)
    _launch(gpu, "groups", ctl, 3, method, {"max_num_steps": 1000}, _dev(part, gpu), None, chunks, None, frames, channels, times,
            active, rows, TABLE)
    got, tm = ctl.cpu(), times.cpu()
    gi = got.view(torch.int32)
    assert _all_nan(got[rows]) and _all_nan(tm[S + 1]), "something was written behind the rows"
    assert active.cpu().tolist() == [sum(len(m) for m, c in zip(members, want) if c.status == RUN), -7]
    for (name, f, err), rows_g, c in zip(GROUP_CASES, members, want):
        lead = rows_g[0]
        for r in rows_g[1:]:
            assert _same_bits(got[r], got[lead]) and _same_bits(tm[:S + 1, r], tm[:S + 1, lead]), f"{name}: row {r} vs its leader"
        line = {k: got[lead, FW[k]].item() for k in FW} | {k: gi[lead, IW[k]].item() for k in IW}
        print(f"{method} frames={frames} {name}: {line}")
        if f.get("status", RUN) != RUN:
            assert _same_bits(got[rows_g], before[rows_g]), name
            continue
        assert (line["status"], line["accepted"], line["rejected"], line["step_rejected"], line["accepted_now"], line["n_valid"]) == \
            (c.status, c.accepted, c.rejected, int(c.step_rejected), int(c.took), c.n_valid), name
        assert line["t"] == float(c.t), name
        assert line["err"] == float(c.err), f"{name}: the group's sum is not the float32 sum in the stated order"
        power = not (c.took and f.get("step_rejected"))
        assert _ulps(line["h_abs"], c.h_abs) <= (1 if power else 0), name
        assert c.status == RUN
        assert _ulps(line["h"], c.h) <= 1 and _ulps(line["t_new"], c.t_new) <= 1, name
        for i in range(S + 1):
            assert _ulps(tm[i, lead].item(), c.t + F(Cn[i]) * c.h) <= 1, (name, i)
    clipped = got[members[4][2]]
    assert clipped[FW["t_new"]] == 1.0 and clipped[FW["h"]] == 1.0 - 0.9375
    assert got[members[2][1], FW["h_abs"]] == 0.03125


def test_light_control_groups_hook_reset_counts_owned_frames(gpu):
    """mode 0 over the plan of clips of 30, 12 and 17 frames, W = 12, O = 3, two candidates, with the plan's ownership mask: every
    row of a group holds n_valid = the clip's valid frames x channels - each frame once - t = t0, counters 0, and with first_step the
    first trial, the same in every row."""
    plan = longform.plan_windows(LENGTHS, W, OV, 2)
    rows, table = plan.rows, plan.groups()
    assert rows == 12 and table == [(0, 3, 2), (1, 3, 2), (6, 1, 2), (7, 1, 2), (8, 2, 2), (9, 2, 2)]
    mask = _dev(torch.tensor(plan.owner_mask(), dtype=torch.uint8), gpu)
    assert tuple(mask.shape) == (rows, W) and torch.equal(mask.cpu().bool(), ref.owner_mask(LENGTHS, W, OV, 2))
    clip_of_row = [0] * 6 + [1] * 2 + [2] * 4
    for first, h in ((None, 0.0), (0.25, 0.25), (1.0, 0.75)):
        ctl = _nan((rows + 1, hip.ODE_CTL_WORDS), torch.float32, gpu)
        times = _nan((8, rows), torch.float32, gpu)
        active = torch.zeros(1, dtype=torch.int32, device=gpu)
        _launch(gpu, "groups", ctl, 0, "dopri5", {"first_step": first}, None, None, 0, mask, W, 256, times, active, rows, table, t0=0.25)
        got = ctl.cpu()
        gi = got.view(torch.int32)
        assert _all_nan(got[rows]) and _all_nan(times.cpu()[7])
        assert gi[:rows, IW["n_valid"]].tolist() == [LENGTHS[b] * 256 for b in clip_of_row] and active.item() == rows
        assert not gi[:rows, [IW[k] for k in ("status", "accepted", "rejected", "step_rejected", "accepted_now")]].any()
        assert got[:rows, FW["t"]].tolist() == [0.25] * rows and got[:rows, FW["h"]].tolist() == [h] * rows
        assert times.cpu()[0].tolist() == [0.25] * rows and times.cpu()[6].tolist() == [0.25 + h] * rows


def _sequence(gpu, hook, table, rows, frames, channels, mask, parts, method="bosh3"):
    """RESET, INIT1, INIT2, STEP, STEP through one hook; the bytes of (ctl, times, active) after each"""
    S = A.tableau(method)[4]
    chunks = parts[0].shape[1]
    ctl = _nan((rows + 1, hip.ODE_CTL_WORDS), torch.float32, gpu)
    times = _nan((S + 2, rows), torch.float32, gpu)
    active = torch.full((2,), -7, dtype=torch.int32, device=gpu)
    seen = []
    for mode, a, b in ((0, None, None), (1, 0, 1), (2, 2, None), (3, 3, None), (3, 4, None)):
        _launch(gpu, hook, ctl, mode, method, {}, None if a is None else _dev(parts[a], gpu), None if b is None else _dev(parts[b], gpu),
                chunks if mode else 0, mask, frames, channels, times, active, rows, table)
        seen.append((ctl.cpu().clone(), times.cpu().clone(), active.cpu().clone()))
    return seen


def _same_sequence(a, b):
    for step, (x, y) in enumerate(zip(a, b)):
        assert _same_bits(x[0], y[0]), f"control blocks after launch {step}"
        assert _same_bits(x[1], y[1]), f"time table after launch {step}"
        assert torch.equal(x[2], y[2]), f"active after launch {step}"


def test_light_control_groups_hook_257_one_row_groups(gpu):
    """257 groups of one row (1 frame x 4 channels): lanes loop.  An explicit table of one-row groups through all five modes gives the
    bytes of the per-row hook, and lane 0's second group (row 256) is stepped like every other."""
    rows = 257
    g = torch.Generator().manual_seed(7)
    parts = [torch.rand(rows, 1, generator=g) * s for s in (4.0, 9.0, 1e-3, 1.0, 6.0)]   # the STEPs: err up to 0.5, then up to 1.2
    table = [(r, 1, 1) for r in range(rows)]
    want = _sequence(gpu, "rows", None, rows, 1, 4, None, parts)
    got = _sequence(gpu, "groups", table, rows, 1, 4, None, parts)
    _same_sequence(got, want)
    last = got[-1][0].view(torch.int32)
    assert last[256, IW["accepted"]] + last[256, IW["rejected"]] == 2 and got[-1][2][0].item() > 0
    assert {int(v) for v in last[:rows, IW["rejected"]]} == {0, 1}, "both decisions were meant to occur"


def test_light_control_groups_hook_null_table_is_the_per_row_hook(gpu):
    """groups = NULL: every row its own group.  Five rows of 17 frames x 256 (two chunks) with a pad mask, through RESET, INIT1, INIT2
    and two STEPs: the control blocks, the time table and the running count of samaudio_op_ode_control, bit for bit."""
    rows, frames = 5, 17
    g = torch.Generator().manual_seed(9)
    mask = _dev((torch.arange(frames)[None, :] < torch.tensor([17, 1, 9, 16, 17])[:, None]).to(torch.uint8), gpu)
    parts = [torch.rand(rows, 2, generator=g) * s for s in (4e3, 9e3, 1.0, 2e3, 5e3)]
    want = _sequence(gpu, "rows", None, rows, frames, 256, mask, parts)
    _same_sequence(_sequence(gpu, "groups", None, rows, frames, 256, mask, parts), want)
    _same_sequence(_sequence(gpu, "groups", [(r, 1, 1) for r in range(rows)], rows, frames, 256, mask, parts), want)
    assert {int(v) for v in want[-1][0].view(torch.int32)[:rows, IW["rejected"]]} >= {0, 1}


# ---------------------------------------------------------------------------------------------------------------------
# 2. the engine's grouped loop against the restatement over the field driven from the host
# ---------------------------------------------------------------------------------------------------------------------
MARGIN = 1e-2
# (seed of the inputs, gain on transformer.output.weight, options): tests/test_ode_adaptive_gpu.py's `pushed` case - a 16 x stronger
# output projection and a first trial of the whole interval, which no embedded pair accepts at 1e-3
ENGINE_CASE = (4, 16.0, {"first_step": 1.0})


def _window_inputs(lengths, w, o, seed, scale=None):
    """whole-clip features, text and noise cut into window rows (longform_ref.window_rows), and the row tables"""
    B, T = len(lengths), max(lengths)
    feats, text, tmask, noise = _solve_inputs(B, T, 5, seed=seed)
    if scale is not None:
        noise = noise * torch.tensor(scale)[:, None, None]
    pad = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]
    clip_of = [b for b, Tb in enumerate(lengths) for _ in range(L.windows(Tb, w, o))]
    return dict(feats=L.window_rows(feats, lengths, w, o), text=text[clip_of], tmask=tmask[clip_of],
                noise=L.window_rows(noise, lengths, w, o), pad=L.window_rows(pad, lengths, w, o, fill=False),
                next_row=L.successor_table(lengths, w, o), grp=ref.groups(lengths, w, o), owner=ref.owner_mask(lengths, w, o))


@pytest.mark.parametrize("method", ref.METHODS)
def test_light_engine_grouped_loop_equals_the_restatement_over_the_host_driven_field(gpu, method):
    """samaudio_ode_solve_adaptive with a group table against tests/ode_windowed_adaptive_ref.py over samaudio_forward with the window
    table set (so the field ends with window_blend_kernel) and per-row times, fp32, rtol = atol = 1e-3.  'mini', clips of 30 and 17
    frames, W = 12, O = 3: 3 + 2 window rows, the second clip at a quarter of the scale; 'tiny' with 8-frame windows (O = 2, clips of 20
    and 11 frames: 3 + 2 rows) on the simulator.
    Condition, asserted on the two reference runs alone (float32 and float64 bookkeeping), exactly as
    test_light_engine_loop_equals_the_restatement_over_the_host_driven_field does: no trial of the float64 run has its err in
    [1 - m, 1 + m], m = 1e-2 (that test's derivation: the estimate is a difference of O(|K|) terms carrying eps |K| each, so err is
    uncertain by about 7 eps |K| h / (atol + rtol |y|) = 2e-3 at |K| <= 5, h <= 1; a group's norm is a mean over more elements of the
    same per-element uncertainty, so the figure carries over; 1e-2 leaves a factor of 5), the float32 run takes the same sequence,
    some group rejects, and the two groups step differently.
    Then: every row of a group reports the group's accepted / rejected steps of the reference, the evaluations are the reference's,
    and the window rows lie within 4 x the float32-vs-float64 reference difference of the float64 run."""
    sim = gpu.type != "cuda"
    cfg = preset_config("tiny" if sim else "mini")
    lengths, w, o = ((20, 11), 8, 2) if sim else ((30, 17), W, OV)
    seed, gain, options = ENGINE_CASE
    sd = init_state_dict(cfg, seed=41, with_codec=False)
    sd["transformer.output.weight"] = sd["transformer.output.weight"] * gain
    x = _window_inputs(lengths, w, o, seed, scale=[1.0, 0.25])
    rows = x["noise"].shape[0]
    assert x["grp"] == [[0, 1, 2], [3, 4]] and x["next_row"] == [1, 2, -1, 4, -1]
    model = _model(cfg, sd, "fp32", gpu)
    lib = model._lib
    model._prepare(x["feats"], x["text"], x["tmask"], None, None, None, x["pad"])
    nxt = _dev(torch.tensor(x["next_row"], dtype=torch.int32), gpu)
    hip.check(lib.samaudio_set_windows(model._ctx, hip.ptr(nxt), rows, o))

    def field(t, y):   # the blend is inside: the successor table is set
        yy, tt = y.float().contiguous(), t.float().contiguous()
        out = torch.empty_like(yy)
        hip.check(lib.samaudio_forward(model._ctx, hip.ptr(yy), hip.ptr(tt), rows, hip.ptr(out), util.stream()))
        return out.to(y.dtype)

    runs = {}
    for dtype in (torch.float64, torch.float32):
        runs[dtype] = ref.solve(field, x["noise"].to(gpu), method, 1e-3, 1e-3, dtype=dtype, grp=x["grp"], owner=x["owner"].to(gpu),
                                **options)
    (y64, s64), (y32, s32) = runs[torch.float64], runs[torch.float32]
    seq = lambda s: [[a for _, _, _, a in r["trials"]] for r in s["groups"]]   # noqa: E731
    errs = [e for r in s64["groups"] for _, _, e, _ in r["trials"]]
    print(f"{method}: float64 reference trials (t, h, err, accepted): {[r['trials'] for r in s64['groups']]}")
    assert all(r["status"] == "finished" for r in s64["groups"] + s32["groups"])
    assert not any(1 - MARGIN <= e <= 1 + MARGIN for e in errs), "an err of the float64 run lies inside the margin: pick another seed"
    assert seq(s64) == seq(s32) and s64["evaluations"] == s32["evaluations"]
    assert any(r["rejected"] >= 1 for r in s64["groups"]), "the pushed case is there for its rejections"
    assert s64["groups"][0]["ts"] != s64["groups"][1]["ts"], "the two groups were meant to step differently"

    table = _dev(torch.tensor([(g[0], len(g), 1) for g in x["grp"]], dtype=torch.int32), gpu)
    owner = _dev(x["owner"].to(torch.uint8), gpu)
    hip.check(lib.samaudio_set_window_groups(model._ctx, hip.ptr(table), len(x["grp"]), hip.ptr(owner)))
    got = model.solve(x["noise"].to(gpu), {"method": method, "rtol": 1e-3, "atol": 1e-3, "options": options})
    hip.check(lib.samaudio_set_windows(model._ctx, None, 0, 0))
    st = model.last_ode_stats
    print(f"{method}: engine {st}")
    for g, want, want32 in zip(x["grp"], s64["groups"], s32["groups"]):
        for r in g:
            e = st["rows"][r]
            assert (e["accepted"], e["rejected"], e["status"], e["t"]) == (want["accepted"], want["rejected"], "finished", 1.0)
            assert e == st["rows"][g[0]], "the rows of a group hold one control block"
            assert abs(e["last_h"] - want32["last_h"]) <= 1e-3 * want32["last_h"]
    assert st["evaluations"] == s64["evaluations"]
    assert st["rows"][0]["last_h"] != st["rows"][3]["last_h"], "the two groups were meant to step differently"
    for r, s in enumerate(x["next_row"]):
        if s >= 0:
            assert _same_bits(got[r, w - o:], got[s, :o]), f"link {r} -> {s}"
    spread = (y32.double() - y64).abs().max().item()
    err = (got.double() - y64).abs().max().item()
    print(f"{method} grouped engine vs float64 restatement: max-abs {err:.3e}; float32 vs float64 restatement {spread:.3e}; ratio "
          f"{err / spread:.2f} (bound 4); |latent| <= {y64.abs().max().item():.2f}")
    assert torch.isfinite(got).all() and err <= 4 * spread


# ---------------------------------------------------------------------------------------------------------------------
# 3. - 5. bits: the overlaps, a batch and its clips, candidates (the windowed solve of separate(), on given latent features)
# ---------------------------------------------------------------------------------------------------------------------
def _clips_case(seed=8):
    """three clips of 30, 12 and 17 frames of different scale; features and noise are zero behind a clip's valid length, as a clip
    solved alone has nothing there"""
    B, T = len(LENGTHS), max(LENGTHS)
    feats, text, tmask, _ = _solve_inputs(B, T, 5, seed=seed)
    noise = synthetic_noise(2 * B, T, seed=seed) * torch.tensor([1.0, 1.0, 0.25, 0.25, 0.5, 0.5])[:, None, None]
    pad = torch.arange(T)[None, :] < torch.tensor(LENGTHS)[:, None]
    z = feats[:, :, :128] * pad[:, :, None]
    noise = noise * pad.repeat_interleave(2, dim=0)[:, :, None]
    return z, text, tmask, pad, noise


def _solve_clips(model, gpu, case, clips, cand, noise_rows, opt):
    """SAMAudio._solve_windowed (what separate() runs between the encoder and the decoder) on the clips `clips` of the case, trimmed to
    their longest; returns (stitched latent, statistics, window rows, plan)"""
    z, text, tmask, pad, noise = case
    lengths = [LENGTHS[b] for b in clips]
    T = max(lengths)
    cond = [z[clips, :T].to(gpu), text[clips].to(gpu), tmask[clips].to(gpu), None, None, None, pad[clips, :T].to(gpu)]
    batch = types.SimpleNamespace(sizes_host=lengths)
    with torch.inference_mode(), (torch.cuda.device(gpu) if gpu.type == "cuda" else contextlib.nullcontext()):
        lat = model._solve_windowed(batch, noise[noise_rows, :T].to(gpu), cond, (W, OV), cand, True, opt)
    return lat.clone(), model.last_ode_stats, model.last_window_latent.clone(), model.last_window_plan


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("method", ref.METHODS)
def test_overlaps_hold_the_same_bits_and_a_batch_equals_its_clips_solved_alone(gpu, prec, method):
    """Clips with 3, 1 and 2 windows in one grouped solve.  (3.) In the window rows the tail of a row equals the head of its successor
    bit for bit: the rows of a clip received the same field bits, the same h and the same decision at every trial.  (4.) The stitched
    latent and the statistics of every clip equal the clip solved alone - the 12-frame clip alone is one row on the per-row path -
    although the clips take different step sequences; and a repeated solve equals itself."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=14, with_codec=False)
    case = _clips_case()
    model = _model(cfg, sd, prec, gpu)
    opt = dict(ADAPTIVE, method=method)
    whole, stats, rows, plan = _solve_clips(model, gpu, case, [0, 1, 2], 1, [0, 2, 4], opt)
    assert plan.counts == [3, 1, 2] and plan.next_row == [1, 2, -1, -1, 5, -1] and stats["windows"] == [3, 1, 2]
    assert len(stats["rows"]) == 3 and all(r["status"] == "finished" and r["t"] == 1.0 for r in stats["rows"])
    for r, s in enumerate(plan.next_row):
        if s >= 0:
            assert _same_bits(rows[r, W - OV:], rows[s, :OV]), f"link {r} -> {s}"
    again, stats2, rows2, _ = _solve_clips(model, gpu, case, [0, 1, 2], 1, [0, 2, 4], opt)
    assert torch.equal(whole, again) and torch.equal(rows, rows2) and stats == stats2, "run-to-run determinism"
    counts = set()
    for b in range(3):
        alone, s1, _, p1 = _solve_clips(model, gpu, case, [b], 1, [2 * b], opt)
        assert p1.counts == [plan.counts[b]]
        assert torch.equal(alone[0], whole[b, :LENGTHS[b]]), f"clip {b} alone differs from the batch"
        assert s1["rows"][0] == stats["rows"][b]
        counts.add((s1["rows"][0]["accepted"], s1["rows"][0]["rejected"], s1["rows"][0]["last_h"]))
    print(f"{prec} {method}: {stats}")
    assert torch.isfinite(whole).all() and len(counts) > 1, "the clips were meant to step differently"


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_two_candidates_equal_the_two_single_candidate_runs(gpu, prec):
    """row stride 2: the groups of candidate 0 and candidate 1 of a clip interleave; each equals its own single-candidate solve"""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=14, with_codec=False)
    case = _clips_case()
    model = _model(cfg, sd, prec, gpu)
    case[4][1::2] *= 0.5   # the second candidate of every clip at another scale
    both, stats, _, plan = _solve_clips(model, gpu, case, [0, 1, 2], 2, list(range(6)), ADAPTIVE)
    assert plan.groups() == [(0, 3, 2), (1, 3, 2), (6, 1, 2), (7, 1, 2), (8, 2, 2), (9, 2, 2)] and len(stats["rows"]) == 6
    for c in range(2):
        one, s1, _, _ = _solve_clips(model, gpu, case, [0, 1, 2], 1, [c, 2 + c, 4 + c], ADAPTIVE)
        assert torch.equal(both[c::2], one), f"candidate {c}"
        assert stats["rows"][c::2] == s1["rows"]
    assert stats["rows"][0] != stats["rows"][1], "the candidates were meant to step differently"


# ---------------------------------------------------------------------------------------------------------------------
# 6. - 8. separate()
# ---------------------------------------------------------------------------------------------------------------------
def _batch(cfg, frames, anchors=None):
    hop = cfg.audio_codec.hop_length
    longest = max(frames)
    clips = [synthetic_clip(i, n * hop if n == longest else (n - 1) * hop + 100) for i, n in enumerate(frames)]
    text, tmask = synthetic_text_features(len(frames), 5, ragged=True)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * len(frames), audios=clips, anchors=anchors, text_features=text,
                                               text_mask=tmask)
    assert batch.sizes_host == list(frames)
    return batch, text, tmask


def _profiled(model, gpu, fn):
    if gpu.type != "cuda":   # (no hipEvents off hardware)
        return fn(), None
    model.profile_begin()
    out = fn()
    return out, {r["name"]: r["launches"] for r in model.profile_end()}


def test_light_a_clip_inside_one_window_is_the_per_row_solve(gpu):
    """Clips with T <= W, step_control="clip" and windows: the bits and the statistics of the plain adaptive separate(), and the
    profile shows the per-row controller and no launch of the windowed solve."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=7)
    batch, _, _ = _batch(cfg, (6, 5))
    batch = batch.to(gpu)
    noise = synthetic_noise(2, 6).to(gpu)
    model = _model(cfg, sd, "fp32", gpu)
    plain, names0 = _profiled(model, gpu, lambda: model.separate(batch, noise=noise, ode_opt=ADAPTIVE))
    lat, stats = model.last_latent.clone(), model.last_ode_stats
    keyword = model.separate(batch, noise=noise, ode_opt=ADAPTIVE, step_control="clip")
    assert torch.equal(model.last_latent, lat) and model.last_ode_stats == stats, "without windows a clip is a row"
    win, names = _profiled(model, gpu, lambda: model.separate(batch, noise=noise, ode_opt=ADAPTIVE, **_win(cfg, 16, 4)))
    assert model.last_window_plan.counts == [1, 1] and model.last_window_plan.next_row == [-1, -1]
    assert torch.equal(model.last_latent, lat) and torch.equal(model.last_window_latent, lat)
    got = model.last_ode_stats
    assert got["rows"] == stats["rows"] and got["evaluations"] == stats["evaluations"] and got["windows"] == [1, 1]
    for a, b, c in zip(plain.target + plain.residual, win.target + win.residual, keyword.target + keyword.residual):
        assert torch.equal(a, b) and torch.equal(a, c)
    if names is not None:
        ode = lambda d: {n: v for n, v in d.items() if "ode_" in n}   # noqa: E731
        assert ode(names) == ode(names0), "the solve's own kernels, the same number of times"
        assert any("ode_control" in n for n in names) and not any("window_blend" in n or "ode_control_groups" in n for n in names)


@functools.lru_cache(maxsize=None)
def _statement_case(preset):
    """inputs and the statement's result, once per session: clips of 29 and 17 frames, W = 16, O = 4 (3 + 2 window rows, the second
    clip's last window with O + 1 valid frames), text prompt plus anchors; longform_ref.separate stepped by the grouped restatement
    in float64"""
    cfg = preset_config(preset)
    sd = init_state_dict(cfg, seed=7)
    anchors = [[("+", _seconds(cfg, 10), _seconds(cfg, 20))], [("-", 0.0, _seconds(cfg, 3)), ("+", _seconds(cfg, 11), _seconds(cfg, 15))]]
    batch, text, tmask = _batch(cfg, (29, 17), anchors)
    noise = synthetic_noise(2, 29)
    stats = []
    keep = L.ode_ref.solve
    L.ode_ref.solve = ref.stepper((29, 17), 16, 4, 1, "dopri5", 1e-3, 1e-3, stats_out=stats)
    try:
        with torch.inference_mode():
            want = L.separate(sd, cfg, batch.audios, batch.sizes.long(), text, tmask, noise, 16, 4, anchors=anchors)
    finally:
        L.ode_ref.solve = keep
    return cfg, sd, anchors, noise, want, stats


@pytest.mark.parametrize("preset,prec", [("tiny", "fp32"), ("mini", "fp16x3")])
def test_windowed_adaptive_separate_matches_the_statement(gpu, preset, prec):
    """Whole separate(window_seconds=, step_control="clip") with dopri5 at rtol = atol = 1e-3 (scipy's initial step: the grouped
    initial-step norms are in the path): stitched latent, window rows and both waveforms within the project's 1e-3 of the statement;
    the step counts of the statement per clip; plain fp16 printed beside fp16x3."""
    cfg, sd, anchors, noise, want, ref_stats = _statement_case(preset)
    t_ref, r_ref, lat_ref, rows_ref = want
    errs = {}
    for p in ([prec, "fp16"] if prec == "fp16x3" else [prec]):
        batch, _, _ = _batch(cfg, (29, 17), anchors)
        model = _model(cfg, sd, p, gpu)
        res = model.separate(batch.to(gpu), noise=noise.to(gpu), ode_opt=ADAPTIVE, **_win(cfg, 16, 4))
        st = model.last_ode_stats
        lat = (model.last_latent.cpu() - lat_ref).abs().max().item()
        wav = max((a.cpu() - b).abs().max().item() for a, b in zip(res.target + res.residual, t_ref + r_ref))
        errs[p] = (lat, wav)
        print(f"windowed separate {preset} {p} dopri5 1e-3: latent {lat:.3e} wave {wav:.3e}; {st}; statement "
              f"{[(s['groups'][0]['accepted'], s['groups'][0]['rejected']) for s in ref_stats]} (|latent| <= {lat_ref.abs().max():.2f})")
        if p != prec:
            continue
        assert st["windows"] == [3, 2] and len(st["rows"]) == 2 and tuple(model.last_latent.shape) == (2, 29, 256)
        util.report(f"windowed adaptive separate {p} window rows", model.last_window_latent, rows_ref, 1e-3)
        util.report(f"windowed adaptive separate {p} latent", model.last_latent, lat_ref, 1e-3)
        assert [t.numel() for t in res.target] == [t.numel() for t in t_ref]
        for got, ref_w in zip(res.target + res.residual, t_ref + r_ref):
            util.report(f"windowed adaptive separate {p} waveform", got, ref_w, 1e-3)


def test_light_refusals_and_a_failed_group(gpu):
    """The C ABI: windows without groups still answer SAMAUDIO_ERR_STATE and leave the state untouched; samaudio_set_window_groups
    before samaudio_set_windows is refused (ERR_STATE), its arguments are checked (ERR_ARG), and a new prepare clears it (the solve is
    the per-row one again).  separate(): without the keyword windows and an adaptive method are a ValueError; a group that fails
    raises the RuntimeError naming clip and candidate, with last_window_latent / last_window_plan and the statistics set."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=13)
    x = _window_inputs((20, 11), 8, 2, seed=7)
    rows = x["noise"].shape[0]
    model = _model(cfg, sd, "fp32", gpu)
    lib = model._lib
    nxt = _dev(torch.tensor(x["next_row"], dtype=torch.int32), gpu)
    table = _dev(torch.tensor([(g[0], len(g), 1) for g in x["grp"]], dtype=torch.int32), gpu)
    owner = _dev(x["owner"].to(torch.uint8), gpu)
    params = ode_adaptive(ADAPTIVE)[1]
    stats = (hip.OdeRowStats * rows)()
    state = x["noise"].to(gpu).contiguous()

    def solve_c():
        return lib.samaudio_ode_solve_adaptive(model._ctx, hip.ptr(state), hip.ODE_DOPRI5, 0.0, 1.0, C.byref(params), stats,
                                               hip.current_stream_ptr())

    with pytest.raises(hip.SamAudioHipError, match="set_windows first"):   # never prepared
        hip.check(lib.samaudio_set_window_groups(model._ctx, hip.ptr(table), 2, hip.ptr(owner)))
    model._prepare(x["feats"], x["text"], x["tmask"], None, None, None, x["pad"])
    model._ensure_stages(hip.ODE_DOPRI5, rows, 8)
    with pytest.raises(hip.SamAudioHipError, match="set_windows first"):   # prepared, no windows
        hip.check(lib.samaudio_set_window_groups(model._ctx, hip.ptr(table), 2, hip.ptr(owner)))
    hip.check(lib.samaudio_set_windows(model._ctx, hip.ptr(nxt), rows, 2))
    with pytest.raises(hip.SamAudioHipError, match="windows are set"):     # windows without groups: as before
        hip.check(solve_c())
    assert torch.equal(state.cpu(), x["noise"])
    for n, mask, why in ((0, owner, "n_groups"), (rows + 1, owner, "n_groups"), (2, None, "ownership mask")):
        with pytest.raises(AssertionError, match=why):   # SAMAUDIO_ERR_ARG
            hip.check(lib.samaudio_set_window_groups(model._ctx, hip.ptr(table), n, None if mask is None else hip.ptr(mask)))
    hip.check(lib.samaudio_set_window_groups(model._ctx, hip.ptr(table), 2, hip.ptr(owner)))
    hip.check(lib.samaudio_set_window_groups(model._ctx, None, 0, None))   # cleared by itself
    with pytest.raises(hip.SamAudioHipError, match="windows are set"):
        hip.check(solve_c())
    hip.check(lib.samaudio_set_window_groups(model._ctx, hip.ptr(table), 2, hip.ptr(owner)))
    hip.check(lib.samaudio_set_windows(model._ctx, None, 0, 0))            # cleared with the windows
    with pytest.raises(hip.SamAudioHipError, match="set_windows first"):
        hip.check(lib.samaudio_set_window_groups(model._ctx, hip.ptr(table), 2, hip.ptr(owner)))
    hip.check(lib.samaudio_set_windows(model._ctx, hip.ptr(nxt), rows, 2))
    hip.check(lib.samaudio_set_window_groups(model._ctx, hip.ptr(table), 2, hip.ptr(owner)))
    model._prepare(x["feats"], x["text"], x["tmask"], None, None, None, x["pad"])   # a new prepare: windows and groups are gone
    per_row = model.solve(x["noise"].to(gpu), ADAPTIVE)
    assert len(model.last_ode_stats["rows"]) == rows and torch.isfinite(per_row).all()
    assert not torch.equal(per_row[0, 6:], per_row[1, :2]), "no blend, no groups: the rows are rows again"
    assert torch.equal(state.cpu(), x["noise"])

    batch, _, _ = _batch(cfg, (20, 11))
    noise = synthetic_noise(2, 20).to(gpu)
    with pytest.raises(ValueError, match="window_seconds"):
        model.separate(batch.to(gpu), noise=noise, ode_opt=ADAPTIVE, window_seconds=_seconds(cfg, 8), window_overlap_seconds=_seconds(cfg, 2))
    model.last_window_latent = model.last_window_plan = None
    with pytest.raises(RuntimeError, match=r"clip 0, candidate 0 stopped at t = .*looser rtol / atol"):
        model.separate(batch.to(gpu), noise=noise, ode_opt=dict(ADAPTIVE, options={"max_num_steps": 1}), **_win(cfg, 8, 2))
    st = model.last_ode_stats
    assert [r["status"] for r in st["rows"]] == ["max_num_steps"] * 2 and st["windows"] == [3, 2]
    assert model.last_window_plan.counts == [3, 2] and tuple(model.last_window_latent.shape) == (5, 8, 256)
    assert tuple(model.last_latent.shape) == (2, 20, 256) and torch.isfinite(model.last_latent).all()


def test_default_and_per_row_paths_launch_what_they_launched(gpu):
    """Without the keyword: a profiled default separate() and a per-row adaptive separate() launch no kernel of this feature, and the
    same kernels the same number of times before and after a grouped solve on the same model, with the same bits; the grouped solve
    launches ode_control_groups where the per-row one launches ode_control, as often, and window_blend once per evaluation."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=7)
    batch, _, _ = _batch(cfg, (29, 17))
    batch = batch.to(gpu)
    noise = synthetic_noise(2, 29).to(gpu)
    model = _model(cfg, sd, "fp32", gpu)
    opts = {"default": DFLT_ODE_OPT, "per row": ADAPTIVE}

    def run(opt, **kw):
        _, names = _profiled(model, gpu, lambda: model.separate(batch, noise=noise, ode_opt=opt, **kw))
        return model.last_latent.clone(), names, model.last_ode_stats if opt is ADAPTIVE else None

    before = {k: run(opt) for k, opt in opts.items()}
    _, grouped, gstats = run(ADAPTIVE, **_win(cfg, 16, 4))
    after = {k: run(opt) for k, opt in opts.items()}
    for k in opts:
        assert torch.equal(before[k][0], after[k][0]) and before[k][1] == after[k][1] and before[k][2] == after[k][2], k
    if grouped is None:
        return
    for k in opts:
        assert not any("ode_control_groups" in n or "window_blend" in n for n in before[k][1]), k
    assert "dit/ode_control" in before["per row"][1] and not any("ode_control" in n for n in before["default"][1])
    assert "dit/ode_control" not in grouped
    assert grouped["dit/ode_control_groups"] == grouped["dit/ode_commit"] + 3 and grouped["dit/window_blend"] == gstats["evaluations"]
