"""dopri5 / bosh3 with per-row step control (samaudio.h samaudio_ode_solve_adaptive) on the device.

The statement is tests/ode_adaptive_ref.py (pinned to scipy's RK45 / RK23 by tests/test_ode_adaptive_cpu.py; unpinned vs torchdiffeq).
Here: the four kernels through their hooks against float64 (bounds as tests/test_glue_kernels_gpu.py derives them: 8 x the error of
the same statement in float32 torch), the controller's decision table against the float32 restatement, the engine's loop against the
restatement over the field driven from the host, whole separate() against the oracle, the bitwise invariances the fixed-grid paths
keep, the tolerance order, the untouched default path and the error paths.  The tests named `light` run on the SIMT simulator as well
(tests/test_ode_adaptive_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import samaudio_oracle as O
from sam_audio_amd import SAMAudio, SAMAudioProcessor, hip, preset_config
from sam_audio_amd.model import DFLT_ODE_OPT, ode_adaptive
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
from tests import ode_adaptive_ref as ref
from tests import util
from tests.test_ode_methods_gpu import _check_separate, _model, _solve_inputs, _tiny_case
from tests.test_tower_kernels_gpu import NAN, _all_nan, _cmp, _dev, _lib, _mk, _nan, _ok, _same_bits

pytestmark = pytest.mark.gpu

CHUNK = 4096                                      # kernels.h kOdeChunk
FW = dict(t=0, h=1, t_new=2, h_abs=3, h_prev=4, err=5, d1=6, h0=7)                                # f32 words of a control block
IW = dict(status=8, accepted=9, rejected=10, step_rejected=11, accepted_now=12, n_valid=13)        # i32 words
RUN, FIN, UNDER, MAXS = 0, 1, 2, 3
METHOD = {"dopri5": hip.ODE_DOPRI5, "bosh3": hip.ODE_BOSH3}
NEW_KERNELS = ("ode_stage_rows", "ode_error", "ode_control", "ode_commit")


def _ctl(rows, **fields):
    """control blocks [rows, 16] f32 (the i32 words through a view); every field a per-row list"""
    f = torch.zeros(rows, hip.ODE_CTL_WORDS)
    i = f.view(torch.int32)
    for name, values in fields.items():
        (f if name in FW else i)[:, FW[name] if name in FW else IW[name]] = torch.tensor(values, dtype=f.dtype if name in FW else i.dtype)
    return f


def _sources(ks, coefs, gpu):
    """host arrays of seven pointers / weights; the slots behind n_src point to NaN with weight 1: never read"""
    poison = _nan(ks[0].shape, torch.float32, gpu)
    n = len(ks)
    ptrs = (C.c_void_p * 7)(*[ks[j].data_ptr() if j < n else poison.data_ptr() for j in range(7)])
    w = (C.c_float * 7)(*[coefs[j] if j < n else 1.0 for j in range(7)])
    return ptrs, w, poison


def _tableau_rows():
    """every (method, what, weights) combination the engine launches: the non-zero weights of each row of A, of B and of E"""
    out = []
    for m in ref.METHODS:
        A, B, _, E, S, _ = ref.tableau(m)
        for i in range(1, S):
            out.append((m, f"a{i}", [float(np.float32(a)) for a in A[i][:i] if a != 0]))
        out.append((m, "b", [float(np.float32(b)) for b in B if b != 0]))
        out.append((m, "e", [float(np.float32(e)) for e in E if e != 0]))
    return out


TABLEAU_ROWS = _tableau_rows()
assert sorted({len(w) for _, what, w in TABLEAU_ROWS if what != "e"}) == [1, 2, 3, 4, 5]


def _combo(ks, w, dtype):
    s = w[0] * ks[0].to(dtype)
    for c, k in zip(w[1:], ks[1:]):
        s = s + c * k.to(dtype)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# ode_stage_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,what,w", [r for r in TABLEAU_ROWS if r[1] != "e"], ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("frames", [5, 17])
def test_light_stage_rows_hook(gpu, method, what, w, frames):
    """out[r] = y[r] + h[r] (w0 k0 + ...) with every source count of both tableaux (1 .. 5), three rows with three steps; against float64.
    Then row 1 finished and row 2 failed with NaN all over their K: their output is their input bit for bit, row 0's is unchanged."""
    rows, n = 3, frames * 256
    y = _mk((rows + 1, n), 2100 + len(w))
    ks = [_mk((rows, n), 2110 + j) for j in range(len(w))]
    h = [0.3, 0.0171, 1.0]
    kd = [_dev(k, gpu) for k in ks]
    ptrs, coefs, _ = _sources(kd, w, gpu)
    yd, out = _dev(y, gpu), _nan((rows + 1, n), torch.float32, gpu)
    ctl = _dev(_ctl(rows, h=h), gpu)
    lib = _lib("fp32")
    _ok("fp32", lib.samaudio_op_ode_stage_rows(hip.ptr(yd), ptrs, coefs, len(w), hip.ptr(ctl), hip.ptr(out), rows, n, util.stream()))
    got = out.cpu()
    assert _all_nan(got[rows]), "the row behind the output was written"
    h32 = torch.tensor(h, dtype=torch.float32)[:, None]
    want = y[:rows].double() + h32.double() * _combo(ks, w, torch.float64)
    f32 = y[:rows] + h32 * _combo(ks, [float(c) for c in w], torch.float32)
    _cmp(f"ode_stage_rows {method} {what} frames={frames}", got[:rows], want, f32)
    for k in kd:
        k[1:] = NAN
    ctl2 = _dev(_ctl(rows, h=h, status=[RUN, FIN, UNDER]), gpu)
    out2 = _nan((rows + 1, n), torch.float32, gpu)
    _ok("fp32", lib.samaudio_op_ode_stage_rows(hip.ptr(yd), ptrs, coefs, len(w), hip.ptr(ctl2), hip.ptr(out2), rows, n, util.stream()))
    got2 = out2.cpu()
    assert _same_bits(got2[0], got[0]) and _same_bits(got2[1:rows], y[1:rows]) and _all_nan(got2[rows])


# ---------------------------------------------------------------------------------------------------------------------
# ode_error
# ---------------------------------------------------------------------------------------------------------------------
def _row_sums(partials):
    """the controller's sum: the chunks of a row in index order, in float32"""
    p = partials.cpu()
    s = torch.zeros(p.shape[0])
    for c in range(p.shape[1]):
        s = s + p[:, c]
    return s


def _error_launch(gpu, y, ynew, ks, w, h, status, mask, rtol, atol, frames):
    rows = y.shape[0]
    chunks = -(-frames * 256 // CHUNK)
    kd = [_dev(k, gpu) for k in ks]
    ptrs, coefs, _ = _sources(kd, w, gpu)
    part = _nan((rows + 1, chunks), torch.float32, gpu)
    ctl = _dev(_ctl(rows, h=h, status=status), gpu)
    yd, nd = _dev(y, gpu), _dev(ynew, gpu)
    md = None if mask is None else _dev(mask.to(torch.uint8), gpu)
    _ok("fp32", _lib("fp32").samaudio_op_ode_error(hip.ptr(yd), hip.ptr(nd), ptrs, coefs, len(w), hip.ptr(ctl),
                                                   None if md is None else hip.ptr(md), rtol, atol, 1, hip.ptr(part), rows, frames, 256,
                                                   util.stream()))
    p = part.cpu()
    assert _all_nan(p[rows]), "partials behind the last row were written"
    return p[:rows]


def _error_stmt(y, ynew, ks, w, h, mask, rtol, atol, dtype):
    est = _combo(ks, w, dtype) * torch.tensor(h, dtype=torch.float32).to(dtype)[:, None, None]
    scale = torch.tensor(atol, dtype=torch.float32).to(dtype) + \
        torch.tensor(rtol, dtype=torch.float32).to(dtype) * torch.maximum(y.to(dtype).abs(), ynew.to(dtype).abs())
    q = (est / scale) ** 2
    if mask is not None:
        q = q * mask.to(dtype)[:, :, None]
    return q.flatten(1).sum(1)


@pytest.mark.parametrize("method", ref.METHODS)
@pytest.mark.parametrize("frames,short", [(5, 4), (20, 17)])
def test_light_error_hook(gpu, method, frames, short):
    """The row's sum of squares of h K^T E / (atol + rtol max(|y|, |y_new|)) over its valid elements, with the estimator weights of
    the method: rows of valid length 1, `short` and `frames`, and the same rows with no mask; against float64.  frames = 5 is one chunk
    of 4096 elements with 1280 live; frames = 20, short = 17 is a valid prefix of 4352 elements that crosses exactly one chunk boundary
    and ends inside the second chunk.  The padding frames hold NaN in every K and in y_new: they never enter.  A finished row's partials
    are +0.  (The candidate itself is ode_stage_rows' combination with the weights b - the estimator's last term is the field AT the
    candidate, so it exists before this kernel runs - and is covered by test_light_stage_rows_hook's `b` cases.)"""
    w = [r for r in TABLEAU_ROWS if r[0] == method and r[1] == "e"][0][2]
    rows, rtol, atol = 3, 1e-3, 1e-4
    valid = [1, short, frames]
    mask = torch.arange(frames)[None, :] < torch.tensor(valid)[:, None]
    y = _mk((rows, frames, 256), 2200)
    ynew = y + 0.05 * _mk((rows, frames, 256), 2201)
    ks = [_mk((rows, frames, 256), 2210 + j, 1e-3) for j in range(len(w))]
    h = [0.25, 0.0625, 0.7]
    hole = ~mask[:, :, None].expand_as(y)
    ks_nan = [torch.where(hole, torch.full_like(k, NAN), k) for k in ks]
    got = _error_launch(gpu, y, torch.where(hole, torch.full_like(y, NAN), ynew), ks_nan, w, h, [RUN] * 3, mask, rtol, atol, frames)
    want = _error_stmt(y, ynew, ks, w, h, mask, rtol, atol, torch.float64)
    f32 = _error_stmt(y, ynew, ks, [float(c) for c in w], h, mask, rtol, atol, torch.float32)
    _cmp(f"ode_error {method} frames={frames} masked", _row_sums(got), want, f32)
    free = _error_launch(gpu, y, ynew, ks, w, h, [RUN] * 3, None, rtol, atol, frames)
    _cmp(f"ode_error {method} frames={frames} no mask", _row_sums(free), _error_stmt(y, ynew, ks, w, h, None, rtol, atol, torch.float64),
         _error_stmt(y, ynew, ks, [float(c) for c in w], h, None, rtol, atol, torch.float32))
    done = _error_launch(gpu, y, ynew, ks, w, h, [RUN, FIN, MAXS], mask, rtol, atol, frames)
    assert _same_bits(done[0], got[0]) and not done[1:].view(torch.int32).any(), "a row that has ended must leave +0 partials"


@pytest.mark.parametrize("frames,short", [(5, 4), (20, 17)])
def test_light_error_sum_is_the_rows_own(gpu, frames, short):
    """The bits of a row's sum depend on nothing but the row: launched alone, among other rows, as another row index, and in a batch
    padded to more frames (the extra frames masked out, holding NaN)."""
    w = [r for r in TABLEAU_ROWS if r[0] == "dopri5" and r[1] == "e"][0][2]
    rtol, atol = 1e-3, 1e-4
    row_y, row_n = _mk((1, frames, 256), 2300), _mk((1, frames, 256), 2301)
    row_k = [_mk((1, frames, 256), 2310 + j, 1e-3) for j in range(len(w))]
    mask1 = (torch.arange(frames) < short)[None]
    alone = _row_sums(_error_launch(gpu, row_y, row_n, row_k, w, [0.37], [RUN], mask1, rtol, atol, frames))

    def among(pad):
        T = frames + pad
        def widen(x, seed):
            full = _mk((3, T, 256), seed)
            full[:, frames:] = NAN
            full[1, :frames] = x[0]
            return full
        mask = torch.zeros(3, T, dtype=torch.bool)
        mask[0, :frames], mask[1, :short], mask[2, :1] = True, True, True
        p = _error_launch(gpu, widen(row_y, 2320), widen(row_n, 2321), [widen(k, 2330 + j) for j, k in enumerate(row_k)], w,
                          [0.9, 0.37, 0.01], [RUN] * 3, mask, rtol, atol, T)
        return _row_sums(p)[1:2]

    assert _same_bits(among(0), alone), "among other rows"
    assert _same_bits(among(3), alone), "in a batch padded by 3 frames"
    assert _same_bits(among(16), alone), "in a batch padded by a whole chunk"


# ---------------------------------------------------------------------------------------------------------------------
# ode_control, ode_commit
# ---------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


CASES = [   # name, row fields before the decision, err
    ("err 0: grows by ifactor", dict(t=0.125, h=0.0625), 0.0),
    ("err 0.5", dict(t=0.125, h=0.0625), 0.5),
    ("err just below 1", dict(t=0.125, h=0.0625), float(np.nextafter(np.float32(1), np.float32(0)))),
    ("err exactly 1: rejected", dict(t=0.125, h=0.0625), 1.0),
    ("err 4: rejected", dict(t=0.125, h=0.0625), 4.0),
    ("accept after a rejection: factor capped at 1", dict(t=0.25, h=0.03125, step_rejected=1, rejected=1), 0.01),
    ("the next step would pass t1: clipped", dict(t=0.875, h=0.0625), 0.001),
    ("the step ends at t1: finished", dict(t=0.96875, h=0.03125, t_new=1.0), 0.5),
    ("a finished row: untouched", dict(t=1.0, h=0.03125, status=FIN, accepted=9, rejected=2), 0.5),
    ("h below min_step after a rejection: failed", dict(t=0.5, h=1e-6), 1e6),
    ("max_num_steps reached", dict(t=0.125, h=0.0625, accepted=4, rejected=2), 0.5),
]


@pytest.mark.parametrize("method", ref.METHODS)
def test_light_control_decision_table(gpu, method):
    """One launch over the table above (n_valid = 4 and one chunk of 4 err^2, so the norm is err after an exact division), against the
    float32 restatement's Controller.  Integers are exact.  t and t_new are exact: sums and differences of h, contraction off.  h_abs,
    h and the stage times may differ in the last place where a factor went through powf (the device's powf and numpy's float32
    power are both faithful, not both correctly rounded): at most 1 ulp, and exact where no power is taken (err 0, the cap, the clip)."""
    S = ref.tableau(method)[4]
    Cn = [float(np.float32(c)) for c in ref.tableau(method)[2]] + [1.0]
    rows = len(CASES)
    F = np.float32
    ctl_ref = ref.Controller(method, F, 1.0, max_num_steps=7)
    fields = {k: [] for k in list(FW) + list(IW)}
    want = []
    for _, f, err in CASES:
        c = ctl_ref.new_row(0.0)
        c.t, c.h = F(f["t"]), F(f["h"])
        c.t_new = F(f.get("t_new", c.t + c.h))
        c.h_abs = c.h
        c.status, c.accepted, c.rejected = f.get("status", RUN), f.get("accepted", 3), f.get("rejected", 0)
        c.step_rejected = bool(f.get("step_rejected", 0))
        for k in FW:
            fields[k].append(float(getattr(c, k, 0.0)))
        for k in IW:
            fields[k].append(int(getattr(c, k, 4 if k == "n_valid" else 0)))
        ss = F(4) * F(err) * F(err)
        if c.status == RUN:
            c.took = ctl_ref.decide(c, np.sqrt(ss / F(4)))
        else:
            c.took = False
        want.append((c, ss))
    before = _ctl(rows, **fields)
    ctl = _dev(before, gpu)
    part = _dev(torch.tensor([[float(ss)] for _, ss in want]), gpu)
    times = _nan((S + 2, rows), torch.float32, gpu)
    active = torch.full((2,), -7, dtype=torch.int32, device=gpu)
    params = ode_adaptive({"method": method, "rtol": 1e-3, "atol": 1e-3, "options": {"max_num_steps": 7}})[1]
    _ok("fp32", _lib("fp32").samaudio_op_ode_control(hip.ptr(ctl), 3, METHOD[method], 0.0, 1.0, C.byref(params), hip.ptr(part), None, 1,
                                                     None, 5, 256, hip.ptr(times), hip.ptr(active), rows, util.stream()))
    got, tm = ctl.cpu(), times.cpu()
    gi = got.view(torch.int32)
    assert _all_nan(tm[S + 1]) and active.cpu().tolist() == [sum(c.status == RUN for c, _ in want), -7]
    for r, ((name, f, err), (c, _)) in enumerate(zip(CASES, want)):
        line = {k: got[r, FW[k]].item() for k in FW} | {k: gi[r, IW[k]].item() for k in IW}
        print(f"{method} {name}: {line}")
        if f.get("status", RUN) != RUN:
            assert _same_bits(got[r], before[r]), name
            continue
        assert (line["status"], line["accepted"], line["rejected"], line["step_rejected"], line["accepted_now"]) == \
            (c.status, c.accepted, c.rejected, int(c.step_rejected), int(c.took)), name
        assert line["t"] == float(c.t) and line["err"] == float(c.err), name
        power = err not in (0.0,) and not (c.took and f.get("step_rejected"))
        assert _ulps(line["h_abs"], c.h_abs) <= (1 if power else 0), name
        if c.status == RUN:
            assert _ulps(line["h"], c.h) <= 1 and _ulps(line["t_new"], c.t_new) <= 1, name
            for i in range(S + 1):
                assert _ulps(tm[i, r].item(), c.t + F(Cn[i]) * c.h) <= 1, (name, i)
        else:
            assert all(tm[i, r].item() == float(c.t) for i in range(S + 1)), name
    by = {name: (gi[r], got[r]) for r, (name, _, _) in enumerate(CASES)}
    assert by["the step ends at t1: finished"][0][IW["status"]] == FIN and by["the step ends at t1: finished"][1][FW["t"]] == 1.0
    clipped = by["the next step would pass t1: clipped"][1]
    assert clipped[FW["t_new"]] == 1.0 and clipped[FW["h"]] == 1.0 - 0.9375
    assert by["h below min_step after a rejection: failed"][0][IW["status"]] == UNDER
    assert by["max_num_steps reached"][0][IW["status"]] == MAXS
    assert by["accept after a rejection: factor capped at 1"][1][FW["h_abs"]] == 0.03125


def test_light_control_reset_and_commit(gpu):
    """mode 0: t = t0, counters 0, n_valid = valid frames x channels from the mask, the time table at t0; with first_step the first trial
    (clipped where it passes t1).  ode_commit: rows with accepted_now take y_new and K[last], the others keep every bit."""
    rows, frames = 3, 5
    mask = _dev((torch.arange(frames)[None, :] < torch.tensor([1, 4, 5])[:, None]).to(torch.uint8), gpu)
    ctl = _nan((rows, hip.ODE_CTL_WORDS), torch.float32, gpu)
    times = _nan((7, rows), torch.float32, gpu)
    active = torch.zeros(1, dtype=torch.int32, device=gpu)
    lib = _lib("fp32")
    for first, h in ((None, 0.0), (0.25, 0.25), (1.0, 0.75)):
        opt = {"method": "dopri5", "rtol": 1e-3, "atol": 1e-3, "options": {"first_step": first}}
        _ok("fp32", lib.samaudio_op_ode_control(hip.ptr(ctl), 0, hip.ODE_DOPRI5, 0.25, 1.0, C.byref(ode_adaptive(opt)[1]), None, None, 0,
                                                hip.ptr(mask), frames, 256, hip.ptr(times), hip.ptr(active), rows, util.stream()))
        got = ctl.cpu()
        gi = got.view(torch.int32)
        assert gi[:, IW["n_valid"]].tolist() == [256, 4 * 256, 5 * 256] and active.item() == rows
        assert not gi[:, [IW[k] for k in ("status", "accepted", "rejected", "step_rejected", "accepted_now")]].any()
        assert got[:, FW["t"]].tolist() == [0.25] * 3 and got[:, FW["h"]].tolist() == [h] * 3
        assert times.cpu()[0].tolist() == [0.25] * 3 and times.cpu()[6].tolist() == [0.25 + h] * 3
    n = frames * 256
    y, ynew, k0, k6 = (_mk((rows + 1, n), 2400 + j) for j in range(4))
    yd, nd, k0d, k6d = (_dev(x.clone(), gpu) for x in (y, ynew, k0, k6))
    cd = _dev(_ctl(rows, accepted_now=[1, 0, 1], status=[RUN, RUN, FIN]), gpu)
    _ok("fp32", lib.samaudio_op_ode_commit(hip.ptr(yd), hip.ptr(nd), hip.ptr(k0d), hip.ptr(k6d), hip.ptr(cd), rows, n, util.stream()))
    for got, old, new in ((yd.cpu(), y, ynew), (k0d.cpu(), k0, k6)):
        assert _same_bits(got[[0, 2]], new[[0, 2]]) and _same_bits(got[[1, 3]], old[[1, 3]])


# ---------------------------------------------------------------------------------------------------------------------
# the engine's loop against the restatement over the field driven from the host
# ---------------------------------------------------------------------------------------------------------------------
MARGIN = 1e-2
# case -> (seed of the inputs, gain on transformer.output.weight, options).  Searched with the oracle's CPU field and the reference runs
# alone.  `plain` is the model as it is initialised: its field is so smooth in t that at 1e-3 no trial is ever rejected (inputs seeds
# 0 .. 11 at 'tiny' and 0 .. 5 at 'mini': err <= 0.65 everywhere, dopri5 finishes in 2 steps), so no seed gives the rejection the loop
# has to be seen handling.  `pushed` is the same model with a 16 x stronger output projection and a first trial of the whole interval:
# 2 (dopri5) or 3 (bosh3) rejections per row, the second of dopri5's after a rejection in the same step.
CASES_ENGINE = {"plain": (3, 1.0, {}), "pushed": (4, 16.0, {"first_step": 1.0})}


@pytest.mark.parametrize("case", list(CASES_ENGINE))
@pytest.mark.parametrize("method", ref.METHODS)
def test_light_engine_loop_equals_the_restatement_over_the_host_driven_field(gpu, method, case):
    """model.solve against tests/ode_adaptive_ref.py over model.forward with per-row times, fp32, rtol = atol = 1e-3; 'mini', 2 rows x 40
    frames with row 1 padded to 31 valid frames on hardware ('tiny', 2 x 8 with 6 valid on the simulator).
    Condition, asserted on the two reference runs alone (float32 and float64 bookkeeping): no trial step of the float64 run has its
    err in [1 - m, 1 + m], m = 1e-2, the float32 run takes the same accept / reject sequence, and some row rejects at least once.  m:
    the estimate h K^T E is a difference of O(|K|) terms that cancel to O(tolerance x scale); each term carries float32 rounding
    eps |K|, so err is uncertain by about 7 eps |K| h / (atol + rtol |y|) = 7 x 6e-8 x 5 / 1e-3 = 2e-3 at |K| <= 5, h <= 1; 1e-2 leaves a
    factor of 5.
    Then: the engine's accepted / rejected per row and its evaluations equal the reference's, the rows' sequences differ, and the
    latent lies within 4 x the float32-vs-float64 reference difference of the float64 run (4: the engine's combination and
    reduction orders round independently of either reference's)."""
    sim = gpu.type != "cuda"
    cfg = preset_config("tiny" if sim else "mini")
    seed, gain, options = CASES_ENGINE[case]
    sd = init_state_dict(cfg, seed=41, with_codec=False)
    sd["transformer.output.weight"] = sd["transformer.output.weight"] * gain
    T, valid = (8, 6) if sim else (40, 31)
    feats, text, tmask, noise = _solve_inputs(2, T, 5, seed=seed)
    pad = torch.arange(T)[None, :] < torch.tensor([T, valid])[:, None]
    model = _model(cfg, sd, "fp32", gpu)

    def field(t, y):
        return model.forward(y.float(), feats, text, t.float(), text_mask=tmask, audio_pad_mask=pad).to(y.dtype)

    runs = {}
    for dtype in (torch.float64, torch.float32):
        runs[dtype] = ref.solve(field, noise.to(gpu), method, 1e-3, 1e-3, dtype=dtype, mask=pad.to(gpu), **options)
    (y64, s64), (y32, s32) = runs[torch.float64], runs[torch.float32]
    seq = lambda s: [[a for _, _, _, a in r["trials"]] for r in s["rows"]]   # noqa: E731
    errs = [e for r in s64["rows"] for _, _, e, _ in r["trials"]]
    print(f"{method}: float64 reference trials (t, h, err, accepted): {[r['trials'] for r in s64['rows']]}")
    assert all(r["status"] == "finished" for r in s64["rows"] + s32["rows"])
    assert not any(1 - MARGIN <= e <= 1 + MARGIN for e in errs), "an err of the float64 run lies inside the margin: pick another seed"
    assert seq(s64) == seq(s32) and s64["evaluations"] == s32["evaluations"]
    if case == "pushed":
        assert all(r["rejected"] >= 2 for r in s64["rows"]), "the pushed case is there for its rejections"
    assert s64["rows"][0]["ts"] != s64["rows"][1]["ts"], "the two rows were meant to step differently"

    model._prepare(feats, text, tmask, None, None, None, pad)
    got = model.solve(noise.to(gpu), {"method": method, "rtol": 1e-3, "atol": 1e-3, "options": options})
    st = model.last_ode_stats
    print(f"{method} {case}: engine {st}")
    assert [(r["accepted"], r["rejected"], r["status"], r["t"]) for r in st["rows"]] == \
        [(r["accepted"], r["rejected"], "finished", 1.0) for r in s64["rows"]]
    assert st["evaluations"] == s64["evaluations"]
    assert st["rows"][0]["last_h"] != st["rows"][1]["last_h"], "the two rows were meant to step differently"
    for r, want in zip(st["rows"], s32["rows"]):   # the float32 restatement's last step: the same bookkeeping up to the norm's rounding
        assert abs(r["last_h"] - want["last_h"]) <= 1e-3 * want["last_h"]
    spread = (y32.double() - y64).abs().max().item()
    err = (got.double() - y64).abs().max().item()
    print(f"{method} {case} engine vs float64 restatement: max-abs {err:.3e}; float32 vs float64 restatement {spread:.3e}; ratio "
          f"{err / spread:.2f} (bound 4); |latent| <= {y64.abs().max().item():.2f}")
    assert torch.isfinite(got).all() and err <= 4 * spread


# ---------------------------------------------------------------------------------------------------------------------
# whole separate() against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_adaptive(monkeypatch, sd, cfg, batch, text, tmask, noise, method, tol, anchors):
    T = noise.shape[1]
    mask = torch.arange(T)[None, :] < batch.sizes.long()[:, None]
    monkeypatch.setattr(O, "ode_fixed_grid", ref.oracle_stepper(method, tol, tol, mask=mask))
    with torch.inference_mode():
        return O.separate(sd, cfg, batch.audios, batch.sizes.long(), text, tmask, noise, anchors=anchors)


def test_separate_matches_oracle_fp32(gpu, monkeypatch):
    """Whole separate() at fp32, 'tiny' dims (ragged clips, anchors), dopri5 at rtol = atol = 1e-3: latent and both waveforms within
    the project's 1e-3 of the oracle stepped by the float64 restatement row by row."""
    cfg, sd, batch, text, tmask, anchors, noise = _tiny_case()
    want = _oracle_adaptive(monkeypatch, sd, cfg, batch, text, tmask, noise, "dopri5", 1e-3, anchors)
    model = _model(cfg, sd, "fp32", gpu)
    res = model.separate(batch.to(gpu), noise=noise.to(gpu), ode_opt={"method": "dopri5", "rtol": 1e-3, "atol": 1e-3})
    print(f"separate dopri5: {model.last_ode_stats}")
    _check_separate("separate dopri5", model, res, want, 1e-3)


def test_separate_fp16x3_matches_oracle(gpu, monkeypatch):
    """The default precision at 'mini' dims: dopri5 within 1e-3 of the oracle for latent and waveforms; plain fp16 printed beside it."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=8)
    hop = cfg.audio_codec.hop_length
    T = 25
    clips = [synthetic_clip(i, T * hop) for i in range(2)]
    text, tmask = synthetic_text_features(2, 8, ragged=True)
    anchors = [[("+", 0.04, 0.12)], [("-", 0.0, 0.08), ("+", 0.08, 0.16)]]
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x", "y"], audios=clips, anchors=anchors, text_features=text,
                                               text_mask=tmask)
    noise = synthetic_noise(2, T)
    t_ref, r_ref, lat_ref = _oracle_adaptive(monkeypatch, sd, cfg, batch, text, tmask, noise, "dopri5", 1e-3, anchors)
    errs = {}
    for p in ("fp16x3", "fp16"):
        model = _model(cfg, sd, p, gpu)
        res = model.separate(batch.to(gpu), noise=noise.to(gpu), ode_opt={"method": "dopri5", "rtol": 1e-3, "atol": 1e-3})
        lat = (model.last_latent.cpu() - lat_ref).abs().max().item()
        wav = max((a.cpu() - b).abs().max().item() for a, b in zip(res.target + res.residual, t_ref + r_ref))
        errs[p] = (lat, wav, model.last_ode_stats["evaluations"])
    print(f"separate 'mini' dopri5 1e-3: fp16x3 latent {errs['fp16x3'][0]:.3e} wave {errs['fp16x3'][1]:.3e} ({errs['fp16x3'][2]} "
          f"evaluations); fp16 latent {errs['fp16'][0]:.3e} wave {errs['fp16'][1]:.3e} ({errs['fp16'][2]} evaluations); |latent| <= "
          f"{lat_ref.abs().max():.2f}")
    assert errs["fp16x3"][0] < 1e-3 and errs["fp16x3"][1] < 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# bitwise invariances
# ---------------------------------------------------------------------------------------------------------------------
ADAPTIVE = {"method": "dopri5", "rtol": 1e-3, "atol": 1e-3}


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("method", ref.METHODS)
def test_a_batch_equals_its_rows_solved_alone_and_itself(gpu, prec, method):
    """Three rows of one padded frame count (one of them padded) in one solve = each row solved alone, bit for bit, although the rows
    take different numbers of steps (the short solves never ride along); and a repeated solve equals itself."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=14, with_codec=False)
    feats, text, tmask, noise = _solve_inputs(3, 12, 5, seed=8)
    noise[1] *= 0.25   # rows of different scale: different step sequences
    pad = torch.arange(12)[None, :] < torch.tensor([12, 12, 9])[:, None]
    model = _model(cfg, sd, prec, gpu)
    opt = dict(ADAPTIVE, method=method)

    def run(rows):
        model._prepare(feats[rows], text[rows], tmask[rows], None, None, None, pad[rows])
        out = model.solve(noise[rows].to(gpu), opt)
        return out, model.last_ode_stats

    whole, stats = run(slice(0, 3))
    again, stats2 = run(slice(0, 3))
    assert torch.equal(whole, again) and stats == stats2, "run-to-run determinism"
    counts = set()
    for r in range(3):
        alone, s1 = run(slice(r, r + 1))
        assert torch.equal(alone[0], whole[r]), f"row {r} alone differs from the batch"
        assert s1["rows"][0] == stats["rows"][r]
        counts.add((s1["rows"][0]["accepted"], s1["rows"][0]["rejected"], s1["rows"][0]["last_h"]))
    print(f"{prec} {method}: {stats}")
    assert torch.isfinite(whole).all() and len(counts) > 1


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_two_streams_are_bitwise_one_stream(gpu, prec):
    """SAMAudio(streams=2): each row group loops on its own context, stream and stage buffers - the latent equals the one-stream one."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=11)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 12 * hop) for i in range(5)]
    text, tmask = synthetic_text_features(5, 6, ragged=True)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * 5, audios=clips, text_features=text, text_mask=tmask).to(gpu)
    noise = synthetic_noise(5, 12).to(gpu)
    one = _model(cfg, sd, prec, gpu)
    one.separate(batch, noise=noise, ode_opt=ADAPTIVE)
    two = _model(cfg, sd, prec, gpu, streams=2)
    for rep in range(2):
        res = two.separate(batch, noise=noise, ode_opt=ADAPTIVE)
        torch.cuda.synchronize()
        assert torch.equal(two.last_latent, one.last_latent), f"repetition {rep}"
    assert two.last_ode_stats["rows"] == one.last_ode_stats["rows"] and len(two.last_ode_stats["rows"]) == 5
    assert two._stages is not None and two._lanes[0]._stages is not None
    assert all(torch.isfinite(w).all() for w in res.target)


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_candidates_equal_single_candidate_runs(gpu, prec):
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=9)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 4 * hop) for i in range(2)]
    text, tmask = synthetic_text_features(2, 4)
    proc = SAMAudioProcessor.from_config(cfg)
    noise = synthetic_noise(4, 4)
    model = _model(cfg, sd, prec, gpu)
    model.separate(proc(["x", "y"], clips, text_features=text, text_mask=tmask).to(gpu), noise=noise.to(gpu), ode_opt=ADAPTIVE,
                   reranking_candidates=2)
    lat2, rows2 = model.last_latent.clone(), model.last_ode_stats["rows"]
    model.separate(proc(["x", "y"], clips, text_features=text, text_mask=tmask).to(gpu), noise=noise[[0, 2]].to(gpu), ode_opt=ADAPTIVE)
    assert torch.equal(lat2[[0, 2]], model.last_latent)
    assert [rows2[0], rows2[2]] == model.last_ode_stats["rows"]


# ---------------------------------------------------------------------------------------------------------------------
# tolerance order, the default path, errors
# ---------------------------------------------------------------------------------------------------------------------
def test_tighter_tolerances_come_closer_to_a_fine_rk4(gpu):
    """'tiny' fp32: the distance to rk4 at step 1/64 does not grow, and the evaluations do not shrink, from 1e-2 to 1e-3 to 1e-4.
    No absolute bound: two correct solvers at one tolerance differ by O(tolerance).
    Two models.  `pushed` (the engine test's: output projection x 16) takes more steps at every tighter tolerance, and both orders are
    asserted in full.  On the model as initialised the evaluations are asserted in full as well, but the distance is NOT monotone from
    1e-2 to 1e-3, for either pair: both tolerances take the same number of steps (dopri5 2, bosh3 3; evaluations 14, 14, 20 and 11, 11,
    17), the tighter one only starts with a smaller first step and so ends with a LONGER last step, clipped to t1, whose error decides
    the distance.  MI355X: dopri5 2.861e-06, 4.530e-06, 1.907e-06 and bosh3 5.771e-04, 6.590e-04, 2.029e-04 on |latent| <= 3.89.
    That is the controller's, not the engine's: the float64 restatement over the oracle's CPU field shows the same rise (dopri5 steps
    0.19 + 0.81 at 1e-2 against 0.12 + 0.88 at 1e-3).  So on this model the consecutive order the solver does not have is printed, and
    what is asserted is 1e-4 (one or two steps more) against 1e-2: no farther from the fine solve, up to the rounding the fine solve
    itself carries - 64 steps, each adding half an ulp of max|latent| at worst."""
    cfg = preset_config("tiny")
    feats, text, tmask, noise = _solve_inputs(2, 8, 5, seed=3)
    for gain in (1.0, 16.0):
        sd = init_state_dict(cfg, seed=41, with_codec=False)
        sd["transformer.output.weight"] = sd["transformer.output.weight"] * gain
        model = _model(cfg, sd, "fp32", gpu)
        model._prepare(feats, text, tmask, None, None, None, None)
        fine = model.solve(noise.to(gpu), {"method": "rk4", "options": {"step_size": 1 / 64}})
        for method in ref.METHODS:
            dist, evals = [], []
            for tol in (1e-2, 1e-3, 1e-4):
                got = model.solve(noise.to(gpu), {"method": method, "rtol": tol, "atol": tol})
                dist.append((got - fine).abs().max().item())
                evals.append(model.last_ode_stats["evaluations"])
            print(f"gain {gain:g} {method} vs rk4 1/64 at tol 1e-2, 1e-3, 1e-4: distance {['%.3e' % d for d in dist]}, evaluations "
                  f"{evals} (|latent| <= {fine.abs().max().item():.2f})")
            assert evals[0] <= evals[1] <= evals[2]
            if gain != 1.0:
                assert dist[0] >= dist[1] >= dist[2]
            else:
                floor = 64 * 2.0 ** -24 * fine.abs().max().item()
                assert dist[2] <= max(dist[0], floor)


def test_default_paths_are_untouched(gpu):
    """A profiled default midpoint solve and an rk4 solve launch none of the new kernels, and the same kernels the same number of times
    as before (midpoint = rk4 minus its 32 ode_stage launches: the counts of test_default_midpoint_solve_has_no_stage_kernel); their
    latents are bit-equal before and after an adaptive solve on the same model, which does launch the new kernels."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=12, with_codec=False)
    feats, text, tmask, noise = _solve_inputs(2, 40, 5, seed=5)
    model = _model(cfg, sd, "fp16x3", gpu)
    opts = {"midpoint": DFLT_ODE_OPT, "rk4": {"method": "rk4", "options": {"step_size": 1 / 8}}}

    def profiled(opt):
        model._prepare(feats, text, tmask, None, None, None, None)
        model.profile_begin()
        out = model.solve(noise.to(gpu), opt)
        return out, {r["name"]: r["launches"] for r in model.profile_end()}

    before = {name: profiled(opt) for name, opt in opts.items()}
    _, adaptive = profiled(ADAPTIVE)
    trials = sum(model.last_ode_stats["rows"][0][k] for k in ("accepted", "rejected"))
    assert all(any(k in n for n in adaptive) for k in NEW_KERNELS)
    assert adaptive["dit/ode_commit"] >= trials and adaptive["dit/ode_control"] == adaptive["dit/ode_commit"] + 3
    after = {name: profiled(opt) for name, opt in opts.items()}
    for name in opts:
        assert torch.equal(before[name][0], after[name][0]), name
        assert before[name][1] == after[name][1], name
        assert not any(k in n for n in before[name][1] for k in NEW_KERNELS), name
    rk4 = dict(before["rk4"][1])
    assert rk4.pop("dit/ode_stage") == 32 and rk4 == before["midpoint"][1]


def test_light_error_paths(gpu):
    """max_num_steps = 1: RuntimeError naming a row, its status in last_ode_stats.  Missing or small stage buffers: SAMAUDIO_ERR_WORKSPACE
    with the state untouched.  The new method ids handed to samaudio_ode_solve: SAMAUDIO_ERR_ARG.  Nothing here faults the device."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=13, with_codec=False)
    feats, text, tmask, noise = _solve_inputs(2, 4, 3, seed=7)
    model = _model(cfg, sd, "fp32", gpu)
    lib = model._lib
    model._prepare(feats, text, tmask, None, None, None, None)
    with pytest.raises(RuntimeError, match=r"row 0 stopped at t = .*looser rtol / atol"):
        model.solve(noise.to(gpu), dict(ADAPTIVE, options={"max_num_steps": 1}))
    rows = model.last_ode_stats["rows"]
    assert [r["status"] for r in rows] == ["max_num_steps"] * 2 and all(r["accepted"] + r["rejected"] == 1 and r["t"] < 1 for r in rows)
    reached = model.last_latent   # the state the rows reached is kept for the caller: one accepted step away from the noise
    assert reached.shape == noise.shape and torch.isfinite(reached).all()
    assert all((reached[r].cpu() != noise[r]).any() == (rows[r]["accepted"] == 1) for r in range(2))
    state = noise.to(gpu).contiguous()
    params = ode_adaptive(ADAPTIVE)[1]
    stats = (hip.OdeRowStats * 2)()
    state_bytes = 2 * 4 * 256 * 4
    for method, arrays in ((hip.ODE_DOPRI5, 8), (hip.ODE_BOSH3, 5)):
        need = lib.samaudio_ode_stage_bytes(model._ctx, method, 2, 4)
        assert arrays * state_bytes < need <= arrays * state_bytes + 8 * 256
        buf = torch.empty(need, dtype=torch.uint8, device=gpu)
        for ptr, nbytes in ((None, 0), (C.c_void_p((buf.data_ptr() + 255) // 256 * 256), need - 256)):
            hip.check(lib.samaudio_set_ode_stages(model._ctx, ptr, nbytes))
            with pytest.raises(hip.SamAudioHipError, match="stage buffers"):
                hip.check(lib.samaudio_ode_solve_adaptive(model._ctx, hip.ptr(state), method, 0.0, 1.0, C.byref(params), stats,
                                                          hip.current_stream_ptr()))
        grid = (C.c_float * 2)(0.0, 1.0)
        with pytest.raises(AssertionError, match="unsupported method"):   # SAMAUDIO_ERR_ARG
            hip.check(lib.samaudio_ode_solve(model._ctx, hip.ptr(state), method, grid, 2, hip.current_stream_ptr()))
    assert torch.equal(state.cpu(), noise)
