"""rk4 / heun3 and custom time grids in separate() (samaudio.h SAMAUDIO_ODE_RK4 / _HEUN3).

The oracle is oracle.samaudio_oracle.separate with its ODE stepper replaced by the restatement of torchdiffeq's steppers in
tests/ode_ref.py (monkeypatched: encode, field, candidates and decode of the oracle are reused unchanged).  The engine's own stepping
is also held against the same field driven from the host, the Runge-Kutta path against the bitwise invariances the midpoint path
keeps (streams, candidates, sharding), and the default midpoint solve against any change of its launches.  The tests whose docstring
starts with "light" run on the SIMT simulator as well (tests/test_ode_methods_cpu.py)."""
import ctypes as C

import pytest
import torch

from oracle import samaudio_oracle as O
from sam_audio_amd import SAMAudio, SAMAudioProcessor, hip, preset_config
from sam_audio_amd.model import DFLT_ODE_OPT
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
from tests import ode_ref, util

pytestmark = pytest.mark.gpu


def _model(cfg, sd, prec, gpu, **kw):
    m = SAMAudio(cfg, precision=prec, device=str(gpu), **kw)
    m.load_state_dict(sd, strict=False)
    return m


def _tiny_case():
    """the inputs of test_path_gpu.py::test_separate_matches_oracle_fp32: ragged clips and text mask, anchors"""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=7)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(0, 6 * hop), synthetic_clip(1, 4 * hop + 100)]
    text, tmask = synthetic_text_features(2, 5, ragged=True)
    anchors = [[("+", 0.04, 0.12)], [("-", 0.0, 0.08), ("+", 0.08, 0.16)]]
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x", "y"], audios=clips, anchors=anchors, text_features=text,
                                               text_mask=tmask)
    return cfg, sd, batch, text, tmask, anchors, synthetic_noise(2, 6)


def _oracle_separate(monkeypatch, sd, cfg, batch, text, tmask, noise, method, grid=None, step_size=2 / 32, **kw):
    monkeypatch.setattr(O, "ode_fixed_grid", ode_ref.oracle_stepper(grid))
    with torch.inference_mode():
        return O.separate(sd, cfg, batch.audios, batch.sizes.long(), text, tmask, noise, method=method, step_size=step_size, **kw)


def _check_separate(name, model, res, ref, tol):
    t_ref, r_ref, lat_ref = ref
    util.report(f"{name} latent", model.last_latent, lat_ref, tol)
    assert [t.numel() for t in res.target] == [t.numel() for t in t_ref]
    for got, want in zip(res.target + res.residual, t_ref + r_ref):
        util.report(f"{name} waveform", got, want, tol)


def _solve_inputs(B, T, Lt, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, T, 128, generator=g)
    feats, text = torch.cat([z, z], 2), torch.randn(B, Lt, 768, generator=g)
    tmask = torch.ones(B, Lt, dtype=torch.bool)
    tmask[-1, Lt // 2:] = False
    return feats, text, tmask, synthetic_noise(B, T, seed=seed)


# ------------------------------------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize("method", ["rk4", "heun3"])
def test_separate_matches_oracle_fp32(gpu, monkeypatch, method):
    """Whole separate() at fp32, 'tiny' dims, step 1/4: latent and both waveforms within 1e-3 of the restated stepper."""
    cfg, sd, batch, text, tmask, anchors, noise = _tiny_case()
    ref = _oracle_separate(monkeypatch, sd, cfg, batch, text, tmask, noise, method, step_size=1 / 4, anchors=anchors)
    model = _model(cfg, sd, "fp32", gpu)
    res = model.separate(batch.to(gpu), noise=noise.to(gpu), ode_opt={"method": method, "options": {"step_size": 1 / 4}})
    _check_separate(f"separate {method}", model, res, ref, 1e-3)


@pytest.mark.parametrize("method", ["rk4", "heun3"])
def test_engine_stepping_equals_the_field_driven_from_the_host(gpu, method):
    """light.  model.solve against a loop of model.forward calls combined with the torchdiffeq formulas in torch on the device, fp32: the
    same field evaluations, so only the rounding of the combination may differ - a wrong node time or weight fails.  'mini' dims and
    step 1/4 on hardware; 'tiny' and two steps on the simulator."""
    sim = gpu.type != "cuda"
    cfg = preset_config("tiny" if sim else "mini")
    sd = init_state_dict(cfg, seed=41, with_codec=False)
    feats, text, tmask, noise = _solve_inputs(2, 8 if sim else 40, 5, seed=3)
    step = 0.5 if sim else 0.25
    model = _model(cfg, sd, "fp32", gpu)

    def field(t, y):
        return model.forward(y, feats, text, t.reshape(1), text_mask=tmask)

    want = ode_ref.solve(field, noise.to(gpu), method, ode_ref.step_grid(step))
    model._prepare(feats, text, tmask, None, None, None, None)
    got = model.solve(noise.to(gpu), {"method": method, "options": {"step_size": step}})
    err = (got - want).abs().max().item()
    print(f"{method} engine vs host-driven field: max-abs {err:.3e} (|latent| <= {want.abs().max().item():.2f})")
    assert torch.isfinite(got).all() and err <= 1e-5


def test_rk4_fp16x3_matches_oracle(gpu, monkeypatch):
    """The default precision at 'mini' dims: rk4 within 1e-3 of the oracle for latent and waveforms; the plain fp16 error beside it."""
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
    opt = {"method": "rk4", "options": {"step_size": 1 / 8}}
    t_ref, r_ref, lat_ref = _oracle_separate(monkeypatch, sd, cfg, batch, text, tmask, noise, "rk4", step_size=1 / 8,
                                             anchors=anchors)
    errs = {}
    for p in ("fp16x3", "fp16"):
        model = _model(cfg, sd, p, gpu)
        res = model.separate(batch.to(gpu), noise=noise.to(gpu), ode_opt=opt)
        lat = (model.last_latent.cpu() - lat_ref).abs().max().item()
        wav = max((a.cpu() - b).abs().max().item() for a, b in zip(res.target + res.residual, t_ref + r_ref))
        errs[p] = (lat, wav)
    print(f"separate 'mini' rk4 8 steps: fp16x3 latent {errs['fp16x3'][0]:.3e} wave {errs['fp16x3'][1]:.3e}; "
          f"fp16 latent {errs['fp16'][0]:.3e} wave {errs['fp16'][1]:.3e} (|latent| <= {lat_ref.abs().max():.2f})")
    assert errs["fp16x3"][0] < 1e-3 and errs["fp16x3"][1] < 1e-3


@pytest.mark.parametrize("method,options,grid", [
    ("midpoint", "constructor", [0.0, 0.1, 0.3, 0.6, 1.0]),
    ("rk4", "constructor", [0.0, 0.1, 0.3, 0.6, 1.0]),
    ("euler", None, [0.0, 1.0]),
    ("rk4", None, [0.0, 1.0]),
])
def test_custom_grids_match_oracle(gpu, monkeypatch, method, options, grid):
    """A non-uniform grid through grid_constructor (which sees the whole batch's noise and t = [0, 1] on the model device), and no
    options (torchdiffeq's default grid: one step over [0, 1]), fp32 'tiny' against the oracle on the same grid."""
    cfg, sd, batch, text, tmask, anchors, noise = _tiny_case()
    ref = _oracle_separate(monkeypatch, sd, cfg, batch, text, tmask, noise, method, grid=grid, anchors=anchors)
    seen = []

    def constructor(func, y0, t):
        seen.append((tuple(y0.shape), t.device, t.tolist()))
        return torch.tensor(grid, device=t.device)

    opt = {"method": method} if options is None else {"method": method, "options": {"grid_constructor": constructor}}
    model = _model(cfg, sd, "fp32", gpu)
    res = model.separate(batch.to(gpu), noise=noise.to(gpu), ode_opt=opt)
    _check_separate(f"separate {method} grid {grid}", model, res, ref, 1e-3)
    if options is not None:
        assert seen == [((2, 6, 256), model.last_latent.device, [0.0, 1.0])]


# ------------------------------------------------------------------------------------------------ bitwise invariances
@pytest.mark.parametrize("prec", ["bf16", "fp16x3"])
def test_rk4_two_streams_are_bitwise_one_stream(gpu, prec):
    """SAMAudio(streams=2): each row group on its own context, with its own stage buffers - the latent equals the one-stream one."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=11)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 12 * hop) for i in range(5)]
    text, tmask = synthetic_text_features(5, 6, ragged=True)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * 5, audios=clips, text_features=text, text_mask=tmask).to(gpu)
    noise = synthetic_noise(5, 12).to(gpu)
    opt = {"method": "rk4", "options": {"step_size": 0.5}}
    one = _model(cfg, sd, prec, gpu)
    one.separate(batch, noise=noise, ode_opt=opt)
    two = _model(cfg, sd, prec, gpu, streams=2)
    for rep in range(2):
        res = two.separate(batch, noise=noise, ode_opt=opt)
        torch.cuda.synchronize()
        assert torch.equal(two.last_latent, one.last_latent), f"repetition {rep}"
    assert two._stages is not None and two._lanes[0]._stages is not None
    assert two._stages.data_ptr() != two._lanes[0]._stages.data_ptr()
    assert all(torch.isfinite(w).all() for w in res.target)


def test_rk4_candidates_equal_single_candidate_runs(gpu):
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=9)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 4 * hop) for i in range(2)]
    text, tmask = synthetic_text_features(2, 4)
    proc = SAMAudioProcessor.from_config(cfg)
    noise = synthetic_noise(4, 4)
    model = _model(cfg, sd, "fp32", gpu)
    opt = {"method": "rk4", "options": {"step_size": 0.5}}
    model.separate(proc(["x", "y"], clips, text_features=text, text_mask=tmask).to(gpu), noise=noise.to(gpu), ode_opt=opt,
                   reranking_candidates=2)
    lat2 = model.last_latent.clone()
    # rows (0,1) belong to clip 0, rows (2,3) to clip 1: compare with single-candidate runs on the same noise rows
    model.separate(proc(["x", "y"], clips, text_features=text, text_mask=tmask).to(gpu), noise=noise[[0, 2]].to(gpu), ode_opt=opt)
    assert torch.equal(lat2[[0, 2]], model.last_latent)


def test_rk4_batch_sharding_is_bitwise_invariant_at_full_width(gpu):
    """concat(shard outputs) == whole-batch output at the reference's default width (2 layers) and 10 s clips, bf16."""
    cfg = preset_config("default", transformer=dict(n_layers=2))
    sd = init_state_dict(cfg, seed=10, device=gpu, with_codec=False)
    B, T = 4, 250
    g = torch.Generator().manual_seed(4)
    z = torch.randn(B, T, 128, generator=g)
    feats, text = torch.cat([z, z], 2), torch.randn(B, 8, 768, generator=g)
    noise = synthetic_noise(B, T)
    model = _model(cfg, sd, "bf16", gpu)
    opt = {"method": "rk4", "options": {"step_size": 0.5}}

    def run(rows):
        model._prepare(feats[rows], text[rows], None, None, None, None, None)
        return model.solve(noise[rows].to(gpu), opt)

    whole = run(slice(0, 4))
    assert torch.equal(whole, run(slice(0, 4))), "run-to-run determinism"
    assert torch.equal(whole, torch.cat([run(slice(0, 1)), run(slice(1, 4))])), "batch sharding changed the result"
    assert torch.isfinite(whole).all()


# ------------------------------------------------------------------------------------------------ the midpoint path and errors
def test_default_midpoint_solve_has_no_stage_kernel(gpu):
    """A profiled default solve (midpoint, step 1/16: 32 evaluations) launches no ode_stage_kernel and allocates no stage buffer; rk4
    at step 1/8 (also 32 evaluations) runs the same kernels the same number of times plus one ode_stage launch per evaluation."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=12, with_codec=False)
    feats, text, tmask, noise = _solve_inputs(2, 40, 5, seed=5)
    model = _model(cfg, sd, "fp16x3", gpu)
    recs = {}
    for name, opt in (("midpoint", DFLT_ODE_OPT), ("rk4", {"method": "rk4", "options": {"step_size": 1 / 8}})):
        model._prepare(feats, text, tmask, None, None, None, None)
        model.solve(noise.to(gpu), opt)   # warm-up: first-use allocations stay out of the profile
        if name == "midpoint":
            assert model._stages is None
        model.profile_begin()
        model.solve(noise.to(gpu), opt)
        recs[name] = {r["name"]: r for r in model.profile_end()}
    stage = recs["rk4"].pop("dit/ode_stage")
    assert not any("ode_stage" in n for n in recs["midpoint"])
    assert stage["launches"] == 32
    assert {n: r["launches"] for n, r in recs["midpoint"].items()} == {n: r["launches"] for n, r in recs["rk4"].items()}
    total = sum(r["ms"] for r in recs["rk4"].values()) + stage["ms"]
    print(f"ode_stage_kernel: {stage['ms']:.3f} ms over 32 launches of a {total:.1f} ms rk4 solve ('mini', 2 x 40 frames)")


def test_grid_longer_than_the_time_table_fails_cleanly(gpu):
    """light.  rk4 needs 4 table entries per step: 1025 steps do not fit the 4096 evaluation times - refused by the host with a
    ValueError and, handed to the engine directly, by samaudio_ode_solve (SAMAUDIO_ERR_ARG) before anything is launched."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=13, with_codec=False)
    feats, text, tmask, noise = _solve_inputs(1, 4, 3, seed=6)
    model = _model(cfg, sd, "fp32", gpu)
    model._prepare(feats, text, tmask, None, None, None, None)
    with pytest.raises(ValueError, match="time table"):
        model.solve(noise.to(gpu), {"method": "rk4", "options": {"step_size": 1 / 1025}})
    state = noise.to(gpu).contiguous()
    n_grid = 1026
    grid = (C.c_float * n_grid)(*[k / (n_grid - 1) for k in range(n_grid)])
    with pytest.raises(AssertionError, match="bad grid"):   # SAMAUDIO_ERR_ARG
        hip.check(model._lib.samaudio_ode_solve(model._ctx, hip.ptr(state), hip.ODE_RK4, grid, n_grid, hip.current_stream_ptr()))
    assert torch.equal(state.cpu(), noise)


def test_missing_or_small_stage_buffer_is_a_workspace_error(gpu):
    """light.  The stage buffers are the caller's: a Runge-Kutta solve without them (or with too few bytes) is refused with
    SAMAUDIO_ERR_WORKSPACE and leaves the state alone; euler and midpoint need none."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=13, with_codec=False)
    feats, text, tmask, noise = _solve_inputs(2, 4, 3, seed=7)
    model = _model(cfg, sd, "fp32", gpu)
    lib = model._lib
    assert lib.samaudio_ode_stage_bytes(model._ctx, hip.ODE_MIDPOINT, 2, 4) == 0
    assert lib.samaudio_ode_stage_bytes(model._ctx, hip.ODE_EULER, 2, 4) == 0
    assert lib.samaudio_ode_stage_bytes(model._ctx, hip.ODE_RK4, 2, 4) == 4 * 2 * 4 * 256 * 4
    assert lib.samaudio_ode_stage_bytes(model._ctx, hip.ODE_HEUN3, 2, 4) == 3 * 2 * 4 * 256 * 4
    model._prepare(feats, text, tmask, None, None, None, None)
    state = noise.to(gpu).contiguous()
    grid = (C.c_float * 3)(0.0, 0.5, 1.0)
    short = lib.samaudio_ode_stage_bytes(model._ctx, hip.ODE_RK4, 2, 4) - 256
    buf = torch.empty(short + 256, dtype=torch.uint8, device=gpu)
    for ptr, nbytes in ((None, 0), (C.c_void_p((buf.data_ptr() + 255) // 256 * 256), short)):
        hip.check(lib.samaudio_set_ode_stages(model._ctx, ptr, nbytes))
        with pytest.raises(hip.SamAudioHipError, match="stage buffers"):
            hip.check(lib.samaudio_ode_solve(model._ctx, hip.ptr(state), hip.ODE_RK4, grid, 3, hip.current_stream_ptr()))
    assert torch.equal(state.cpu(), noise)
