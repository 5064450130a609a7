"""Whole-path bitwise invariances of the compensated precisions "fp16x3" / "bf16x3" (whole-vs-shard and
1-vs-2-stream results are bitwise equal; shards are concatenated, never reconciled).

The kernels of an x3 model are pinned one by one against float64 elsewhere (tests/test_x3_gpu.py, test_x3_gemm_forms_gpu.py,
test_layer_kernels_gpu.py, test_codec_forms_gpu.py).  Here: the HOST-SIDE decisions above them, which pick a kernel, a tile, a launch
split or a scratch buffer from the number of rows of a call - gemm8x (256 x 256) <-> gemm8s (128 x 128) <-> the tail split (gemm.hip
gemm_variant / gemm_tail_split), split3 into the x3a / x3u scratch, the SwiGLU epilogue that writes w2's split operand where
x3_w2_pre says so, self_attn_x3_kernel, cross_attn_probs3 / cross_attn_fold3, the ".x3" / ".fly" weight twins in both layouts, the
codec's FLY and X3 / X3Block launches.  tests/test_path_gpu.py states the same invariances for the plain 16-bit modes, which take other
code in every one of these.

Every assertion is torch.equal on fp32 latents and waveforms (plus isfinite): there is no tolerance in this file.  Where the profile
records exist (hipEvents: hardware only) each test also shows that the two sides of an equality really ran different kernels.
"""
import os

import pytest
import torch

from oracle import samaudio_oracle as O
from sam_audio_amd import SAMAudio, SAMAudioProcessor, hip, preset_config
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
X3 = ["bf16x3"] if SIM else ["fp16x3", "bf16x3"]
HUGE = 1 << 30


def _model(cfg, sd, prec, gpu, **kw):
    m = SAMAudio(cfg, precision=prec, device=str(gpu), **kw)
    m.load_state_dict(sd, strict=False)
    return m


def _set(prec, flags):
    for k, v in flags.items():
        hip.lib(hip.operands_for(prec)).samaudio_debug_set_flag(k, v)


def _names(model, gpu, fn):
    """fn() bracketed by the per-kernel profile records: (result, {record name: launches}); no records off hardware (hipEvents)"""
    if gpu.type != "cuda":
        return fn(), None
    model.profile_begin()
    out = fn()
    return out, {r["name"]: r["launches"] for r in model.profile_end()}


def _is256(n):   # an x3 launch of the 256 x 256 8-phase kernel
    return "256x256" in n and n.endswith("_x3")


def _is128(n):   # ... of the 128 x 128 kernel on its own (not as the tail of a split launch)
    return "gemm8s" in n and n.endswith("_x3") and "_tail" not in n


def _launches(names, pred):
    return sum(v for k, v in names.items() if pred(k))


def _same(a, b):
    return torch.equal(a, b) and bool(torch.isfinite(a).all())


# ------------------------------------------------------------------------- (a) shards, where the policy changes kernel
def _wide_case(gpu, rows=16):
    """Reference-default width (D = 2048, F = 5504; 2 layers keep it quick), 10 s of frames, ragged text mask, ragged clip lengths and
    anchors on some rows: what _prepare takes, every item with the batch in front."""
    cfg = preset_config("default", transformer=dict(n_layers=2))
    sd = init_state_dict(cfg, seed=10, device=gpu, with_codec=False)
    T, Lt = 250, 8
    g = torch.Generator().manual_seed(4)
    z = torch.randn(rows, T, 128, generator=g)
    text = torch.randn(rows, Lt, 768, generator=g)
    tmask = torch.ones(rows, Lt, dtype=torch.bool)
    pad = torch.ones(rows, T, dtype=torch.bool)
    kinds = [[], [("+", 1.0, 2.5)], [("-", 0.0, 0.8), ("+", 3.0, 3.1)]]
    anchors = []
    for b in range(rows):   # row 0, the 1-row shard: 7 tokens, 227 frames, one anchor
        if (b + 1) % 4:
            tmask[b, Lt - (b + 1) % 4:] = False        # 7, 6, 5, 8 tokens
        if (b + 1) % 3:
            pad[b, T - 23 * ((b + 1) % 3):] = False    # 227, 204, 250 frames
        anchors.append(kinds[(b + 1) % 3])
    ids, align = O.anchors_to_ids(anchors, pad, cfg.audio_codec.hop_length, cfg.audio_codec.sample_rate)
    cond = dict(feats=torch.cat([z, z], 2), text=text, tmask=tmask, ids=ids, align=align, pad=pad)
    return cfg, sd, cond, synthetic_noise(rows, T)


def _solve(model, gpu, cond, noise, rows, opt={"method": "midpoint", "options": {"step_size": 0.5}}):
    c = {k: v[rows] for k, v in cond.items()}
    model._prepare(c["feats"], c["text"], c["tmask"], None, c["ids"], c["align"], c["pad"])
    return model.solve(noise[rows].to(gpu), opt).clone()


@pytest.mark.skipif(SIM, reason="D = 2048 at 4000 rows: hardware only")
@pytest.mark.parametrize("prec", X3)
def test_shard_invariance_where_the_policy_changes_kernel(gpu, prec):
    """cat(shards of 1, 3 and 12 rows) == the 16-row batch, bit for bit, at row counts chosen from gemm_variant (the 256 x 256 kernel
    from 128 tiles) and gemm_tail_split:

        rows  M      qkv (N = 6144)               w13 (N = 11008)                  N = D classes
        16    4000   384 tiles: 256 + 128 tail    688 tiles, one 256 x 256 launch  128 tiles, 256 x 256
        12    3000   288 tiles: 256 + 32 tail     516 tiles (rem 4: no split)      128 x 128
         3     750   128 x 128                    129 tiles, 256 x 256             128 x 128
         1     250   128 x 128                    128 x 128                        128 x 128

    and a model that has only ever seen the 1-row shard gives that shard's bits too (nothing of the larger call's split scratch is
    read).  The profile records show the two sides ran different kernels."""
    cfg, sd, cond, noise = _wide_case(gpu)
    model = _model(cfg, sd, prec, gpu)
    whole, names16 = _names(model, gpu, lambda: _solve(model, gpu, cond, noise, slice(0, 16)))
    again = _solve(model, gpu, cond, noise, slice(0, 16))
    assert _same(whole, again), "run-to-run determinism"
    one, names1 = _names(model, gpu, lambda: _solve(model, gpu, cond, noise, slice(0, 1)))
    three, names3 = _names(model, gpu, lambda: _solve(model, gpu, cond, noise, slice(1, 4)))
    twelve, names12 = _names(model, gpu, lambda: _solve(model, gpu, cond, noise, slice(4, 16)))
    print(f"{prec} 16 rows: {sorted(names16)}\n{prec} 12 rows: {sorted(names12)}\n{prec} 3 rows: {sorted(names3)}\n"
          f"{prec} 1 row: {sorted(names1)}")
    # the condition of the comparison: the whole batch ran the 256 x 256 kernel and a split launch's tail, the 1-row shard neither
    assert any(_is256(n) for n in names16) and any("_tail" in n and n.endswith("_x3") for n in names16), sorted(names16)
    assert not any("256x256" in n or "_tail" in n for n in names1), sorted(names1)
    assert any(_is128(n) for n in names1), sorted(names1)
    assert any(_is256(n) for n in names3) and not any("_tail" in n for n in names3), sorted(names3)   # w13 alone: 129 tiles
    assert any("_tail" in n for n in names12), sorted(names12)
    for name, got, rows in (("1", one, slice(0, 1)), ("3", three, slice(1, 4)), ("12", twelve, slice(4, 16))):
        d = (got - whole[rows]).abs()
        assert torch.equal(got, whole[rows]), (f"the {name}-row shard differs from its rows of the 16-row batch: max |diff| "
                                               f"{d.max().item():.3e}, {int((d > 0).sum())} of {d.numel()} elements")
    assert torch.equal(whole, torch.cat([one, three, twelve]))
    fresh = _model(cfg, sd, prec, gpu)
    assert _same(_solve(fresh, gpu, cond, noise, slice(0, 1)), one), "a model that only ever saw the 1-row shard"


@pytest.mark.skipif(SIM, reason="D = 2048 at 4000 rows: hardware only")
@pytest.mark.parametrize("prec", X3)
def test_launch_form_flags_that_need_many_tiles(gpu, prec):
    """The launch-form flags that cannot change anything at 'mini' dims, at the width and row counts of the shard test: the tail floor
    (DBG_TAIL_SPLIT_MIN = 1 splits w13 at 12 rows: 516 tiles = 2 x 256 + 4, below the shipped floor of 8), one workgroup per tile
    instead of the persistent walk (DBG_GEMM8_NOT_PERSISTENT: w13 at 16 rows is 688 tiles on 256 workgroups), 128 x 128 tiles
    everywhere (DBG_GEMM8_MIN_TILES huge) and 256 x 256 wherever N allows on ONE row (DBG_GEMM8_MIN_TILES = 1)."""
    cfg, sd, cond, noise = _wide_case(gpu)
    model = _model(cfg, sd, prec, gpu)
    base, seen = {}, {}
    for rows in (slice(0, 16), slice(4, 16), slice(0, 1)):
        base[rows.stop - rows.start], seen[rows.stop - rows.start] = _names(model, gpu, lambda: _solve(model, gpu, cond, noise, rows))
    tail = lambda names: _launches(names, lambda n: "_tail" in n)       # noqa: E731
    big = lambda names: _launches(names, _is256)                        # noqa: E731
    cases = (("tail floor 1, 12 rows", {hip.DBG_TAIL_SPLIT_MIN: 1}, slice(4, 16), lambda n, b: tail(n) > tail(b)),
             # (same kernel names either way: the record shows the launch the flag acts on, a 256 x 256 x3 launch of > 256 tiles, ran)
             ("one workgroup per tile, 16 rows", {hip.DBG_GEMM8_NOT_PERSISTENT: 1}, slice(0, 16), lambda n, b: big(n) == big(b) > 0),
             ("128 x 128 everywhere, 16 rows", {hip.DBG_GEMM8_MIN_TILES: HUGE}, slice(0, 16), lambda n, b: big(b) > 0 and big(n) == 0 and tail(n) == 0),
             ("256 x 256 wherever N allows, 1 row", {hip.DBG_GEMM8_MIN_TILES: 1}, slice(0, 1), lambda n, b: big(b) == 0 and big(n) > 0))
    for what, flags, rows, changed in cases:
        try:
            _set(prec, flags)
            got, names = _names(model, gpu, lambda: _solve(model, gpu, cond, noise, rows))
        finally:
            _set(prec, {k: 0 for k in flags})
        r = rows.stop - rows.start
        print(f"{prec} {what}: {sorted(names.items())}")
        assert changed(names, seen[r]), (what, sorted(names.items()), sorted(seen[r].items()))
        assert _same(got, base[r]), what


# ------------------------------------------------------------------------------------------- (b) one stream vs two
@pytest.mark.skipif(SIM, reason="the dry run has no streams")
@pytest.mark.parametrize("prec", X3)
def test_two_streams_equal_one_stream_latents_and_waveforms(gpu, prec):
    """SAMAudio(streams=2): two row groups on two engine contexts / HIP streams from two host threads, each decoding its own rows -
    the whole separate(), codec included, against the one-stream model: latent, targets and residuals bit for bit, twice."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=11)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 12 * hop) for i in range(5)]
    text, tmask = synthetic_text_features(5, 6, ragged=True)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * 5, audios=clips, text_features=text, text_mask=tmask).to(gpu)
    noise = synthetic_noise(5, 12).to(gpu)
    opt = {"method": "midpoint", "options": {"step_size": 0.25}}
    one = _model(cfg, sd, prec, gpu)
    want = one.separate(batch, noise=noise, ode_opt=opt)
    ref = one.last_latent.clone()
    assert torch.isfinite(ref).all()
    two = _model(cfg, sd, prec, gpu, streams=2)
    for rep in range(2):
        res = two.separate(batch, noise=noise, ode_opt=opt)
        torch.cuda.synchronize()
        if not torch.equal(two.last_latent, ref):   # say where
            d = (two.last_latent.float() - ref.float()).abs()
            per_clip = d.flatten(1).max(dim=1).values.tolist()
            raise AssertionError(f"two-stream latent differs from the one-stream one in repetition {rep}: max |diff| per clip "
                                 f"{per_clip}, {int((d > 0).sum())} of {d.numel()} elements, "
                                 f"finite={bool(torch.isfinite(two.last_latent).all())}")
        for kind, got_w, want_w in (("target", res.target, want.target), ("residual", res.residual, want.residual)):
            assert len(got_w) == len(want_w) == 5
            for i, (a, b) in enumerate(zip(got_w, want_w)):
                assert _same(a, b), f"{kind} waveform of clip {i} differs in repetition {rep}: max |diff| {(a - b).abs().max().item():.3e}"


# ------------------------------------------------------------------------------------------- (c) layout and prefetch
@pytest.mark.parametrize("prec", X3)
def test_twin_layout_and_prefetch_option_are_bitwise_invisible(gpu, prec):
    """weight_layout of an x3 model is the layout of the ".x3" twins (K-tile-major [K' / 64][N][64] | row-major [N, K']): the same
    accumulation order either way.  prefetch_rows is carried through the matrix of tests/test_path_gpu.py as well: an fp32 context
    never prefetches, so the option must change nothing.  One stream and two row groups."""
    cfg = preset_config("mini")
    sd = init_state_dict(cfg, seed=12)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 12 * hop) for i in range(3)]
    text, tmask = synthetic_text_features(3, 6, ragged=True)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * 3, audios=clips, text_features=text, text_mask=tmask).to(gpu)
    noise = synthetic_noise(3, 12).to(gpu)
    opt = {"method": "midpoint", "options": {"step_size": 0.5}}
    lat = {}
    for streams in (1,) if SIM else (1, 2):
        for layout in ("rows", "ktm"):
            for pf in (0, 1 << 20):
                m = _model(cfg, sd, prec, gpu, weight_layout=layout, prefetch_rows=pf, streams=streams)
                w3 = m.engine_tensors()["L0.wqkv.x3"]
                assert w3.dim() == (3 if layout == "ktm" else 2) and w3.dtype == hip.half_dtype(prec), (layout, w3.shape)
                assert m.engine_tensors()["L0.wqkv"].dim() == 2
                res = m.separate(batch, noise=noise, ode_opt=opt)
                lat[(layout, pf, streams)] = (m.last_latent.clone(), [w.clone() for w in res.target + res.residual])
    ref = lat[("rows", 0, 1)]
    assert torch.isfinite(ref[0]).all()
    for key, (v, wavs) in lat.items():
        assert torch.equal(ref[0], v), key
        assert all(_same(a, b) for a, b in zip(ref[1], wavs)), key


# ------------------------------------------------------------------------- (d) launch-form flags across the whole path
@pytest.mark.parametrize("prec", X3)
def test_launch_form_flags_leave_the_latent_bit_identical(gpu, prec):
    """Each launch-form debug flag alone against all flags at 0, 'mini' dims ('tiny' on the simulator), 3 rows of 40 frames (M = 120),
    ragged text: tile size
    (DBG_GEMM8_MIN_TILES = 1: 256 x 256 wherever N allows; huge: 128 x 128 everywhere - at these dims what the policy picks anyway,
    so its other side is the MIN_TILES = 1 run), the wave roles of the pipelined 128 x 128 kernel, the epilogue forms (GENERAL also
    makes x3_w2_pre refuse the split-form SwiGLU output: w2 then splits its operand with the stand-alone kernel, into x3u).
    Not here: DBG_TAIL_SPLIT_MIN and DBG_GEMM8_NOT_PERSISTENT need launches of more than 256 tiles (the test above);
    DBG_FOLD_PER_LAYER has no effect in an x3 context (the fold on compensated operands is one launch for all layers, whatever the
    flag; without class CWO an fp32 context does not fold); DBG_X3_PLAIN_WALK legitimately changes bits (tests/test_x3_gpu.py)."""
    cfg = preset_config("tiny" if SIM else "mini")   # (the simulator: D = 256, 2 layers - the same launch forms at a sixth of the work)
    sd = init_state_dict(cfg, seed=16, with_codec=False)
    B, T, Lt = 3, 40, 5
    g = torch.Generator().manual_seed(6)
    z = torch.randn(B, T, 128, generator=g)
    feats, text = torch.cat([z, z], 2), torch.randn(B, Lt, 768, generator=g)
    tmask = torch.ones(B, Lt, dtype=torch.bool)
    tmask[2, 2:] = False
    noise = synthetic_noise(B, T).to(gpu)
    # (the simulator: one evaluation of the field per flag instead of four - the same launches, once)
    opt = {"method": "euler", "options": {"step_size": 1.0}} if SIM else {"method": "midpoint", "options": {"step_size": 0.5}}
    model = _model(cfg, sd, prec, gpu)

    def run():
        model._prepare(feats, text, tmask, None, None, None, None)
        return model.solve(noise, opt).clone()

    base, seen = _names(model, gpu, run)
    assert torch.isfinite(base).all()
    big = lambda names: _launches(names, _is256)                                # noqa: E731
    small = lambda names: _launches(names, _is128)                              # noqa: E731
    split = lambda names: _launches(names, lambda n: n.endswith("/split3"))     # noqa: E731
    acts_on_128 = lambda n, b: small(n) == small(b) > 0 and big(n) == 0         # noqa: E731  (same names: the launches the flag acts on ran)
    cases = [("256 x 256 wherever N allows", {hip.DBG_GEMM8_MIN_TILES: 1}, lambda n, b: big(b) == 0 and big(n) > 0 and small(n) < small(b)),
             ("128 x 128 everywhere", {hip.DBG_GEMM8_MIN_TILES: HUGE}, lambda n, b: big(n) == 0 and small(n) == small(b) > 0)]
    cases += [(f"roles {v}", {hip.DBG_GEMM8S_ROLES: v}, acts_on_128) for v in (hip.DBG_ROLES_NONE, hip.DBG_ROLES_PROD0, hip.DBG_ROLES_PROD2)]
    cases += [("general epilogue", {hip.DBG_GEMM8_EPILOGUE: hip.DBG_EPI_GENERAL}, lambda n, b: split(n) > split(b)),
              ("register epilogue", {hip.DBG_GEMM8_EPILOGUE: hip.DBG_EPI_LINEAR}, acts_on_128),
              ("LDS-staged epilogue", {hip.DBG_GEMM8_EPILOGUE: hip.DBG_EPI_ROWS}, acts_on_128)]
    failed = []
    for what, flags, changed in cases:
        try:
            _set(prec, flags)
            got, names = _names(model, gpu, run)
        finally:
            _set(prec, {k: 0 for k in flags})
        if names is not None:
            print(f"{prec} {what}: x3 launches 256x256 {big(names)} (flags 0: {big(seen)}), 128x128 {small(names)} ({small(seen)}), "
                  f"split3 {split(names)} ({split(seen)})")
            assert changed(names, seen), (what, sorted(names.items()), sorted(seen.items()))
        if not _same(got, base):
            d = (got - base).abs()
            failed.append(f"{what}: max |diff| {d.max().item():.3e}, {int((d > 0).sum())} of {d.numel()} elements")
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------- (e) codec
@pytest.mark.parametrize("dec", ["32", "16"])
@pytest.mark.parametrize("prec", X3)
def test_codec_chunking_and_residual_unit_forms_in_an_x3_context(gpu, prec, dec, monkeypatch):
    """The DAC-VAE of an x3 model (encoder and, with codec_decode "32", decoder: FLY launches on operands split in registers and the
    wide convolutions' X3 / X3Block launches on ".x3" twins; codec_decode "16": the decoder on a 16-bit context of its own) passes its
    items in chunks of what the workspace holds: 5 waveforms and 5 latents with SAMAUDIO_CODEC_CHUNK 16, 2 and 1, and the (target,
    residual) pairs of separate() at 2 and 16 - the same bits.  codec_decode "16": the three forms of a residual unit as well."""
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=6)
    hop = cfg.audio_codec.hop_length
    wav = torch.stack([synthetic_clip(i, 2 * hop) for i in range(5)])
    lat = torch.randn(5, 2, 128, generator=torch.Generator().manual_seed(3))
    clips = [synthetic_clip(i, 3 * hop) for i in range(3)]
    text, tmask = synthetic_text_features(3, 4, ragged=True)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * 3, audios=clips, text_features=text, text_mask=tmask).to(gpu)
    noise = synthetic_noise(3, 3).to(gpu)
    opt = {"method": "euler", "options": {"step_size": 0.5}}
    model = _model(cfg, sd, prec, gpu, codec_decode=dec)
    outs = {}
    for chunk in ("16", "2", "1"):
        monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", chunk)
        model._workspace = None
        outs[chunk] = [model.encode_audio(wav).clone(), model.decode_audio(lat).clone()]
        if chunk != "1":
            model._workspace = None
            res = model.separate(batch, noise=noise, ode_opt=opt)
            outs[chunk] += [model.last_latent.clone()] + [w.clone() for w in res.target + res.residual]
    assert all(torch.isfinite(t).all() for t in outs["16"]) and len(outs["16"]) == 9
    for chunk in ("2", "1"):
        for i, (a, b) in enumerate(zip(outs["16"], outs[chunk])):
            assert torch.equal(a, b), f"chunk {chunk} against 16: output {i} (encode, decode, latent, 3 targets, 3 residuals) differs"
    monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", "16")
    model._workspace = None
    if dec != "16":
        return
    TWO, FUSE, WS = hip.DBG_RESUNIT_TWO_LAUNCHES, hip.DBG_RESUNIT_FUSE_ALWAYS, hip.DBG_RESUNIT_WS
    forms = {}
    try:
        for name, flags in (("two", {TWO: 1, FUSE: 0, WS: 0}), ("fused", {TWO: 0, FUSE: 1, WS: hip.DBG_WS_NEVER}),
                            ("ws", {TWO: 0, FUSE: 1, WS: hip.DBG_WS_ALWAYS_GRID3})):
            _set(prec, flags)
            forms[name], ran = _names(model, gpu, lambda: model.decode_audio(lat).clone())
            if ran is not None:   # the per-kernel records say which form ran
                assert any("resunit" in r for r in ran) == (name != "two"), sorted(ran)
    finally:
        _set(prec, {TWO: 0, FUSE: 0, WS: 0})
    for name in ("fused", "ws"):
        assert _same(forms["two"], forms[name]), name
    assert torch.equal(forms["two"], outs["16"][1])


# -------------------------------------------------------------------------------------------------- (f) candidates
@pytest.mark.parametrize("prec", X3)
def test_candidates_repeat_is_sample_major_in_the_x3_modes(gpu, prec):
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=9)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 4 * hop) for i in range(2)]
    text, tmask = synthetic_text_features(2, 4)
    proc = SAMAudioProcessor.from_config(cfg)
    noise = synthetic_noise(4, 4)
    model = _model(cfg, sd, prec, gpu)
    opt = {"method": "euler", "options": {"step_size": 0.5}}
    model.separate(proc(["x", "y"], clips, text_features=text, text_mask=tmask).to(gpu), noise=noise.to(gpu),
                   ode_opt=opt, reranking_candidates=2)
    lat2 = model.last_latent.clone()
    # rows (0,1) belong to clip 0, rows (2,3) to clip 1: compare with single-candidate runs on the same noise rows
    model.separate(proc(["x", "y"], clips, text_features=text, text_mask=tmask).to(gpu), noise=noise[[0, 2]].to(gpu),
                   ode_opt=opt)
    assert _same(lat2[[0, 2]], model.last_latent)
    assert not torch.equal(lat2[[1, 3]], model.last_latent)   # the other candidates had other noise


# ------------------------------------------------------------------------------------------------------ (g) reload
@pytest.mark.parametrize("first_classes", ["auto", "w13,w2"])
@pytest.mark.parametrize("prec", X3)
def test_second_load_state_dict_replaces_every_twin(gpu, prec, first_classes):
    """A second load_state_dict replaces every weight AND every 16-bit twin made from it (".x3" of the layers, the patcher and the
    codec's wide convolutions, ".fly" of its narrow ones): the model then equals a fresh one loaded with the second checkpoint, bit
    for bit, latents and waveforms.  `first_classes` "w13,w2": checkpoint A was loaded with those two classes on compensated operands
    only, then the model is switched to all of them and loads B - twins that did not exist under A must be made from B."""
    cfg = preset_config("tiny")
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 4 * hop) for i in range(3)]
    text, tmask = synthetic_text_features(3, 4)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * 3, audios=clips, text_features=text, text_mask=tmask).to(gpu)
    noise = synthetic_noise(3, 4).to(gpu)
    sd_a, sd_b = init_state_dict(cfg, seed=21), init_state_dict(cfg, seed=22)
    fresh = _model(cfg, sd_b, prec, gpu)
    want = fresh.separate(batch, noise=noise)
    want_lat = fresh.last_latent.clone()
    assert torch.isfinite(want_lat).all()
    twice = SAMAudio(cfg, precision=prec, device=str(gpu), streams=1 if SIM else 2, x3_classes=first_classes)   # (dry run: no streams)
    twice.load_state_dict(sd_a, strict=False)
    first = twice.separate(batch, noise=noise)
    assert not torch.equal(twice.last_latent, want_lat)
    assert all(torch.isfinite(w).all() for w in first.target)
    if first_classes != "auto":
        twice.x3_classes = hip.CLS_X3_DEFAULT   # what x3_classes="auto" means; the engine learns it with the weights it needs
    twice.load_state_dict(sd_b, strict=False)
    if first_classes != "auto":
        twice._set_precision_options(twice._ctx)
    got = twice.separate(batch, noise=noise)
    assert torch.equal(twice.last_latent, want_lat), f"latent: max |diff| {(twice.last_latent - want_lat).abs().max().item():.3e}"
    for a, b in zip(got.target + got.residual, want.target + want.residual):
        assert _same(a, b)
