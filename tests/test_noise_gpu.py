"""separate(seed=...): noise_rows_kernel through samaudio_op_noise / noise.seeded_noise against the float64 statement of
tests/noise_ref.py, its bitwise properties (a value depends on seed, clip id, candidate, frame and channel
and on nothing else), its refusals, and SAMAudio.separate(seed=) at 'tiny' dims: whole batch, shards, two streams, windows, an
adaptive solve - each bit for bit the call that is handed the same tensor as `noise=`.

The tests named test_light_* make sense on the SIMT simulator as well (tests/test_noise_cpu.py runs them there).

Error bound of the op, from the number formats: e32 = the largest difference between the numpy float32 evaluation of the statement
and its float64 evaluation over the 2^20 values of (seed 1234, clip 0, candidate 0, 4096 x 256) - what fp32 arithmetic with
correctly working logf / sqrtf / cosf / sinf costs; computed here, 1.63e-6 - times 4 for the device's functions differing from the
host's by a few ulp each.  One wrong bit of Philox moves a value by O(1), so the bound cannot hide one.
MI355X: the largest error over all cases is 1.788e-06 ([1, 2049, 1024]; 1.603e-06 on the 2^20 set, where numpy float32 has 1.631e-06)
against the bound 6.526e-06 (profiles/seeded_noise/gpu_tests.log)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from sam_audio_amd import SAMAudio, SAMAudioProcessor, hip, preset_config
from sam_audio_amd.dist import shard_batch
from sam_audio_amd.noise import seeded_noise
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_text_features
from tests import noise_ref as R
from tests import util

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""

IDS = (0, 1, 2 ** 32, 2 ** 63 - 1)
SEEDS = (0, 1, 2 ** 32, 2 ** 64 - 1)
N_STAT = (4096, 256)   # the 2^20-value set of the statistics and of e32


@functools.lru_cache(maxsize=None)
def _stat_set():
    """the statement on (seed 1234, clip 0, candidate 0), float64 and float32, and its three neighbours: computed once"""
    z64 = R.stream(1234, 0, 0, *N_STAT)
    z32 = R.stream(1234, 0, 0, *N_STAT, dtype=np.float32)
    others = {"clip": R.stream(1234, 1, 0, *N_STAT), "candidate": R.stream(1234, 0, 1, *N_STAT), "seed": R.stream(1235, 0, 0, *N_STAT)}
    return z64, float(np.abs(z32.astype(np.float64) - z64).max()), others


def _bound():
    e32 = _stat_set()[1]
    assert 0 < 4 * e32 < 1e-5, e32
    return 4 * e32


def _check(name, got, seed, ids, cand, frames, channels):
    want = R.noise(seed, ids, cand, frames, channels)
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"{name}: max-abs err vs float64 {err:.3e} (bound {_bound():.3e}, max |z| {np.abs(want).max():.3f})")
    assert err <= _bound(), f"{name}: {err} > {_bound()}"
    return err


# ------------------------------------------------------------------------------------------------ 1. the op against the statement
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 3, 5, 260), (3, 2, 8, 256)], ids=lambda s: "x".join(map(str, s)))
def test_light_op_matches_float64(gpu, shape):
    """a single quad | Q = 65: no power of two, a tail block | the engine's width; every clip id of IDS (rotated to `clips` distinct
    ones) under every seed of SEEDS"""
    clips, cand, frames, channels = shape
    for seed in SEEDS:
        for r in range(len(IDS)):
            ids = [IDS[(r + b) % len(IDS)] for b in range(clips)]
            got = seeded_noise(seed, ids, cand, frames, channels, gpu)
            _check(f"noise {shape} seed {seed:#x} ids {[hex(i) for i in ids]}", got, seed, ids, cand, frames, channels)


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_light_op_more_clips_than_one_argument_pack(gpu, seed):
    """hip.NOISE_PACK_CLIPS + 6 clips: a second launch whose output starts behind the first pack's rows; the ids span both words"""
    clips = hip.NOISE_PACK_CLIPS + 6
    ids = [IDS[b % 4] + 3 * (b // 4) * (1 if b % 4 < 3 else -1) for b in range(clips)]
    assert len(set(ids)) == clips and min(ids) == 0 and max(ids) == 2 ** 63 - 1
    _check(f"noise {clips} clips seed {seed:#x}", seeded_noise(seed, ids, 2, 3, 8, gpu), seed, ids, 2, 3, 8)


@pytest.mark.skipif(SIM, reason="half a million lanes: hardware only")
def test_op_beyond_one_pass_of_the_capped_grid(gpu):
    """hip.NOISE_GRID_CAP blocks of 256 lanes cover cap * 256 quads in one pass: one frame more, and the first 256 lanes walk a second"""
    channels = 1024
    frames = hip.NOISE_GRID_CAP * 256 // (channels // 4) + 1
    assert frames * (channels // 4) == hip.NOISE_GRID_CAP * 256 + 256
    got = seeded_noise(2 ** 64 - 1, [2 ** 63 - 1], 1, frames, channels, gpu)
    _check(f"noise [1, {frames}, {channels}]", got, 2 ** 64 - 1, [2 ** 63 - 1], 1, frames, channels)


# ------------------------------------------------------------------------------------------------ 2. bitwise properties
def test_light_op_depends_on_nothing_but_seed_id_candidate_frame_channel(gpu):
    seed = 2 ** 40 + 9
    a = seeded_noise(seed, [5, 9], 4, 12, 256, gpu)
    assert torch.equal(a, seeded_noise(seed, [5, 9], 4, 12, 256, gpu)), "two calls"
    assert torch.equal(a[:, :8], seeded_noise(seed, [5, 9], 4, 8, 256, gpu)), "a longer call extends a shorter one"
    one = seeded_noise(seed, [5, 9], 1, 12, 256, gpu)
    assert torch.equal(a[0::4], one), "candidate 0 of 4 is the only candidate of 1"
    five, nine = seeded_noise(seed, [5], 4, 12, 256, gpu), seeded_noise(seed, [9], 4, 12, 256, gpu)
    assert torch.equal(a, torch.cat([five, nine])), "a clip's rows do not depend on the batch around it"
    assert torch.equal(seeded_noise(seed, [9, 5], 4, 12, 256, gpu), torch.cat([nine, five]))
    flat = a.reshape(8, -1)
    assert len({tuple(r[:8].tolist()) for r in flat.cpu()}) == 8, "eight (clip, candidate) streams, all different"
    assert not torch.equal(a, seeded_noise(seed + 1, [5, 9], 4, 12, 256, gpu))


def test_light_op_fills_a_view_and_nothing_else(gpu):
    """out= a view 16 bytes into a NaN-filled buffer: every element outside stays NaN, the inside is the plain call"""
    shape = (2 * 3, 5, 260)
    n = math.prod(shape)
    buf = torch.full((n + 8,), float("nan")).to(gpu)
    assert buf.data_ptr() % 16 == 0
    out = buf[4:4 + n].view(shape)
    got = seeded_noise(77, [3, 4], 3, 5, 260, gpu, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.isnan(buf[:4]).all() and torch.isnan(buf[4 + n:]).all()
    assert torch.equal(out, seeded_noise(77, [3, 4], 3, 5, 260, gpu)) and torch.isfinite(out).all()
    with pytest.raises(ValueError, match="aligned"):   # 4 bytes in: refused before the library is asked
        seeded_noise(77, [3, 4], 3, 5, 260, gpu, out=buf[1:1 + n].view(shape))


@pytest.mark.skipif(SIM, reason="2^20 values: hardware only")
def test_statistics_of_the_gpu_draw(gpu):
    """the 5-sigma conditions of tests/test_noise_cpu.py on the device's own 2^20 values (row 0 of one launch over two clips and two
    candidates, 4 MB a row), beside the device's own neighbours in clip, candidate and seed"""
    z = seeded_noise(1234, [0, 1], 2, *N_STAT, gpu).cpu().numpy()
    other_seed = seeded_noise(1235, [0], 1, *N_STAT, gpu).cpu().numpy()[0]
    fig = R.check_statistics(z[0], {"clip": z[2], "candidate": z[1], "seed": other_seed})
    print("gpu draw:", {k: f"{float(v):.3e}" for k, v in fig.items()})
    err = float(np.abs(z[0].astype(np.float64) - _stat_set()[0]).max())
    print(f"gpu draw vs float64 on the 2^20 set: {err:.3e} (numpy float32: {_stat_set()[1]:.3e})")
    assert err <= _bound()


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_light_refusals_leave_the_output_alone(gpu):
    """every SAMAUDIO_ERR_ARG of samaudio_op_noise, before any launch; then the Python surface's ValueErrors"""
    lib = hip.lib()
    out = torch.full((2 * 2 * 4 * 8 + 4,), 7.0).to(gpu)
    keep = out.clone()
    ids = (C.c_int64 * 2)(3, 4)
    neg = (C.c_int64 * 2)(3, -1)

    def call(o=out, clips=2, cand=2, frames=4, channels=8, seed=1, ids=ids):
        return lib.samaudio_op_noise(None if o is None else C.c_void_p(o.data_ptr()), clips, cand, frames, channels, seed, ids,
                                     util.stream())

    for kw, why in ((dict(o=None), "null"), (dict(ids=None), "null"), (dict(o=out[1:]), "aligned"), (dict(clips=0), "< 1"),
                    (dict(cand=0), "< 1"), (dict(frames=0), "< 1"), (dict(channels=6), "channels"), (dict(channels=0), "channels"),
                    (dict(channels=2), "channels"), (dict(frames=2 ** 31 - 1, channels=12), "2\\^32"), (dict(ids=neg), "negative")):
        with pytest.raises(AssertionError, match=why):   # SAMAUDIO_ERR_ARG
            hip.check(call(**kw))
    assert torch.equal(out, keep)
    hip.check(call())
    assert torch.equal(out[:128].view(4, 4, 8), seeded_noise(1, [3, 4], 2, 4, 8, gpu)) and torch.equal(out[128:], keep[128:])
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(clip_ids=[-1]), dict(clip_ids=[2 ** 63]), dict(clip_ids=[]),
               dict(candidates=0), dict(frames=0), dict(channels=6), dict(frames=2 ** 31 + 1, channels=8)):
        args = dict(seed=1, clip_ids=[0], candidates=1, frames=2, channels=8, device=gpu)
        args.update(kw)
        with pytest.raises(ValueError):
            seeded_noise(**args)


# ------------------------------------------------------------------------------------------------ 4. separate(seed=)
FRAMES = (8, 5, 3)
CLIP_IDS = [2 ** 32 + 7, 11, 2 ** 62]
MIDPOINT2 = {"method": "midpoint", "options": {"step_size": 1 / 2}}


def _batch(cfg, clip_ids=None):
    """three ragged clips of 8, 5 and 3 latent frames (the shorter ones not a whole number of hops), ragged text"""
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, n * hop if n == max(FRAMES) else (n - 1) * hop + 100) for i, n in enumerate(FRAMES)]
    text, tmask = synthetic_text_features(len(FRAMES), 5, ragged=True)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * len(FRAMES), audios=clips, text_features=text, text_mask=tmask,
                                               clip_ids=clip_ids)
    assert batch.sizes_host == list(FRAMES)
    return batch


def _ranker(extracted_audio, input_audio, descriptions, sample_rate, **kw):
    return torch.tensor([[0.0, 1.0]] * len(extracted_audio), device=extracted_audio[0].device)


@functools.lru_cache(maxsize=None)
def _case(streams: int, dev: str):
    cfg = preset_config("tiny")
    kw = dict(precision="bf16x3") if SIM else {}   # default precision on the hardware; the simulator build has bf16 operands only
    model = SAMAudio(cfg, device=dev, streams=streams, **kw)
    model.load_state_dict(init_state_dict(cfg, seed=5), strict=False)
    model.text_ranker = _ranker
    return cfg, model


def _pair(model, batch, ids, **kw):
    """separate(seed=7) and the same call handed seeded_noise(7, ...) as noise=: (noise, latent) of the first, both pairs compared"""
    dev = model.device
    res = model.separate(batch, seed=7, reranking_candidates=2, **kw)
    lat = model.last_latent.clone()
    T = max(batch.sizes_host)
    explicit = seeded_noise(7, ids, 2, T, 256, dev)
    assert tuple(res.noise.shape) == (2 * len(ids), T, 256) and torch.equal(res.noise, explicit)
    again = model.separate(batch, noise=explicit.clone(), reranking_candidates=2, **kw)
    assert torch.equal(again.noise, explicit) and torch.equal(model.last_latent, lat) and torch.isfinite(lat).all()
    for a, b in zip(res.target + res.residual, again.target + again.residual):
        assert torch.equal(a, b)
    return res.noise, lat


@pytest.mark.parametrize("with_ids", [False, True], ids=["rows", "clip_ids"])
def test_separate_seed_whole_batch_and_every_shard(gpu, with_ids):
    """the whole batch, then every shard of world sizes 2 and 3: a shard's noise is the whole batch's rows trimmed to the shard's
    length, with the processor's clip ids and with none (shard_batch then names the clips by their rows in the whole batch)"""
    cfg, model = _case(1, str(gpu))
    ids = CLIP_IDS if with_ids else [0, 1, 2]
    whole = _batch(cfg, CLIP_IDS if with_ids else None)
    noise, lat = _pair(model, whole.to(gpu), ids, ode_opt=MIDPOINT2)
    assert torch.equal(noise, seeded_noise(7, ids, 2, 8, 256, gpu))
    for world in (2, 3):
        seen = 0
        for rank in range(world):
            shard = shard_batch(_batch(cfg, CLIP_IDS if with_ids else None), rank, world)
            rows = [ids.index(i) for i in shard.clip_ids]
            seen += len(rows)
            T = max(shard.sizes_host)
            sn, sl = _pair(model, shard.to(gpu), shard.clip_ids, ode_opt=MIDPOINT2)
            pick = [2 * b + c for b in rows for c in range(2)]
            assert torch.equal(sn, noise[pick, :T]), f"world {world} rank {rank}"
            assert tuple(sl.shape) == (len(pick), T, 256)
        assert seen == 3
    model.separate(whole, seed=8, reranking_candidates=2, ode_opt=MIDPOINT2)
    assert not torch.equal(model.last_latent, lat), "another seed, another latent"


@pytest.mark.skipif(SIM, reason="the dry run has no streams")
def test_separate_seed_two_streams(gpu):
    cfg, model = _case(2, str(gpu))
    noise, lat = _pair(model, _batch(cfg, CLIP_IDS).to(gpu), CLIP_IDS, ode_opt=MIDPOINT2)
    _, one = _case(1, str(gpu))
    one.separate(_batch(cfg, CLIP_IDS).to(gpu), seed=7, reranking_candidates=2, ode_opt=MIDPOINT2)
    assert torch.equal(one.last_latent, lat), "two streams, one stream: the same bits"


def test_separate_seed_windowed(gpu):
    """W = 6, O = 2: the 8-frame clip splits into two windows, the others stay one row each"""
    cfg, model = _case(1, str(gpu))
    sec = lambda frames: frames * cfg.audio_codec.hop_length / cfg.audio_codec.sample_rate   # noqa: E731
    _pair(model, _batch(cfg, CLIP_IDS).to(gpu), CLIP_IDS, ode_opt=MIDPOINT2, window_seconds=sec(6), window_overlap_seconds=sec(2))
    assert model.last_window_plan.counts == [2, 1, 1]


def test_separate_seed_adaptive(gpu):
    cfg, model = _case(1, str(gpu))
    _pair(model, _batch(cfg, CLIP_IDS).to(gpu), CLIP_IDS, ode_opt={"method": "bosh3", "rtol": 1e-2, "atol": 1e-2})
    assert len(model.last_ode_stats["rows"]) == 6


def test_separate_without_seed_draws_with_torch(gpu):
    """seed=None: the noise is torch.randn of the same shape from torch's generator, as before"""
    cfg, model = _case(1, str(gpu))
    batch = _batch(cfg, CLIP_IDS).to(gpu)
    torch.manual_seed(31)
    res = model.separate(batch, reranking_candidates=2, ode_opt=MIDPOINT2)
    torch.manual_seed(31)
    want = torch.randn(6, 8, 256, device=model.device)
    assert torch.equal(res.noise, want)
    assert not torch.equal(res.noise, seeded_noise(31, CLIP_IDS, 2, 8, 256, gpu))
    with pytest.raises(ValueError, match="mutually exclusive"):
        model.separate(batch, noise=want, seed=31)
