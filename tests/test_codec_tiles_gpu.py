"""The time-tiled DAC-VAE on the GPU: tiled encode / decode / decode-pairs against the untiled calls, bit
for bit, in every precision the codec runs in; the reach the library reports, observed through the engine; the workspace of a tiled
call; and separate(codec_tile_seconds=...) against separate() on every path that reaches the codec.

There is no tolerance in this file: every comparison of results is torch.equal on fp32 tensors (plus isfinite).  `h` below is the
direction's halo as the library reports it (6 frames for the encoder, 8 for the decoder at the rates 2, 8, 10, 12; tests/
test_codec_tiles_cpu.py holds the figure to the restatement of tests/codec_tiles_ref.py)."""
import functools

import pytest
import torch

from sam_audio_amd import SAMAudio, SAMAudioProcessor, preset_config
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
from tests import codec_tiles_ref as R

pytestmark = pytest.mark.gpu

# (precision, codec_decode): what SAMAudio runs the codec in - the decoder of an x3 model in its own fp32 context ("32") or on plain
# 16-bit operands ("16")
ENCODE = [("fp32", "auto"), ("bf16", "auto"), ("fp16", "auto"), ("fp16x3", "32"), ("bf16x3", "32")]
DECODE = ENCODE + [("fp16x3", "16"), ("bf16x3", "16")]
MIDPOINT2 = {"method": "midpoint", "options": {"step_size": 1 / 2}}


@functools.lru_cache(maxsize=None)
def _weights():
    cfg = preset_config("tiny")
    return cfg, init_state_dict(cfg, seed=7)


_MODELS = {}


def _model(gpu, prec, dec="auto", fresh=False, **kw):
    key = (prec, dec)
    if fresh or kw or key not in _MODELS:
        cfg, sd = _weights()
        m = SAMAudio(cfg, precision=prec, device=str(gpu), codec_decode=dec, **kw)
        m.load_state_dict(sd, strict=False)
        if fresh or kw:
            return m
        _MODELS[key] = m
    return _MODELS[key]


def _halo(model, decode):
    return model._lib.samaudio_codec_halo_frames(model._ctx, int(decode))


def _drop_workspace(model):
    """the next call allocates exactly what it asks for: the engine then runs the items per pass SAMAUDIO_CODEC_CHUNK says"""
    for own in [model] + list(model._lanes):
        own._workspace = None


def _same(a, b):
    return torch.equal(a, b) and bool(torch.isfinite(a).all())


def _shapes(h):
    """(T, L): three tiles - clamped left, both halos complete, clamped right; a short last tile; one tile (the untiled call); single
    frames around a clip where only the middle frame has both halos; and the case that crosses the tile policy's row thresholds: the
    frame-rate GEMMs of a tile see M = 32 + 2h rows per item where the whole pass sees 300"""
    L = h + 1
    return [(3 * L, L), (3 * L - 2, L), (3 * L, 3 * L + 5), (2 * h + 1, 1), (300, 32)]


def _waves(T, hop):
    """3 ragged waveforms in a batch padded to T frames, the shorter ones not a whole number of hops"""
    lengths = [T * hop, (T - 1) * hop - 100, max(1, T - 5) * hop - 7]
    wav = torch.zeros(3, 1, T * hop)
    for i, n in enumerate(lengths):
        wav[i, 0, :n] = synthetic_clip(i, n).view(-1)[:n]
    return wav


# ------------------------------------------------------------------------------------------------ 1. tiled == whole
@pytest.mark.parametrize("prec,dec", ENCODE, ids=[p for p, _ in ENCODE])
def test_tiled_encode_equals_whole_bitwise(gpu, monkeypatch, prec, dec):
    model = _model(gpu, prec, dec)
    hop, h = model.cfg.audio_codec.hop_length, _halo(model, False)
    for T, L in _shapes(h):
        wav = _waves(T, hop).to(gpu)
        monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", "16")
        whole = model.encode_audio(wav)
        for chunk in ("16", "1"):
            monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", chunk)
            _drop_workspace(model)
            tiled = model.encode_audio(wav, tile_frames=L)
            rec = model.last_codec_tiles["encode"]
            assert _same(tiled, whole), f"{prec} encode T={T} L={L} chunk={chunk}: {(tiled != whole).any(2).nonzero()[:6].tolist()}"
            assert rec == dict(tile_frames=L, halo_frames=h, tiles=-(-T // L) if L < T else 1, passes=1 if chunk == "16" else 3), rec
        _drop_workspace(model)


@pytest.mark.parametrize("pairs", [False, True], ids=["items", "pairs"])
@pytest.mark.parametrize("prec,dec", DECODE, ids=[p + ("" if d != "16" else "+dec16") for p, d in DECODE])
def test_tiled_decode_equals_whole_bitwise(gpu, monkeypatch, prec, dec, pairs):
    model = _model(gpu, prec, dec)
    CD, h = model.cfg.audio_codec.codebook_dim, _halo(model, True)
    for T, L in _shapes(h):
        g = torch.Generator().manual_seed(T)
        lat = (torch.randn(2, T, 2 * CD, generator=g) if pairs else torch.randn(3, T, CD, generator=g)).to(gpu)
        if not pairs:   # ragged: zero latent behind the shorter clips
            lat[1, T - 2:], lat[2, max(1, T - 5):] = 0, 0
        items = 4 if pairs else 3
        monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", "16")
        whole = model.decode_audio(lat, pairs=pairs)
        for chunk in ("16", "2" if pairs else "1"):   # (a pass of pairs holds whole pairs)
            monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", chunk)
            _drop_workspace(model)
            tiled = model.decode_audio(lat, pairs=pairs, tile_frames=L)
            rec = model.last_codec_tiles["decode"]
            assert _same(tiled, whole), f"{prec}/{dec} decode pairs={pairs} T={T} L={L} chunk={chunk}: first difference at " \
                                        f"{(tiled != whole).nonzero()[:4].tolist()}"
            # (the 16-bit decoder of an x3 model runs in the workspace sized for the fp32 context: more items fit a pass)
            passes = 1 if chunk == "16" else rec["passes"] if dec == "16" else items // int(chunk)
            assert rec == dict(tile_frames=L, halo_frames=h, tiles=-(-T // L) if L < T else 1, passes=passes), rec
            assert 1 <= rec["passes"] <= items // int(chunk) or chunk == "16"
        _drop_workspace(model)


# ------------------------------------------------------------------------------------------------ 2. the reach
def test_encoder_reach_through_the_engine(gpu):
    """One input sample changed in the middle of a 4h-frame clip: latent frame f reads samples [f hop - lo, (f + 1) hop - 1 + hi]
    (tests/codec_tiles_ref.reach_rows), so exactly the frames from ceil((s - hi - hop + 1) / hop) to floor((s + lo) / hop) may differ;
    everything else is bit-equal, no frame farther than h away differs, and the outermost frame differs on the side that sets h."""
    model = _model(gpu, "fp32")
    a = model.cfg.audio_codec
    hop, h = a.hop_length, _halo(model, False)
    lo, hi, per = R.reach_rows(a.encoder_rates, a.decoder_rates, False)
    assert per == hop and h == max(-(-lo // hop), -(-hi // hop))
    T = 4 * h
    worst = []
    # the sample positions inside their frame at which the reach to the right / to the left is longest
    for s in (2 * h * hop + (-lo) % hop, 2 * h * hop + (hi + hop - 1) % hop, 2 * h * hop + hop // 2):
        wav = synthetic_clip(0, T * hop).view(1, 1, -1).to(gpu).clone()
        base = model.encode_audio(wav)
        wav[0, 0, s] += 1.0
        diff = (model.encode_audio(wav) != base).any(2)[0].nonzero().view(-1).tolist()
        first, last = -((-(s - hi - hop + 1)) // hop), (s + lo) // hop
        print(f"encoder reach: sample {s} (frame {s // hop} + {s % hop}) changes frames {diff[0]} .. {diff[-1]}; allowed {first} .. {last}")
        assert diff and first <= diff[0] and diff[-1] <= last
        assert s // hop - h <= diff[0] and diff[-1] <= s // hop + h
        worst.append((s // hop - diff[0], diff[-1] - s // hop, s // hop - first, last - s // hop))
    # the restatement's reach is attained: on the side (or sides) whose reach in frames is h, some sample position reaches that far
    if -(-lo // hop) == h:
        assert max(w[1] for w in worst) == h, worst
    if -(-hi // hop) == h:
        assert max(w[0] for w in worst) == h, worst


def test_decoder_reach_through_the_engine(gpu):
    """One input frame t changed in the middle of a 4h-frame clip: output frame f reads latent frames [f - lo, f + hi], so the samples
    of frames t - hi .. t + lo may differ and nothing else; both outermost frames do differ."""
    model = _model(gpu, "fp32")
    a = model.cfg.audio_codec
    hop, h, CD = a.hop_length, _halo(model, True), a.codebook_dim
    lo, hi, per = R.reach_rows(a.encoder_rates, a.decoder_rates, True)
    assert per == 1 and h == max(lo, hi)
    T, t = 4 * h, 2 * h
    lat = torch.randn(1, T, CD, generator=torch.Generator().manual_seed(5)).to(gpu)
    base = model.decode_audio(lat)
    lat[0, t] += 1.0
    diff = (model.decode_audio(lat) != base).view(T, hop).any(1).nonzero().view(-1).tolist()
    print(f"decoder reach: frame {t} changes output frames {diff[0]} .. {diff[-1]}; allowed {t - hi} .. {t + lo}")
    assert diff[0] == t - hi and diff[-1] == t + lo
    assert t - h <= diff[0] and diff[-1] <= t + h


# ------------------------------------------------------------------------------------------------ 3. the workspace
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_workspace_of_a_tiled_call_does_not_grow_with_the_clip(gpu, monkeypatch, prec):
    model = _model(gpu, prec, fresh=True)
    a = model.cfg.audio_codec
    monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", "2")
    L, sizes = 16, {}
    for what in ("encode", "decode"):
        for T in (120, 240):
            _drop_workspace(model)
            if what == "encode":
                model.encode_audio(torch.zeros(2, 1, T * a.hop_length, device=gpu), tile_frames=L)
            else:
                model.decode_audio(torch.zeros(2, T, a.codebook_dim, device=gpu), tile_frames=L)
            seg = (L + 2 * _halo(model, what == "decode")) * a.hop_length
            assert model._lib.samaudio_codec_tile_samples(model._ctx, T, L, int(what == "decode")) == seg
            need = model._lib.samaudio_workspace_bytes(model._ctx, 0, 0, 0, 2, seg)
            assert model._workspace.numel() - 256 == need, (what, T)
            sizes[what, T] = need
        whole = model._lib.samaudio_workspace_bytes(model._ctx, 0, 0, 0, 2, 240 * a.hop_length)
        print(f"{prec} {what}: {sizes[what, 240]} bytes tiled (L = {L}) at 120 and at 240 frames, {whole} untiled at 240")
        assert sizes[what, 120] == sizes[what, 240] < whole


# ------------------------------------------------------------------------------------------------ 4. separate()
FRAMES, TILE, W, OV = (29, 17), 9, 16, 4   # TILE: between h (8) and T / 3; windows: 3 + 2 rows


def _seconds(cfg, frames):
    return frames * cfg.audio_codec.hop_length / cfg.audio_codec.sample_rate


def _batch(cfg):
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, n * hop if n == max(FRAMES) else (n - 1) * hop + 100) for i, n in enumerate(FRAMES)]
    text, tmask = synthetic_text_features(len(FRAMES), 5, ragged=True)
    return SAMAudioProcessor.from_config(cfg)(descriptions=["x"] * len(FRAMES), audios=clips, text_features=text, text_mask=tmask)


def _prefers_candidate_1(extracted_audio, **kw):
    return torch.tensor([[0.0, 1.0]] * len(extracted_audio))


def _equal_results(a, b):
    return all(_same(x, y) for x, y in zip(a.target + a.residual, b.target + b.residual)) and len(a.target) == len(b.target)


PATHS = {
    "plain": (dict(), dict()),
    "windows": (dict(), dict(window_seconds=W, window_overlap_seconds=OV)),
    "streams2": (dict(streams=2), dict()),
    "candidates": (dict(), dict(reranking_candidates=2)),
    "resampled": (dict(), dict(output_sampling_rate=16000)),
    "decode16": (dict(dec="16"), dict()),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_separate_with_codec_tiles_equals_separate_without(gpu, path):
    cfg, _ = _weights()
    model_kw, call_kw = PATHS[path]
    call_kw = {k: _seconds(cfg, v) if k.startswith("window") else v for k, v in call_kw.items()}
    cand = call_kw.get("reranking_candidates", 1)
    noise = synthetic_noise(len(FRAMES) * cand, max(FRAMES)).to(gpu)
    model = _model(gpu, "fp16x3", fresh=True, **model_kw)
    if cand > 1:
        model.text_ranker = _prefers_candidate_1
    h = _halo(model, True)
    assert h <= TILE <= max(FRAMES) / 3
    plain = model.separate(_batch(cfg).to(gpu), noise=noise, ode_opt=MIDPOINT2, **call_kw)
    lat_plain = model.last_latent.clone()
    assert model.last_codec_tiles == {}
    tiled = model.separate(_batch(cfg).to(gpu), noise=noise, ode_opt=MIDPOINT2, codec_tile_seconds=_seconds(cfg, TILE), **call_kw)
    rec = model.last_codec_tiles
    print(f"{path}: {rec}")
    assert _same(model.last_latent, lat_plain) and _equal_results(tiled, plain), path
    tiles = -(-max(FRAMES) // TILE)
    assert rec["encode"] == dict(tile_frames=TILE, halo_frames=_halo(model, False), tiles=tiles, passes=1)
    assert rec["decode"] == dict(tile_frames=TILE, halo_frames=h, tiles=tiles, passes=2 if path == "streams2" else 1)
    if path == "windows":
        assert model.last_window_plan.counts == [3, 2]
    if path == "plain":
        # the setting on the model is the same call; a call without the setting after one with it equals a fresh model's
        other = _model(gpu, "fp16x3", fresh=True, codec_tile_seconds=_seconds(cfg, TILE))
        assert _equal_results(other.separate(_batch(cfg).to(gpu), noise=noise, ode_opt=MIDPOINT2), plain)
        assert other.last_codec_tiles == rec
        again = model.separate(_batch(cfg).to(gpu), noise=noise, ode_opt=MIDPOINT2)
        fresh = _model(gpu, "fp16x3", fresh=True).separate(_batch(cfg).to(gpu), noise=noise, ode_opt=MIDPOINT2)
        assert _equal_results(again, fresh) and _equal_results(again, plain) and model.last_codec_tiles == {}
        with pytest.raises(ValueError):
            model.separate(_batch(cfg).to(gpu), noise=noise, codec_tile_seconds=_seconds(cfg, 0.4))
        with pytest.raises(ValueError):
            SAMAudio(cfg, device=str(gpu), codec_tile_seconds=0.0)
