"""The CLAP ranker on the GPU: the log-mel front end (sam_audio_amd/csrc/kernels.hip clap_logmel_kernel;
include/samaudio.h samaudio_op_logmel; sam_audio_amd/clap.py logmel) against the float64 statement of tests/clap_ref.py, which
tests/test_clap_cpu.py pins to transformers' ClapFeatureExtractor; the towers' new kernels alone (csrc/clap_kernels.hip) and the whole
towers (csrc/clap.hip, clap.ClapTower) against transformers' ClapModel in float64; ranking.ClapRanker alone, in an ensemble and
through separate(); the error paths.

Every tower bound is 8 x the error of the same computation done by torch in float32 against float64, measured in the test itself.

The dB bound is derived, not chosen: the same statement is evaluated in float32 throughout on the CPU (torch.stft + matmul), its largest
|dB difference| against float64 over the very inputs of a test is measured in that test, and the kernel is allowed 4 x that - another FFT
factorisation and summation order rounds differently, but within the same order of magnitude.  Figures of the one GPU run
(profiles/clap/README.md):
"""
# MEASURED (MI355X, largest |dB error| against float64 over all cases of a parameter set; float32 CPU statement | kernel | bound):
#   clap-mini  (FFT 64, hop 8, 2 000 samples, 16 mels):        1.624e-05 | 1.439e-05 | 6.498e-05
#   real       (FFT 1024, hop 480, 480 000 samples, 64 mels):  4.131e-05 | 2.371e-05 | 1.652e-04
# unit-norm embeddings (float32 transformers | towers | bound): clap-mini audio 5.4e-08 | 1.2e-07 | 4.3e-07, text 2.8e-08 | 3.1e-08 |
#   2.2e-07; real dims audio 1.4e-08 | 2.0e-08 | 1.1e-07, text 9.1e-09 | 1.4e-08 | 7.3e-08; ranker scores 7.7e-08 | 9.3e-08 | 6.1e-07

import ctypes as C
import math

import pytest
import torch

from sam_audio_amd import clap, hip, synthetic
from sam_audio_amd.synthetic import synthetic_clip
from tests import clap_ref as R

pytestmark = pytest.mark.gpu
FACTOR = 4.0

# name -> (fft_size, hop, max_length, n_mels, the second crop offset of the 1.5 x clip)
PARAMS = {
    # the issue's second offset, 12 345, does not exist at clap-mini (a 3 000-sample clip can be cropped at 0..1 000): 345 stands in
    "mini": (64, 8, 2_000, 16, 345),
    "real": (1024, 480, 480_000, 64, 12_345),
}
_cache = {}


def _bank(name):
    fft, _, _, n_mels, _ = PARAMS[name]
    return clap.mel_bank(fft, n_mels)


def _clip(index, n):
    return synthetic_clip(index, n)[0]


def _cases(name):
    """[(label, wav [rows, n], lengths, offsets)] - the issue's inputs"""
    _, _, L, _, second = PARAMS[name]
    short = int(0.37 * L)
    pair = torch.zeros(2, L)
    pair[0, :short] = _clip(0, short)
    pair[1] = _clip(1, L)
    long = _clip(2, L + L // 2)
    tail = _clip(3, L).clone()
    tail[L // 2:] = 0.0                          # digital silence behind the middle
    return [("pair", pair, [short, L], None),
            ("long", torch.stack([long, long]), None, [0, second]),
            ("tail", tail[None], None, None)]


def _statements(name, label, quantise):
    """(float64, float32) statements of a case, computed once"""
    key = (name, label, quantise)
    if key not in _cache:
        fft, hop, L, _, _ = PARAMS[name]
        wav, lengths, offsets = next(c[1:] for c in _cases(name) if c[0] == label)
        kw = dict(lengths=lengths, offsets=offsets, max_length=L, fft_size=fft, hop=hop, bank=_bank(name), quantise=quantise)
        _cache[key] = (R.logmel(wav, **kw), R.logmel(wav, dtype=torch.float32, **kw).double())
    return _cache[key]


def _kernel(gpu, name, label, quantise, **extra):
    fft, hop, L, _, _ = PARAMS[name]
    wav, lengths, offsets = next(c[1:] for c in _cases(name) if c[0] == label)
    out = clap.logmel(wav.to(gpu), lengths, offsets, max_length=L, fft_size=fft, hop=hop, bank=_bank(name), quantise=quantise, **extra)
    assert out.dtype == torch.float32 and out.device.type == gpu.type
    assert tuple(out.shape) == (wav.shape[0], 1 + L // hop, PARAMS[name][3])
    return out


@pytest.mark.parametrize("name", list(PARAMS))
def test_frontend_against_the_float64_statement(gpu, name):
    """0.37 x and 1.0 x max_length with the int16 round trip on and off, a 1.5 x clip cropped at two offsets, a clip with a silent tail:
    every dB value within 4 x the float32 statement's own largest error over these inputs; all-zero frames are exactly -100 dB; a second
    run is bitwise equal"""
    fft, hop, L, n_mels, _ = PARAMS[name]
    runs = [("pair", True), ("pair", False), ("long", True), ("tail", True)]
    f32_err = max((f32 - f64).abs().max().item() for f64, f32 in (_statements(name, *r) for r in runs))
    bound = FACTOR * f32_err
    worst = 0.0
    for label, quantise in runs:
        f64, _ = _statements(name, label, quantise)
        got = _kernel(gpu, name, label, quantise)
        again = _kernel(gpu, name, label, quantise)
        assert torch.equal(got, again), (name, label, quantise)
        err = (got.cpu().double() - f64).abs().max().item()
        worst = max(worst, err)
        print(f"{name} {label} quantise={quantise}: kernel max |dB err| {err:.3e}, float32 statement {f32_err:.3e}, bound {bound:.3e}")
        assert torch.isfinite(got).all()
        assert err <= bound, (name, label, quantise, err, bound)
        if label == "tail":
            # frames whose every sample (reflection included) lies in the silent half: f hop - N / 2 >= L / 2
            first = -(-(L // 2 + fft // 2) // hop)
            assert first < 1 + L // hop - 1
            assert (f64[0, first:] == -100.0).all()
            assert (got[0, first:] == -100.0).all()
            # ... and in the live half only a mel filter without a bin is at the floor (clap-mini's bank has three)
            live = bool((_bank(name).sum(0) > 0).all())
            assert torch.equal(got[0, : first // 2].cpu() == -100.0, f64[0, : first // 2] == -100.0)
            assert (got[0, : first // 2] > -100.0).any() and (not live or (got[0, : first // 2] > -100.0).all())
    print(f"{name}: float32 statement {f32_err:.3e} dB, kernel {worst:.3e} dB, bound {bound:.3e} dB")


def test_frontend_crop_offset_is_the_sliced_waveform(gpu):
    """a longer clip at an offset == the same samples handed over as a clip of exactly max_length, bit for bit"""
    fft, hop, L, _, second = PARAMS["mini"]
    long = _clip(2, L + L // 2)
    a = clap.logmel(long[None].to(gpu), None, [second], max_length=L, fft_size=fft, hop=hop, bank=_bank("mini"))
    b = clap.logmel(long[second: second + L][None].to(gpu), max_length=L, fft_size=fft, hop=hop, bank=_bank("mini"))
    assert torch.equal(a, b)


def test_frontend_rows_do_not_depend_on_their_neighbours_or_on_the_view(gpu):
    """a row of a ragged batch == that clip alone; a strided [cand, n] view is read in place"""
    fft, hop, L, _, _ = PARAMS["mini"]
    kw = dict(max_length=L, fft_size=fft, hop=hop, bank=_bank("mini"))
    lens = [700, 2_000, 1_001, 1_001, 3_000]
    batch = torch.zeros(5, 3_000)
    for r, n in enumerate(lens):
        batch[r, :n] = _clip(10 + r, n)
    dev = batch.to(gpu)
    got = clap.logmel(dev, lens, [0, 0, 0, 0, 77], **kw)
    for r, n in enumerate(lens):
        alone = clap.logmel(batch[r, :n].clone().to(gpu), None, [77 if n > L else 0], **kw)
        assert torch.equal(got[r], alone[0]), r
    wide = torch.zeros(3, 4_000, device=dev.device)
    wide[:, :3_000] = dev[:3]
    view = wide[:, :3_000]
    assert not view.is_contiguous()
    assert torch.equal(clap.logmel(view, lens[:3], **kw), got[:3])


def test_frontend_batch_norm_fold_and_the_htk_bank(gpu):
    """the per-mel scale and shift against the statement (the bound scales with the largest |scale|), and the extractor's other bank"""
    fft, hop, L, n_mels, _ = PARAMS["mini"]
    g = torch.Generator().manual_seed(5)
    scale, shift = clap.fold_batch_norm(torch.randn(n_mels, generator=g), torch.randn(n_mels, generator=g),
                                        10 * torch.randn(n_mels, generator=g), 20 + 10 * torch.rand(n_mels, generator=g))
    wav = _clip(4, 1_500)[None]
    for bank in (_bank("mini"), clap.mel_bank(fft, n_mels, form="htk")):
        kw = dict(max_length=L, fft_size=fft, hop=hop, bank=bank)
        f64, f32 = R.logmel(wav, **kw), R.logmel(wav, dtype=torch.float32, **kw).double()
        bound = FACTOR * (f32 - f64).abs().max().item()
        plain = clap.logmel(wav.to(gpu), **kw).cpu().double()
        assert (plain - f64).abs().max().item() <= bound
        f64n = R.logmel(wav, bn_scale=scale, bn_shift=shift, **kw)
        f32n = R.logmel(wav, bn_scale=scale, bn_shift=shift, dtype=torch.float32, **kw).double()
        folded = clap.logmel(wav.to(gpu), bn_scale=scale, bn_shift=shift, **kw).cpu().double()
        assert (folded - f64n).abs().max().item() <= FACTOR * (f32n - f64n).abs().max().item()


@pytest.mark.parametrize("fft", [128, 256, 512, 2048])
def test_frontend_other_fft_sizes(gpu, fft):
    """every frames-per-workgroup class of the kernel (8 | 8 | 8 | 2 frames; 1024 is the real case above), a hop that does not divide
    max_length and a mel count that is no multiple of 16"""
    hop, L, n_mels = fft // 2 - 3, 5 * fft + 11, 20
    bank = clap.mel_bank(fft, n_mels)
    wav = _clip(6, L - 9)[None]
    kw = dict(max_length=L, fft_size=fft, hop=hop, bank=bank)
    f64, f32 = R.logmel(wav, **kw), R.logmel(wav, dtype=torch.float32, **kw).double()
    got = clap.logmel(wav.to(gpu), **kw)
    assert tuple(got.shape) == (1, 1 + L // hop, n_mels)
    assert (got.cpu().double() - f64).abs().max().item() <= FACTOR * (f32 - f64).abs().max().item()


# ---- the towers' kernels alone --------------------------------------------------------------------------------------------------

TOWER_FACTOR = 8.0
_models = {}


def _model(name):
    """(the seeded transformers.ClapModel in float32, its float64 copy), built once"""
    if name not in _models:
        import copy
        m = synthetic.init_clap_model(synthetic.clap_config(name), seed=3)
        _models[name] = (m, copy.deepcopy(m).double())
    return _models[name]


def _window_attention_torch(qkv, table, H, W, heads, hd, ws, shift, dtype):
    """roll -> window_partition -> scores + bias + mask -> softmax -> PV -> window_reverse -> roll back, as ClapAudioLayer /
    ClapAudioSelfAttention do it (modeling_clap.py:350-399, 526-613), on q|k|v rows [n H W, 3 C]"""
    from transformers.models.clap.modeling_clap import window_partition, window_reverse
    C_ = heads * hd
    n = qkv.shape[0] // (H * W)
    x = qkv.to(dtype).view(n, H, W, 3 * C_)
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    win = window_partition(x, ws).view(-1, ws * ws, 3 * C_)
    q, k, v = (win[..., i * C_: (i + 1) * C_].reshape(-1, ws * ws, heads, hd).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    bias = table.to(dtype)[clap.relative_position_index(ws).view(-1)].view(ws * ws, ws * ws, heads).permute(2, 0, 1)
    s = s + bias[None]
    if shift:
        h = torch.arange(H)
        w = torch.arange(W)
        region = ((h >= H - ws).long() + (h >= H - shift).long())[None, :, None, None] * 3 + \
                 ((w >= W - ws).long() + (w >= W - shift).long())[None, None, :, None]
        mw = window_partition(region.to(dtype), ws).view(-1, ws * ws)
        mask = mw[:, None, :] - mw[:, :, None]
        mask = mask.masked_fill(mask != 0, -100.0)
        nw = mask.shape[0]
        s = (s.view(n, nw, heads, ws * ws, ws * ws) + mask[None, :, None]).view(-1, heads, ws * ws, ws * ws)
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(-1, ws, ws, C_)
    o = window_reverse(o, ws, H, W)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(n * H * W, C_)


@pytest.mark.parametrize("hd", [24, 32])
@pytest.mark.parametrize("form", ["unshifted", "shifted", "whole"])
@pytest.mark.parametrize("ws", [4, 8])
def test_window_attention_alone(gpu, ws, form, hd):
    """2 x 2 windows (resolution 2 ws: 8 with window 4, 16 with window 8 and shift 4) or resolution == window; q, k, v and the bias
    table of magnitude 1; 3 clips, 3 heads"""
    H = W = ws if form == "whole" else 2 * ws
    shift = ws // 2 if form == "shifted" else 0
    n, heads = 3, 3
    g = torch.Generator().manual_seed(100 * ws + hd + shift)
    qkv = torch.randn(n * H * W, 3 * heads * hd, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    f64 = _window_attention_torch(qkv, table, H, W, heads, hd, ws, shift, torch.float64)
    f32 = _window_attention_torch(qkv, table, H, W, heads, hd, ws, shift, torch.float32)
    bound = TOWER_FACTOR * (f32.double() - f64).abs().max().item()
    dq, dt = qkv.to(gpu), table.to(gpu)
    out = torch.full((n * H * W, heads * hd), float("nan"), device=dq.device)
    hip.check(hip.clap_lib().samaudio_op_swin_window_attn(hip.ptr(dq), hip.ptr(dt), hip.ptr(out), n, H, W, heads, hd, ws, shift,
                                                          hip.current_stream_ptr()))
    err = (out.cpu().double() - f64).abs().max().item()
    print(f"window attention ws {ws} {form} hd {hd}: err {err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(out).all() and err <= bound


@pytest.mark.parametrize("frames", [256, 251])
def test_patch_embedding_alone(gpu, frames):
    """reshape_mel2img + patch_embed of the clap-mini module in float64, for 256 frames (no interpolation) and 251 (bicubic to 256)"""
    m32, m64 = _model("mini")
    enc32, enc64 = m32.audio_model.audio_encoder, m64.audio_model.audio_encoder
    feat = torch.randn(2, 1, frames, 16, generator=torch.Generator().manual_seed(frames))
    with torch.no_grad():
        f64 = enc64.patch_embed(enc64.reshape_mel2img(feat.double()))
        f32 = enc32.patch_embed(enc32.reshape_mel2img(feat)).double()
    bound = TOWER_FACTOR * (f32 - f64).abs().max().item()
    pe = enc32.patch_embed
    w = pe.proj.weight.detach().reshape(96, 16).contiguous().to(gpu)
    args = [t.detach().contiguous().to(gpu) for t in (pe.proj.bias, pe.norm.weight, pe.norm.bias)]
    dfeat = feat[:, 0].contiguous().to(gpu)
    out = torch.full((2, 256, 96), float("nan"), device=dfeat.device)
    hip.check(hip.clap_lib().samaudio_op_clap_patch_embed(hip.ptr(dfeat), 2, frames, 16, 64, 4, 4, 96, hip.ptr(w), *[hip.ptr(t) for t in args],
                                                          1e-5, hip.ptr(out), hip.current_stream_ptr()))
    err = (out.cpu().double() - f64).abs().max().item()
    print(f"patch embedding, {frames} frames: err {err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(out).all() and err <= bound


def test_patch_merge_alone(gpu):
    """ClapAudioPatchMerging's gather order and LayerNorm(4 C) (its reduction is a plain GEMM): 3 clips, an 8 x 6 map, C = 96"""
    from transformers.models.clap.modeling_clap import ClapAudioPatchMerging
    torch.manual_seed(4)
    mod = ClapAudioPatchMerging(96).eval()
    with torch.no_grad():
        mod.norm.weight.copy_(1 + 0.2 * torch.randn(384))
        mod.norm.bias.copy_(0.2 * torch.randn(384))
    n, H, W = 3, 8, 6
    x = torch.randn(n, H * W, 96)

    def gathered(module, t):   # everything in front of the reduction
        t = t.view(n, H, W, 96)
        t = torch.cat([t[:, row::2, col::2, :] for col in range(2) for row in range(2)], dim=-1)
        return module.norm(t.view(n, -1, 384))

    import copy
    with torch.no_grad():
        f64 = gathered(copy.deepcopy(mod).double(), x.double())
        f32 = gathered(mod, x).double()
        assert torch.allclose(mod.reduction(gathered(mod, x)), mod(x, (H, W)))   # (the restatement of the module's gather is the module's)
    bound = TOWER_FACTOR * (f32 - f64).abs().max().item()
    dx, lw, lb = x.to(gpu), mod.norm.weight.detach().to(gpu), mod.norm.bias.detach().to(gpu)
    out = torch.full((n, H * W // 4, 384), float("nan"), device=dx.device)
    hip.check(hip.clap_lib().samaudio_op_swin_patch_merge(hip.ptr(dx), hip.ptr(lw), hip.ptr(lb), 1e-5, hip.ptr(out), n, H, W, 96,
                                                          hip.current_stream_ptr()))
    err = (out.cpu().double() - f64).abs().max().item()
    print(f"patch merge: err {err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(out).all() and err <= bound


# ---- the whole towers ---------------------------------------------------------------------------------------------------------------

_towers = {}
FRONTENDS = {"mini": synthetic.CLAP_MINI_FRONTEND, "real": {}}


def _tower(gpu, name):
    if name not in _towers:
        _towers[name] = clap.ClapTower.from_module(_model(name)[0], gpu, FRONTENDS[name])
    return _towers[name]


def _extractor(name):
    from transformers import ClapFeatureExtractor
    fe = FRONTENDS[name]
    return ClapFeatureExtractor(feature_size=fe.get("feature_size", 64), sampling_rate=48_000, hop_length=fe.get("hop_length", 480),
                                fft_window_size=fe.get("fft_window_size", 1024), truncation="rand_trunc", padding="repeatpad")


def _hf_audio(name, clips):
    """(float64, float32) unit-norm audio embeddings of transformers' ClapModel on ClapFeatureExtractor's features of `clips`"""
    m32, m64 = _model(name)
    L = FRONTENDS[name].get("nb_max_samples", 480_000)
    feats = _extractor(name)([c.numpy() for c in clips], sampling_rate=48_000, max_length=L, return_tensors="pt")["input_features"]
    with torch.no_grad():
        return (m64.get_audio_features(input_features=feats.double()).pooler_output,
                m32.get_audio_features(input_features=feats.float()).pooler_output.double())


def _hf_text(name, ids, mask):
    m32, m64 = _model(name)
    with torch.no_grad():
        return (m64.get_text_features(input_ids=ids, attention_mask=mask).pooler_output,
                m32.get_text_features(input_ids=ids, attention_mask=mask).pooler_output.double())


def _pad_rows(clips):
    out = torch.zeros(len(clips), max(c.numel() for c in clips))
    for r, c in enumerate(clips):
        out[r, : c.numel()] = c
    return out


def _tokens(name, n):
    """n ragged token rows (bos, words, eos, padding), padded to the longest"""
    vocab = synthetic.clap_config(name).text_config.vocab_size
    g = torch.Generator().manual_seed(11)
    rows = [[0] + torch.randint(3, vocab, (3 + 4 * r,), generator=g).tolist() + [2] for r in range(n)]
    T = max(map(len, rows))
    ids = torch.tensor([r + [1] * (T - len(r)) for r in rows])
    return ids, (ids != 1).long()


@pytest.mark.parametrize("name", ["mini", "real"])
def test_whole_towers_against_transformers(gpu, name):
    """clap-mini: 3 ragged clips and 3 ragged token rows; HTSAT-tiny / RoBERTa-base dims: 2 clips of 1 s and 2 prompts.  The tower is
    given the waveform (int16 round trip off: the extractor has none), transformers the extractor's features"""
    lens = [700, 2_000, 1_300] if name == "mini" else [48_000, 48_000]
    clips = [_clip(20 + r, n) for r, n in enumerate(lens)]
    tower = _tower(gpu, name)
    a64, a32 = _hf_audio(name, clips)
    got = tower.audio_embed(_pad_rows(clips).to(gpu), 48_000, lengths=lens, quantise=False)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(lens), tower.dim) and got.device.type == gpu.type
    a_err, a_f32 = (got.cpu().double() - a64).abs().max().item(), (a32 - a64).abs().max().item()
    ids, mask = _tokens(name, len(lens))
    t64, t32 = _hf_text(name, ids, mask)
    tgot = tower.text_embed(ids.to(gpu), mask.to(gpu))
    t_err, t_f32 = (tgot.cpu().double() - t64).abs().max().item(), (t32 - t64).abs().max().item()
    print(f"{name}: audio embedding err {a_err:.3e} (float32 transformers {a_f32:.3e}, bound {TOWER_FACTOR * a_f32:.3e}); "
          f"text embedding err {t_err:.3e} (float32 transformers {t_f32:.3e}, bound {TOWER_FACTOR * t_f32:.3e})")
    assert torch.isfinite(got).all() and torch.isfinite(tgot).all()
    assert (got.norm(dim=1) - 1).abs().max() < 1e-5 and (tgot.norm(dim=1) - 1).abs().max() < 1e-5
    assert a_err <= TOWER_FACTOR * a_f32
    assert t_err <= TOWER_FACTOR * t_f32
    assert torch.equal(got, tower.audio_embed(_pad_rows(clips).to(gpu), 48_000, lengths=lens, quantise=False))


# ---- the ranker ---------------------------------------------------------------------------------------------------------------------

class _Tokenizer:
    """stands in for the checkpoint's RoBERTa tokenizer: bos, one id per character, eos, padded with the pad id"""

    def __call__(self, texts, padding=True, truncation=True, max_length=None, return_tensors="pt"):
        rows = [[0] + [3 + ord(c) % 90 for c in t][: (max_length or 512) - 2] + [2] for t in texts]
        T = max(map(len, rows))
        ids = torch.tensor([r + [1] * (T - len(r)) for r in rows])
        return {"input_ids": ids, "attention_mask": (ids != 1).long()}


def _ranker(gpu, **kw):
    from sam_audio_amd.ranking import ClapRanker
    return ClapRanker(model=_tower(gpu, "mini"), tokenizer=_Tokenizer(), **kw)


def _statement_scores(candidates, descriptions):
    """(float64, float32) scores [clips, candidates] of the reference's definition on transformers' ClapModel"""
    from tests.clap_ref import int16_round_trip
    tok = _Tokenizer()(descriptions, max_length=38)
    t64, t32 = _hf_text("mini", tok["input_ids"], tok["attention_mask"])
    clips = [int16_round_trip(c) for cand in candidates for c in cand]
    a64, a32 = _hf_audio("mini", clips)
    n = len(candidates[0])
    return ((a64.view(len(candidates), n, -1) @ t64[:, :, None])[..., 0], (a32.view(len(candidates), n, -1) @ t32[:, :, None])[..., 0])


def test_ranker_forward_and_ensemble(gpu):
    """2 clips x 3 candidates of ragged clip lengths: the scores against the float64 statement, the argmax wherever the statement's
    top-two gap exceeds twice the measured error, and the weighted sum of an ensemble with a constant ranker"""
    from sam_audio_amd.ranking import EnsembleRanker, Ranker
    cands = [torch.stack([_clip(30 + 3 * b + c, n) for c in range(3)]) for b, n in enumerate((1_200, 1_700))]
    descriptions = ["a dog barks", "rain on a roof"]
    s64, s32 = _statement_scores(cands, descriptions)
    ranker = _ranker(gpu)
    scores = ranker(extracted_audio=[c.to(gpu) for c in cands], descriptions=descriptions, sample_rate=48_000, input_audio=None)
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (2, 3) and scores.device.type == gpu.type
    err, f32_err = (scores.cpu().double() - s64).abs().max().item(), (s32 - s64).abs().max().item()
    print(f"ranker scores {scores.cpu().tolist()}, statement {s64.tolist()}: err {err:.3e}, float32 transformers {f32_err:.3e}")
    assert err <= TOWER_FACTOR * f32_err
    top = s64.topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1])
    assert (gap > 2 * err).all(), "the seed's clips must separate the top two candidates (checked when the test was written)"
    assert torch.equal(scores.cpu().argmax(dim=1), s64.argmax(dim=1))
    const = type("Const", (Ranker,), {"forward": lambda self, **kw: torch.tensor([[1.0, 2.0, 3.0], [6.0, 5.0, 4.0]]).to(gpu)})()
    ens = EnsembleRanker([ranker, const], [0.75, 0.25])
    both = ens(extracted_audio=[c.to(gpu) for c in cands], descriptions=descriptions, sample_rate=48_000)
    assert torch.allclose(both, 0.75 * scores + 0.25 * const(), rtol=0, atol=1e-7)
    # rand_trunc: a candidate longer than max_length is cropped where the generator says; the same generator state, the same scores
    long = [torch.stack([_clip(40 + c, 3_000) for c in range(3)]).to(gpu)]
    draws = [_ranker(gpu, truncation="rand_trunc", generator=torch.Generator().manual_seed(9))(
        extracted_audio=long, descriptions=["x"], sample_rate=48_000) for _ in range(2)]
    assert torch.equal(draws[0], draws[1]) and not torch.equal(draws[0], _ranker(gpu)(extracted_audio=long, descriptions=["x"]))


def test_ranker_through_separate(gpu):
    """tiny DiT, reranking_candidates=3, model.text_ranker = ClapRanker: the chosen candidate is the argmax of the ranker called on the
    returned candidates, and the run is bitwise repeatable"""
    from sam_audio_amd import SAMAudio, SAMAudioProcessor, preset_config
    from sam_audio_amd.synthetic import init_state_dict, synthetic_noise, synthetic_text_features
    cfg = preset_config("tiny")
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, f * hop) for i, f in enumerate((30, 22))]
    text, tmask = synthetic_text_features(2, 3)
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["a dog barks", "rain"], audios=clips, text_features=text, text_mask=tmask).to(gpu)
    model = SAMAudio(cfg, precision="fp32", device=str(gpu))
    model.load_state_dict(init_state_dict(cfg, seed=3))
    noise = synthetic_noise(6, 30).to(gpu)
    ranker, seen = _ranker(gpu), []

    def spy(**kw):
        seen.append(dict(kw, scores=ranker(**kw)))
        return seen[-1]["scores"]

    model.text_ranker = spy
    runs = [model.separate(batch, noise=noise, reranking_candidates=3) for _ in range(2)]
    assert len(seen) == 2 and tuple(seen[0]["scores"].shape) == (2, 3)
    picks = ranker(**{k: v for k, v in seen[0].items() if k != "scores"}).argmax(dim=1).tolist()
    for b, pick in enumerate(picks):
        assert torch.equal(runs[0].target[b], seen[0]["extracted_audio"][b][pick])
        assert torch.equal(runs[0].target[b], runs[1].target[b])
    assert torch.equal(seen[0]["scores"], seen[1]["scores"])


# ---- error paths: every case is a status code, nothing is launched ------------------------------------------------------------------

def test_error_paths(gpu):
    lib = hip.clap_lib()
    cfg = clap.tower_config(synthetic.clap_config("mini"), synthetic.CLAP_MINI_FRONTEND)
    h = C.c_void_p()
    cfg.enable_fusion = 1
    assert lib.samaudio_clap_create(C.byref(cfg), C.byref(h)) == hip.ERR_ARG and b"enable_fusion" in lib.samaudio_last_error()
    with pytest.raises(NotImplementedError, match="enable_fusion"):
        import copy
        fused = copy.deepcopy(synthetic.clap_config("mini"))
        fused.audio_config.enable_fusion = True
        clap.tower_config(fused)
    cfg.enable_fusion = 0
    cfg.embed_dim = 80          # head width 20, K = 80: refused at finalize
    cfg.heads[0], cfg.heads[1], cfg.heads[2] = 4, 8, 16
    assert lib.samaudio_clap_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.samaudio_clap_finalize(h) == hip.ERR_ARG
    lib.samaudio_clap_destroy(h)
    cfg.embed_dim, cfg.text_hidden = 96, 48      # K = 48 in the text tower
    h = C.c_void_p()
    assert lib.samaudio_clap_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.samaudio_clap_finalize(h) == hip.ERR_ARG and b"multiples of 32" in lib.samaudio_last_error()
    lib.samaudio_clap_destroy(h)
    tower = clap.ClapTower.from_module(_model("mini")[0], gpu, synthetic.CLAP_MINI_FRONTEND)   # a tower of its own: its workspace is replaced
    wav = _clip(50, 1_500)[None].to(gpu)
    out = torch.zeros(1, tower.dim, device=wav.device)
    small = torch.zeros(4_096, dtype=torch.uint8, device=wav.device)
    base = (small.data_ptr() + 255) // 256 * 256
    assert lib.samaudio_clap_set_workspace(tower._h, C.c_void_p(base), 1_024) == 0

    def embed(length):
        return lib.samaudio_clap_audio_embed(tower._h, hip.ptr(wav), 1, 1_500, (C.c_int64 * 1)(length), None, 1, hip.ptr(out),
                                             hip.current_stream_ptr())

    assert embed(1_500) == hip.ERR_WORKSPACE
    ids = torch.zeros(1, 39, dtype=torch.int64, device=wav.device)
    mask = torch.ones(1, 39, dtype=torch.uint8, device=wav.device)
    assert lib.samaudio_clap_text_embed(tower._h, hip.ptr(ids), hip.ptr(mask), 1, 8, hip.ptr(out), hip.current_stream_ptr()) == hip.ERR_WORKSPACE
    tower._workspace = None
    tower._ensure(1, 1, 39)
    assert embed(0) == hip.ERR_ARG and b"length < 1" in lib.samaudio_last_error()
    # 40 positions, pad id 1: positions 2 .. 39 exist, so 38 tokens fit and 39 do not
    assert lib.samaudio_clap_text_embed(tower._h, hip.ptr(ids), hip.ptr(mask), 1, 39, hip.ptr(out), hip.current_stream_ptr()) == hip.ERR_ARG
    assert b"position table" in lib.samaudio_last_error()
    with pytest.raises(AssertionError, match="position table"):
        tower.text_embed(ids, mask)
    assert embed(1_500) == 0 and torch.isfinite(out).all()
