"""Resampling, mono mix and padding of PCM clips in one HIP kernel (sam_audio_amd/csrc/kernels.hip resample_mix_kernel;
include/samaudio.h samaudio_op_resample; sam_audio_amd/audio.py).

The yardstick is the float64 direct form of tests/resample_ref.py, pinned to processor.resample by tests/test_audio_frontend_cpu.py.
The bound is R.tolerance(K, C, S, A) = 1.01 (K + C + 2) 2^-24 S A: the first-order bound of an fp32 dot product of K fp32-rounded
weights over inputs that carry a C-term mean (K: longest tap run, S: max_p sum |h|, A: max |x|).  It is derived, not measured.
Impulses, the padding, the guard behind the output and the invariances are checked bit for bit.
"""
import ctypes as C
import os
import wave

import pytest
import torch

from sam_audio_amd import SAMAudioProcessor, audio, hip, preset_config
from tests import resample_ref as R

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
GUARD = 37      # floats behind out_capacity that must stay as they were
# more than 32 inputs per output: even the smallest tile's input window passes the kernel's LDS array, so its tiles read the clip
# straight from memory (the other path of the kernel); 291 taps on each side
STEEP = (48000, 1000)


def _figures(orig, new):
    return (1, 1.0) if orig == new else R.bank_figures(orig, new)


def _upload(gpu, x, layout, shift=0):
    """x [C, S] on the CPU -> (device tensor whose first element is sample (0, 0), channel stride, sample stride).  `shift`: that many
    elements of other data in front, so that the base pointer is aligned to the element size only."""
    ch, samples = x.shape
    flat = (x.t() if layout == "interleaved" else x).contiguous().flatten()
    if shift:
        flat = torch.cat([torch.full((shift,), 77, dtype=x.dtype), flat])
    dev = flat.to(gpu)[shift:]
    return (dev, 1, ch) if layout == "interleaved" else (dev, samples, 1)


def _resample(gpu, x, orig, new, layout, shift=0, extra=0):
    """samaudio_op_resample on a NaN-filled destination with `extra` floats of padding and a guard -> (status, out, length)"""
    pcm, cs, ss = _upload(gpu, x, layout, shift)
    bank, taps, first = audio.device_bank(orig, new, gpu)
    length = R.out_length(x.shape[1], orig, new)
    out = torch.full((length + extra + GUARD,), float("nan"), device=gpu)
    rc = hip.lib().samaudio_op_resample(C.c_void_p(pcm.data_ptr()), hip.PCM_S16 if x.dtype == torch.int16 else hip.PCM_F32,
                                        x.shape[0], x.shape[1], cs, ss, hip.ptr(taps), hip.ptr(first), bank.n, bank.o, bank.K,
                                        hip.ptr(out), length + extra, hip.current_stream_ptr())
    return rc, out.cpu(), length


def _check(gpu, x, orig, new, layout, shift=0, extra=0):
    rc, out, length = _resample(gpu, x, orig, new, layout, shift, extra)
    hip.check(rc)
    K, S = _figures(orig, new)
    A = R.to_float64(x).abs().max().item()
    tol = R.tolerance(K, x.shape[0], S, A)
    err = (out[:length].double() - R.direct(x, orig, new)).abs().max().item()
    what = f"{orig} -> {new}, {tuple(x.shape)} {x.dtype} {layout} shift {shift}"
    print(f"{what}: max-abs {err:.3e}, bound {tol:.3e} ({err / tol:.3f})")
    assert err <= tol, what
    assert torch.equal(out[length: length + extra], torch.zeros(extra)), f"{what}: padding"
    assert bool(out[length + extra:].isnan().all()), f"{what}: something was written behind out_capacity"
    return out[:length]


@pytest.mark.parametrize("orig,new", R.PAIRS + [(48000, 48000)], ids=lambda v: str(v))
def test_kernel_against_the_direct_form(gpu, orig, new):
    """every length class x channels 1, 2, 3 x int16 interleaved (also at a base pointer one sample off) and fp32 planar"""
    for i, samples in enumerate(R.lengths(orig, new)):
        for ch in (1, 2, 3):
            _check(gpu, R.pcm_int16(ch, samples, seed=10 * i + ch), orig, new, "interleaved", shift=ch % 2, extra=(0, 1, 300)[ch - 1])
            _check(gpu, R.pcm_float(ch, samples, seed=20 * i + ch), orig, new, "planar", extra=(300, 0, 1)[ch - 1])
    samples = R.lengths(orig, new)[3]
    _check(gpu, R.pcm_int16(2, samples, seed=5), orig, new, "planar", shift=1, extra=3)
    _check(gpu, R.pcm_float(3, samples, seed=6), orig, new, "interleaved", shift=1, extra=3)


def test_kernel_reads_memory_directly_when_the_window_passes_lds(gpu):
    """48 inputs per output: a tile of 256 outputs reaches 12 800 inputs, more than the LDS array holds, and reads the clip straight
    from memory.  A clip short enough for one small tile (150 outputs: 7 800 inputs) goes through LDS; the same clip followed by
    zeros is the other path and must give the same bits where the short clip has outputs."""
    orig, new = STEEP
    short = R.pcm_int16(2, 150 * 48, seed=3)
    long_ = torch.cat([short, torch.zeros(2, 300 * 48, dtype=torch.int16)], 1)
    a = _check(gpu, short, orig, new, "interleaved", extra=5)
    b = _check(gpu, long_, orig, new, "interleaved", extra=5)
    assert a.numel() == 150 and b.numel() == 450
    assert torch.equal(a, b[:150])
    _check(gpu, R.pcm_float(3, 300 * 48 + 1, seed=4), orig, new, "planar", shift=1)


@pytest.mark.parametrize("orig,new", [(44100, 48000), (48000, 44100), (3, 2), (16000, 48000), (48000, 16000)], ids=lambda v: str(v))
def test_impulses_return_the_fp32_weights_exactly(gpu, orig, new):
    """One sample of value 1: every output is a single product, so it must BE the fp32-rounded float64 weight h(p, c - f o) - any
    dropped, shifted or mis-phased tap shows."""
    o, n, _, width = R.geometry(orig, new)
    h32 = R.weights64(orig, new).float()                       # [n, 2 width + o], column = d + width
    samples = 5 * o + 61
    length = R.out_length(samples, orig, new)
    j = torch.arange(length)
    for c in (0, samples // 2, samples - 1):
        x = torch.zeros(1, samples)
        x[0, c] = 1.0
        col = c - (j // n) * o + width
        ok = (col >= 0) & (col < h32.shape[1])
        want = torch.where(ok, h32[j % n, col.clamp(0, h32.shape[1] - 1)], torch.zeros(()))
        assert int((want != 0).sum()) >= 5
        rc, out, _ = _resample(gpu, x, orig, new, "planar", extra=2)
        hip.check(rc)
        assert torch.equal(out[:length], want), f"impulse at {c}"


def test_result_does_not_depend_on_capacity_or_batch(gpu):
    """The same clip alone, with a larger out_capacity (more workgroups), through audio.mix_into as a row of a mixed-rate batch, and
    through audio.resample: equal bits."""
    x = R.pcm_int16(2, 9000, seed=8)
    rc, alone, length = _resample(gpu, x, 44100, 48000, "interleaved")
    hip.check(rc)
    rc, roomy, _ = _resample(gpu, x, 44100, 48000, "interleaved", extra=5000)
    hip.check(rc)
    assert torch.equal(alone[:length], roomy[:length])
    other = R.pcm_float(3, 7000, seed=9)
    rows = torch.full((2, 1, R.out_length(7000, 16000, 48000)), float("nan"), device=gpu)
    pcm, cs, ss = _upload(gpu, x, "interleaved")
    assert audio.mix_into(rows[1, 0], other.to(gpu), 3, 7000, 7000, 1, 16000, 48000) == rows.shape[-1]
    assert audio.mix_into(rows[0, 0], pcm, 2, 9000, cs, ss, 44100, 48000) == length
    assert torch.equal(rows[0, 0, :length].cpu(), alone[:length]) and float(rows[0, 0, length:].abs().max()) == 0.0
    # audio.resample: one launch per row of a [..., samples] tensor, fp32 on the device; int16 rows are PCM
    mono = x[:1]
    got = audio.resample(mono.to(gpu), 44100, 48000)
    assert got.shape == (1, length) and got.dtype == torch.float32 and got.device.type == gpu.type
    rc, want, _ = _resample(gpu, mono, 44100, 48000, "planar")
    hip.check(rc)
    assert torch.equal(got[0].cpu(), want[:length])
    both = audio.resample((x.float() / 32768.0).to(gpu)[None], 44100, 48000)          # [1, 2, samples] fp32
    assert both.shape == (1, 2, length) and torch.equal(both[0, 0].cpu(), want[:length])
    y = torch.zeros(3, 5, device=gpu)
    assert audio.resample(y, 48000, 48000) is y


@pytest.mark.skipif(SIM, reason="13.5 M samples: MI355X only")
def test_long_clip_offsets_past_2_31(gpu):
    """44 100 -> 16 000 on 13.5 M int16 samples: j o passes 2^31 for the last outputs.  The first and the last 2 000 outputs against
    the direct form, which is evaluated on the matching input windows only."""
    orig, new, samples = 44100, 16000, 13_500_000
    o, n = R.reduced(orig, new)
    x = R.pcm_int16(1, samples, seed=11)
    length = R.out_length(samples, orig, new)
    assert (length - 1) * o > 2 ** 31
    rc, out, _ = _resample(gpu, x, orig, new, "planar", extra=1000)
    hip.check(rc)
    K, S = _figures(orig, new)
    tol = R.tolerance(K, 1, S, 1.0)
    for j0, j1 in ((0, 2000), (length - 2000, length)):
        err = (out[j0:j1].double() - R.direct(x, orig, new, j0, j1)).abs().max().item()
        print(f"outputs [{j0}, {j1}): max-abs {err:.3e}, bound {tol:.3e}")
        assert err <= tol
    assert torch.equal(out[length: length + 1000], torch.zeros(1000)) and bool(out[length + 1000:].isnan().all())
    assert bool(torch.isfinite(out[:length]).all())


def _write_wav(path, x_int16, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(x_int16.shape[0])
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(x_int16.t().contiguous().numpy().astype("<i2").tobytes())
    return str(path)


def _processors(gpu):
    cfg = preset_config("tiny")
    return cfg, SAMAudioProcessor.from_config(cfg), SAMAudioProcessor.from_config(cfg, audio_transform="hip", device=gpu)


def _same_host_fields(a, b):
    for name in ("sizes", "wav_sizes", "audio_pad_mask", "anchor_ids", "anchor_alignment"):
        assert torch.equal(getattr(a, name).cpu(), getattr(b, name).cpu()), name
    assert a.sizes_host == b.sizes_host and a.descriptions == b.descriptions and a.anchors == b.anchors


def test_processor_hip_against_torch(gpu, tmp_path):
    """a stereo 16-bit 44.1 kHz WAV file, a mono fp32 tensor at the model's rate and a 3-channel 16 kHz tensor in one batch"""
    cfg, p_torch, p_hip = _processors(gpu)
    rate = cfg.audio_codec.sample_rate
    stereo = R.pcm_int16(2, 5000, seed=21)
    clips = [_write_wav(tmp_path / "stereo.wav", stereo, 44100), R.pcm_float(1, 6001, seed=22), R.pcm_float(3, 1500, seed=23)]
    kw = dict(descriptions=["a", "b", "c"], audios=clips, sampling_rates=[None, None, 16000],
              anchors=[[("+", 0.0, 0.05)], [], [("-", 0.01, 0.06)]])
    want, got = p_torch(**kw), p_hip(**kw)
    assert got.audios.device.type == gpu.type and got.audios.dtype == torch.float32 and got.audios.shape == want.audios.shape
    _same_host_fields(want, got)
    lengths = [R.out_length(5000, 44100, rate), 6001, R.out_length(1500, 16000, rate)]
    assert want.wav_sizes.tolist() == lengths
    for i, (x, orig) in enumerate(((stereo, 44100), (clips[1], rate), (clips[2], 16000))):
        K, S = _figures(orig, rate)
        tol = R.tolerance(K, x.shape[0], S, R.to_float64(x).abs().max().item())
        err = (got.audios[i, 0].cpu() - want.audios[i, 0]).abs().max().item()
        print(f"clip {i} ({orig} Hz, {x.shape[0]} channels): hip against torch {err:.3e}, bound {tol:.3e}")
        assert err <= tol
        assert torch.equal(got.audios[i, 0, lengths[i]:].cpu(), want.audios[i, 0, lengths[i]:])      # the padding: zeros
    moved = got.to(gpu)
    assert moved.sizes.device.type == gpu.type and moved.anchor_ids.device.type == gpu.type
    _same_host_fields(want, moved)


def _same_rate_batches(gpu, tmp_path, cfg, p_torch, p_hip, **more):
    hop, rate = cfg.audio_codec.hop_length, cfg.audio_codec.sample_rate
    clips = [_write_wav(tmp_path / "mono.wav", R.pcm_int16(1, 4 * hop, seed=31), rate),
             _write_wav(tmp_path / "stereo.wav", R.pcm_int16(2, 3 * hop - 7, seed=32), rate)]
    kw = dict(descriptions=["a", "b"], audios=clips, **more)
    return p_torch(**kw), p_hip(**kw)


def test_same_rate_int16_batch_is_bit_equal(gpu, tmp_path):
    """the conversion (x / 32768) and a two-term mean are exact in fp32: the kernel's batch IS the CPU's"""
    cfg, p_torch, p_hip = _processors(gpu)
    want, got = _same_rate_batches(gpu, tmp_path, cfg, p_torch, p_hip)
    assert torch.equal(got.audios.cpu(), want.audios)
    _same_host_fields(want, got)


def test_separate_from_the_hip_batch_and_output_sampling_rate(gpu, tmp_path):
    """separate() from the "hip" batch equals separate() from the "torch" batch with the same noise (the batches are bit-equal), and
    output_sampling_rate=44100 returns exactly audio.resample of the plain result."""
    from sam_audio_amd import SAMAudio
    from sam_audio_amd.synthetic import init_state_dict, synthetic_noise, synthetic_text_features
    cfg, p_torch, p_hip = _processors(gpu)
    text, tmask = synthetic_text_features(2, 3)
    want_b, got_b = _same_rate_batches(gpu, tmp_path, cfg, p_torch, p_hip, text_features=text, text_mask=tmask)
    model = SAMAudio(cfg, precision="fp32", device=str(gpu))
    model.load_state_dict(init_state_dict(cfg, seed=3))
    noise = synthetic_noise(2, 4).to(gpu)
    want = model.separate(want_b.to(gpu), noise=noise)
    got = model.separate(got_b.to(gpu), noise=noise)
    for a, b in zip(want.target + want.residual, got.target + got.residual):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    rate = cfg.audio_codec.sample_rate
    same = model.separate(got_b, noise=noise, output_sampling_rate=rate)
    down = model.separate(got_b, noise=noise, output_sampling_rate=44100)
    for a, b, c in zip(got.target + got.residual, same.target + same.residual, down.target + down.residual):
        assert torch.equal(a, b)
        assert c.shape[-1] == -(-147 * a.shape[-1] // 160) and c.shape[:-1] == a.shape[:-1]
        assert torch.equal(c, audio.resample(a, rate, 44100))
        assert torch.isfinite(c).all() and float(c.abs().max()) > 0


def test_error_returns_reach_python(gpu):
    x = R.pcm_float(2, 100, seed=1).to(gpu)
    short = torch.empty(R.out_length(100, 44100, 48000) - 1, device=gpu)
    with pytest.raises(AssertionError, match="resample"):
        audio.mix_into(short, x, 2, 100, 100, 1, 44100, 48000)
    with pytest.raises(AssertionError, match="resample"):
        audio.mix_into(torch.empty(200, device=gpu), x, 0, 100, 100, 1, 44100, 48000)
    with pytest.raises(TypeError):
        audio.mix_into(torch.empty(200, device=gpu), x.double(), 2, 100, 100, 1, 44100, 48000)
    with pytest.raises(ValueError):
        audio.mix_into(torch.empty(200, device=gpu, dtype=torch.float64), x, 2, 100, 100, 1, 44100, 48000)
    with pytest.raises(ValueError):
        audio.resample(x, 0, 48000)
    bank, taps, first = audio.device_bank(44100, 48000, gpu)
    rc = hip.lib().samaudio_op_resample(hip.ptr(x), 7, 2, 100, 100, 1, hip.ptr(taps), hip.ptr(first), bank.n, bank.o, bank.K,
                                        hip.ptr(torch.empty(200, device=gpu)), 200, hip.current_stream_ptr())
    assert rc == hip.ERR_ARG and b"resample" in hip.lib().samaudio_last_error()
    with pytest.raises(ValueError):
        SAMAudioProcessor.from_config(preset_config("tiny"), audio_transform="hip")
