"""The CPU side of the audio front end (tests/test_audio_frontend_gpu.py holds the kernel to tests/resample_ref.py on the GPU):
the float64 direct form against processor.resample, the compact filter bank against processor.resample's dense one, the "torch"
processor with sampling_rates, the C-ABI / Python wiring, the argument refusals of the real library, and the GPU tests on the SIMT
simulator."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import wave

import pytest
import torch

from sam_audio_amd import SAMAudioProcessor, audio, hip, preset_config, processor
from tests import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_PAIRS = R.PAIRS + R.MORE_PAIRS
# the longest run of fp32-non-zero taps per pair, counted on processor.resample's dense bank when this change was made
LONGEST_RUN = {(44100, 48000): 13, (22050, 48000): 13, (16000, 48000): 13, (8000, 48000): 13, (32000, 48000): 13, (2, 3): 13,
               (48000, 44100): 14, (3, 2): 19, (96000, 48000): 25, (44100, 16000): 34, (48000, 16000): 37}


def _dense_bank(orig, new, lw=6, rolloff=0.99):
    """processor.resample's own float64 filter bank [n, 2 width + o], recovered from it as the response to unit impulses: an impulse at
    input c puts h(p, c - f o) at output f n + p, exactly (one product with 1, sums with 0).  Frame F = ceil(width / o) is the first
    whose taps all lie inside the signal."""
    o, n, _, width = R.geometry(orig, new, lw, rolloff)
    D, F = 2 * width + o, -(-width // o)
    y = processor.resample(torch.eye((F + 1) * o + D, dtype=torch.float64), orig, new, lw, rolloff)    # row c: an impulse at input c
    return y[F * o - width: F * o - width + D, F * n: (F + 1) * n].t().contiguous(), width


@pytest.mark.parametrize("orig,new", ALL_PAIRS)
def test_direct_form_agrees_with_processor_resample(orig, new):
    o, n = R.reduced(orig, new)
    worst = 0.0
    for channels, samples in ((1, 1), (2, 5), (3, 3 * o + 1), (2, 40 * o)):
        x = R.pcm_float(channels, samples, seed=samples).double()
        want = processor.resample(x, orig, new).mean(0)
        got = R.direct(x, orig, new)
        assert got.shape == want.shape == (R.out_length(samples, orig, new),)
        worst = max(worst, (got - want).abs().max().item())
        # a slice of the outputs is the same numbers
        a, b = got.numel() // 3, got.numel() // 3 + min(7, got.numel())
        assert torch.allclose(R.direct(x, orig, new, a, b), got[a:b], rtol=0, atol=1e-15)
    print(f"{orig} -> {new}: direct form against processor.resample {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("orig,new", ALL_PAIRS)
def test_filter_bank_is_the_dense_bank_rounded_to_fp32(orig, new):
    bank = audio.filter_bank(orig, new)
    dense, width = _dense_bank(orig, new)
    o, n = R.reduced(orig, new)
    assert (bank.o, bank.n) == (o, n) and bank.first.dtype == torch.int32 and bank.weights.dtype == torch.float32
    assert bank.weights.shape == (n, bank.K) and bank.first.shape == (n,)
    assert 1 <= bank.K <= 2 * width + 1
    assert bank.K == LONGEST_RUN[(orig, new)] == R.bank_figures(orig, new)[0]
    scattered = torch.zeros(n, dense.shape[1] + bank.K)
    cols = bank.first.long()[:, None] + width + torch.arange(bank.K)[None, :]
    assert int(cols.min()) >= 0
    scattered.scatter_(1, cols, bank.weights)
    assert torch.equal(scattered[:, : dense.shape[1]], dense.float())
    assert float(scattered[:, dense.shape[1]:].abs().max()) == 0.0          # nothing behind the statement's range
    assert bool((bank.weights[:, 0] != 0).all())                             # first[p] is the first non-zero tap
    assert 1.45 <= R.bank_figures(orig, new)[1] <= 1.87
    assert audio.filter_bank(orig * 3, new * 3) is bank                       # cached per reduced ratio


def test_filter_bank_sizes_and_refusal():
    bank = audio.filter_bank(47999, 48000)         # 2.3 G entries dense, 0.6 M compact
    assert (bank.o, bank.n) == (47999, 48000) and bank.n * bank.K <= audio.MAX_BANK_ELEMENTS // 4
    rows = torch.tensor([0, 1, 23999, 47999])      # (the dense float64 bank of this pair is what cannot be formed: four of its rows)
    want = R.weights64(47999, 48000, phases=rows).float()
    width = R.geometry(47999, 48000)[3]
    for p, row in zip(rows.tolist(), want):
        got = torch.zeros_like(row)
        lo = int(bank.first[p]) + width
        got[lo: lo + bank.K] = bank.weights[p]
        assert torch.equal(got, row), p
    with pytest.raises(ValueError, match="999983 -> 1000003"):
        audio.filter_bank(999983, 1000003)
    with pytest.raises(ValueError):
        audio.filter_bank(0, 48000)
    assert audio.resample_length(44100, 44100, 48000) == 48000 and audio.resample_length(1, 48000, 16000) == 1
    for samples in (1, 2, 146, 147, 148, 100003):
        assert audio.resample_length(samples, 44100, 48000) == math.ceil(160 * samples / 147) == R.out_length(samples, 44100, 48000)


def _write_wav(path, x_int16, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(x_int16.shape[0])
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(x_int16.t().contiguous().numpy().astype("<i2").tobytes())
    return str(path)


def test_torch_processor_with_sampling_rates_is_resample_then_batch_audio(tmp_path):
    cfg = preset_config("tiny")
    rate = cfg.audio_codec.sample_rate
    proc = SAMAudioProcessor.from_config(cfg)
    assert proc.audio_transform == "torch" and proc.device is None
    clips = [R.pcm_float(2, 3000, 1), R.pcm_float(1, 2500, 2), R.pcm_float(3, 901, 3)]
    rates = [44100, None, 16000]
    batch = proc(descriptions=["a", "b", "c"], audios=clips, sampling_rates=rates, anchors=[[("+", 0.0, 0.01)], [], []])
    want = [processor.resample(clips[0], 44100, rate), clips[1], processor.resample(clips[2], 16000, rate)]
    wavs, sizes = processor.batch_audio(want, rate)
    assert torch.equal(batch.audios, wavs) and torch.equal(batch.wav_sizes, sizes)
    assert sizes.tolist() == [R.out_length(3000, 44100, rate), 2500, R.out_length(901, 16000, rate)]
    assert torch.equal(batch.sizes, proc.wav_to_feature_idx(sizes))
    assert torch.equal(batch.audio_pad_mask, processor.mask_from_sizes(batch.sizes))
    # without sampling_rates (and with the model's rate spelled out): today's output
    plain = proc(descriptions=["a", "b", "c"], audios=clips)
    same = proc(descriptions=["a", "b", "c"], audios=clips, sampling_rates=[rate, None, rate])
    wavs, sizes = processor.batch_audio(clips, rate)
    for b in (plain, same):
        assert torch.equal(b.audios, wavs) and torch.equal(b.wav_sizes, sizes)
    # a WAV file keeps its own rate, whatever sampling_rates says about it
    pcm = R.pcm_int16(2, 1200, 4)
    path = _write_wav(tmp_path / "a.wav", pcm, 44100)
    b = proc(descriptions=["a"], audios=[path], sampling_rates=[8000])
    assert torch.equal(b.audios, processor.batch_audio([processor.resample(pcm.float() / 32768.0, 44100, rate)], rate)[0])
    with pytest.raises(ValueError):
        proc(descriptions=["a"], audios=[clips[0]], sampling_rates=[44100, 48000])


def test_header_and_python_wiring():
    header = open(os.path.join(ROOT, "include", "samaudio.h")).read()
    for name in ("samaudio_op_resample", "samaudio_resample_length"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in hip.EXPORTED_SYMBOLS
    for name, code in (("S16", 0), ("F32", 1)):
        assert re.search(r"#define\s+SAMAUDIO_PCM_%s\s+%d\b" % (name, code), header)
        assert getattr(hip, "PCM_" + name) == code
    assert "h(p, d) = sinc(pi t) cos^2(pi t / (2 lw)) base / o" in header          # the statement the kernel is held to
    kernels_h = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "kernels.h")).read()
    assert re.search(r"__attribute__\(\(weak\)\)\s+hipError_t\s+launch_resample_mix\(", kernels_h)
    cfg = preset_config("tiny")
    for make in (lambda **kw: SAMAudioProcessor(cfg.audio_codec.hop_length, cfg.audio_codec.sample_rate, **kw),
                 lambda **kw: SAMAudioProcessor.from_config(cfg, **kw)):
        assert make().audio_transform == "torch"
        p = make(audio_transform="hip", device="cuda:0")
        assert p.audio_transform == "hip" and p.device == torch.device("cuda:0")
        with pytest.raises(ValueError):
            make(audio_transform="hip")
        with pytest.raises(ValueError):
            make(audio_transform="bogus")
    import inspect
    from sam_audio_amd import SAMAudio
    assert inspect.signature(SAMAudio.separate).parameters["output_sampling_rate"].default is None
    assert {"audio_transform", "device"} <= set(inspect.signature(SAMAudioProcessor.from_pretrained).parameters)
    x = torch.zeros(2, 8)
    assert audio.resample(x, 48000, 48000) is x                                  # equal rates: the argument, on any device
    with pytest.raises(hip.SamAudioHipError):
        audio.resample(x, 44100, 48000)                                          # no CPU fallback


def test_library_refuses_bad_resample_arguments_without_a_gpu():
    """argument validation happens before any launch, so it is checked on the real library here"""
    lib = hip.lib()
    buf = (C.c_float * 64)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)

    def call(pcm=p, fmt=hip.PCM_F32, channels=1, samples=10, taps=p, first=p, phases=3, step=2, k=13, out=p, capacity=15):
        return lib.samaudio_op_resample(pcm, fmt, channels, samples, 1, 1, taps, first, phases, step, k, out, capacity, None)

    for kw in (dict(pcm=null), dict(taps=null), dict(first=null), dict(out=null), dict(channels=0), dict(samples=0), dict(step=0),
               dict(phases=0), dict(k=0), dict(fmt=2), dict(fmt=-1), dict(capacity=14)):
        assert call(**kw) == hip.ERR_ARG, kw
        assert b"resample" in lib.samaudio_last_error(), kw
    assert lib.samaudio_resample_length(10, 2, 3) == 15 and lib.samaudio_resample_length(3, 441, 160) == 2
    assert lib.samaudio_resample_length(13_500_000, 441, 160) == math.ceil(160 * 13_500_000 / 441)
    assert lib.samaudio_resample_length(0, 2, 3) == -1 and lib.samaudio_resample_length(5, 0, 3) == -1


def test_audio_kernel_on_the_simulator():
    """tests/test_audio_frontend_gpu.py on the SIMT simulator (the real kernel code compiled for the host, as tests/test_simt_cpu.py runs
    its selections): every rate pair, length, channel count, format and layout, the impulses, the bitwise invariance, the processor
    end to end and the error returns.  (The 13.5 M sample clip and separate() run on the GPU only.)"""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_audio_frontend_gpu.py", "-k", "not long and not separate"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail
