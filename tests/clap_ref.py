"""CPU statement of CLAP's log-mel front end (include/samaudio.h samaudio_op_logmel, sam_audio_amd/clap.py logmel, DESIGN.md section
10.8): `logmel` here has the signature of `sam_audio_amd.clap.logmel` and evaluates the same definition with torch on the CPU, in
float64 by default.  tests/test_clap_cpu.py pins it to `transformers.ClapFeatureExtractor(truncation="rand_trunc",
padding="repeatpad")` itself; it is unpinned vs laion_clap (absent): the int16 constant and the random crop are not checked against it.

`dtype=torch.float32` evaluates the same statement in float32 throughout (torch.stft + matmul): the yardstick the GPU test derives its
dB bound from.  The int16 round trip is float32 arithmetic in either mode - that IS its definition (laion_clap does it on float32
tensors): x 32767 rounded to float32 decides which integer the truncation lands on.
"""
import math

import torch

from sam_audio_amd import clap

INT16_SCALE = clap.INT16_SCALE


def int16_round_trip(x: torch.Tensor) -> torch.Tensor:
    """laion_clap's int16_to_float32_torch(float32_to_int16_torch(x)) on a float32 tensor"""
    q = (torch.clamp(x.float(), min=-1.0, max=1.0) * INT16_SCALE).to(torch.int16)   # (the cast truncates toward zero)
    return (q / INT16_SCALE).to(torch.float32)


def fit(x: torch.Tensor, max_length: int, offset: int = 0) -> torch.Tensor:
    """feature_extraction_clap.py:204-258 for truncation="rand_trunc", padding="repeatpad", with the crop offset named"""
    n = x.numel()
    if n > max_length:
        assert 0 <= offset <= n - max_length
        return x[offset: offset + max_length]
    if n < max_length:
        x = x.repeat(int(max_length / n))
        x = torch.cat([x, x.new_zeros(max_length - x.numel())])
    return x


def logmel(wav, lengths=None, offsets=None, max_length=clap.MAX_LENGTH, fft_size=clap.FFT_SIZE, hop=clap.HOP, bank=None,
           quantise=True, bn_scale=None, bn_shift=None, dtype=torch.float64):
    """[rows, 1 + max_length // hop, n_mels] in `dtype` on the CPU; arguments as sam_audio_amd.clap.logmel"""
    wav = torch.as_tensor(wav).detach().cpu().float()
    wav = wav[None] if wav.dim() == 1 else wav
    rows, samples = wav.shape
    lengths = [samples] * rows if lengths is None else list(lengths)
    offsets = [0] * rows if offsets is None else list(offsets)
    bank = clap.mel_bank(fft_size) if bank is None else torch.as_tensor(bank)
    bank = bank.float().to(dtype)        # the kernel reads the bank rounded to float32
    j = torch.arange(fft_size, dtype=torch.float64)
    window = (0.5 - 0.5 * torch.cos(2 * math.pi * j / fft_size)).float().to(dtype)   # ... and the window
    out = []
    for r in range(rows):
        x = wav[r, : int(lengths[r])]
        if quantise:
            x = int16_round_trip(x)
        y = fit(x, int(max_length), int(offsets[r])).to(dtype)
        spec = torch.stft(y, fft_size, hop_length=hop, win_length=fft_size, window=window, center=True, pad_mode="reflect",
                          return_complex=True)                      # [bins, frames]
        power = spec.real ** 2 + spec.imag ** 2
        mel = power.T @ bank
        db = torch.where(mel > 1e-10, 10.0 * torch.log10(mel.clamp(min=1e-10)), torch.full_like(mel, -100.0))
        if bn_scale is not None:
            db = db * torch.as_tensor(bn_scale).float().to(dtype) + torch.as_tensor(bn_shift).float().to(dtype)
        out.append(db)
    return torch.stack(out)
