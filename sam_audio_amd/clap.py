"""CLAP's log-mel front end on the GPU (csrc/kernels.hip clap_logmel_kernel, include/samaudio.h samaudio_op_logmel, DESIGN.md section
10.8): what `transformers.ClapFeatureExtractor(truncation="rand_trunc", padding="repeatpad")` computes for a clip - repeatpad or crop
to `max_length`, centred reflect-padded STFT with the periodic Hann window, power, mel filter bank, dB - with the reference ranker's
int16 round trip in front (sam_audio/ranking/clap.py:50-52), in one launch per group of equally long rows.

Its CPU statement is tests/clap_ref.py (float64, the same signature as `logmel`), pinned to ClapFeatureExtractor itself; it is
unpinned vs laion_clap, which is not part of this build's environment: the int16 constant (samaudio.h SAMAUDIO_CLAP_INT16_SCALE) and
laion's `fmin` are taken on trust, and a clip longer than `max_length` is cropped at the offset the caller names (default 0, the
head), where the extractor draws the offset at random.  Everything the kernel needs that takes a transcendental function on the host -
the window, the FFT twiddles, the filter bank - is evaluated here in float64 and uploaded once.  There is no CPU fallback.

Behind the front end, `ClapTower` binds the HTSAT audio tower and the RoBERTa text tower of `transformers.ClapModel` (csrc/clap.hip,
csrc/clap_kernels.hip; fp32 only, no feature fusion): `ranking.ClapRanker` scores candidates with them.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import torch

from . import hip
from .context import Context

SAMPLE_RATE = 48_000
MAX_LENGTH = 480_000       # 10 s
FFT_SIZE, HOP, N_MELS = 1024, 480, 64
INT16_SCALE = 32767.0      # samaudio.h SAMAUDIO_CLAP_INT16_SCALE

_device_tables: Dict[tuple, torch.Tensor] = {}
_banks: Dict[tuple, torch.Tensor] = {}


def check_fft_size(fft_size: int) -> int:
    fft_size = int(fft_size)
    if fft_size < 64 or fft_size > 2048 or fft_size & (fft_size - 1):
        raise ValueError(f"fft_size must be a power of two in [64, 2048], got {fft_size}")
    return fft_size


def logmel_tables(fft_size: int) -> torch.Tensor:
    """fp32 [2 N]: the periodic Hann window [N], then (cos, -sin)(2 pi t / N) interleaved for t < N / 2; evaluated in float64"""
    n = check_fft_size(fft_size)
    j = torch.arange(n, dtype=torch.float64)
    window = 0.5 - 0.5 * torch.cos(2 * math.pi * j / n)
    t = 2 * math.pi * torch.arange(n // 2, dtype=torch.float64) / n
    twiddle = torch.stack([torch.cos(t), -torch.sin(t)], dim=1).reshape(-1)
    return torch.cat([window, twiddle]).float()


def mel_bank(fft_size: int = FFT_SIZE, n_mels: int = N_MELS, sample_rate: int = SAMPLE_RATE, fmin: float = 0.0,
             fmax: float = 14_000.0, form: str = "slaney") -> torch.Tensor:
    """float64 [N / 2 + 1, n_mels]: ClapFeatureExtractor's `mel_filters_slaney` ("slaney": what rand_trunc uses, and the ranker) or
    `mel_filters` ("htk": what fusion uses), by transformers' own `mel_filter_bank`.  Cached per argument tuple."""
    if form not in ("slaney", "htk"):
        raise ValueError(f"form must be 'slaney' or 'htk', got {form!r}")
    key = (check_fft_size(fft_size), int(n_mels), int(sample_rate), float(fmin), float(fmax), form)
    if key not in _banks:
        from transformers.audio_utils import mel_filter_bank
        bank = mel_filter_bank(num_frequency_bins=key[0] // 2 + 1, num_mel_filters=key[1], min_frequency=key[3], max_frequency=key[4],
                               sampling_rate=key[2], norm="slaney" if form == "slaney" else None, mel_scale=form)
        _banks[key] = torch.from_numpy(bank).double()
    return _banks[key]


def frames(max_length: int, hop: int) -> int:
    """1 + max_length // hop: the centred STFT of a clip padded or cropped to max_length"""
    if max_length < 1 or hop < 1:
        raise ValueError("max_length and hop must be positive")
    return 1 + int(max_length) // int(hop)


def _rows(wav: torch.Tensor) -> torch.Tensor:
    """[rows, n] fp32 whose rows are contiguous in time and do not overlap; a view is kept where it already is one"""
    if wav.dim() == 1:
        wav = wav[None]
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[1] < 1:
        raise ValueError(f"logmel needs waveforms [rows, samples] with at least one row and one sample, got {tuple(wav.shape)}")
    if wav.dtype != torch.float32:
        wav = wav.float()
    if wav.stride(1) != 1 or (wav.shape[0] > 1 and wav.stride(0) < wav.shape[1]):
        wav = wav.contiguous()
    return wav


def _device_f32(t, device) -> torch.Tensor:
    t = torch.as_tensor(t)
    return t.to(device=device, dtype=torch.float32).contiguous()


def logmel(wav: torch.Tensor, lengths: Optional[Sequence[int]] = None, offsets: Optional[Sequence[int]] = None,
           max_length: int = MAX_LENGTH, fft_size: int = FFT_SIZE, hop: int = HOP, bank=None, quantise: bool = True,
           bn_scale=None, bn_shift=None) -> torch.Tensor:
    """dB features [rows, 1 + max_length // hop, n_mels] fp32 on the device of `wav` ([rows, n] or [n], fp32; a strided view whose rows
    are contiguous in time is read in place).  Row r is the clip wav[r, :lengths[r]] (default: the whole row): shorter than `max_length`
    it is repeated int(max_length / n) times and zero padded, longer it is cropped at offsets[r] (default 0).  `bank`
    [fft_size / 2 + 1, n_mels] is the mel filter bank (default: `mel_bank()` of this fft_size, CLAP's); `quantise` applies the int16
    round trip; `bn_scale` / `bn_shift` [n_mels] are applied to the dB values where given.  Nothing is read back."""
    fft_size = check_fft_size(fft_size)
    n_frames = frames(max_length, hop)
    hip.require_gpu(wav.device, "clap.logmel")
    x = _rows(wav)
    rows, samples = x.shape
    device = x.device
    lens = [samples] * rows if lengths is None else [int(v) for v in lengths]
    offs = [0] * rows if offsets is None else [int(v) for v in offsets]
    if len(lens) != rows or len(offs) != rows:
        raise ValueError(f"{rows} rows but {len(lens)} lengths and {len(offs)} offsets")
    if any(v > samples for v in lens):
        raise ValueError("a length above the number of samples of a row")
    bank = mel_bank(fft_size) if bank is None else bank
    bank = _device_f32(bank, device)
    if bank.dim() != 2 or bank.shape[0] != fft_size // 2 + 1:
        raise ValueError(f"bank must be [fft_size / 2 + 1, n_mels], got {tuple(bank.shape)}")
    n_mels = int(bank.shape[1])
    if (bn_scale is None) != (bn_shift is None):
        raise ValueError("bn_scale and bn_shift go together")
    if bn_scale is not None:
        bn_scale, bn_shift = _device_f32(bn_scale, device), _device_f32(bn_shift, device)
        if tuple(bn_scale.shape) != (n_mels,) or tuple(bn_shift.shape) != (n_mels,):
            raise ValueError("bn_scale and bn_shift must be [n_mels]")
    key = (fft_size, str(device))
    if key not in _device_tables:
        _device_tables[key] = logmel_tables(fft_size).to(device)
    out = torch.empty(rows, n_frames, n_mels, dtype=torch.float32, device=device)
    lib = hip.lib()
    with torch.cuda.device(device):
        hip.check(lib.samaudio_op_logmel(C.c_void_p(x.data_ptr()), rows, x.stride(0) if rows > 1 else samples,
                                         (C.c_int64 * rows)(*lens), (C.c_int64 * rows)(*offs), int(max_length), int(bool(quantise)),
                                         fft_size, int(hop), n_mels, hip.ptr(_device_tables[key]), hip.ptr(bank), hip.ptr(bn_scale),
                                         hip.ptr(bn_shift), hip.ptr(out), hip.current_stream_ptr()))
    return out


def fold_batch_norm(weight, bias, running_mean, running_var, eps: float = 1e-5):
    """(scale, shift) float64 [n_mels] of an eval-mode BatchNorm2d over the mel bins (`ClapAudioEncoder.batch_norm`):
    y = (x - mean) / sqrt(var + eps) * weight + bias = x * scale + shift"""
    w, b, m, v = (torch.as_tensor(t).detach().double().cpu() for t in (weight, bias, running_mean, running_var))
    scale = w / torch.sqrt(v + eps)
    return scale, b - m * scale


# ---- the towers (csrc/clap.hip, samaudio.h "CLAP ranker towers") --------------------------------------------------------------------

def relative_position_index(window: int) -> torch.Tensor:
    """[window^2, window^2] int64: row (iy - jy + window - 1) (2 window - 1) + (ix - jx + window - 1) of the bias table for query i, key j
    (`ClapAudioSelfAttention.create_relative_position_index`).  swin_window_attn_kernel evaluates this expression in place; a checkpoint's
    `relative_position_index` buffer is checked against it at load."""
    c = torch.arange(window)
    y, x = torch.meshgrid(c, c, indexing="ij")
    y, x = y.reshape(-1), x.reshape(-1)
    return (y[:, None] - y[None, :] + window - 1) * (2 * window - 1) + (x[:, None] - x[None, :] + window - 1)


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


def tower_config(config, frontend: Optional[dict] = None) -> "hip.ClapConfig":
    """`samaudio_clap_config` of a `transformers.ClapConfig` (or its dict) and a `ClapFeatureExtractor`'s settings (`frontend`: the
    keys of preprocessor_config.json; missing ones take the extractor's defaults)."""
    a, t, fe = _get(config, "audio_config"), _get(config, "text_config"), dict(frontend or {})
    problems = []
    if _get(a, "enable_fusion", False):
        problems.append("enable_fusion=True (feature fusion)")
    if _get(a, "hidden_act", "gelu") != "gelu" or _get(t, "hidden_act", "gelu") != "gelu":
        problems.append("hidden_act other than 'gelu'")
    if _get(config, "projection_hidden_act", "relu") != "relu" or _get(a, "projection_hidden_act", "relu") != "relu":
        problems.append("projection_hidden_act other than 'relu'")
    if _get(a, "patch_embed_input_channels", 1) != 1 or not _get(a, "flatten_patch_embeds", True):
        problems.append("patch_embed_input_channels != 1 or flatten_patch_embeds=False")
    if float(_get(a, "mlp_ratio", 4.0)) != int(_get(a, "mlp_ratio", 4.0)):
        problems.append("a fractional mlp_ratio")
    depths, heads = list(_get(a, "depths")), list(_get(a, "num_attention_heads"))
    if len(depths) != len(heads) or not 1 <= len(depths) <= 4:
        problems.append("more than 4 stages")
    if _get(a, "hidden_size") != _get(a, "patch_embeds_hidden_size") << (len(depths) - 1):
        problems.append("audio hidden_size != patch_embeds_hidden_size * 2^(stages - 1)")
    if problems:
        raise NotImplementedError("ClapConfig outside what the HIP towers build: " + "; ".join(problems))
    rate = int(fe.get("sampling_rate", SAMPLE_RATE))
    c = hip.ClapConfig(
        fft_size=int(fe.get("fft_window_size", FFT_SIZE)), hop=int(fe.get("hop_length", HOP)),
        max_length=int(fe.get("nb_max_samples", int(fe.get("max_length_s", 10)) * rate)),
        spec_size=_get(a, "spec_size"), num_mel_bins=_get(a, "num_mel_bins"), patch_size=_get(a, "patch_size"),
        patch_stride=_get(a, "patch_stride")[0] if isinstance(_get(a, "patch_stride"), (list, tuple)) else _get(a, "patch_stride"),
        embed_dim=_get(a, "patch_embeds_hidden_size"), num_stages=len(depths), window_size=_get(a, "window_size"),
        mlp_ratio=int(_get(a, "mlp_ratio", 4.0)), patch_norm=int(bool(_get(a, "enable_patch_layer_norm", True))), enable_fusion=0,
        audio_ln_eps=float(_get(a, "layer_norm_eps", 1e-5)),
        text_vocab=_get(t, "vocab_size"), text_hidden=_get(t, "hidden_size"), text_heads=_get(t, "num_attention_heads"),
        text_layers=_get(t, "num_hidden_layers"), text_intermediate=_get(t, "intermediate_size"),
        text_max_positions=_get(t, "max_position_embeddings"), text_pad_id=_get(t, "pad_token_id", 1),
        text_ln_eps=float(_get(t, "layer_norm_eps", 1e-12)), projection_dim=_get(config, "projection_dim"))
    for i, (d, h) in enumerate(zip(depths, heads)):
        c.depths[i], c.heads[i] = int(d), int(h)
    return c


def convert_clap(sd: Dict[str, torch.Tensor], c: "hip.ClapConfig", frontend: dict, device) -> Dict[str, torch.Tensor]:
    """ClapModel.state_dict() (Hugging Face key names) -> the engine tensors of csrc/clap.hip, fp32 on `device`:
      fe.tables / fe.bank / fe.bn_scale / fe.bn_shift   the front end's tables, the mel bank, audio_encoder.batch_norm folded
      a.patch.{w, b, ln_w, ln_b}                         audio_encoder.patch_embed.{proj, norm}
      a.S<s>.B<i>.{ln1_*, wqkv, bqkv, rpb, wo, bo, ln2_*, w1, b1, w2, b2}
                                                         layers.<s>.blocks.<i>.{layernorm_before, attention.self.{query | key | value},
                                                         attention.self.relative_position_bias_table, attention.output.dense,
                                                         layernorm_after, intermediate.dense, output.dense}
      a.S<s>.merge.{ln_w, ln_b, w}                       layers.<s>.downsample.{norm, reduction}
      a.norm_{w, b}, a.proj.{w1, b1, w2, b2}             audio_encoder.norm, audio_projection.{linear1, linear2}
      t.word / t.pos / t.type / t.emb_ln_{w, b}          text_model.embeddings (type: row 0 of token_type_embeddings)
      t.L<i>.{wqkv, bqkv, wo, bo, ln1_*, w1, b1, w2, b2, ln2_*}
                                                         encoder.layer.<i>.{attention.self, attention.output.{dense, LayerNorm},
                                                         intermediate.dense, output.{dense, LayerNorm}}
      t.pool.{w, b}, t.proj.{w1, b1, w2, b2}             text_model.pooler.dense, text_projection.{linear1, linear2}"""
    f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()   # noqa: E731
    out: Dict[str, torch.Tensor] = {}

    def lin(dst_w, dst_b, src, rows=None):
        out[dst_w] = f32(sd[src + ".weight"])
        b = sd.get(src + ".bias")
        out[dst_b] = f32(b) if b is not None else torch.zeros(out[dst_w].shape[0], dtype=torch.float32, device=device)

    def fused_qkv(dst, src):
        out[dst + "wqkv"] = f32(torch.cat([sd[f"{src}.{n}.weight"] for n in ("query", "key", "value")]))
        dim = sd[f"{src}.query.weight"].shape[0]
        out[dst + "bqkv"] = f32(torch.cat([sd.get(f"{src}.{n}.bias", torch.zeros(dim)) for n in ("query", "key", "value")]))

    def norm(dst, src):
        out[dst + "_w"], out[dst + "_b"] = f32(sd[src + ".weight"]), f32(sd[src + ".bias"])

    ae = "audio_model.audio_encoder."
    rate = int(frontend.get("sampling_rate", SAMPLE_RATE))
    out["fe.tables"] = logmel_tables(c.fft_size).to(device)
    out["fe.bank"] = f32(mel_bank(c.fft_size, c.num_mel_bins, rate, float(frontend.get("frequency_min", 0.0)),
                                  float(frontend.get("frequency_max", 14_000.0))))
    scale, shift = fold_batch_norm(*(sd[ae + "batch_norm." + n] for n in ("weight", "bias", "running_mean", "running_var")))
    out["fe.bn_scale"], out["fe.bn_shift"] = f32(scale), f32(shift)
    out["a.patch.w"] = f32(sd[ae + "patch_embed.proj.weight"].reshape(c.embed_dim, -1))
    out["a.patch.b"] = f32(sd[ae + "patch_embed.proj.bias"])
    if c.patch_norm:
        out["a.patch.ln_w"], out["a.patch.ln_b"] = f32(sd[ae + "patch_embed.norm.weight"]), f32(sd[ae + "patch_embed.norm.bias"])
    index = relative_position_index(c.window_size)
    for s in range(c.num_stages):
        for i in range(c.depths[s]):
            src, dst = f"{ae}layers.{s}.blocks.{i}.", f"a.S{s}.B{i}."
            norm(dst + "ln1", src + "layernorm_before")
            fused_qkv(dst, src + "attention.self")
            out[dst + "rpb"] = f32(sd[src + "attention.self.relative_position_bias_table"])
            stored = sd.get(src + "attention.self.relative_position_index")
            if stored is not None and not torch.equal(stored.cpu().long(), index):
                raise RuntimeError(f"{src}attention.self.relative_position_index is not the window's index the kernel evaluates")
            lin(dst + "wo", dst + "bo", src + "attention.output.dense")
            norm(dst + "ln2", src + "layernorm_after")
            lin(dst + "w1", dst + "b1", src + "intermediate.dense")
            lin(dst + "w2", dst + "b2", src + "output.dense")
        if s + 1 < c.num_stages:
            src, dst = f"{ae}layers.{s}.downsample.", f"a.S{s}.merge."
            out[dst + "ln_w"], out[dst + "ln_b"] = f32(sd[src + "norm.weight"]), f32(sd[src + "norm.bias"])
            out[dst + "w"] = f32(sd[src + "reduction.weight"])
    norm("a.norm", ae + "norm")
    lin("a.proj.w1", "a.proj.b1", "audio_projection.linear1")
    lin("a.proj.w2", "a.proj.b2", "audio_projection.linear2")
    te = "text_model.embeddings."
    out["t.word"], out["t.pos"] = f32(sd[te + "word_embeddings.weight"]), f32(sd[te + "position_embeddings.weight"])
    out["t.type"] = f32(sd[te + "token_type_embeddings.weight"][0])
    norm("t.emb_ln", te + "LayerNorm")
    for i in range(c.text_layers):
        src, dst = f"text_model.encoder.layer.{i}.", f"t.L{i}."
        fused_qkv(dst, src + "attention.self")
        lin(dst + "wo", dst + "bo", src + "attention.output.dense")
        norm(dst + "ln1", src + "attention.output.LayerNorm")
        lin(dst + "w1", dst + "b1", src + "intermediate.dense")
        lin(dst + "w2", dst + "b2", src + "output.dense")
        norm(dst + "ln2", src + "output.LayerNorm")
    lin("t.pool.w", "t.pool.b", "text_model.pooler.dense")
    lin("t.proj.w1", "t.proj.b1", "text_projection.linear1")
    lin("t.proj.w2", "t.proj.b2", "text_projection.linear2")
    return out


def load_checkpoint(path: str):
    """(config dict, preprocessor dict, state dict) of a local `ClapModel.save_pretrained` directory.  laion_clap's own `.pt` files
    carry other key names, which cannot be checked in this environment: they are refused, not renamed from memory."""
    import json
    import os
    path = os.fspath(path)
    if os.path.isfile(path) or path.endswith((".pt", ".pth", ".ckpt")):
        raise ValueError(f"{path}: a laion_clap .pt checkpoint is not read here - convert it with transformers' converter "
                         "(transformers/models/clap/convert_clap_original_pytorch_to_hf.py) and pass the directory that "
                         "ClapModel.save_pretrained wrote")
    cfg_file = os.path.join(path, "config.json")
    if not os.path.isdir(path) or not os.path.exists(cfg_file):
        raise FileNotFoundError(f"{path}: not a local ClapModel.save_pretrained directory (no config.json)")
    with open(cfg_file) as f:
        config = json.load(f)
    frontend = {}
    if os.path.exists(os.path.join(path, "preprocessor_config.json")):
        with open(os.path.join(path, "preprocessor_config.json")) as f:
            frontend = json.load(f)
    st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.exists(pt):
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{path}: neither model.safetensors nor pytorch_model.bin")
    return config, frontend, sd


class ClapTower(Context):
    """The two CLAP towers on the HIP library: `audio_embed(wavs, sample_rate) -> [rows, projection_dim]`,
    `text_embed(input_ids, attention_mask) -> [rows, projection_dim]` (both unit norm, fp32, on the device), `logmel(wavs)` - the
    front end alone with this checkpoint's BatchNorm folded in - and `score(audio, text, candidates)`.  Owns its workspace."""

    def __init__(self, config, frontend: Optional[dict] = None, device: Optional[str] = None):
        self.frontend = dict(frontend or {})
        self.cfg = tower_config(config, self.frontend)
        self.device = torch.device(device) if device is not None else None
        super().__init__(hip.clap_lib(), "samaudio_clap", self.cfg, device=self.device)

    @property
    def sample_rate(self) -> int:
        return int(self.frontend.get("sampling_rate", SAMPLE_RATE))

    @property
    def dim(self) -> int:
        return int(self.cfg.projection_dim)

    @classmethod
    def from_module(cls, module, device, frontend: Optional[dict] = None) -> "ClapTower":
        """from a `transformers.ClapModel` (its config and weights) and, optionally, a ClapFeatureExtractor's `to_dict()`"""
        tower = cls(module.config, frontend, device=str(device))
        tower.load_state_dict(module.state_dict())
        return tower

    @classmethod
    def from_pretrained(cls, path: str, device=None) -> "ClapTower":
        config, frontend, sd = load_checkpoint(path)
        tower = cls(config, frontend, device=None if device is None else str(device))
        tower.load_state_dict(sd)
        return tower

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor]) -> None:
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        hip.require_gpu(self.device, "ClapTower")
        with torch.cuda.device(self.device):
            self.register(convert_clap(state_dict, self.cfg, self.frontend, self.device))
            self.finalize()

    _ensure = Context.ensure_workspace   # (audio rows, text rows, tokens)

    def _ready(self) -> None:
        if not self._loaded:
            raise hip.SamAudioHipError("ClapTower: no weights loaded")

    def _at_rate(self, wavs: torch.Tensor, sample_rate: int) -> torch.Tensor:
        if int(sample_rate) == self.sample_rate:
            return wavs
        from . import audio
        return audio.resample(wavs, int(sample_rate), self.sample_rate)

    @torch.inference_mode()
    def logmel(self, wavs: torch.Tensor, sample_rate: Optional[int] = None, lengths=None, offsets=None, quantise: bool = True,
               normalise: bool = True) -> torch.Tensor:
        """[rows, frames, n_mels]: what the audio tower reads (`normalise`: with the BatchNorm folded in)"""
        self._ready()
        wavs = self._at_rate(wavs, self.sample_rate if sample_rate is None else sample_rate)
        bn = dict(bn_scale=self._tensors["fe.bn_scale"], bn_shift=self._tensors["fe.bn_shift"]) if normalise else {}
        return logmel(wavs, lengths, offsets, max_length=self.cfg.max_length, fft_size=self.cfg.fft_size, hop=self.cfg.hop,
                      bank=self._tensors["fe.bank"], quantise=quantise, **bn)

    @torch.inference_mode()
    def audio_embed(self, wavs: torch.Tensor, sample_rate: Optional[int] = None, lengths=None, offsets=None, quantise: bool = True,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[rows, projection_dim]: `wavs` [rows, n] (or [n]) on the device, a strided view whose rows are contiguous in time is read in
        place; row r is the clip wavs[r, :lengths[r]], cropped at offsets[r] where it is longer than max_length (default 0, the head)"""
        self._ready()
        x = _rows(self._at_rate(wavs, self.sample_rate if sample_rate is None else sample_rate))
        hip.require_gpu(x.device, "ClapTower.audio_embed")
        rows, samples = x.shape
        lens = [samples] * rows if lengths is None else [int(v) for v in lengths]
        offs = [0] * rows if offsets is None else [int(v) for v in offsets]
        if len(lens) != rows or len(offs) != rows or any(v > samples for v in lens):
            raise ValueError("lengths / offsets must name every row, and no length may pass the row")
        with torch.cuda.device(self.device):
            res = out if out is not None else torch.empty(rows, self.dim, dtype=torch.float32, device=self.device)
            if res.dtype != torch.float32 or tuple(res.shape) != (rows, self.dim) or not res.is_contiguous():
                raise ValueError("out must be a contiguous fp32 [rows, projection_dim] tensor")
            self._ensure(rows, 0, 0)
            hip.check(self._lib.samaudio_clap_audio_embed(self._h, C.c_void_p(x.data_ptr()), rows, x.stride(0) if rows > 1 else samples,
                                                          (C.c_int64 * rows)(*lens), (C.c_int64 * rows)(*offs), int(bool(quantise)),
                                                          hip.ptr(res), hip.current_stream_ptr()))
        return res

    @torch.inference_mode()
    def text_embed(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[rows, projection_dim] of token rows [rows, tokens] (attention_mask None: every token counts)"""
        self._ready()
        assert input_ids.dim() == 2, "input_ids must be [rows, tokens]"
        rows, tokens = input_ids.shape
        ids_host = input_ids.detach().to("cpu", torch.int64)
        if rows and tokens and (int(ids_host.min()) < 0 or int(ids_host.max()) >= self.cfg.text_vocab):
            raise IndexError(f"token id outside [0, {self.cfg.text_vocab})")
        with torch.cuda.device(self.device):
            ids = input_ids.to(self.device, torch.int64).contiguous()
            mask = (torch.ones_like(ids, dtype=torch.uint8) if attention_mask is None
                    else (attention_mask.to(self.device) != 0).to(torch.uint8).contiguous())
            out = torch.empty(rows, self.dim, dtype=torch.float32, device=self.device)
            self._ensure(0, rows, tokens)
            hip.check(self._lib.samaudio_clap_text_embed(self._h, hip.ptr(ids), hip.ptr(mask), rows, tokens, hip.ptr(out),
                                                         hip.current_stream_ptr()))
        return out

    @torch.inference_mode()
    def score(self, audio: torch.Tensor, text: torch.Tensor, candidates: int) -> torch.Tensor:
        """[clips, candidates] = <audio [clips * candidates, dim], text [clips, dim]>"""
        clips = text.shape[0]
        assert audio.shape == (clips * candidates, self.dim) and text.shape == (clips, self.dim)
        out = torch.empty(clips, candidates, dtype=torch.float32, device=audio.device)
        with torch.cuda.device(self.device):
            hip.check(self._lib.samaudio_clap_score(hip.ptr(audio), hip.ptr(text), clips, candidates, self.dim, hip.ptr(out),
                                                    hip.current_stream_ptr()))
        return out
