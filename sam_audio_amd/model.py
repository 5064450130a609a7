"""`SAMAudio` - drop-in host class for the reference's SAMAudio.separate() path
(reference sam_audio/model/model.py:75-359), backed by libsamaudio_hip.so.

PyTorch-ROCm is used for device memory, streams, RNG and weight plumbing only; every arithmetic step
of separate() - DAC-VAE encode, the 32 DiT evaluations of the midpoint ODE, DAC-VAE decode - runs in
hand-written HIP kernels behind the C ABI of include/samaudio.h.  No eager/CPU fallback exists.
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import math
import os
import warnings
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional

import torch

from . import hip
from .config import SAMAudioConfig
from .context import Context, scratch
from .processor import Batch
from .weights import (F32_SOURCE_KEYS, convert_codec, convert_codec_fly16, convert_codec_x3, convert_dit, convert_dit_f32, convert_dit_x3,
                      split_missing_unexpected)

DFLT_ODE_OPT = {"method": "midpoint", "options": {"step_size": 2 / 32}}  # reference model.py:22
# Layout of the five big DiT weight matrices and the next-weights prefetch of few-row launches (SAMAudio.__init__; DESIGN.md
# section 7 has the measurements behind the defaults).  Environment overrides (tuning): SAMAUDIO_WEIGHT_LAYOUT,
# SAMAUDIO_PREFETCH_ROWS.
DEFAULT_WEIGHT_LAYOUT = "ktm"
DEFAULT_PREFETCH_ROWS = 2048


@dataclass
class SeparationResult:  # reference model.py:68-72
    target: List[torch.Tensor]
    residual: List[torch.Tensor]
    noise: torch.Tensor


# torchdiffeq's fixed-grid solvers the engine runs (samaudio.h SAMAUDIO_ODE_*), and the two adaptive pairs.  torchdiffeq's adaptive
# solvers size every step from the error norm of the whole batch, so a row's result would depend on which rows share the call
# (sharding, streams=2 and the candidate repeat rely on rows being independent); here every row carries its own time, step and error
# norm on the device instead (`ode_adaptive` below): pinned to scipy's RK45 / RK23, unpinned vs torchdiffeq.
# The other adaptive methods and the Adams family cannot be restated without their source: DESIGN.md section 1 row a6.
ODE_METHODS = {"euler": hip.ODE_EULER, "midpoint": hip.ODE_MIDPOINT, "rk4": hip.ODE_RK4, "heun3": hip.ODE_HEUN3}
ODE_ADAPTIVE_METHODS = {"dopri5": hip.ODE_DOPRI5, "bosh3": hip.ODE_BOSH3}
# options of the adaptive methods (torchdiffeq's names) and their defaults: scipy's SAFETY / MAX_FACTOR / MIN_FACTOR
ODE_ADAPTIVE_OPTIONS = {"first_step": None, "safety": 0.9, "ifactor": 10.0, "dfactor": 0.2, "max_num_steps": 2 ** 31 - 1}


def is_adaptive(ode_opt: Dict[str, Any]) -> bool:
    return ode_opt.get("method", "midpoint") in ODE_ADAPTIVE_METHODS


def ode_adaptive(ode_opt: Dict[str, Any], windowed: bool = False):
    """(method id, hip.OdeAdaptive) for `ode_opt` = {"method": "dopri5" | "bosh3", "rtol": r, "atol": a, "options": {...}}, the shape
    torchdiffeq.odeint takes (reference model.py:285-290).  The solver is this build's own: embedded Runge-Kutta pairs with PER-ROW step
    control, pinned to scipy's RK45 / RK23 (tableaux, controller, initial step) and unpinned vs torchdiffeq, from which it differs in
    three known ways - the error norm and the step are per row, not per call (identical for one row); the last step is clipped to
    t1 instead of stepping past it and interpolating back; the accept factor is capped at 1 after a rejection within the same step -
    so the two agree to O(tolerance), no closer.
    rtol, atol: required, positive.  options: first_step (default: scipy's select_initial_step, one more field evaluation), safety
    (0.9), ifactor (10), dfactor (0.2), max_num_steps (trial steps per row).  Everything else - other keys, missing tolerances, a
    windowed solve (`windowed`: window_seconds= without separate()'s step_control="clip", which steps per clip instead of per row:
    DESIGN.md section 10.11) - is a ValueError."""
    method = ode_opt.get("method", "midpoint")
    if method not in ODE_ADAPTIVE_METHODS:
        raise ValueError(f"ode method {method!r} is not an adaptive method of the HIP path ({' | '.join(ODE_ADAPTIVE_METHODS)})")
    if windowed:
        raise ValueError(f"window_seconds= with the adaptive method {method!r}: the rows of one clip share their blended frames and "
                         "must share their times, which per-row step control does not give them; pass step_control=\"clip\" to "
                         "separate() (step control per clip, DESIGN.md section 10.11) or use a fixed-grid method")
    unknown = sorted(set(ode_opt) - {"method", "rtol", "atol", "options"})
    if unknown:
        raise ValueError(f"ode_opt: unsupported {unknown} for {method!r} (method | rtol | atol | options)")
    if ode_opt.get("rtol") is None or ode_opt.get("atol") is None:
        raise ValueError(f"ode method {method!r} needs ode_opt['rtol'] and ode_opt['atol']: torchdiffeq's defaults (1e-7 / 1e-9) lie "
                         "below what an fp32 vector field resolves, so there is no default here; 1e-3 .. 1e-5 are sensible")
    rtol, atol = float(ode_opt["rtol"]), float(ode_opt["atol"])
    if not (rtol > 0 and atol > 0 and math.isfinite(rtol) and math.isfinite(atol)):
        raise ValueError(f"ode_opt: rtol and atol must be positive floats (got {ode_opt['rtol']!r}, {ode_opt['atol']!r})")
    options = dict(ode_opt.get("options") or {})
    unknown = sorted(set(options) - set(ODE_ADAPTIVE_OPTIONS))
    if unknown:
        raise ValueError(f"ode_opt['options']: unsupported {unknown} for {method!r} ({' | '.join(ODE_ADAPTIVE_OPTIONS)})")
    o = {k: (v if options.get(k) is None else options[k]) for k, v in ODE_ADAPTIVE_OPTIONS.items()}
    first = 0.0 if o["first_step"] is None else float(o["first_step"])
    if o["first_step"] is not None and not (0 < first <= 1.0):
        raise ValueError(f"ode_opt['options']['first_step'] must lie in (0, 1] (got {o['first_step']!r})")
    safety, ifactor, dfactor, steps = float(o["safety"]), float(o["ifactor"]), float(o["dfactor"]), int(o["max_num_steps"])
    if not (safety > 0 and ifactor >= 1 and 0 < dfactor < 1 and steps >= 1):
        raise ValueError("ode_opt['options']: safety > 0, ifactor >= 1, 0 < dfactor < 1 and max_num_steps >= 1 are required")
    return ODE_ADAPTIVE_METHODS[method], hip.OdeAdaptive(rtol, atol, first, safety, ifactor, dfactor, min(steps, 2 ** 31 - 1))


STEP_CONTROLS = (None, "row", "clip")


def check_step_control(step_control: Optional[str], ode_opt: Dict[str, Any]) -> bool:
    """separate()'s `step_control`: None | "row" (the unit of an adaptive method's step control is the engine row: section 10.9) |
    "clip" (the window rows of one clip and candidate share one time, step, error norm and decision: section 10.11).  True for
    "clip"; ValueError for another value, and for "clip" with a fixed-grid method, which has no step control."""
    if step_control not in STEP_CONTROLS:
        raise ValueError(f"step_control={step_control!r}: None | 'row' | 'clip'")
    if step_control == "clip" and not is_adaptive(ode_opt):
        raise ValueError(f"step_control='clip' with the fixed-grid method {ode_opt.get('method', 'midpoint')!r}: only the adaptive "
                         f"methods ({' | '.join(ODE_ADAPTIVE_METHODS)}) control their step")
    return step_control == "clip"


def _field_stand_in(t, y):
    raise NotImplementedError("grid_constructor: the HIP path passes a stand-in for the vector field; a grid constructor that "
                              "evaluates the field is not supported")


def ode_grid(ode_opt: Dict[str, Any], t0: float = 0.0, t1: float = 1.0, y0: Optional[torch.Tensor] = None):
    """(method id, grid) for the fixed-grid solvers torchdiffeq would run for `ode_opt` (reference model.py:285-290; quirk Q11).
    method: euler | midpoint | rk4 | heun3.  options, with the semantics of torchdiffeq's FixedGridODESolver:
      {"step_size": h}        t0, t0 + h, ... with the last point clamped to t1;
      {"grid_constructor": g} g(func, y0, t) with t = tensor([t0, t1]) on y0's device and `func` a stand-in that raises if called;
                              1-D, strictly increasing (also as float32, what the engine integrates over), from t0 to t1 exactly;
      none / {}               one step over [t0, t1].
    Everything else - other methods (dopri5 | bosh3 are ode_adaptive's), other keys, step_size together with grid_constructor - is a
    ValueError."""
    method = ode_opt.get("method", "midpoint")
    if method not in ODE_METHODS:
        raise ValueError(f"ode method {method!r} is not a fixed-grid method of the HIP path ({' | '.join(ODE_METHODS)}; "
                         f"{' | '.join(ODE_ADAPTIVE_METHODS)} go through ode_adaptive; the other adaptive and the Adams solvers are "
                         "not supported: DESIGN.md section 1 row a6)")
    options = dict(ode_opt.get("options") or {})
    step = options.pop("step_size", None)
    constructor = options.pop("grid_constructor", None)
    if options:
        raise ValueError(f"ode_opt['options']: unsupported {sorted(options)} (step_size | grid_constructor)")
    if step is not None and constructor is not None:
        raise ValueError("ode_opt['options']: step_size and grid_constructor are mutually exclusive")
    if step is not None:
        n = int(math.ceil((t1 - t0) / step + 1))
        grid = [min(t0 + k * step, t1) for k in range(n)]
        grid[-1] = t1
    elif constructor is not None:
        grid = _constructed_grid(constructor, y0, t0, t1)
    else:
        grid = [t0, t1]
    stages = hip.ODE_STAGES.get(ODE_METHODS[method])
    if stages is not None and stages * (len(grid) - 1) > hip.ODE_TIME_SLOTS:
        raise ValueError(f"ode grid of {len(grid) - 1} steps: {method} evaluates the field {stages} times per step, the engine's "
                         f"time table holds {hip.ODE_TIME_SLOTS} evaluations")
    return ODE_METHODS[method], grid


def _constructed_grid(constructor: Callable, y0: Optional[torch.Tensor], t0: float, t1: float) -> List[float]:
    t = torch.tensor([t0, t1], device=y0.device if y0 is not None else None)
    g = torch.as_tensor(constructor(_field_stand_in, y0, t)).detach()
    if g.dim() != 1 or g.numel() < 2:
        raise ValueError(f"grid_constructor must return a 1-D grid of at least two points (got shape {tuple(g.shape)})")
    g = g.to("cpu")
    if float(g[0]) != t0 or float(g[-1]) != t1:
        raise ValueError(f"grid_constructor: the grid must start at {t0} and end at {t1} exactly "
                         f"(got {float(g[0])} .. {float(g[-1])})")
    g32 = g.to(torch.float32)
    if not bool((g32[1:] > g32[:-1]).all()):
        raise ValueError("grid_constructor: the grid must be strictly increasing (as float32)")
    return g32.tolist()


def _alt16_weight(alt16_classes: int, name: str) -> bool:
    """engine tensor `name` is the weight of a class that reads alt-format (bfloat16) operands in a model with these alt16 classes"""
    leaf = name.rsplit(".", 1)[-1]
    return name.startswith("L") and leaf in hip.ALT16_WEIGHTS and bool(alt16_classes & hip.CLS[hip.ALT16_WEIGHTS[leaf]])


class _Codec16(Context):
    """A codec-only engine context on plain 16-bit operands beside an fp32-storage model (precision "fp16x3", `codec_decode="16"`):
    SAMAudio.decode_audio runs on it.  It borrows the model's 16-bit copies of the codec weights and whatever workspace its owner
    (the model or a stream lane) holds at the time of the call."""

    _ctx = property(lambda self: self._h)

    def __init__(self, model: "SAMAudio"):
        hc = hip.Config.from_buffer_copy(model._hc)
        hc.precision = hip.BF16   # "the library's 16-bit operand format"
        super().__init__(model._lib, "samaudio", hc, device=model.device, operands=hip.operands_for(model.precision))
        self.register(model._codec16_tensors, borrowed=True)
        self.finalize(1)


class _Lane(Context):
    """An extra engine context bound to its own HIP stream.  It borrows the model's weight tensors (no copy) and
    owns only a workspace; `SAMAudio(streams=S)` solves S contiguous row groups of a batch concurrently so that one
    group's GEMM tails / epilogues / launch gaps are filled by the other group's workgroups."""

    _ctx = property(lambda self: self._h)

    def __init__(self, model: "SAMAudio"):
        super().__init__(model._lib, "samaudio", model._hc, device=model.device, operands=model._operands, alt16=model._alt16)
        self.register(model._tensors, borrowed=True)
        self.finalize(0)
        model._set_precision_options(self._ctx)
        if model._has_codec:   # the lane also decodes its own row group (SAMAudio._solve_concurrent)
            self.finalize(1)
        self._stages: Optional[torch.Tensor] = None   # rk4 / heun3 stage buffers of this context (SAMAudio._ensure_stages)
        self._live = None
        self._codec16: Optional[_Codec16] = None
        self.stream = torch.cuda.Stream(device=model.device)


class SAMAudio(Context):
    config_cls = SAMAudioConfig
    _ctx = property(lambda self: self._h)
    _register = Context.register   # (the name tests register extra tensors by)

    def __init__(self, cfg: SAMAudioConfig, precision: str = "fp16x3", device: Optional[str] = None,
                 text_encoder: Optional[Callable] = None, streams: int = 1, f32_classes="auto",
                 weight_layout: str = "auto", prefetch_rows: Optional[int] = None, x3_classes="auto",
                 codec_decode: str = "auto", tower_precision: Optional[str] = None, frame_transform: Optional[str] = None,
                 codec_tile_seconds: Optional[float] = None):
        """`codec_tile_seconds` (None = off, the default; this build's own definition): separate() runs the
        DAC-VAE - the mixture's encode and the decode of (target, residual) pairs - in time tiles of this length, each with the
        codec's own reach of context either side, so the codec scratch is sized by the tile and not by the clip.  The results are
        bitwise those of the untiled codec.  separate(codec_tile_seconds=...) overrides it for one call.
        `frame_transform`: `PerceptionEncoder(frame_transform=...)` of the vision encoder that load_state_dict builds - None (default)
        = its default "torch"; "hip" resizes, rounds and normalises uint8 videos inside the tower's first kernel.
        `tower_precision`: the precision of the PE-Core vision tower that load_state_dict builds when the checkpoint carries one.
        None (default) = hip.tower_precision(precision): plain 16-bit operands beside an x3 DiT.  "fp16x3" / "bf16x3" opt the tower
        into its compensated mode.
        `precision`: "fp16x3" (default: the reference computes in fp32, README.md:48 - fp32 storage and every big contraction on
        hi/lo-split IEEE-half operands hold its results to 1e-3 on benign and trained-like weights) | "fp16" |
        "mixed" | "bf16" (plain 16-bit GEMM operands: ~3x the throughput, inside 1e-3 on benign weights only / not at all) | "fp32"
        (exact-fp32 MFMA) | "bf16x3".
        `weight_layout` (16-bit precisions): "ktm" stores the weights of the five big GEMM classes of the DiT layers
        K-tile-major (weights.ktm_layout; a launch then streams its weights front to back), "rows" keeps them row-major;
        "auto" = DEFAULT_WEIGHT_LAYOUT.  In the x3 precisions it is the layout of the 16-bit ".x3" twins of the compensated classes (the
        fp32 weights stay row-major; `prefetch_rows` has no effect there: an fp32 context never prefetches).
        `prefetch_rows`: evaluations of at most this many rows (batch x frames) let the CUs a
        GEMM launch leaves idle read the next GEMM's weights (samaudio.h SAMAUDIO_OPT_PREFETCH_ROWS; None =
        DEFAULT_PREFETCH_ROWS, 0 = off).  Both are scheduling / layout choices: results are bitwise the same.
        `f32_classes` (16-bit precisions): the GEMM classes that run on exact-fp32 operands inside the 16-bit engine
        (hip.CLASSES names or a mask; "auto" = hip.CLS_F32_DEFAULT: the input and output projections that touch the ODE
        state and the hoisted conditioning, which carry most of a 16-bit mode's error for < 1 % of a step; "time" and
        "yemb" can be added - DESIGN.md section 4)."""
        cfg.check_supported()
        hip.check_precision(precision, x3_ok=True)
        if tower_precision is not None:
            hip.check_precision(tower_precision, x3_ok=True)
        self.cfg = cfg
        self.precision = precision
        self.tower_precision = tower_precision
        if frame_transform is not None:
            from .vision_encoder import FRAME_TRANSFORMS
            if frame_transform not in FRAME_TRANSFORMS:
                raise ValueError(f"frame_transform must be one of {FRAME_TRANSFORMS}, not {frame_transform!r}")
        self.frame_transform = frame_transform
        self._codec_tile_frames(codec_tile_seconds, cfg)   # (ValueError below one frame)
        self.codec_tile_seconds = codec_tile_seconds
        # per direction ("encode" / "decode") of the last tiled codec call: tile_frames, halo_frames, tiles, passes
        self.last_codec_tiles: Dict[str, Dict[str, int]] = {}
        # precision "fp16x3" (and "bf16x3"): fp32 storage and fp32 small classes, the six big GEMM classes of the layers on
        # compensated 16-bit operands (samaudio.h SAMAUDIO_OPT_X3_CLASSES; `x3_classes`: names or a mask, "auto" = all six)
        self.x3_classes = 0 if not hip.is_x3(precision) else (
            hip.CLS_X3_DEFAULT if x3_classes == "auto" else hip.class_mask(x3_classes))
        # x3 precisions: the DAC-VAE DECODER in the model's own fp32 context ("32": its convolutions multiply on operands split on
        # the fly like the encoder's - hip.CLS["codec"] of x3_classes) or on plain 16-bit operands ("16": a codec-only context of
        # the same library beside the fp32 one).  Measured on the hostile weights (profiles/r6_call2/): with
        # the 16-bit decoder the waveform misses the 1e-3 bound (1.6e-3 small*, 1.9e-3 large*; latent 1e-4 either way), so "32" is
        # the default; "16" stays selectable (benign weights: 2e-4).  "auto" = environment SAMAUDIO_X3_DECODE, default "32".
        if codec_decode == "auto":
            codec_decode = os.environ.get("SAMAUDIO_X3_DECODE", "32")
        if codec_decode not in ("16", "32"):
            raise ValueError("codec_decode must be 'auto', '16' or '32'")
        self.codec_decode = codec_decode if hip.is_x3(precision) else "native"
        self._codec16_tensors: Dict[str, torch.Tensor] = {}
        self._codec16: Optional[_Codec16] = None
        precision = hip.storage_precision(precision)   # what everything below means by "fp32"
        self.f32_classes = 0 if precision == "fp32" else (
            hip.CLS_F32_DEFAULT if f32_classes == "auto" else hip.class_mask(f32_classes))
        self.quant_classes, self.quant_format = 0, 0   # fp32 engines: operand-rounding emulation (error budget)
        # precision="mixed": bf16 operands for the five big GEMM classes inside the fp16 build (hip.CLS_ALT16_MIXED)
        self.alt16_classes = hip.CLS_ALT16_MIXED if precision == "mixed" else 0
        if weight_layout == "auto":
            weight_layout = os.environ.get("SAMAUDIO_WEIGHT_LAYOUT", DEFAULT_WEIGHT_LAYOUT)
        if weight_layout not in ("ktm", "rows"):
            raise ValueError("weight_layout must be 'auto', 'ktm' or 'rows'")
        self.weight_layout = "rows" if precision == "fp32" else weight_layout
        # x3 precisions: the fp32 weights stay row-major; the layout is that of their 16-bit "<name>.x3" twins, the operands the big
        # GEMMs of the layers actually stream (weights.convert_dit_x3; the engine takes either form of a twin)
        self.x3_weight_layout = weight_layout if hip.is_x3(self.precision) else None
        if prefetch_rows is None:
            prefetch_rows = int(os.environ.get("SAMAUDIO_PREFETCH_ROWS", DEFAULT_PREFETCH_ROWS))
        self.prefetch_rows = 0 if precision == "fp32" else int(prefetch_rows)
        self.device = torch.device(device) if device is not None else None
        self.text_encoder = text_encoder      # callable: list[str] -> (features [B,Lt,768], mask [B,Lt])
        # rerankers (reference model.py:94-95): any callable with the reference's Ranker.forward keywords that returns
        # scores [B, candidates]; sam_audio_amd.ranking.JudgeRanker is the HIP-backed one.  Configured rankers are
        # built lazily from LOCAL checkpoint directories only (no hub access offline), see attach_rankers().
        self.visual_ranker = None
        self.text_ranker = None
        # span predictor (reference model.py:96-102): a sam_audio_amd.judge.PEAudioFrame plus the tokenizer-like
        # transform that turns descriptions into its text inputs
        self.span_predictor = None
        self.span_predictor_transform = None
        self.vision_encoder = None            # callable: list of [T,3,H,W] videos -> [B, T, vision_encoder.dim]
        self.fix_span_order = False           # quirk Q13, see separate()
        self._stages: Optional[torch.Tensor] = None
        self._has_dit = self._has_codec = False
        if int(streams) not in (1, 2) and not os.environ.get("SAMAUDIO_ALLOW_STREAMS"):
            # measured on MI355X: 2 groups +3 %, 3-4 groups no further gain
            raise ValueError("streams must be 1 or 2 (set SAMAUDIO_ALLOW_STREAMS=1 to experiment with more)")
        self.streams = int(streams)           # row groups solved concurrently on separate HIP streams
        # GEMM launches split into whole rounds + a small-tile tail (samaudio.h SAMAUDIO_OPT_TAIL_SPLIT): None = automatic,
        # on when the batch is solved as one row group, off when two groups share the GPU (their kernels fill each other's
        # tails: +2 % without the split, profiles/r2_call7/); True / False pin it (bench.py keeps the instrumented step on
        # the same kernels as the timed ones)
        self.tail_split: Optional[bool] = None
        self._lanes: List[_Lane] = []
        self._f32_have = 0                    # F32-capable classes whose fp32 operand copies are registered
        self._f32_sd: Dict[str, torch.Tensor] = {}
        self._profiling = self._serial_groups = False
        self._sentinel = False
        t, c = cfg.transformer, cfg.audio_codec
        hc = hip.Config(
            precision=hip.precision_code(self.precision), dim=t.dim, n_heads=t.n_heads,
            n_layers=t.n_layers, ffn_hidden=t.ffn_hidden, latent_channels=t.out_channels,
            text_dim=cfg.text_encoder.dim, video_dim=cfg.vision_encoder.dim, freq_dim=t.frequency_embedding_dim,
            anchor_dim=cfg.anchor_embedding_dim, anchor_vocab=cfg.num_anchors + 1, max_positions=t.max_positions,
            norm_eps=t.norm_eps, codec_dim=c.codebook_dim, codec_latent=c.latent_dim, enc_dim=c.encoder_dim,
            dec_dim=c.decoder_dim, enc_rates=(C.c_int32 * 4)(*c.encoder_rates),
            dec_rates=(C.c_int32 * 4)(*c.decoder_rates))
        self._hc = hc
        operands = hip.operands_for(self.precision)
        super().__init__(hip.lib(operands), "samaudio", hc, device=self.device, operands=operands,   # (raises if the HIP library is not built)
                         alt16=functools.partial(_alt16_weight, self.alt16_classes))
        self._set_precision_options(self._ctx)

    # ------------------------------------------------------------------ nn.Module-ish surface
    @property
    def act_dtype(self) -> torch.dtype:
        return hip.act_dtype(self.precision)

    @property
    def sample_rate(self) -> int:  # reference model.py:104-106
        return self.cfg.audio_codec.sample_rate

    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if self._tensors and self.device != device:
            raise RuntimeError("move the model before load_state_dict (weights are converted onto the device)")
        self.device = device
        return self

    def cuda(self, index: int = 0):
        return self.to(f"cuda:{index}")

    @classmethod
    def from_pretrained(cls, model_id: str, map_location: str = "cpu", strict: bool = True,
                        precision: str = "fp16x3", device: Optional[str] = None, tower_precision: Optional[str] = None,
                        frame_transform: Optional[str] = None, codec_tile_seconds: Optional[float] = None, **model_kwargs):
        """Local directory with the reference's `config.json` + `checkpoint.pt`
        (reference base.py:17-62; hub download needs network access this build does not have).

        `tower_precision`: the precision of the rankers built here and of the PE-Core vision tower built by load_state_dict.  None
        (default) = hip.tower_precision(precision): plain 16-bit operands beside an x3 DiT.  "fp16x3" / "bf16x3" opt the Judge and
        the vision tower into their compensated modes (fp32 storage, the big contractions on hi/lo-split 16-bit operands; DESIGN.md
        sections 10.1 and 10.2).
        `frame_transform`, `codec_tile_seconds`: see SAMAudio(...)."""
        if not os.path.isdir(model_id):
            raise FileNotFoundError(f"{model_id}: only local checkpoint directories are supported offline")
        with open(os.path.join(model_id, "config.json")) as fin:
            config = json.load(fin)
        for key, value in model_kwargs.items():
            if key in config:
                config[key] = value
        model = cls(SAMAudioConfig(**config), precision=precision, device=device, tower_precision=tower_precision,
                    frame_transform=frame_transform, codec_tile_seconds=codec_tile_seconds)
        sd = torch.load(os.path.join(model_id, "checkpoint.pt"), weights_only=True, map_location=map_location)
        model.load_state_dict(sd, strict=strict)
        # the reference builds its T5 encoder and rankers in __init__ from hub ids (model.py:82,94-95); offline they
        # can only come from local directories - attach what is reachable, leave the rest to the caller
        try:   # a directory, or a hub id that is already in the local Hugging Face cache (local_files_only)
            from .text_encoder import T5TextEncoder
            model.text_encoder = T5TextEncoder(model.cfg.text_encoder, device=model.device)
        except FileNotFoundError as exc:
            warnings.warn(f"text encoder not attached ({exc}); pass text_features / text_mask to the processor or set "
                          "model.text_encoder")
        model.attach_rankers(precision=hip.tower_precision(precision), tower_precision=tower_precision)
        return model

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """Reference key names in, engine tensors out (see weights.py).  Missing text-encoder / ranker /
        span-predictor keys are tolerated exactly like reference model.py:346-359."""
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        hip.require_gpu(self.device, "SAMAudio (the separate() hot path)")
        missing, unexpected = split_missing_unexpected(state_dict.keys(), self.cfg)
        codec_missing = [k for k in missing if k.startswith("audio_codec.")]
        dit_missing = [k for k in missing if not k.startswith("audio_codec.")]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Missing keys: {missing}, unexpected_keys: {unexpected}")
        vis = {k[len("vision_encoder."):]: v for k, v in state_dict.items() if k.startswith("vision_encoder.")}
        if vis and self.vision_encoder is None and self._covers_vision_tower(vis):
            # reference model.py:83: SAMAudio owns `PerceptionEncoder(cfg.vision_encoder)`; build it when the checkpoint
            # really carries the PE-Core tower (a text-only deployment pays nothing for it)
            from .vision_encoder import PerceptionEncoder
            self.vision_encoder = PerceptionEncoder(self.cfg.vision_encoder, device=self.device,
                                                    precision=self.tower_precision or hip.tower_precision(self.precision),
                                                    frame_transform=self.frame_transform or "torch")
        if vis and hasattr(self.vision_encoder, "load_state_dict"):
            # The tower's key list is restated from the published PE-Core architecture (perception_models is not
            # importable offline), so it is validated for what the engine NEEDS, not for what a genuine checkpoint may carry
            # on top (buffers, layer-scale or text-side keys under `visual.`): missing tensors still fail a strict load,
            # extra ones are reported - an unverified key list must not make a whole SAMAudio checkpoint unloadable.
            v_missing, v_unexpected = self.vision_encoder.load_state_dict(vis, strict=False)
            if strict and v_missing:
                raise RuntimeError(f"Missing keys: {['vision_encoder.' + k for k in v_missing]}")
            if v_unexpected:
                warnings.warn(f"vision_encoder: {len(v_unexpected)} checkpoint tensors are not consumed by the PE-Core tower "
                              f"engine (first: {v_unexpected[:3]})")
        with torch.cuda.device(self.device):
            self._lanes = []   # extra stream contexts borrow the weight tensors registered below: rebuilt on demand
            # register everything first: replacing a tensor the engine already holds (a second load_state_dict) marks BOTH
            # weight sets as not finalized, so each set the model has is finalized again afterwards
            if not dit_missing:
                alt = [leaf for leaf, c in hip.ALT16_WEIGHTS.items() if self.alt16_classes & hip.CLS[c]]
                dit = convert_dit(state_dict, self.cfg, self.act_dtype, self.device, alt16_leaves=alt,
                                  f32_classes=self.f32_classes, ktm=self.weight_layout == "ktm")
                self.register(dit)
                if self.x3_classes:
                    self.register(convert_dit_x3(dit, self.cfg.transformer.n_layers, hip.half_dtype(self.precision),
                                                  self.x3_classes, ktm=self.x3_weight_layout == "ktm"))
                # fp32 operand copies exist for the classes that run in fp32 now; set_f32_classes adds a class's later
                # from these references to the checkpoint entries (no copy is made here)
                self._f32_have = self.f32_classes
                self._f32_sd = {k: state_dict[k] for k in F32_SOURCE_KEYS}
                self._has_dit = True
            if not codec_missing:
                codec = convert_codec(state_dict, self.cfg, self.act_dtype, self.device)
                self.register(codec)
                if self.x3_classes & hip.CLS["codec"]:   # the wide convolutions' split twins (8-phase 16-bit launches over K' = 3K)
                    self.register(convert_codec_x3(codec, hip.half_dtype(self.precision)))
                    # ... and the narrow ones' weights split once, for the fp32 kernel that splits its activations on the fly
                    self.register(convert_codec_fly16(codec, hip.half_dtype(self.precision)))
                self._has_codec = True
                if self.codec_decode == "16":
                    self._codec16_tensors = convert_codec(state_dict, self.cfg, hip.half_dtype(self.precision), self.device)
                    self._codec16 = None
                    for lane in self._lanes:
                        lane._codec16 = None
            if self._has_dit and not (dit_missing and codec_missing):
                self.finalize(0)
            if self._has_codec and not (dit_missing and codec_missing):
                self.finalize(1)
        return missing, unexpected

    def _covers_vision_tower(self, vis: Dict[str, torch.Tensor]) -> bool:
        from .config import PE_VISION_CONFIGS
        from .vision_tower import expected_keys
        pe = PE_VISION_CONFIGS.get(self.cfg.vision_encoder.name)
        return pe is not None and all(("model.visual." + k) in vis for k in expected_keys(pe))

    def _set_precision_options(self, ctx) -> None:
        if hip.storage_precision(self.precision) != "fp32":
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_F32_CLASSES, self.f32_classes))
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_ALT16_CLASSES, self.alt16_classes))
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_PREFETCH_ROWS, self.prefetch_rows))
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_SENTINEL, int(getattr(self, "_sentinel", False))))
        else:
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_QUANT_CLASSES, self.quant_classes))
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_QUANT_FORMAT, self.quant_format))
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_X3_CLASSES, self.x3_classes))

    def set_f32_classes(self, classes) -> None:
        """Switch the exact-fp32 GEMM classes of a 16-bit model (see __init__); takes effect from the next call."""
        self.f32_classes = 0 if hip.storage_precision(self.precision) == "fp32" else hip.class_mask(classes)
        need = self.f32_classes & ~self._f32_have
        if need and self._has_dit:   # the classes switched on for the first time: their "<name>.f32" operand copies
            with torch.cuda.device(self.device):
                self.register(convert_dit_f32(self._f32_sd, self.cfg, self.device, need))
                self._f32_have |= need
                self._lanes = []   # stream lanes borrow the registered tensors: rebuilt on demand
                # binds the new names.  Registering a name the engine already holds (the copies of an earlier checkpoint that
                # a later load_state_dict left behind) marks EVERY weight set as not finalized: each set the model has is
                # finalized again (the codec set was not, and the next separate() failed in the codec)
                self.finalize(0)
                if self._has_codec:
                    self.finalize(1)
        for ctx in [self._ctx] + [lane._ctx for lane in self._lanes]:
            self._set_precision_options(ctx)

    def set_quantised_classes(self, classes, fmt: str = "bf16") -> None:
        """fp32 models only - measurement aid: the GEMMs of `classes` round both operands to `fmt` ("bf16" | "fp16")
        before multiplying, everything else stays exact (samaudio.h SAMAUDIO_OPT_QUANT_CLASSES)."""
        if hip.storage_precision(self.precision) != "fp32":
            raise ValueError("operand-rounding emulation needs precision='fp32'")
        self.quant_classes, self.quant_format = hip.class_mask(classes), hip.QUANT_FORMATS[fmt]
        for ctx in [self._ctx] + [lane._ctx for lane in self._lanes]:
            self._set_precision_options(ctx)

    def engine_tensors(self) -> Dict[str, torch.Tensor]:
        return self._tensors

    # ------------------------------------------------------------------ validation aid
    def sentinel(self, on: bool = True) -> None:
        """samaudio.h SAMAUDIO_OPT_SENTINEL: every 16-bit tensor a GEMM of the hot path writes (and the RMSNorm / attention
        outputs that feed GEMMs) is scanned for its largest magnitude and for non-finite values; sentinel_report() reads and
        resets the figures.  An fp16 overflow is then reported with its GEMM class instead of propagating."""
        self._sentinel = bool(on)
        for ctx in [self._ctx] + [lane._ctx for lane in self._lanes]:
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_SENTINEL, int(self._sentinel)))

    def sentinel_report(self) -> Dict[str, Dict[str, float]]:
        """{class: {"absmax": ..., "nonfinite": ...}} over every engine context since the last report (synchronises)."""
        out = {n: {"absmax": 0.0, "nonfinite": 0.0} for n in hip.SENTINEL_NAMES}
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            for ctx in [self._ctx] + [lane._ctx for lane in self._lanes]:
                mx, bad = (C.c_float * hip.SENTINEL_SLOTS)(), (C.c_double * hip.SENTINEL_SLOTS)()
                hip.check(self._lib.samaudio_sentinel_read(ctx, mx, bad, hip.current_stream_ptr()))
                for i, n in enumerate(hip.SENTINEL_NAMES):
                    out[n]["absmax"] = max(out[n]["absmax"], float(mx[i]))
                    out[n]["nonfinite"] += float(bad[i])
        return out

    # ------------------------------------------------------------------ measurement (bench.py)
    def profile_begin(self, serial_groups: bool = True) -> None:
        """Bracket every kernel launch with a hipEvent pair on its launch stream until profile_end(), on every engine
        context of the model (the row groups of `streams` > 1 have one each).  `serial_groups`: while profiling, the row
        groups run ONE AFTER THE OTHER on the caller's stream, so that an event pair times a kernel that has the GPU to
        itself - the launches (shapes, tile policy, options) are exactly those of the concurrent run."""
        self._profiling, self._serial_groups = True, bool(serial_groups)
        for ctx in self._profiled_ctxs():
            hip.check(self._lib.samaudio_profile_begin(ctx))

    def _profiled_ctxs(self):
        """every engine context that launches kernels of a step: the model's, its stream lanes', and their 16-bit codec contexts"""
        owners = [self] + list(self._lanes)
        if self.codec_decode == "16" and self._has_codec:
            for own in owners:
                if own._codec16 is None:
                    own._codec16 = _Codec16(self)
        return [o._ctx for o in owners] + [o._codec16._ctx for o in owners if o._codec16 is not None]

    def profile_end(self) -> List[Dict[str, Any]]:
        """[{name, launches, flops, bytes, ms}] per (class, kernel) since profile_begin() (synchronises), summed over the
        contexts.  name = "dit/<kernel>" | "codec/<kernel>" | "prep/<kernel>"; flops / bytes are algorithmic (see
        include/samaudio.h)."""
        merged: Dict[str, Dict[str, Any]] = {}
        for ctx in self._profiled_ctxs():
            buf = (hip.KernelStat * 64)()
            n = C.c_int(0)
            hip.check(self._lib.samaudio_profile_end(ctx, buf, 64, C.byref(n)))
            for i in range(n.value):
                name = buf[i].name.decode()
                row = merged.setdefault(name, dict(name=name, launches=0, flops=0.0, bytes=0.0, ms=0.0))
                row["launches"] += int(buf[i].launches)
                row["flops"] += float(buf[i].flops)
                row["bytes"] += float(buf[i].bytes)
                row["ms"] += float(buf[i].ms)
        self._profiling = self._serial_groups = False
        return list(merged.values())

    # ------------------------------------------------------------------ workspace
    def _ensure_workspace(self, rows: int, frames: int, text_len: int, codec_items: int, samples: int,
                          lane: Optional[_Lane] = None) -> None:
        own = lane if lane is not None else self   # whoever owns the context owns its workspace
        own.ensure_workspace(rows, frames, max(1, text_len), codec_items, samples)
        base = own._workspace.data_ptr()
        # contexts never share scratch: the workspaces of the model and of its stream lanes are pairwise disjoint
        for other in [self] + list(self._lanes):
            ws = other._workspace
            if other is not own and ws is not None:
                lo, hi = ws.data_ptr(), ws.data_ptr() + ws.numel()
                if base < hi and lo < base + own._workspace.numel():
                    raise RuntimeError("engine contexts were handed overlapping workspaces")

    def _ensure_stages(self, method: int, rows: int, frames: int, lane: Optional[_Lane] = None) -> None:
        """Stage buffers of a Runge-Kutta solve (samaudio_set_ode_stages), owned per engine context like the workspace and apart from
        it; euler and midpoint need none and allocate nothing."""
        own = lane if lane is not None else self
        need = self._lib.samaudio_ode_stage_bytes(own._ctx, method, rows, frames)
        if need:   # (poisoned as the workspace is: a stage read before it was written shows up as NaN)
            hip.check(self._lib.samaudio_set_ode_stages(own._ctx, *scratch(own, "_stages", need, self.device)))

    def _codec_chunk(self, items: int) -> int:
        return min(items, int(os.environ.get("SAMAUDIO_CODEC_CHUNK", "16")))

    # ------------------------------------------------------------------ codec (reference codec.py)
    def _pad_to_hop(self, wavs: torch.Tensor) -> torch.Tensor:
        hop = self.cfg.audio_codec.hop_length
        rem = wavs.size(-1) % hop
        return wavs if rem == 0 else torch.nn.functional.pad(wavs, (0, hop - rem), mode="reflect")

    @staticmethod
    def _codec_tile_frames(seconds: Optional[float], cfg: SAMAudioConfig) -> Optional[int]:
        """`codec_tile_seconds` in latent frames, as longform.py turns seconds into frames; None stays None (no tiles)"""
        if seconds is None:
            return None
        from . import longform
        frames = longform.seconds_to_frames(seconds, cfg.audio_codec.sample_rate, cfg.audio_codec.hop_length)
        if frames < 1:
            raise ValueError(f"codec_tile_seconds={seconds!r} is less than one latent frame "
                             f"({cfg.audio_codec.hop_length} samples at {cfg.audio_codec.sample_rate} Hz)")
        return frames

    def _codec_segment(self, frames: int, tile_frames: int, decode: bool) -> int:
        """the samples of the longest segment a pass over tiles of `tile_frames` runs (samaudio_codec_tile_samples): what the
        workspace of a tiled call is sized by"""
        if int(tile_frames) < 1:
            raise ValueError(f"tile_frames={tile_frames!r}: a codec tile holds at least one latent frame")
        return int(self._lib.samaudio_codec_tile_samples(self._ctx, frames, int(tile_frames), int(decode)))

    def _codec_tiles_record(self, ctx, own: Context, items: int, frames: int, tile_frames: int, segment: int, decode: bool,
                            pairs: bool = False) -> Dict[str, int]:
        """what a tiled call on `ctx` in `own`'s workspace runs: the engine takes as many items per pass as the workspace holds
        segments of (samaudio_workspace_bytes is linear in the items; a pass holds whole pairs)"""
        from .context import _aligned
        usable = _aligned(own._workspace)[1]
        one = self._lib.samaudio_workspace_bytes(ctx, 0, 0, 0, 1, segment)
        per_item = self._lib.samaudio_workspace_bytes(ctx, 0, 0, 0, 2, segment) - one
        chunk = min(items, (usable - (one - per_item)) // per_item)
        if pairs and chunk > 1:
            chunk &= ~1
        return dict(tile_frames=int(tile_frames), halo_frames=int(self._lib.samaudio_codec_halo_frames(ctx, int(decode))),
                    tiles=-(-frames // int(tile_frames)) if tile_frames < frames else 1, passes=-(-items // chunk))

    def encode_audio(self, audios: torch.Tensor, tile_frames: Optional[int] = None) -> torch.Tensor:
        """audios [B,1,Tw] -> mean latent, channels-last [B, T, codebook_dim] (reference codec.py:65-78;
        the reference returns [B, C, T] and transposes at model.py:183).
        `tile_frames` (None: one pass over the whole waveforms): in time tiles of that many latent frames -
        the same bits from a workspace sized by the tile; `last_codec_tiles["encode"]` says what ran."""
        if not self._has_codec:
            raise RuntimeError("audio_codec weights are not loaded")
        wav = self._pad_to_hop(audios.to(self.device, torch.float32)).squeeze(1).contiguous()
        items, samples = wav.shape
        frames = samples // self.cfg.audio_codec.hop_length
        z = torch.empty(items, frames, self.cfg.audio_codec.codebook_dim, device=self.device)
        with torch.cuda.device(self.device):
            if tile_frames is not None:
                segment = self._codec_segment(frames, tile_frames, False)
                self._ensure_workspace(0, 0, 0, self._codec_chunk(items), segment)
                hip.check(self._lib.samaudio_codec_encode_tiled(self._ctx, hip.ptr(wav), items, samples, int(tile_frames), hip.ptr(z),
                                                                hip.current_stream_ptr()))
                self.last_codec_tiles["encode"] = self._codec_tiles_record(self._ctx, self, items, frames, tile_frames, segment, False)
                return z
            self._ensure_workspace(0, 0, 0, self._codec_chunk(items), samples)
            hip.check(self._lib.samaudio_codec_encode(self._ctx, hip.ptr(wav), items, samples, hip.ptr(z),
                                                      hip.current_stream_ptr()))
        return z

    def decode_audio(self, latents: torch.Tensor, lane: Optional[_Lane] = None,
                     out: Optional[torch.Tensor] = None, pairs: bool = False, tile_frames: Optional[int] = None,
                     record: Optional[list] = None) -> torch.Tensor:
        """latents channels-last [N, T, codebook_dim] -> [N, T*hop] (reference codec.py:86-89).  `lane`: run on that
        lane's context (and on the current stream); `out`: a contiguous [N, T*hop] fp32 destination.
        `pairs`: `latents` is the ODE state [rows, T, 2*codebook_dim]; waveform 2b = the first codebook_dim channels of row
        block b (target), 2b + 1 the rest (residual) - reference model.py:291-295, gathered inside the engine instead of a
        transposed copy.
        `tile_frames` (None: one pass over the whole latents): in time tiles of that many latent frames -
        the same bits from a workspace sized by the tile; `last_codec_tiles["decode"]` says what ran (`record`: a list that takes
        the entry instead - the row groups of `streams` > 1 each decode their own rows)."""
        if not self._has_codec:
            raise RuntimeError("audio_codec weights are not loaded")
        lat = latents.to(self.device, torch.float32).contiguous()
        items, frames, _ = lat.shape
        if pairs:
            assert lat.shape[2] == 2 * self.cfg.audio_codec.codebook_dim
            items *= 2
        samples = frames * self.cfg.audio_codec.hop_length
        wav = out if out is not None else torch.empty(items, samples, device=self.device)
        assert wav.shape == (items, samples) and wav.is_contiguous() and wav.dtype == torch.float32
        # (tiles: every workspace below is sized for the longest segment instead of the whole waveform)
        span = samples if tile_frames is None else self._codec_segment(frames, tile_frames, True)
        with torch.cuda.device(self.device):
            self._ensure_workspace(0, 0, 0, self._codec_chunk(items), span, lane=lane)
            ctx = self._ctx if lane is None else lane._ctx
            own = lane if lane is not None else self
            if self.codec_decode == "16":
                # the 16-bit codec context of this owner, on the owner's workspace (sized for the fp32 context's codec pass, which
                # needs more; stream order keeps the two contexts' uses of it apart)
                if own._codec16 is None:
                    own._codec16 = _Codec16(self)
                ctx = own._codec16._ctx
                own.lend_workspace(own._codec16, 0, 0, 1, self._codec_chunk(items), span)
            if tile_frames is not None:
                fn = self._lib.samaudio_codec_decode_pairs_tiled if pairs else self._lib.samaudio_codec_decode_tiled
                hip.check(fn(ctx, hip.ptr(lat), items // 2 if pairs else items, frames, int(tile_frames), hip.ptr(wav),
                             hip.current_stream_ptr()))
                rec = self._codec_tiles_record(ctx, own, items, frames, tile_frames, span, True, pairs)
                if record is not None:
                    record.append(rec)
                else:
                    self.last_codec_tiles["decode"] = rec
            elif pairs:
                hip.check(self._lib.samaudio_codec_decode_pairs(ctx, hip.ptr(lat), items // 2, frames, hip.ptr(wav),
                                                                hip.current_stream_ptr()))
            else:
                hip.check(self._lib.samaudio_codec_decode(ctx, hip.ptr(lat), items, frames, hip.ptr(wav),
                                                          hip.current_stream_ptr()))
        return wav

    # ------------------------------------------------------------------ DiT
    def _prepare(self, audio_features, text_features, text_mask, masked_video_features, anchor_ids,
                 anchor_alignment, audio_pad_mask, lane: Optional[_Lane] = None, anchors_validated: bool = False,
                 candidates: int = 1, latent: bool = False) -> None:
        """`latent`: `audio_features` is the codec latent z [B, T, codebook_dim] and every conditioning tensor holds B clips, each
        serving `candidates` consecutive rows of the solve (samaudio_prepare_latent: (z | z) and the sample-major repeat of
        reference model.py:182-184,193-203 happen inside the engine, nothing is concatenated or repeated here)."""
        dev = self.device
        own = lane if lane is not None else self
        feats = audio_features.to(dev, torch.float32).contiguous()
        rows, frames, _ = feats.shape
        text = tmask = video = ids = align = pad = None
        text_len = 1
        if text_features is not None:
            text = text_features.to(dev, torch.float32).contiguous()
            assert text.size(0) == rows, "text_features batch mismatch"
            text_len = text.size(1)
            if text_mask is not None:
                tmask = text_mask.to(dev).to(torch.uint8).contiguous()
        if masked_video_features is not None:  # reference layout [B, C, T] -> channels-last
            video = masked_video_features.to(dev, torch.float32).transpose(1, 2).contiguous()
            assert video.shape[:2] == (rows, frames), "masked_video_features must be [B, C, T]"
        n_ids = 0
        if anchor_ids is not None:
            ids = anchor_ids.to(dev, torch.long).contiguous()
            align = anchor_alignment.to(dev, torch.long).contiguous()
            n_ids = ids.size(1)
            # the reference's gather / nn.Embedding raise on out-of-range indices (model.py:61).  Tensors a Batch built on the
            # host are in range by construction (processor.Batch.process_anchors checks them there); anything else - forward()
            # called with hand-made tensors - is checked here, at the price of blocking device -> host reads
            if not anchors_validated:
                lo, hi = int(align.min()), int(align.max())
                if lo < 0 or hi >= n_ids:
                    raise IndexError(f"anchor_alignment values must be in [0, {n_ids}): found [{lo}, {hi}]")
                lo, hi = int(ids.min()), int(ids.max())
                if lo < 0 or hi > self.cfg.num_anchors:
                    raise IndexError(f"anchor_ids must be in [0, {self.cfg.num_anchors}]: found [{lo}, {hi}]")
        if audio_pad_mask is not None:
            pad = audio_pad_mask.to(dev).to(torch.uint8).contiguous()
        own._live = (feats, text, tmask, video, ids, align, pad)
        if latent:
            self._ensure_workspace(rows * candidates, frames, text_len, 0, 0, lane)
            hip.check(self._lib.samaudio_prepare_latent(
                own._ctx, rows * candidates, frames, text_len, candidates, hip.ptr(feats), hip.ptr(text), hip.ptr(tmask),
                hip.ptr(video), hip.ptr(ids), n_ids, hip.ptr(align), hip.ptr(pad), hip.current_stream_ptr()))
            return
        assert candidates == 1
        self._ensure_workspace(rows, frames, text_len, 0, 0, lane)
        hip.check(self._lib.samaudio_prepare(
            own._ctx, rows, frames, text_len, hip.ptr(feats), hip.ptr(text), hip.ptr(tmask), hip.ptr(video),
            hip.ptr(ids), n_ids, hip.ptr(align), hip.ptr(pad), hip.current_stream_ptr()))

    def forward(self, noisy_audio: torch.Tensor, audio_features: torch.Tensor, text_features: torch.Tensor,
                time: torch.Tensor, masked_video_features: Optional[torch.Tensor] = None,
                text_mask: Optional[torch.Tensor] = None, anchor_ids: Optional[torch.Tensor] = None,
                anchor_alignment: Optional[torch.Tensor] = None,
                audio_pad_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One ODE function evaluation; same signature as reference model.py:130-141."""
        if not self._has_dit:
            raise RuntimeError("transformer weights are not loaded")
        with torch.cuda.device(self.device):
            self._prepare(audio_features, text_features, text_mask, masked_video_features, anchor_ids,
                          anchor_alignment, audio_pad_mask)
            noisy = noisy_audio.to(self.device, torch.float32).contiguous()
            t = time.to(self.device, torch.float32).reshape(-1).contiguous()
            out = torch.empty_like(noisy)
            hip.check(self._lib.samaudio_forward(self._ctx, hip.ptr(noisy), hip.ptr(t), t.numel(), hip.ptr(out),
                                                 hip.current_stream_ptr()))
        return out

    __call__ = forward

    def solve(self, noise: torch.Tensor, ode_opt: Dict[str, Any] = DFLT_ODE_OPT) -> torch.Tensor:
        """Integrate the flow ODE from `noise` with the conditioning of the last `_prepare` call."""
        state = noise.to(self.device, torch.float32).clone().contiguous()
        if is_adaptive(ode_opt):
            method, params = ode_adaptive(ode_opt)
            with torch.cuda.device(self.device):
                rows = self._solve_adaptive(None, state, method, params)
            self._set_ode_stats([rows], state)
            return state
        method, grid = ode_grid(ode_opt, y0=state)
        g = (C.c_float * len(grid))(*grid)
        with torch.cuda.device(self.device):
            self._ensure_stages(method, state.size(0), state.size(1))
            hip.check(self._lib.samaudio_ode_solve(self._ctx, hip.ptr(state), method, g, len(grid),
                                                   hip.current_stream_ptr()))
        return state

    def _solve_adaptive(self, lane: Optional[_Lane], state: torch.Tensor, method: int, params: "hip.OdeAdaptive") -> List[dict]:
        """samaudio_ode_solve_adaptive on `state` (rows of the context's last prepare), in place, from t = 0 to 1; the call synchronises
        the current stream once per trial step.  Returns the rows' statistics."""
        ctx = self._ctx if lane is None else lane._ctx
        rows, frames = state.size(0), state.size(1)
        self._ensure_stages(method, rows, frames, lane)
        stats = (hip.OdeRowStats * rows)()
        hip.check(self._lib.samaudio_ode_solve_adaptive(ctx, hip.ptr(state), method, 0.0, 1.0, C.byref(params), stats,
                                                        hip.current_stream_ptr()))
        return [dict(accepted=s.accepted, rejected=s.rejected, t=s.t, last_h=s.last_h, status=hip.ODE_ROW_STATUS[s.status],
                     evaluations=s.evaluations) for s in stats]

    def _set_ode_stats(self, groups: List[List[dict]], state: torch.Tensor, names: Optional[List[str]] = None,
                       windows: Optional[List[int]] = None) -> None:
        """`last_ode_stats` of an adaptive solve: per row accepted / rejected / t / last_h / status, and `evaluations`, the field
        launches of the solve (summed over the row groups of a streams > 1 solve).  A row that failed raises RuntimeError; nothing of
        the solve is rolled back, and the state as the solve left it is kept in `last_latent` before raising: finished rows are
        complete there, a failed row holds its state at the `t` of its statistics.  `names`: what an entry is called in that
        error ("row i" by default; the clip and candidate of a solve with step control per clip), `windows`: the window counts per
        clip of such a solve, added to the statistics."""
        self.last_latent = state
        rows = [dict(r) for g in groups for r in g]
        evaluations = sum(g[0]["evaluations"] for g in groups if g)
        for r in rows:
            del r["evaluations"]
        self.last_ode_stats = {"rows": rows, "evaluations": evaluations}
        if windows is not None:
            self.last_ode_stats["windows"] = list(windows)
        for i, r in enumerate(rows):
            if r["status"] != "finished":
                why = ("its step fell below 10 ulp(t)" if r["status"] == "step_underflow"
                       else "it used up options['max_num_steps'] trial steps")
                raise RuntimeError(f"adaptive ODE solve: {names[i] if names else f'row {i}'} stopped at t = {r['t']:.6g} after {r['accepted']} accepted and "
                                   f"{r['rejected']} rejected steps ({why}); try a looser rtol / atol (the state every row "
                                   "reached is in model.last_latent, the statistics in model.last_ode_stats)")

    def _apply_options(self, groups: int) -> None:
        split = int(self.tail_split if self.tail_split is not None else groups == 1)
        for ctx in [self._ctx] + [lane._ctx for lane in self._lanes]:
            hip.check(self._lib.samaudio_set_option(ctx, hip.OPT_TAIL_SPLIT, split))

    def _solve_concurrent(self, noise: torch.Tensor, ode_opt: Dict[str, Any], cond: List[Optional[torch.Tensor]],
                          groups: int, decode: bool = False, anchors_validated: bool = False, candidates: int = 1,
                          latent: bool = False, codec_tile: Optional[int] = None):
        """`codec_tile`: the time tile of the groups' decodes in latent frames (None: whole waveforms).
        prepare + ODE solve (+ DAC-VAE decode of target and residual when `decode`) of `groups` contiguous row groups,
        each on its own engine context and HIP stream, driven by one host thread per group (the C calls release the GIL).
        Rows are independent, so the result equals the single-stream one bit for bit.  Returns the
        latent state, and with `decode` also the waveforms [rows, 2, samples] (model.py:291-295)."""
        import threading
        from .dist import shard_range
        state = noise.to(self.device, torch.float32).clone().contiguous()
        adaptive = is_adaptive(ode_opt)   # rows are independent there as well: each lane loops on its own context and stream
        if adaptive:
            method, params = ode_adaptive(ode_opt)
            group_stats: List[List[dict]] = [[] for _ in range(groups)]
        else:
            method, grid = ode_grid(ode_opt, y0=state)   # one grid for the whole batch (a grid_constructor sees all rows)
            g = (C.c_float * len(grid))(*grid)
        rows, frames, C2 = state.shape
        wavs = (torch.empty(rows * 2, frames * self.cfg.audio_codec.hop_length, device=self.device)
                if decode else None)
        while len(self._lanes) < groups - 1:
            self._lanes.append(_Lane(self))
            if self._profiling:
                hip.check(self._lib.samaudio_profile_begin(self._lanes[-1]._ctx))
                if self.codec_decode == "16":
                    self._lanes[-1]._codec16 = _Codec16(self)
                    hip.check(self._lib.samaudio_profile_begin(self._lanes[-1]._codec16._ctx))
        self._apply_options(groups)
        main = torch.cuda.current_stream(self.device)
        errors: List[BaseException] = []
        tile_recs: List[Dict[str, int]] = []   # tiled decodes: one entry per group

        def work(i: int, lane: Optional[_Lane]):
            try:
                # contiguous groups of CLIPS (all candidates of a clip stay in one group: SURVEY.md section 8e)
                cr = shard_range(rows // candidates, i, groups)
                rr = range(cr.start * candidates, cr.stop * candidates)
                sl = slice(rr.start, rr.stop)
                csl = slice(cr.start, cr.stop) if latent else sl   # `latent`: the conditioning is per clip
                part = [None if c is None else c[csl] for c in cond]
                stream = main if (lane is None or self._serial_groups) else lane.stream
                if stream is not main:
                    # tensors allocated on the caller's stream and used on the lane's: tell the caching allocator, so that
                    # none of their blocks is handed out again before the lane's work on them has finished (the explicit
                    # wait_stream pair below already orders it for the tensors this frame holds; this covers the views
                    # `_prepare` keeps in `lane._live` beyond this call)
                    for t in [state, wavs] + list(cond):
                        if t is not None and t.is_cuda:
                            t.record_stream(stream)
                with torch.inference_mode(), torch.cuda.device(self.device), torch.cuda.stream(stream):
                    self._prepare(*part, lane=lane, anchors_validated=anchors_validated, candidates=candidates, latent=latent)
                    ctx = self._ctx if lane is None else lane._ctx
                    if adaptive:
                        group_stats[i] = self._solve_adaptive(lane, state[sl], method, params)
                    else:
                        self._ensure_stages(method, len(rr), frames, lane)
                        hip.check(self._lib.samaudio_ode_solve(ctx, hip.ptr(state[sl]), method, g, len(grid),
                                                               hip.current_stream_ptr()))
                    if decode:   # waveforms (2b, 2b+1) = (target, residual) of row b, gathered from the state inside the engine
                        self.decode_audio(state[sl], lane=lane, out=wavs[2 * rr.start: 2 * rr.stop], pairs=True,
                                          tile_frames=codec_tile, record=tile_recs)
            except BaseException as exc:  # re-raised on the caller's thread
                errors.append(exc)

        if self._serial_groups:   # profiling: the same launches, one group after the other on the caller's stream
            for i in range(groups):
                work(i, None if i == 0 else self._lanes[i - 1])
        else:
            for lane in self._lanes[:groups - 1]:
                lane.stream.wait_stream(main)
            threads = [threading.Thread(target=work, args=(i, None if i == 0 else self._lanes[i - 1])) for i in range(groups)]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            for lane in self._lanes[:groups - 1]:
                main.wait_stream(lane.stream)
        if errors:
            raise errors[0]
        if tile_recs:   # the groups' passes add up; tile, halo and tile count are the same for all
            self.last_codec_tiles["decode"] = dict(tile_recs[0], passes=sum(r["passes"] for r in tile_recs))
        if adaptive:
            self._set_ode_stats(group_stats, state)
        return (state, wavs.view(rows, 2, -1)) if decode else state

    # ------------------------------------------------------------------ separate()
    def _text(self, batch: Batch):
        if batch.text_features is not None:
            feats = batch.text_features
            mask = batch.text_mask if batch.text_mask is not None else torch.ones(feats.shape[:2], dtype=torch.bool)
            return feats, mask
        if self.text_encoder is None:
            raise RuntimeError(
                "no text encoder is attached (t5-base cannot be downloaded offline): pass "
                "text_features/text_mask to the processor or set model.text_encoder")
        return self.text_encoder(batch.descriptions)

    @staticmethod
    def _repeat(x: Optional[torch.Tensor], candidates: int):
        """Sample-major repeat, reference model.py:193-203."""
        if x is None or candidates == 1:
            return x
        return x.repeat_interleave(candidates, dim=0)

    @torch.inference_mode()
    def separate(self, batch: Batch, noise: Optional[torch.Tensor] = None,
                 ode_opt: Dict[str, Any] = DFLT_ODE_OPT, reranking_candidates: int = 1,
                 predict_spans: bool = False, output_sampling_rate: Optional[int] = None,
                 window_seconds: Optional[float] = None, window_overlap_seconds: Optional[float] = None,
                 seed: Optional[int] = None, step_control: Optional[str] = None,
                 codec_tile_seconds: Optional[float] = None) -> SeparationResult:
        """Reference model.py:247-338.  `codec_tile_seconds` (None = the model's setting, see SAMAudio(...)):
        the mixture's encode and the decode of the pairs run in time tiles of that length on every path below - the same bits, a
        codec scratch sized by the tile; `last_codec_tiles` says what ran.  The rerankers and the span predictor see whole clips.  `reranking_candidates > 1` draws that many ODE solutions per clip and lets
        `visual_ranker` / `text_ranker` pick one (model.py:306-330); `predict_spans` runs `span_predictor` first
        (model.py:259-268; mind quirk Q13 below).  `output_sampling_rate`: when set and different from the codec's rate, the chosen
        target and residual of every clip are resampled to it on the device (sam_audio_amd/audio.py resample: what the reference's
        evaluation does with torchaudio behind separate()); None leaves the results as the codec wrote them.
        `ode_opt`: torchdiffeq's shape.  The fixed-grid methods (`ode_grid`) or {"method": "dopri5" | "bosh3", "rtol": r, "atol": a,
        "options": {...}} (`ode_adaptive`): embedded pairs with per-row step control, pinned to scipy's RK45 / RK23 and unpinned vs
        torchdiffeq.  An adaptive solve leaves `last_ode_stats` and raises RuntimeError when a row fails (the
        state every row reached is then in `last_latent`); it combines with `window_seconds` only under `step_control="clip"`.
        `step_control` (None | "row" | "clip"; None = "row"; this build's own definition): the unit of an
        adaptive method's step control.  "row": every engine row on its own, which window rows cannot be - ValueError together with
        `window_seconds`.  "clip": the window rows of one (clip, candidate) carry ONE time, step, error norm - over the clip's valid
        frames, each counted once, whichever windows hold it - and accept / reject decision, so a clip's result does not depend on the
        clips beside it.  `last_ode_stats["rows"]` then has one entry per (clip, candidate) in the stitched latent's row order, and
        `last_ode_stats["windows"]` the window counts per clip; a failed one raises the RuntimeError above, naming clip and candidate,
        with `last_window_latent` / `last_window_plan` set.  Without windows, or when every clip fits one window, a clip is a row and
        "clip" is the per-row path: no table, no other launch.  ValueError with a fixed-grid method.
        `window_seconds` / `window_overlap_seconds` (both or neither; this build's own definition): clips longer
        than the window are solved as overlapping windows of that length - rows of ONE batch whose overlapping frames are cross-faded
        after every evaluation of the vector field, so they hold the same bits through the whole solve; the latent is stitched by index
        and decoded once over its whole length.  Encoder, text, visual features, span predictor and rerankers see whole clips.  All
        windows of a batch are solved together (no splitting when they do not fit in memory), on the model's own context: `streams` > 1
        is ignored for a windowed solve.  `last_latent` is the stitched latent, `last_window_latent` the window rows,
        `last_window_plan` the longform.WindowPlan.  A clip that fits one window is one row without a successor: the plain path.
        `seed` (an int in [0, 2**64); not together with `noise`; this build's own definition): the start state
        is `noise.seeded_noise(seed, ids, candidates, T, 256)` instead of a `torch.randn` draw - one counter-based stream per (seed,
        clip id, candidate), ids = `batch.clip_ids` (SAMAudioProcessor(..., clip_ids=...); `dist.shard_batch` keeps each clip's) or
        range(B).  What a clip starts from then depends on nothing but those three: not on the batch around it, its padded length,
        the number of candidates, earlier draws or the rank that owns it.  The tensor comes back in `SeparationResult.noise`, and every
        path takes it as it takes a caller's.  None (default): `torch.randn`, as the reference draws."""
        if seed is not None:   # before anything runs
            if noise is not None:
                raise ValueError("seed and noise are mutually exclusive: a seed stands for the noise it generates")
            from .noise import check_seed
            seed = check_seed(seed)
        by_clip = check_step_control(step_control, ode_opt)   # before anything runs
        if is_adaptive(ode_opt):   # before anything runs: the tolerances, the options, and no windows unless stepped per clip
            ode_adaptive(ode_opt, windowed=window_seconds is not None and not by_clip)
        if not (self._has_dit and self._has_codec):
            raise RuntimeError("load_state_dict() first")
        if (window_seconds is None) != (window_overlap_seconds is None):
            raise ValueError("window_seconds and window_overlap_seconds go together: give both or neither")
        window = None
        if window_seconds is not None:
            from . import longform
            c = self.cfg.audio_codec
            window = (longform.seconds_to_frames(window_seconds, c.sample_rate, c.hop_length),
                      longform.seconds_to_frames(window_overlap_seconds, c.sample_rate, c.hop_length))
            longform.check_window(*window, self.cfg.transformer.max_positions)
        tile = self._codec_tile_frames(self.codec_tile_seconds if codec_tile_seconds is None else codec_tile_seconds, self.cfg)
        res = self._separate(batch, noise, ode_opt, reranking_candidates, predict_spans, window, seed, tile)   # (windows + adaptive: per clip)
        if output_sampling_rate is None or int(output_sampling_rate) == self.sample_rate:
            return res
        from . import audio
        with torch.cuda.device(self.device):
            return SeparationResult(target=[audio.resample(w, self.sample_rate, output_sampling_rate) for w in res.target],
                                    residual=[audio.resample(w, self.sample_rate, output_sampling_rate) for w in res.residual],
                                    noise=res.noise)

    def _separate(self, batch: Batch, noise: Optional[torch.Tensor], ode_opt: Dict[str, Any], reranking_candidates: int,
                  predict_spans: bool, window: Optional[tuple] = None, seed: Optional[int] = None,
                  codec_tile: Optional[int] = None) -> SeparationResult:
        """`codec_tile`: the codec's time tile in latent frames (None: whole waveforms), handed to every codec call below"""
        cand = int(reranking_candidates)
        self.last_codec_tiles = {}
        with torch.cuda.device(self.device):
            # Nothing of torch's own arithmetic runs between the first and the last kernel of a step: the noise is drawn first
            # (model.py:274-275: `torch.randn_like` on the model device), features = (z | z) (model.py:182-184), the sample-major
            # repeat for the candidates (model.py:193-203) and the (target, residual) split of the state (model.py:291-295) are
            # index arithmetic inside the engine (samaudio_prepare_latent / samaudio_codec_decode_pairs).
            hop = self.cfg.audio_codec.hop_length
            B, T = batch.audios.size(0), -(-batch.audios.size(-1) // hop)
            C2 = self.cfg.transformer.out_channels
            if seed is not None:   # one stream per (seed, clip id, candidate): noise_rows_kernel
                from .noise import check_clip_ids, seeded_noise
                ids = getattr(batch, "clip_ids", None)
                noise = seeded_noise(seed, range(B) if ids is None else check_clip_ids(ids, B, distinct=True), cand, T, C2, self.device)
            if noise is None:
                noise = torch.randn(B * cand, T, C2, device=self.device)         # model.py:274-275
            assert tuple(noise.shape) == (B * cand, T, C2), "noise must be [B*candidates, T, 256]"
            z = self.encode_audio(batch.audios, tile_frames=codec_tile)          # [B, T, 128]
            assert z.shape[:2] == (B, T) and 2 * z.size(2) == C2
            text, text_mask = self._text(batch)
            video = None
            if batch.masked_video is not None:                                   # model.py:186-191
                if self.vision_encoder is None:
                    raise NotImplementedError(
                        "visual prompting needs a vision encoder: set model.vision_encoder to a callable "
                        "list[video [T,3,H,W]] -> features [B, T, vision_encoder.dim] (PE-Core tower, SURVEY.md section 8 f3)")
                video = self.vision_encoder(batch.masked_video).transpose(1, 2)  # reference layout [B, C, T]
            # forward args are assembled BEFORE the span predictor runs (reference model.py:257 vs :259-268), and
            # process_anchors rebinds new tensors, so in the reference snapshot predicted spans never reach the ODE
            # (quirk Q13).  fix_span_order=True opts into the evidently intended order.
            anchor_ids, anchor_alignment = batch.anchor_ids, batch.anchor_alignment
            # host-built anchors, range-checked against THIS model's anchor vocabulary: no device-side range check
            validated = getattr(batch, "anchor_vocab_validated", 0) == self.cfg.num_anchors + 1
            if predict_spans and batch.anchors is None:
                if self.span_predictor is None:
                    warnings.warn("predict_spans=True ignored: no span predictor attached (model.span_predictor)")
                else:
                    batch = self.predict_spans(batch, z, batch.audio_pad_mask)   # model.py:259-268 (reads channels [0, 128))
                    if self.fix_span_order:
                        anchor_ids, anchor_alignment = batch.anchor_ids, batch.anchor_alignment
            cond = [z, text, text_mask, video, anchor_ids, anchor_alignment, batch.audio_pad_mask]   # per clip: B items each
            groups = min(self.streams, B)
            wavs = None
            if window is not None:   # (window, overlap) in frames: all windows of the batch as rows of one solve on the main context
                latent = self._solve_windowed(batch, noise, cond, window, cand, validated, ode_opt)
            elif groups > 1:
                cond = [None if c is None else c.to(self.device) for c in cond]
                # each group also decodes its own rows on its stream: the codec's HBM-bound convolutions of one group run
                # beside the other group's kernels instead of after both solves
                latent, wavs = self._solve_concurrent(noise, ode_opt, cond, groups, decode=True, anchors_validated=validated,
                                                      candidates=cand, latent=True, codec_tile=codec_tile)
            else:
                self._apply_options(1)
                self._prepare(*cond, anchors_validated=validated, candidates=cand, latent=True)
                latent = self.solve(noise, ode_opt)                              # states[-1], [Bc, T, 256]
            self.last_latent = latent
            # [Bc, T, 2C] -> waveforms (2b, 2b+1) = (target, residual) of row b (model.py:291-295)
            Bc = latent.size(0)
            if wavs is None:
                wavs = self.decode_audio(latent, pairs=True, tile_frames=codec_tile).view(Bc, 2, -1)
            # codec.py:91-97, from the batch's host copy of the frame counts: slicing by device scalars would block on the GPU
            sizes = [n * hop for n in (getattr(batch, "sizes_host", None) or [int(v) for v in batch.sizes.tolist()])]
            target = self.unbatch(wavs[:, 0].view(B, cand, -1), sizes)
            residual = self.unbatch(wavs[:, 1].view(B, cand, -1), sizes)
            if cand == 1:   # nothing to pick: views, no index kernels, no device -> host reads
                return SeparationResult(target=[w[0] for w in target], residual=[w[0] for w in residual], noise=noise)
            idxs = self._rerank(batch, target, sizes, cand)                      # model.py:306-330
            return SeparationResult(
                target=[w[i] for w, i in zip(target, idxs)],
                residual=[w[i] for w, i in zip(residual, idxs)],
                noise=noise)

    def _solve_windowed(self, batch: Batch, noise: torch.Tensor, cond: List[Optional[torch.Tensor]], window: tuple, cand: int,
                        validated: bool, ode_opt: Dict[str, Any]) -> torch.Tensor:
        """The ODE solve of separate() over overlapping windows.  `cond` holds the whole clips' conditioning
        (B items each), `noise` is [B * cand, T, C2] over the whole clips.  Everything here is index plumbing: gathers into window rows,
        one prepare, the successor table, one solve, the stitch.  Returns the stitched latent [B * cand, T, C2]."""
        from . import longform
        z, text, text_mask, video, anchor_ids, anchor_alignment, pad = cond
        dev = self.device
        B, T = z.shape[:2]
        lengths = getattr(batch, "sizes_host", None) or [int(v) for v in batch.sizes.tolist()]
        plan = longform.plan_windows(lengths, window[0], window[1], cand, batch_frames=T,
                                     max_positions=self.cfg.transformer.max_positions)
        clip_of, frame_of, inside = plan.gather_index()
        clip = torch.tensor(clip_of, device=dev)
        frame = torch.tensor(frame_of, device=dev)                                # [window rows, L]: whole-clip frame of a row's frame
        hole = ~torch.tensor(inside, device=dev) if not all(map(all, inside)) else None   # row frames past the padded batch

        def rows_of(x: Optional[torch.Tensor], row, frames, holes, fill=0):       # [.., T, ...] -> [rows, L, ...]
            if x is None:
                return None
            out = x.to(dev)[row[:, None], frames]
            if holes is not None:
                out.masked_fill_(holes.view(holes.shape + (1,) * (out.dim() - 2)), fill)
            return out

        if pad is None:
            pad = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]

        def per_row(x: Optional[torch.Tensor]):                                   # text, text mask, anchor ids: repeated per window
            return None if x is None else x.to(dev)[clip]

        cond_rows = [rows_of(z, clip, frame, hole), per_row(text), per_row(text_mask),
                     None if video is None else rows_of(video.transpose(1, 2), clip, frame, hole).transpose(1, 2),
                     per_row(anchor_ids),
                     None if anchor_ids is None else rows_of(anchor_alignment, clip, frame, hole, fill=1),   # 1 = the <pad> slot
                     rows_of(pad, clip, frame, hole, fill=False)]
        # the noise of engine row (window row g, candidate c) = the frames of whole-clip noise row clip(g) * cand + c: overlapping frames
        # of neighbouring windows start identical
        nrow = (clip[:, None] * cand + torch.arange(cand, device=dev)[None, :]).reshape(-1)
        wnoise = rows_of(noise.to(dev, torch.float32), nrow, frame.repeat_interleave(cand, dim=0),
                         None if hole is None else hole.repeat_interleave(cand, dim=0))
        self._apply_options(1)
        self._prepare(*cond_rows, anchors_validated=validated, candidates=cand, latent=True)
        linked = any(s >= 0 for s in plan.next_row)   # clips that all fit one window: plain rows, no table, no extra launch
        table = torch.tensor(plan.next_row, dtype=torch.int32, device=dev) if linked else None
        # an adaptive method over linked rows (separate() has checked step_control="clip"): one step control per (clip, candidate),
        # whose norms count the frames a row owns.  Unlinked rows are clips: the per-row solve as it is
        adaptive = is_adaptive(ode_opt)
        groups = plan.groups()
        gtable = torch.tensor(groups, dtype=torch.int32, device=dev) if linked and adaptive else None
        owner = torch.tensor(plan.owner_mask(), dtype=torch.uint8, device=dev) if linked and adaptive else None
        row_stats = None
        try:
            if linked:
                hip.check(self._lib.samaudio_set_windows(self._ctx, hip.ptr(table), plan.rows, plan.overlap))
            if gtable is not None:
                hip.check(self._lib.samaudio_set_window_groups(self._ctx, hip.ptr(gtable), len(groups), hip.ptr(owner)))
            if adaptive:
                method, params = ode_adaptive(ode_opt)
                rows = wnoise.to(dev, torch.float32).clone().contiguous()
                row_stats = self._solve_adaptive(None, rows, method, params)
            else:
                rows = self.solve(wnoise, ode_opt)
        finally:
            if linked:   # the tables are this call's: the context does not keep the pointers (clearing the windows clears the groups)
                hip.check(self._lib.samaudio_set_window_groups(self._ctx, None, 0, None))
                hip.check(self._lib.samaudio_set_windows(self._ctx, None, 0, 0))
        srow, soff, have = plan.stitch_index()
        latent = rows[torch.tensor(srow, device=dev), torch.tensor(soff, device=dev)]   # frame t from window min(t // S, n - 1)
        if not all(map(all, have)):   # padding frames behind the last window's row: zero
            latent.masked_fill_(~torch.tensor(have, device=dev)[:, :, None], 0)
        self.last_window_latent, self.last_window_plan = rows, plan
        if row_stats is not None:   # one entry per (clip, candidate): every row of a group holds the group's counters
            names = [f"clip {b}, candidate {c}" for b in range(B) for c in range(cand)]
            self._set_ode_stats([[row_stats[first] for first, _, _ in groups]], latent, names=names, windows=plan.counts)
        return latent

    def _rerank(self, batch: Batch, target_wavs: List[torch.Tensor], sizes: List[int], cand: int) -> torch.Tensor:
        """Candidate selection, reference model.py:306-330: visual ranker if a masked video came with the batch, else
        the text ranker, else candidate 0; `idxs = scores.argmax(dim=1)`."""
        B = len(target_wavs)
        sr = self.cfg.audio_codec.sample_rate
        if cand > 1 and self.text_ranker is None and (self.visual_ranker is None or batch.masked_video is None):
            warnings.warn(f"reranking_candidates={cand} but no applicable ranker is attached (model.text_ranker / "
                          "model.visual_ranker): candidate 0 is returned for every clip")
        if cand > 1 and batch.masked_video is not None and self.visual_ranker is not None:
            # (a third-party callable that expects tensors: a MaskedVideo is materialised for it)
            videos = [v.materialize() if hasattr(v, "materialize") else v for v in batch.masked_video]
            scores = self.visual_ranker(extracted_audio=target_wavs, videos=videos, sample_rate=sr)
            return scores.argmax(dim=1)
        if cand > 1 and self.text_ranker is not None:
            input_audio = [audio[:, : int(size)].expand(cand, -1) for audio, size in zip(batch.audios, sizes)]
            more = {}
            if getattr(self.text_ranker, "needs_spans", False):   # (ranking.SoundActivityRanker; after predict_spans the
                if batch.anchors is None:                          # predicted spans are batch.anchors already)
                    raise ValueError("the attached text ranker scores candidates against the prompt's spans: give the processor "
                                     "anchors= or call separate(predict_spans=True) with a span predictor attached")
                more["spans"] = batch.anchors
            scores = self.text_ranker(extracted_audio=target_wavs, input_audio=input_audio,
                                      descriptions=batch.descriptions, sample_rate=sr, **more)
            return scores.argmax(dim=1)
        return torch.zeros(B, dtype=torch.long, device=self.device)

    def predict_spans(self, batch: Batch, audio_features: torch.Tensor, audio_pad_mask: torch.Tensor) -> Batch:
        """reference model.py:231-245: PE-A-Frame on the first 128 feature channels (the codec mean latent) and the
        descriptions -> spans -> "+" anchors -> batch.process_anchors."""
        if self.span_predictor_transform is None:
            raise RuntimeError("predict_spans needs model.span_predictor_transform (descriptions -> the span predictor's "
                               "text inputs: input_ids / attention_mask, or text_pooled)")
        inputs = self.span_predictor_transform(text=batch.descriptions)
        inputs = {k: v for k, v in dict(inputs).items() if k in ("input_ids", "attention_mask", "text_pooled")}
        half = self.cfg.audio_codec.codebook_dim
        output = self.span_predictor(input_features=audio_features[:, :, :half].contiguous(),
                                     padding_mask=audio_pad_mask, return_spans=True, **inputs)
        anchors = [[("+", float(s), float(e)) for s, e in spans] for spans in output.spans]
        batch.process_anchors(anchors)
        return batch

    def attach_rankers(self, tower_precision: Optional[str] = None, **kwargs) -> None:
        """Build the rankers named in the config (reference model.py:94-95) when they point at LOCAL checkpoint
        directories; hub ids cannot be resolved offline and are left unattached (a warning says so).
        `tower_precision` (None = whatever `precision=` says): see from_pretrained."""
        from .ranking import create_ranker
        if tower_precision is not None:
            hip.check_precision(tower_precision, x3_ok=True)
            kwargs["precision"] = tower_precision
        for name in ("visual_ranker", "text_ranker"):
            rc = getattr(self.cfg, name)
            if rc is None or getattr(self, name) is not None:
                continue
            path = getattr(rc, "checkpoint_or_model_id", None)
            if path is not None and not os.path.isdir(path):
                warnings.warn(f"{name}: {path!r} is not a local directory (no hub access offline); not attached")
                continue
            try:
                setattr(self, name, create_ranker(rc, device=str(self.device) if self.device else None, **kwargs))
            except NotImplementedError as exc:  # CLAP / ImageBind / ... wrap third-party models this build does not ship
                warnings.warn(f"{name} not attached: {exc}")

    def unbatch(self, wavs: torch.Tensor, sizes, time_dim: int = -1):
        """reference model.py:340-344"""
        return [row.narrow(dim=time_dim, start=0, length=int(size)) for row, size in zip(wavs, sizes)]
