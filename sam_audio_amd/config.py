"""Configuration objects for the MI355X-native SAM-Audio separate() path.

Same field names / defaults as the reference's plain-Python config classes
(/root/reference/sam_audio/model/config.py:10-41 DACVAEConfig, :49-60 T5EncoderConfig,
:69-83 PerceptionEncoderConfig, :86-135 TransformerConfig, :204-231 SAMAudioConfig) so a
reference ``config.json`` parses unchanged.  Re-expressed as dataclasses and without the
``core`` (perception_models) import the reference needs only as a type annotation.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, fields
from typing import Any, Dict, List, Optional


def _build(cls, raw):
    if raw is None:
        return cls()
    if isinstance(raw, cls):
        return raw
    known = {f.name for f in fields(cls)}
    unknown = set(raw) - known
    if unknown:
        # the reference would raise TypeError from cls(**raw) as well
        raise TypeError(f"{cls.__name__}: unexpected config keys {sorted(unknown)}")
    return cls(**raw)


@dataclass
class DACVAEConfig:
    encoder_dim: int = 64
    encoder_rates: List[int] = field(default_factory=lambda: [2, 8, 10, 12])
    latent_dim: int = 1024
    decoder_dim: int = 1536
    decoder_rates: List[int] = field(default_factory=lambda: [12, 10, 8, 2])
    n_codebooks: int = 16
    codebook_size: int = 1024
    codebook_dim: int = 128
    quantizer_dropout: bool = False
    sample_rate: int = 48_000
    mean: float = 0.0
    std: float = 1.0

    @property
    def hop_length(self) -> int:
        return int(math.prod(self.encoder_rates))


@dataclass
class T5EncoderConfig:
    name: str = "t5-base"
    max_length: Optional[int] = 512
    pad_mode: str = "longest"
    dim: int = 768


@dataclass
class PerceptionEncoderConfig:
    dim: int = 1024
    batch_size: int = 300
    name: str = "PE-Core-L14-336"
    normalize_feature: bool = True
    interpolation_mode: str = "BICUBIC"
    image_size: int = 336


@dataclass
class PEVisionConfig:
    """Architecture of the PE-Core vision tower the reference instantiates by NAME
    (`pe.CLIP.from_config(cfg.name)`, reference sam_audio/model/vision_encoder.py:86; the table of named configs
    lives in the un-vendored perception_models package, so the published PE-Core-L14-336 numbers are restated here)."""
    image_size: int = 336
    patch_size: int = 14
    width: int = 1024
    layers: int = 24
    heads: int = 16
    mlp_ratio: float = 4.0
    output_dim: int = 1024
    use_cls_token: bool = True
    use_abs_posemb: bool = True
    use_rope2d: bool = True
    use_ln_pre: bool = True
    use_ln_post: bool = True
    pool_type: str = "attn"          # "attn" | "tok" | "avg"
    attn_pooler_heads: int = 8
    act: str = "gelu"                # "gelu" (erf) | "quick_gelu"
    ln_eps: float = 1e-5

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def tokens(self) -> int:
        return self.grid * self.grid + int(self.use_cls_token)

    @property
    def mlp_width(self) -> int:
        return int(self.width * self.mlp_ratio)


PE_VISION_CONFIGS = {
    "PE-Core-L14-336": PEVisionConfig(),
    # stand-ins for tests (not published models): same structure, small dims
    "pe-tiny": PEVisionConfig(image_size=56, patch_size=14, width=128, layers=2, heads=2, output_dim=64,
                              attn_pooler_heads=2),
    "pe-mini": PEVisionConfig(image_size=112, patch_size=14, width=256, layers=3, heads=4, output_dim=128,
                              attn_pooler_heads=2),
}


@dataclass
class TransformerConfig:
    dim: int = 2048
    n_heads: int = 16
    n_layers: int = 16
    dropout: float = 0.1
    norm_eps: float = 1.0e-05
    qk_norm: bool = True
    fc_bias: bool = False
    ffn_exp: int = 4
    ffn_dim_multiplier: int = 1
    multiple_of: int = 64
    non_linearity: str = "swiglu"
    use_rope: bool = True
    max_positions: int = 10000
    frequency_embedding_dim: int = 256
    timestep_non_linearity: str = "swiglu"
    t_block_non_linearity: str = "silu"
    t_block_bias: bool = True
    context_dim: int = 2048
    context_non_linearity: str = "swiglu"
    context_embedder_dropout: float = 0.0
    context_norm: bool = False
    out_channels: int = 256
    in_channels: Optional[int] = None

    @property
    def head_dim(self) -> int:
        return self.dim // self.n_heads

    @property
    def ffn_hidden(self) -> int:
        """SwiGLU hidden width, rule of reference transformer.py:176-185."""
        hidden = int(self.ffn_exp * self.dim)
        if self.non_linearity == "swiglu":
            hidden = int(2 * hidden / 3)
        hidden = int(self.ffn_dim_multiplier * hidden)
        return self.multiple_of * ((hidden + self.multiple_of - 1) // self.multiple_of)

    @property
    def rope_theta(self) -> float:
        # reference transformer.py:405-409
        return float(max(10000, 2 * self.max_positions))

    def check_supported(self) -> None:
        """The HIP path implements the configuration family the reference ships."""
        problems = []
        if self.head_dim not in (64, 128):   # 128: every kernel tuned for it; 64: the general kernel forms (csrc/engine.hip finalize)
            problems.append(f"head_dim (dim / n_heads) must be 128 or 64 (got {self.head_dim})")
        if self.dim % self.n_heads:
            problems.append("dim must be divisible by n_heads")
        if not self.qk_norm:
            problems.append("qk_norm=False")
        if self.fc_bias:
            problems.append("fc_bias=True")
        if not self.use_rope:
            problems.append("use_rope=False")
        if not self.t_block_bias:
            problems.append("t_block_bias=False")
        if self.context_norm:
            problems.append("context_norm=True")
        if self.context_dim != self.dim:
            problems.append("context_dim != dim")
        if self.in_channels is not None:
            problems.append("in_channels (data_proj) is not used by SAMAudio")
        for name in ("non_linearity", "timestep_non_linearity", "context_non_linearity"):
            if getattr(self, name) != "swiglu":
                problems.append(f"{name} must be 'swiglu'")
        if self.t_block_non_linearity != "silu":
            problems.append("t_block_non_linearity must be 'silu'")
        if self.frequency_embedding_dim % 64:
            problems.append("frequency_embedding_dim must be a multiple of 64")
        if self.ffn_hidden % 64:   # w2's K axis: every GEMM form (fp32, 16-bit, split operands over K' = 3F) steps K by 64
            problems.append(f"ffn_hidden must be a multiple of 64 (got {self.ffn_hidden}: multiple_of={self.multiple_of})")
        if problems:
            raise NotImplementedError(
                "TransformerConfig outside the HIP path's supported family: " + "; ".join(problems)
            )


@dataclass
class JudgeRankerConfig:
    checkpoint_or_model_id: str = "facebook/sam-audio-judge"
    kind: str = "judge"


@dataclass
class SoundActivityRankerConfig:
    """reference model/config.py:163-174.  The mode and the metric are checked here; the reference fails on them at the first call."""
    threshold_mode: str = "rel_to_max"
    sil_threshold: float = -40
    metric: str = "iou"
    kind: str = "sound_activity"

    def __post_init__(self):
        if self.threshold_mode not in ("abs", "rel_to_max"):
            raise ValueError(f"SoundActivityRankerConfig: threshold_mode must be 'abs' or 'rel_to_max', got {self.threshold_mode!r}")
        if self.metric not in ("iou", "recall", "precision"):
            raise ValueError(f"SoundActivityRankerConfig: metric must be 'iou', 'recall' or 'precision', got {self.metric!r}")


@dataclass
class ClapRankerConfig:
    """reference model/config.py ClapRankerConfig.  `checkpoint`: a local `ClapModel.save_pretrained` directory (Hugging Face key
    names).  None is what the reference resolves by downloading lukewys/laion_clap's 630k-best.pt from the hub: impossible offline,
    and laion's own key names cannot be checked here - ranking.create_ranker refuses it."""
    checkpoint: Optional[str] = None
    kind: str = "clap"


def parse_ranker_config(raw: Optional[Dict[str, Any]]):
    """The Judge ranker, the sound-activity ranker and the CLAP ranker (section 10.8) are
    built here; ImageBind is a third-party model without a statement in this environment, so its config is kept as an opaque dict.
    So is an ensemble's: ranking.create_ranker parses its members with this function."""
    if raw is None:
        return None
    raw = dict(raw)
    if raw.get("kind") == "judge":
        raw.pop("kind")
        return JudgeRankerConfig(**raw)
    if raw.get("kind") == "sound_activity":
        raw.pop("kind")
        return SoundActivityRankerConfig(**raw)
    if raw.get("kind") == "clap":
        raw.pop("kind")
        return ClapRankerConfig(**raw)
    return raw


class SAMAudioConfig:
    def __init__(
        self,
        in_channels: int = 768,
        audio_codec=None,
        text_encoder=None,
        vision_encoder=None,
        transformer=None,
        num_anchors: int = 3,
        anchor_embedding_dim: int = 128,
        visual_ranker=None,
        text_ranker=None,
        span_predictor: Optional[str] = "pe-a-frame-large",
    ):
        self.in_channels = in_channels
        self.audio_codec = _build(DACVAEConfig, audio_codec)
        self.text_encoder = _build(T5EncoderConfig, text_encoder)
        self.vision_encoder = _build(PerceptionEncoderConfig, vision_encoder)
        self.transformer = _build(TransformerConfig, transformer)
        self.num_anchors = num_anchors
        self.anchor_embedding_dim = anchor_embedding_dim
        self.visual_ranker = parse_ranker_config(visual_ranker)
        self.text_ranker = parse_ranker_config(text_ranker)
        self.span_predictor = span_predictor

    def check_supported(self) -> None:
        self.transformer.check_supported()
        c = self.audio_codec
        if self.in_channels != 6 * c.codebook_dim:
            raise NotImplementedError("in_channels must be 6*codebook_dim (noisy|zeros|features)")
        if self.transformer.out_channels != 2 * c.codebook_dim:
            raise NotImplementedError("transformer.out_channels must be 2*codebook_dim")
        if len(c.encoder_rates) != 4 or len(c.decoder_rates) != 4:
            raise NotImplementedError("codec must have 4 down/up-sampling stages")
        if any(r % 2 for r in list(c.encoder_rates) + list(c.decoder_rates)):
            raise NotImplementedError("codec strides must be even")
        if self.anchor_embedding_dim % 64 or c.codebook_dim % 64:
            raise NotImplementedError("anchor_embedding_dim / codebook_dim must be multiples of 64")


@dataclass
class PEAVTransformerConfig:
    """Configuration of the PE-AV `Transformer` the Judge / PE-A-Frame instantiate (reference judge.py:46-47;
    the class is `core.audio_visual_encoder.config.TransformerConfig` of the un-vendored perception_models, used by
    the reference only as a type: config.py:6,238-249).  Field names follow the Hugging Face port of the same
    network (transformers/models/pe_audio/configuration_pe_audio.py:50-68, defaults = pe-av-large) - a documented
    assumption, since the original field names are not reachable offline."""
    hidden_size: int = 1792
    intermediate_size: int = 4800
    num_hidden_layers: int = 6
    num_attention_heads: int = 14
    num_key_value_heads: Optional[int] = None
    head_dim: int = 128
    hidden_act: str = "silu"
    max_position_embeddings: int = 10000
    rms_norm_eps: float = 1e-5
    rope_parameters: Optional[Dict[str, Any]] = None
    attention_bias: bool = False
    attention_dropout: float = 0.0
    initializer_range: float = 0.02

    @property
    def rope_theta(self) -> float:
        return float((self.rope_parameters or {}).get("rope_theta", 20000))

    def check_supported(self) -> None:
        problems = []
        if self.head_dim != 128 or self.hidden_size != self.num_attention_heads * 128:
            problems.append("hidden_size must be num_attention_heads * 128")
        if self.hidden_size % 256:
            problems.append("hidden_size must be a multiple of 256")
        if self.num_key_value_heads not in (None, self.num_attention_heads):
            problems.append("grouped-query attention")
        if self.hidden_act != "silu":
            problems.append("hidden_act must be 'silu'")
        if self.intermediate_size % 64:
            problems.append("intermediate_size must be a multiple of 64")
        if (self.rope_parameters or {}).get("rope_type", "default") != "default":
            problems.append("only default RoPE")
        if problems:
            raise NotImplementedError("PEAVTransformerConfig outside the HIP path's family: " + "; ".join(problems))


class SAMAudioJudgeConfig:
    """reference config.py:234-251.  `text_model` stays a plain dict of ModernBertConfig arguments (the text tower
    runs on PyTorch-ROCm through transformers)."""

    _warned_prenorm = False

    def __init__(self, audio_codec=None, transformer=None, text_model: Optional[Dict[str, Any]] = None,
                 finetune_transformer=None, nth_text_layer: Optional[int] = 22, bottleneck_dim: int = 256,
                 last_text_layer_prenorm: Optional[bool] = None):
        """`last_text_layer_prenorm` (no reference counterpart): what `hidden_states[nth_text_layer]` means when
        nth_text_layer == num_hidden_layers (the reference's default, 22 on a 22-layer tower, judge.py:74-88).  transformers
        4.48 - 4.5x - the generation the reference pins and the released Judge checkpoint was trained with - append the last
        layer's output BEFORE `final_norm`; transformers 5.x record the normalised tensor there.  True (default) = the 4.x
        meaning whatever transformers version is installed; False = the 5.x meaning (= last_hidden_state)."""
        if last_text_layer_prenorm is None:   # left at its default: say so once where the two meanings differ
            last_text_layer_prenorm = True
            layers = (text_model or {}).get("num_hidden_layers", 22)
            if nth_text_layer == layers and not SAMAudioJudgeConfig._warned_prenorm:
                try:
                    import transformers
                    major = int(transformers.__version__.split(".")[0])
                except Exception:   # transformers absent: nothing to disagree with
                    major = 0
                if major >= 5:
                    import warnings
                    warnings.warn(
                        f"SAMAudioJudgeConfig: nth_text_layer == num_hidden_layers ({layers}) and transformers {transformers.__version__} "
                        "is installed - under transformers 5.x the reference's hidden_states[nth_text_layer] is the tensor AFTER "
                        "final_norm, this build defaults to the 4.x meaning (before it, what the released Judge checkpoint was "
                        "trained with).  Pass last_text_layer_prenorm=True / False to choose explicitly.")
                    SAMAudioJudgeConfig._warned_prenorm = True
        self.last_text_layer_prenorm = bool(last_text_layer_prenorm)
        self.audio_codec = _build(DACVAEConfig, audio_codec)
        self.transformer = _build(PEAVTransformerConfig, transformer)
        self.text_model = dict(text_model or {})
        self.finetune_transformer = _build(PEAVTransformerConfig, finetune_transformer)
        self.nth_text_layer = nth_text_layer
        self.bottleneck_dim = bottleneck_dim

    @property
    def text_hidden(self) -> int:
        return int(self.text_model.get("hidden_size", 768))  # ModernBertConfig default

    def check_supported(self) -> None:
        self.transformer.check_supported()
        self.finetune_transformer.check_supported()
        if self.bottleneck_dim % 64 or self.audio_codec.codebook_dim % 64 or self.text_hidden % 64:
            raise NotImplementedError("bottleneck_dim / codebook_dim / text hidden size must be multiples of 64")


class PEAudioFrameConfig:
    """PE-A-Frame span predictor (reference model.py:96-102: `PEAudioFrame.from_config("pe-a-frame-large")`,
    un-vendored).  Shape of the Hugging Face port: transformers/models/pe_audio/configuration_pe_audio.py:88-135
    (audio tower = PE-AV transformer on DAC codec features, text tower = ModernBERT, contrastive heads)."""

    def __init__(self, audio=None, text_model: Optional[Dict[str, Any]] = None, codebook_dim: int = 128,
                 threshold: float = 0.5):
        self.audio = _build(PEAVTransformerConfig, audio)
        tm = dict(hidden_size=1024, intermediate_size=2624, num_hidden_layers=22, num_attention_heads=16)
        tm.update(text_model or {})
        self.text_model = tm
        self.codebook_dim = codebook_dim
        self.threshold = threshold

    @property
    def text_hidden(self) -> int:
        return int(self.text_model["hidden_size"])

    def check_supported(self) -> None:
        self.audio.check_supported()
        if self.codebook_dim % 64 or self.text_hidden % 64:
            raise NotImplementedError("codebook_dim / text hidden size must be multiples of 64")


# Labelled stand-ins for the checkpoint sizes whose real config.json is not reachable offline
# (SURVEY.md §0, §8d).  head_dim 128 and the reference FFN rule are kept.
SIZE_PRESETS: Dict[str, Dict[str, int]] = {
    "tiny": dict(dim=256, n_heads=2, n_layers=2),        # test-only
    "mini": dict(dim=512, n_heads=4, n_layers=3),        # test-only
    "small*": dict(dim=1536, n_heads=12, n_layers=12),   # ASSUMED stand-in for sam-audio-small
    "default": dict(dim=2048, n_heads=16, n_layers=16),  # reference config.py defaults
    "large*": dict(dim=2816, n_heads=22, n_layers=22),   # ASSUMED stand-in for sam-audio-large
}


def preset_config(size: str, **overrides) -> SAMAudioConfig:
    dims = dict(SIZE_PRESETS[size])
    dims["context_dim"] = dims["dim"]
    dims.update(overrides.pop("transformer", {}))
    return SAMAudioConfig(transformer=dims, **overrides)
