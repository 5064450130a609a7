"""Rerankers for `separate(reranking_candidates > 1)` - the reference's `sam_audio.ranking` surface
(reference sam_audio/ranking/ranker.py:9-36, ranking/judge.py:11-42, ranking/__init__.py:15-30) for the rows this build
covers: the Judge, the sound-activity ranker (ranking/sound_activity.py),
the CLAP ranker (ranking/clap.py; DESIGN.md section 10.8: the model is transformers' ClapModel on the HIP towers of
sam_audio_amd/clap.py, from a local checkpoint directory) and ensembles of rankers.  The ImageBind ranker wraps a third-party model
that is not part of this build's environment, and so does a CLAP config without a local checkpoint (the reference downloads
laion_clap's): those configs are reported, not silently ignored.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .config import ClapRankerConfig, JudgeRankerConfig, SoundActivityRankerConfig


class Ranker:
    """forward(**kwargs) -> scores [batch, candidates] (higher = better); reference ranking/ranker.py:9-20."""

    def forward(self, **kwargs) -> torch.Tensor:
        raise NotImplementedError

    def __call__(self, **kwargs) -> torch.Tensor:
        return self.forward(**kwargs)


class EnsembleRanker(Ranker):
    """Weighted sum of rankers (reference ranking/ranker.py:23-36)."""

    def __init__(self, rankers: Sequence[Ranker], weights: Sequence[float]):
        assert len(rankers) == len(weights)
        self.rankers, self.weights = list(rankers), list(weights)

    @property
    def needs_spans(self) -> bool:
        """separate() hands `spans=` over when any member asks for them (the others take them as **kwargs)"""
        return any(getattr(r, "needs_spans", False) for r in self.rankers)

    def forward(self, **kwargs) -> torch.Tensor:
        result = None
        for weight, ranker in zip(self.weights, self.rankers):
            score = weight * ranker(**kwargs)
            result = score if result is None else result + score
        return result


class JudgeRanker(Ranker):
    """reference ranking/judge.py:11-42.  `model` is a loaded `SAMAudioJudgeModel`, `processor` a
    `SAMAudioJudgeProcessor`; from a config they are loaded from the local checkpoint directory.

    The reference expands the mixture to one copy per candidate before the processor (ranking/judge.py:31-33) and the
    Judge encodes every copy; here the mixture is handed over once per clip (`score_candidates`), same scores."""

    def __init__(self, config: Optional[JudgeRankerConfig] = None, model=None, processor=None,
                 tower_precision: Optional[str] = None, **model_kwargs):
        self.config = config
        if tower_precision is not None:   # the Judge's precision by its SAMAudio-side name ("fp16x3": the compensated towers)
            model_kwargs["precision"] = tower_precision
        if model is None or processor is None:
            from .judge import SAMAudioJudgeModel
            from .processor import SAMAudioJudgeProcessor
            path = config.checkpoint_or_model_id
            model = model or SAMAudioJudgeModel.from_pretrained(path, **model_kwargs)
            processor = processor or SAMAudioJudgeProcessor.from_pretrained(path)
        self.model, self.processor = model, processor

    @torch.inference_mode()
    def forward(self, input_audio: List[torch.Tensor], extracted_audio: List[torch.Tensor], descriptions: List[str],
                sample_rate: int = 48_000, **kwargs) -> torch.Tensor:
        bsz, ncandidates = len(extracted_audio), len(extracted_audio[0])
        # input_audio[b] is the mixture expanded to [candidates, n] (reference model.py:319-322): row 0 is the clip
        mixtures = [x[0][None] for x in input_audio]
        extracted = [x[None] for candidates in extracted_audio for x in candidates]
        processed = self.processor(text=list(descriptions), input_audio=mixtures, separated_audio=extracted,
                                   sampling_rate=sample_rate)
        return self.model.score_candidates(
            input_ids=processed["input_ids"], attention_mask=processed.get("attention_mask"),
            input_values=processed["input_values"], separated_values=processed["separated_values"],
            candidates=ncandidates, padding_mask=processed["padding_mask"]).view(bsz, ncandidates)


class SoundActivityRanker(Ranker):
    """reference ranking/sound_activity.py:96-129: how well a candidate's nonsilent spans (pydub's silence detection at 24 kHz)
    overlap the prompt's spans - iou, recall or precision.  No weights.  The work is two HIP launches per clip on the
    [candidates, n] view (sam_audio_amd/activity.py), nothing is read back.

    Departure from the reference (like quirk Q13, the reference class cannot do what it is for): its forward hands `wav`
    [candidates, n] to the encoder as the CHANNELS of one clip, returns one score per clip instead of [batch, candidates], and
    SAMAudio.separate never passes it `spans` (dead code).  This class keeps its algorithm and its config and
    gives it the `Ranker` contract: every candidate is scored as a mono clip, the result is [batch, candidates] (higher = better),
    and `SAMAudio.separate` passes `spans=batch.anchors` to rankers with `needs_spans`.  Kept from the reference: the reference
    spans are (start, end) of EVERY anchor of the clip, whatever its token ("+" or "-"), and overlapping ones count twice.
    The statement it is held to is tests/activity_ref.py: pinned to CPython's audioop, unpinned vs pydub / torchcodec."""

    needs_spans = True

    def __init__(self, config: Optional[SoundActivityRankerConfig] = None):
        self.config = config if config is not None else SoundActivityRankerConfig()

    @torch.inference_mode()
    def forward(self, extracted_audio: List[torch.Tensor], spans, sample_rate: int = 48_000, **kwargs) -> torch.Tensor:
        from . import activity
        if len(spans) != len(extracted_audio):
            raise ValueError(f"{len(extracted_audio)} clips but spans for {len(spans)}")
        device = extracted_audio[0].device
        bsz, ncandidates = len(extracted_audio), len(extracted_audio[0])
        # every clip's reference spans in one small float64 upload; a clip's rows of it are a view
        flat = [[float(a[1]), float(a[2])] for clip in spans for a in clip]
        ref = torch.tensor(flat, dtype=torch.float64).reshape(len(flat), 2).to(device) if flat else None
        scores = torch.empty(bsz, ncandidates, dtype=torch.float32, device=device)
        first = 0
        for b, (wav, clip) in enumerate(zip(extracted_audio, spans)):
            activity.activity(wav, sample_rate, ref[first: first + len(clip)] if clip else None, self.config.metric,
                              self.config.sil_threshold, self.config.threshold_mode, out=scores[b])
            first += len(clip)
        return scores


class ClapRanker(Ranker):
    """reference ranking/clap.py:33-86: the cosine of CLAP's audio embedding of every candidate and its text embedding of the clip's
    description, [batch, candidates] fp32 on the device (higher = better).  `model` is a loaded `clap.ClapTower`, `tokenizer` the
    checkpoint's (RoBERTa's); from a config both are loaded from the local checkpoint directory.  Every clip's [candidates, n] view
    goes to the tower as it is; nothing is read back.

    Pinned to transformers' ClapModel / ClapFeatureExtractor, unpinned vs laion_clap (absent here): the int16 round trip's constant
    and laion's `fmin` are taken on trust.  A candidate longer than 10 s is cropped at the head (`truncation="head"`, deterministic:
    this build's default); the reference crops at a random offset - `truncation="rand_trunc"` draws one per candidate from
    `generator` (a torch.Generator; None = torch's global one).  The towers are fp32 only: a `precision=` is accepted and ignored."""

    def __init__(self, config: Optional[ClapRankerConfig] = None, model=None, tokenizer=None, truncation: str = "head",
                 generator: Optional[torch.Generator] = None, device=None, **_ignored):
        if truncation not in ("head", "rand_trunc"):
            raise ValueError(f"truncation must be 'head' or 'rand_trunc', got {truncation!r}")
        self.config, self.truncation, self.generator = config, truncation, generator
        if model is None or tokenizer is None:
            path = getattr(config, "checkpoint", None)
            if path is None:
                raise NotImplementedError(_CLAP_NEEDS_A_DIRECTORY)
            if model is None:
                from .clap import ClapTower
                model = ClapTower.from_pretrained(path, device=device)
            if tokenizer is None:
                from transformers import AutoTokenizer
                tokenizer = AutoTokenizer.from_pretrained(path)
        self.model, self.tokenizer = model, tokenizer

    def _offsets(self, samples: int, sample_rate: int, candidates: int) -> Optional[List[int]]:
        """crop offsets of one clip's candidates, at the tower's rate; None = the head"""
        if self.truncation == "head":
            return None
        from .audio import resample_length
        n = resample_length(samples, sample_rate, self.model.sample_rate) if sample_rate != self.model.sample_rate else samples
        overflow = n - int(self.model.cfg.max_length)
        if overflow <= 0:
            return None
        return torch.randint(0, overflow + 1, (candidates,), generator=self.generator).tolist()

    @torch.inference_mode()
    def forward(self, extracted_audio: List[torch.Tensor], descriptions: List[str], sample_rate: int = 48_000, **kwargs) -> torch.Tensor:
        bsz, ncandidates = len(extracted_audio), len(extracted_audio[0])
        if len(descriptions) != bsz:
            raise ValueError(f"{bsz} clips but {len(descriptions)} descriptions")
        device = extracted_audio[0].device
        audio = torch.empty(bsz * ncandidates, self.model.dim, dtype=torch.float32, device=device)
        for b, wav in enumerate(extracted_audio):
            if wav.dim() != 2 or wav.shape[0] != ncandidates:
                raise ValueError("every clip must be [candidates, samples] with the same number of candidates")
            self.model.audio_embed(wav, int(sample_rate), offsets=self._offsets(wav.shape[1], int(sample_rate), ncandidates),
                                   out=audio[b * ncandidates: (b + 1) * ncandidates])
        limit = min(77, int(self.model.cfg.text_max_positions) - int(self.model.cfg.text_pad_id) - 1)   # (77: laion_clap's tokenizer call)
        tokens = self.tokenizer(list(descriptions), padding=True, truncation=True, max_length=limit, return_tensors="pt")
        text = self.model.text_embed(tokens["input_ids"], tokens.get("attention_mask"))
        return self.model.score(audio, text, ncandidates)


_CLAP_NEEDS_A_DIRECTORY = (
    "ranker kind 'clap' without a checkpoint wraps a third-party model: the reference downloads laion_clap's 630k-best.pt from the "
    "hub, which this build cannot do.  Pass {'kind': 'clap', 'checkpoint': <local ClapModel.save_pretrained directory>}, or attach "
    "a callable ranker to model.text_ranker")


def create_ranker(config, **kwargs) -> Optional[Ranker]:
    """reference ranking/__init__.py:15-30."""
    if config is None:
        return None
    if isinstance(config, Ranker) or callable(config):
        return config
    if isinstance(config, JudgeRankerConfig):
        return JudgeRanker(config, **kwargs)
    if isinstance(config, SoundActivityRankerConfig):
        return SoundActivityRanker(config)
    if isinstance(config, dict) and config.get("kind") == "clap":
        from .config import parse_ranker_config
        config = parse_ranker_config(config)
    if isinstance(config, ClapRankerConfig):
        return ClapRanker(config, **kwargs)   # (NotImplementedError without a checkpoint directory: nothing can be downloaded)
    kind = config.get("kind") if isinstance(config, dict) else getattr(config, "kind", None)
    if kind == "ensemble":
        pairs = config["rankers"].values() if isinstance(config, dict) else config.rankers.values()
        from .config import parse_ranker_config
        cfgs, weights = zip(*[(parse_ranker_config(c) if isinstance(c, dict) else c, w) for c, w in pairs])
        return EnsembleRanker([create_ranker(c, **kwargs) for c in cfgs], list(weights))
    raise NotImplementedError(
        f"ranker kind {kind!r} wraps a third-party model (ImageBind / ...) that this build does not ship; "
        "attach a callable ranker to model.text_ranker / model.visual_ranker instead")
