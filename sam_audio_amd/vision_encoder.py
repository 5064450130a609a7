"""`PerceptionEncoder` - host wrapper with the interface of the reference's visual-prompt encoder
(reference sam_audio/model/vision_encoder.py:40-113; SURVEY.md section 8 row a4 / "next" row f3).

This wrapper owns what the reference file owns - resize, scaling, normalisation, chunking by `batch_size`, time
padding.  With `frame_transform="hip"` the first three run inside the tower's first kernel
(`PEVisionTower.encode_frames`).  The tower is `pe.CLIP.from_config(cfg.name)` in the reference (un-vendored
perception_models); here it is `sam_audio_amd.vision_tower.PEVisionTower`, the same network on the HIP library (built by default for the config
names in `config.PE_VISION_CONFIGS`), or any injected callable `encode_image(frames [N,3,S,S] float, normalize=bool)
-> [N, dim]`.  `SAMAudio.vision_encoder = PerceptionEncoder(cfg.vision_encoder, device=...)` + `load_state_dict`
enables `separate()` with `masked_videos`.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import torch

from .config import PerceptionEncoderConfig

_MODES = {"NEAREST": "nearest", "BILINEAR": "bilinear", "BICUBIC": "bicubic"}
FRAME_TRANSFORMS = ("torch", "hip")


class PerceptionEncoder:
    def __init__(self, cfg: Optional[PerceptionEncoderConfig] = None, tower: Optional[Callable] = None, device=None,
                 precision: str = "bf16", frame_transform: str = "torch"):
        """`frame_transform`: who resizes, rounds and normalises the frames.
        "torch" (default): `transform` - torch ops on a float copy of the whole video, then the tower in chunks of `batch_size`.
        "hip": a uint8 video on a tower that has `encode_frames` (PEVisionTower) is chunked by `batch_size` AS uint8 and every chunk goes
        through `tower.encode_frames`, where one HIP kernel resizes, rounds, normalises and writes the patch embedding's operand: no
        float copy of the video exists, whatever its resolution; frames that already have the target size take the same path.  A
        video of any other dtype, or an injected tower without `encode_frames`, takes the "torch" path.  A `processor.MaskedVideo`
        item (`SAMAudioProcessor(video_transform="hip")`) is masked and picked by that kernel as well, each distinct frame encoded
        once (`_encode_masked`); on the "torch" path it is materialised first."""
        if frame_transform not in FRAME_TRANSFORMS:
            raise ValueError(f"frame_transform must be one of {FRAME_TRANSFORMS}, not {frame_transform!r}")
        self.frame_transform = frame_transform
        self.cfg = cfg or PerceptionEncoderConfig()
        self.batch_size, self.dim = self.cfg.batch_size, self.cfg.dim
        self.normalize_feature, self.image_size = self.cfg.normalize_feature, self.cfg.image_size
        mode = self.cfg.interpolation_mode.upper()
        if mode not in _MODES:  # reference vision_encoder.py:93-99
            raise ValueError(f"Unsupported interpolation_mode: {self.cfg.interpolation_mode}")
        self.mode = _MODES[mode]
        self.device = device
        if tower is None:
            from .config import PE_VISION_CONFIGS
            if self.cfg.name in PE_VISION_CONFIGS:   # reference vision_encoder.py:86: pe.CLIP.from_config(cfg.name)
                from .vision_tower import PEVisionTower
                pe = PE_VISION_CONFIGS[self.cfg.name]
                if pe.output_dim != self.dim or pe.image_size != self.image_size:
                    raise ValueError(f"vision_encoder dim / image_size ({self.dim}, {self.image_size}) do not match the "
                                     f"named PE config {self.cfg.name!r} ({pe.output_dim}, {pe.image_size})")
                tower = PEVisionTower(name=self.cfg.name, precision=precision, device=device)
        self.tower = tower

    def load_state_dict(self, state_dict, strict: bool = True):
        """The `vision_encoder.*` tensors of a SAMAudio checkpoint (`model.visual.*` = the PE-Core tower)."""
        if not hasattr(self.tower, "load_state_dict"):
            raise NotImplementedError("the attached tower takes no weights")
        if self.device is not None and getattr(self.tower, "device", None) is None:
            self.tower.to(self.device)
        return self.tower.load_state_dict(state_dict, strict=strict)

    def transform(self, video: torch.Tensor) -> torch.Tensor:
        """uint8 / float frames [T, 3, H, W] -> normalised float [T, 3, S, S] (reference vision_encoder.py:91-113:
        Resize((S, S), interp) on a tensor -> x / 255 -> Normalize(0.5, 0.5)).  torchvision's tensor Resize
        antialiases bilinear / bicubic down-scaling by default; F.interpolate(antialias=True) is the same kernel."""
        x = video.float()
        if x.shape[-2:] != (self.image_size, self.image_size):
            kw = {"antialias": True, "align_corners": False} if self.mode != "nearest" else {}
            x = torch.nn.functional.interpolate(x, size=(self.image_size, self.image_size), mode=self.mode, **kw)
            if not video.is_floating_point():
                # torchvision's tensor Resize interpolates integer frames in float and casts back (round; uint8 is
                # clamped to 0..255, which also removes bicubic overshoot) before the `/ 255`
                x = x.round()
                if video.dtype == torch.uint8:
                    x = x.clamp(0, 255)
        return (x / 255.0 - 0.5) / 0.5

    def encode(self, frames: torch.Tensor) -> torch.Tensor:
        if self.tower is None:
            raise NotImplementedError(
                f"no vision tower for config name {self.cfg.name!r}: known PE configs are built on the HIP library "
                "(sam_audio_amd.vision_tower), anything else needs `tower=` (a callable encode_image(frames, "
                "normalize=...) -> [N, dim])")
        return self.tower(frames, normalize=self.normalize_feature)

    @torch.no_grad()
    def forward(self, videos: List[torch.Tensor]) -> torch.Tensor:
        """list of [T_i, 3, H, W] -> [B, max T_i, dim], zero-padded along time (reference vision_encoder.py:47-70)."""
        result = []
        for video in videos:
            video = video.to(self.device) if self.device is not None else video
            if hasattr(video, "materialize"):   # processor.MaskedVideo: frames, mask and index of `(frames * mask.eq(0))[index]`
                if self.frame_transform == "hip" and hasattr(self.tower, "encode_frames"):
                    result.append(self._encode_masked(video))
                    continue
                video = video.materialize()
            if self.frame_transform == "hip" and video.dtype == torch.uint8 and hasattr(self.tower, "encode_frames"):
                encode = lambda v: self.tower.encode_frames(v, self.mode, normalize=self.normalize_feature)   # noqa: E731
            else:
                video, encode = self.transform(video), self.encode
            if self.batch_size > 0 and video.size(0) > self.batch_size:
                parts = [encode(video[i: i + self.batch_size]) for i in range(0, video.size(0), self.batch_size)]
                result.append(torch.cat(parts, dim=0))
            else:
                result.append(encode(video))
        return torch.nn.utils.rnn.pad_sequence(result, batch_first=True, padding_value=0.0)

    def _encode_masked(self, video) -> torch.Tensor:
        """A MaskedVideo on the tower's kernel: every DISTINCT picked frame is encoded once, in chunks of `batch_size`, masked and
        picked by the launch that resizes it (`tower.encode_frames(frames, masks=, index=)`); the features are then gathered into
        the picked order - a video with fewer frames than the clip has latent steps does not go through the tower repeatedly."""
        index = video.index if video.index is not None else torch.arange(video.frames.size(0))
        uniq, inverse = index.unique(return_inverse=True)
        step = self.batch_size if self.batch_size > 0 else uniq.numel()
        parts = [self.tower.encode_frames(video.frames, self.mode, normalize=self.normalize_feature, masks=video.mask,
                                          index=uniq[i: i + step]) for i in range(0, uniq.numel(), step)]
        feats = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        return feats[inverse.to(feats.device)]

    __call__ = forward
