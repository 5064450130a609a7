"""Resize, rounding, normalisation and patchify of uint8 frames in one HIP kernel (sam_audio_amd/csrc/vit_kernels.hip
resize_frames_kernel; include/samaudio.h samaudio_op_resize_frames / samaudio_vit_encode_frames).

The yardstick is the float64 restatement in tests/resize_ref.py, pinned to torch's CPU kernels by tests/test_vit_frames_cpu.py.  The
kernel must choose the level clamp(rint(reference)) for every pixel, except where the reference lies within delta of a half-integer:
there fp32 arithmetic cannot decide the rounding and one level of difference is allowed.  delta = max(1e-3, 2 x the largest
|torch fp32 - reference| of the case) comes from torch on the CPU, never from the kernel, and such pixels may be at most 2 % of a case
(the reference alone gives 0.1 - 1.3 % on these inputs).  The normalised float of the chosen level is checked bit for bit.
"""
import ctypes as C
import os

import pytest
import torch

from oracle import vit_oracle as V
from sam_audio_amd import hip
from sam_audio_amd.config import PE_VISION_CONFIGS, PerceptionEncoderConfig
from sam_audio_amd.synthetic import init_vision_state_dict
from sam_audio_amd.vision_encoder import PerceptionEncoder
from sam_audio_amd.vision_tower import PEVisionTower
from tests import resize_ref as R

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
# fp32, the plain 16-bit operands and the compensated mode; the CPU simulator carries the bfloat16 library only
PRECISIONS = ["fp32", "bf16", "bf16x3"] if SIM else ["fp32", "bf16", "fp16", "fp16x3"]


def _resize(gpu, u8, S, mode):
    """samaudio_op_resize_frames -> (status, planar f32 [n,3,S,S] on the device)"""
    n, _, H, W = u8.shape
    x = u8.to(gpu).contiguous()
    out = torch.full((n, 3, S, S), float("nan"), device=gpu)
    rc = hip.lib().samaudio_op_resize_frames(hip.ptr(x), n, H, W, S, hip.RESIZE_MODES[mode], hip.ptr(out), hip.current_stream_ptr())
    return rc, out


def _check_levels(got, ref, delta, what):
    """`got`: the kernel's normalised floats; `ref`: the float64 reference, not rounded"""
    level = ((got.double() * 0.5 + 0.5) * 255.0).round()
    assert torch.equal(got, R.normalise(level)), f"{what}: a value is not the normalised float of a level"
    want = R.levels(ref)
    near = ((ref - ref.floor()) - 0.5).abs() <= delta          # within delta of a half-integer
    diff = (level - want).abs()
    wrong = int((diff[~near] != 0).sum())
    print(f"{what}: delta {delta:.2e}, undecided pixels {near.float().mean().item() * 100:.2f} %, of them one level off "
          f"{int((diff[near] != 0).sum())}, wrong elsewhere {wrong}, largest difference {diff.max().item():.0f}")
    assert wrong == 0 and diff.max().item() <= 1
    assert near.float().mean().item() <= 0.02
    assert float(level.min()) >= 0 and float(level.max()) <= 255


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("hw,S", R.CASES, ids=[f"{h}x{w}-{s}" for (h, w), s in R.CASES])
def test_resize_kernel_against_the_float64_restatement(gpu, hw, S, mode):
    u8, ref, delta, _ = R.case(hw[0], hw[1], S, mode)
    rc, out = _resize(gpu, u8, S, mode)
    hip.check(rc)
    _check_levels(out.cpu(), ref, delta, f"resize {mode} {hw} -> {S}")


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
def test_resize_kernel_clamps_bicubic_overshoot_on_a_checkerboard(gpu, mode):
    u8, ref, delta, _ = R.case(45, 61, 56, mode, "checkerboard")
    if mode == "bicubic":
        assert ((ref < -0.5) | (ref > 255.5)).float().mean().item() > 0.2, "the board must overshoot for this check to mean anything"
    rc, out = _resize(gpu, u8, 56, mode)
    hip.check(rc)
    _check_levels(out.cpu(), ref, delta, f"checkerboard {mode}")


@pytest.mark.parametrize("hw,S", R.CASES, ids=[f"{h}x{w}-{s}" for (h, w), s in R.CASES])
def test_resize_kernel_nearest_equals_torch(gpu, hw, S):
    u8 = R.case(hw[0], hw[1], S, "nearest")[0]
    rc, out = _resize(gpu, u8, S, "nearest")
    hip.check(rc)
    assert torch.equal(out.cpu(), R.normalise(R.torch_resize(u8, S, "nearest")))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("S", [56, 112])
def test_frames_of_the_target_size_pass_through_bit_for_bit(gpu, S, mode):
    u8 = R.random_frames(2, S, S, seed=S)
    rc, out = _resize(gpu, u8, S, mode)
    hip.check(rc)
    assert torch.equal(out.cpu(), (u8.float() / 255.0 - 0.5) / 0.5)


def test_unaligned_frame_pointer_and_neighbouring_memory(gpu):
    """The u8 rows are read as aligned 16-byte pieces: a frame pointer at an odd byte offset inside a larger tensor (the slices
    PerceptionEncoder hands over) must give what the same frames give at an aligned address, whatever lies around them."""
    u8 = R.random_frames(3, 45, 61, seed=5)
    hip.check(_resize(gpu, u8, 56, "bicubic")[0])
    want = _resize(gpu, u8, 56, "bicubic")[1].cpu()
    flat = torch.full((u8.numel() + 64,), 255, dtype=torch.uint8)
    for shift in (1, 7, 13):
        flat[shift: shift + u8.numel()] = u8.flatten()
        dev = flat.to(gpu)
        x = dev[shift: shift + u8.numel()].view(u8.shape)
        out = torch.empty(3, 3, 56, 56, device=gpu)
        hip.check(hip.lib().samaudio_op_resize_frames(hip.ptr(x), 3, 45, 61, 56, hip.RESIZE_BICUBIC, hip.ptr(out),
                                                      hip.current_stream_ptr()))
        assert torch.equal(out.cpu(), want), f"shift {shift}"


@pytest.mark.skipif(SIM, reason="2 GB of frames: MI355X only")
def test_frame_offsets_past_2_31(gpu):
    """87 frames of 2160 x 3840 are 2.16 GB: the last frame's second and third channel lie behind byte 2^31, and 77 taps per axis
    loop over many passes through LDS.  A frame must equal what the kernel computes from that frame alone."""
    n, H, W, S = 87, 2160, 3840, 56
    g = torch.Generator(device=gpu).manual_seed(1)
    u8 = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8, device=gpu)
    assert u8.numel() - 2 * H * W > 2 ** 31 > u8.numel() - 3 * H * W
    rc, out = _resize(gpu, u8, S, "bicubic")
    hip.check(rc)
    for f in (0, n - 1):
        rc, one = _resize(gpu, u8[f: f + 1], S, "bicubic")
        hip.check(rc)
        assert torch.equal(out[f: f + 1], one), f"frame {f}"
    last = u8[n - 1:, 2:].cpu()
    _check_levels(out[n - 1:, 2:].cpu(), R.resize64(last, S, "bicubic"), 1e-3, "last channel of 2.16 GB")


def _tower(precision, gpu, name="pe-tiny", seed=8):
    cfg = PE_VISION_CONFIGS[name]
    sd = init_vision_state_dict(cfg, seed=seed)
    tower = PEVisionTower(cfg, precision=precision, device=str(gpu))
    tower.load_state_dict(sd)
    return cfg, sd, tower


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,hw", [(5, (80, 64)), (2, (431, 97))])
def test_encode_frames_equals_encode_image_of_the_planar_output(gpu, precision, n, hw):
    """The kernel's second form - the patch embedding's operand written directly, in the tower's operand type - against its first form
    through patchify: features and tokens bit for bit (im2col indexing, zero padding of Kp), under the poisoned workspace."""
    cfg, _, tower = _tower(precision, gpu)
    u8 = R.random_frames(n, hw[0], hw[1], seed=n)
    for mode in ("bicubic", "nearest"):
        rc, planar = _resize(gpu, u8, cfg.image_size, mode)
        hip.check(rc)
        want, want_tok = tower.encode_image(planar, normalize=True, return_tokens=True)
        got, tok = tower.encode_frames(u8.to(gpu), mode, normalize=True, return_tokens=True)
        assert torch.isfinite(got).all()
        assert torch.equal(got, want) and torch.equal(tok, want_tok), f"{precision} {mode}"


def _encoder(gpu, sd, **kw):
    pe = PE_VISION_CONFIGS["pe-tiny"]
    ecfg = PerceptionEncoderConfig(dim=pe.output_dim, batch_size=3, name="pe-tiny", image_size=pe.image_size)
    enc = PerceptionEncoder(ecfg, device=gpu, precision="fp32", **kw)
    enc.load_state_dict({"model.visual." + k: v for k, v in sd.items()} | {"model.logit_scale": torch.ones(())}, strict=True)
    return enc


def test_perception_encoder_with_the_hip_frame_transform(gpu):
    """uint8 videos of 7 and 4 frames in chunks of batch_size = 3, never as floats: shape, zero time-padding, and every video's features
    within 1e-4 (the bound tests/test_vit_gpu.py holds the torch transform to) of the oracle tower on frames built from the float64
    reference's levels.  A video that already has the target size takes the same path.  The default frame_transform is inert."""
    pe = PE_VISION_CONFIGS["pe-tiny"]
    sd = init_vision_state_dict(pe, seed=8)
    g = torch.Generator().manual_seed(9)
    videos = [torch.randint(0, 256, (7, 3, 80, 64), generator=g, dtype=torch.uint8),
              torch.randint(0, 256, (4, 3, 80, 64), generator=g, dtype=torch.uint8)]
    enc = _encoder(gpu, sd, frame_transform="hip")
    out = enc(videos).cpu()
    assert out.shape == (2, 7, pe.output_dim)
    assert float(out[1, 4:].abs().max()) == 0.0       # time padding
    for i, v in enumerate(videos):
        x = R.normalise(R.levels(R.resize64(v, pe.image_size, "bicubic")))
        want = V.encode_image(sd, pe, x, normalize=True)
        err = (out[i, : v.shape[0]] - want).abs().max().item()
        print(f"hip frame transform, video {i}: features max-abs {err:.2e}")
        assert err < 1e-4
    native = torch.randint(0, 256, (4, 3, pe.image_size, pe.image_size), generator=g, dtype=torch.uint8)
    torch_enc, torch_enc2 = _encoder(gpu, sd), _encoder(gpu, sd)
    assert torch_enc.frame_transform == "torch"
    # identity resize: the tower sees exactly the normalised levels (rows of a batch are independent, so chunking is invisible)
    assert torch.equal(enc([native])[0], enc.tower.encode_image(((native.float() / 255.0 - 0.5) / 0.5).to(gpu), normalize=True))
    # float videos and towers without encode_frames keep the torch path
    assert torch.equal(enc([native.float()]), torch_enc([native.float()]))
    calls = []
    plain = PerceptionEncoder(enc.cfg, tower=lambda f, normalize: calls.append(f.dtype) or torch.zeros(f.shape[0], pe.output_dim),
                              frame_transform="hip")
    plain(videos[1:])
    assert calls == [torch.float32, torch.float32]
    assert torch.equal(torch_enc(videos), torch_enc2(videos))


def test_separate_with_the_hip_frame_transform(gpu):
    """SAMAudio(frame_transform="hip") hands the switch to the PerceptionEncoder that load_state_dict builds; separate() with masked
    videos runs on it and is finite (the parity of this path with the torch transform: the tests above)."""
    from sam_audio_amd import SAMAudio, SAMAudioProcessor, preset_config
    from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
    pe = PE_VISION_CONFIGS["pe-tiny"]
    cfg = preset_config("tiny")
    cfg.vision_encoder = PerceptionEncoderConfig(dim=pe.output_dim, batch_size=3, name="pe-tiny", image_size=pe.image_size)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 4 * hop) for i in range(2)]
    text, tmask = synthetic_text_features(2, 3)
    g = torch.Generator().manual_seed(12)
    videos = [torch.randint(0, 256, (7, 3, 70, 60), generator=g, dtype=torch.uint8),
              torch.randint(0, 256, (5, 3, 56, 56), generator=g, dtype=torch.uint8)]
    batch = SAMAudioProcessor.from_config(cfg)(descriptions=["a", "b"], audios=clips, masked_videos=videos, text_features=text,
                                               text_mask=tmask)
    full = dict(init_state_dict(cfg, seed=3))
    full.update({"vision_encoder.model.visual." + k: v for k, v in init_vision_state_dict(pe, seed=6).items()})
    full["vision_encoder.model.logit_scale"] = torch.ones(())
    with pytest.raises(ValueError):
        SAMAudio(cfg, precision="fp32", device=str(gpu), frame_transform="bogus")
    model = SAMAudio(cfg, precision="fp32", device=str(gpu), frame_transform="hip")
    model.load_state_dict(full, strict=True)
    assert model.vision_encoder.frame_transform == "hip" and hasattr(model.vision_encoder.tower, "encode_frames")
    assert all(v.dtype == torch.uint8 for v in batch.masked_video)
    res = model.separate(batch.to(gpu), noise=synthetic_noise(2, 4).to(gpu))
    assert torch.isfinite(model.last_latent).all()
    assert all(torch.isfinite(w).all() for w in res.target + res.residual)


def test_resize_entry_points_refuse_bad_arguments(gpu):
    u8 = R.random_frames(1, 8, 8, seed=0).to(gpu)
    out = torch.empty(1, 3, 56, 56, device=gpu)
    lib, st = hip.lib(), hip.current_stream_ptr()
    args = lambda **kw: [kw.get("frames", hip.ptr(u8)), kw.get("n", 1), kw.get("height", 8), 8]   # noqa: E731
    for kw in (dict(frames=C.c_void_p(0)), dict(n=0), dict(height=0), dict(mode=7)):
        rc = lib.samaudio_op_resize_frames(*args(**kw), 56, kw.get("mode", hip.RESIZE_BICUBIC), hip.ptr(out), st)
        assert rc == hip.ERR_ARG and lib.samaudio_last_error(), kw
    cfg, _, tower = _tower("fp32", gpu)
    feats = tower.encode_frames(u8, "bicubic")         # sizes the workspace for one frame
    assert torch.isfinite(feats).all()
    for kw in (dict(frames=C.c_void_p(0)), dict(n=0), dict(height=0), dict(mode=7)):
        rc = lib.samaudio_vit_encode_frames(tower._h, *args(**kw), kw.get("mode", hip.RESIZE_BICUBIC), 0, hip.ptr(feats), None, st)
        assert rc == hip.ERR_ARG and lib.samaudio_last_error(), kw
    with pytest.raises(ValueError):
        tower.encode_frames(u8, "lanczos")
    with pytest.raises(TypeError):
        tower.encode_frames(u8.float(), "bicubic")
