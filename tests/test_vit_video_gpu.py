"""Frame picking and the object mask inside the frame kernel (sam_audio_amd/csrc/vit_kernels.hip resize_frames_kernel with a ResizeVideo
argument; include/samaudio.h samaudio_op_resize_video / samaudio_vit_encode_video).

The statement is the reference's own: `(frames * mask.eq(0))[pick]`, materialised by torch and handed to the plain entry points
(samaudio_op_resize_frames / samaudio_vit_encode_frames, held to the float64 restatement by tests/test_vit_frames_gpu.py).  The masked
value 0 goes through the same taps in the same order with the same weights, so everything here is compared BIT FOR BIT - the one
exception is the 1700-pixel-wide case, which no small test pins for the plain kernel either and which is therefore also held to
tests/resize_ref.py directly, by the acceptance rule of tests/test_vit_frames_gpu.py.
"""
import ctypes as C
import functools
import os

import pytest
import torch

from sam_audio_amd import hip
from sam_audio_amd.config import PE_VISION_CONFIGS, PerceptionEncoderConfig
from sam_audio_amd.processor import MaskedVideo
from sam_audio_amd.synthetic import init_vision_state_dict
from sam_audio_amd.vision_encoder import PerceptionEncoder
from sam_audio_amd.vision_tower import PEVisionTower
from tests import resize_ref as R

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
# fp32, the plain 16-bit operands and the compensated mode; the CPU simulator carries the bfloat16 library only
PRECISIONS = ["fp32", "bf16", "bf16x3"] if SIM else ["fp32", "bf16", "fp16", "fp16x3"]

SRC = 7                     # source frames
PICK = [6, 0, 0, 3, 6]      # repeats, runs backwards, skips
# (H, W) -> S: an odd width (every row misaligned, a 1-channel mask row differently from its frame row); more source rows than one pass
# through LDS holds; wider than one column chunk of the kernel (768); the smallest frame; a target wider than 64 columns
CASES = [((45, 61), 56), ((431, 97), 56), ((5, 1700), 56), ((1, 3), 56), ((97, 131), 112)]
IDS = [f"{h}x{w}-{s}" for (h, w), s in CASES]


@functools.lru_cache(maxsize=None)
def video(H, W, mc):
    """(frames u8 [7,3,H,W], mask u8 [7,mc,H,W], materialised u8 [7,3,H,W]): computed once, shared, never modified.  The mask is a
    low-resolution random field, upsampled by nearest and thresholded so that about 40 % of the pixels are masked; its non-zero bytes
    are drawn from {1, 7, 255}, so code that tests `== 1` or `== 255` fails."""
    g = torch.Generator().manual_seed(H * 1000 + W + mc)
    frames = torch.randint(0, 256, (SRC, 3, H, W), generator=g, dtype=torch.uint8)
    hl, wl = (H + 7) // 8, (W + 7) // 8
    field = torch.rand(SRC, mc, hl, wl, generator=g)
    field = field[:, :, torch.arange(H) * hl // H][:, :, :, torch.arange(W) * wl // W]
    values = torch.tensor([1, 7, 255], dtype=torch.uint8)[torch.randint(0, 3, (SRC, mc, H, W), generator=g)]
    mask = torch.where(field < 0.4, values, torch.zeros((), dtype=torch.uint8))
    return frames, mask, frames * mask.eq(0)


def _resize(gpu, u8, S, mode):
    """samaudio_op_resize_frames -> planar f32 [n,3,S,S] on the CPU"""
    n, _, H, W = u8.shape
    x = u8.to(gpu).contiguous()
    out = torch.full((n, 3, S, S), float("nan"), device=gpu)
    hip.check(hip.lib().samaudio_op_resize_frames(hip.ptr(x), n, H, W, S, hip.RESIZE_MODES[mode], hip.ptr(out), hip.current_stream_ptr()))
    return out.cpu()


def _resize_video(gpu, frames, mask, pick, S, mode):
    """samaudio_op_resize_video -> planar f32 [n,3,S,S] on the CPU; `frames` / `mask`: CPU tensors or tensors already on the device"""
    src, _, H, W = frames.shape
    x = frames.to(gpu).contiguous()
    m = None if mask is None else mask.to(gpu).contiguous()
    m = m.view(torch.uint8) if m is not None and m.dtype == torch.bool else m
    p = None if pick is None else torch.tensor(pick, dtype=torch.int32).to(gpu)
    n = src if pick is None else len(pick)
    out = torch.full((n, 3, S, S), float("nan"), device=gpu)
    hip.check(hip.lib().samaudio_op_resize_video(hip.ptr(x), src, H, W, hip.ptr(m), 1 if m is None else m.shape[1], hip.ptr(p), n, S,
                                                 hip.RESIZE_MODES[mode], hip.ptr(out), hip.current_stream_ptr()))
    return out.cpu()


@pytest.mark.parametrize("mode", ["bicubic", "bilinear", "nearest"])
@pytest.mark.parametrize("mc", [1, 3])
@pytest.mark.parametrize("hw,S", CASES, ids=IDS)
def test_masked_picked_resize_is_bitwise_the_plain_resize_of_the_materialised_frames(gpu, hw, S, mc, mode):
    frames, mask, mat = video(hw[0], hw[1], mc)
    share = mask.ne(0).float().mean().item()
    print(f"{hw} mc {mc}: {share * 100:.1f} % of the pixels masked")
    want_all = _resize(gpu, mat, S, mode)
    plain_all = _resize(gpu, frames, S, mode)
    # mask and pick; (resizing is per frame, so the picked rows of the full result ARE the plain kernel's result on mat[pick] - which
    # the first assertion checks once instead of assuming)
    assert torch.equal(_resize(gpu, mat[PICK], S, mode), want_all[PICK])
    assert torch.equal(_resize_video(gpu, frames, mask, PICK, S, mode), want_all[PICK]), "mask + pick"
    assert torch.equal(_resize_video(gpu, frames, mask, None, S, mode), want_all), "mask, pick = NULL"
    assert torch.equal(_resize_video(gpu, frames, None, PICK, S, mode), plain_all[PICK]), "mask = NULL"
    assert torch.equal(_resize_video(gpu, frames, torch.zeros_like(mask), PICK, S, mode), plain_all[PICK]), "all-zero mask"
    full = torch.full_like(mask, 7)
    full[::2] = 255
    full[:, :, ::2, 1::2] = 1
    assert torch.equal(_resize_video(gpu, frames, full, PICK, S, mode), torch.full((len(PICK), 3, S, S), -1.0)), "all-non-zero mask"
    if mc == 1 and mode == "bicubic":   # bool storage (bytes 0 / 1) works unchanged
        assert torch.equal(_resize_video(gpu, frames, mask.ne(0), PICK, S, mode), want_all[PICK]), "bool mask"


def _check_levels(got, ref, delta, what):
    """The acceptance rule of tests/test_vit_frames_gpu.py, restated.  `got`: the kernel's normalised floats; `ref`: the float64
    reference, not rounded.  The kernel must choose the level clamp(rint(ref)) for every pixel, except where ref lies within delta of a
    half-integer: there fp32 cannot decide the rounding and one level of difference is allowed; such pixels may be at most 2 % (by the
    reference alone they are 0.16 - 0.22 % at 5 x 1700 on these inputs, so the cap cannot hide a failure)."""
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
@pytest.mark.parametrize("mc", [1, 3])
def test_the_wide_case_against_the_float64_restatement(gpu, mc, mode):
    """5 x 1700: three column chunks per row.  No small test holds the plain kernel to the reference at such a width, so the bitwise
    comparison above is not enough here: the masked, picked result against resize64 of the materialised frames."""
    frames, mask, mat = video(5, 1700, mc)
    picked = mat[PICK]
    ref = R.resize64(picked, 56, mode)
    dev = (R.torch_resize(picked, 56, mode).double() - ref).abs().max().item()
    delta = max(1e-3, 2.0 * dev)
    _check_levels(_resize_video(gpu, frames, mask, PICK, 56, mode), ref, delta, f"video 5x1700 {mode} mc {mc}")


@pytest.mark.parametrize("mc", [1, 3])
def test_unaligned_frame_and_mask_pointers_and_neighbouring_memory(gpu, mc):
    """Frames and mask at byte offsets 1, 7 and 13 inside larger 255-filled buffers, the two offsets varied independently: the mask
    piece is loaded by its own aligned address and shifted into the frame's byte positions, and neither the bytes in front of a tensor
    nor those behind it may leak in (255 is a non-zero mask byte and a bright pixel)."""
    frames, mask, mat = video(45, 61, mc)
    want = _resize_video(gpu, frames, mask, PICK, 56, "bicubic")
    assert torch.equal(want, _resize(gpu, mat[PICK], 56, "bicubic"))

    def shifted(t, shift):
        flat = torch.full((t.numel() + 64,), 255, dtype=torch.uint8)
        flat[shift: shift + t.numel()] = t.flatten()
        return flat.to(gpu)[shift: shift + t.numel()].view(t.shape)

    for fs in (1, 7, 13):
        x = shifted(frames, fs)
        for ms in (1, 7, 13):
            assert torch.equal(_resize_video(gpu, x, shifted(mask, ms), PICK, 56, "bicubic"), want), f"frames +{fs}, mask +{ms}"
        assert torch.equal(_resize_video(gpu, x, mask, PICK, 56, "bicubic"), want), f"frames +{fs}, mask aligned"


def _tower(precision, gpu, name="pe-tiny", seed=8):
    cfg = PE_VISION_CONFIGS[name]
    sd = init_vision_state_dict(cfg, seed=seed)
    tower = PEVisionTower(cfg, precision=precision, device=str(gpu))
    tower.load_state_dict(sd)
    return cfg, sd, tower


@pytest.mark.parametrize("precision", PRECISIONS)
def test_encode_frames_with_mask_and_index_equals_the_materialised_encode(gpu, precision):
    """5 picked frames of 7 at 80 x 64 on pe-tiny: the kernel's second form (the patch embedding's operand, in the tower's operand type)
    with the mask and the table, against the same form on the materialised frames - features and tokens bit for bit."""
    _, _, tower = _tower(precision, gpu)
    for mc in (1, 3):
        frames, mask, mat = video(80, 64, mc)
        want, want_tok = tower.encode_frames(mat[PICK].to(gpu), "bicubic", normalize=True, return_tokens=True)
        got, tok = tower.encode_frames(frames.to(gpu), "bicubic", normalize=True, return_tokens=True, masks=mask.to(gpu),
                                       index=torch.tensor(PICK))
        assert torch.isfinite(got).all()
        assert torch.equal(got, want) and torch.equal(tok, want_tok), f"{precision} mc {mc}"
    got = tower.encode_frames(frames.to(gpu), "bicubic", normalize=True, masks=mask.ne(0).to(gpu))      # bool mask, no index
    assert torch.equal(got, tower.encode_frames(mat.to(gpu), "bicubic", normalize=True))
    got = tower.encode_frames(frames.to(gpu), "nearest", index=[-1, 0])                                   # index alone
    assert torch.equal(got, tower.encode_frames(frames[[6, 0]].to(gpu), "nearest"))


@pytest.mark.skipif(SIM, reason="140 frames through the tower: MI355X only")
def test_the_two_stream_split_slices_the_pick_table(gpu):
    """From 64 frames on the tower encodes two halves on two streams: with a mask or a table the halves are slices of the TABLE (the
    identity table is made where none was given), both contexts read the one video."""
    _, _, tower = _tower("fp16", gpu)
    assert tower.streams == 2
    frames, mask, mat = video(80, 64, 3)
    index = torch.arange(70) * 5 % SRC
    want = tower.encode_frames(mat[index].to(gpu), "bicubic", normalize=True)
    assert torch.equal(tower.encode_frames(frames.to(gpu), "bicubic", normalize=True, masks=mask.to(gpu), index=index), want)
    many, many_mask = frames.repeat(10, 1, 1, 1), mask.repeat(10, 1, 1, 1)
    want = tower.encode_frames((many * many_mask.eq(0)).to(gpu), "bicubic", normalize=True)
    assert torch.equal(tower.encode_frames(many.to(gpu), "bicubic", normalize=True, masks=many_mask.to(gpu)), want)


def _encoder(gpu, sd, batch_size, **kw):
    pe = PE_VISION_CONFIGS["pe-tiny"]
    ecfg = PerceptionEncoderConfig(dim=pe.output_dim, batch_size=batch_size, name="pe-tiny", image_size=pe.image_size)
    enc = PerceptionEncoder(ecfg, device=gpu, precision="fp32", **kw)
    enc.load_state_dict({"model.visual." + k: v for k, v in sd.items()} | {"model.logit_scale": torch.ones(())}, strict=True)
    return enc


@pytest.mark.parametrize("batch_size", [2, 3])
def test_perception_encoder_encodes_every_distinct_frame_once(gpu, batch_size):
    pe = PE_VISION_CONFIGS["pe-tiny"]
    sd = init_vision_state_dict(pe, seed=8)
    frames, mask, mat = video(80, 64, 1)
    index = torch.tensor([5, 5, 1, 1, 1, 3, 6, 6, 0, 0, 0])       # 5 distinct of 7 source frames, 11 picked
    item = MaskedVideo(frames, mask, index)
    enc = _encoder(gpu, sd, batch_size, frame_transform="hip")
    # by hand: the distinct frames through encode_frames in the same chunks, gathered by the inverse
    uniq, inverse = index.unique(return_inverse=True)
    assert uniq.tolist() == [0, 1, 3, 5, 6]
    parts = [enc.tower.encode_frames(mat[uniq[i: i + batch_size]].to(gpu), "bicubic", normalize=enc.normalize_feature)
             for i in range(0, len(uniq), batch_size)]
    want = torch.cat(parts)[inverse.to(gpu)]
    seen = []
    inner = enc.tower.encode_frames

    def counting(frames_u8, *a, **kw):
        seen.append(frames_u8.shape[0] if kw.get("index") is None else len(kw["index"]))
        return inner(frames_u8, *a, **kw)

    enc.tower.encode_frames = counting
    out = enc([item])
    assert out.shape == (1, len(index), pe.output_dim)
    assert torch.equal(out[0], want)
    assert sum(seen) == len(uniq) and max(seen) <= batch_size, seen
    # a plain tensor beside it: time padding and the existing path are untouched
    both = enc([item, mat[:4]])
    assert torch.equal(both[0], want) and float(both[1, 4:].abs().max()) == 0.0
    assert torch.equal(both[1, :4], enc([mat[:4]])[0])
    # frame_transform="torch": the same object gives exactly what the materialised tensor gives today
    torch_enc = _encoder(gpu, sd, batch_size)
    assert torch.equal(torch_enc([item]), torch_enc([item.materialize()]))
    # ... and so does an injected tower without encode_frames, even under "hip"
    calls = []
    plain = PerceptionEncoder(enc.cfg, tower=lambda f, normalize: calls.append(tuple(f.shape)) or torch.zeros(f.shape[0], pe.output_dim),
                              frame_transform="hip")
    plain([item])
    assert sum(c[0] for c in calls) == len(index) and all(c[1:] == (3, pe.image_size, pe.image_size) for c in calls)


def test_separate_with_the_hip_video_transform(gpu):
    """SAMAudioProcessor(video_transform="hip") + mask_videos against the default processor's mask_videos, both on a model with
    frame_transform="hip": target and residual bit for bit.  The videos have exactly as many frames as the clips have latent steps,
    so the pick is the identity and no chunk of the tower changes size."""
    from sam_audio_amd import SAMAudio, SAMAudioProcessor, preset_config
    from sam_audio_amd.synthetic import init_state_dict, synthetic_clip, synthetic_noise, synthetic_text_features
    pe = PE_VISION_CONFIGS["pe-tiny"]
    cfg = preset_config("tiny")
    cfg.vision_encoder = PerceptionEncoderConfig(dim=pe.output_dim, batch_size=3, name="pe-tiny", image_size=pe.image_size)
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, 4 * hop) for i in range(2)]
    text, tmask = synthetic_text_features(2, 3)
    g = torch.Generator().manual_seed(12)
    videos = [torch.randint(0, 256, (4, 3, 70, 60), generator=g, dtype=torch.uint8),
              torch.randint(0, 256, (4, 3, 56, 56), generator=g, dtype=torch.uint8)]
    masks = [(torch.rand(4, 1, 70, 60, generator=g) < 0.4).to(torch.uint8) * 255, torch.rand(4, 3, 56, 56, generator=g) < 0.4]
    full = dict(init_state_dict(cfg, seed=3))
    full.update({"vision_encoder.model.visual." + k: v for k, v in init_vision_state_dict(pe, seed=6).items()})
    full["vision_encoder.model.logit_scale"] = torch.ones(())
    model = SAMAudio(cfg, precision="fp32", device=str(gpu), frame_transform="hip")
    model.load_state_dict(full, strict=True)
    results = []
    for transform in ("torch", "hip"):
        proc = SAMAudioProcessor.from_config(cfg, video_transform=transform)
        masked = proc.mask_videos(videos, masks)
        assert all(isinstance(v, MaskedVideo) == (transform == "hip") for v in masked)
        batch = proc(descriptions=["a", "b"], audios=clips, masked_videos=masked, text_features=text, text_mask=tmask)
        assert all(len(v) == 4 for v in batch.masked_video)
        res = model.separate(batch.to(gpu), noise=synthetic_noise(2, 4).to(gpu))
        assert all(torch.isfinite(w).all() for w in res.target + res.residual)
        results.append(res)
    for a, b in zip(results[0].target + results[0].residual, results[1].target + results[1].residual):
        assert torch.equal(a, b)


def test_video_entry_points_refuse_bad_arguments(gpu):
    frames = R.random_frames(2, 8, 8, seed=0).to(gpu)
    mask = torch.zeros(2, 1, 8, 8, dtype=torch.uint8).to(gpu)
    pick = torch.tensor([1, 0, 1], dtype=torch.int32).to(gpu)
    out = torch.empty(3, 3, 56, 56, device=gpu)
    lib, st = hip.lib(), hip.current_stream_ptr()
    null = C.c_void_p(0)
    good = dict(frames=hip.ptr(frames), src=2, height=8, width=8, mask=hip.ptr(mask), mc=1, pick=hip.ptr(pick), n=3, size=56,
                mode=hip.RESIZE_BICUBIC, out=hip.ptr(out))
    bad = (dict(frames=null), dict(out=null), dict(src=0), dict(n=0), dict(height=0), dict(width=0), dict(size=0), dict(mc=2),
           dict(mc=0), dict(mode=7), dict(mode=-1), dict(pick=null), dict(pick=null, n=1))      # (no table: n must be src_frames)

    def op(**kw):
        a = dict(good, **kw)
        return lib.samaudio_op_resize_video(a["frames"], a["src"], a["height"], a["width"], a["mask"], a["mc"], a["pick"], a["n"],
                                            a["size"], a["mode"], a["out"], st)

    hip.check(op())
    hip.check(op(mask=null, mc=0))          # without a mask mask_channels is ignored
    hip.check(op(pick=null, n=2))
    for kw in bad:
        assert op(**kw) == hip.ERR_ARG and b"resize_video" in lib.samaudio_last_error(), kw
    cfg, _, tower = _tower("fp32", gpu)
    feats = tower.encode_frames(frames, "bicubic", masks=mask, index=[1, 0, 1])       # sizes the workspace for three frames
    assert torch.isfinite(feats).all()

    def enc(**kw):
        a = dict(good, **{"out": hip.ptr(feats), **kw})
        return lib.samaudio_vit_encode_video(tower._h, a["frames"], a["src"], a["height"], a["width"], a["mask"], a["mc"], a["pick"],
                                             a["n"], a["mode"], 0, a["out"], None, st)

    hip.check(enc())
    for kw in bad:
        if "size" in kw:
            continue                        # (the tower's own image size)
        assert enc(**kw) == hip.ERR_ARG and b"vit_encode_video" in lib.samaudio_last_error(), kw
    # an index outside the video never reaches the device: IndexError from Python, before anything is launched
    for index in ([0, 2], [-3]):
        with pytest.raises(IndexError):
            tower.encode_frames(frames, "bicubic", index=index)
        with pytest.raises(IndexError):
            MaskedVideo(frames, None, torch.tensor(index))
    with pytest.raises(IndexError):
        MaskedVideo(frames).select(torch.tensor([2]))
    with pytest.raises(ValueError):
        tower.encode_frames(frames, "bicubic", masks=mask[:1])
    with pytest.raises(TypeError):
        tower.encode_frames(frames, "bicubic", masks=mask.float())
