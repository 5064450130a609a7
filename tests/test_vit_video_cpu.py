"""The CPU side of the masked, picked video path (tests/test_vit_video_gpu.py holds the kernel to the plain frame kernel on the GPU): the
C-ABI / Python wiring, the host semantics of `MaskedVideo`, the library's argument refusals, and the GPU tests on the SIMT simulator."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from sam_audio_amd import MaskedVideo, SAMAudioProcessor, hip, preset_config
from sam_audio_amd.processor import Batch, sample_video_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _video(T=6, H=9, W=7, mc=1, seed=0, boolean=False):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (T, 3, H, W), generator=g, dtype=torch.uint8)
    hit = torch.rand(T, mc, H, W, generator=g) < 0.4
    values = torch.tensor([1, 7, 255], dtype=torch.uint8)[torch.randint(0, 3, hit.shape, generator=g)]
    return frames, hit if boolean else hit * values


def test_header_and_python_wiring():
    header = open(os.path.join(ROOT, "include", "samaudio.h")).read()
    for name in ("samaudio_op_resize_video", "samaudio_vit_encode_video"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in hip.EXPORTED_SYMBOLS
        assert hasattr(hip.lib(), name)
    assert hip._PROTOS["samaudio_op_resize_video"][1][1] is C.c_int64 and hip._PROTOS["samaudio_vit_encode_video"][1][2] is C.c_int64
    cfg = preset_config("tiny")
    for make in (lambda **kw: SAMAudioProcessor(cfg.audio_codec.hop_length, cfg.audio_codec.sample_rate, **kw),
                 lambda **kw: SAMAudioProcessor.from_config(cfg, **kw)):
        assert make().video_transform == "torch" and make(video_transform="hip").video_transform == "hip"
        with pytest.raises(ValueError):
            make(video_transform="bogus")
    import inspect
    from sam_audio_amd.vision_tower import PEVisionTower
    assert "video_transform" in inspect.signature(SAMAudioProcessor.from_pretrained).parameters
    assert {"masks", "index"} <= set(inspect.signature(PEVisionTower.encode_frames).parameters)


def test_the_default_processor_is_unchanged():
    """video_transform="torch": mask_videos returns the product, __call__ gathers - plain tensors, equal to today's"""
    cfg = preset_config("tiny")
    proc = SAMAudioProcessor.from_config(cfg)
    frames, mask = _video(mc=3)
    masked = proc.mask_videos([frames], [mask])
    assert torch.is_tensor(masked[0]) and torch.equal(masked[0], frames * mask.eq(0))
    batch = proc(descriptions=["a"], audios=[torch.zeros(1, 9 * cfg.audio_codec.hop_length)], masked_videos=masked)
    idx = torch.linspace(0, 5, 9).round().long()
    assert torch.is_tensor(batch.masked_video[0]) and torch.equal(batch.masked_video[0], masked[0][idx])


@pytest.mark.parametrize("boolean", [False, True])
@pytest.mark.parametrize("mc", [1, 3])
def test_masked_video_host_semantics(mc, boolean):
    frames, mask = _video(mc=mc, boolean=boolean)
    assert mask.dtype == (torch.bool if boolean else torch.uint8)
    want = frames * mask.eq(0)
    video = MaskedVideo(frames, mask)
    assert len(video) == 6 and video.size(0) == 6 and tuple(video.size()) == (6, 3, 9, 7)
    assert torch.equal(video.materialize(), want)
    assert want.ne(frames).any() and want[mask.expand_as(frames).ne(0)].eq(0).all()
    index = torch.tensor([5, 0, 0, 3, 5, 2])
    picked = MaskedVideo(frames, mask, index)
    assert len(picked) == 6 and torch.equal(picked.materialize(), want[index])
    # an index composes with the one that is there, as indexing the materialised tensor twice would
    again = picked.select(torch.tensor([1, 1, 4, 3, -1]))
    assert len(again) == 5 and again.size(0) == 5 and again.index.tolist() == [0, 0, 5, 3, 2]
    assert torch.equal(again.materialize(), want[index][torch.tensor([1, 1, 4, 3, -1])])
    assert torch.equal(MaskedVideo(frames, None, index).materialize(), frames[index])
    assert torch.equal(MaskedVideo(frames).materialize(), frames)
    # .to("cpu") moves nothing and computes nothing
    moved = picked.to("cpu")
    assert isinstance(moved, MaskedVideo) and len(moved) == 6 and moved.index.device.type == "cpu"
    assert torch.equal(moved.frames, frames) and torch.equal(moved.mask, mask) and torch.equal(moved.index, index)
    assert moved.frames.dtype == torch.uint8 and moved.mask.dtype == mask.dtype
    for bad in ([6], [-7]):
        with pytest.raises(IndexError):
            MaskedVideo(frames, mask, torch.tensor(bad))
        with pytest.raises(IndexError):
            picked.select(torch.tensor(bad))
    with pytest.raises(TypeError):
        MaskedVideo(frames.float())
    with pytest.raises(TypeError):
        MaskedVideo(frames, mask.float())
    with pytest.raises(ValueError):
        MaskedVideo(frames, mask[:, :, :-1])


def test_the_hip_processor_describes_and_does_not_compute():
    cfg = preset_config("tiny")
    hop = cfg.audio_codec.hop_length
    proc = SAMAudioProcessor.from_config(cfg, video_transform="hip")
    default = SAMAudioProcessor.from_config(cfg)
    (f1, m1), (f2, m2) = _video(T=6, mc=1, seed=1), _video(T=4, mc=3, seed=2, boolean=True)
    floats = torch.rand(5, 3, 9, 7)
    masked = proc.mask_videos([f1, f2, floats], [m1, m2, m1[:5]])
    assert isinstance(masked[0], MaskedVideo) and masked[0].frames is f1 and masked[0].mask is m1 and masked[0].index is None
    assert isinstance(masked[1], MaskedVideo) and masked[1].mask is m2
    assert torch.is_tensor(masked[2]) and torch.equal(masked[2], floats * m1[:5].eq(0))         # any other dtype: today's product
    audios = [torch.zeros(1, 9 * hop), torch.zeros(1, 4 * hop), torch.zeros(1, 7 * hop)]
    batch = proc(descriptions=["a", "b", "c"], audios=audios, masked_videos=masked)
    want = default(descriptions=["a", "b", "c"], audios=audios, masked_videos=default.mask_videos([f1, f2, floats], [m1, m2, m1[:5]]))
    assert [len(v) for v in batch.masked_video] == [9, 4, 7]
    assert batch.masked_video[0].frames is f1 and batch.masked_video[0].index.tolist() == torch.linspace(0, 5, 9).round().long().tolist()
    assert batch.masked_video[1].index.tolist() == [0, 1, 2, 3]
    for got, ref in zip(batch.masked_video, want.masked_video):
        assert torch.equal(got.materialize() if isinstance(got, MaskedVideo) else got, ref)
    # a plain uint8 tensor is wrapped without a mask; an index that is already there composes
    batch = proc(descriptions=["a", "b"], audios=audios[:2], masked_videos=[f1, MaskedVideo(f2, m2, torch.tensor([3, 3, 0]))])
    assert isinstance(batch.masked_video[0], MaskedVideo) and batch.masked_video[0].mask is None
    assert torch.equal(batch.masked_video[0].materialize(), f1[torch.linspace(0, 5, 9).round().long()])
    assert batch.masked_video[1].index.tolist() == [3, 3, 3, 0]       # linspace(0, 2, 4).round() = [0, 1, 1, 2] of [3, 3, 0]
    moved = batch.to("cpu")
    assert isinstance(moved, Batch) and all(isinstance(v, MaskedVideo) for v in moved.masked_video)
    # sample_video_frames itself: tensors are gathered unless asked otherwise
    assert torch.is_tensor(sample_video_frames(torch.tensor([9]), [f1])[0])
    assert isinstance(sample_video_frames(torch.tensor([9]), [f1], lazy=True)[0], MaskedVideo)


def test_to_device_uploads_only_the_frames_a_sparse_index_uses():
    frames, mask = _video(T=6, mc=1, seed=3)
    sparse = MaskedVideo(frames, mask, torch.tensor([4, 1, 4]))
    moved = sparse.to("meta")
    assert moved.frames.shape[0] == 2 and moved.mask.shape[0] == 2 and moved.index.tolist() == [1, 0, 1]
    assert moved.index.device.type == "cpu" and moved.frames.dtype == torch.uint8
    dense = MaskedVideo(frames, mask, torch.tensor([0, 1, 2, 4])).to("meta")
    assert dense.frames.shape[0] == 6 and dense.index.tolist() == [0, 1, 2, 4]


def test_visual_ranker_gets_materialised_videos():
    from sam_audio_amd import SAMAudio
    model = SAMAudio(preset_config("tiny"), precision="fp32")
    frames, mask = _video()
    item = MaskedVideo(frames, mask, torch.tensor([2, 2, 0]))
    seen = []

    def ranker(extracted_audio, videos, sample_rate):
        seen.extend(videos)
        return torch.tensor([[0.0, 1.0]])

    model.visual_ranker = ranker

    class _B:
        masked_video = [item]
    assert model._rerank(_B(), [torch.zeros(2, 8)], [8], 2).tolist() == [1]
    assert torch.is_tensor(seen[0]) and torch.equal(seen[0], item.materialize())


def test_library_refuses_bad_video_arguments_without_a_gpu():
    """argument validation happens before any launch (and, for the tower's entry, before the context's state is looked at), so it is
    checked on the real library here"""
    lib = hip.lib()
    buf = (C.c_uint8 * 64)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)
    good = dict(frames=p, src=2, height=2, width=2, mask=p, mc=1, pick=p, n=3, size=56, mode=2, out=p)
    bad = (dict(frames=null), dict(out=null), dict(src=0), dict(n=0), dict(height=0), dict(width=0), dict(size=0), dict(mc=2),
           dict(mc=0), dict(mode=7), dict(pick=null), dict(pick=null, n=1))
    for kw in bad:
        a = dict(good, **kw)
        rc = lib.samaudio_op_resize_video(a["frames"], a["src"], a["height"], a["width"], a["mask"], a["mc"], a["pick"], a["n"],
                                          a["size"], a["mode"], a["out"], None)
        assert rc == hip.ERR_ARG and b"resize_video" in lib.samaudio_last_error(), kw
    vc = hip.VitConfig(precision=hip.precision_code("fp32"), image_size=56, patch_size=14, width=64, layers=1, heads=1, mlp_width=128,
                       output_dim=32, use_cls_token=1, use_rope2d=1, use_ln_pre=1, use_ln_post=1, pool_type=0, pool_heads=1, act=4,
                       ln_eps=1e-5)
    h = C.c_void_p()
    hip.check(lib.samaudio_vit_create(C.byref(vc), C.byref(h)))
    try:
        for kw in bad:
            if "size" in kw:
                continue
            a = dict(good, **kw)
            rc = lib.samaudio_vit_encode_video(h, a["frames"], a["src"], a["height"], a["width"], a["mask"], a["mc"], a["pick"],
                                               a["n"], a["mode"], 0, a["out"], None, None)
            assert rc == hip.ERR_ARG and b"vit_encode_video" in lib.samaudio_last_error(), kw
        # good arguments on a context without weights: refused by its state, still before any launch
        a = good
        assert lib.samaudio_vit_encode_video(h, a["frames"], a["src"], a["height"], a["width"], a["mask"], a["mc"], a["pick"], a["n"],
                                             a["mode"], 0, a["out"], None, None) == hip.ERR_STATE
        assert lib.samaudio_vit_encode_video(None, p, 2, 2, 2, p, 1, p, 3, 2, 0, p, None, None) == hip.ERR_ARG
    finally:
        lib.samaudio_vit_destroy(h)


def test_video_kernel_on_the_simulator():
    """tests/test_vit_video_gpu.py on the SIMT simulator (the real kernel code compiled for the host, as tests/test_simt_cpu.py runs its
    selections): every bitwise case incl. the ones that need several passes through LDS and several column chunks, the unaligned frame
    and mask pointers, the fused im2col layout in fp32 / bf16 / bf16x3, the PerceptionEncoder path and the error returns.
    (separate() runs on the GPU only: the codec makes it slow here, and it adds no kernel of this file.)"""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_vit_video_gpu.py", "-k", "not separate"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail
