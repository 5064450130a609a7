"""The CPU side of the uint8 frame path (tests/test_vit_frames_gpu.py holds the kernel to tests/resize_ref.py on the GPU):
the float64 restatement against torch's own kernels, the C-ABI / Python wiring, and the GPU tests on the SIMT simulator."""
import os
import re
import subprocess
import sys

import pytest
import torch

from sam_audio_amd import hip
from tests import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind,hw,S", [("random", hw, S) for hw, S in R.CASES] + [("checkerboard", (45, 61), 56)])
def test_float64_restatement_matches_torch(kind, hw, S):
    """The yardstick of the GPU test: its deviation from F.interpolate(antialias=True) on the CPU is torch's fp32 noise (< 1e-2 of a
    level; measured 2e-5 .. 3e-3), for down-scaling, up-scaling, mixed cases and a single source row; nearest is exactly equal."""
    for mode in ("bicubic", "bilinear"):
        u8, ref, delta, dev = R.case(hw[0], hw[1], S, mode, kind)
        assert ref.shape == (3, 3, S, S) and ref.dtype == torch.float64
        assert dev < 1e-2 and delta == max(1e-3, 2 * dev), f"{mode} {hw} -> {S}: {dev:.2e}"
        near = ((ref - ref.floor()) - 0.5).abs() <= delta
        assert near.float().mean().item() <= 0.02      # the share of pixels whose rounding fp32 cannot decide, by the reference alone
    u8 = R.case(hw[0], hw[1], S, "nearest", kind)[0]
    assert torch.equal(R.resize64(u8, S, "nearest").float(), R.torch_resize(u8, S, "nearest"))


def test_identity_and_normalisation_of_the_restatement():
    u8 = R.random_frames(2, 56, 56, seed=1)
    for mode in R.MODES:
        assert torch.equal(R.resize64(u8, 56, mode), u8.double())
    lv = torch.arange(256)
    assert torch.equal(R.normalise(lv), (lv.to(torch.uint8).float() / 255.0 - 0.5) / 0.5)
    assert torch.equal(R.levels(torch.tensor([-3.2, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0], dtype=torch.float64)),
                       torch.tensor([0.0, 0.0, 2.0, 2.0, 254.0, 255.0, 255.0], dtype=torch.float64))
    board = R.case(45, 61, 56, "bicubic", "checkerboard")[1]
    assert ((board < -0.5) | (board > 255.5)).float().mean().item() > 0.2    # the clamp has work to do


def test_header_and_python_wiring():
    header = open(os.path.join(ROOT, "include", "samaudio.h")).read()
    for name in ("samaudio_op_resize_frames", "samaudio_vit_encode_frames"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in hip.EXPORTED_SYMBOLS
    for name, code in (("NEAREST", 0), ("BILINEAR", 1), ("BICUBIC", 2)):
        assert re.search(r"#define\s+SAMAUDIO_RESIZE_%s\s+%d\b" % (name, code), header)
        assert hip.RESIZE_MODES[name.lower()] == code
    from sam_audio_amd import SAMAudio, preset_config
    from sam_audio_amd.vision_encoder import PerceptionEncoder
    from sam_audio_amd.vision_tower import PEVisionTower
    assert hasattr(PEVisionTower, "encode_frames")
    tower = lambda frames, normalize: torch.zeros(frames.shape[0], 4)   # noqa: E731
    assert PerceptionEncoder(tower=tower).frame_transform == "torch"
    assert PerceptionEncoder(tower=tower, frame_transform="hip").frame_transform == "hip"
    with pytest.raises(ValueError):
        PerceptionEncoder(tower=tower, frame_transform="bogus")
    with pytest.raises(ValueError):
        SAMAudio(preset_config("tiny"), precision="fp32", frame_transform="bogus")
    assert SAMAudio(preset_config("tiny"), precision="fp32").frame_transform is None


def test_library_refuses_bad_resize_arguments_without_a_gpu():
    """argument validation happens before any launch, so it is checked on the real library here"""
    import ctypes as C
    lib = hip.lib()
    buf = (C.c_uint8 * 16)()
    p = C.cast(buf, C.c_void_p)
    for frames, n, h, mode in ((C.c_void_p(0), 1, 2, 2), (p, 0, 2, 2), (p, 1, 0, 2), (p, 1, 2, 7)):
        assert lib.samaudio_op_resize_frames(frames, n, h, 2, 56, mode, p, None) == hip.ERR_ARG
        assert b"resize_frames" in lib.samaudio_last_error()


def test_frame_kernel_on_the_simulator():
    """tests/test_vit_frames_gpu.py on the SIMT simulator (the real kernel code compiled for the host, as tests/test_simt_cpu.py runs
    its selections): every resize case incl. the ones that need several passes through LDS, the unaligned frame pointers, the fused
    im2col layout in fp32 / bf16 / bf16x3, the PerceptionEncoder path and the error returns.  (separate() runs on the GPU only: the
    codec makes it slow here, and it adds no kernel of this file.)"""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_vit_frames_gpu.py", "-k", "not separate"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail
