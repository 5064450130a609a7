"""separate(seed=...) without a GPU: the float64 statement of tests/noise_ref.py against Random123's known
answers and its own statistics, the wiring of samaudio_op_noise through header, binding and kernels, the launcher emulation's refusal,
clip ids through the processor and dist.shard_batch, the argument errors, and the light cases of tests/test_noise_gpu.py on the SIMT
simulator (noise_rows_kernel's real code)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sam_audio_amd import SAMAudio, SAMAudioProcessor, hip, preset_config
from sam_audio_amd.dist import shard_batch
from sam_audio_amd.noise import seeded_noise
from sam_audio_amd.synthetic import synthetic_clip, synthetic_text_features
from tests import noise_ref as R
from tests.test_emu_cpu import emu  # noqa: F401  (fixture: the launcher emulation library, built on demand)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    assert " ".join("%08x" % int(w) for w in R.philox4x32_10(counter, key)) == want


def test_counter_layout_of_a_stream():
    """value (t, c) of a stream = word c % 4 of the call with counter (t * Q + c // 4, candidate, id lo, id hi), key (seed lo, hi)"""
    seed, cid, cand, t, c, channels = 2 ** 40 + 5, 2 ** 33 + 2, 3, 6, 9, 12
    z = R.stream(seed, cid, cand, 8, channels)
    x = [int(w) for w in R.philox4x32_10((t * 3 + 2, cand, cid & 0xFFFFFFFF, cid >> 32), (seed & 0xFFFFFFFF, seed >> 32))]
    ua, ub = ((x[0] >> 8) + 1) * 2.0 ** -24, (x[1] >> 8) * 2.0 ** -24
    assert abs(z[t, c] - np.sqrt(-2 * np.log(ua)) * np.sin(2 * np.pi * ub)) < 1e-14 and c % 4 == 1
    assert np.array_equal(z[2:], R.stream(seed, cid, cand, 6, channels, frame0=2)), "frame-major: frames do not know the frame count"
    assert np.array_equal(R.noise(seed, [7, cid], 4, 8, channels)[4 + cand], z), "row b * candidates + c"


def test_statistics_of_the_statement():
    """seed 1234, clip 0, candidate 0, 4096 x 256 (n = 2^20): the 5-sigma conditions (noise_ref.check_statistics), and what float32
    arithmetic costs against float64 on that set - the e32 of the GPU test's bound"""
    z = R.stream(1234, 0, 0, 4096, 256)
    fig = R.check_statistics(z, {"clip": R.stream(1234, 1, 0, 4096, 256), "candidate": R.stream(1234, 0, 1, 4096, 256),
                                 "seed": R.stream(1235, 0, 0, 4096, 256)})
    print({k: f"{float(v):.3e}" for k, v in fig.items()})
    assert len(fig) == 9 and z.size == 2 ** 20
    e32 = np.abs(R.stream(1234, 0, 0, 4096, 256, dtype=np.float32).astype(np.float64) - z).max()
    print(f"e32 = {e32:.3e}")
    assert 0 < 4 * e32 < 1e-5
    edge = R._pair(np.array([0xFFFFFFFF, 0], dtype=np.uint32), np.array([0, 0], dtype=np.uint32), np.float64)[0]
    assert edge[0] == 0.0 and abs(edge[1] - R.Z_MAX) < 1e-12, "u_a = 1 gives r = 0, u_a = 2^-24 the largest |z|"


# ------------------------------------------------------------------------------------------------ wiring
def test_header_binding_and_kernels_agree():
    header = open(os.path.join(ROOT, "include", "samaudio.h")).read()
    assert re.search(r"\bsamaudio_op_noise\s*\(float\* out, int clips, int candidates, int frames, int channels,\s*uint64_t seed, "
                     r"const int64_t\* clip_ids_host,\s*samaudio_stream stream\);", header)
    assert "samaudio_op_noise" in hip.EXPORTED_SYMBOLS
    res, args = hip._PROTOS["samaudio_op_noise"]
    assert res is C.c_int and args[5] is C.c_uint64 and len(args) == 8
    assert "tests/noise_ref.py" in header and "unpinned vs torch's" in header and "Random123" in header
    kernels_h = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "kernels.h")).read()
    assert re.search(r"__attribute__\(\(weak\)\)\s+hipError_t\s+launch_noise_rows\(", kernels_h)
    pack = re.search(r"struct NoiseClipPack \{\s*static constexpr int N = (\d+);", kernels_h)
    cap = re.search(r"constexpr int kNoiseGridCap = (\d+);", kernels_h)
    assert (int(pack.group(1)), int(cap.group(1))) == (hip.NOISE_PACK_CLIPS, hip.NOISE_GRID_CAP)
    kernels = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "kernels.hip")).read()
    assert re.search(r"__global__[^;{]*\bnoise_rows_kernel\(", kernels)
    for const in ("0xD2511F53u", "0xCD9E8D57u", "0x9E3779B9u", "0xBB67AE85u"):
        assert const in kernels
    api = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "api.hip")).read()
    assert "if (!sa::launch_noise_rows)" in api
    with pytest.raises(hip.SamAudioHipError, match="no CPU fallback"):
        seeded_noise(1, [0], 1, 2, 8, "cpu")


def _call(lib, out, clips=2, cand=2, frames=4, channels=8, seed=1, ids=(3, 4)):
    arr = None if ids is None else (C.c_int64 * len(ids))(*ids)
    return lib.samaudio_op_noise(out, clips, cand, frames, channels, seed, arr, None)


def test_emulated_build_binds_and_refuses_the_op(emu):
    """oracle/emu has no launch_noise_rows: the library still binds every entry point (the emu fixture) and the hook, after its
    argument checks, answers SAMAUDIO_ERR_STATE with the output untouched"""
    out = torch.full((128,), 7.0)
    assert _call(emu, hip.ptr(out)) == hip.ERR_STATE
    assert "not available in this build" in emu.samaudio_last_error().decode()
    assert _call(emu, hip.ptr(out), channels=6) == hip.ERR_ARG
    assert bool((out == 7).all())


def test_library_refuses_bad_arguments_without_a_gpu():
    """argument validation happens before any launch, so it is checked on the real library here"""
    lib = hip.lib()
    out = torch.full((132,), 7.0)
    p, odd = hip.ptr(out), C.c_void_p(out.data_ptr() + 4)
    assert out.data_ptr() % 16 == 0
    for kw, why in ((dict(out=None), "null"), (dict(ids=None), "null"), (dict(out=odd), "aligned"), (dict(clips=0), "< 1"),
                    (dict(cand=0), "< 1"), (dict(frames=0), "< 1"), (dict(clips=-1), "< 1"), (dict(channels=6), "channels"),
                    (dict(channels=0), "channels"), (dict(frames=2 ** 31 - 1, channels=12), r"2\^32"),
                    (dict(ids=(3, -1)), "negative"), (dict(ids=(-2 ** 63, 0)), "negative")):
        args = dict(out=p)
        args.update(kw)
        assert _call(lib, **args) == hip.ERR_ARG, kw
        assert re.search(why, lib.samaudio_last_error().decode()), (kw, lib.samaudio_last_error().decode())
    assert bool((out == 7).all())


# ------------------------------------------------------------------------------------------------ clip ids
FRAMES = (8, 5, 3, 6, 2)


def _batch(cfg, clip_ids=None):
    hop = cfg.audio_codec.hop_length
    clips = [synthetic_clip(i, n * hop if n == max(FRAMES) else (n - 1) * hop + 100) for i, n in enumerate(FRAMES)]
    text, tmask = synthetic_text_features(len(FRAMES), 5, ragged=True)
    return SAMAudioProcessor.from_config(cfg)(descriptions=[f"clip {i}" for i in range(len(FRAMES))], audios=clips, text_features=text,
                                              text_mask=tmask, clip_ids=clip_ids)


@pytest.mark.parametrize("ids", [None, [2 ** 32 + 7, 3, 0, 2 ** 63 - 1, 12]], ids=["rows", "clip_ids"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_shard_batch_carries_clip_ids(world, ids):
    cfg = preset_config("tiny")
    batch = _batch(cfg, ids)
    assert batch.clip_ids == ids and batch.to("cpu").clip_ids == ids and batch.sizes_host == list(FRAMES)
    got = []
    for rank in range(world):
        shard = shard_batch(batch, rank, world)
        assert len(shard.clip_ids) == len(shard.descriptions) == shard.audios.size(0)
        assert all(isinstance(v, int) for v in shard.clip_ids)
        rows = [int(d.split()[1]) for d in shard.descriptions]
        assert shard.clip_ids == [rows[i] if ids is None else ids[r] for i, r in enumerate(rows)]
        assert shard.to("cpu").clip_ids == shard.clip_ids
        again = shard_batch(shard, 0, 1)   # a shard of a shard keeps the ids of the whole batch
        assert again.clip_ids == shard.clip_ids
        got += shard.clip_ids
    assert got == (list(range(len(FRAMES))) if ids is None else ids)
    assert batch.clip_ids == ids, "the whole batch is left as it was"


def test_processor_refuses_bad_clip_ids():
    cfg = preset_config("tiny")
    for bad, why in (([1, 2, 3, 4, 1], "distinct"), ([0, 1, 2, 3, -4], r"\[0, 2\*\*63\)"), ([0, 1, 2, 3, 2 ** 63], r"\[0, 2\*\*63\)"),
                     ([0, 1, 2], "3 ids for 5 clips"), ([0, 1, 2, 3, 4.5], "integers"), ([0, 1, 2, 3, True], "integers")):
        with pytest.raises(ValueError, match=why):
            _batch(cfg, bad)


def test_separate_argument_errors():
    """seed together with noise, a seed outside [0, 2^64): ValueError before anything runs (no weights, no GPU needed to get there)"""
    model = SAMAudio(preset_config("tiny"), precision="fp32", device="cpu")
    batch = _batch(preset_config("tiny"))
    with pytest.raises(ValueError, match="mutually exclusive"):
        model.separate(batch, noise=torch.zeros(5, 8, 256), seed=3)
    for bad in (-1, 2 ** 64, 1.0, "7", True):
        with pytest.raises(ValueError, match="seed must be"):
            model.separate(batch, seed=bad)
    with pytest.raises(RuntimeError, match="load_state_dict"):   # a good seed gets as far as a call without one
        model.separate(batch, seed=2 ** 64 - 1)
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(clip_ids=[-1]), dict(clip_ids=[2 ** 63])):
        args = dict(seed=1, clip_ids=[0], candidates=1, frames=2, channels=8, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError):   # before the device is even looked at
            seeded_noise(**args)


# ------------------------------------------------------------------------------------------------ the kernel on the simulator
def test_light_noise_cases_on_the_simulator():
    """tests/test_noise_gpu.py's light cases with every product source on the SIMT simulator (conftest.py, SAMAUDIO_EMU_DRYRUN=simt):
    noise_rows_kernel against the float64 statement over every shape, id and seed, the second argument pack, the bitwise properties,
    the view inside a NaN buffer and the refusals."""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "tests/test_noise_gpu.py", "-k", "light"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    out = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, out
    assert "10 passed" in out and "failed" not in out
