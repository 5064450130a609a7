"""The DAC-VAE workspace plan (engine.hip plan_codec / codec_chunk) on the CPU emulation of tests/test_emu_cpu.py: what
samaudio_workspace_bytes asks for, how many waveforms a workspace of a given size holds per pass, and that a pass stays inside the bytes
it was handed.

The sizes are the linear model 64 KiB + n * per_item; the numbers pinned here were measured on the emulation build of the commit
before the codec got its one plan (per_item = 8 340 992 bytes for one 1920-sample frame in fp32).  Passes are observed from outside: the
profiled launches of a call are a whole multiple of those of a call that runs as one pass.  Every call runs in a workspace of exactly
the bytes asked for, inside a buffer of 0xFF bytes: a pass that carved past its plan would leave its mark behind it.
"""
import ctypes as C

import pytest
import torch

from sam_audio_amd import hip, preset_config
from sam_audio_amd.synthetic import init_state_dict
from sam_audio_amd.weights import convert_codec, convert_codec_fly16, convert_codec_x3
from tests.test_emu_cpu import _check, _engine, _set, emu  # noqa: F401  (emu: the session fixture that builds / loads the library)

FIXED, PER_ITEM_FP32 = 65536, 8340992
MODES = ["fp32", "fp32+x3codec", "bf16"]
GUARD = 1 << 20


class _Codec:
    """one engine context with the codec weights of `mode`, one frame per waveform"""

    def __init__(self, lib, mode):
        self.lib, self.cfg, self.keep = lib, preset_config("tiny"), []
        bf16 = mode == "bf16"
        self.ctx = _engine(lib, self.cfg, hip.BF16 if bf16 else hip.F32, self.keep)
        sd = init_state_dict(self.cfg, seed=3)
        codec = convert_codec(sd, self.cfg, torch.bfloat16 if bf16 else torch.float32, "cpu")
        tensors = dict(codec)
        if mode == "fp32+x3codec":   # the twins SAMAudio.load_state_dict registers for an x3 precision (model.py)
            _check(lib, lib.samaudio_set_option(self.ctx, hip.OPT_X3_CLASSES, hip.CLS["codec"]))
            tensors.update(convert_codec_x3(codec, torch.bfloat16))
            tensors.update(convert_codec_fly16(codec, torch.bfloat16))
        _set(lib, lib.samaudio_set_tensor, self.ctx, tensors, self.keep)
        _check(lib, lib.samaudio_finalize(self.ctx, 1))
        self.S = self.cfg.audio_codec.hop_length
        self.CD = self.cfg.audio_codec.codebook_dim

    def need(self, n):
        return self.lib.samaudio_workspace_bytes(self.ctx, 0, 0, 0, n, self.S)

    def run(self, what, items, nbytes, again=False):
        """encode | decode | pairs over the first `items` waveforms of a fixed set, in a workspace of exactly `nbytes` inside a buffer of
        0xFF bytes (`again`: in the previous call's workspace as that call left it): (return code, profiled launches, result).
        Asserts that the bytes around the workspace are untouched."""
        lib, g = self.lib, torch.Generator().manual_seed(1)
        if not again:
            self.buf = torch.full((nbytes + 256 + GUARD,), 255, dtype=torch.uint8)
        buf = self.buf
        off = (buf.data_ptr() + 255) // 256 * 256 - buf.data_ptr()
        _check(lib, lib.samaudio_set_workspace(self.ctx, C.c_void_p(buf.data_ptr() + off), nbytes))
        _check(lib, lib.samaudio_profile_begin(self.ctx))
        if what == "encode":
            src, out = (0.1 * torch.randn(8, self.S, generator=g))[:items].clone(), torch.full((items, 1, self.CD), float("nan"))
            rc = lib.samaudio_codec_encode(self.ctx, hip.ptr(src), items, self.S, hip.ptr(out), None)
        elif what == "decode":
            src, out = torch.randn(8, 1, self.CD, generator=g)[:items].clone(), torch.full((items, self.S), float("nan"))
            rc = lib.samaudio_codec_decode(self.ctx, hip.ptr(src), items, 1, hip.ptr(out), None)
        else:   # the ODE state layout: row b = (target | residual) of waveforms 2b, 2b + 1
            src, out = torch.randn(4, 1, 2 * self.CD, generator=g)[:items // 2].clone(), torch.full((items, self.S), float("nan"))
            rc = lib.samaudio_codec_decode_pairs(self.ctx, hip.ptr(src), items // 2, 1, hip.ptr(out), None)
        st, n = (hip.KernelStat * 64)(), C.c_int()
        _check(lib, lib.samaudio_profile_end(self.ctx, st, 64, C.byref(n)))
        bad = (buf[off + nbytes:] != 255).nonzero()
        assert bad.numel() == 0, f"{what} of {items} wrote {bad.numel()} bytes behind its {nbytes}-byte workspace (first at +{int(bad[0])})"
        assert (buf[:off] == 255).all()
        if rc == 0:
            assert torch.isfinite(out).all(), f"{what} of {items}: the result holds values nobody computed"
        return rc, sum(st[i].launches for i in range(n.value)), out


_CODECS = {}


@pytest.fixture
def codec(emu, request):  # noqa: F811
    mode = request.param
    if mode not in _CODECS:
        _CODECS[mode] = _Codec(emu, mode)
    return _CODECS[mode]


@pytest.mark.parametrize("codec", ["fp32"], indirect=True)
def test_workspace_bytes_are_the_pinned_linear_model(codec):
    assert codec.need(1) == 8406528 == FIXED + PER_ITEM_FP32
    for n in (2, 3, 5):
        assert codec.need(n) == FIXED + n * PER_ITEM_FP32
    assert codec.need(0) == 0


@pytest.mark.parametrize("codec", MODES, indirect=True)
def test_workspace_bytes_are_linear_in_the_items(codec):
    per_item = codec.need(1) - FIXED
    print(f"codec workspace per item: {per_item} bytes")
    assert per_item > 0
    for n in (2, 3, 5, 16, 64):
        assert codec.need(n) == FIXED + n * per_item


@pytest.mark.parametrize("codec", ["fp32"], indirect=True)
def test_decode_runs_capacity_items_per_pass(codec):
    """items waveforms in a workspace sized for `capacity` of them: ceil(items / capacity) passes, each the launches of a single pass"""
    rc, one, _ = codec.run("decode", 1, codec.need(1))
    assert rc == 0 and one > 0
    for items, cap, passes in ((2, 2, 1), (3, 3, 1), (5, 5, 1), (3, 2, 2), (5, 2, 3), (5, 4, 2)):
        rc, launches, _ = codec.run("decode", items, codec.need(cap))
        assert rc == 0, codec.lib.samaudio_last_error().decode()
        assert launches == passes * one, (items, cap, launches, one)
    rc, launches, _ = codec.run("decode", 3, codec.need(3) - 1)   # one byte short of three items: two per pass
    assert rc == 0 and launches == 2 * one


@pytest.mark.parametrize("codec", MODES, indirect=True)
def test_passes_stay_inside_the_workspace_they_were_handed(codec):
    """encode, decode and decode of (target, residual) pairs over more than one pass, in exactly the bytes asked for (run() asserts the
    guard); a pass of pairs holds whole pairs - capacity 3 runs 2 + 2 - and a workspace for one item cannot hold a pair."""
    for what in ("encode", "decode"):
        rc, one, full = codec.run(what, 1, codec.need(1))
        assert rc == 0, codec.lib.samaudio_last_error().decode()
        rc, launches, part = codec.run(what, 3, codec.need(2))
        assert rc == 0 and launches == 2 * one
        assert torch.equal(part[:1], full)   # (item 0 is the same waveform: the size of its pass does not change its result)
    rc, one, first = codec.run("pairs", 2, codec.need(2))
    assert rc == 0
    for cap in (2, 3):
        rc, launches, out = codec.run("pairs", 4, codec.need(cap))
        assert rc == 0 and launches == 2 * one, (cap, launches, one)
        assert torch.equal(out[:2], first)
    rc, launches, _ = codec.run("pairs", 4, codec.need(1))
    assert rc == hip.ERR_WORKSPACE and launches == 0
    rc, launches, _ = codec.run("decode", 1, codec.need(1) - 1)
    assert rc == hip.ERR_WORKSPACE and launches == 0


@pytest.mark.parametrize("codec", MODES, indirect=True)
def test_a_second_call_in_the_same_workspace_is_bitwise_equal(codec):
    for what, items in (("encode", 1), ("decode", 1), ("pairs", 2)):
        first = codec.run(what, items, codec.need(items))
        again = codec.run(what, items, codec.need(items), again=True)
        assert first[0] == 0 and first[:2] == again[:2] and torch.equal(first[2], again[2])
