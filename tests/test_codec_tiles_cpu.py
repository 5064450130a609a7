"""The time-tiled DAC-VAE calls (engine.hip codec_encode_tiled / codec_decode_tiled) on the CPU emulation of
tests/test_emu_cpu.py, with the codec contexts of tests/test_codec_plan_cpu.py: the reach the library derives against its restatement
(tests/codec_tiles_ref.py), the tile plan, that a tiled call equals the whole call bit for bit inside a workspace of exactly the bytes
asked for ONE SEGMENT, how many launches it issues, and what it refuses.

Every call runs in its workspace inside a buffer of 0xFF bytes, as in test_codec_plan_cpu.py: a pass that carved past the segment's
plan - or a tile that wrote outside its own rows of the NaN-filled destination - would leave its mark."""
import ctypes as C

import pytest
import torch

from sam_audio_amd import hip
from tests import codec_tiles_ref as R
from tests.test_codec_plan_cpu import GUARD, _Codec
from tests.test_emu_cpu import _check, emu  # noqa: F401  (emu: the session fixture that builds / loads the library)

_CODECS = {}


@pytest.fixture
def codec(emu, request):  # noqa: F811
    mode = request.param
    if mode not in _CODECS:
        _CODECS[mode] = _Codec(emu, mode)
    return _CODECS[mode]


def _halo(codec, decode):
    return codec.lib.samaudio_codec_halo_frames(codec.ctx, int(decode))


def _need(codec, n, T, L, decode):
    """the bytes of a workspace for passes of n items over the longest segment of (T, L)"""
    seg = codec.lib.samaudio_codec_tile_samples(codec.ctx, T, L, int(decode))
    return codec.lib.samaudio_workspace_bytes(codec.ctx, 0, 0, 0, n, seg)


def _run(codec, what, items, T, L, nbytes):
    """encode | decode | pairs of `items` fixed waveforms of T frames, in tiles of L frames (None: the untiled call), in a workspace of
    exactly `nbytes` inside 0xFF bytes: (return code, profiled launches, result)"""
    lib, g, hop, CD = codec.lib, torch.Generator().manual_seed(T), codec.S, codec.CD
    buf = torch.full((nbytes + 256 + GUARD,), 255, dtype=torch.uint8)
    off = (buf.data_ptr() + 255) // 256 * 256 - buf.data_ptr()
    _check(lib, lib.samaudio_set_workspace(codec.ctx, C.c_void_p(buf.data_ptr() + off), nbytes))
    _check(lib, lib.samaudio_profile_begin(codec.ctx))
    if what == "encode":
        src, out = 0.1 * torch.randn(items, T * hop, generator=g), torch.full((items, T, CD), float("nan"))
        rc = (lib.samaudio_codec_encode(codec.ctx, hip.ptr(src), items, T * hop, hip.ptr(out), None) if L is None else
              lib.samaudio_codec_encode_tiled(codec.ctx, hip.ptr(src), items, T * hop, L, hip.ptr(out), None))
    elif what == "decode":
        src, out = torch.randn(items, T, CD, generator=g), torch.full((items, T * hop), float("nan"))
        rc = (lib.samaudio_codec_decode(codec.ctx, hip.ptr(src), items, T, hip.ptr(out), None) if L is None else
              lib.samaudio_codec_decode_tiled(codec.ctx, hip.ptr(src), items, T, L, hip.ptr(out), None))
    else:   # the ODE state layout: row b = (target | residual) of waveforms 2b, 2b + 1
        src, out = torch.randn(items // 2, T, 2 * CD, generator=g), torch.full((items, T * hop), float("nan"))
        rc = (lib.samaudio_codec_decode_pairs(codec.ctx, hip.ptr(src), items // 2, T, hip.ptr(out), None) if L is None else
              lib.samaudio_codec_decode_pairs_tiled(codec.ctx, hip.ptr(src), items // 2, T, L, hip.ptr(out), None))
    st, n = (hip.KernelStat * 64)(), C.c_int()
    _check(lib, lib.samaudio_profile_end(codec.ctx, st, 64, C.byref(n)))
    bad = (buf[off + nbytes:] != 255).nonzero()
    assert bad.numel() == 0, f"{what} T={T} L={L} wrote {bad.numel()} bytes behind its {nbytes}-byte workspace (first at +{int(bad[0])})"
    assert (buf[:off] == 255).all()
    if rc == 0:
        assert torch.isfinite(out).all(), f"{what} T={T} L={L}: the result holds values nobody computed"
    return rc, sum(st[i].launches for i in range(n.value)), out


@pytest.mark.parametrize("codec", ["fp32"], indirect=True)
def test_halo_frames_equal_the_restatement(codec):
    a = codec.cfg.audio_codec
    for decode in (False, True):
        lo, hi, per = R.reach_rows(a.encoder_rates, a.decoder_rates, decode)
        h = _halo(codec, decode)
        print(f"{'decode' if decode else 'encode'}: reach {lo} rows before, {hi} behind, {per} rows per frame -> halo {h} frames")
        assert h == R.halo_frames(a.encoder_rates, a.decoder_rates, decode) and h >= 1
    assert codec.lib.samaudio_codec_halo_frames(None, 0) < 0


@pytest.mark.parametrize("h", [0, 1, 6, 8])
def test_tile_plan_partitions_the_clip(h):
    for T in range(1, 41):
        for L in range(1, 43):
            plan = R.tile_plan(T, L, h)
            assert plan[0].keep0 == 0 and plan[-1].keep1 == T
            for k, t in enumerate(plan):
                assert t.keep0 < t.keep1 and (k == 0 or plan[k - 1].keep1 == t.keep0)       # the kept ranges partition [0, T)
                assert 0 <= t.seg0 <= t.keep0 and t.keep1 <= t.seg1 <= T                    # a segment lies inside the clip ...
                assert t.seg0 == t.keep0 - h or (t.seg0 == 0 and t.keep0 < h)               # ... with h frames either side where
                assert t.seg1 == t.keep1 + h or (t.seg1 == T and T - t.keep1 < h)           # the clip has that much
                assert t.keep1 - t.keep0 == L or k == len(plan) - 1


@pytest.mark.parametrize("codec", ["fp32"], indirect=True)
def test_tile_samples_are_the_longest_segment(codec):
    for decode in (False, True):
        h = _halo(codec, decode)
        for T in range(1, 41):
            for L in (1, 2, 3, 5, h, h + 1, 2 * h + 1, 17, 40, 41):
                got = codec.lib.samaudio_codec_tile_samples(codec.ctx, T, L, int(decode))
                assert got == R.longest_segment(T, L, h) * codec.S, (decode, T, L)
        assert codec.lib.samaudio_codec_tile_samples(codec.ctx, 10, 0, int(decode)) < 0
        assert codec.lib.samaudio_codec_tile_samples(codec.ctx, 0, 4, int(decode)) < 0
    # the memory contract: what a tiled call needs does not depend on the clip's length once both halos are complete
    h = _halo(codec, True)
    assert _need(codec, 2, 3 * h + 3, h + 1, True) == _need(codec, 2, 40, h + 1, True) < _need(codec, 2, 40, 40, True)


@pytest.mark.parametrize("codec", ["fp32"], indirect=True)
@pytest.mark.parametrize("what", ["encode", "decode", "pairs"])
def test_launches_are_tiles_times_passes_and_rows_land_in_place(codec, what):
    """The emulation runs a frame of the codec in a fraction of a second, so the shapes with complete halos (L = h + 1 on T = 3L:
    minutes here) are left to tests/test_codec_tiles_gpu.py.  Here T = 3, where every segment is the whole clip: what is checked is
    the loop nest (tiles x passes x the launches of one pass), that each tile's last launch computes its own rows and writes them to
    their place in the NaN-filled destination - bit-equal to the whole call - and that L >= T is the plain call, launch for launch."""
    decode = what != "encode"
    T, items = 3, 2
    rc, one, whole = _run(codec, what, items, T, None, codec.lib.samaudio_workspace_bytes(codec.ctx, 0, 0, 0, items, T * codec.S))
    assert rc == 0, codec.lib.samaudio_last_error().decode()
    for L, cap, tiles in ((1, 2 if what == "pairs" else 1, 3), (2, 2, 2)):   # (L = 2: a short last tile)
        rc, launches, tiled = _run(codec, what, items, T, L, _need(codec, cap, T, L, decode))
        assert rc == 0, codec.lib.samaudio_last_error().decode()
        assert torch.equal(tiled, whole), (what, L, cap, (tiled != whole).nonzero()[:4])
        assert launches == tiles * (items // cap) * one, (what, L, cap, launches, one)
    rc, launches, same = _run(codec, what, items, T, T, _need(codec, items, T, T, decode))
    assert rc == 0 and launches == one and torch.equal(same, whole)


@pytest.mark.parametrize("codec", ["fp32"], indirect=True)
def test_refusals(codec):
    h = _halo(codec, True)
    T, L = 3 * h + 3, h + 1
    for what in ("encode", "decode", "pairs"):
        rc, launches, _ = _run(codec, what, 2, T, 0, _need(codec, 2, T, L, what != "encode"))
        assert rc == hip.ERR_ARG and launches == 0, what
    # one byte short of one segment of one item / of one pair
    rc, launches, _ = _run(codec, "encode", 1, T, L, _need(codec, 1, T, L, False) - 1)
    assert rc == hip.ERR_WORKSPACE and launches == 0
    rc, launches, _ = _run(codec, "decode", 1, T, L, _need(codec, 1, T, L, True) - 1)
    assert rc == hip.ERR_WORKSPACE and launches == 0
    rc, launches, _ = _run(codec, "pairs", 2, T, L, _need(codec, 2, T, L, True) - 1)
    assert rc == hip.ERR_WORKSPACE and launches == 0
