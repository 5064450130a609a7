"""Kernel-level parity of the glue kernels between the compute kernels, one C-ABI hook each (include/samaudio.h, csrc/api.hip):

    time_features_kernel, add_rowvec_kernel, headnorm_layers_kernel (every field evaluation)   samaudio_op_time_features / _add_rowvec / _headnorm_layers
    to_act_kernel, zero_halo_kernel, anchor_gather_kernel (prepare, codec, all towers)          samaudio_op_to_act / _zero_halo / _anchor_gather
    set_floats_kernel, ode_stage_kernel (the solvers)                                           samaudio_op_set_floats / _ode_stage
    repeat_rows_u8_kernel, repeat_items_f32_kernel (candidates, Judge)                          samaudio_op_repeat_rows / _repeat_items
    t5_embed_kernel (T5, ModernBERT), clap_text_embed_kernel, clap_score_kernel (CLAP)          samaudio_op_embed_rows / _clap_text_embed, samaudio_clap_score
    sentinel_scan_kernel + sentinel_fold_kernel, hash_items_kernel (the validation aids)        samaudio_op_sentinel / _hash_items

Conventions, helpers and the bound are those of tests/test_tower_kernels_gpu.py (imported, not copied): float64 torch references on the
CPU, fed the inputs rounded to the storage type; NaN-filled outputs with a guard row or item behind what the kernel owns; padding that
must be zero asserted bit-zero; bits compared where a kernel only copies or casts - a cast against torch's .to(bfloat16 / float16), which
rounds to nearest even.  No bound is chosen: arithmetic kernels get that file's _cmp (8 x the error of the same statement in float32
torch, floor 2^-23 max|ref|, plus half a storage ulp per element for 16-bit outputs).  Measured figures: profiles/glue_kernels/.

Passed counts: 315 on MI355X (both libraries), 206 on the SIMT simulator plain and with poisoned LDS (SAMAUDIO_EMU_DRYRUN=simt: bfloat16
library only, no CLAP kernels, so the fp16 and CLAP cases are hardware only; nothing else is left out, the cases above a grid cap
included), 160 passed + 46 skipped under the launcher emulation (SAMAUDIO_EMU_DRYRUN=1: ode_stage, embed_rows, sentinel and head_dim 64
of headnorm_layers are "not in this build of the library" there; its own C++ versions of the other launchers meet the same float64
statements).
"""
import ctypes as C
import math

import pytest
import torch

from sam_audio_amd import hip
from tests import util
from tests.test_tower_kernels_gpu import (LAUNCHER_EMU, NAN, S16, SIM, STORAGE, _act, _all_nan, _at, _bit_zero, _cmp, _code, _dev, _lib,
                                          _mk, _nan, _ok, _rnd, _same_bits)

pytestmark = pytest.mark.gpu
EPS = 1e-5   # norm_eps of every preset: what the engine hands launch_headnorm_layers


def _ints(shape, lo, hi, seed, dtype=torch.int64):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------
# time_features
# ---------------------------------------------------------------------------------------------------------------------
def _freqs(width):
    """sam_audio_amd/weights.py t_freqs / mem_inv_freq for a feature row of `width`"""
    half = width // 2
    return torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)


def _time_stmt(t, freqs, dtype):
    a = t.to(dtype)[:, None] * freqs.to(dtype)[None, :]
    return torch.cat([torch.cos(a), torch.sin(a)], 1)


def _time_values(nt):
    """a midpoint of a 1/16 step first, then 0, 1, 2^-20, the other midpoints and grid points, then a spread over [0, 1]"""
    base = [1 / 32, 0.0, 1.0, 2.0 ** -20] + [(2 * k + 1) / 32 for k in range(1, 16)] + [k / 16 for k in range(1, 16)]
    more = torch.rand(96, generator=torch.Generator().manual_seed(7)).tolist()
    return torch.tensor((base + more)[:nt], dtype=torch.float32)


def _time_run(gpu, prec, tag, t, fdim, D):
    nt, dt = t.numel(), _act(prec)
    freqs, inv = _freqs(fdim), _freqs(D)
    temb, tsin = _nan((nt + 1, fdim), dt, gpu), _nan((nt + 1, D), torch.float32, gpu)
    td, fd, vd = _dev(t, gpu), _dev(freqs, gpu), _dev(inv, gpu)
    _ok(prec, _lib(prec).samaudio_op_time_features(hip.ptr(td), nt, hip.ptr(fd), fdim, hip.ptr(vd), D, hip.ptr(temb), hip.ptr(tsin),
                                                   _code(prec), util.stream()))
    temb, tsin = temb.cpu(), tsin.cpu()
    assert _all_nan(temb[nt]) and _all_nan(tsin[nt]), "the row behind the output was written"
    for j in (t == 0).nonzero().flatten().tolist():
        one = torch.cat([torch.ones(fdim // 2), torch.zeros(fdim // 2)])
        assert _same_bits(temb[j], one.to(dt)), "temb of t = 0 must be 1 | 0 bit for bit"
        assert _same_bits(tsin[j], torch.cat([torch.ones(D // 2), torch.zeros(D // 2)])), "tsin of t = 0 must be 1 | 0 bit for bit"
    _cmp(f"{tag} temb", temb[:nt], _time_stmt(t, freqs, torch.float64), _time_stmt(t, freqs, torch.float32), dt)
    _cmp(f"{tag} tsin", tsin[:nt], _time_stmt(t, inv, torch.float64), _time_stmt(t, inv, torch.float32))


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("nt", [1, 2, 96])
@pytest.mark.parametrize("fdim,D", [(2, 4), (256, 512), (600, 1024), (256, 1024)])
def test_time_features(gpu, prec, nt, fdim, D):
    """One workgroup per time value, 256 threads striding over fdim / 2 and D / 2: one pair (2, 4), exactly one pass (256, 512), a
    ragged second pass (600: hf = 300) and two full passes (1024).  t holds 0 (whose row is exactly 1 | 0), 1, 2^-20 and the midpoints
    of a 1/16 step; temb is in the storage type, tsin always fp32."""
    _time_run(gpu, prec, f"time_features {prec} nt={nt} fdim={fdim} D={D}", _time_values(nt), fdim, D)


@pytest.mark.parametrize("prec", STORAGE)
def test_time_features_outside_the_solver_range(gpu, prec):
    """t = 37.5 (and -37.5): arguments up to 37.5 rad, where cosf / sinf have to reduce the argument; the same bound.  MI355X: fp32
    temb err 1.664e-6 and tsin 1.734e-6 of bounds 1.319e-5 and 1.363e-5 (the float32 statement's own error, 1.649e-6 and 1.704e-6, is
    the rounding of t * freq: half an ulp of 37.5 is 1.9e-6) - cosf and sinf reduce such arguments as well as float32 torch does."""
    _time_run(gpu, prec, f"time_features {prec} t=+-37.5", torch.tensor([37.5, -37.5, 0.0]), 600, 1024)


# ---------------------------------------------------------------------------------------------------------------------
# add_rowvec
# ---------------------------------------------------------------------------------------------------------------------
def _rowvec_run(gpu, prec, tag, rows, D, rpb, shared):
    dt = _act(prec)
    nb = (rows + rpb - 1) // rpb
    x = _mk((rows, D), 1000 + rows + D)
    vec = _mk((nb, D), 1001 + rpb)
    held = vec.clone()
    if shared:
        held[1:] = NAN   # vec_ld = 0: only row 0 exists for the kernel
    out = _nan((rows + 1, D), dt, gpu)
    xd, vd = _dev(x, gpu), _dev(held, gpu)
    _ok(prec, _lib(prec).samaudio_op_add_rowvec(hip.ptr(xd), hip.ptr(vd), 0 if shared else D, hip.ptr(out), _code(prec), rows, D, rpb,
                                                util.stream()))
    o = out.cpu()
    assert _all_nan(o[rows]), "the row behind the output was written"
    b = torch.zeros(rows, dtype=torch.long) if shared else torch.arange(rows) // rpb
    _cmp(tag, o[:rows], x.double() + vec.double()[b], x + vec[b], dt)


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("rpb", [1, 3, 7])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("D", [4, 516])
def test_add_rowvec(gpu, prec, rpb, shared, D):
    """out[r] = x[r] + vec[r / rows_per_b] (vec_ld = D) or + vec[0] (vec_ld = 0: the shared time value; the rows behind vec[0] hold
    NaN).  2 rows_per_b + 1 rows: the last item has one row only; D = 4 is one float4 per row, 516 = 129 float4: rows straddle the
    workgroups."""
    _rowvec_run(gpu, prec, f"add_rowvec {prec} rpb={rpb} {'shared' if shared else 'per item'} D={D}", 2 * rpb + 1, D, rpb, shared)


@pytest.mark.parametrize("prec", STORAGE)
def test_add_rowvec_above_the_grid_cap(gpu, prec):
    """1026 x 2048 = 525 312 float4 against the cap of 2048 x 256 = 524 288: the last 1024 float4 (rows 1024 and 1025) come from the
    second pass of the grid-stride loop; the guard row behind them stays NaN."""
    _rowvec_run(gpu, prec, f"add_rowvec {prec} 1026 x 2048", 1026, 2048, 7, False)


# ---------------------------------------------------------------------------------------------------------------------
# headnorm_layers
# ---------------------------------------------------------------------------------------------------------------------
def _headnorm_stmt(k, w, dtype, eps=EPS):
    """k [rows, L, H, hd], w [L, hd]"""
    k, w = k.to(dtype), w.to(dtype)
    return k * torch.rsqrt((k * k).mean(-1, keepdim=True) + eps) * w[None, :, None, :]


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("H", [1, 2, 5])
@pytest.mark.parametrize("hd", [64, 128])
def test_headnorm_layers(gpu, prec, rows, L, H, hd):
    """In place on the K half of every layer block of kv_all [rows, L * 2 * H * hd], one wave per (row, layer, head), four per
    workgroup: rows L H = 1 .. 45, mostly no multiple of four.  Every layer has its own weight row (a kernel that uses row 0 for all
    fails from L = 3 on); the V halves and the guard row come back with the same bits."""
    if LAUNCHER_EMU and hd == 64:
        pytest.skip("headnorm_layers with head_dim 64: not in this build of the library (the launcher emulation has head_dim 128 only)")
    dt = _act(prec)
    x = _mk((rows + 1, L, 2, H, hd), 1100 + rows + L + H + hd, 2.0)
    w = _mk((L, hd), 1101) + 1.5 * torch.arange(1, L + 1)[:, None]
    xd, wd = _dev(x.to(dt), gpu), _dev(w, gpu)
    _ok(prec, _lib(prec).samaudio_op_headnorm_layers(hip.ptr(xd), hip.ptr(wd), _code(prec), rows, L, H, hd, EPS, util.stream()))
    got = xd.cpu()
    assert _same_bits(got[rows], x[rows].to(dt)), "the row behind the last was changed"
    assert _same_bits(got[:rows, :, 1], x[:rows, :, 1].to(dt)), "a V half was changed"
    seen = _rnd(x[:rows, :, 0], prec)
    _cmp(f"headnorm_layers {prec} rows={rows} L={L} H={H} hd={hd}", got[:rows, :, 0], _headnorm_stmt(seen, w, torch.float64),
         _headnorm_stmt(seen, w, torch.float32), dt)


# ---------------------------------------------------------------------------------------------------------------------
# to_act, zero_halo
# ---------------------------------------------------------------------------------------------------------------------
# rounding ties of both 16-bit formats (to even: down and up), +-0, fp32 and fp16 subnormals, the fp16 overflow edge (65 519.996 rounds to
# 65 504, 65 520 is the tie that rounds to Inf), values beyond fp16 and the bfloat16 overflow edge
SPECIALS = torch.tensor([0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9,
                         1e-40, -1e-45, 3e-6, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -6e-8, 65504.0, 65519.996, 65520.0, -65520.0, 7e4, -1e5,
                         3.3895313892515355e38, 3.3961775292304e38, 3.4e38, -3.4e38, 1e-38, 2.0 ** -126, 2.0 ** -133 * 3], dtype=torch.float32)


def _with_specials(x):
    flat = x.reshape(-1)
    n = min(flat.numel(), SPECIALS.numel())
    flat[:n] = SPECIALS[:n]
    if flat.numel() >= 2 * SPECIALS.numel():
        flat[-SPECIALS.numel():] = SPECIALS.flip(0)
    return x


def _to_act(prec, src, in_bstride, in_ld, in_col0, out, out_bstride, B, T, C_in, C_out, halo, byte_offset=0):
    _ok(prec, _lib(prec).samaudio_op_to_act(hip.ptr(src), in_bstride, in_ld, in_col0, _at(out, byte_offset), out_bstride, _code(prec), B,
                                            T, C_in, C_out, halo, util.stream()))


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("T,C", [(1, 1), (37, 5), (300, 28)])
def test_to_act_dense_cast(gpu, prec, T, C):
    """The form of prepare and the towers: one item, in_ld = C_in = C_out, no halo.  The output carries the bits of torch's
    round-to-nearest-even cast of every input, ties, signed zeros, subnormals and overflow to Inf included (fp32: the input's bits)."""
    dt = _act(prec)
    x = _with_specials(_mk((T, C), 1200 + T))
    out = _nan((T + 1, C), dt, gpu)
    _to_act(prec, _dev(x, gpu), 0, C, 0, out, 0, 1, T, C, C, 0)
    o = out.cpu()
    assert _all_nan(o[T]), "the row behind the output was written"
    assert _same_bits(o[:T], x.to(dt)), "not the round-to-nearest-even cast"


@pytest.mark.parametrize("prec", STORAGE)
def test_to_act_waveform_into_8_channels(gpu, prec):
    """The codec encoder's form: mono samples (in_ld = 1, C_in = 1, items S apart) into channel 0 of 8, halo 40, dense items
    (out_bstride = 0).  Channels 1 .. 7 are bit-zero, the halo rows and the item behind the last stay NaN."""
    B, S, halo = 3, 50, 40
    dt = _act(prec)
    wav = _with_specials(_mk((B, S), 1210))
    out = _nan((B + 1, S + 2 * halo, 8), dt, gpu)
    _to_act(prec, _dev(wav, gpu), S, 1, 0, out, 0, B, S, 1, 8, halo)
    o = out.cpu()
    assert _all_nan(o[B]), "the item behind the last was written"
    assert _all_nan(o[:B, :halo]) and _all_nan(o[:B, halo + S:]), "a halo row was written"
    assert _bit_zero(o[:B, halo:halo + S, 1:]), "the padded channels must be bit-zero"
    assert _same_bits(o[:B, halo:halo + S, 0], wav.to(dt)), "channel 0 is not the round-to-nearest-even cast of the samples"


@pytest.mark.parametrize("prec", STORAGE)
def test_to_act_latent_halves(gpu, prec):
    """The decoder's form for (target | residual) pairs: state rows of 2 CD channels, item 2 b + s of the output = columns
    [s CD, (s + 1) CD) of state block b (in_ld = 2 CD, in_col0 = s CD), written behind a byte offset of s items with out_bstride of two
    items.  The s = 1 launch alone leaves the even items NaN."""
    n, T0, CD, halo = 4, 9, 6, 3
    dt = _act(prec)
    esz = 4 if dt == torch.float32 else 2
    item = (T0 + 2 * halo) * CD
    lat = _with_specials(_mk((n // 2, T0, 2 * CD), 1220))
    src = _dev(lat, gpu)
    out = _nan((n + 1, T0 + 2 * halo, CD), dt, gpu)
    for s in (1, 0):
        _to_act(prec, src, T0 * 2 * CD, 2 * CD, s * CD, out, 2 * item, n // 2, T0, CD, CD, halo, byte_offset=s * item * esz)
        o = out.cpu()
        if s == 1:
            assert _all_nan(o[0::2]), "the launch of the odd items wrote an even item"
        assert _all_nan(o[n]), "the item behind the last was written"
    assert _all_nan(o[:n, :halo]) and _all_nan(o[:n, halo + T0:]), "a halo row was written"
    for s in (0, 1):
        assert _same_bits(o[s:n:2, halo:halo + T0], lat[:, :, s * CD:(s + 1) * CD].contiguous().to(dt)), f"half {s}"


@pytest.mark.parametrize("prec", STORAGE)
def test_to_act_above_the_grid_cap(gpu, prec):
    """T C_out = 4099 x 64 = 262 336 against the cap of 1024 x 256 = 262 144: the last 192 elements of each of the two items come from
    the second pass of the grid-stride loop.  C_in = 60 of 64, halo 2."""
    B, T, C_in, C_out, halo = 2, 4099, 60, 64, 2
    dt = _act(prec)
    x = _with_specials(_mk((B, T, C_in), 1230))
    out = _nan((B + 1, T + 2 * halo, C_out), dt, gpu)
    _to_act(prec, _dev(x, gpu), T * C_in, C_in, 0, out, 0, B, T, C_in, C_out, halo)
    o = out.cpu()
    assert _all_nan(o[B]) and _all_nan(o[:B, :halo]) and _all_nan(o[:B, halo + T:]), "a halo row or the item behind the last was written"
    assert _bit_zero(o[:B, halo:halo + T, C_in:]), "the padded channels must be bit-zero"
    assert _same_bits(o[:B, halo:halo + T, :C_in], x.to(dt)), "not the round-to-nearest-even cast"


ZERO_HALO_CASES = [(B, T, C, 3) for B in (1, 3) for T in (1, 50) for C in (1, 8, 96)] + [(2, 5, 96, 171)]


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("B,T,C,halo", ZERO_HALO_CASES)
def test_zero_halo(gpu, prec, B, T, C, halo):
    """Both halos of every item become +0 bit for bit (they start as NaN), the interior keeps its bits and the item behind the last
    stays NaN.  halo C = 171 x 96 = 16 416 is above the cap of 64 x 256 = 16 384: the grid-stride loop iterates."""
    dt = _act(prec)
    x = _mk((B + 1, T + 2 * halo, C), 1300 + B + T + C)
    x[:, :halo] = NAN
    x[:, halo + T:] = NAN
    x[B] = NAN
    buf = _dev(x.to(dt), gpu)
    _ok(prec, _lib(prec).samaudio_op_zero_halo(hip.ptr(buf), _code(prec), B, T, C, halo, util.stream()))
    o = buf.cpu()
    assert _all_nan(o[B]), "the item behind the last was written"
    assert _bit_zero(o[:B, :halo]) and _bit_zero(o[:B, halo + T:]), "a halo is not bit-zero"
    assert _same_bits(o[:B, halo:halo + T], x[:B, halo:halo + T].to(dt)), "the interior was changed"


# ---------------------------------------------------------------------------------------------------------------------
# anchor_gather, embed_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("n_ids", [1, 3])
def test_anchor_gather(gpu, prec, E, n_ids):
    """out[b T + t] = emb[ids[b][align[b][t]]] cast to the storage type; 64 threads stride over E (below, at, above one pass, two
    passes and a tail).  B T = 21 rows.  As the kernel's comment says, a slot outside [0, n_ids) and a token outside [0, vocab) are
    clamped: slots -1 and n_ids, tokens -5 and vocab occur."""
    B, T, vocab = 3, 7, 11
    dt = _act(prec)
    emb = _mk((vocab, E), 1400 + E)
    ids = _ints((B, n_ids), 0, vocab, 1401 + n_ids)
    ids[0, 0], ids[2, n_ids - 1] = -5, vocab
    align = _ints((B, T), 0, n_ids, 1402)
    align[0, 1], align[1, 2], align[2, 6], align[0, 0] = -1, n_ids, n_ids, 0
    out = _nan((B * T + 1, E), dt, gpu)
    ed, idd, ald = _dev(emb, gpu), _dev(ids, gpu), _dev(align, gpu)
    _ok(prec, _lib(prec).samaudio_op_anchor_gather(hip.ptr(ed), hip.ptr(idd), n_ids, hip.ptr(ald), hip.ptr(out), _code(prec), B, T, E,
                                                   vocab, util.stream()))
    o = out.cpu()
    assert _all_nan(o[B * T]), "the row behind the output was written"
    tok = ids.gather(1, align.clamp(0, n_ids - 1)).clamp(0, vocab - 1)
    assert _same_bits(o[:B * T], emb[tok.reshape(-1)].to(dt)), "not the cast rows of the clamped tokens"


@pytest.mark.parametrize("D", [4, 768, 1028])
def test_embed_rows(gpu, D):
    """t5_embed_kernel copies table rows as float4, 256 threads per row: one float4, 192 (ModernBERT's width) and 257 - a second pass of
    one thread.  ids at 0 and vocab - 1 and outside both ends (clamped, as the kernel's comment says)."""
    vocab = 9
    ids = torch.tensor([0, vocab - 1, -3, vocab, vocab + 100, 4, -(2 ** 40), 2 ** 40, 5], dtype=torch.int64)
    M = ids.numel()
    table = _mk((vocab, D), 1500 + D)
    out = _nan((M + 1, D), torch.float32, gpu)
    idd, td = _dev(ids, gpu), _dev(table, gpu)
    _ok("fp32", _lib("fp32").samaudio_op_embed_rows(hip.ptr(idd), hip.ptr(td), hip.ptr(out), M, D, vocab, util.stream()))
    o = out.cpu()
    assert _all_nan(o[M]), "the row behind the output was written"
    assert _same_bits(o[:M], table[ids.clamp(0, vocab - 1)]), "not the rows of the clamped ids"


# ---------------------------------------------------------------------------------------------------------------------
# set_floats, ode_stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_set_floats(gpu, n):
    """Host values travel as kernel arguments, 64 per launch: below, at and above one launch, and three launches with a tail of 2.
    The three floats behind n stay NaN."""
    vals = _mk((n,), 1600 + n)
    vals[0] = -0.0
    dst = _nan((n + 3,), torch.float32, gpu)
    host = (C.c_float * n)(*vals.tolist())
    _ok("fp32", _lib("fp32").samaudio_op_set_floats(hip.ptr(dst), host, n, util.stream()))
    o = dst.cpu()
    assert _all_nan(o[n:]), "values behind n were written"
    assert _same_bits(o[:n], vals), "not the host values"


def _ode_stmt(y0, ks, coef, scale, dtype):
    s = coef[0] * ks[0].to(dtype)
    for c, k in zip(coef[1:], ks[1:]):
        s = s + c * k.to(dtype)
    return y0.to(dtype) + scale * s


ODE_COEF = [1.0 / 6, 1.0 / 3, -0.75, 2.0]   # (1/6 and 1/3 are not exact in fp32: the kernel sees what float(...) makes of them)
ODE_SIZES = [4, 4 * 257, 2048 * 256 * 4 + 4 * 257]


def _ode_run(gpu, n_src, n):
    coef32 = torch.tensor(ODE_COEF, dtype=torch.float32)
    scale = 0.0625 * 1.1
    scale32 = torch.tensor(scale, dtype=torch.float32).item()
    y0 = _mk((n + 4,), 1700 + n_src)
    ks = [_mk((n,), 1710 + j) for j in range(n_src)]
    kd = [_dev(k, gpu) for k in ks]
    poison = _nan((n,), torch.float32, gpu)   # what the slots n_src .. 3 point to, with a coefficient of 1: never read
    ptrs = (C.c_void_p * 4)(*[kd[j].data_ptr() if j < n_src else poison.data_ptr() for j in range(4)])
    coefs = (C.c_float * 4)(*[ODE_COEF[j] if j < n_src else 1.0 for j in range(4)])
    lib = _lib("fp32")
    # out a separate array
    yd = _dev(y0, gpu)
    out = _nan((n + 4,), torch.float32, gpu)
    _ok("fp32", lib.samaudio_op_ode_stage(hip.ptr(yd), ptrs, coefs, n_src, scale, hip.ptr(out), n, util.stream()))
    sep = out.cpu()
    assert _all_nan(sep[n:]), "values behind n were written"
    assert _same_bits(yd.cpu(), y0), "y0 was changed although out is another array"
    # out == y0
    _ok("fp32", lib.samaudio_op_ode_stage(hip.ptr(yd), ptrs, coefs, n_src, scale, hip.ptr(yd), n, util.stream()))
    inp = yd.cpu()
    assert _same_bits(inp[n:], y0[n:]), "values behind n were changed"
    assert _same_bits(inp[:n], sep[:n]), "in place and out of place differ"
    c64 = coef32.double().tolist()[:n_src]
    want = _ode_stmt(y0[:n], ks, c64, scale32, torch.float64)
    f32 = _ode_stmt(y0[:n], ks, coef32.tolist()[:n_src], scale32, torch.float32)
    for name, got in (("out of place", sep), ("in place", inp)):
        _cmp(f"ode_stage n_src={n_src} n={n} {name}", got[:n], want, f32)


@pytest.mark.parametrize("n_src", [1, 2, 3, 4])
@pytest.mark.parametrize("n", ODE_SIZES[:2])
def test_ode_stage(gpu, n_src, n):
    """out = y0 + scale (c0 k0 + ...) with 1 .. 4 sources, into another array and over y0 itself: the same bits both ways, each held
    against float64.  n = 4 is one float4 on one lane, 4 x 257 a second workgroup with one live lane.  The pointer slots n_src .. 3
    point to a NaN array with coefficient 1 - the engine leaves the sources with a zero tableau coefficient out of the list, so the
    kernel must not look past n_src."""
    _ode_run(gpu, n_src, n)


@pytest.mark.parametrize("n_src", [1, 4])
def test_ode_stage_above_the_grid_cap(gpu, n_src):
    """n = 2048 x 256 x 4 + 4 x 257: the grid is capped at 2048 workgroups and the last 257 float4 come from the second pass."""
    _ode_run(gpu, n_src, ODE_SIZES[2])


# ---------------------------------------------------------------------------------------------------------------------
# repeat_rows, repeat_items
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("T", [1, 255, 257])
def test_repeat_rows(gpu, rep, T):
    """dst[b rep + c] = src[b], sample-major (repeat_interleave), bytes; 3 rows of T bytes: below and across the 256-thread
    workgroups.  The row behind the last keeps its 0xEE bytes."""
    rows = 3
    src = _ints((rows, T), 0, 256, 1800 + T, torch.uint8)
    dst = torch.full((rows * rep + 1, T), 0xEE, dtype=torch.uint8, device=gpu)
    sd = _dev(src, gpu)
    _ok("fp32", _lib("fp32").samaudio_op_repeat_rows(hip.ptr(sd), hip.ptr(dst), rows, rep, T, util.stream()))
    o = dst.cpu()
    assert bool((o[rows * rep] == 0xEE).all()), "the row behind the last was written"
    assert torch.equal(o[:rows * rep], src.repeat_interleave(rep, 0)), "not the sample-major repeat"


@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("elems", [4, 1028])
def test_repeat_items(gpu, rep, elems):
    """The same for items of fp32 values moved as float4: one float4 per item, and 257 (items straddle the workgroups)."""
    items = 3
    src = _mk((items, elems), 1810 + elems)
    src[0, 0] = -0.0
    dst = _nan((items * rep + 1, elems), torch.float32, gpu)
    sd = _dev(src, gpu)
    _ok("fp32", _lib("fp32").samaudio_op_repeat_items(hip.ptr(sd), hip.ptr(dst), items, rep, elems, util.stream()))
    o = dst.cpu()
    assert _all_nan(o[items * rep]), "the item behind the last was written"
    assert _same_bits(o[:items * rep], src.repeat_interleave(rep, 0)), "not the sample-major repeat"


# ---------------------------------------------------------------------------------------------------------------------
# CLAP: clap_text_embed, clap_score (clap_kernels.hip is in the product libraries only: hardware only, like tests/test_clap_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
if not SIM:
    def _position_ids(ids, pad):
        """transformers' create_position_ids_from_input_ids (modeling_clap.py), written out"""
        mask = ids.ne(pad).int()
        incremental = torch.cumsum(mask, dim=1).type_as(mask) * mask
        return incremental.long() + pad

    def _clap_embed_stmt(ids, word, pos, typ, pad, dtype):
        vocab = word.shape[0]
        return (word.to(dtype)[ids.clamp(0, vocab - 1)] + typ.to(dtype)[0]) + pos.to(dtype)[_position_ids(ids, pad)]

    def _clap_ids(T, vocab, pad):
        """row 0: pads at the head | 1: pads in the middle | 2: pads only | 3: no pad, ids outside [0, vocab) | 4: pads at the tail"""
        ids = _ints((5, T), 2, vocab, 1900 + T)
        ids[0, :max(1, T // 3)] = pad
        ids[1, T // 3:T // 3 + max(1, T // 4)] = pad
        ids[2] = pad
        ids[3, 0], ids[3, T - 1] = -2, vocab + 5
        ids[4, T - max(1, T // 5):] = pad
        return ids

    @pytest.mark.parametrize("T", [1, 256, 257, 512])
    def test_clap_text_embed(gpu, T):
        """word + token type 0 + position rows, the position ids from the running count of non-pad ids (one thread scans the flags of
        a row in LDS): T = 1, one pass of the 256 threads, one token more, two passes.  The position table has exactly
        pad + T + 1 rows; an id outside the vocabulary is clamped for the lookup but counts as a non-pad token."""
        vocab, pad, D = 13, 1, 8
        ids = _clap_ids(T, vocab, pad)
        rows = ids.shape[0]
        word, pos, typ = _mk((vocab, D), 1901), _mk((pad + T + 1, D), 1902), _mk((2, D), 1903)
        out = _nan((rows + 1, T, D), torch.float32, gpu)
        idd, wd, pd, td = _dev(ids, gpu), _dev(word, gpu), _dev(pos, gpu), _dev(typ, gpu)
        _ok("fp32", _lib("fp32").samaudio_op_clap_text_embed(hip.ptr(idd), hip.ptr(wd), hip.ptr(pd), hip.ptr(td), hip.ptr(out), rows, T, D,
                                                             vocab, pad, pad + T + 1, util.stream()))
        o = out.cpu()
        assert _all_nan(o[rows]), "the item behind the output was written"
        assert int(_position_ids(ids, pad).max()) == pad + T, "the case must reach the last row of the position table"
        _cmp(f"clap_text_embed T={T}", o[:rows], _clap_embed_stmt(ids, word, pos, typ, pad, torch.float64),
             _clap_embed_stmt(ids, word, pos, typ, pad, torch.float32))
        # one row fewer in the table: refused, nothing written
        out2 = _nan((rows, T, D), torch.float32, gpu)
        lib = _lib("fp32")
        rc = lib.samaudio_op_clap_text_embed(hip.ptr(idd), hip.ptr(wd), hip.ptr(pd), hip.ptr(td), hip.ptr(out2), rows, T, D, vocab, pad,
                                             pad + T, util.stream())
        assert rc == hip.ERR_ARG and b"position table" in lib.samaudio_last_error() and _all_nan(out2.cpu())

    @pytest.mark.parametrize("dim", [1, 63, 64, 65, 512])
    @pytest.mark.parametrize("cand", [1, 3])
    @pytest.mark.parametrize("clips", [1, 2])
    def test_clap_score(gpu, dim, cand, clips):
        """scores[b][c] = <audio[b cand + c], text[b]>: one wave per score striding over dim (one lane, below, at and above one pass,
        eight passes); candidate c of clip b must meet text row b, not b cand + c."""
        audio, text = _mk((clips * cand, dim), 1950 + dim), _mk((clips, dim), 1951 + cand)
        out = _nan((clips * cand + 2,), torch.float32, gpu)
        ad, td = _dev(audio, gpu), _dev(text, gpu)
        hip.check(hip.clap_lib().samaudio_clap_score(hip.ptr(ad), hip.ptr(td), clips, cand, dim, hip.ptr(out), util.stream()))
        o = out.cpu()
        assert _all_nan(o[clips * cand:]), "values behind the output were written"
        stmt = lambda dtype: torch.einsum("bcd,bd->bc", audio.to(dtype).view(clips, cand, dim), text.to(dtype))
        _cmp(f"clap_score dim={dim} cand={cand} clips={clips}", o[:clips * cand].view(clips, cand), stmt(torch.float64), stmt(torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the validation aids: sentinel, hash_items
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL_FORMATS = [("bf16", 0), ("bf16", 1), ("bf16", 2)] + ([] if SIM else [("fp16", 1), ("fp16", 2)])
SENTINEL_SHAPES = [(1, 1, 3), (17, 241, 250), (1025, 1024, 1032)]   # (rows, cols, ld): totals 1, 4097 and 1 049 600 > 256 x 4096


def _sentinel_dtype(prec, fmt):
    return torch.float32 if fmt == 0 else (torch.bfloat16 if fmt == 2 else _act(prec))


def _sentinel_scan(gpu, prec, fmt, x, slot, rows, cols, ld):
    """one launch on a pitched copy of x [rows, cols] whose gap holds NaN, with a scratch that starts as NaN; -> the slot afterwards"""
    held = torch.full((rows, ld), NAN, dtype=x.dtype)
    held[:, :cols] = x
    scratch = _nan((2 * 256 + 2,), torch.float32, gpu)
    xd = _dev(held, gpu)
    _ok(prec, _lib(prec).samaudio_op_sentinel(hip.ptr(xd), fmt, rows, cols, ld, hip.ptr(scratch), hip.ptr(slot), util.stream()))
    grid = min(256, max(1, (rows * cols + 4095) // 4096))
    s = scratch.cpu()
    assert bool(torch.isfinite(s[:2 * grid]).all()), "a partial of a launched workgroup was not written"
    assert _all_nan(s[2 * grid:]), "partials behind the launched workgroups were written"
    return slot.cpu().clone()


@pytest.mark.parametrize("prec,fmt", SENTINEL_FORMATS)
@pytest.mark.parametrize("rows,cols,ld", SENTINEL_SHAPES)
def test_sentinel(gpu, prec, fmt, rows, cols, ld):
    """What tests/test_hostile_gpu.py relies on.  A slot preset to {5, 2} accumulates over five launches and is never overwritten:
    clean data below 5 leaves it, a largest magnitude of 7.5 at the first element raises it, then a single NaN, +Inf and -Inf in the
    LAST element of the pitched tensor add one each - while the NaN in the pitch gap and the NaN partials of the scratch that no
    workgroup wrote are never counted.  The rule of samaudio.h: non-finite = NaN and +-Inf only, so the largest finite values of the
    format (bfloat16 3.39e38, fp16 65 504, fp32 3.40e38 - the scan used to count everything above 3.0e38 as non-finite) are
    magnitudes: a fresh slot reports them with a count of 0."""
    dt = _sentinel_dtype(prec, fmt)
    x = (_mk((rows, cols), 2000 + rows).clamp(-4, 4) * 0.75).to(dt)
    slot = _dev(torch.tensor([5.0, 2.0]), gpu)
    assert _sentinel_scan(gpu, prec, fmt, x, slot, rows, cols, ld).tolist() == [5.0, 2.0], "clean data below the slot's maximum"
    x[0, 0] = -7.5
    assert _sentinel_scan(gpu, prec, fmt, x, slot, rows, cols, ld).tolist() == [7.5, 2.0], "a larger magnitude"
    for i, bad in enumerate((NAN, float("inf"), float("-inf"))):
        y = x.clone()
        y[rows - 1, cols - 1] = bad
        assert _sentinel_scan(gpu, prec, fmt, y, slot, rows, cols, ld).tolist() == [7.5, 3.0 + i], f"a single {bad} in the last element"
    top = torch.finfo(dt).max
    y = x.clone()
    y[rows - 1, cols - 1] = top
    y[0, 0] = -top
    fresh = _dev(torch.zeros(2), gpu)
    assert _sentinel_scan(gpu, prec, fmt, y, fresh, rows, cols, ld).tolist() == [top, 0.0], "the largest finite value is a magnitude"


def _hash(words):
    h = 0
    for i, w in enumerate(words):
        h += (w ^ ((i * 0x9E3779B1) & 0xFFFFFFFF)) * (2 * i + 1)
    return h & 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("words", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("items", [1, 3])
def test_hash_items(gpu, words, items):
    """out[b] = sum_i (x[b][i] ^ (i 0x9E3779B1 mod 2^32)) (2 i + 1) mod 2^64 in Python integers; 256 threads stride over the words:
    one, one short of a pass, a pass, one more, four ragged passes.  One flipped bit changes the item's hash and no other; so does
    swapping two unequal words."""
    x = _ints((items, words), 0, 2 ** 32, 2100 + words)   # the words as unsigned values
    lib = _lib("fp32")

    def run(t):
        td = _dev(torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32), gpu)
        out = torch.full((items + 1,), -0x1111111111111112, dtype=torch.int64, device=gpu)
        _ok("fp32", lib.samaudio_op_hash_items(hip.ptr(td), words, items, hip.ptr(out), util.stream()))
        o = out.cpu().tolist()
        assert o[items] == -0x1111111111111112, "the value behind the output was written"
        got = [v & 0xFFFFFFFFFFFFFFFF for v in o[:items]]
        assert got == [_hash(row) for row in t.tolist()]
        return got

    base = run(x)
    b, i = items - 1, words - 1
    flipped = x.clone()
    flipped[b, i] ^= 1 << 31
    got = run(flipped)
    assert got[b] != base[b] and got[:b] == base[:b], "a flipped bit"
    if words > 1:
        swapped = x.clone()
        swapped[b, 0], swapped[b, i] = x[b, i], x[b, 0]
        assert int(x[b, 0]) != int(x[b, i])
        assert run(swapped)[b] != base[b], "two words swapped"


# ---------------------------------------------------------------------------------------------------------------------
# what the hooks refuse
# ---------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_the_kernels_do_not_cover(gpu):
    """Every refusal of the hooks, each on otherwise valid arguments (real buffers, so that the named reason is the only one) and by its
    message; nothing is launched: the NaN-filled outputs are untouched afterwards.  The argument checks come before the "not in this
    build" answer, so this runs on every library."""
    lib = _lib("bf16")
    st = util.stream()
    src = _dev(torch.zeros(4096), gpu)
    ids = _dev(torch.zeros(64, dtype=torch.int64), gpu)
    u8 = _dev(torch.ones(64, dtype=torch.uint8), gpu)
    o32, o16 = _nan((4096,), torch.float32, gpu), _nan((4096,), torch.bfloat16, gpu)
    S, I, O, H, z = hip.ptr(src), hip.ptr(ids), hip.ptr(o32), hip.ptr(o16), C.c_void_p(0)

    def refused(rc, why):
        msg = lib.samaudio_last_error().decode()
        assert rc == hip.ERR_ARG and why in msg, (rc, why, msg)

    tf = lambda t=S, temb=O, tsin=O, nt=1, fdim=4, D=4: lib.samaudio_op_time_features(t, nt, S, fdim, S, D, temb, tsin, hip.F32, st)
    refused(tf(fdim=5), "odd freq_dim")
    refused(tf(D=7), "odd dim")
    refused(tf(nt=0), "n_time < 1")
    for null in ("t", "temb", "tsin"):
        refused(tf(**{null: z}), "null argument")
    rv = lambda x=S, vec=S, out=O, prec=hip.F32, vec_ld=4, rows=2, D=4, rpb=1: lib.samaudio_op_add_rowvec(x, vec, vec_ld, out, prec, rows,
                                                                                                         D, rpb, st)
    refused(rv(D=6), "dim % 4")
    refused(rv(vec_ld=2), "vec_ld % 4")
    refused(rv(rows=0), "rows / rows_per_batch < 1")
    refused(rv(rpb=0), "rows / rows_per_batch < 1")
    refused(rv(x=_at(src, 4)), "aligned to 16 bytes")
    refused(rv(vec=_at(src, 8)), "aligned to 16 bytes")
    refused(rv(out=_at(o32, 8)), "aligned to 16 bytes")
    refused(rv(out=_at(o16, 4), prec=hip.BF16), "aligned to 16 bytes")
    refused(rv(out=z), "null argument")
    hn = lambda kv=O, w=S, prec=hip.F32, rows=1, L=1, Hh=1, hd=64: lib.samaudio_op_headnorm_layers(kv, w, prec, rows, L, Hh, hd, EPS, st)
    refused(hn(hd=32), "head_dim")
    refused(hn(hd=96), "head_dim")
    refused(hn(L=0), "rows / layers / heads < 1")
    refused(hn(kv=_at(o32, 4)), "aligned to 8")
    refused(hn(kv=_at(o16, 2), prec=hip.BF16), "aligned to 8")
    refused(hn(kv=z), "null argument")
    ta = lambda inp=S, out=O, B=1, T=2, ci=2, co=2, halo=0, in_ld=2: lib.samaudio_op_to_act(inp, 0, in_ld, 0, out, 0, hip.F32, B, T, ci, co,
                                                                                           halo, st)
    refused(ta(ci=3), "c_in > c_out")
    refused(ta(T=0), "< 1")
    refused(ta(halo=-1), "negative")
    refused(ta(in_ld=-2), "negative")
    refused(ta(out=z), "null argument")
    refused(lib.samaudio_op_zero_halo(O, hip.F32, 1, 2, 2, 0, st), "halo < 1")
    refused(lib.samaudio_op_zero_halo(z, hip.F32, 1, 2, 2, 1, st), "null buf")
    ag = lambda emb=S, i=I, al=I, out=O, n_ids=1, vocab=4: lib.samaudio_op_anchor_gather(emb, i, n_ids, al, out, hip.F32, 1, 2, 4, vocab, st)
    refused(ag(n_ids=0), "< 1")
    refused(ag(vocab=0), "< 1")
    refused(ag(i=_at(ids, 4)), "aligned to 8 bytes")
    refused(ag(out=z), "null argument")
    host = (C.c_float * 4)(1, 2, 3, 4)
    refused(lib.samaudio_op_set_floats(O, host, 0, st), "n < 1")
    refused(lib.samaudio_op_set_floats(z, host, 4, st), "null argument")
    ks = (C.c_void_p * 4)(src.data_ptr(), src.data_ptr(), src.data_ptr(), src.data_ptr())
    cs = (C.c_float * 4)(1, 1, 1, 1)
    ode = lambda y0=S, k=ks, out=O, n_src=1, n=8: lib.samaudio_op_ode_stage(y0, k, cs, n_src, 1.0, out, n, st)
    refused(ode(n_src=0), "n_src outside [1, 4]")
    refused(ode(n_src=5), "n_src outside [1, 4]")
    refused(ode(n=6), "n % 4")
    refused(ode(n=0), "n % 4")
    refused(ode(y0=_at(src, 4)), "aligned to 16 bytes")
    refused(ode(out=_at(o32, 8)), "aligned to 16 bytes")
    refused(ode(k=(C.c_void_p * 4)(src.data_ptr(), src.data_ptr() + 4, 0, 0), n_src=2), "aligned to 16 bytes")
    refused(ode(k=(C.c_void_p * 4)(src.data_ptr(), 0, 0, 0), n_src=2), "null argument")
    refused(ode(out=z), "null argument")
    refused(lib.samaudio_op_repeat_rows(hip.ptr(u8), hip.ptr(u8), 1, 0, 4, st), "< 1")
    refused(lib.samaudio_op_repeat_rows(hip.ptr(u8), z, 1, 1, 4, st), "null argument")
    refused(lib.samaudio_op_repeat_items(S, O, 1, 1, 6, st), "elems % 4")
    refused(lib.samaudio_op_repeat_items(S, O, 0, 1, 4, st), "< 1")
    refused(lib.samaudio_op_repeat_items(_at(src, 4), O, 1, 1, 4, st), "aligned to 16 bytes")
    refused(lib.samaudio_op_repeat_items(S, _at(o32, 8), 1, 1, 4, st), "aligned to 16 bytes")
    er = lambda i=I, table=S, out=O, M=2, D=4, vocab=4: lib.samaudio_op_embed_rows(i, table, out, M, D, vocab, st)
    refused(er(D=6), "dim % 4")
    refused(er(M=0), "< 1")
    refused(er(table=_at(src, 4)), "aligned to 16 bytes")
    refused(er(out=_at(o32, 4)), "aligned to 16 bytes")
    refused(er(out=z), "null argument")
    ce = lambda i=I, out=O, T=2, pad=1, maxp=4, rows=1: lib.samaudio_op_clap_text_embed(i, S, S, S, out, rows, T, 4, 4, pad, maxp, st)
    refused(ce(T=1025, maxp=4096), "tokens > 1024")
    refused(ce(maxp=3), "position table")
    refused(ce(T=0), "< 1")
    refused(ce(pad=-1), "pad_id < 0")
    refused(ce(out=z), "null argument")
    sn = lambda x=S, fmt=0, rows=2, cols=2, ld=2, scratch=O, slot=O: lib.samaudio_op_sentinel(x, fmt, rows, cols, ld, scratch, slot, st)
    refused(sn(fmt=3), "format outside 0..2")
    refused(sn(ld=1), "ld < cols")
    refused(sn(rows=0), "rows / cols < 1")
    refused(sn(x=_at(src, 2)), "element size")
    refused(sn(slot=z), "null argument")
    refused(lib.samaudio_op_hash_items(S, 0, 1, I, st), "< 1")
    refused(lib.samaudio_op_hash_items(S, 4, 1, z, st), "null argument")
    assert _all_nan(o32.cpu()) and _all_nan(o16.cpu()), "a refused call wrote its output"
    assert not bool(ids.cpu().any()), "a refused call wrote its output"
