"""Kernel-level parity of the kernels that only the towers launch, one C-ABI hook each (include/samaudio.h, csrc/api.hip):

    t5_attention_kernel (T5, ModernBERT and CLAP text towers), mbert_rope_kernel, geglu_kernel       samaudio_op_tower_attention / _mbert_rope / _geglu
    rope2d_split_kernel, rope2d_split_bf16_kernel, pool_attention_kernel, l2_normalize_kernel,
    token_mean_kernel (PE-Core vision tower)                           samaudio_op_rope2d_split / _pool_attention / _l2_normalize / _token_mean
    peav_cls_mask_kernel, judge_pool_head_kernel, frame_logits_kernel (Judge, span predictor)       samaudio_op_peav_cls_mask / _judge_pool_head / _frame_logits

Conventions of tests/test_layer_kernels_gpu.py: every reference is float64 torch on the CPU; a 16-bit form's reference is fed the inputs
rounded to the storage type; every output starts as NaN and carries a guard row (or item) behind what the kernel owns, which must still
be NaN afterwards; padding that must be zero is asserted bit-zero; where a kernel only copies, the bits are compared.

No bound is chosen (the rule of tests/test_clap_gpu.py): each test evaluates the very statement of its float64 reference in float32 torch
on the CPU and allows the kernel 8 x that statement's largest error, with a floor of 2^-23 x the largest |reference| (a tiny case can make
the float32 error exactly 0).  A 16-bit form gets, per element, half a unit in the last place of the storage type at the larger of |got|
and |reference| on top: the stores round to nearest even (csrc/common.h f2bf, pack_h16x2).  Measured figures: profiles/tower_kernels/.

On the CPU the file runs on the functional SIMT simulator (SAMAUDIO_EMU_DRYRUN=simt: bfloat16 library only, so the fp16 cases are
hardware only).  The launcher emulation (SAMAUDIO_EMU_DRYRUN=1) carries the three PE-AV launchers only: the other hooks answer "not in
this build of the library" there and their tests skip with that reason.
"""
import ctypes as C
import math
import os

import pytest
import torch

from sam_audio_amd import hip
from tests import util

pytestmark = pytest.mark.gpu
EMU_MODE = os.environ.get("SAMAUDIO_EMU_DRYRUN", "")
SIM = EMU_MODE != ""
LAUNCHER_EMU = EMU_MODE == "1"
S16 = ["bf16"] if SIM else ["bf16", "fp16"]
STORAGE = ["fp32"] + S16
NAN = float("nan")
FACTOR = 8.0


def _lib(prec):
    return hip.lib(hip.operands_for(prec))


def _code(prec):
    return hip.precision_code(prec)


def _act(prec):
    return hip.act_dtype(prec)


def _rnd(x, prec):
    """what a kernel of this storage type sees of an fp32 host tensor, as float64"""
    return x.to(_act(prec)).double()


def _mk(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _nan(shape, dtype, gpu):
    return torch.full(shape, NAN, dtype=dtype, device=gpu)


def _dev(x, gpu, dtype=None):
    return x.to(gpu, dtype).contiguous() if dtype is not None else x.to(gpu).contiguous()


def _at(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _bit_zero(t):
    return t.numel() == 0 or not bool(_bits(t.cpu()).any())   # (+0.0 only: -0.0 and NaN have bits set)


def _ok(prec, rc):
    """hip.check, but a hook whose launcher the launcher emulation lacks skips the test there (and only there)"""
    if rc == hip.ERR_STATE and LAUNCHER_EMU:
        msg = _lib(prec).samaudio_last_error().decode()
        if "not in this build" in msg:
            pytest.skip(msg)
    hip.check(rc)


def _ulp16(x, dtype):
    """unit in the last place of a 16-bit value's binade (IEEE half: the subnormal quantum below 2^-14)"""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


def _cmp(name, got, want, f32, dtype=torch.float32):
    """`want`: the float64 statement, `f32`: the same statement evaluated in float32, `dtype`: the storage type `got` was rounded to.
    Prints the error next to its bound, then asserts (a NaN in `got` fails: the comparison is False)."""
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    e32 = (f32.double() - want).abs().max().item()
    bound = max(FACTOR * e32, 2.0 ** -23 * want.abs().max().item())
    err = (got - want).abs()
    room = torch.full_like(err, bound)
    if dtype != torch.float32:
        room = room + 0.5 * _ulp16(torch.maximum(got.abs(), want.abs()), dtype)
    excess = (err - room).max().item()
    ratio = (err / room.clamp_min(2.0 ** -1074)).max().item()   # (an all-zero reference has bound 0: 0 / tiny = 0, anything else is huge)
    half = "" if dtype == torch.float32 else f" + half a {str(dtype)[6:]} ulp per element"
    print(f"{name}: max-abs err {err.max().item():.3e} (bound {bound:.3e}{half}: float32 statement {e32:.3e}, |ref| <= "
          f"{want.abs().max().item():.3f}); worst err / bound {ratio:.3f}")
    assert excess <= 0, f"{name}: error exceeds the bound by {excess} ({ratio} x)"


# ---------------------------------------------------------------------------------------------------------------------
# tower attention (t5_attention_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def _attn_stmt(qkv, mask, bias, B, Lt, H, dkv, max_len, scale, window, dtype):
    """softmax over the allowed keys (unmasked, and within +-window when window > 0) of scale q k^T + bias[h][k - q]; a query row
    without an allowed key attends uniformly over all Lt keys; every query row is computed.  -> [B * Lt, H * dkv]"""
    x = qkv.to(dtype).view(B, Lt, 3, H, dkv)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * scale
    pos = torch.arange(Lt)
    dist = pos[None, :] - pos[:, None]   # [query, key] = k - q
    if bias is not None:
        s = s + bias.to(dtype)[:, dist + (max_len - 1)][None]
    allowed = mask.bool()[:, None, None, :].expand(B, H, Lt, Lt)
    if window > 0:
        allowed = allowed & (dist.abs() <= window)[None, None]
    s = s.masked_fill(~allowed, float("-inf"))
    s = torch.where(allowed.any(-1, keepdim=True), s, torch.zeros((), dtype=dtype))
    p = torch.softmax(s, -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * Lt, H * dkv)


def _attn_run(gpu, prec, tag, qkv, mask, bias, B, Lt, H, dkv, max_len, scale, window):
    dt = _act(prec)
    qd, md = _dev(qkv, gpu, dt), _dev(mask.to(torch.uint8), gpu)
    bd = _dev(bias, gpu) if bias is not None else None
    out = _nan((B * Lt + 1, H * dkv), dt, gpu)
    _ok(prec, _lib(prec).samaudio_op_tower_attention(hip.ptr(qd), hip.ptr(md), hip.ptr(bd), hip.ptr(out), _code(prec), B, Lt, H, dkv,
                                                     max_len, scale, window, util.stream()))
    o = out.cpu()
    assert _all_nan(o[B * Lt]), "the row behind the output was written"
    assert _same_bits(qd, qkv.to(dt)), "the kernel changed its input"
    seen = _rnd(qkv, prec)
    want = _attn_stmt(seen, mask, bias, B, Lt, H, dkv, max_len, scale, window, torch.float64)
    f32 = _attn_stmt(seen, mask, bias, B, Lt, H, dkv, max_len, scale, window, torch.float32)
    _cmp(tag, o[:B * Lt], want, f32, dt)


def _t5_mask(Lt):
    """item 0: holes at keys 0, 3 and Lt - 1 where they exist | item 1: no valid key | item 2: every key (another non-zero byte)"""
    m = torch.zeros(3, Lt, dtype=torch.uint8)
    m[0] = 1
    for k in (0, 3, Lt - 1):
        if k < Lt:
            m[0, k] = 0
    m[2] = 255
    return m


T5_CASES = ([("fp32", Lt, dkv) for Lt in (1, 64, 65, 200) for dkv in (64, 128)] + [("fp32", 512, dkv) for dkv in (16, 64, 128)]
            + [(p, Lt, dkv) for p in S16 for Lt, dkv in ((65, 64), (200, 64), (200, 128))])


@pytest.mark.parametrize("prec,Lt,dkv", T5_CASES)
def test_tower_attention_t5_form(gpu, prec, Lt, dkv):
    """The T5 form: bias per head and signed distance, scale 1, no window.  Lt = 1, the chunk edges 64 / 65, chunk 3 (200) and all 8
    chunks with ps[512] full (512: what the CLAP text tower launches); max_len = Lt + 5 (512 at 512) so the row offset
    (max_len - 1) - q of the bias matters; masks with holes, without any valid key (the uniform branch) and full.  q carries
    dkv^-0.5 so that the softmax mixes many keys."""
    B, H = 3, 2
    max_len = 512 if Lt == 512 else Lt + 5
    qkv = _mk((B * Lt, 3, H, dkv), 100 + Lt + dkv)
    qkv[:, 0] *= dkv ** -0.5
    bias = _mk((H, 2 * max_len - 1), 101 + Lt)
    _attn_run(gpu, prec, f"tower_attention T5 {prec} Lt={Lt} dkv={dkv}", qkv.reshape(B * Lt, -1), _t5_mask(Lt), bias, B, Lt, H, dkv,
              max_len, 1.0, 0)


def _mbert_mask(Lt):
    """the T5 items, and item 3: key 0 alone - a query further than `window` from it has its whole window masked"""
    m = torch.zeros(4, Lt, dtype=torch.uint8)
    m[:3] = _t5_mask(Lt)
    m[3, 0] = 1
    return m


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("Lt", [9, 150])
@pytest.mark.parametrize("window", [0, 4, 64])
def test_tower_attention_modernbert_form(gpu, prec, Lt, window):
    """The ModernBERT form: no bias, scale dkv^-0.5, key k allowed iff unmasked and |k - q| <= window (distance `window` in, window + 1
    out: tests/test_mbert_gpu.py pins that against transformers).  Item 3 has key 0 alone valid: with a window, queries beyond it take
    the uniform branch while queries within it attend to key 0 only."""
    B, H, dkv = 4, 2, 32
    qkv = _mk((B * Lt, 3 * H * dkv), 110 + Lt + window)
    _attn_run(gpu, prec, f"tower_attention ModernBERT {prec} Lt={Lt} window={window}", qkv, _mbert_mask(Lt), None, B, Lt, H, dkv,
              Lt, dkv ** -0.5, window)


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("peak", [80, 100])
def test_tower_attention_large_logits(gpu, prec, peak):
    """q scaled until the scores reach +-80, and +-100.  fp32 exp() overflows from 88.7 on: at 80 a softmax without the max subtraction
    still gets finite terms (the seeded fault survived that case on the simulator), at 100 it divides inf by inf."""
    B, H, Lt, dkv = 3, 2, 65, 64
    qkv = _mk((B * Lt, 3, H, dkv), 120)
    s = torch.einsum("bqhd,bkhd->bhqk", qkv[:, 0].reshape(B, Lt, H, dkv), qkv[:, 1].reshape(B, Lt, H, dkv))
    qkv[:, 0] *= peak / s.abs().max()
    _attn_run(gpu, prec, f"tower_attention logits to +-{peak} {prec}", qkv.reshape(B * Lt, -1), _t5_mask(Lt), None, B, Lt, H, dkv, Lt,
              1.0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# mbert_rope, geglu
# ---------------------------------------------------------------------------------------------------------------------
def _rotate_half_stmt(x, cos, sin, B, Lt, H, hd, dtype):
    """x [B * Lt, 3, H, hd]: q and k segments -> x cos + rotate_half(x) sin with the table row of the token's position; v as it is"""
    x = x.to(dtype).view(B, Lt, 3, H, hd)
    c, s = cos.to(dtype)[:Lt, None, None, :], sin.to(dtype)[:Lt, None, None, :]
    qk = x[:, :, :2]
    rot = torch.cat([-qk[..., hd // 2:], qk[..., :hd // 2]], -1)
    return torch.cat([qk * c + rot * s, x[:, :, 2:]], 2).reshape(B * Lt, 3, H, hd)


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("Lt", [1, 70])
@pytest.mark.parametrize("hd", [32, 128])
def test_mbert_rope(gpu, prec, Lt, hd):
    """In place on the q and k segments; B = 2 so that the position is m % Lt; H = 3, hd = 128 makes the 256-thread loop iterate
    (384 pairs per segment kind).  The tables are random [Lt + 3, hd], so the two halves of a row differ - the kernel reads both - and a
    half swap, a cos / sin swap or a wrong row lands on other values.  v comes back with the same bits, and so does the guard row."""
    B, H = 2, 3
    M = B * Lt
    dt = _act(prec)
    x = _mk((M + 1, 3, H, hd), 200 + Lt + hd)
    cos, sin = _mk((Lt + 3, hd), 201), _mk((Lt + 3, hd), 202)
    xd, cd, sd = _dev(x, gpu, dt), _dev(cos, gpu), _dev(sin, gpu)
    _ok(prec, _lib(prec).samaudio_op_mbert_rope(hip.ptr(xd), hip.ptr(cd), hip.ptr(sd), _code(prec), M, Lt, H, hd, util.stream()))
    got = xd.cpu()
    assert _same_bits(got[M], x[M].to(dt)), "the row behind the last was changed"
    assert _same_bits(got[:M, 2], x[:M, 2].to(dt)), "the v segment was changed"
    seen = _rnd(x[:M], prec)
    want = _rotate_half_stmt(seen, cos, sin, B, Lt, H, hd, torch.float64)
    f32 = _rotate_half_stmt(seen, cos, sin, B, Lt, H, hd, torch.float32)
    _cmp(f"mbert_rope {prec} Lt={Lt} hd={hd}", got[:M, :2], want[:, :2], f32[:, :2], dt)


def _geglu_stmt(x, F, dtype):
    x = x.to(dtype)
    a, g = x[:, :F], x[:, F:]
    return 0.5 * a * (1 + torch.erf(a * (2.0 ** -0.5))) * g


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("M,F", [(3, 7), (5, 96), (129, 8200)])
def test_geglu(gpu, prec, M, F):
    """erf-form GELU of the first F columns times the gate in the last F; odd F, and M F > 4096 x 256 so that the grid-stride loop
    iterates.  The inputs hold 0, +-10, large negatives (GELU -> -0) and a spread around 0 beside the normal values."""
    dt = _act(prec)
    x = _mk((M, 2 * F), 210 + M, 2.0)
    special = torch.tensor([0.0, 10.0, -10.0, -40.0, -1e4, 1e-3, -1e-3])
    x[0, :7] = special
    x[M - 1, F - 7:F] = special.flip(0)
    x[M // 2, :F] = torch.linspace(-6, 6, F)
    xd = _dev(x, gpu, dt)
    out = _nan((M + 1, F), dt, gpu)
    _ok(prec, _lib(prec).samaudio_op_geglu(hip.ptr(xd), hip.ptr(out), _code(prec), M, F, util.stream()))
    o = out.cpu()
    assert _all_nan(o[M]), "the row behind the output was written"
    seen = _rnd(x, prec)
    _cmp(f"geglu {prec} M={M} F={F}", o[:M], _geglu_stmt(seen, F, torch.float64), _geglu_stmt(seen, F, torch.float32), dt)


# ---------------------------------------------------------------------------------------------------------------------
# PE-Core vision tower: rope2d_split, pool_attention, l2_normalize, token_mean
# ---------------------------------------------------------------------------------------------------------------------
def _rope2d_stmt(qkv, rc, rs, n, T, H, hd, dtype):
    """qkv [n * T, 3, H, hd] -> Q, K [n, H, T, hd] (adjacent pairs rotated by rc / rs [T, hd / 2]; None: as they are), V^T [n, H, hd, T]"""
    x = qkv.to(dtype).view(n, T, 3, H, hd).permute(2, 0, 3, 1, 4)   # [3, n, H, T, hd]
    out = []
    for z in (x[0], x[1]):
        if rc is not None:
            c, s = rc.to(dtype)[None, None], rs.to(dtype)[None, None]
            z0, z1 = z[..., 0::2], z[..., 1::2]
            z = torch.stack([z0 * c - z1 * s, z0 * s + z1 * c], -1).reshape(z.shape)
        out.append(z)
    return out[0], out[1], x[2].transpose(-1, -2)


def _rope2d_launch(gpu, prec, dt, qkv, rc, rs, n, T, Tp, H, hd):
    q, k, vt = _nan((n + 1, H, Tp, hd), dt, gpu), _nan((n + 1, H, Tp, hd), dt, gpu), _nan((n + 1, H, hd, Tp), dt, gpu)
    xd = _dev(qkv, gpu, dt)
    cd, sd = (_dev(rc, gpu), _dev(rs, gpu)) if rc is not None else (None, None)
    _ok(prec, _lib(prec).samaudio_op_rope2d_split(hip.ptr(xd), hip.ptr(cd), hip.ptr(sd), hip.ptr(q), hip.ptr(k), hip.ptr(vt),
                                                  hip.F32 if dt == torch.float32 else hip.BF16, n, T, Tp, H, hd, util.stream()))
    return q.cpu(), k.cpu(), vt.cpu()


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("T,Tp", [(1, 64), (64, 64), (65, 128), (70, 192)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("tables", [True, False])
def test_rope2d_split(gpu, prec, T, Tp, hd, tables):
    """The generic kernel (fp32) and the 16-byte fast path (16-bit) at both head widths, with the rotation and as a plain split: T = 1,
    a full block, one token into the second block, and a whole block of padding (70 of 192).  Q / K rows and V^T columns T .. Tp are
    bit-zero, the slab behind the last item stays NaN, V^T - and Q, K without tables - carry the input's bits.  16-bit: the fast path
    is also held against the generic kernel's own fp32 output on the same (rounded) data."""
    n, H = 2, 2
    dt = _act(prec)
    qkv = _mk((n * T, 3, H, hd), 300 + T + hd)
    rc, rs = (_mk((T, hd // 2), 301), _mk((T, hd // 2), 302)) if tables else (None, None)
    q, k, vt = _rope2d_launch(gpu, prec, dt, qkv, rc, rs, n, T, Tp, H, hd)
    tag = f"rope2d_split {prec} hd={hd} T={T} Tp={Tp} {'rotated' if tables else 'plain'}"
    assert _all_nan(q[n]) and _all_nan(k[n]) and _all_nan(vt[n]), "the slab behind the last item was written"
    assert _bit_zero(q[:n, :, T:]) and _bit_zero(k[:n, :, T:]) and _bit_zero(vt[:n, :, :, T:]), "padding must be bit-zero"
    seen = _rnd(qkv, prec)
    wq, wk, wv = _rope2d_stmt(seen, rc, rs, n, T, H, hd, torch.float64)
    fq, fk, _ = _rope2d_stmt(seen, rc, rs, n, T, H, hd, torch.float32)
    assert _same_bits(vt[:n, :, :, :T], wv.to(dt)), "V^T is not the input's bits"
    if tables:
        _cmp(f"{tag} q", q[:n, :, :T], wq, fq, dt)
        _cmp(f"{tag} k", k[:n, :, :T], wk, fk, dt)
    else:
        assert _same_bits(q[:n, :, :T], wq.to(dt)) and _same_bits(k[:n, :, :T], wk.to(dt)), "Q / K without tables are not the input's bits"
    if prec != "fp32":
        gq, gk, gvt = _rope2d_launch(gpu, prec, torch.float32, seen.float(), rc, rs, n, T, Tp, H, hd)
        assert _same_bits(vt[:n], gvt[:n].to(dt)), "fast path V^T != generic kernel's"
        if tables:   # the same bound as against float64, around the generic kernel's output: f32 = reference + the float32 statement's error

            _cmp(f"{tag} q against the generic kernel", q[:n, :, :T], gq[:n, :, :T], fq.double() - wq + gq[:n, :, :T].double(), dt)
            _cmp(f"{tag} k against the generic kernel", k[:n, :, :T], gk[:n, :, :T], fk.double() - wk + gk[:n, :, :T].double(), dt)
        else:
            assert _same_bits(q[:n], gq[:n].to(dt)) and _same_bits(k[:n], gk[:n].to(dt)), "fast path Q / K != generic kernel's"


def _pool_stmt(q, kv, n, T, H, hd, dtype):
    q, kv = q.to(dtype).view(H, hd), kv.to(dtype).view(n, T, 2, H, hd)
    s = torch.einsum("hd,nthd->nht", q, kv[:, :, 0]) * hd ** -0.5
    return torch.einsum("nht,nthd->nhd", torch.softmax(s, -1), kv[:, :, 1]).reshape(n, H * hd)


def _pool_case(order, n, T, H, hd, seed):
    """q and kv whose scores run over t as `order` says: "rising" from -60 to 60 (every step of the online softmax rescales), "falling"
    (the maximum at t = 0, never moved), "random" (plain normal data: many tokens carry weight)"""
    q, kv = _mk((H, hd), seed), _mk((n, T, 2, H, hd), seed + 1)
    if order != "random":
        a = torch.linspace(-60, 60, T) if T > 1 else torch.tensor([60.0])
        if order == "falling":
            a = a.flip(0)
        unit = q * math.sqrt(hd) / (q * q).sum(-1, keepdim=True)   # q_h . unit_h hd^-0.5 = 1
        kv[:, :, 0] = 0.05 * kv[:, :, 0] + a[None, :, None, None] * unit[None, None]
    return q.reshape(-1), kv.reshape(n * T, 2 * H * hd)


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("T", [1, 3, 4, 5, 70])
@pytest.mark.parametrize("hd", [64, 128])
def test_pool_attention(gpu, prec, T, hd):
    """One fp32 query per head over T tokens of (k | v) in every storage type; four waves take tokens w, w + 4, ... with an online
    softmax and merge through LDS.  T < 4 leaves waves without a token (state m = -inf, l = 0), T = 5 gives wave 0 two and the others
    one, T = 70 many.  Scores reach +-60, rising with t, falling from t = 0, and unordered."""
    n, H = 2, 3
    dt = _act(prec)
    for i, order in enumerate(("rising", "falling", "random")):
        q, kv = _pool_case(order, n, T, H, hd, 400 + 10 * T + hd + i)
        qd, kd = _dev(q, gpu), _dev(kv, gpu, dt)
        out = _nan((n + 1, H * hd), dt, gpu)
        _ok(prec, _lib(prec).samaudio_op_pool_attention(hip.ptr(qd), hip.ptr(kd), hip.ptr(out), _code(prec), n, T, H, hd, util.stream()))
        o = out.cpu()
        assert _all_nan(o[n]), "the row behind the output was written"
        seen = _rnd(kv, prec)
        _cmp(f"pool_attention {prec} hd={hd} T={T} {order}", o[:n], _pool_stmt(q, seen, n, T, H, hd, torch.float64),
             _pool_stmt(q, seen, n, T, H, hd, torch.float32), dt)


def _l2_stmt(x, dtype):
    x = x.to(dtype)
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", [64, 100, 1024])
def test_l2_normalize(gpu, rows, D):
    """In place, one wave per row, four rows per workgroup (5 rows: a second workgroup with one live wave); D below, off and above the
    64-lane stride.  Row norms near 1e-3 and 1e3; with 5 rows, row 2 is all zero and stays zero bit for bit."""
    x = _mk((rows + 1, D), 500 + rows + D)
    x[:rows] *= torch.tensor([1e3, 1e-3, 1.0, 1e-3, 1e3])[:rows, None] / math.sqrt(D)
    if rows > 2:
        x[2] = 0
    xd = _dev(x, gpu)
    _ok("fp32", _lib("fp32").samaudio_op_l2_normalize(hip.ptr(xd), rows, D, util.stream()))
    got = xd.cpu()
    assert _same_bits(got[rows], x[rows]), "the row behind the last was changed"
    if rows > 2:
        assert _bit_zero(got[2]), "the all-zero row must stay zero"
    _cmp(f"l2_normalize rows={rows} D={D}", got[:rows], _l2_stmt(x[:rows], torch.float64), _l2_stmt(x[:rows], torch.float32))


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("D", [100, 260])
def test_token_mean(gpu, prec, T, D):
    """Mean over the T tokens of each item, rows of stride D + 12 whose last 12 columns hold NaN (never read); D = 260 makes the
    256-thread loop iterate.  The three output forms: fp32 only, the storage type only, both - and with both, the storage-type output
    is the fp32 output's value rounded, bit for bit."""
    n, ld = 2, D + 12
    dt = _act(prec)
    x = torch.full((n * T, ld), NAN)
    x[:, :D] = _mk((n * T, D), 600 + T + D)
    xd = _dev(x, gpu)
    want = x[:, :D].double().reshape(n, T, D).mean(1)
    f32 = x[:, :D].reshape(n, T, D).mean(1)
    outs = {}
    for form in ("f32", "act", "both"):
        o32 = _nan((n + 1, D), torch.float32, gpu) if form != "act" else None
        oact = _nan((n + 1, D), dt, gpu) if form != "f32" else None
        _ok(prec, _lib(prec).samaudio_op_token_mean(hip.ptr(xd), ld, hip.ptr(o32), hip.ptr(oact), _code(prec), n, T, D, util.stream()))
        for o, odt, what in ((o32, torch.float32, "fp32"), (oact, dt, "storage-type")):
            if o is None:
                continue
            o = o.cpu()
            assert _all_nan(o[n]), f"the row behind the {what} output was written"
            _cmp(f"token_mean {prec} T={T} D={D} {form}: {what} output", o[:n], want, f32, odt)
            outs[form, what] = o[:n]
    assert _same_bits(outs["both", "storage-type"], outs["both", "fp32"].to(dt)), "out_act != the rounded out_f32"
    assert _same_bits(outs["both", "fp32"], outs["f32", "fp32"]) and _same_bits(outs["both", "storage-type"], outs["act", "storage-type"])


# ---------------------------------------------------------------------------------------------------------------------
# PE-AV Judge and span predictor: peav_cls_mask, judge_pool_head, frame_logits (the launcher emulation has these three)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 300])
@pytest.mark.parametrize("with_pad", [False, True])
def test_peav_cls_mask(gpu, T, with_pad):
    """Copies only: the class-token row of every item is cls bit for bit and rows 1 .. T stay NaN; mask_s[b][0] = pad[b][0] != 0 and
    mask_s[b][1 + t] = pad[b][t] != 0 with pad bytes 0, 1 and 255 (all 1 without pad); T + 1 = 301 makes the 256-thread loop iterate.
    The item behind the last keeps its NaN rows and its 0xEE mask bytes."""
    B, D, S = 2, 8, T + 1
    cls = _mk((D,), 700)
    pad = torch.tensor([0, 1, 255], dtype=torch.uint8)[torch.randint(0, 3, (B, T), generator=torch.Generator().manual_seed(701 + T))]
    pad[0, 0], pad[1, 0] = 0, 255
    h = _nan((B + 1, S, D), torch.float32, gpu)
    ms = torch.full((B + 1, S), 0xEE, dtype=torch.uint8, device=gpu)
    cd, pd = _dev(cls, gpu), (_dev(pad, gpu) if with_pad else None)
    _ok("fp32", _lib("fp32").samaudio_op_peav_cls_mask(hip.ptr(h), hip.ptr(cd), hip.ptr(pd), hip.ptr(ms), B, T, D, util.stream()))
    h, ms = h.cpu(), ms.cpu()
    for b in range(B):
        assert _same_bits(h[b, 0], cls), f"item {b}: the class-token row is not cls"
    assert _all_nan(h[:B, 1:]) and _all_nan(h[B]), "rows other than the class token's were written"
    want = torch.cat([pad[:, :1], pad], 1).ne(0).to(torch.uint8) if with_pad else torch.ones(B, S, dtype=torch.uint8)
    assert torch.equal(ms[:B], want), "mask_s"
    assert bool((ms[B] == 0xEE).all()), "the mask row behind the last item was written"


def _judge_stmt(hidden, valid, head_w, mean, std, dtype):
    """hidden [B, T + 1, D], valid [B, T] bool -> (mean over the valid frames of hidden[:, 1:]) . head_w^T * std + mean"""
    hdn, m = hidden.to(dtype)[:, 1:], valid.to(dtype)[..., None]
    pooled = torch.where(valid[..., None], hdn, torch.zeros((), dtype=dtype)).sum(1) / m.sum(1).clamp_min(1)
    return pooled @ head_w.to(dtype).T * std.to(dtype) + mean.to(dtype)


@pytest.mark.parametrize("T", [1, 9])
@pytest.mark.parametrize("D", [64, 260, 4096])
def test_judge_pool_head(gpu, T, D):
    """Masked mean over the frames, then the 4-row head: D below and off the 256-thread stride and at the LDS limit 4096.  Item 0 has
    holes (T = 9: frames 0, 3, 8), item 1 no valid frame - its scores are exactly `mean` - item 2 every frame.  The class-token row and
    every masked frame hold 1e30 (finite: a kernel that adds them fails, one that multiplies by the mask does not), and mask_s[:, 0]
    is (0, 1, 1): it must not matter, although item 1's says "valid"."""
    B, S = 3, T + 1
    hidden = _mk((B, S, D), 800 + T + D)
    valid = torch.ones(B, T, dtype=torch.bool)
    valid[1] = False
    if T > 1:
        valid[0, [0, 3, 8]] = False
    hidden[:, 0] = 1e30
    hidden[:, 1:][~valid] = 1e30
    mask_s = torch.cat([torch.tensor([[0], [1], [1]], dtype=torch.uint8), valid.to(torch.uint8) * torch.tensor([[1], [1], [255]], dtype=torch.uint8)], 1)
    head_w, mean, std = _mk((4, D), 801, D ** -0.5), _mk((4,), 802), _mk((4,), 803).abs() + 0.5
    out = _nan((B + 1, 4), torch.float32, gpu)
    hd_, md, wd, mn, sd = _dev(hidden, gpu), _dev(mask_s, gpu), _dev(head_w, gpu), _dev(mean, gpu), _dev(std, gpu)
    _ok("fp32", _lib("fp32").samaudio_op_judge_pool_head(hip.ptr(hd_), hip.ptr(md), hip.ptr(wd), hip.ptr(mn), hip.ptr(sd), hip.ptr(out),
                                                         B, T, D, util.stream()))
    o = out.cpu()
    assert _all_nan(o[B]), "the row behind the output was written"
    assert _same_bits(o[1], mean), "an item without a valid frame must score exactly `mean`"
    _cmp(f"judge_pool_head T={T} D={D}", o[:B], _judge_stmt(hidden, valid, head_w, mean, std, torch.float64),
         _judge_stmt(hidden, valid, head_w, mean, std, torch.float32))


def _logits_stmt(audio, text, scale, bias, dtype):
    return torch.einsum("bte,be->bt", audio.to(dtype), text.to(dtype)) * scale.to(dtype) + bias.to(dtype)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("E", [4, 260])
def test_frame_logits(gpu, T, E):
    """One wave per (item, frame), four per workgroup: B T = 3 and 15 leave the last workgroup with idle waves; E = 4 is one float4 on
    one lane, E = 260 makes the 64-lane loop iterate with a ragged end.  The audio rows sit at a_off = 4 inside items of stride
    T E + 8 whose gaps hold NaN, so a dropped offset or a dense stride reads NaN; scale and bias are device scalars."""
    B = 3
    a_off, a_bstride = 4, T * E + 8
    audio, text = _mk((B, T, E), 900 + T + E), _mk((B, E), 901)
    scale, bias = torch.tensor([1.7]), torch.tensor([-0.4])
    buf = torch.full((B, a_bstride), NAN)
    buf[:, a_off:a_off + T * E] = audio.reshape(B, T * E)
    out = _nan((B * T + 4,), torch.float32, gpu)
    ad, td, sd, bd = _dev(buf, gpu), _dev(text, gpu), _dev(scale, gpu), _dev(bias, gpu)
    _ok("fp32", _lib("fp32").samaudio_op_frame_logits(hip.ptr(ad), a_bstride, a_off, hip.ptr(td), hip.ptr(sd), hip.ptr(bd), hip.ptr(out),
                                                      B, T, E, util.stream()))
    o = out.cpu()
    assert _all_nan(o[B * T:]), "values behind the output were written"
    _cmp(f"frame_logits T={T} E={E}", o[:B * T].view(B, T), _logits_stmt(audio, text, scale, bias, torch.float64),
         _logits_stmt(audio, text, scale, bias, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# what the hooks refuse
# ---------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_the_kernels_do_not_cover(gpu):
    """Every refusal of the ten hooks, each on otherwise valid arguments (real buffers, so that the named reason is the only one) and by
    its message; nothing is launched.  The argument checks come before the "not in this build" answer, so this runs on every library."""
    lib = _lib("bf16")
    st = util.stream()
    f32 = _dev(torch.zeros(4096), gpu)
    h16 = _dev(torch.zeros(4096), gpu, torch.bfloat16)
    u8 = _dev(torch.ones(64, dtype=torch.uint8), gpu)
    F, H, z = hip.ptr(f32), hip.ptr(h16), C.c_void_p(0)

    def refused(rc, why):
        msg = lib.samaudio_last_error().decode()
        assert rc == hip.ERR_ARG and why in msg, (rc, why, msg)

    # tower attention: B = 1, Lt = 4, H = 1, dkv = 8, max_len = 4 is fine
    attn = lambda qkv=F, mask=hip.ptr(u8), bias=F, out=F, Lt=4, dkv=8, max_len=4: lib.samaudio_op_tower_attention(
        qkv, mask, bias, out, hip.F32, 1, Lt, 1, dkv, max_len, 1.0, 0, st)
    refused(attn(Lt=0), "tokens outside [1, 512]")
    refused(attn(Lt=513, max_len=513), "tokens outside [1, 512]")
    refused(attn(dkv=129), "head_dim outside [1, 128]")
    refused(attn(max_len=3), "max_len < tokens")
    for null in ("qkv", "mask", "out"):
        refused(attn(**{null: z}), "null qkv / mask / out")
    refused(lib.samaudio_op_mbert_rope(F, F, F, hip.F32, 2, 2, 1, 7, st), "odd head_dim")
    split = lambda qkv=H, q=H, k=H, vt=H, prec=hip.BF16, T=1, Tp=64, hd=64: lib.samaudio_op_rope2d_split(
        qkv, z, z, q, k, vt, prec, 1, T, Tp, 1, hd, st)
    refused(split(hd=32), "head_dim")
    refused(split(Tp=65), "tokens_padded")
    refused(split(T=65, Tp=64), "tokens_padded")
    for arg in ("qkv", "q", "k", "vt"):
        refused(split(**{arg: _at(h16, 2)}), "aligned to 16 bytes")
    refused(lib.samaudio_op_pool_attention(F, F, F, hip.F32, 1, 1, 1, 32, st), "head_dim")
    refused(lib.samaudio_op_pool_attention(F, F, F, hip.F32, 1, 0, 1, 64, st), "tokens < 1")
    refused(lib.samaudio_op_judge_pool_head(F, hip.ptr(u8), F, F, F, F, 1, 1, 4100, st), "dim outside [1, 4096]")
    logits = lambda E=4, a_off=0, a_bstride=4: lib.samaudio_op_frame_logits(F, a_bstride, a_off, F, F, F, F, 1, 1, E, st)
    refused(logits(E=6), "embed_dim % 4")
    refused(logits(a_off=2), "a_off % 4")
    refused(logits(a_bstride=6), "a_bstride % 4")
    refused(lib.samaudio_op_token_mean(F, 8, z, z, hip.F32, 1, 1, 8, st), "both outputs null")
