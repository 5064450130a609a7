"""Kernel-level parity of the kernels a DiT layer launches today (csrc/engine.hip Engine::forward), one C-ABI hook each:

    mod_tables + rmsnorm_gs (plain, alt-16 and split [lo | hi | hi] outputs)     samaudio_op_mod_tables / _rmsnorm_gs
    qkv_prep at head_dim 64 / 128 and its fp32 fast path of the compensated mode samaudio_op_qkv_prep_hd
    self_attn_{f32,bf16,x3}_kernel at head_dim 64 / 128, OUT_ALT and OUT3        samaudio_op_self_attention_hd
    headnorm + cross_attn_kernel / cross_attn_mfma_kernel, kv_ld > 2 D           samaudio_op_cross_attention_hd
    cross_attn_probs_kernel, cross_attn_probs3_kernel<8 | 16>                    samaudio_op_cross_attn_probs / _probs3
    cross_attn_fold3_kernel                                                      samaudio_op_cross_attn_fold3

Every reference is float64 torch on the CPU.  A 16-bit kernel's reference is fed the inputs rounded to the operand type, so the
bound measures the kernel and not the format.  Every output buffer starts as NaN and carries a guard row (or batch item) behind
the part the kernel owns: padding that must be zero is asserted to be zero, what must stay untouched to still be NaN.  The bounds
are the sibling tests' (tests/test_kernels_gpu.py, tests/test_x3_gpu.py: same data scale) or follow from the number formats;
where one is derived, the test's docstring says how.

On the CPU the file runs on the functional SIMT simulator (SAMAUDIO_EMU_DRYRUN=simt: bfloat16 library only, so the fp16 / fp16x3
cases are hardware only).  The launcher emulation (SAMAUDIO_EMU_DRYRUN=1) has no 64-wide heads and none of the folded
cross-attention kernels: those tests skip there.
"""
import ctypes as C
import math
import os

import pytest
import torch

from oracle import samaudio_oracle as O
from sam_audio_amd import hip
from tests import util

pytestmark = pytest.mark.gpu
EMU_MODE = os.environ.get("SAMAUDIO_EMU_DRYRUN", "")
SIM = EMU_MODE != ""
LAUNCHER_EMU = EMU_MODE == "1"
S16 = ["bf16"] if SIM else ["bf16", "fp16"]          # the 16-bit kernels, per library
STORAGE = ["fp32"] + S16                            # kernels templated on the activation type
X3 = ["bf16x3"] if SIM else ["fp16x3", "bf16x3"]    # fp32 tensors, compensated 16-bit operands
NAN = float("nan")
EPS = 1e-5


def _lib(prec):
    return hip.lib(hip.operands_for(prec))


def _code(prec):
    return hip.precision_code(prec)


def _act(prec):
    return hip.act_dtype(prec)


def _rnd(x, prec):
    """what a kernel of this precision sees of an fp32 host tensor, as float64"""
    return x.to(_act(prec)).double()


def _mk(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _nan(shape, dtype, gpu):
    return torch.full(shape, NAN, dtype=dtype, device=gpu)


def _dev(x, gpu, dtype=None):
    return x.to(gpu, dtype).contiguous() if dtype is not None else x.to(gpu).contiguous()


def _at(t):
    return C.c_void_p(t.data_ptr())


def _no_launcher_emu(what):
    if LAUNCHER_EMU:
        pytest.skip(f"the launcher emulation has no {what}")


def _err(name, got, want, tol):
    """print the max-abs error next to its bound, then assert; `got` may hold NaN only if that is an error"""
    err = (got.double().cpu() - want).abs().max().item()
    print(f"{name}: max-abs err {err:.3e} (bound {tol:.1e}, |ref| <= {want.abs().max().item():.3f})")
    assert err <= tol, f"{name}: {err} > {tol}"   # (NaN fails: the comparison is False)
    return err


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _ulp16(x, dtype):
    """unit in the last place of a 16-bit value's binade (IEEE half: the subnormal quantum below 2^-14)"""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


def _rms64(x, w, eps=EPS):
    x = x.double()
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.double()


# ---------------------------------------------------------------------------------------------------------------------
# norm family
# ---------------------------------------------------------------------------------------------------------------------
B_N, T_N = 3, 37          # rows = B * T: the batch boundaries fall inside a workgroup's four rows
N_NORMS, USED = 3, 1      # three norms in the table, the middle one consumed
OFFS = [(0, 1), (3, 4), (5, 2)]   # (shift_off, scale_off) / D of each norm inside a 6 D time vector


def _norm_case(D, shared_time):
    x = _mk((B_N * T_N, D), 1)
    w = [_mk((D,), 2 + n, 0.1) + 1 for n in range(N_NORMS)]
    tabs = [_mk((2, D), 10 + n, 0.2) for n in range(N_NORMS)]     # (shift_tab, scale_tab) of each norm
    tvec = _mk((1 if shared_time else B_N, 6 * D), 4, 0.2)
    return x, w, tabs, tvec


def _mod_tables(gpu, prec, D, w, tabs, tvec):
    """gs [norm][time][g | s][D] from the kernel, with a guard row of D floats behind it"""
    nt = tvec.shape[0]
    gs = _nan((N_NORMS * nt * 2 + 1, D), torch.float32, gpu)
    wd = [_dev(t, gpu) for t in w]
    td = [_dev(t, gpu) for t in tabs]
    tv = _dev(tvec, gpu)
    ptrs = lambda ts: (C.c_void_p * N_NORMS)(*[t.data_ptr() for t in ts])
    ints = lambda k: (C.c_int * N_NORMS)(*[OFFS[n][k] * D for n in range(N_NORMS)])
    hip.check(_lib(prec).samaudio_op_mod_tables(ptrs(wd), ptrs([t[0] for t in td]), ptrs([t[1] for t in td]), ints(0), ints(1),
                                                N_NORMS, hip.ptr(tv), 6 * D, nt, hip.ptr(gs), D, util.stream()))
    out = gs.cpu()
    del wd, td, tv
    return gs, out


def _gs_ref(D, w, tabs, tvec, n):
    """float64 (g, s) of norm n per time value: g = w (1 + scale_tab + t_scale), s = shift_tab + t_shift"""
    so, co = OFFS[n][0] * D, OFFS[n][1] * D
    scale = tabs[n][1].double()[None] + tvec.double()[:, co:co + D]
    shift = tabs[n][0].double()[None] + tvec.double()[:, so:so + D]
    return w[n].double()[None] * (1 + scale), shift, scale


def _norm_want(D, x, w, tabs, tvec, eps=EPS):
    _, shift, scale = _gs_ref(D, w, tabs, tvec, USED)
    rep = lambda z: z.expand(B_N, -1).repeat_interleave(T_N, 0)
    return _rms64(x, w[USED], eps) * (1 + rep(scale)) + rep(shift)


@pytest.mark.parametrize("lib", S16)
@pytest.mark.parametrize("shared_time", [False, True])
@pytest.mark.parametrize("D", [512, 2816, 3072])
def test_mod_tables(gpu, lib, shared_time, D):
    """mod_tables_kernel is elementwise fp32 - one add and one multiply-add per value - so every g and s sits within 4 fp32 ulp
    of max(1, |want|) of the float64 formula.  Three norms with their own weights, tables and (non-zero) offsets into the time
    vector: a wrong [norm][time] stride or offset lands on another norm's or another clip's values."""
    x, w, tabs, tvec = _norm_case(D, shared_time)
    nt = tvec.shape[0]
    _, gs = _mod_tables(gpu, lib, D, w, tabs, tvec)
    assert _all_nan(gs[-1]), "the row behind the table was written"
    gs = gs[:-1].reshape(N_NORMS, nt, 2, D).double()
    worst = 0.0
    for n in range(N_NORMS):
        g, s, _ = _gs_ref(D, w, tabs, tvec, n)
        for k, want in ((0, g), (1, s)):
            ulp = torch.pow(2.0, torch.floor(torch.log2(want.abs().clamp_min(1.0))) - 23)
            worst = max(worst, ((gs[n, :, k] - want).abs() / ulp).max().item())
    print(f"mod_tables D={D} nt={nt} ({lib} library): worst error {worst:.2f} fp32 ulp of max(1, |want|) (bound 4)")
    assert worst <= 4


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("shared_time", [False, True])
@pytest.mark.parametrize("D", [512, 2816, 3072])
def test_rmsnorm_gs(gpu, prec, shared_time, D):
    """rmsnorm_gs_reg_kernel on the middle norm's slice of the table mod_tables wrote, against rms_norm(x) w (1 + scale) + shift in
    float64: test_rmsnorm_modulate's data and bounds (1e-5 fp32, 4e-2 16-bit).  16-bit libraries also run the alt-16 output of the
    mixed mode: bfloat16 in both libraries, so the same bound.  In the bfloat16 library the two outputs round the same formula to the same
    format, but not always the same fp32 value: hipcc sums the row statistic in another order in the two instantiations (v_fmac chains
    against packed multiplies + adds), 1 / rms can differ in its last bit, and a value next to a rounding boundary then lands on the
    other side (seen on MI355X, not on the simulator).  So: at most one bfloat16 ulp apart."""
    x, w, tabs, tvec = _norm_case(D, shared_time)
    nt, M = tvec.shape[0], B_N * T_N
    gs_d, _ = _mod_tables(gpu, prec, D, w, tabs, tvec)
    gs_n = gs_d.view(-1)[USED * nt * 2 * D:]
    want = _norm_want(D, x, w, tabs, tvec)
    tol = 1e-5 if prec == "fp32" else 4e-2
    xd = _dev(x, gpu)
    outs = {}
    for form in ((0,) if prec == "fp32" else (0, 1)):
        out = _nan((M + 1, D), _act(prec), gpu)
        hip.check(_lib(prec).samaudio_op_rmsnorm_gs(hip.ptr(xd), _at(gs_n), 0 if nt == 1 else 2 * D, hip.ptr(out), _code(prec), form,
                                                    M, D, T_N, EPS, util.stream()))
        o = out.cpu()
        assert _all_nan(o[M]), "the row behind the output was written"
        outs[form] = o[:M].view(torch.bfloat16) if form == 1 else o[:M]
        _err(f"rmsnorm_gs {prec} D={D} nt={nt} form {form}", outs[form], want, tol)
    if 1 in outs and prec == "bf16":   # both are bfloat16 roundings of the row's fp32 values
        differ = int((outs[0].view(torch.int16) != outs[1].view(torch.int16)).sum())
        worst = ((outs[0].double() - outs[1].double()).abs() / _ulp16(outs[0], torch.bfloat16)).max().item()
        print(f"rmsnorm_gs bf16 D={D} nt={nt}: alt-16 and plain output differ in {differ} of {M * D} values, by <= {worst:.1f} bfloat16 ulp (bound 1)")
        assert worst <= 1
    # the kernel it replaced in the layers (still the final norm): how far the re-associated arithmetic sits from it
    old = _nan((M, D), _act(prec), gpu)
    wd, td, tv = _dev(w[USED], gpu), _dev(tabs[USED], gpu), _dev(tvec, gpu)
    hip.check(_lib(prec).samaudio_op_rmsnorm_mod(hip.ptr(xd), hip.ptr(wd), _at(td[0]), _at(td[1]), hip.ptr(tv), 0 if nt == 1 else 6 * D,
                                                 OFFS[USED][0] * D, OFFS[USED][1] * D, hip.ptr(old), _code(prec), M, D, T_N, EPS,
                                                 util.stream()))
    print(f"rmsnorm_gs vs rmsnorm_mod {prec} D={D}: max-abs difference {(old.cpu().double() - outs[0].double()).abs().max().item():.3e}")


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("shared_time", [False, True])
@pytest.mark.parametrize("D", [512, 2816, 3072])
def test_rmsnorm_gs_split3(gpu, prec, shared_time, D):
    """rmsnorm_gs_split3_kernel: the row as a compensated operand [lo | hi | hi].  Both hi blocks carry the same bits; hi + lo is the
    fp32 row (bound 1e-5 as above) to the pair's 2^-21 |y| (IEEE half: 11 + 11 significant bits, minus one for lo's sign) or 2^-15 |y|
    (bfloat16: 8 + 8); and lo is a rounding remainder: |lo| <= half a 16-bit ulp of hi (in IEEE half never below the subnormal
    quantum 2^-24, which lo itself is rounded to)."""
    half = hip.half_dtype(prec)
    x, w, tabs, tvec = _norm_case(D, shared_time)
    nt, M = tvec.shape[0], B_N * T_N
    gs_d, _ = _mod_tables(gpu, prec, D, w, tabs, tvec)
    gs_n = gs_d.view(-1)[USED * nt * 2 * D:]
    want = _norm_want(D, x, w, tabs, tvec)
    xd = _dev(x, gpu)
    out = _nan((M + 1, 3 * D), half, gpu)
    hip.check(_lib(prec).samaudio_op_rmsnorm_gs(hip.ptr(xd), _at(gs_n), 0 if nt == 1 else 2 * D, hip.ptr(out), hip.F32, 2, M, D, T_N,
                                                EPS, util.stream()))
    o = out.cpu()
    assert _all_nan(o[M]), "the row behind the output was written"
    lo, hi, hi2 = o[:M, :D], o[:M, D:2 * D], o[:M, 2 * D:]
    assert torch.equal(hi.view(torch.int16), hi2.view(torch.int16)), "the two hi blocks differ"
    rel = 2.0 ** -21 if half == torch.float16 else 2.0 ** -15
    excess = ((hi.double() + lo.double() - want).abs() - (1e-5 + rel * want.abs())).max().item()
    print(f"rmsnorm_gs_split3 {prec} D={D} nt={nt}: max (|hi + lo - want| - (1e-5 + {rel:.1e} |want|)) = {excess:.3e} (bound 0)")
    assert excess <= 0
    room = 0.5 * _ulp16(hi, half)
    if half == torch.float16:
        room = room.clamp_min(2.0 ** -24)
    worst = (lo.double().abs() / room).max().item()
    print(f"rmsnorm_gs_split3 {prec} D={D}: max |lo| / (half a 16-bit ulp of hi) = {worst:.3f} (bound 1)")
    assert worst <= 1


def test_hooks_refuse_what_the_kernels_do_not_cover(gpu):
    lib = _lib("bf16")
    z = C.c_void_p(0)
    assert lib.samaudio_op_rmsnorm_gs(z, z, 0, z, hip.F32, 0, 4, 3076, 4, EPS, z) == hip.ERR_ARG      # D > 3072: rmsnorm_mod's
    assert lib.samaudio_op_rmsnorm_gs(z, z, 0, z, hip.F32, 1, 4, 512, 4, EPS, z) == hip.ERR_ARG       # alt-16 is a 16-bit output
    assert lib.samaudio_op_rmsnorm_gs(z, z, 0, z, hip.BF16, 2, 4, 512, 4, EPS, z) == hip.ERR_ARG      # split belongs to fp32 contexts
    assert lib.samaudio_op_qkv_prep_hd(z, z, z, z, z, z, z, z, hip.F32, 1, 1, 4, 64, 2, 64, EPS, z) == hip.ERR_ARG   # f32x: 128 only
    assert lib.samaudio_op_self_attention_hd(z, z, z, z, z, hip.F32, 1, 1, 4, 64, 2, 64, z) == hip.ERR_ARG           # out_alt: 16-bit only
    assert lib.samaudio_op_self_attention_hd(z, z, z, z, z, hip.BF16, 2, 1, 4, 64, 2, 64, z) == hip.ERR_ARG          # out3: compensated only
    assert lib.samaudio_op_self_attention_hd(z, z, z, z, z, hip.F32, 0, 1, 4, 64, 2, 96, z) == hip.ERR_ARG
    assert lib.samaudio_op_cross_attn_probs3(z, z, z, 1024, z, z, 64, 1, 4, 9, 8, 4, EPS, z) == hip.ERR_ARG          # 9 tokens in 8 slots


# ---------------------------------------------------------------------------------------------------------------------
# qkv_prep
# ---------------------------------------------------------------------------------------------------------------------
def _qkv_want(x, B, T, H, hd, qw, kw, cos, sin, eps=EPS):
    """x float64 [B, T, 3 D] (head-major columns) -> Q, K [B, H, T, hd] and V^T [B, H, hd, T]"""
    D = H * hd
    heads = lambda z: z.reshape(B, T, H, hd).permute(0, 2, 1, 3)
    q = O.apply_rope(_rms64(heads(x[..., :D]), qw, eps), cos.double(), sin.double())
    k = O.apply_rope(_rms64(heads(x[..., D:2 * D]), kw, eps), cos.double(), sin.double())
    return q, k, heads(x[..., 2 * D:]).transpose(2, 3)


@pytest.mark.parametrize("T", [1, 12, 64, 70, 129])
@pytest.mark.parametrize("prec,hd", [(p, hd) for p in STORAGE for hd in (64, 128)] + [("f32x:" + p, 128) for p in X3])
def test_qkv_prep(gpu, prec, T, hd):
    """Per-head RMSNorm + RoPE of q / k and the transposition of v, in the general kernel (both head widths, both types), the 16-byte
    fast path (16-bit, 128) and the fp32 fast path of the compensated mode ("f32x", 128 only) - test_qkv_prep's bounds: 2e-5 fp32,
    4e-2 16-bit, V^T a copy (1e-6).  Q / K rows and V^T columns T .. Tp are the zeros the attention kernels' MFMAs read; the slab
    behind the last batch item stays NaN."""
    f32x = prec.startswith("f32x:")
    lib_prec = prec[5:] if f32x else prec
    prec = "fp32" if f32x else prec
    if hd == 64:
        _no_launcher_emu("64-wide heads")
    B, H = 2, 3
    D, Tp = H * hd, (T + 63) // 64 * 64
    qkv = _mk((B, T, 3 * D), 10 + T)
    qw, kw = _mk((hd,), 11, 0.1) + 1, _mk((hd,), 12, 0.1) + 1
    cos, sin = O.rope_tables(hd, T, 20000.0)   # [T, hd / 2]
    dt = _act(prec)
    q, k, vt = _nan((B + 1, H, Tp, hd), dt, gpu), _nan((B + 1, H, Tp, hd), dt, gpu), _nan((B + 1, H, hd, Tp), dt, gpu)
    xd, qwd, kwd, cd, sd = _dev(qkv, gpu, dt), _dev(qw, gpu), _dev(kw, gpu), _dev(cos, gpu), _dev(sin, gpu)
    hip.check(_lib(lib_prec).samaudio_op_qkv_prep_hd(hip.ptr(xd), hip.ptr(qwd), hip.ptr(kwd), hip.ptr(cd), hip.ptr(sd), hip.ptr(q),
                                                     hip.ptr(k), hip.ptr(vt), _code(prec), 1 if f32x else 0, B, T, Tp, H, hd, EPS,
                                                     util.stream()))
    q, k, vt = q.cpu(), k.cpu(), vt.cpu()
    qr, kr, vr = _qkv_want(_rnd(qkv, prec), B, T, H, hd, qw, kw, cos, sin)
    tol = 2e-5 if prec == "fp32" else 4e-2
    tag = f"qkv_prep {'f32x ' + lib_prec if f32x else prec} hd={hd} T={T}"
    _err(f"{tag} q", q[:B, :, :T], qr, tol)
    _err(f"{tag} k", k[:B, :, :T], kr, tol)
    _err(f"{tag} vt", vt[:B, :, :, :T], vr, 1e-6)
    zero = lambda z: z.numel() == 0 or float(z.float().abs().max()) == 0   # (NaN fails)
    assert zero(q[:B, :, T:]) and zero(k[:B, :, T:]) and zero(vt[:B, :, :, T:]), "padding must be zero"
    assert _all_nan(q[B]) and _all_nan(k[B]) and _all_nan(vt[B]), "the slab behind the last batch item was written"


# ---------------------------------------------------------------------------------------------------------------------
# self-attention
# ---------------------------------------------------------------------------------------------------------------------
ATTN_T = [1, 63, 64, 65, 127, 128, 129, 250, 577]   # Tp % 128 == 0 and != 0: the 128- and the 64-row workgroup; 577 = PE-Core's tokens
MASKS = ["none", "tail", "inside", "first_tile", "last_only"]


def _key_mask(kind, B, T):
    """[B, T] bool, every row with at least one valid key; None where T is too short for the kind (tail: T >= 2, a stretch inside:
    T >= 3, the whole first 64-key tile: T > 64).  The extent differs per batch item."""
    m = torch.ones(B, T, dtype=torch.bool)
    for b in range(B):
        if kind == "tail":
            if T < 2:
                return None
            m[b, T - min(T - 1, 13 + 9 * b):] = False
        elif kind == "inside":
            if T < 3:
                return None
            a = 1 + (T // 3) * b // B
            m[b, a:min(T - 1, a + max(1, T // 4) + 5 * b)] = False
        elif kind == "first_tile":
            if T <= 64:
                return None
            m[b, :min(T - 1, 64 + 3 * b)] = False
        elif kind == "last_only":
            m[b, :T - 1] = False
    return m


def _attn_ref(q, k, v, mask, hd, round_p=None):
    """float64 softmax attention of [B, H, T, hd] tensors -> [B * T, H * hd]"""
    B, H, T, _ = q.shape
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(hd)
    s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    if round_p is not None:
        p = p.to(round_p).double()
    return (p @ v.double()).permute(0, 2, 1, 3).reshape(B * T, H * hd)


def _attn_inputs(T, hd, B=3, H=3):
    g = torch.Generator().manual_seed(20 + T + hd)
    q, k, v = (torch.randn(B, H, T, hd, generator=g) for _ in range(3))
    return q * 1.5, k, v   # (sharpens the softmax a little, as the sibling tests do)


def _attn_launch(gpu, prec, code, form, q, k, v, mask, hd, out_dtype, out_cols):
    """one launch on the padded layout qkv_prep produces (rows / columns T .. Tp zero); returns the output rows and the guard row"""
    B, H, T, _ = q.shape
    Tp = (T + 63) // 64 * 64
    dt = _act(prec)
    pad = lambda z: torch.nn.functional.pad(z, (0, 0, 0, Tp - T))
    qd, kd, vtd = _dev(pad(q), gpu, dt), _dev(pad(k), gpu, dt), _dev(pad(v).transpose(2, 3), gpu, dt)
    md = _dev(mask.to(torch.uint8), gpu)
    out = _nan((B * T + 1, out_cols), out_dtype, gpu)
    hip.check(_lib(prec).samaudio_op_self_attention_hd(hip.ptr(qd), hip.ptr(kd), hip.ptr(vtd), hip.ptr(md), hip.ptr(out), code, form, B, T,
                                                       Tp, H, hd, util.stream()))
    o = out.cpu()
    assert _all_nan(o[B * T]), "the row behind the output was written"
    return o[:B * T]


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("T", ATTN_T)
@pytest.mark.parametrize("hd", [64, 128])
def test_self_attention(gpu, prec, T, hd):
    """self_attn_f32_kernel / self_attn_bf16_kernel<4 | 8, hd> under every mask kind, against float64 softmax attention of the
    (rounded) inputs: test_self_attention's bounds, 2e-5 fp32 and 2e-2 16-bit (P and the output are rounded to 16 bits).  16-bit:
    the OUT_ALT form of the mixed mode as well - bfloat16 rows; in the fp16 library the same fp32 values rounded to the other format
    (half a bfloat16 ulp + half an IEEE-half ulp <= one bfloat16 ulp from the plain output), in the bfloat16 library the same bits.
    One bfloat16 ulp holds where IEEE half is the finer format, |x| >= 2^-14.  Below, half's values are 2^-24 apart whatever their size
    and the plain output is the coarser one (first hardware run: up to 42 bfloat16 ulp apart, only in launches with enough values for
    a few to fall below 6.1e-5): there the distance is held to what the two roundings allow, half a bfloat16 ulp + 2^-25."""
    if hd == 64:
        _no_launcher_emu("64-wide heads")
    q, k, v = _attn_inputs(T, hd)
    B, H = q.shape[:2]
    for kind in MASKS:
        mask = _key_mask(kind, B, T)
        if mask is None:
            continue
        want = _attn_ref(_rnd(q, prec), _rnd(k, prec), _rnd(v, prec), mask, hd)
        out = _attn_launch(gpu, prec, _code(prec), 0, q, k, v, mask, hd, _act(prec), H * hd)
        _err(f"self_attention {prec} hd={hd} T={T} mask={kind}", out, want, 2e-5 if prec == "fp32" else 2e-2)
        if prec == "fp32":
            continue
        alt = _attn_launch(gpu, prec, _code(prec), 1, q, k, v, mask, hd, torch.bfloat16, H * hd)
        _err(f"self_attention {prec} hd={hd} T={T} mask={kind} out_alt", alt, want, 2e-2)
        if prec == "bf16":
            assert torch.equal(alt.view(torch.int16), out.view(torch.int16)), "out_alt = the plain output in the bfloat16 library"
        else:
            ulp = _ulp16(out, torch.bfloat16)
            room = torch.maximum(ulp, 0.5 * ulp + 2.0 ** -25)
            worst = ((alt.double() - out.double()).abs() / room).max().item()
            print(f"self_attention {prec} hd={hd} T={T} mask={kind}: max |alt - plain| / (one bfloat16 ulp; IEEE-half subnormals: half of "
                  f"one + 2^-25) = {worst:.3f} (bound 1; {int((out.double().abs() < 2.0 ** -14).sum())} subnormal values)")
            assert worst <= 1


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("T", ATTN_T)
@pytest.mark.parametrize("hd", [64, 128])
def test_self_attention_compensated(gpu, prec, T, hd):
    """self_attn_x3_kernel<4 | 8, hd> (fp32 tensors, both contractions on hi/lo-split operands) under every mask kind, with
    test_self_attention_on_split_operands' criteria: 2e-5 (IEEE-half halves) / 2e-4 (bfloat16 halves) against float64, and less than
    a tenth of what plain 16-bit operands and probabilities give.  OUT3 - the rows as wo's compensated operand - splits the same fp32
    values: bit-equal to samaudio_op_split3 of the kernel's own fp32 output."""
    if hd == 64:
        _no_launcher_emu("64-wide heads")
    half = hip.half_dtype(prec)
    q, k, v = _attn_inputs(T, hd)
    B, H = q.shape[:2]
    D = H * hd
    for kind in MASKS:
        mask = _key_mask(kind, B, T)
        if mask is None:
            continue
        want = _attn_ref(q, k, v, mask, hd)
        plain = _attn_ref(q.to(half), k.to(half), v.to(half), mask, hd, round_p=half)
        out = _attn_launch(gpu, prec, 2, 0, q, k, v, mask, hd, torch.float32, D)
        e_plain = (plain - want).abs().max().item()
        err = _err(f"self_attention x3 {prec} hd={hd} T={T} mask={kind} (plain 16-bit operands {e_plain:.3e})", out, want,
                   2e-5 if half == torch.float16 else 2e-4)
        assert err < e_plain / 10
        out3 = _attn_launch(gpu, prec, 2, 2, q, k, v, mask, hd, half, 3 * D)
        split = _nan((B * T, 3 * D), half, gpu)
        od = _dev(out, gpu)
        hip.check(_lib(prec).samaudio_op_split3(hip.ptr(od), D, hip.ptr(split), B * T, D, util.stream()))
        assert torch.equal(out3.view(torch.int16), split.cpu().view(torch.int16)), f"OUT3 != split3(out) (mask={kind})"


# ---------------------------------------------------------------------------------------------------------------------
# cross-attention
# ---------------------------------------------------------------------------------------------------------------------
def _text_mask(B, Lt):
    """ragged: every token | two thirds of them, the first masked too where that leaves one | a single valid token"""
    m = torch.zeros(B, Lt, dtype=torch.bool)
    m[0] = True
    n1 = max(1, Lt * 2 // 3)
    m[1, :n1] = True
    if n1 >= 3:
        m[1, 0] = False
    m[2:, min(Lt - 1, 2)] = True
    return m


def _cross_ref(q, k, v, mask, hd, T):
    """q [B * T, D], k / v [B * Lt, D] float64 (q and k normalised) -> probabilities [B, H, T, Lt] and rows [B * T, D]"""
    B, Lt = mask.shape
    H = q.shape[1] // hd
    heads = lambda z, n: z.reshape(B, n, H, hd).permute(0, 2, 1, 3)
    s = (heads(q, T) @ heads(k, Lt).transpose(-1, -2)) / math.sqrt(hd)
    p = torch.softmax(s.masked_fill(~mask[:, None, None, :], float("-inf")), -1)
    return p, (p @ heads(v, Lt)).permute(0, 2, 1, 3).reshape(B * T, H * hd)


def _per_head(x, w, hd):
    return _rms64(x.reshape(*x.shape[:-1], -1, hd), w).reshape(x.shape)


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("Lt", [1, 6, 8, 9, 16, 17, 40])
@pytest.mark.parametrize("hd", [64, 128])
def test_cross_attention(gpu, prec, Lt, hd):
    """headnorm (in place, at the head width) + cross-attention at T = 1 / 40 / 64 / 70 under a ragged text mask: the MFMA form
    (16-bit, <= 16 tokens, 128-wide heads) and the general one-wave-per-(row, head) form (everything else; cross_attn_kernel<bf16, 128>
    from 17 tokens on), each with dense kv rows and with the layer's (k | v) columns inside [Mt, 3 * 2 D] rows as the engine lays them
    out - where the neighbouring layers' columns must come back untouched.  test_cross_attention's bounds: 2e-5 fp32, 2e-2 16-bit."""
    if hd == 64:
        _no_launcher_emu("64-wide heads")
    B, H = 3, 3
    D = H * hd
    mask = _text_mask(B, Lt)
    qw, kw = _mk((hd,), 32, 0.1) + 1, _mk((hd,), 33, 0.1) + 1
    dt = _act(prec)
    tol = 2e-5 if prec == "fp32" else 2e-2
    for T in (1, 40, 64, 70):
        q, kv = _mk((B * T, D), 30 + T), _mk((B * Lt, 3, 2 * D), 31 + T + Lt)
        qq = _per_head(_rnd(q, prec), qw, hd)
        kk = _per_head(_rnd(kv[:, 1, :D], prec), kw, hd)
        kk = kk.to(dt).double()   # the normalised keys are stored back in the activation type
        _, want = _cross_ref(qq, kk, _rnd(kv[:, 1, D:], prec), mask, hd, T)
        for wide in (False, True):
            kv_d = _dev(kv if wide else kv[:, 1], gpu, dt)
            kv_ld = 6 * D if wide else 2 * D
            out = _nan((B * T + 1, D), dt, gpu)
            qd, qwd, kwd, md = _dev(q, gpu, dt), _dev(qw, gpu), _dev(kw, gpu), _dev(mask.to(torch.uint8), gpu)
            hip.check(_lib(prec).samaudio_op_cross_attention_hd(
                hip.ptr(qd), hip.ptr(qwd), _at(kv_d[:, 1]) if wide else hip.ptr(kv_d), kv_ld, hip.ptr(kwd), hip.ptr(md), hip.ptr(out),
                _code(prec), B, T, Lt, H, hd, EPS, util.stream()))
            o, kv_o = out.cpu(), kv_d.cpu()
            assert _all_nan(o[B * T]), "the row behind the output was written"
            tag = f"cross_attention {prec} hd={hd} Lt={Lt} T={T} kv_ld={kv_ld}"
            _err(tag, o[:B * T], want, tol)
            mine = kv_o[:, 1] if wide else kv_o
            _err(f"{tag}: k normalised in place", mine[:, :D], kk, 2e-5 if prec == "fp32" else 4e-2)
            assert torch.equal(mine[:, D:], kv[:, 1, D:].to(dt)), "v changed"
            if wide:
                assert torch.equal(kv_o[:, 0], kv[:, 0].to(dt)) and torch.equal(kv_o[:, 2], kv[:, 2].to(dt)), "a neighbouring layer's columns changed"


# ---------------------------------------------------------------------------------------------------------------------
# folded cross-attention: probabilities, the U operand, and their product
# ---------------------------------------------------------------------------------------------------------------------
PROBS_CASES = [(ltp, Lt, H) for ltp, lts in ((8, (1, 5, 8)), (16, (9, 13, 16))) for Lt in lts for H in (2, 4, 10, 22)]


def _probs_case(Lt, H, B=3, T=70):
    D = H * 128
    q, kv = _mk((B * T, D), 50 + H), _mk((B * Lt, 3, 2 * D), 51 + H + Lt)   # the layer's columns inside [Mt, 3 * 2 D], as in the engine
    qw = _mk((128,), 52, 0.1) + 1
    return D, q, kv, qw, _text_mask(B, Lt)


def _probs_want(p, mask, ltp, kp):
    """[B, H, T, Lt] probabilities -> [B * T, kp] with head h's token j at column h * ltp + j; NaN where nothing is written"""
    B, H, T, Lt = p.shape
    want = torch.zeros(B, T, H, ltp, dtype=torch.float64)
    want[..., :Lt] = p.permute(0, 2, 1, 3)
    full = torch.full((B * T, kp), NAN, dtype=torch.float64)
    full[:, :H * ltp] = want.reshape(B * T, H * ltp)
    return full


def _check_probs_layout(name, got, want, mask, ltp, H, tol):
    """got / want [B * T, kp] float64: exact zeros for masked tokens and for the slots Lt .. ltp, NaN kept in the columns past H * ltp"""
    B, Lt = mask.shape
    T = got.shape[0] // B
    used = got[:, :H * ltp].reshape(B, T, H, ltp)
    assert _all_nan(got[:, H * ltp:]), f"{name}: columns past H * LtP were written"
    assert float(used[..., Lt:].abs().sum()) == 0, f"{name}: slots Lt .. LtP must be zero"   # (NaN fails; an empty slice sums to 0)
    dead = (~mask)[:, None, None, :].expand(B, T, H, Lt)
    assert float(used[..., :Lt][dead].abs().sum()) == 0, f"{name}: masked tokens must be zero"
    _err(name, used, want[:, :H * ltp].reshape(B, T, H, ltp), tol)
    sums = (used.sum(-1) - 1).abs().max().item()
    print(f"{name}: rows sum to 1 within {sums:.3e} (bound {tol:.1e})")
    assert sums <= tol


@pytest.mark.parametrize("prec", S16)
@pytest.mark.parametrize("ltp,Lt,H", PROBS_CASES)
def test_cross_attn_probs(gpu, prec, ltp, Lt, H):
    """cross_attn_probs_kernel (the shipped 16-bit cross-attention for <= 16 text tokens): head h's probability of token j at column
    h * LtP + j.  Read off the kernel: a lane group stores its four slots wherever 4 g < LtP, so masked tokens and the slots
    Lt .. LtP are written as exact zeros, and nothing is written past column H * LtP of the ldp-wide row (those columns meet zeros of
    U in the GEMM; here they must stay NaN).  Bound 2e-2: the project's bound for the 16-bit cross-attention output, a convex
    combination of O(1) values under these weights; the sum over a head's slots is held to the same bound."""
    _no_launcher_emu("folded cross-attention kernels")
    B, T = 3, 70
    D, q, kv, qw, mask = _probs_case(Lt, H, B, T)
    kp = (H * ltp + 63) // 64 * 64
    dt = _act(prec)
    kv_d, qd, qwd, md = _dev(kv, gpu, dt), _dev(q, gpu, dt), _dev(qw, gpu), _dev(mask.to(torch.uint8), gpu)
    P = _nan((B * T + 1, kp), dt, gpu)
    hip.check(_lib(prec).samaudio_op_cross_attn_probs(hip.ptr(qd), hip.ptr(qwd), _at(kv_d[:, 1]), 6 * D, hip.ptr(md), hip.ptr(P), kp, B, T,
                                                      Lt, ltp, H, EPS, util.stream()))
    got = P.cpu().double()
    assert _all_nan(got[B * T]), "the row behind the output was written"
    p, _ = _cross_ref(_per_head(_rnd(q, prec), qw, 128), _rnd(kv[:, 1, :D], prec), _rnd(kv[:, 1, D:], prec), mask, 128, T)
    _check_probs_layout(f"cross_attn_probs {prec} LtP={ltp} Lt={Lt} H={H}", got[:B * T], _probs_want(p, mask, ltp, kp), mask, ltp, H, 2e-2)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("ltp,Lt,H", PROBS_CASES)
def test_cross_attn_probs3(gpu, prec, ltp, Lt, H):
    """cross_attn_probs3_kernel<8 | 16>: the same probabilities from fp32 q / k with the scores on split operands, written as the
    compensated operand [P_lo | P_hi | P_hi] of 3 KP columns.  hi + lo against the float64 softmax <= 2e-5; both hi blocks the same
    bits; and in all three blocks exact zeros where the 16-bit kernel has zeros, nothing written past column H * LtP."""
    _no_launcher_emu("folded cross-attention kernels")
    half = hip.half_dtype(prec)
    B, T = 3, 70
    D, q, kv, qw, mask = _probs_case(Lt, H, B, T)
    kp = (H * ltp + 63) // 64 * 64
    kv_d, qd, qwd, md = _dev(kv, gpu), _dev(q, gpu), _dev(qw, gpu), _dev(mask.to(torch.uint8), gpu)
    P3 = _nan((B * T + 1, 3 * kp), half, gpu)
    hip.check(_lib(prec).samaudio_op_cross_attn_probs3(hip.ptr(qd), hip.ptr(qwd), _at(kv_d[:, 1]), 6 * D, hip.ptr(md), hip.ptr(P3), kp, B,
                                                       T, Lt, ltp, H, EPS, util.stream()))
    got = P3.cpu()
    assert _all_nan(got[B * T]), "the row behind the output was written"
    lo, hi, hi2 = (got[:B * T, i * kp:(i + 1) * kp] for i in range(3))
    assert torch.equal(hi.view(torch.int16), hi2.view(torch.int16)), "the two hi blocks differ"
    p, _ = _cross_ref(_per_head(q.double(), qw, 128), kv[:, 1, :D].double(), kv[:, 1, D:].double(), mask, 128, T)
    want = _probs_want(p, mask, ltp, kp)
    name = f"cross_attn_probs3 {prec} LtP={ltp} Lt={Lt} H={H}"
    _check_probs_layout(name, hi.double() + lo.double(), want, mask, ltp, H, 2e-5)
    zeros = want == 0
    for blk, t in (("lo", lo), ("hi", hi)):
        assert _all_nan(t[:, H * ltp:]), f"{name}: {blk} columns past H * LtP were written"
        assert float(t.double()[zeros].abs().sum()) == 0, f"{name}: {blk} is not zero where the 16-bit kernel has zeros"


FOLD_CASES = [(3, 8, 3, 4), (8, 8, 3, 4), (11, 16, 3, 4), (8, 8, 6, 6), (16, 16, 5, 2), (8, 8, 5, 22), (8, 8, 33, 10), (13, 16, 9, 22),
              (8, 8, 16, 22), (8, 8, 13, 4)]   # test_cross_attn_fold_operand's grid: partial head groups, runs clipped at KP, ragged batch trips


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("Lt,ltp,B,H", FOLD_CASES)
def test_cross_attn_fold3(gpu, prec, Lt, ltp, B, H):
    """cross_attn_fold3_kernel: U = Wo V per (batch item, head, token) from fp32 Wo / V on split operands, written as the per-batch
    weight operand [U_hi | U_lo | U_hi] of 3 KP columns - zeros for the slots Lt .. LtP, for the heads past H of the last 8-head run
    and for the K padding, in all three blocks; the batch item behind the last stays NaN.  test_x3_gemm_is_the_fp32_product's
    criteria: U_hi + U_lo within 2e-5 max|ref| of the float64 product (IEEE-half halves), less than 1/20 of what plain 16-bit
    operands give (bfloat16 halves)."""
    _no_launcher_emu("folded cross-attention kernels")
    half = hip.half_dtype(prec)
    D = H * 128
    kp = (H * ltp + 63) // 64 * 64
    wo, kv = _mk((D, D), 30, 1 / math.sqrt(D)), _mk((B * Lt, 3, 2 * D), 31)
    ut = _nan((B + 1, D, 3 * kp), half, gpu)
    wod, kv_d = _dev(wo, gpu), _dev(kv, gpu)
    hip.check(_lib(prec).samaudio_op_cross_attn_fold3(hip.ptr(wod), _at(kv_d[:, 1]), 6 * D, hip.ptr(ut), kp, B, Lt, ltp, H, util.stream()))
    got = ut.cpu()
    assert _all_nan(got[B]), "the batch item behind the last was written"
    u_hi, u_lo, u_hi2 = (got[:B, :, i * kp:(i + 1) * kp] for i in range(3))
    assert torch.equal(u_hi.view(torch.int16), u_hi2.view(torch.int16)), "[U_hi | U_lo | U_hi]: the outer blocks differ"

    def fold(w, v):
        ref = torch.zeros(B, D, H, ltp, dtype=torch.float64)
        ref[..., :Lt] = torch.einsum("nhd,bjhd->bnhj", w.double().reshape(D, H, 128), v.double().reshape(B, Lt, H, 128))
        full = torch.zeros(B, D, kp, dtype=torch.float64)
        full[:, :, :H * ltp] = ref.reshape(B, D, H * ltp)
        return full

    want = fold(wo, kv[:, 1, D:])
    plain = fold(wo.to(half), kv[:, 1, D:].to(half))
    pad = want == 0
    for blk, t in (("U_hi", u_hi), ("U_lo", u_lo)):
        assert float(t.double()[pad].abs().sum()) == 0, f"{blk}: padding must be zero"   # (NaN fails)
    err = (u_hi.double() + u_lo.double() - want).abs().max().item()
    e_plain, scale = (plain - want).abs().max().item(), want.abs().max().item()
    print(f"cross_attn_fold3 {prec} Lt={Lt} LtP={ltp} B={B} H={H}: max-abs err {err:.3e} (plain 16-bit operands {e_plain:.3e}, "
          f"|ref| <= {scale:.3f}; bound {'2e-5 |ref|' if half == torch.float16 else 'plain / 20'})")
    if half == torch.float16:
        assert err <= 2e-5 * scale
    else:
        assert err < e_plain / 20


@pytest.mark.parametrize("prec", S16 + X3)
def test_folded_cross_attention_is_the_unfolded_one(gpu, prec):
    """P . U^T from the folded pieces equals Wo . cross_attention(...) from the unfolded kernels (both products taken in float64 on the
    CPU from the kernels' outputs), within the sum of the two pieces' bounds: 2e-2 (probabilities) + 2e-2 (test_cross_attn_fold_operand's)
    for the 16-bit kernels, 2e-5 (probs3) + fold3's bound - 2e-5 max|U| on IEEE-half halves, 1/20 of plain 16-bit operands' error in U
    on bfloat16 halves - for the compensated ones."""
    _no_launcher_emu("folded cross-attention kernels")
    x3 = hip.is_x3(prec)
    store = hip.storage_precision(prec)
    half = hip.half_dtype(prec) if x3 else _act(prec)
    B, T, Lt, ltp, H = 3, 40, 6, 8, 4
    D, kp = H * 128, 64
    q, kv, wo = _mk((B * T, D), 60), _mk((B * Lt, 2 * D), 61), _mk((D, D), 62, 1 / math.sqrt(D))
    qw, kw = _mk((128,), 63, 0.1) + 1, _mk((128,), 64, 0.1) + 1
    mask = _text_mask(B, Lt)
    dt = _act(store)
    lib = _lib(prec)
    qd, kv_d, wod, qwd, kwd, md = _dev(q, gpu, dt), _dev(kv, gpu, dt), _dev(wo, gpu, dt), _dev(qw, gpu), _dev(kw, gpu), _dev(mask.to(torch.uint8), gpu)
    ca = _nan((B * T, D), dt, gpu)
    hip.check(lib.samaudio_op_cross_attention_hd(hip.ptr(qd), hip.ptr(qwd), hip.ptr(kv_d), 2 * D, hip.ptr(kwd), hip.ptr(md), hip.ptr(ca),
                                                 _code(store), B, T, Lt, H, 128, EPS, util.stream()))
    # kv_d now holds the normalised keys: what the folded kernels expect
    if x3:
        P3, ut3 = _nan((B * T, 3 * kp), half, gpu), _nan((B, D, 3 * kp), half, gpu)
        hip.check(lib.samaudio_op_cross_attn_probs3(hip.ptr(qd), hip.ptr(qwd), hip.ptr(kv_d), 2 * D, hip.ptr(md), hip.ptr(P3), kp, B, T, Lt, ltp,
                                                    H, EPS, util.stream()))
        hip.check(lib.samaudio_op_cross_attn_fold3(hip.ptr(wod), hip.ptr(kv_d), 2 * D, hip.ptr(ut3), kp, B, Lt, ltp, H, util.stream()))
        P3, ut3 = P3.cpu().double(), ut3.cpu().double()
        P = P3[:, :kp] + P3[:, kp:2 * kp]
        U = ut3[:, :, :kp] + ut3[:, :, kp:2 * kp]
        u_ref = torch.einsum("nhd,bjhd->bnhj", wo.double().reshape(D, H, 128), kv[:, D:].double().reshape(B, Lt, H, 128))
        u_plain = torch.einsum("nhd,bjhd->bnhj", wo.to(half).double().reshape(D, H, 128), kv[:, D:].to(half).double().reshape(B, Lt, H, 128))
        tol = 2e-5 + (2e-5 * u_ref.abs().max().item() if half == torch.float16 else (u_plain - u_ref).abs().max().item() / 20)
    else:
        Pd, utd = _nan((B * T, kp), dt, gpu), _nan((B, D, kp), dt, gpu)
        hip.check(lib.samaudio_op_cross_attn_probs(hip.ptr(qd), hip.ptr(qwd), hip.ptr(kv_d), 2 * D, hip.ptr(md), hip.ptr(Pd), kp, B, T, Lt, ltp, H,
                                                   EPS, util.stream()))
        hip.check(lib.samaudio_op_cross_attn_fold(hip.ptr(wod), hip.ptr(kv_d), 2 * D, hip.ptr(utd), kp, B, Lt, ltp, H, util.stream()))
        P, U = Pd.cpu().double(), utd.cpu().double()
        tol = 2e-2 + 2e-2
    used = H * ltp   # (the columns past it are unwritten in P and zero in U)
    folded = torch.einsum("btk,bnk->btn", P[:, :used].reshape(B, T, used), U[:, :, :used]).reshape(B * T, D)
    unfolded = ca.cpu().double() @ wo.to(dt).double().T
    _err(f"folded vs unfolded cross-attention {prec}", folded, unfolded, tol)
