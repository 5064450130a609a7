"""Every launch form the engine and the towers give the 8-phase kernels on compensated operands (precision "fp16x3" / "bf16x3": A rows
[x_lo | x_hi | x_hi] from samaudio_op_split3, W rows [W_hi | W_lo | W_hi] from weights.x3_weight, K' = 3K), each on its own against
float64 - DESIGN.md section 4.5.

  form 1  wo / w2        gate table + per-item gate (rows_per_gate = T), residual in place, fp32 output       epilogue8_rows
  form 2  w13            SwiGLU, result written as w2's split operand [lo | hi | hi] (GEMM_FLAG_OUT_SPLIT3)     epilogue8_linear
  form 3  w13            SwiGLU with an fp32 output (what host.h x3_operands makes of it when x3_w2_pre declines) general epilogue
  form 4  fold_gemm      batched h += P . U: per-item weight (w_bstride), a_bstride, residual in place, M = T < one tile, K' = 576
  form 5  towers         bias + residual in place, fp32 output
  form 6  cat_audio_proj batched A with a_off != 0 (rows 1 .. T of items of T + 1 rows), one shared weight, bias

Every form runs through samaudio_op_gemm on gemm8x_kernel / gemm8_kernel (GV_GEMM8_256x256) and gemm8s_kernel (GV_GEMM8S_128x128), on the
plain walk over K' and the operand-sharing one (GEMM_FLAG_X3_SHARE), with the weight in rows and K-tile-major.  Asserted per case:

  ownership   outputs start as a NaN sentinel with a guard row (a guard item for batched forms) behind them: every owned element is
              finite afterwards, every guard element untouched; in-place forms start from a fresh copy of h for every launch
  float64     tol_acc = (2e-5 fp16x3 | 1e-4 bf16x3) x max(1, max|acc_ref|): the bounds of test_x3_gemm_is_the_fp32_product and of
              test_fp32_gemm_with_operands_split_on_the_fly (tests/test_x3_gpu.py, the same data recipe).  fp32 outputs element by
              element: |got - want| <= |g| tol_acc + 2^-22 |want| (g: the float64 gate, 1 without one; 2^-22: the fp32 rounding of the
              epilogue's two operations).  SwiGLU: 2 tol_acc x max(1, max|gate-branch accumulator|).  And the max-abs error is at most
              1/200 (fp16x3) | 1/20 (bf16x3) of what the same float64 expression gives on operands rounded to the plain 16-bit type -
              the condition a lost product cannot meet
  invariance  for one walk, both kernels and both weight layouts give the same bits; the sharing walk's error is at most twice the
              plain walk's + 1e-6 max|ref|; with DBG_GEMM8_EPILOGUE = DBG_EPI_GENERAL (and DBG_EPI_LINEAR: the register epilogue with a
              residual) forms 1, 4, 5, 6 give the bits of the shipped epilogue
  split form  form 2's hi blocks are equal and its row is, bit for bit, the split of form 3's fp32 output of the same launch

On the CPU simulator (SAMAUDIO_EMU_DRYRUN=simt: bfloat16 library only) the bf16x3 cases run the same kernels and host code; the
272-tile case (persistent walk, tail split) is hardware only.
"""
import ctypes as C
import os

import pytest
import torch

from sam_audio_amd import hip
from sam_audio_amd.weights import _interleave16, x3_weight
from tests import util

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
X3 = ["bf16x3"] if SIM else ["fp16x3", "bf16x3"]
HALF = {"fp16x3": torch.float16, "bf16x3": torch.bfloat16}
TOL_ACC = {"fp16x3": 2e-5, "bf16x3": 1e-4}
PLAIN_FACTOR = {"fp16x3": 200, "bf16x3": 20}
VARIANTS = (hip.GV_GEMM8_256x256, hip.GV_GEMM8S_128x128)
WALKS = (0, hip.GEMM_FLAG_X3_SHARE)
SENT = 0x7FC5A5A5   # a quiet NaN no kernel produces


def _sentinel(shape, dev, dtype=torch.float32):
    if dtype != torch.float32:
        return torch.full(shape, float("nan"), dtype=dtype, device=dev)
    t = torch.empty(shape, dtype=torch.float32, device=dev)
    t.view(torch.int32).fill_(SENT)
    return t


def _untouched(t):
    return bool((t.view(torch.int32) == SENT).all()) if t.dtype == torch.float32 else bool(torch.isnan(t.float()).all())


def same_bits(a, b):
    v = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


class Form:
    """One GEMM launch, stated on CPU tensors.  x [n, S, K]: items of S rows, of which rows a_row0 .. a_row0 + M - 1 are read;
    w [N, K], or [n, N, K] (one weight per item: w_bstride); swiglu: w = [w1; w3] (2F rows, launched through weights._interleave16);
    gate [M n / T, N] + tab [N]: row r of the flattened [n M] rows is scaled by gate[r // T] + tab; bias [N]; h [n, M, N]: the residual,
    added in place."""

    def __init__(self, name, x, w, M, *, a_row0=0, gate=None, tab=None, T=1, bias=None, h=None, swiglu=False):
        self.name, self.x, self.w, self.M, self.a_row0 = name, x, w, M, a_row0
        self.gate, self.tab, self.T, self.bias, self.h, self.swiglu = gate, tab, T, bias, h, swiglu
        self.n, self.S, self.K = x.shape
        self.N = w.shape[-2]
        self.n_out = self.N // 2 if swiglu else self.N
        self.dev = {}
        self._exp = {}

    def expected(self, half=None):
        """float64 from the fp32 operands, or from operands rounded to `half`: dict(acc [n, M, N], want [n, M, n_out], g, a)"""
        if half not in self._exp:
            xv, wv = (self.x, self.w) if half is None else (self.x.to(half).float(), self.w.to(half).float())
            xv = xv[:, self.a_row0:self.a_row0 + self.M].double()
            acc = torch.einsum("bmk,bnk->bmn", xv, wv.double()) if wv.dim() == 3 else torch.einsum("bmk,nk->bmn", xv, wv.double())
            g = torch.ones(())
            a = None
            if self.swiglu:
                a, up = acc[..., :self.n_out], acc[..., self.n_out:]
                want = a * torch.sigmoid(a) * up
            else:
                want = acc if self.bias is None else acc + self.bias.double()
                if self.gate is not None:
                    rows = torch.arange(self.n * self.M) // self.T
                    g = (self.gate.double() + self.tab.double())[rows].reshape(self.n, self.M, self.N)
                    want = want * g
                if self.h is not None:
                    want = want + self.h.double()
            self._exp[half] = dict(acc=acc, want=want, g=g, a=a)
        return self._exp[half]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _xw(g, n, S, N, K, per_item_w=False):
    """the sibling recipe (tests/test_x3_gpu.py): column scales 1e-2 .. 10 put many lo halves into IEEE half's subnormal range"""
    x = torch.randn(n, S, K, generator=g) * torch.logspace(-2, 1, K)[None, None, :]
    w = torch.randn(*((n, N, K) if per_item_w else (N, K)), generator=g) * 0.05
    return x, w


def form_gated_residual(M, N, K, seed, n=1, T=None):
    """form 1: h += (gate[item] + tab) * (x W^T), items of T rows in ONE launch of M rows (the engine's wo / w2); n > 1: the same as a
    batched launch of n x M rows - the gate row of row m of batch item b is (b M + m) / T"""
    g = _gen(seed)
    items = M // T if T else (3 if M % 3 == 0 else 1)
    x, w = _xw(g, n, M, N, K)
    return Form(f"gated in-place residual{f' n {n}' if n > 1 else ''} ({M}, {N}, {K}) T {M // items}", x, w, M,
                gate=torch.randn(n * items, N, generator=g), tab=torch.randn(N, generator=g), T=M // items,
                h=torch.randn(n, M, N, generator=g))


def form_swiglu(M, F, K, seed):
    """forms 2 / 3: silu(x W1^T) * (x W3^T)"""
    g = _gen(seed)
    x, w = _xw(g, 1, M, 2 * F, K)
    return Form(f"SwiGLU ({M}, 2 x {F}, {K})", x, w, M, swiglu=True)


def form_fold(n, T, N, K, seed):
    """form 4: h[i] += P[i] U[i]^T, one weight per item"""
    g = _gen(seed)
    x, w = _xw(g, n, T, N, K, per_item_w=True)
    return Form(f"batched fold n {n} ({T}, {N}, {K})", x, w, T, h=torch.randn(n, T, N, generator=g))


def form_bias_residual(M, N, K, seed):
    """form 5: h += x W^T + bias (the towers' out_proj / c_proj)"""
    g = _gen(seed)
    x, w = _xw(g, 1, M, N, K)
    return Form(f"bias + in-place residual ({M}, {N}, {K})", x, w, M, bias=torch.randn(N, generator=g) * 0.1,
                h=torch.randn(1, M, N, generator=g))


def form_cat_proj(n, S, N, K, seed):
    """form 6: rows 1 .. S - 1 of n items of S rows against one weight, + bias (the Judge's cat_audio_proj)"""
    g = _gen(seed)
    x, w = _xw(g, n, S, N, K)
    return Form(f"batched rows 1.. n {n} ({S - 1} of {S}, {N}, {K})", x, w, S - 1, a_row0=1, bias=torch.randn(N, generator=g) * 0.1)


def _operands(f: Form, prec, gpu):
    """device copies shared by every launch of (form, precision): A split by samaudio_op_split3, W by weights.x3_weight"""
    if prec not in f.dev:
        lib, half = hip.lib(hip.operands_for(prec)), HALF[prec]
        xd = f.x.reshape(f.n * f.S, f.K).to(gpu).contiguous()
        a3 = torch.empty(f.n * f.S, 3 * f.K, dtype=half, device=gpu)
        hip.check(lib.samaudio_op_split3(hip.ptr(xd), f.K, hip.ptr(a3), f.n * f.S, f.K, util.stream()))
        w = _interleave16(f.w[:f.n_out], f.w[f.n_out:]) if f.swiglu else f.w
        d = dict(a3=a3)
        if w.dim() == 3:
            d[False] = torch.stack([x3_weight(w[i], half, ktm=False) for i in range(f.n)]).to(gpu).contiguous()
        else:
            d[False], d[True] = x3_weight(w, half, ktm=False).to(gpu), x3_weight(w, half, ktm=True).to(gpu)
        for k in ("tab", "bias"):
            d[k] = None if getattr(f, k) is None else getattr(f, k).to(gpu)
        if f.gate is not None:   # as the engine's t0: the gate is a column block of wider rows
            wide = torch.randn(f.gate.shape[0], 2 * f.N, generator=_gen(99))
            wide[:, f.N:] = f.gate
            d["gate_wide"] = wide.to(gpu)
        f.dev[prec] = d
    return f.dev[prec]


def params(f: Form, prec, gpu, flags, *, ktm=False, out="f32", prefetch=None):
    """(GemmParams, output buffer, tensors to keep alive) of one launch of `f`; out: "f32" | "split3" (form 2)"""
    d = _operands(f, prec, gpu)
    K3, n, M = 3 * f.K, f.n, f.M
    kw = {}
    if f.gate is not None:
        kw.update(gate_tab=d["tab"], gate=d["gate_wide"][:, f.N:], gate_ld=2 * f.N, rows_per_gate=f.T)
    if out == "split3":
        buf = _sentinel((M + 1, 3 * f.n_out), gpu, HALF[prec])   # one canary row behind
        kw.update(out_act=buf, act_geom=(0, 3 * f.n_out, 0))
        flags |= hip.GEMM_FLAG_OUT_SPLIT3
    else:
        buf = _sentinel((n + 1, M, f.n_out) if n > 1 else (M + 1, f.n_out), gpu)   # a guard item / a guard row behind
        geom = (M * f.n_out if n > 1 else 0, f.n_out, 0)
        kw.update(out_f32=buf, f32_geom=geom)
        if f.h is not None:   # in place: a fresh copy of h
            (buf[:n] if n > 1 else buf[:M]).copy_(f.h if n > 1 else f.h[0])
            kw.update(res=buf, res_geom=geom)
    w3 = d[ktm]
    p = util.gemm_params(d["a3"], w3, M, f.N, K3, nbatch=n, a_off=f.a_row0 * K3, a_bstride=f.S * K3 if n > 1 else 0,
                         w_bstride=f.N * K3 if f.w.dim() == 3 else 0, bias=d["bias"], swiglu=int(f.swiglu),
                         flags=flags | (hip.GEMM_FLAG_W_KTM if ktm else 0), prefetch=prefetch, **kw)
    return p, buf


def launch(f: Form, prec, gpu, variant, share, *, ktm=False, out="f32", prefetch=None, dbg=()):
    """one launch; returns the owned part of the output on the CPU ([n, M, n_out], split form: [M, 3 n_out]) after the ownership check"""
    lib = hip.lib(hip.operands_for(prec))
    p, buf = params(f, prec, gpu, share, ktm=ktm, out=out, prefetch=prefetch)
    flags = list(dbg)
    lib.samaudio_debug_force_gemm_variant(variant)
    for k, v in flags:
        lib.samaudio_debug_set_flag(k, v)
    try:
        hip.check(lib.samaudio_op_gemm(C.byref(p), C.sizeof(p), hip.BF16, util.stream()))
        if gpu.type == "cuda":
            torch.cuda.synchronize()
    finally:
        lib.samaudio_debug_force_gemm_variant(-1)
        for k, _ in flags:
            lib.samaudio_debug_set_flag(k, 0)
    host = buf.cpu()
    own = f.n if (f.n > 1 and out == "f32") else f.M
    mine, guard = host[:own], host[own:]
    what = f"{f.name} {prec} variant {variant} share {share != 0} ktm {ktm} {out}"
    assert torch.isfinite(mine.float()).all(), f"{what}: elements the launch owns are not all finite"
    assert _untouched(guard), f"{what}: the guard behind the output was written"
    return mine.reshape(f.n, f.M, f.n_out) if out == "f32" else mine


def value(f: Form, o):
    """what an output represents, as float64 [n, M, n_out]: an fp32 output itself, a split row's hi + lo"""
    if o.dtype == torch.float32:
        return o.double()
    F = f.n_out
    return (o[:, :F].double() + o[:, F:2 * F].double()).reshape(1, f.M, F)


def check_f64(f: Form, prec, got, what):
    """item 2 of the module text on `got` [n, M, n_out] float64; returns (max-abs error, max|want|)"""
    ref, plain = f.expected(), f.expected(HALF[prec])
    tol_acc = TOL_ACC[prec] * max(1.0, ref["acc"].abs().max().item())
    err = (got - ref["want"]).abs()
    if f.swiglu:
        bound = torch.full_like(err, 2 * tol_acc * max(1.0, ref["a"].abs().max().item()))
    else:
        bound = ref["g"].abs() * tol_acc + 2.0 ** -22 * ref["want"].abs()
    e, e_plain = err.max().item(), (plain["want"] - ref["want"]).abs().max().item()
    at = (err / bound).argmax()
    ratio = (err / bound).flatten()[at].item()
    print(f"x3 form {f.name} ({prec}) {what}: err {e:.3e}; err / bound {ratio:.3f} ({err.flatten()[at].item():.3e} against "
          f"{bound.flatten()[at].item():.3e} there; tol_acc {tol_acc:.3e}); plain 16-bit operands {e_plain:.3e} (x {e_plain / max(e, 1e-300):.0f}); "
          f"|acc| <= {ref['acc'].abs().max().item():.2f}, |ref| <= {ref['want'].abs().max().item():.2f}")
    assert ratio <= 1.0, f"{f.name} {what}: {ratio:.3f} x the float64 bound"
    assert e <= e_plain / PLAIN_FACTOR[prec], (f"{f.name} {what}: {e:.3e} is not 1/{PLAIN_FACTOR[prec]} of the plain 16-bit operands' "
                                              f"{e_plain:.3e}")
    return e, ref["want"].abs().max().item()


def run_form(f: Form, prec, gpu, *, out="f32", general=False):
    """every (kernel, walk, weight layout) launch of one form: ownership, float64 parity of both walks, tile / layout invariance and
    - `general` - the shipped epilogue against the other two.  Returns {(ktm, variant, share): owned output}"""
    layouts = (False,) if f.w.dim() == 3 else (False, True)
    outs = {(ktm, v, s): launch(f, prec, gpu, v, s, ktm=ktm, out=out) for ktm in layouts for v in VARIANTS for s in WALKS}
    base = {s: outs[(False, hip.GV_GEMM8_256x256, s)] for s in WALKS}
    for key, o in outs.items():
        assert same_bits(o, base[key[2]]), f"{f.name} {prec} (ktm, variant, share) = {key}: the bits depend on the tile size or the weight layout"
    e = {s: check_f64(f, prec, value(f, base[s]), f"{out} {'sharing' if s else 'plain'} walk") for s in WALKS}
    e_plain, e_share, scale = e[0][0], e[hip.GEMM_FLAG_X3_SHARE][0], e[0][1]
    assert e_share <= 2 * e_plain + 1e-6 * scale, f"{f.name}: sharing walk {e_share:.3e} against the plain walk's {e_plain:.3e}"
    if general:   # the shipped epilogue (epilogue8_rows) against the general one and the register one (epilogue8_linear)
        for mode, name in ((hip.DBG_EPI_GENERAL, "general"), (hip.DBG_EPI_LINEAR, "register")):
            for v in VARIANTS:
                for s in WALKS:
                    o = launch(f, prec, gpu, v, s, out=out, dbg=[(hip.DBG_GEMM8_EPILOGUE, mode)])
                    assert same_bits(o, base[s]), f"{f.name} {prec} variant {v} share {s != 0}: the {name} epilogue differs from the shipped one"
    return outs


# ---- form 1: gate table + per-item gate, residual in place ----------------------------------------------------------------------
# (339, 320, 192): 3 items of 113 rows - a whole 256-row tile and a partial one whose second 128-row half is outside the problem, both
# gate boundaries inside a 16-row block; N = 320: 256 + one 64-wide wave column; K = 64 / 192 / 448: 1 / 3 / 7 original K-tiles;
# M = 1 and 129: the row tails
@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("shape", [(339, 320, 192), (339, 512, 64), (339, 320, 448), (1, 320, 192), (129, 320, 192)])
def test_gated_in_place_residual(gpu, prec, shape):
    run_form(form_gated_residual(*shape, seed=100 + sum(shape)), prec, gpu, general=True)


@pytest.mark.parametrize("prec", X3)
def test_gated_in_place_residual_batched(gpu, prec):
    """the gate row of a BATCHED launch: 2 batch items of 226 rows, each 2 gates of 113 rows - gate row (b M + m) / T, rows 2 and 3 of the
    gates for the second item (no launch of the engine is batched and gated; the contract of GemmParams is)"""
    run_form(form_gated_residual(226, 320, 192, seed=150, n=2, T=113), prec, gpu, general=True)


# ---- forms 2 and 3: SwiGLU, fp32 output and split-form output -----------------------------------------------------------------------
# F = 160: output rows of 3 F = 480 elements; K = 128: 2 original K-tiles
@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("shape", [(339, 160, 192), (339, 256, 64), (339, 160, 128), (339, 256, 448), (1, 160, 192), (129, 160, 192)])
def test_swiglu_fp32_output_and_split_form_output(gpu, prec, shape):
    """Form 3 (general epilogue) against float64; form 2 (register epilogue): [lo | hi | hi] with both hi blocks equal, bit for bit the
    split of form 3's output of the same launch - hi = v.to(half), lo = (v - hi.float()).to(half), the statement of
    tests/test_x3_gpu.py::test_split3_writes_lo_hi_hi - and hi + lo within the float64 bound."""
    f = form_swiglu(*shape, seed=200 + sum(shape))
    half, F = HALF[prec], f.n_out
    v32 = run_form(f, prec, gpu, out="f32")
    s3 = run_form(f, prec, gpu, out="split3")
    for key, row in s3.items():
        assert same_bits(row[:, F:2 * F], row[:, 2 * F:]), f"{f.name} {key}: the two hi blocks differ"
        v = v32[key][0]
        hi = v.to(half)
        lo = (v - hi.float()).to(half)
        assert same_bits(row[:, F:2 * F], hi), f"{f.name} {key}: hi is not the fp32 output rounded"
        assert same_bits(row[:, :F], lo), f"{f.name} {key}: lo is not the rounded residual of the fp32 output"


@pytest.mark.parametrize("prec", X3)
def test_split_form_output_needs_whole_16_byte_column_groups(gpu, prec):
    """F % 8 != 0 with GEMM_FLAG_OUT_SPLIT3 is refused, nothing is launched (F = 164: N = 2 F is no multiple of 32 either, which gemm_check
    asks of every SwiGLU launch - N % 32 == 0 implies F % 16 == 0, so the F % 8 test of gemm8_split3_ok is the second line of defence)"""
    lib, half = hip.lib(hip.operands_for(prec)), HALF[prec]
    M, F, K3 = 16, 164, 576
    a3, w3 = torch.zeros(M, K3, dtype=half, device=gpu), torch.zeros(2 * F, K3, dtype=half, device=gpu)
    out = _sentinel((M, 3 * F), gpu, half)
    lib.samaudio_debug_force_gemm_variant(hip.GV_GEMM8S_128x128)
    try:
        p = util.gemm_params(a3, w3, M, 2 * F, K3, swiglu=1, out_act=out, act_geom=(0, 3 * F, 0), flags=hip.GEMM_FLAG_OUT_SPLIT3)
        assert lib.samaudio_op_gemm(C.byref(p), C.sizeof(p), hip.BF16, util.stream()) == hip.ERR_ARG
    finally:
        lib.samaudio_debug_force_gemm_variant(-1)
    assert _untouched(out.cpu())


# ---- form 4: the batched fold ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", X3)
def test_batched_fold_per_item_weight(gpu, prec):
    """nbatch = 3, M = T = 70, N = 320, K = 192 (K' = 576, the engine's): a_bstride = T K', w_bstride = N K', res_bstride = f32_bstride =
    T N, a guard item behind the buffer.  Rows only: a K-tile-major launch of per-item weights is refused."""
    f = form_fold(3, 70, 320, 192, seed=300)
    run_form(f, prec, gpu, general=True)
    lib = hip.lib(hip.operands_for(prec))
    for variant in VARIANTS:
        p, buf = params(f, prec, gpu, hip.GEMM_FLAG_W_KTM)
        before = buf.cpu()
        lib.samaudio_debug_force_gemm_variant(variant)
        try:
            assert lib.samaudio_op_gemm(C.byref(p), C.sizeof(p), hip.BF16, util.stream()) == hip.ERR_ARG
            assert "K-tile-major" in lib.samaudio_last_error().decode()
        finally:
            lib.samaudio_debug_force_gemm_variant(-1)
        assert same_bits(buf.cpu(), before)


# ---- form 5: bias + residual ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("shape", [(339, 320, 192), (339, 512, 128), (339, 320, 448)])
def test_bias_in_place_residual(gpu, prec, shape):
    run_form(form_bias_residual(*shape, seed=400 + sum(shape)), prec, gpu, general=True)


# ---- form 6: batched A with an offset, one shared weight -------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("shape", [(320, 192), (512, 64), (320, 128), (320, 448)])
def test_batched_rows_behind_an_offset_shared_weight(gpu, prec, shape):
    """nbatch = 3, items of S = 71 rows of which rows 1 .. 70 are read: a_off = K', a_bstride = S K'"""
    run_form(form_cat_proj(3, 71, *shape, seed=500 + sum(shape)), prec, gpu, general=True)


# ---- the idle prefetch workgroups ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", X3)
def test_prefetch_workgroups_change_nothing(gpu, prec):
    """form 1 at (339, 320, 192) with pf_ptr on a NaN-filled buffer: launches of fewer than 256 workgroups are padded to 256 and the
    workgroups beyond the tiles read it - the output is the bits of the launch without, the buffer is unchanged"""
    f = form_gated_residual(339, 320, 192, seed=100 + 339 + 320 + 192)
    pf = _sentinel((1 << 18,), gpu)   # 1 MiB: 8192 lines over 247 - 252 idle workgroups
    for v in VARIANTS:
        for s in WALKS:
            want = launch(f, prec, gpu, v, s)
            got = launch(f, prec, gpu, v, s, prefetch=pf)
            assert same_bits(got, want), f"variant {v} share {s != 0}: a launch with prefetch workgroups computes something else"
    assert _untouched(pf.cpu())


# ---- more than one round of tiles: persistent walk and tail split ---------------------------------------------------------------------
@pytest.mark.skipif(SIM, reason="272 tiles of 256 x 256 (4352 x 4096): a launch of 6.8 GFLOP, hardware only")
@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("form", ["gated", "swiglu"])
def test_persistent_walk_and_tail_split(gpu, prec, form):
    """(4352, 4096, 64): 17 x 16 = 272 tiles, as form 1 with 32 items of 136 rows (gate boundaries inside 16-row blocks) and as form 2
    (the register epilogue: no barrier between a workgroup's tiles).  The policy (variant -1) splits the launch - 256 tiles on
    gemm8x_kernel / gemm8_kernel with tile_count, 16 as 64 quadrants on gemm8s_kernel with skip256; the forced 256 x 256 kernel walks the
    272 tiles persistently on 256 workgroups; DBG_GEMM8_NOT_PERSISTENT = 1 gives every tile its workgroup; the forced 128 x 128 kernel has
    1088 tiles (its double-buffered form: more than 256 workgroups).  The same bits from all four, within the float64 bound, on both
    walks."""
    M, N, K = 4352, 4096, 64
    if form == "gated":
        g = _gen(600)
        x, w = _xw(g, 1, M, N, K)
        f = Form(f"gated in-place residual ({M}, {N}, {K}) T 136", x, w, M, gate=torch.randn(32, N, generator=g),
                 tab=torch.randn(N, generator=g), T=136, h=torch.randn(1, M, N, generator=g))
        out = "f32"
    else:
        f, out = form_swiglu(M, N // 2, K, seed=601), "split3"
    e = {}
    for s in WALKS:
        split = launch(f, prec, gpu, -1, s, ktm=True, out=out)
        walk = launch(f, prec, gpu, hip.GV_GEMM8_256x256, s, ktm=True, out=out)
        each = launch(f, prec, gpu, hip.GV_GEMM8_256x256, s, ktm=True, out=out, dbg=[(hip.DBG_GEMM8_NOT_PERSISTENT, 1)])
        small = launch(f, prec, gpu, hip.GV_GEMM8S_128x128, s, ktm=True, out=out)
        assert same_bits(walk, each), f"share {s != 0}: the persistent walk differs from one workgroup per tile"
        assert same_bits(split, each), f"share {s != 0}: the tail-split launch differs from the single launch"
        assert same_bits(small, each), f"share {s != 0}: the 128 x 128 kernel differs from the 256 x 256 kernel"
        if out == "split3":
            assert same_bits(split[:, N // 2:N], split[:, N:]), "the two hi blocks differ"
        e[s] = check_f64(f, prec, value(f, split), f"272 tiles, {out} {'sharing' if s else 'plain'} walk")
    assert e[hip.GEMM_FLAG_X3_SHARE][0] <= 2 * e[0][0] + 1e-6 * e[0][1]
