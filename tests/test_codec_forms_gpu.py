"""Every convolution form the DAC-VAE of a compensated context (precision "fp16x3" / "bf16x3": SAMAUDIO_OPT_X3_CLASSES bit CODEC) launches,
each on its own against float64 (tests/conv_ref.py), and the codec end to end at clip lengths that leave row tails at every stage.

Engine::codec_encode / codec_decode launch ten forms.  The narrow ones (N < 256) multiply on operands split in registers (gemm.hip
gemm_kernel<.., FLY>: GEMM_FLAG_X3_FLY | GEMM_FLAG_W_FLY16, 4 x 1 waves, the rolled "lean" epilogue); the wide ones run as split3 + one
16-bit launch over K' = 3K on the 8-phase kernels + an elementwise activation pass (host.h codec_x3_*).  Both are reached through
samaudio_op_codec_conv, which launches by the functions the engine launches by, with twins made by weights.convert_codec_x3 /
convert_codec_fly16 under the engine's own weight names.

Every case fills its output buffers, halo rows included, with a NaN sentinel; afterwards every row the launch owns must be finite and
every other row must still hold the sentinel's bits.  Bounds against float64 are those of
tests/test_x3_gpu.py::test_fp32_gemm_with_operands_split_on_the_fly: raw result within tol = (4e-6 fp16x3 | 1e-4 bf16x3) x max(1, max|ref|),
activated result within 2 tol, error at most 1/20 of what plain 16-bit operands give.  On the CPU simulator (SAMAUDIO_EMU_DRYRUN=simt:
bfloat16 library only) the bf16x3 forms run the same kernels and host geometry.
"""
import ctypes as C
import math
import os

import pytest
import torch

from oracle import samaudio_oracle as O
from sam_audio_amd import SAMAudio, hip, preset_config
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip
from sam_audio_amd.weights import convert_codec_fly16, convert_codec_x3
from tests import conv_ref as R
from tests import util
from tests.test_codec_workspace_gpu import TOL as CODEC_TOL

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
X3 = ["bf16x3"] if SIM else ["fp16x3", "bf16x3"]
HALF = {"fp16x3": torch.float16, "bf16x3": torch.bfloat16}
HALO = R.HALO
SENT = 0x7FC5A5A5   # a quiet NaN no kernel produces
ACTS = {"none": hip.ACT_NONE, "snake": hip.ACT_SNAKE, "tanh": hip.ACT_TANH}
PATHS = {hip.CODEC_PATH_FLY: "fly", hip.CODEC_PATH_X3_BLOCK: "x3block", hip.CODEC_PATH_X3: "x3"}


def _sentinel(shape, dev):
    t = torch.empty(shape, dtype=torch.float32, device=dev)
    t.view(torch.int32).fill_(SENT)
    return t


class Form:
    """One convolution launch, stated on CPU tensors.  x: the interior [n, T, Cin] of the halo buffer the launch reads; w [N, K];
    geom: the K-axis side of GemmParams (rows / offsets in units of input rows are turned into elements here); raw / act: None or
    (rows of the buffer per item, columns, first owned row, owned rows, ld, off) of the fp32 / activated output;
    ref(x, w) -> float64 accumulator [n, owned rows, columns]."""

    def __init__(self, name, wname, x, w, M, *, lda, kc, tap_stride, a_row0, ref, bias=None, act="none", alpha=None, res=False,
                 raw=None, actout=None, chan_mod=0, window=None, f32_act=0, seed=0):
        self.name, self.wname, self.x, self.w, self.M = name, wname, x, w, M
        self.lda, self.kc, self.tap_stride, self.a_row0, self.ref = lda, kc, tap_stride, a_row0, ref
        self.bias, self.act, self.alpha, self.res, self.raw, self.actout = bias, act, alpha, res, raw, actout
        self.chan_mod, self.window, self.f32_act = chan_mod, window, f32_act
        self.resval = None
        if res:   # the fp32 stream the k1 convolution adds in place
            g = torch.Generator().manual_seed(1000 + seed)
            self.resval = torch.randn(x.shape[0], raw[3], raw[1], generator=g)

    def expected(self, half=None):
        """(raw, activated) in float64 from the fp32 operands, or from operands rounded to `half`"""
        xv, wv = (self.x, self.w) if half is None else (R.rounded(self.x, half), R.rounded(self.w, half))
        return R.finish(self.ref(xv, wv), self.bias, self.resval, self.act, self.alpha)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _acts(g, n, T, C):   # per-channel scales 10^-1.5 .. 10: lo halves reach IEEE half's subnormals
    return torch.randn(n, T, C, generator=g) * torch.logspace(-1.5, 1, C)[None, None, :]


def _halo_out(T, C):   # a halo buffer of T rows: (rows, cols, first owned row, owned rows, ld, off)
    return (T + 2 * HALO, C, HALO, T, C, HALO * C)


def form_same(n, T, Cin, Cout, taps, dil, *, wname, act="snake", raw=False, actout=True, res=False, dense=False, f32_act=0, seed=0):
    """'same' convolution, k = taps, dilation dil (conv_same of engine.hip)"""
    g = _gen(seed)
    x, w = _acts(g, n, T, Cin), torch.randn(Cout, taps * Cin, generator=g) * 0.05
    bias = torch.randn(Cout, generator=g) * 0.1
    alpha = torch.rand(Cout, generator=g) + 0.5 if act == "snake" else None
    out = (T, Cout, 0, T, Cout, 0) if dense else _halo_out(T, Cout)
    return Form(f"k{taps} dil {dil} C {Cin}->{Cout} M {T} n {n}", wname, x, w, T, lda=Cin, kc=Cin, tap_stride=(Cin if taps == 1 else dil * Cin),
                a_row0=HALO - (taps // 2) * dil, ref=lambda xv, wv: R.conv_same(xv, wv, taps, dil), bias=bias, act=act, alpha=alpha, res=res,
                raw=out if raw else None, actout=out if actout else None, f32_act=f32_act, seed=seed)


def form_input(n, S, *, seed=0):
    """the encoder's input convolution: rows of 8 (padded) channels, a window of 8 rows = one 64-wide K: lda = 8 < kc = 64"""
    g = _gen(seed)
    x, w = _acts(g, n, S, 8), torch.randn(64, 64, generator=g) * 0.05
    bias, alpha = torch.randn(64, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5
    return Form(f"input conv M {S} n {n}", "enc.in.w", x, w, S, lda=8, kc=64, tap_stride=0, a_row0=HALO - 3,
                ref=lambda xv, wv: R.conv_same(xv, wv, 8, 1), bias=bias, act="snake", alpha=alpha, raw=_halo_out(S, 64), actout=_halo_out(S, 64),
                seed=seed)


def form_strided(n, M, C, s, *, wname="enc.s0.down.w", seed=0):
    """k = 2s, stride s: the 2s input rows of one output row are contiguous, lda = s C != kc = K = 2 s C"""
    g = _gen(seed)
    T = M * s
    x, w = _acts(g, n, T, C), torch.randn(2 * C, 2 * s * C, generator=g) * 0.05
    bias, alpha = torch.randn(2 * C, generator=g) * 0.1, torch.rand(2 * C, generator=g) + 0.5
    return Form(f"strided s {s} C {C}->{2 * C} M {M} n {n}", wname, x, w, M, lda=s * C, kc=2 * s * C, tap_stride=0,
                a_row0=HALO - math.ceil(s / 2), ref=lambda xv, wv: R.conv_strided(xv, wv, s), bias=bias, act="snake", alpha=alpha,
                raw=_halo_out(M, 2 * C), actout=_halo_out(M, 2 * C), seed=seed)


def form_transposed(n, T, Cin, C, s, *, wname="dec.s0.up.w", seed=0):
    """ConvTranspose1d(k = 2s, stride s, pad ceil(s / 2)): M = T + 1 rows of N = s C, each the s output rows x[q - 1] W[r + s] + x[q] W[r];
    the window [c_lo, c_hi) clips the first and the last of them"""
    g = _gen(seed)
    x, w = _acts(g, n, T, Cin), torch.randn(s * C, 2 * Cin, generator=g) * 0.05
    bias, alpha = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    pad, To = math.ceil(s / 2), T * s
    out = (To + 2 * HALO, C, HALO, To, s * C, (HALO - pad) * C)
    return Form(f"transposed s {s} Cin {Cin}->{C} T {T} n {n}", wname, x, w, T + 1, lda=Cin, kc=2 * Cin, tap_stride=0, a_row0=HALO - 1,
                ref=lambda xv, wv: R.conv_transposed(xv, wv, s), bias=bias, act="snake", alpha=alpha, raw=out, actout=out, chan_mod=C,
                window=(pad * C, (To + pad) * C, s * C), seed=seed)


def twin_of(f: Form, half):
    """(kind, tensor, cin): the twin the model would register for an engine weight of this name and shape"""
    x3 = convert_codec_x3({f.wname: f.w}, half)
    if x3:
        t = x3[f.wname + ".x3"]
        return hip.CODEC_TWIN_X3, t, t.shape[2] // 3
    fly = convert_codec_fly16({f.wname: f.w}, half)
    if fly:
        return hip.CODEC_TWIN_FLY, fly[f.wname + ".fly"], 0
    return hip.CODEC_TWIN_NONE, None, 0


def launch(f: Form, prec, gpu, mode, *, items=None, M=None, act=None, dbg_old_tiles=0, expect_path=None):
    """Run `f` (or its items [i0, i1)) and return {"raw": .., "act": ..}: the WHOLE output buffers on the CPU.
    mode: "exact" (flags 0), "fly" (X3_FLY, the fp32 weight), "twin" (X3_FLY | W_FLY16 through samaudio_op_gemm), "hook"
    (samaudio_op_codec_conv with the weight's twin: what the engine runs)."""
    lib = hip.lib(hip.operands_for(prec))
    half = HALF[prec]
    i0, i1 = items or (0, f.x.shape[0])
    n, Cin = i1 - i0, f.x.shape[2]
    M = f.M if M is None else M
    act = f.act if act is None else act
    xd = R.halo_buffer(f.x[i0:i1]).to(gpu).contiguous()
    kind, twin, cin = twin_of(f, half)
    twin_d = None if twin is None else twin.to(gpu).contiguous()
    wd = f.w.to(gpu).contiguous()
    bufs, kw = {}, {}
    for key, spec in (("raw", f.raw), ("act", f.actout)):
        if spec is None:
            continue
        rows, cols, r0, own, ld, off = spec
        b = _sentinel((n, rows, cols), gpu)
        if key == "raw" and f.res:
            b[:, r0:r0 + own] = f.resval[i0:i1].to(gpu)
        bufs[key] = b
        kw["out_f32" if key == "raw" else "out_act"] = b
        kw["f32_geom" if key == "raw" else "act_geom"] = (rows * cols, ld, off)
    if f.res:
        kw["res"], kw["res_geom"] = bufs["raw"], kw["f32_geom"]
    if f.window:
        kw["c_lo"], kw["c_hi"], kw["c_ld_rel"] = f.window
    keep = [t.to(gpu) for t in (f.bias, f.alpha) if t is not None]   # (kept alive across the call)
    bd = f.bias.to(gpu) if f.bias is not None else None
    ad = f.alpha.to(gpu) if (f.alpha is not None and act == "snake") else None
    flags = {"exact": 0, "fly": hip.GEMM_FLAG_X3_FLY, "twin": hip.GEMM_FLAG_X3_FLY | hip.GEMM_FLAG_W_FLY16, "hook": 0}[mode]
    p = util.gemm_params(xd, twin_d if mode == "twin" else wd, M, f.w.shape[0], f.w.shape[1], nbatch=n, a_off=f.a_row0 * Cin,
                         a_bstride=xd.shape[1] * Cin, lda=f.lda, kc=f.kc, tap_stride=f.tap_stride, bias=bd, chan_mod=f.chan_mod,
                         act=ACTS[act], f32_act=f.f32_act if act != "none" else 0, act_alpha=ad, flags=flags, **kw)
    p.tag = 1   # the codec's own instantiations
    path = C.c_int(-1)
    lib.samaudio_debug_set_flag(hip.DBG_FLY_OLD_TILES, dbg_old_tiles)
    try:
        if mode == "hook":
            nbytes = n * xd.shape[1] * 3 * Cin * 2 if kind == hip.CODEC_TWIN_X3 else 0
            scratch = torch.full((max(nbytes, 16),), 255, dtype=torch.uint8, device=gpu)
            hip.check(lib.samaudio_op_codec_conv(C.byref(p), C.sizeof(p), hip.ptr(twin_d), kind, cin, hip.ptr(scratch), nbytes,
                                                 C.byref(path), util.stream()))
            if expect_path is not None:
                assert path.value == expect_path, f"{f.name}: ran as {PATHS.get(path.value)}, the engine's choice is {PATHS[expect_path]}"
        else:
            hip.check(lib.samaudio_op_gemm(C.byref(p), C.sizeof(p), hip.F32, util.stream()))
        if gpu.type == "cuda":
            torch.cuda.synchronize()
    finally:
        lib.samaudio_debug_set_flag(hip.DBG_FLY_OLD_TILES, 0)
    del keep
    return {k: b.cpu() for k, b in bufs.items()}


def owned(f: Form, out, key, M=None):
    """the rows of buffer `key` the launch owns [n, own, cols]; asserts they are finite and every other row is untouched"""
    rows, cols, r0, own, ld, off = f.raw if key == "raw" else f.actout
    if M is not None and M != f.M:
        assert not f.window
        own = M
    b = out[key]
    mine = b[:, r0:r0 + own]
    assert torch.isfinite(mine).all(), f"{f.name}: {key} rows the launch owns are not all finite"
    rest = torch.cat([b[:, :r0], b[:, r0 + own:]], 1)
    assert (rest.view(torch.int32) == SENT).all(), f"{f.name}: {key} rows outside the launch's own were written"
    return mine


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_against_f64(f: Form, prec, got, what, exact=None):
    """the bounds of the existing fly test on the owned rows `got` = {"raw": .., "act": ..}"""
    half = HALF[prec]
    ref_raw, ref_act = f.expected()
    pl_raw, pl_act = f.expected(half)
    scale = max(1.0, ref_raw.abs().max().item())
    tol = (4e-6 if half == torch.float16 else 1e-4) * scale
    msg = [f"{what} {f.name} ({prec}): tol {tol:.3e}"]
    lead = "raw" if "raw" in got else "act"
    errs = {}
    for key, ref, plain in (("raw", ref_act if f.f32_act else ref_raw, pl_act if f.f32_act else pl_raw), ("act", ref_act, pl_act)):
        if key not in got:
            continue
        e = (got[key].double() - ref).abs().max().item()
        e_plain = (plain - ref).abs().max().item()
        activated = key == "act" or f.f32_act
        errs[key] = (e, e_plain, (2 if activated and f.act != "none" else 1) * tol)
        msg.append(f"{key} err {e:.3e} (bound {errs[key][2]:.3e}; plain 16-bit operands {e_plain:.3e}"
                   + (f"; exact-fp32 launch {(exact[key].double() - ref).abs().max().item():.3e})" if exact else ")"))
    print("; ".join(msg) + f"; |ref| <= {ref_raw.abs().max().item():.2f}")
    for key, (e, e_plain, bound) in errs.items():
        assert e < bound, f"{f.name} {key}: {e:.3e} >= {bound:.3e}"
    e, e_plain, _ = errs[lead]
    assert e < e_plain / 20, f"{f.name} {lead}: {e:.3e} is not 1/20 of the plain 16-bit operands' {e_plain:.3e}"


def run_narrow(f: Form, prec, gpu, path=hip.CODEC_PATH_FLY):
    """One narrow form: the engine's launch (hook) against float64, beside the exact-fp32 launch; bitwise against the register split
    (X3_FLY alone), the direct W_FLY16 launch and the tiles of the plain policy; items of a batched launch against single launches."""
    n = f.x.shape[0]
    keys = [k for k, s in (("raw", f.raw), ("act", f.actout)) if s]
    hook = launch(f, prec, gpu, "hook", expect_path=path)
    got = {k: owned(f, hook, k) for k in keys}
    exact = launch(f, prec, gpu, "exact")
    check_against_f64(f, prec, got, "narrow", exact={k: owned(f, exact, k) for k in keys})
    if n == 1:
        others = {"fly": launch(f, prec, gpu, "fly"), "twin": launch(f, prec, gpu, "twin"),
                  "old tiles": launch(f, prec, gpu, "hook", dbg_old_tiles=1)}
        for name, o in others.items():
            for k in keys:
                assert same_bits(o[k], hook[k]), f"{f.name}: {k} of the {name} launch differs from the shipped launch"
    else:
        for i in range(n):
            one = launch(f, prec, gpu, "hook", items=(i, i + 1))
            for k in keys:
                assert same_bits(one[k][0], hook[k][i]), f"{f.name}: item {i} of the batched launch differs from its single launch ({k})"
    return hook


# ---- narrow forms (the fly tiles) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("n", [1, 3])
def test_input_convolution_overlapping_rows(gpu, prec, n):
    run_narrow(form_input(n, 131, seed=11), prec, gpu)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("M", [97, 129])
@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("C_", [64, 96, 128, 192])
def test_k7_same_act_only(gpu, prec, C_, dil, M, n):
    f = form_same(n, M, C_, C_, 7, dil, wname="enc.s0.r0.w1", seed=20 + C_ + dil)
    full = run_narrow(f, prec, gpu)
    if M == 129 and n == 1:   # accumulation order depends only on k: a shorter launch on the same buffer writes the same rows
        short = launch(f, prec, gpu, "hook", M=97)
        assert same_bits(owned(f, short, "act", M=97), owned(f, full, "act")[:, :97]), f"{f.name}: rows common to M = 97 and M = 129 differ"


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("M", [1, 33, 127, 131])
@pytest.mark.parametrize("C_", [64, 96, 128, 192])
def test_k1_in_place_residual_and_snake_copy(gpu, prec, C_, M, n):
    run_narrow(form_same(n, M, C_, C_, 1, 1, wname="enc.s0.r0.w2", raw=True, res=True, seed=40 + C_ + M), prec, gpu)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("n", [1, 3])
def test_strided(gpu, prec, n):
    run_narrow(form_strided(n, 65, 64, 2, seed=60), prec, gpu)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T", [1, 37, 128])
def test_transposed_windowed(gpu, prec, T, n):
    run_narrow(form_transposed(n, T, 192, 96, 2, seed=70 + T), prec, gpu)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("M", [1, 20])
def test_encoder_proj_dense_rows(gpu, prec, M, n):
    run_narrow(form_same(n, M, 1024, 128, 1, 1, wname="enc.proj.w", act="none", raw=True, actout=False, dense=True, seed=80 + M), prec, gpu)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("n", [1, 3])
def test_final_convolution_tanh(gpu, prec, n):
    run_narrow(form_same(n, 130, 96, 1, 7, 1, wname="dec.out.w", act="tanh", raw=True, actout=False, dense=True, f32_act=1, seed=90), prec, gpu)


# ---- wide forms (split3 + one 16-bit launch over K' = 3K + the activation pass) ---------------------------------------------------
def run_wide(f: Form, prec, gpu, path):
    """One wide form through the hook against float64; then the activation pass alone: the same launch without its activation must
    leave the same raw bits, and act(raw) must be the fp32 evaluation of the float64 activation OF THAT RAW VALUE:
    |act - act64(raw)| <= 8 x 2^-24 x (|raw| + 1 / alpha) - hardware-accurate sinf, one square, one division, one add."""
    keys = [k for k, s in (("raw", f.raw), ("act", f.actout)) if s]
    hook = launch(f, prec, gpu, "hook", expect_path=path)
    got = {k: owned(f, hook, k) for k in keys}
    check_against_f64(f, prec, got, "wide")
    if f.act == "none":
        return
    plain = launch(f, prec, gpu, "hook", act="none", expect_path=path)
    raw = owned(f, plain, "raw" if "raw" in keys else "act")
    if "raw" in keys:
        assert same_bits(plain["raw"], hook["raw"]), f"{f.name}: the raw stream depends on the activation"
        if "act" in keys:
            assert same_bits(owned(f, plain, "act"), raw), f"{f.name}: without an activation the second output is a copy of the raw one"
    want = R.finish(raw.double(), act=f.act, alpha=f.alpha)[1]
    inv_a = 1.0 / f.alpha.double() if f.alpha is not None else torch.ones(())
    bound = 8 * 2.0 ** -24 * (raw.double().abs() + inv_a)
    err = (got["act"].double() - want).abs()
    print(f"wide {f.name} ({prec}): activation pass max err / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), f"{f.name}: activation pass off by {(err / bound).max().item():.2f} x its bound"


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("dil", [1, 9])
@pytest.mark.parametrize("C_", [256, 384])
def test_wide_k7(gpu, prec, C_, dil):
    run_wide(form_same(2, 131, C_, C_, 7, dil, wname="dec.s0.r0.w1", seed=100 + C_ + dil), prec, gpu, hip.CODEC_PATH_X3_BLOCK)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("M", [1, 131])
def test_wide_k1_in_place_residual(gpu, prec, M):
    run_wide(form_same(1, M, 256, 256, 1, 1, wname="dec.s0.r0.w2", raw=True, res=True, seed=120 + M), prec, gpu, hip.CODEC_PATH_X3)


@pytest.mark.parametrize("prec", X3)
def test_wide_strided(gpu, prec):
    run_wide(form_strided(1, 66, 128, 2, wname="enc.s1.down.w", seed=130), prec, gpu, hip.CODEC_PATH_X3_BLOCK)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("T", [1, 37])
def test_wide_transposed_windowed(gpu, prec, T):
    run_wide(form_transposed(1, T, 256, 128, 2, seed=140 + T), prec, gpu, hip.CODEC_PATH_X3_BLOCK)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T", [1, 37, 128])
def test_transposed_many_phases_takes_the_engines_path(gpu, prec, T, n):
    """s = 12, Cin = 64 -> 32 channels: N = s C = 384 has an x3 twin, so the engine runs it wide - the hook must as well"""
    f = form_transposed(n, T, 64, 32, 12, seed=150 + T)
    run_wide(f, prec, gpu, hip.CODEC_PATH_X3_BLOCK)
    if n == 3:
        whole = launch(f, prec, gpu, "hook")
        for i in range(n):
            one = launch(f, prec, gpu, "hook", items=(i, i + 1))
            assert same_bits(one["raw"][0], whole["raw"][i]) and same_bits(one["act"][0], whole["act"][i]), f"{f.name}: item {i}"


@pytest.mark.parametrize("prec", X3)
def test_wide_whole_k_with_sharing(gpu, prec):
    """dec.proj: k1, K = 128 -> K' = 384, N = 1024, one activated output without an activation: the whole-K X3 launch, operand tiles shared"""
    run_wide(form_same(1, 20, 128, 1024, 1, 1, wname="dec.proj.w", act="none", seed=160), prec, gpu, hip.CODEC_PATH_X3)


@pytest.mark.parametrize("prec", X3)
def test_wide_k3_same(gpu, prec):
    """the form of enc.out: k3 'same', no activation, one output"""
    run_wide(form_same(1, 37, 256, 256, 3, 1, wname="enc.out.w", act="none", seed=170), prec, gpu, hip.CODEC_PATH_X3_BLOCK)


# ---- codec clip lengths, end to end -------------------------------------------------------------------------------------------
PRECS = ["fp32", "bf16", "bf16x3"] if SIM else ["fp32", "bf16", "fp16", "fp16x3", "bf16x3"]
_REF, _MODELS = {}, {}


def _reference(T0):
    """3 clips of T0 latent frames, the oracle's latents of them and its decode of those - once per length"""
    if "cfg" not in _REF:
        cfg = preset_config("tiny")
        _REF.update(cfg=cfg, sd={k: v for k, v in init_state_dict(cfg, seed=6).items() if k.startswith("audio_codec.")})
    if T0 not in _REF:
        cfg, sd = _REF["cfg"], _REF["sd"]
        wav = torch.stack([synthetic_clip(i, T0 * cfg.audio_codec.hop_length) for i in range(3)])
        with torch.inference_mode():
            z = O.dac_encode(sd, cfg.audio_codec, wav)
            w = O.dac_decode(sd, cfg.audio_codec, z).squeeze(1)
        _REF[T0] = (wav, z.transpose(1, 2).contiguous(), w)
    return _REF[T0]


def _model(prec, gpu):
    if prec not in _MODELS:
        _reference(1)
        m = SAMAudio(_REF["cfg"], precision=prec, device=str(gpu), codec_decode="32")
        m.load_state_dict(_REF["sd"], strict=False)
        _MODELS[prec] = m
    return _MODELS[prec]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T0", [1, 2, 7, 33])
def test_codec_clip_lengths(gpu, prec, T0):
    """encode_audio / decode_audio of 1 and 3 clips of T0 latent frames against the oracle, under the workspace guard: T0 = 1 gives
    the deepest stage M = 1 and a transposed convolution M = 2; 7 and 33 leave row tails at every stage.  Bounds: the per-precision
    (latent, waveform) pairs of tests/test_codec_workspace_gpu.py.  Three clips in one call equal three calls, bit for bit."""
    wav, z_ref, w_ref = _reference(T0)
    model = _model(prec, gpu)
    model._workspace = None
    with util.workspace_guard(model):
        z3 = model.encode_audio(wav.to(gpu)).clone()
        w3 = model.decode_audio(z_ref.to(gpu)).clone()
        z1 = [model.encode_audio(wav[i:i + 1].to(gpu)).clone() for i in range(3)]
        w1 = [model.decode_audio(z_ref[i:i + 1].to(gpu)).clone() for i in range(3)]
    model._workspace = None
    for n, z, w in ((1, z1[0], w1[0]), (3, z3, w3)):
        util.report(f"codec encode {prec} T0 {T0} n {n}", z, z_ref[:n], CODEC_TOL[prec][0])
        util.report(f"codec decode {prec} T0 {T0} n {n}", w, w_ref[:n], CODEC_TOL[prec][1])
    for i in range(3):
        assert same_bits(z1[i][0].cpu(), z3[i].cpu()), f"encode: clip {i} of three differs from its own call"
        assert same_bits(w1[i][0].cpu(), w3[i].cpu()), f"decode: clip {i} of three differs from its own call"
