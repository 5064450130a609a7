"""Compensated 16-bit operands for the PE-Core vision tower: `PEVisionTower(precision="fp16x3" | "bf16x3")`
(include/samaudio.h samaudio_vit_set_option).

fp32 storage; the four GEMMs of every block, the pooling head's k|v projection and the self-attention multiply hi/lo-split 16-bit
operands; the LayerNorms in front of q|k|v, c_fc and pool.wkv write the split rows themselves (layernorm_rows_split3_kernel) and
c_fc's epilogue writes c_proj's split operand (GEMM_FLAG_OUT_SPLIT3 with bias + GELU).  The reference is oracle/vit_oracle.py in fp32
on the CPU, held to 1e-4 x max(1, |v|) of its float64 form on the hostile weights by tests/test_vit_x3_cpu.py.  The bar of every
parity check is the project's - 1e-3 x max(1, |reference|max) - and the asserted bounds are 2x the errors measured on MI355X
(MEASURED below, profiles/vit_x3/gpu_tests.log), never above the bar.  On the CPU simulator (SAMAUDIO_EMU_DRYRUN=simt: the bfloat16
library only) the bf16x3 cases exercise the same kernels, layouts and plumbing.
"""
import ctypes as C
import dataclasses
import functools
import os

import pytest
import torch

from oracle import vit_oracle as V
from sam_audio_amd import hip
from sam_audio_amd.config import PE_VISION_CONFIGS, PEVisionConfig, PerceptionEncoderConfig
from sam_audio_amd.synthetic import init_vision_state_dict, make_hostile_vision
from sam_audio_amd.vision_tower import PEVisionTower, convert_vision
from sam_audio_amd.weights import x3_weight
from tests import util

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
X3 = ["bf16x3"] if SIM else ["fp16x3", "bf16x3"]
HALF = {"fp16x3": torch.float16, "bf16x3": torch.bfloat16}
PLAIN = {"fp16x3": "fp16", "bf16x3": "bf16"}   # the plain 16-bit mode of the same library
BAR = 1e-3                                     # the project's parity bar


def _bar(want):
    return BAR * max(1.0, want.abs().max().item())


def _frames(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, size, size, generator=g).clamp(-1, 1)   # the range Normalize(0.5, 0.5) produces


@functools.lru_cache(maxsize=None)
def _case(cfg_key, hostile, n=3, seed=11):
    """(cfg, state dict, frames, oracle tokens after the last block, oracle raw features): computed once, shared, never modified"""
    cfg = PE_VISION_CONFIGS[cfg_key] if isinstance(cfg_key, str) else PEVisionConfig(**dict(cfg_key))
    sd = init_vision_state_dict(cfg, seed=seed)
    if hostile:
        sd = make_hostile_vision(sd, cfg, seed=0)
    x = _frames(n, cfg.image_size, seed + 1)
    taps = {}
    with torch.inference_mode():
        feats = V.vision_tower(sd, cfg, x, taps)
    tok = taps[f"layer{cfg.layers - 1}"] if cfg.layers else taps["embed"]
    return cfg, sd, x, tok, feats


def _key(cfg):
    return tuple(sorted(dataclasses.asdict(cfg).items()))


def _encode(cfg, sd, x, precision, gpu, **kw):
    tower = PEVisionTower(cfg, precision=precision, device=str(gpu), **kw)
    tower.load_state_dict(sd)
    raw, tok = tower.encode_image(x.to(gpu), normalize=False, return_tokens=True)
    nrm = tower.encode_image(x.to(gpu), normalize=True)
    return tok.cpu(), raw.cpu(), nrm.cpu()


def _errs(got, want_tok, want_raw):
    tok, raw, nrm = got
    want_nrm = torch.nn.functional.normalize(want_raw, dim=-1)
    return ((tok - want_tok).abs().max().item(), (raw - want_raw).abs().max().item(), (nrm - want_nrm).abs().max().item())


# ---------------------------------------------------------------------------------------------------- 1: tower parity
# Errors measured on MI355X in this change (max-abs; tokens / raw features / normalised features), profiles/vit_x3/gpu_tests.log.
# The asserted bound is 2x the measured error, and never above the bar 1e-3 x max(1, |ref|).
MEASURED = {
    # (precision, config, hostile): (tokens, raw features, normalised features)          |tokens| <= / the plain mode's token error
    ("fp16x3", "pe-tiny", False): (3.099e-06, 6.743e-07, 3.558e-07),                    # 4.08
    ("bf16x3", "pe-tiny", False): (8.583e-06, 2.444e-06, 1.304e-06),
    ("fp16x3", "pe-tiny", True): (3.624e-05, 8.047e-07, 3.502e-07),                     # 41.07 / fp16 2.7e-2
    ("bf16x3", "pe-tiny", True): (4.177e-04, 1.037e-05, 4.336e-06),                     #         bf16 2.5e-1
    ("fp16x3", "pe-mini", False): (4.530e-06, 7.153e-07, 3.874e-07),                    # 4.97
    ("bf16x3", "pe-mini", False): (1.073e-05, 2.168e-06, 9.164e-07),
    ("fp16x3", "pe-mini", True): (1.755e-04, 1.222e-06, 3.874e-07),                     # 60.79 / fp16 1.1e-1
    ("bf16x3", "pe-mini", True): (1.403e-03, 7.182e-06, 2.056e-06),                     #         bf16 1.2
}


def _bounds(prec, name, hostile, want_tok, want_raw):
    bars = (_bar(want_tok), _bar(want_raw), BAR)
    m = MEASURED.get((prec, name, hostile))
    return bars if m is None else tuple(min(2 * e, b) for e, b in zip(m, bars))


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("hostile", [False, True], ids=["benign", "hostile"])
@pytest.mark.parametrize("name", ["pe-tiny", "pe-mini"])
def test_tower_x3_matches_oracle(gpu, prec, name, hostile):
    """pe-tiny / pe-mini, seeded and trained-like (make_hostile_vision) weights, 3 frames: tokens after the last block, raw and
    L2-normalised features against the fp32 CPU oracle.  On the hostile set the plain 16-bit mode of the same library runs beside
    it and the x3 error must be at most a tenth of its error: the compensated path is what ran."""
    cfg, sd, x, want_tok, want_raw = _case(name, hostile)
    e = _errs(_encode(cfg, sd, x, prec, gpu), want_tok, want_raw)
    b = _bounds(prec, name, hostile, want_tok, want_raw)
    print(f"vit x3 {prec} {name} {'hostile' if hostile else 'benign'}: tokens {e[0]:.3e} (|ref| <= {want_tok.abs().max():.2f}, bound "
          f"{b[0]:.1e}), raw features {e[1]:.3e} (|ref| <= {want_raw.abs().max():.2f}, bound {b[1]:.1e}), normalised features {e[2]:.3e} "
          f"(bound {b[2]:.1e})")
    if hostile:
        p = _errs(_encode(cfg, sd, x, PLAIN[prec], gpu), want_tok, want_raw)
        print(f"vit plain {PLAIN[prec]} {name} hostile: tokens {p[0]:.3e}, raw features {p[1]:.3e}, normalised features {p[2]:.3e}; "
              f"plain / x3 = {p[0] / e[0]:.0f} / {p[1] / e[1]:.0f} / {p[2] / e[2]:.0f}")
        assert e[0] <= p[0] / 10 and e[2] <= p[2] / 10, "the x3 error is not a tenth of the plain 16-bit mode's"
    assert all(b_ <= bar for b_, bar in zip(b, (_bar(want_tok), _bar(want_raw), BAR)))
    assert e[0] <= b[0] and e[1] <= b[1] and e[2] <= b[2]


# ---------------------------------------------------------------------------------------------------- 2: structure flags
FLAGS = [("pe-mini", dict(heads=2)), ("pe-tiny", dict(pool_type="tok")), ("pe-tiny", dict(pool_type="avg")),
         ("pe-tiny", dict(use_rope2d=False)), ("pe-tiny", dict(act="quick_gelu")),
         ("pe-tiny", dict(use_cls_token=False, pool_type="avg")), ("pe-tiny", dict(use_ln_pre=False)),
         ("pe-tiny", dict(use_ln_post=False))]


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("base,change", FLAGS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for _, c in FLAGS])
def test_tower_x3_structure_flags(gpu, prec, base, change):
    """every structural switch under x3: 128-wide heads (pe-mini with 2 heads), pooling types, no RoPE, quick GELU, no class token,
    no ln_pre / ln_post (without ln_post the pooling head's k|v launch splits the residual stream itself)"""
    cfg = dataclasses.replace(PE_VISION_CONFIGS[base], **change)
    cfg, sd, x, want_tok, want_raw = _case(_key(cfg), False, 2, 21)
    e = _errs(_encode(cfg, sd, x, prec, gpu), want_tok, want_raw)
    print(f"vit x3 {prec} flags {change}: tokens {e[0]:.3e}, raw features {e[1]:.3e}, normalised features {e[2]:.3e}")
    assert e[0] <= _bar(want_tok) and e[1] <= _bar(want_raw) and e[2] <= BAR


@pytest.mark.parametrize("prec", X3)
def test_tower_x3_per_class_masks(gpu, prec):
    """Every bit of SAMAUDIO_CLS_X3_VIT alone, and all of them but wo / but w13 (the scratch rows are shared between the LayerNorm
    output and the attention's split output; without w13 c_proj's operand is split from c_fc's fp32 output), on pe-tiny.  Only the
    twins of the classes that are on are registered; finalize takes that.  The classes left in fp32 are exact: same bar."""
    cfg, sd, x, want_tok, want_raw = _case("pe-tiny", False)
    single = [hip.CLS[b] for b in ("qkv", "wo", "w13", "w2")] + [hip.X3_ATTENTION]
    assert sum(single) == hip.CLS_X3_VIT
    for classes in single + [hip.CLS_X3_VIT & ~hip.CLS["wo"], hip.CLS_X3_VIT & ~hip.CLS["w13"]]:
        e = _errs(_encode(cfg, sd, x, prec, gpu, x3_classes=classes), want_tok, want_raw)
        print(f"vit x3 {prec} classes {classes:#x}: tokens {e[0]:.3e}, raw features {e[1]:.3e}, normalised features {e[2]:.3e}")
        assert e[0] <= _bar(want_tok) and e[1] <= _bar(want_raw) and e[2] <= BAR, hex(classes)


# ---------------------------------------------------------------------------------------------------- 3: full width
@pytest.mark.skipif(SIM, reason="PE-Core-L width on the 256x256 sharing walk: MI355X only")
@pytest.mark.parametrize("prec", X3)
def test_tower_x3_one_layer_at_full_width(gpu, prec):
    """One block at PE-Core-L width (1024, 16 x 64 heads, mlp 4096) on 56 x 56 frames (17 tokens), 20 frames: M = 340 rows = one whole
    256-row tile plus a partial one, N = 3072 / 1024 / 4096 on the operand-sharing walk."""
    cfg = PEVisionConfig(image_size=56, patch_size=14, width=1024, layers=1, heads=16, output_dim=256)
    cfg, sd, x, want_tok, want_raw = _case(_key(cfg), False, 20, 41)
    e = _errs(_encode(cfg, sd, x, prec, gpu), want_tok, want_raw)
    print(f"vit x3 {prec} full width, 1 layer, M = {20 * cfg.tokens}: tokens {e[0]:.3e} (|ref| <= {want_tok.abs().max():.2f}), raw "
          f"features {e[1]:.3e} (|ref| <= {want_raw.abs().max():.2f}), normalised features {e[2]:.3e}")
    assert e[0] <= _bar(want_tok) and e[1] <= _bar(want_raw) and e[2] <= BAR


# ---------------------------------------------------------------------------------------------------- 4: kernels, bitwise
def _bits(t):
    return t.cpu().view(torch.int16)


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("D", [128, 1024, 1536])
def test_layernorm_rows_split3_is_layernorm_then_split3(gpu, prec, D, strided):
    """samaudio_op_layernorm_rows_split3 against samaudio_op_layernorm_rows (fp32 output) followed by samaudio_op_split3: the same
    bits.  5 rows (one whole workgroup of 4 and a partial one), rows contiguous or 3 D apart (the class-token rows of a tower);
    D = 1536 takes the 8-registers-per-lane instantiation.  Column scales put values beyond IEEE half's range (the clamp of hi)."""
    lib = hip.lib(hip.operands_for(prec))
    M, ld = 5, (3 * D if strided else D)
    g = torch.Generator().manual_seed(D + strided)
    x = torch.randn(M, ld, generator=g) * 2 + 0.5
    w = (torch.randn(D, generator=g) * 0.3 + 1) * torch.logspace(-3, 5.2, D)
    b = torch.randn(D, generator=g) * 0.1
    xd, wd, bd = x.to(gpu).contiguous(), w.to(gpu), b.to(gpu)
    o32 = torch.full((M, D), float("nan"), device=gpu)
    hip.check(lib.samaudio_op_layernorm_rows(hip.ptr(xd), ld, hip.ptr(wd), hip.ptr(bd), hip.ptr(o32), None, hip.F32, M, D, 1e-5,
                                             util.stream()))
    want = torch.full((M, 3 * D), float("nan"), dtype=HALF[prec], device=gpu)
    hip.check(lib.samaudio_op_split3(hip.ptr(o32), D, hip.ptr(want), M, D, util.stream()))
    got = torch.full((M + 1, 3 * D), float("nan"), dtype=HALF[prec], device=gpu)   # one canary row behind
    hip.check(lib.samaudio_op_layernorm_rows_split3(hip.ptr(xd), ld, hip.ptr(wd), hip.ptr(bd), hip.ptr(got), M, D, 1e-5, util.stream()))
    assert torch.isnan(got[M].float()).all(), "a row past M was written"
    assert not torch.isnan(got[:M].float()).any()
    ref = torch.nn.functional.layer_norm(x[:, :D], (D,), w, b, 1e-5)
    assert (o32.cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    assert torch.equal(_bits(got[:M]), _bits(want))
    assert lib.samaudio_op_layernorm_rows_split3(hip.ptr(xd), ld, hip.ptr(wd), hip.ptr(bd), hip.ptr(got), M, 4096, 1e-5,
                                                 util.stream()) == hip.ERR_ARG


@pytest.mark.parametrize("prec", X3)
@pytest.mark.parametrize("variant", [hip.GV_GEMM8_256x256, hip.GV_GEMM8S_128x128])
@pytest.mark.parametrize("act", [hip.ACT_NONE, hip.ACT_GELU, hip.ACT_QUICK_GELU], ids=["none", "gelu", "quick_gelu"])
def test_gemm8_bias_act_split3_epilogue_is_fp32_output_then_split3(gpu, prec, act, variant):
    """GEMM_FLAG_OUT_SPLIT3 on a launch without SwiGLU - v = act(acc + bias) written as [lo | hi | hi] rows of 3 N elements by the
    register epilogue - against the same launch with an fp32 output through the general epilogue followed by samaudio_op_split3:
    the same bits.  M = 340 (a whole 256-row tile and a partial one), N = 512, K' = 3 x 256 compensated operands, both 8-phase
    kernels, the plain walk over K' and the operand-sharing one.  A flagged launch with a residual is refused."""
    lib = hip.lib(hip.operands_for(prec))
    M, N, K = 340, 512, 256
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, K, generator=g) * torch.logspace(-1, 1, K)[None, :]
    w = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    xd, bd = x.to(gpu).contiguous(), bias.to(gpu)
    a3 = torch.empty(M, 3 * K, dtype=HALF[prec], device=gpu)
    hip.check(lib.samaudio_op_split3(hip.ptr(xd), K, hip.ptr(a3), M, K, util.stream()))
    w3 = x3_weight(w, HALF[prec], ktm=False).to(gpu)
    ref = torch.nn.functional.linear(x.double(), w.double(), bias.double())
    ref = {hip.ACT_NONE: ref, hip.ACT_GELU: torch.nn.functional.gelu(ref), hip.ACT_QUICK_GELU: ref * torch.sigmoid(1.702 * ref)}[act]
    lib.samaudio_debug_force_gemm_variant(variant)
    try:
        for share in (0, hip.GEMM_FLAG_X3_SHARE):
            o32 = torch.full((M, N), float("nan"), device=gpu)
            util.gemm(PLAIN[prec], a3, w3, M, N, 3 * K, bias=bd, out_f32=o32, f32_geom=(0, N, 0), act=act, f32_act=1, flags=share)
            want = torch.full((M, 3 * N), float("nan"), dtype=HALF[prec], device=gpu)
            hip.check(lib.samaudio_op_split3(hip.ptr(o32), N, hip.ptr(want), M, N, util.stream()))
            got = torch.full((M + 1, 3 * N), float("nan"), dtype=HALF[prec], device=gpu)   # one canary row behind
            util.gemm(PLAIN[prec], a3, w3, M, N, 3 * K, bias=bd, out_act=got, act_geom=(0, 3 * N, 0), act=act,
                      flags=share | hip.GEMM_FLAG_OUT_SPLIT3)
            assert torch.isnan(got[M].float()).all(), "a row past M was written"
            err = (o32.cpu().double() - ref).abs().max().item()
            print(f"gemm8 split3 epilogue {prec} act {act} variant {variant} share {share != 0}: fp32 launch vs float64 {err:.3e} "
                  f"(|ref| <= {ref.abs().max():.2f})")
            assert err <= 1e-3 * ref.abs().max().item()
            assert torch.equal(_bits(got[:M]), _bits(want)), f"share {share != 0}"
        res = torch.zeros(M, N, device=gpu)
        p = util.gemm_params(a3, w3, M, N, 3 * K, bias=bd, res=res, res_geom=(0, N, 0), out_act=got, act_geom=(0, 3 * N, 0), act=act,
                             flags=hip.GEMM_FLAG_OUT_SPLIT3)
        assert lib.samaudio_op_gemm(C.byref(p), C.sizeof(p), hip.BF16, util.stream()) == hip.ERR_ARG
        assert "split3" in lib.samaudio_last_error().decode()
    finally:
        lib.samaudio_debug_force_gemm_variant(-1)


# ---------------------------------------------------------------------------------------------------- 5: plumbing
@pytest.mark.parametrize("prec", X3)
def test_tower_x3_workspace_is_exactly_what_the_plan_takes(gpu, prec):
    """An encode in a NaN-poisoned buffer of exactly samaudio_vit_workspace_bytes followed by a canary tail: the same bits as through
    the class's own workspace, the canary intact; one plan unit less is refused with SAMAUDIO_ERR_WORKSPACE.  The x3 plan is larger
    than the fp32 plan by the split scratch."""
    cfg, sd, x, want_tok, want_raw = _case("pe-tiny", False)
    tower = PEVisionTower(cfg, precision=prec, device=str(gpu))
    tower.load_state_dict(sd)
    xd = x.to(gpu).contiguous()
    n = xd.shape[0]
    want = tower.encode_image(xd, normalize=True).cpu()
    lib = tower._lib
    need = lib.samaudio_vit_workspace_bytes(tower._h, n)
    plain = PEVisionTower(cfg, precision="fp32", device=str(gpu))
    M, W, F = n * cfg.tokens, cfg.width, cfg.mlp_width
    assert need >= lib.samaudio_vit_workspace_bytes(plain._h, n) + M * 3 * W * 2 + M * 3 * F * 2
    canary = 1 << 20
    buf = torch.full((need + 256 + canary,), 255, dtype=torch.uint8, device=gpu)   # 0xFF bytes: NaN as fp32 and as 16-bit
    off = (-buf.data_ptr()) % 256
    feats = torch.empty(n, cfg.output_dim, device=gpu)

    def encode(nbytes):
        hip.check(lib.samaudio_vit_set_workspace(tower._h, C.c_void_p(buf.data_ptr() + off), nbytes))
        hip.check(lib.samaudio_vit_encode(tower._h, hip.ptr(xd), n, 1, hip.ptr(feats), None, util.stream()))

    with pytest.raises(hip.SamAudioHipError, match=r"\[-3\]"):
        encode(need - 256)   # the plan is carved in 256-byte units
    encode(need)
    assert torch.equal(feats.cpu(), want)
    tail = buf[off + need:].cpu()
    assert (tail == 255).all(), f"{int((tail != 255).sum())} canary bytes behind a {need}-byte workspace were written"
    print(f"vit x3 workspace ({n} frames of pe-tiny, {prec}): {need} bytes")
    tower._workspace = None   # the class sizes and hands over its own buffer again on the next call


@pytest.mark.parametrize("prec", X3)
def test_tower_x3_ragged_frame_counts_share_one_workspace(gpu, prec):
    """1, 5, 2 frames through one x3 tower: the workspace (split scratch included) is re-planned; rows are independent, bit for bit"""
    cfg = PE_VISION_CONFIGS["pe-tiny"]
    sd = init_vision_state_dict(cfg, seed=3)
    tower = PEVisionTower(cfg, precision=prec, device=str(gpu))
    tower.load_state_dict(sd)
    x = _frames(5, cfg.image_size, 4)
    one = tower.encode_image(x[:1].to(gpu), normalize=True).cpu()
    full = tower.encode_image(x.to(gpu), normalize=True).cpu()
    two = tower.encode_image(x[3:].to(gpu), normalize=True).cpu()
    assert torch.equal(one, full[:1]) and torch.equal(two, full[3:])


@pytest.mark.parametrize("prec", X3)
def test_tower_x3_two_streams_are_bitwise_equal_to_one(gpu, prec):
    """64 frames of pe-tiny as two halves on two HIP streams / engine contexts (the option is set on the side context too, before its
    finalize) against one stream: frames are independent, so the same bits"""
    if gpu.type != "cuda":
        pytest.skip("needs real HIP streams")
    cfg = PE_VISION_CONFIGS["pe-tiny"]
    sd = init_vision_state_dict(cfg, seed=13)
    x = _frames(64, cfg.image_size, 14).to(gpu)
    outs = []
    for streams in (1, 2):
        tower = PEVisionTower(cfg, precision=prec, device=str(gpu), streams=streams)
        tower.load_state_dict(sd)
        outs.append(tower.encode_image(x, normalize=True).cpu())
        assert (tower._side is not None) == (streams == 2)
    assert torch.equal(outs[0], outs[1])


def test_option_value_0_is_the_fp32_tower_bit_for_bit(gpu):
    """SAMAUDIO_OPT_X3_CLASSES = 0 on an fp32 context: the launches, the workspace and the bits of a context that never set it"""
    cfg, sd, x, _, _ = _case("pe-tiny", False)
    never = PEVisionTower(cfg, precision="fp32", device=str(gpu))
    zero = PEVisionTower(cfg, precision="fp32", device=str(gpu))
    assert zero._lib.samaudio_vit_set_option(zero._h, hip.OPT_X3_CLASSES, hip.CLS_X3_VIT) == 0
    assert zero._lib.samaudio_vit_set_option(zero._h, hip.OPT_X3_CLASSES, 0) == 0
    outs = []
    for tower in (never, zero):
        tower.load_state_dict(sd)
        f, t = tower.encode_image(x.to(gpu), normalize=True, return_tokens=True)
        outs.append((f.cpu(), t.cpu()))
    assert zero._lib.samaudio_vit_workspace_bytes(zero._h, 3) == never._lib.samaudio_vit_workspace_bytes(never._h, 3)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_vit_x3_option_errors(gpu):
    """No launch: the option on a 16-bit context, another option and a foreign bit are SAMAUDIO_ERR_ARG; finalize without a twin of a
    class that is switched on is SAMAUDIO_ERR_WEIGHT and names the twin; the option un-finalizes a context."""
    cfg, sd, x, _, _ = _case("pe-tiny", False)
    lib = hip.lib()
    t16 = PEVisionTower(cfg, precision="bf16", device=str(gpu))
    assert lib.samaudio_vit_set_option(t16._h, hip.OPT_X3_CLASSES, hip.CLS["qkv"]) == hip.ERR_ARG
    assert "fp32 contexts" in lib.samaudio_last_error().decode()
    t32 = PEVisionTower(cfg, precision="fp32", device=str(gpu))
    for bit in ("patch", "cwq", "cwo", "ckv", "codec", "out"):
        assert lib.samaudio_vit_set_option(t32._h, hip.OPT_X3_CLASSES, hip.CLS_X3_VIT | hip.CLS[bit]) == hip.ERR_ARG, bit
    assert lib.samaudio_vit_set_option(t32._h, hip.OPT_TAIL_SPLIT, 0) == hip.ERR_ARG
    assert lib.samaudio_vit_set_option(None, hip.OPT_X3_CLASSES, 0) == hip.ERR_ARG
    # a missing twin: the fp32 tensors alone, class w2 on
    assert lib.samaudio_vit_set_option(t32._h, hip.OPT_X3_CLASSES, hip.CLS["w2"]) == 0
    t32.register(convert_vision(sd, cfg, torch.float32, gpu))
    assert lib.samaudio_vit_finalize(t32._h) == hip.ERR_WEIGHT
    assert "L0.w2.x3" in lib.samaudio_last_error().decode()
    assert lib.samaudio_vit_set_option(t32._h, hip.OPT_X3_CLASSES, hip.CLS["qkv"]) == 0
    assert lib.samaudio_vit_finalize(t32._h) == hip.ERR_WEIGHT
    assert "L0.wqkv.x3" in lib.samaudio_last_error().decode()
    assert lib.samaudio_vit_set_option(t32._h, hip.OPT_X3_CLASSES, 0) == 0
    feats = torch.empty(1, cfg.output_dim, device=gpu)
    xd = x[:1].to(gpu).contiguous()
    assert lib.samaudio_vit_encode(t32._h, hip.ptr(xd), 1, 1, hip.ptr(feats), None, util.stream()) == hip.ERR_STATE, \
        "setting the option marks the context as not finalized"
    assert lib.samaudio_vit_finalize(t32._h) == 0, "with the mask at 0 the fp32 tensors alone finalize"
    with pytest.raises(ValueError):
        PEVisionTower(cfg, precision="bf16x3", device=str(gpu), x3_classes="patch")


def test_samaudio_tower_precision_reaches_the_vision_encoder(gpu):
    """SAMAudio(..., tower_precision="bf16x3") loading a checkpoint that carries `vision_encoder.*` builds an x3 tower whose features
    are the oracle's to the bar; tower_precision=None builds what it built before: the plain 16-bit tower beside an x3 DiT."""
    from sam_audio_amd import SAMAudio, preset_config
    from sam_audio_amd.synthetic import init_state_dict
    pe = PE_VISION_CONFIGS["pe-tiny"]
    cfg = preset_config("tiny")
    cfg.vision_encoder = PerceptionEncoderConfig(dim=pe.output_dim, batch_size=3, name="pe-tiny", image_size=pe.image_size)
    _, vsd, x, _, want_raw = _case("pe-tiny", False)
    full = dict(init_state_dict(cfg, seed=3))
    full.update({"vision_encoder.model.visual." + k: v for k, v in vsd.items()})
    model = SAMAudio(cfg, precision="bf16x3", device=str(gpu), tower_precision="bf16x3")
    model.load_state_dict(full, strict=True)
    tower = model.vision_encoder.tower
    assert tower.precision == "bf16x3" and tower.x3_classes == hip.CLS_X3_VIT and tower.act_dtype == torch.float32
    assert "L0.wqkv.x3" in tower._tensors and "pool.wkv.x3" in tower._tensors
    got = tower.encode_image(x.to(gpu), normalize=True).cpu()
    util.report("SAMAudio's x3 vision tower, normalised features", got, torch.nn.functional.normalize(want_raw, dim=-1), BAR)
    default = SAMAudio(cfg, precision="bf16x3", device=str(gpu))
    default.load_state_dict(full, strict=True)
    assert default.tower_precision is None
    assert default.vision_encoder.tower.precision == hip.tower_precision("bf16x3") == "bf16"
    assert default.vision_encoder.tower.x3_classes == 0 and "L0.wqkv.x3" not in default.vision_encoder.tower._tensors
    with pytest.raises(ValueError):
        SAMAudio(cfg, precision="bf16x3", device=str(gpu), tower_precision="fp8")
