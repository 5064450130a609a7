"""CPU side of the compensated PE-AV towers (tests/test_towers_x3_gpu.py is the GPU side): the host-side twins, the hostile tower
weight set as a yardstick, and the GPU tests themselves on the functional SIMT simulator / in the plain emulation dry run (the
latter links no kernel of this repository: it covers the host sequencing with the weak split-form launcher ABSENT, i.e. the
fp32-write + split3 fallback of peav.hip)."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch

from oracle import gen_golden_judge as G
from oracle import judge_oracle as J
from sam_audio_amd import hip
from sam_audio_amd.config import PEAudioFrameConfig, SAMAudioJudgeConfig
from sam_audio_amd.synthetic import init_frame_state_dict, init_judge_state_dict, make_hostile_peav
from sam_audio_amd.weights import convert_peav_x3, ktm_to_rows, x3_tower_weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_TEXT = dict(G.TINY_TEXT)
GPU_FILE = "tests/test_towers_x3_gpu.py"


def _cfg():
    return SAMAudioJudgeConfig(audio_codec=None, transformer=G.TINY_TC, finetune_transformer=G.TINY_FT, text_model=TINY_TEXT,
                               nth_text_layer=2, bottleneck_dim=64)


# ---------------------------------------------------------------------------------------------------- twins
def _rows(t):
    return ktm_to_rows(t) if t.dim() == 3 else t


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
def test_tower_twins_reconstruct_the_fp32_weights(half):
    """Every "<name>.x3" twin is [W_hi | W_lo | W_hi] of its fp32 weight (the convolutions per tap), hi + lo = W to the split bound
    (2^-21 relative for IEEE half with half a subnormal quantum as floor, 2^-15 for bfloat16); the ".gs" tables are [gain | 0]."""
    from sam_audio_amd.judge import convert_judge, convert_judge_x3
    cfg = _cfg()
    sd = init_judge_state_dict(cfg, seed=9, with_codec=False)
    t = convert_judge(sd, cfg, torch.float32, "cpu")
    x3 = convert_judge_x3(t, cfg, half)
    rel, floor = (2.0 ** -21, 2.0 ** -25) if half == torch.float16 else (2.0 ** -15, 0.0)

    def check(w, w3, name):
        n, k = w.shape
        assert w3.dtype == half and w3.shape == (n, 3 * k), name
        hi, lo, hi2 = w3[:, :k].float(), w3[:, k:2 * k].float(), w3[:, 2 * k:].float()
        assert torch.equal(hi, hi2) and torch.equal(hi, w.to(half).float()), name
        assert ((hi + lo - w).abs() <= (w.abs() * rel).clamp_min(floor)).all(), name

    names = []
    for P, tc in (("t.", cfg.transformer), ("ft.", cfg.finetune_transformer)):
        D = tc.hidden_size
        for i in range(tc.num_hidden_layers):
            for leaf in ("wqkv", "wo", "w13", "w2"):
                names.append(f"{P}L{i}.{leaf}")
            for norm in ("attn_norm", "ffn_norm"):
                gs = x3[f"{P}L{i}.{norm}.gs"]
                assert gs.shape == (2, D) and torch.equal(gs[0], t[f"{P}L{i}.{norm}"]) and (gs[1] == 0).all()
        names.append(P + "out.w")
        assert torch.equal(x3[P + "norm.gs"][0], t[P + "norm"]) and (x3[P + "norm.gs"][1] == 0).all()
        for n in (1, 2):   # per tap: [D, 3 taps x 3D]
            w, w3 = t[f"{P}conv{n}.w"], _rows(x3[f"{P}conv{n}.w.x3"])
            assert w3.shape == (D, 9 * D)
            for j in range(3):
                check(w[:, j * D:(j + 1) * D], w3[:, 3 * j * D:3 * (j + 1) * D], f"{P}conv{n}.w tap {j}")
    names += ["cat.wh", "cat.wi"]
    for name in names:
        check(t[name], _rows(x3[name + ".x3"]), name)
    assert len(x3) == len(names) + 2 * 2 + 2 * (2 + 1) + 2, sorted(x3)   # + conv twins, two gs tables per layer (2 + 1 layers), final norms
    # K-tile-major exactly where the 8-phase family takes the launch (N >= 256)
    assert x3["t.L0.wqkv.x3"].dim() == 3 and x3["cat.wh.x3"].dim() == 2
    assert x3_tower_weight(torch.randn(256, 64), half).shape == (3, 256, 64)
    # a subset of classes makes only that subset's tensors
    only = convert_peav_x3(t, "t.", 2, half, hip.CLS["w2"])
    assert sorted(only) == ["t.L0.w2.x3", "t.L1.w2.x3"]


def test_tower_precision_mapping_is_unchanged():
    assert [hip.tower_precision(p) for p in ("bf16", "fp16", "mixed", "fp32", "fp16x3", "bf16x3")] == \
        ["bf16", "fp16", "mixed", "fp32", "fp16", "bf16"]
    assert hip.CLS_X3_TOWER == hip.CLS["qkv"] | hip.CLS["wo"] | hip.CLS["w13"] | hip.CLS["w2"] | hip.CLS["patch"] | hip.X3_ATTENTION
    with pytest.raises(ValueError):
        hip.check_precision("fp16x4", x3_ok=True)


# ---------------------------------------------------------------------------------------------------- hostile yardstick
@contextlib.contextmanager
def _oracle_in_float64():
    """The oracle casts with `.float()` in places; for the yardstick check its whole arithmetic must be float64."""
    old = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.Tensor.float = old


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def test_hostile_tower_weights_are_finite_and_a_sound_yardstick():
    """make_hostile_peav: finite in fp32, really hostile (outlier rows, spread gains), and the fp32 oracle on it agrees with the same
    oracle in float64 to 1e-4 x max(1, |value|) - otherwise it could not judge a 1e-3 bar."""
    from tests.test_zz_next_rows_gpu import _judge_case
    cfg = _cfg()
    base = init_judge_state_dict(cfg, seed=9)
    sd = make_hostile_peav(base, "transformer.", cfg.transformer, seed=1, in_proj="data_proj")
    sd = make_hostile_peav(sd, "finetune_transformer.", cfg.finetune_transformer, seed=2, in_proj="finetune_data_proj")
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert sorted(sd) == sorted(base) and base["data_proj.weight"].abs().max() < 1, "the input is not modified"
    ratio = sd["transformer.layers.0.self_attn.o_proj.weight"].abs().amax(1) / base["transformer.layers.0.self_attn.o_proj.weight"].abs().amax(1)
    assert (ratio > 29).sum() == 4 and (ratio < 1.01).sum() == ratio.numel() - 4
    gn = sd["transformer.patch_embedder.resnet_block.block1.groupnorm.weight"] / base["transformer.patch_embedder.resnet_block.block1.groupnorm.weight"]
    assert gn.max() / gn.min() > 5
    inp = _judge_case(cfg)
    tm = G.text_tower(cfg)
    pooled = G.text_pooled(tm, cfg, inp["input_ids"], inp["attention_mask"])
    with torch.inference_mode():
        w32 = J.judge_forward(sd, cfg, pooled, inp["input_values"], inp["separated_values"], inp["padding_mask"])
        with _oracle_in_float64():
            w64 = J.judge_forward(_f64(sd), cfg, pooled.double(), inp["input_values"].double(), inp["separated_values"].double(),
                                  inp["padding_mask"])
    assert w64.dtype == torch.float64
    err = (w32 - w64).abs().max().item()
    print(f"hostile judge: fp32 oracle vs float64 oracle {err:.3e} on |scores| <= {w64.abs().max().item():.3f}")
    assert err <= 1e-4 * max(1.0, w64.abs().max().item())

    fcfg = PEAudioFrameConfig(audio=G.TINY_TC, text_model=dict(TINY_TEXT, hidden_size=64), codebook_dim=128)
    g = torch.Generator().manual_seed(6)
    feats, fpooled = torch.randn(3, 50, 128, generator=g), torch.randn(3, fcfg.text_hidden, generator=g)
    pad = torch.arange(50)[None] < torch.tensor([50, 31, 9])[:, None]
    fsd = make_hostile_peav(init_frame_state_dict(fcfg, seed=2), "audio_encoder.", fcfg.audio, seed=3,
                            in_proj="audio_encoder.embedder.data_proj")
    assert all(torch.isfinite(v).all() for v in fsd.values())
    with torch.inference_mode():
        f32 = J.frame_logits(fsd, fcfg, fpooled, feats, pad) * pad
        with _oracle_in_float64():
            f64 = J.frame_logits(_f64(fsd), fcfg, fpooled.double(), feats.double(), pad) * pad
    err = (f32 - f64).abs().max().item()
    print(f"hostile frame logits: fp32 oracle vs float64 oracle {err:.3e} on |logits| <= {f64.abs().max().item():.3f}")
    assert f64.dtype == torch.float64 and err <= 1e-4 * max(1.0, f64.abs().max().item())


# ---------------------------------------------------------------------------------------------------- simulator / emulation runs
def _run(mode, args, timeout, **extra):
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN=mode, **extra)
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", GPU_FILE] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    return tail


def test_x3_towers_on_the_simulator():
    """The new kernel, one transformer, the Judge, the span predictor and the option errors with every kernel compiled for the host
    (bf16x3: the simulator build is the bfloat16 library)."""
    out = _run("simt", ["-k", "masked_groupnorm or peav_transformer_x3 or judge_x3_forward or dedup or frame_x3 or option_errors"], 2400)
    assert "7 passed" in out and "failed" not in out


def test_x3_transformer_on_the_simulator_with_late_dma():
    """SAMAUDIO_SIMT_DMA=late (tests/test_simt_cpu.py): the x3 launches of one transformer with every global_load_lds landing as
    late as the ISA allows."""
    out = _run("simt", ["-k", "peav_transformer_x3"], 1800, SAMAUDIO_SIMT_DMA="late")
    assert "2 passed" in out and "failed" not in out


def test_x3_towers_in_the_emulation_dry_run():
    """No kernel of the product is linked there, so the weak launcher of the split-form GroupNorm is absent: the x3 path runs its
    fallback (fp32 halo buffer + launch_split3) through the Judge and the span predictor, and one transformer under every
    per-class mask."""
    out = _run("1", ["-k", "judge_x3_forward or dedup or frame_x3 or per_class_masks"], 1200)
    assert "4 passed" in out and "failed" not in out
