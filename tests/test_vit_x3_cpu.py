"""CPU side of the compensated PE-Core vision tower (tests/test_vit_x3_gpu.py is the GPU side): the split twins convert_vision
makes, the hostile tower weight set as a yardstick, the host-side error paths that need no library, and part of the GPU file on the
functional SIMT simulator (bf16x3: the simulator build is the bfloat16 library)."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

from oracle import vit_oracle as V
from sam_audio_amd import hip
from sam_audio_amd.config import PE_VISION_CONFIGS
from sam_audio_amd.synthetic import init_vision_state_dict, make_hostile_vision
from sam_audio_amd.vision_tower import PEVisionTower, convert_vision
from sam_audio_amd.weights import ktm_to_rows
from tests.test_towers_x3_cpu import _f64, _oracle_in_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_FILE = "tests/test_vit_x3_gpu.py"


# ---------------------------------------------------------------------------------------------------- twins
@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
def test_vision_twins_reconstruct_the_fp32_weights(half):
    """Every "<name>.x3" twin of convert_vision is [W_hi | W_lo | W_hi] of its fp32 weight - row-major, or K-tile-major where the
    8-phase family takes the launch (N >= 256) -, hi = rn16(W), hi + lo = W to the split bound (2^-21 relative for IEEE half with half
    a subnormal quantum as floor, 2^-15 for bfloat16); a class mask makes only that class's twins; 16-bit contexts get none."""
    cfg = PE_VISION_CONFIGS["pe-tiny"]
    sd = init_vision_state_dict(cfg, seed=5)
    t = convert_vision(sd, cfg, torch.float32, "cpu", half)
    plain = convert_vision(sd, cfg, torch.float32, "cpu")
    assert not any(k.endswith(".x3") for k in plain)
    assert all(torch.equal(t[k], v) for k, v in plain.items()), "the fp32 tensors are the ones an fp32 tower registers"
    rel, floor = (2.0 ** -21, 2.0 ** -25) if half == torch.float16 else (2.0 ** -15, 0.0)
    names = [f"L{i}.{leaf}" for i in range(cfg.layers) for leaf in ("wqkv", "wo", "w1", "w2")] + ["pool.wkv"]
    assert sorted(k for k in t if k.endswith(".x3")) == sorted(n + ".x3" for n in names)
    for name in names:
        w, w3 = t[name], t[name + ".x3"]
        n, k = w.shape
        assert w3.dtype == half and (w3.dim() == 3) == (n >= 256), name
        w3 = ktm_to_rows(w3) if w3.dim() == 3 else w3
        assert w3.shape == (n, 3 * k), name
        hi, lo, hi2 = w3[:, :k].float(), w3[:, k:2 * k].float(), w3[:, 2 * k:].float()
        assert torch.equal(hi, hi2) and torch.equal(hi, w.to(half).float()), name
        assert ((hi + lo - w).abs() <= (w.abs() * rel).clamp_min(floor)).all(), name
    W, F = cfg.width, cfg.mlp_width
    assert ktm_to_rows(t["L0.wqkv.x3"]).shape == (3 * W, 3 * W) and t["L0.wo.x3"].shape == (W, 3 * W)
    assert ktm_to_rows(t["L0.w1.x3"]).shape == (F, 3 * W) and t["L0.w2.x3"].shape == (W, 3 * F)
    only = convert_vision(sd, cfg, torch.float32, "cpu", half, hip.CLS["w2"] | hip.X3_ATTENTION)
    assert sorted(k for k in only if k.endswith(".x3")) == ["L0.w2.x3", "L1.w2.x3"]
    tok_cfg = dataclasses.replace(cfg, pool_type="tok")   # no pooling head: no pool.wkv twin
    assert "pool.wkv.x3" not in convert_vision(init_vision_state_dict(tok_cfg, seed=5), tok_cfg, torch.float32, "cpu", half)
    with pytest.raises(ValueError):
        convert_vision(sd, cfg, torch.bfloat16, "cpu", half)


def test_vision_class_mask_and_precision_mapping():
    assert hip.CLS_X3_VIT == hip.CLS["qkv"] | hip.CLS["wo"] | hip.CLS["w13"] | hip.CLS["w2"] | hip.X3_ATTENTION
    assert hip.CLS_X3_VIT == hip.CLS_X3_TOWER & ~hip.CLS["patch"]
    assert hip.X3_VIT_WEIGHTS == {"wqkv": "qkv", "wo": "wo", "w1": "w13", "w2": "w2"}
    assert "samaudio_vit_set_option" in hip.EXPORTED_SYMBOLS and "samaudio_op_layernorm_rows_split3" in hip.EXPORTED_SYMBOLS
    # the DEFAULT mapping of the towers beside the DiT does not move
    assert [hip.tower_precision(p) for p in ("bf16", "fp16", "mixed", "fp32", "fp16x3", "bf16x3")] == \
        ["bf16", "fp16", "mixed", "fp32", "fp16", "bf16"]


# ---------------------------------------------------------------------------------------------------- hostile yardstick
@pytest.mark.parametrize("name", ["pe-tiny", "pe-mini"])
def test_hostile_vision_weights_are_finite_and_a_sound_yardstick(name):
    """make_hostile_vision: finite in fp32, really hostile (outlier rows x 30, ln gains spread), the input not modified, and the fp32
    oracle on it agrees with the same oracle in float64 to 1e-4 x max(1, |value|) - tokens after the last block, raw and normalised
    features - otherwise it could not judge a 1e-3 bar."""
    cfg = PE_VISION_CONFIGS[name]
    base = init_vision_state_dict(cfg, seed=11)
    keep = {k: v.clone() for k, v in base.items()}
    sd = make_hostile_vision(base, cfg, seed=0)
    assert sorted(sd) == sorted(base) and all(torch.equal(base[k], keep[k]) for k in base), "the input is not modified"
    assert all(torch.isfinite(v).all() for v in sd.values())
    for key in ("conv1.weight", "transformer.resblocks.0.attn.out_proj.weight", f"transformer.resblocks.{cfg.layers - 1}.mlp.c_proj.weight"):
        ratio = sd[key].flatten(1).abs().amax(1) / base[key].flatten(1).abs().amax(1)
        assert (ratio > 29).sum() == 4 and (ratio < 1.01).sum() == ratio.numel() - 4, key
    rb = sd["transformer.resblocks.0.mlp.c_proj.bias"] / base["transformer.resblocks.0.mlp.c_proj.bias"]
    assert ((rb - 30).abs() < 1e-3).sum() == 4
    gain = sd["transformer.resblocks.0.ln_1.weight"] / base["transformer.resblocks.0.ln_1.weight"]
    assert gain.max() / gain.min() > 5
    assert torch.equal(sd["ln_pre.weight"], base["ln_pre.weight"]) and torch.equal(sd["proj"], base["proj"])
    assert not torch.equal(make_hostile_vision(base, cfg, seed=1)["conv1.weight"], sd["conv1.weight"])
    g = torch.Generator().manual_seed(12)
    x = torch.randn(3, 3, cfg.image_size, cfg.image_size, generator=g).clamp(-1, 1)
    t32, t64 = {}, {}
    with torch.inference_mode():
        f32 = V.vision_tower(sd, cfg, x, t32)
        with _oracle_in_float64():
            f64 = V.vision_tower(_f64(sd), cfg, x.double(), t64)
    assert f64.dtype == torch.float64
    last = f"layer{cfg.layers - 1}"
    for what, a, b in (("tokens", t32[last], t64[last]), ("raw features", f32, f64),
                       ("normalised features", torch.nn.functional.normalize(f32, dim=-1), torch.nn.functional.normalize(f64, dim=-1))):
        err, top = (a - b).abs().max().item(), b.abs().max().item()
        print(f"hostile {name} {what}: fp32 oracle vs float64 oracle {err:.3e} on |v| <= {top:.3f}")
        assert b.dtype == torch.float64 and err <= 1e-4 * max(1.0, top), what


# ---------------------------------------------------------------------------------------------------- host-side errors
def test_host_side_errors_need_no_library(monkeypatch):
    """Precision and class names are checked before the library is touched."""
    def no_lib(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(hip, "lib", no_lib)
    cfg = PE_VISION_CONFIGS["pe-tiny"]
    with pytest.raises(ValueError, match="precision"):
        PEVisionTower(cfg, precision="fp16x4")
    with pytest.raises(ValueError, match="x3_classes"):
        PEVisionTower(cfg, precision="fp16x3", x3_classes="qkv,patch")
    with pytest.raises(ValueError, match="x3_classes"):
        PEVisionTower(cfg, precision="bf16x3", x3_classes=hip.CLS_X3_VIT | hip.CLS["codec"])
    with pytest.raises(KeyError):
        PEVisionTower(cfg, precision="bf16x3", x3_classes="w1")
    from sam_audio_amd import SAMAudio, preset_config
    with pytest.raises(ValueError, match="precision"):
        SAMAudio(preset_config("tiny"), precision="fp32", tower_precision="x3")


# ---------------------------------------------------------------------------------------------------- simulator run
def test_x3_vision_tower_on_the_simulator():
    """The whole GPU file with every kernel compiled for the host: the split-form LayerNorm and the bias + GELU split epilogue of both
    8-phase kernels bit for bit, the towers against the oracle, the plumbing (the full-width layer and the two-stream case are
    hardware only)."""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", GPU_FILE],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=2400)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert "30 passed, 2 skipped" in tail and "failed" not in tail, tail
