"""The towers the launcher emulation does not build - vision tower, T5, ModernBERT - on the functional simulator library of one side.

    SAMAUDIO_EMU_DRYRUN=simt SAMAUDIO_EMU_NOBUILD=1 python towers_simt.py <repo root of the side, oracle/_simt built> <out.json>

Runs the tiny configurations of the simulator tests (tests/test_vit_x3_gpu.py, test_t5_gpu.py, test_mbert_gpu.py, whose helpers it
borrows) and writes, per entry, the sha256 of the output bytes, return codes, samaudio_last_error() texts and
samaudio_vit_workspace_bytes.  compare_json.py then compares the two sides entry by entry.  An experiment aid, not a test."""
import hashlib
import json
import os
import sys

root, out = os.path.abspath(sys.argv[1]), sys.argv[2]
assert os.environ.get("SAMAUDIO_EMU_DRYRUN") == "simt"
sys.path.insert(0, root)
os.chdir(root)

import ctypes as C  # noqa: E402

import torch  # noqa: E402

import tests.conftest  # noqa: E402,F401  (binds sam_audio_amd.hip to oracle/_simt/libsamaudio_simt.so of `root`)
from sam_audio_amd import hip  # noqa: E402
from sam_audio_amd.mbert_encoder import MBertDims, ModernBertHIP  # noqa: E402
from sam_audio_amd.t5_encoder import T5Dims, T5EncoderHIP  # noqa: E402
from sam_audio_amd.vision_tower import PEVisionTower, convert_vision  # noqa: E402
from tests import test_mbert_gpu as TM, test_t5_gpu as TT, test_vit_x3_gpu as TV  # noqa: E402

dev = torch.device("cpu")
res = {}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


def err():
    return hip.lib().samaudio_last_error().decode()


# ---- vision tower: fp32, 16-bit, CLS_X3_VIT, each of its five bits alone (pe-tiny; pe-mini for the whole mask too)
cfg, sd, x, _, _ = TV._case("pe-tiny", False)
single = [hip.CLS[b] for b in ("qkv", "wo", "w13", "w2")] + [hip.X3_ATTENTION]
for name, prec, kw in [("fp32", "fp32", {}), ("bf16", "bf16", {}), ("x3 all", "bf16x3", {})] + \
        [(f"x3 {c:#x}", "bf16x3", dict(x3_classes=c)) for c in single + [hip.CLS_X3_VIT & ~hip.CLS["wo"], hip.CLS_X3_VIT & ~hip.CLS["w13"]]]:
    tower = PEVisionTower(cfg, precision=prec, device="cpu", **kw)
    tower.load_state_dict(sd)
    raw, tok = tower.encode_image(x.to(dev), normalize=False, return_tokens=True)
    nrm = tower.encode_image(x.to(dev), normalize=True)
    res[f"vit pe-tiny {name}"] = dict(out=sha(tok, raw, nrm), workspace=[hip.lib().samaudio_vit_workspace_bytes(tower._h, n) for n in (1, 3, 7)])
for key, change in TV.FLAGS:
    c2 = TV.dataclasses.replace(TV.PE_VISION_CONFIGS[key], **change)
    cfg2, sd2, x2, _, _ = TV._case(TV._key(c2), False)
    tok, raw, nrm = TV._encode(cfg2, sd2, x2, "bf16x3", dev)
    res[f"vit {key} {sorted(change.items())} x3 all"] = dict(out=sha(tok, raw, nrm))

# ---- the option / twin / workspace errors of tests/test_vit_x3_gpu.py::test_vit_x3_option_errors, codes and texts
lib = hip.lib()
log = []


def rc(what, code):
    log.append([what, int(code), err() if code else ""])


t16 = PEVisionTower(cfg, precision="bf16", device="cpu")
rc("x3 on a 16-bit context", lib.samaudio_vit_set_option(t16._h, hip.OPT_X3_CLASSES, hip.CLS["qkv"]))
t32 = PEVisionTower(cfg, precision="fp32", device="cpu")
for bit in ("patch", "cwq", "cwo", "ckv", "codec", "out"):
    rc(f"foreign bit {bit}", lib.samaudio_vit_set_option(t32._h, hip.OPT_X3_CLASSES, hip.CLS_X3_VIT | hip.CLS[bit]))
rc("another option", lib.samaudio_vit_set_option(t32._h, hip.OPT_TAIL_SPLIT, 0))
rc("null handle: set_option", lib.samaudio_vit_set_option(None, hip.OPT_X3_CLASSES, 0))
rc("null handle: finalize", lib.samaudio_vit_finalize(None))
rc("null handle: set_workspace", lib.samaudio_vit_set_workspace(None, None, 0))
rc("w2 on", lib.samaudio_vit_set_option(t32._h, hip.OPT_X3_CLASSES, hip.CLS["w2"]))
t32.register(convert_vision(sd, cfg, torch.float32, dev))
rc("finalize without L0.w2.x3", lib.samaudio_vit_finalize(t32._h))
rc("qkv on", lib.samaudio_vit_set_option(t32._h, hip.OPT_X3_CLASSES, hip.CLS["qkv"]))
rc("finalize without L0.wqkv.x3", lib.samaudio_vit_finalize(t32._h))
rc("mask 0", lib.samaudio_vit_set_option(t32._h, hip.OPT_X3_CLASSES, 0))
feats = torch.empty(1, cfg.output_dim)
xd = x[:1].contiguous()
rc("encode before finalize", lib.samaudio_vit_encode(t32._h, hip.ptr(xd), 1, 1, hip.ptr(feats), None, None))
rc("finalize with mask 0", lib.samaudio_vit_finalize(t32._h))
rc("encode without a workspace", lib.samaudio_vit_encode(t32._h, hip.ptr(xd), 1, 1, hip.ptr(feats), None, None))
buf = torch.zeros(1 << 16, dtype=torch.uint8)
off = (-buf.data_ptr()) % 256
rc("misaligned workspace", lib.samaudio_vit_set_workspace(t32._h, C.c_void_p(buf.data_ptr() + off + 8), 1024))
rc("small workspace", lib.samaudio_vit_set_workspace(t32._h, C.c_void_p(buf.data_ptr() + off), 1024))
rc("encode in a small workspace", lib.samaudio_vit_encode(t32._h, hip.ptr(xd), 1, 1, hip.ptr(feats), None, None))
x3t = PEVisionTower(cfg, precision="bf16x3", device="cpu")
x3t.load_state_dict(sd)
need = lib.samaudio_vit_workspace_bytes(x3t._h, 1)
big = torch.zeros(need + 512, dtype=torch.uint8)
boff = (-big.data_ptr()) % 256
rc("x3: one plan unit short", lib.samaudio_vit_set_workspace(x3t._h, C.c_void_p(big.data_ptr() + boff), need - 256))
rc("x3: encode one plan unit short", lib.samaudio_vit_encode(x3t._h, hip.ptr(xd), 1, 1, hip.ptr(feats), None, None))
rc("x3: exact workspace", lib.samaudio_vit_set_workspace(x3t._h, C.c_void_p(big.data_ptr() + boff), need))
rc("x3: encode in the exact workspace", lib.samaudio_vit_encode(x3t._h, hip.ptr(xd), 1, 1, hip.ptr(feats), None, None))
res["vit errors"] = dict(log=log, out=sha(feats), workspace=[need])

# ---- T5 and ModernBERT encoders (the small configurations of their simulator tests), and their error entry points
for kw, B, L in [(TT.SMALL, 4, 40), (dict(TT.SMALL, d_kv=16, num_heads=4, feed_forward_proj="gelu_new"), 2, 150)]:
    for prec in ("fp32", "bf16"):
        m, tc = TT._model(3, **kw)
        ids, mask = TT._inputs(tc, B, L, 4)
        enc = T5EncoderHIP(T5Dims.from_hf(tc), precision=prec, device="cpu")
        enc.load_state_dict(m.state_dict())
        res[f"t5 {kw['feed_forward_proj']} B={B} L={L} {prec}"] = dict(out=sha(enc(ids.to(dev), mask.to(dev))))
log = []
tc = hip.T5Config(precision=hip.F32, vocab=10, d_model=60, d_kv=32, heads=2, d_ff=128, layers=1, max_len=16, act=hip.ACT_RELU, ln_eps=1e-6)
h = C.c_void_p()
rc("t5 create", lib.samaudio_t5_create(C.byref(tc), C.byref(h)))
rc("t5 finalize d_model 60", lib.samaudio_t5_finalize(h))
rc("t5 null handle", lib.samaudio_t5_finalize(None))
lib.samaudio_t5_destroy(h)
rc("mbert null handle", lib.samaudio_mbert_finalize(None))
res["text errors"] = dict(log=log)
# (intermediate 96 is refused by a 16-bit context at finalize - that text is the entry; 128 runs the 16-bit launches)
for kw, B, L in [(TM.SMALL, 3, 40), (dict(TM.SMALL, global_attn_every_n_layers=2, num_hidden_layers=3), 2, 9),
                 (dict(TM.SMALL, intermediate_size=128), 2, 20)]:
    for prec in ("fp32", "bf16"):
        m, mc = TM._model(3, **kw)
        ids, mask = TM._inputs(mc, B, L, 4)
        key = f"mbert layers={mc.num_hidden_layers} F={mc.intermediate_size} B={B} L={L} {prec}"
        try:
            tower = ModernBertHIP.from_module(m, dev, precision=prec)
        except AssertionError as e:
            res[key] = dict(log=[["finalize", -1, str(e)]])
            continue
        outs = [tower(ids.to(dev), mask.to(dev), n, last_prenorm=False) for n in (0, 1, mc.num_hidden_layers, None)]
        res[key] = dict(out=sha(*outs))

json.dump(res, open(out, "w"), indent=1, sort_keys=True)
print(f"{len(res)} entries -> {out}")
