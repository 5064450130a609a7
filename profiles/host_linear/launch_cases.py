"""Runs the comparison cases of the host refactor on ONE logging build of the launcher emulation (build_log_emu.sh):

    python profiles/host_linear/launch_cases.py <libsamaudio_emu_log.so> <out dir>

-> <out dir>/launches.log   one line per launch / memset / copy the host code issued: name and every argument, pointers as
                            <buffer>+<offset>, "## <case>" in front of every case
   <out dir>/results.json   per case: return codes and samaudio_last_error() texts, sha256 of every output tensor, the profile records
                            (name, launches, flops, bytes), the sentinel figures, the workspace sizes asked for
compare.py diffs the two files of the parent commit's build against this tree's.  The folded cross-attention kernels are not emulated:
they are logged and skipped (gen_log_shim.py), which is enough to compare the host sequence around them; the outputs of those cases
are then equal bits of an unfinished computation, not a result."""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.pop("SAMAUDIO_NO_FOLD", None)
from oracle import gen_golden_judge as G  # noqa: E402
from sam_audio_amd import hip, preset_config  # noqa: E402
from sam_audio_amd.config import PEAudioFrameConfig  # noqa: E402
from sam_audio_amd.judge import convert_frame, convert_judge, convert_judge_x3, peav_dims  # noqa: E402
from sam_audio_amd.synthetic import init_frame_state_dict, init_judge_state_dict, init_state_dict  # noqa: E402
from sam_audio_amd.weights import (convert_codec, convert_codec_fly16, convert_codec_x3, convert_dit, convert_dit_x3,  # noqa: E402
                                   convert_peav_x3)

HALF = torch.bfloat16   # the emulation is the bfloat16 library
RESULTS = {}
KEEP = []               # every registered buffer of the running case stays alive (addresses are not reused inside a case)


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in hip._PROTOS.items():
        if not name.startswith(("samaudio_vit_", "samaudio_t5_", "samaudio_mbert_")):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    lib.emu_log_register.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    return lib


def reg(lib, name, t):
    KEEP.append(t)
    lib.emu_log_register(name.encode(), C.c_void_p(t.data_ptr()), t.numel() * t.element_size())
    return t


def begin(lib, case):
    KEEP.clear()
    lib.emu_log_clear()
    lib.emu_log_mark(case.encode())
    RESULTS[case] = {"calls": [], "sha": {}}
    return RESULTS[case]


def call(lib, r, what, rc):
    r["calls"].append([what, rc, lib.samaudio_last_error().decode() if rc else ""])
    return rc


def sha(r, name, t):
    r["sha"][name] = hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def set_tensors(lib, r, fn, h, tensors, prefix="w:"):
    for name, t in tensors.items():
        reg(lib, prefix + name, t)
        dt = hip.DT_BF16 if t.dtype == torch.bfloat16 else hip.DT_F32
        rc = fn(h, name.encode(), hip.ptr(t), dt, t.dim(), hip.shape_array(t.shape))
        if rc:
            call(lib, r, "set_tensor " + name, rc)


def workspace(lib, nbytes, short=0):
    buf = reg(lib, "ws", torch.zeros(nbytes + 512, dtype=torch.uint8))
    aligned = (buf.data_ptr() + 255) // 256 * 256
    lib.emu_log_register(b"ws", C.c_void_p(aligned), nbytes)
    return C.c_void_p(aligned), nbytes - short


def profile(lib, ctx, r, key):
    st, n = (hip.KernelStat * 256)(), C.c_int()
    lib.samaudio_profile_end(ctx, st, 256, C.byref(n))
    r[key] = [[st[i].name.decode(), st[i].launches, st[i].flops, st[i].bytes] for i in range(n.value)]


# ---------------------------------------------------------------------------------------------------------------- engine
def engine(lib, cfg, bf16):
    t, c = cfg.transformer, cfg.audio_codec
    hc = hip.Config(precision=hip.BF16 if bf16 else hip.F32, dim=t.dim, n_heads=t.n_heads, n_layers=t.n_layers, ffn_hidden=t.ffn_hidden,
                    latent_channels=t.out_channels, text_dim=cfg.text_encoder.dim, video_dim=cfg.vision_encoder.dim,
                    freq_dim=t.frequency_embedding_dim, anchor_dim=cfg.anchor_embedding_dim, anchor_vocab=cfg.num_anchors + 1,
                    max_positions=t.max_positions, norm_eps=t.norm_eps, codec_dim=c.codebook_dim, codec_latent=c.latent_dim,
                    enc_dim=c.encoder_dim, dec_dim=c.decoder_dim, enc_rates=(C.c_int32 * 4)(*c.encoder_rates),
                    dec_rates=(C.c_int32 * 4)(*c.decoder_rates))
    ctx = C.c_void_p()
    assert lib.samaudio_create(C.byref(hc), C.byref(ctx)) == 0
    return ctx


def dit_case(lib, cfg, sd, label, bf16, x3, Lt, cand, ktm=False, prefetch=0):
    r = begin(lib, f"dit {label} Lt={Lt} candidates={cand}")
    ctx = engine(lib, cfg, bf16)
    call(lib, r, "sentinel", lib.samaudio_set_option(ctx, hip.OPT_SENTINEL, 1))
    tensors = convert_dit(sd, cfg, torch.bfloat16 if bf16 else torch.float32, "cpu", ktm=ktm)
    if x3:
        tensors.update(convert_dit_x3(tensors, cfg.transformer.n_layers, HALF, x3))
        call(lib, r, "x3", lib.samaudio_set_option(ctx, hip.OPT_X3_CLASSES, x3))
    if prefetch:
        call(lib, r, "prefetch", lib.samaudio_set_option(ctx, hip.OPT_PREFETCH_ROWS, prefetch))
    set_tensors(lib, r, lib.samaudio_set_tensor, ctx, tensors)
    call(lib, r, "finalize", lib.samaudio_finalize(ctx, 0))
    B, T, C2 = 2, 5, cfg.transformer.out_channels
    rows = B * cand
    g = torch.Generator().manual_seed(11)
    z = reg(lib, "latent", torch.randn(B, T, C2 // 2, generator=g))
    text = reg(lib, "text", torch.randn(B, Lt, cfg.text_encoder.dim, generator=g))
    tmask = reg(lib, "text_mask", (torch.arange(Lt)[None] < torch.tensor([Lt, max(1, Lt - 2)])[:, None]).to(torch.uint8))
    pad = reg(lib, "pad_mask", (torch.arange(T)[None] < torch.tensor([T, 3])[:, None]).to(torch.uint8))
    ids = reg(lib, "anchor_ids", torch.tensor([[0, 1], [0, 2]]))
    align = reg(lib, "anchor_alignment", torch.tensor([[0, 0, 1, 1, 0], [1, 1, 0, 0, 0]]))
    r["workspace_bytes"] = need = lib.samaudio_workspace_bytes(ctx, rows, T, Lt, 0, 0)
    p, n = workspace(lib, need)
    call(lib, r, "set_workspace", lib.samaudio_set_workspace(ctx, p, n))
    lib.samaudio_profile_begin(ctx)
    call(lib, r, "prepare_latent", lib.samaudio_prepare_latent(ctx, rows, T, Lt, cand, hip.ptr(z), hip.ptr(text), hip.ptr(tmask), None,
                                                               hip.ptr(ids), 2, hip.ptr(align), hip.ptr(pad), None))
    noisy = reg(lib, "noisy", torch.randn(rows, T, C2, generator=g))
    time = reg(lib, "time", torch.linspace(0.1, 0.9, rows))
    out = reg(lib, "out", torch.zeros(rows, T, C2))
    call(lib, r, "forward", lib.samaudio_forward(ctx, hip.ptr(noisy), hip.ptr(time), rows, hip.ptr(out), None))
    sha(r, "forward", out)
    state = reg(lib, "state", torch.randn(rows, T, C2, generator=g))
    call(lib, r, "ode_solve", lib.samaudio_ode_solve(ctx, hip.ptr(state), hip.ODE_MIDPOINT, (C.c_float * 3)(0.0, 0.5, 1.0), 3, None))
    sha(r, "state", state)
    profile(lib, ctx, r, "profile")
    amax, bad = (C.c_float * 16)(), (C.c_double * 16)()
    call(lib, r, "sentinel_read", lib.samaudio_sentinel_read(ctx, amax, bad, None))
    r["sentinel"] = [list(amax), list(bad)]
    lib.samaudio_destroy(ctx)


def codec_case(lib, cfg, sd, label, bf16, x3):
    r = begin(lib, f"codec {label}")
    ctx = engine(lib, cfg, bf16)
    codec = convert_codec(sd, cfg, torch.bfloat16 if bf16 else torch.float32, "cpu")
    tensors = dict(codec)
    if x3:
        call(lib, r, "x3", lib.samaudio_set_option(ctx, hip.OPT_X3_CLASSES, hip.CLS["codec"]))
        tensors.update(convert_codec_x3(codec, HALF))
        tensors.update(convert_codec_fly16(codec, HALF))
    set_tensors(lib, r, lib.samaudio_set_tensor, ctx, tensors)
    call(lib, r, "finalize", lib.samaudio_finalize(ctx, 1))
    c = cfg.audio_codec
    items, frames = 2, 1
    S = frames * c.hop_length
    r["workspace_bytes"] = need = lib.samaudio_workspace_bytes(ctx, 0, 0, 0, items, S)
    p, n = workspace(lib, need)
    call(lib, r, "set_workspace", lib.samaudio_set_workspace(ctx, p, n))
    g = torch.Generator().manual_seed(4)
    wav = reg(lib, "wav", 0.1 * torch.randn(items, S, generator=g))
    z = reg(lib, "z", torch.zeros(items, frames, c.codebook_dim))
    lib.samaudio_profile_begin(ctx)
    call(lib, r, "encode", lib.samaudio_codec_encode(ctx, hip.ptr(wav), items, S, hip.ptr(z), None))
    sha(r, "latent", z)
    out = reg(lib, "wav_out", torch.zeros(items, S))
    call(lib, r, "decode", lib.samaudio_codec_decode(ctx, hip.ptr(z), items, frames, hip.ptr(out), None))
    sha(r, "decoded", out)
    pairs = reg(lib, "pairs", torch.randn(1, frames, 2 * c.codebook_dim, generator=g))
    call(lib, r, "decode_pairs", lib.samaudio_codec_decode_pairs(ctx, hip.ptr(pairs), 1, frames, hip.ptr(out), None))
    sha(r, "decoded_pairs", out)
    profile(lib, ctx, r, "profile")
    lib.samaudio_destroy(ctx)


# ---------------------------------------------------------------------------------------------------------------- towers
def judge(lib, r, cfg, sd, bf16, x3):
    jc = hip.JudgeConfig(precision=hip.BF16 if bf16 else hip.F32, transformer=peav_dims(cfg.transformer, cfg.audio_codec.codebook_dim),
                         finetune_transformer=peav_dims(cfg.finetune_transformer, cfg.bottleneck_dim),
                         codec_dim=cfg.audio_codec.codebook_dim, text_hidden=cfg.text_hidden, bottleneck_dim=cfg.bottleneck_dim)
    h = C.c_void_p()
    assert lib.samaudio_judge_create(C.byref(jc), C.byref(h)) == 0
    tensors = convert_judge(sd, cfg, torch.bfloat16 if bf16 else torch.float32, "cpu")
    if x3:
        call(lib, r, "x3", lib.samaudio_judge_set_option(h, hip.OPT_X3_CLASSES, x3))
        tensors.update(convert_judge_x3(tensors, cfg, HALF, x3))
    set_tensors(lib, r, lib.samaudio_judge_set_tensor, h, tensors)
    call(lib, r, "finalize", lib.samaudio_judge_finalize(h))
    return h


def judge_case(lib, cfg, sd, label, bf16, x3):
    r = begin(lib, f"judge {label}")
    h = judge(lib, r, cfg, sd, bf16, x3)
    Bi, cand, T, CD = 2, 3, 50, cfg.audio_codec.codebook_dim
    g = torch.Generator().manual_seed(8)
    in_lat = reg(lib, "in_lat", torch.randn(Bi, T, CD, generator=g))
    sep_lat = reg(lib, "sep_lat", torch.randn(Bi * cand, T, CD, generator=g))
    pooled = reg(lib, "pooled", torch.randn(Bi * cand, cfg.text_hidden, generator=g))
    mask = reg(lib, "pad_mask", (torch.arange(T)[None] < torch.tensor([50, 9])[:, None]).to(torch.uint8))
    r["workspace_bytes"] = need = lib.samaudio_judge_workspace_bytes(h, Bi, cand, T)
    p, n = workspace(lib, need)
    call(lib, r, "set_workspace", lib.samaudio_judge_set_workspace(h, p, n))
    scores = reg(lib, "scores", torch.zeros(Bi * cand, 4))
    call(lib, r, "score", lib.samaudio_judge_score(h, hip.ptr(in_lat), hip.ptr(sep_lat), Bi, cand, T, hip.ptr(pooled), hip.ptr(mask),
                                                   hip.ptr(scores), None))
    sha(r, "scores", scores)
    for which, tc, in_dim in ((0, cfg.transformer, CD), (1, cfg.finetune_transformer, cfg.bottleneck_dim)):
        x = reg(lib, f"x{which}", torch.randn(Bi, T, in_dim, generator=g))
        hidden = reg(lib, f"hidden{which}", torch.zeros(Bi, T + 1, tc.hidden_size))
        r[f"encode{which}_workspace_bytes"] = lib.samaudio_judge_workspace_bytes(h, Bi, 1, T)
        call(lib, r, f"encode {which}", lib.samaudio_judge_encode(h, which, hip.ptr(x), hip.ptr(mask), Bi, T, hip.ptr(hidden), None))
        sha(r, f"hidden{which}", hidden)
    lib.samaudio_judge_destroy(h)


def frame_case(lib, label, bf16, x3):
    r = begin(lib, f"frame {label}")
    cfg = PEAudioFrameConfig(audio=G.TINY_TC, text_model=dict(G.TINY_TEXT, hidden_size=64), codebook_dim=128)
    sd = init_frame_state_dict(cfg, seed=2)
    fc = hip.FrameConfig(precision=hip.BF16 if bf16 else hip.F32, audio=peav_dims(cfg.audio, cfg.codebook_dim), codec_dim=cfg.codebook_dim,
                         embed_dim=cfg.text_hidden)
    h = C.c_void_p()
    assert lib.samaudio_frame_create(C.byref(fc), C.byref(h)) == 0
    tensors = convert_frame(sd, cfg, torch.bfloat16 if bf16 else torch.float32, "cpu")
    if x3:
        call(lib, r, "x3", lib.samaudio_frame_set_option(h, hip.OPT_X3_CLASSES, x3))
        tensors.update(convert_peav_x3(tensors, "a.", cfg.audio.num_hidden_layers, HALF, x3))
    set_tensors(lib, r, lib.samaudio_frame_set_tensor, h, tensors)
    call(lib, r, "finalize", lib.samaudio_frame_finalize(h))
    B, T = 2, 50
    g = torch.Generator().manual_seed(6)
    feats = reg(lib, "feats", torch.randn(B, T, 128, generator=g))
    pooled = reg(lib, "pooled", torch.randn(B, cfg.text_hidden, generator=g))
    mask = reg(lib, "pad_mask", (torch.arange(T)[None] < torch.tensor([50, 9])[:, None]).to(torch.uint8))
    r["workspace_bytes"] = need = lib.samaudio_frame_workspace_bytes(h, B, T)
    p, n = workspace(lib, need)
    call(lib, r, "set_workspace", lib.samaudio_frame_set_workspace(h, p, n))
    out = reg(lib, "logits", torch.zeros(B, T))
    call(lib, r, "logits", lib.samaudio_frame_logits(h, hip.ptr(feats), hip.ptr(pooled), hip.ptr(mask), B, T, hip.ptr(out), None))
    sha(r, "logits", out)
    lib.samaudio_frame_destroy(h)


# ---------------------------------------------------------------------------------------------------------------- error paths
def error_cases(lib, cfg, sd, jcfg, jsd):
    r = begin(lib, "errors engine")
    c16, c32 = engine(lib, cfg, True), engine(lib, cfg, False)
    call(lib, r, "x3 on a 16-bit context", lib.samaudio_set_option(c16, hip.OPT_X3_CLASSES, hip.CLS["qkv"]))
    call(lib, r, "class outside the capable mask", lib.samaudio_set_option(c32, hip.OPT_X3_CLASSES, hip.CLS["out"]))
    t32 = convert_dit(sd, cfg, torch.float32, "cpu")
    set_tensors(lib, r, lib.samaudio_set_tensor, c32, t32)
    for name in ("qkv", "wo", "cwq", "cwo", "w13", "w2", "patch", "ckv"):   # the twin is missing: named at finalize
        call(lib, r, f"option {name}", lib.samaudio_set_option(c32, hip.OPT_X3_CLASSES, hip.CLS[name]))
        call(lib, r, f"finalize without the {name} twins", lib.samaudio_finalize(c32, 0))
    call(lib, r, "option off", lib.samaudio_set_option(c32, hip.OPT_X3_CLASSES, 0))
    call(lib, r, "finalize", lib.samaudio_finalize(c32, 0))
    for name in ("qkv", "w2", "patch", "ckv"):   # ... and at set_option after finalize
        call(lib, r, f"option {name} after finalize, twins absent", lib.samaudio_set_option(c32, hip.OPT_X3_CLASSES, hip.CLS[name]))
    # twins of one class only: that class may be switched on after finalize(0), another may not; the workspace then one byte short
    w2 = convert_dit_x3(t32, cfg.transformer.n_layers, HALF, hip.CLS["w2"])
    set_tensors(lib, r, lib.samaudio_set_tensor, c32, w2)
    call(lib, r, "finalize with w2 twins", lib.samaudio_finalize(c32, 0))
    call(lib, r, "option w2 after finalize", lib.samaudio_set_option(c32, hip.OPT_X3_CLASSES, hip.CLS["w2"]))
    call(lib, r, "option w2 | w13 after finalize", lib.samaudio_set_option(c32, hip.OPT_X3_CLASSES, hip.CLS["w2"] | hip.CLS["w13"]))
    g = torch.Generator().manual_seed(1)
    feats = reg(lib, "feats", torch.randn(2, 5, cfg.transformer.out_channels, generator=g))
    need = lib.samaudio_workspace_bytes(c32, 2, 5, 1, 0, 0)
    for short in (1, 4096 + 1):   # (workspace_bytes = the plan + 4096)
        p, n = workspace(lib, need, short)
        call(lib, r, "set_workspace", lib.samaudio_set_workspace(c32, p, n))
        call(lib, r, f"prepare in a workspace {short} bytes short", lib.samaudio_prepare(c32, 2, 5, 0, hip.ptr(feats), None, None, None, None, 0,
                                                                                      None, None, None))
    lib.samaudio_destroy(c16)
    lib.samaudio_destroy(c32)

    r = begin(lib, "errors towers")
    for bf16, opt in ((True, hip.CLS["qkv"]), (False, hip.CLS["cwq"]), (False, hip.CLS_X3_TOWER | hip.CLS["codec"])):
        jc = hip.JudgeConfig(precision=hip.BF16 if bf16 else hip.F32, transformer=peav_dims(jcfg.transformer, jcfg.audio_codec.codebook_dim),
                             finetune_transformer=peav_dims(jcfg.finetune_transformer, jcfg.bottleneck_dim),
                             codec_dim=jcfg.audio_codec.codebook_dim, text_hidden=jcfg.text_hidden, bottleneck_dim=jcfg.bottleneck_dim)
        h = C.c_void_p()
        assert lib.samaudio_judge_create(C.byref(jc), C.byref(h)) == 0
        call(lib, r, f"judge option {opt:#x} bf16={bf16}", lib.samaudio_judge_set_option(h, hip.OPT_X3_CLASSES, opt))
        call(lib, r, "judge unknown option", lib.samaudio_judge_set_option(h, hip.OPT_X3_CLASSES + 100, 0))
        lib.samaudio_judge_destroy(h)
    for bit in ("qkv", "wo", "w13", "w2", "patch"):   # a missing twin, named
        h = C.c_void_p()
        jc.precision = hip.F32
        assert lib.samaudio_judge_create(C.byref(jc), C.byref(h)) == 0
        call(lib, r, f"judge option {bit}", lib.samaudio_judge_set_option(h, hip.OPT_X3_CLASSES, hip.CLS[bit]))
        set_tensors(lib, r, lib.samaudio_judge_set_tensor, h, convert_judge(jsd, jcfg, torch.float32, "cpu"))
        call(lib, r, f"judge finalize without the {bit} twins", lib.samaudio_judge_finalize(h))
        lib.samaudio_judge_destroy(h)
    h = judge(lib, r, jcfg, jsd, False, hip.CLS_X3_TOWER)
    need = lib.samaudio_judge_workspace_bytes(h, 2, 3, 50)
    g = torch.Generator().manual_seed(8)
    in_lat, sep_lat = reg(lib, "in_lat", torch.randn(2, 50, 64, generator=g)), reg(lib, "sep_lat", torch.randn(6, 50, 64, generator=g))
    pooled, scores = reg(lib, "pooled", torch.randn(6, jcfg.text_hidden, generator=g)), reg(lib, "scores", torch.zeros(6, 4))
    for short in (1, 4096 + 1):
        p, n = workspace(lib, need, short)
        call(lib, r, "set_workspace", lib.samaudio_judge_set_workspace(h, p, n))
        call(lib, r, f"judge_score in a workspace {short} bytes short",
             lib.samaudio_judge_score(h, hip.ptr(in_lat), hip.ptr(sep_lat), 2, 3, 50, hip.ptr(pooled), None, hip.ptr(scores), None))
    lib.samaudio_judge_destroy(h)


def main():
    lib = load(os.path.abspath(sys.argv[1]))
    out = sys.argv[2]
    os.makedirs(out, exist_ok=True)
    lib.emu_log_open(os.path.join(out, "launches.log").encode())
    cfg = preset_config("tiny")
    sd = init_state_dict(cfg, seed=3)
    CLS, ATT = hip.CLS, hip.X3_ATTENTION
    bits = [CLS[n] for n in ("qkv", "wo", "cwq", "cwo", "w13", "w2", "patch", "ckv", "codec")] + [ATT]
    assert sum(bits) == hip.CLS_X3_DEFAULT
    masks = [("fp32", False, 0), ("16-bit", True, 0), ("x3 default", False, hip.CLS_X3_DEFAULT)]
    masks += [(f"x3 {b:#x} alone", False, b) for b in bits]
    masks += [("x3 gemms, no attention", False, hip.CLS_X3_DEFAULT & ~ATT)]
    for label, bf16, x3 in masks:
        for Lt in (3, 20):
            for cand in (1, 2):
                dit_case(lib, cfg, sd, label, bf16, x3, Lt, cand)
    for Lt in (3, 20):
        dit_case(lib, cfg, sd, "16-bit ktm prefetch", True, 0, Lt, 1, ktm=True, prefetch=2048)
    for label, bf16, x3 in (("fp32", False, False), ("16-bit", True, False), ("x3", False, True)):
        codec_case(lib, cfg, sd, label, bf16, x3)   # the default DAC-VAE dims: stages of 64 .. 1024 / 1536 .. 96 channels
    jcfg = G.tiny_judge_config()
    jsd = init_judge_state_dict(jcfg, seed=9, with_codec=False)
    tower = [("fp32", False, 0), ("16-bit", True, 0), ("x3 tower", False, hip.CLS_X3_TOWER)]
    tower += [(f"x3 {b:#x} alone", False, b) for b in (CLS["qkv"], CLS["wo"], CLS["w13"], CLS["w2"], CLS["patch"], ATT)]
    tower += [("x3 tower, wo off", False, hip.CLS_X3_TOWER & ~CLS["wo"])]
    for label, bf16, x3 in tower:
        judge_case(lib, jcfg, jsd, label, bf16, x3)
        frame_case(lib, label, bf16, x3)
    error_cases(lib, cfg, sd, jcfg, jsd)
    lib.emu_log_close()
    with open(os.path.join(out, "results.json"), "w") as f:
        json.dump(RESULTS, f, indent=1, sort_keys=True)
    print(f"{len(RESULTS)} cases")


if __name__ == "__main__":
    main()
