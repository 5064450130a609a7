"""Workspace sizes and codec pass partition of one build of the CPU emulation library (oracle/emu/build.sh), as a table.

    python profiles/codec_plan/workspace_compare.py <libsamaudio_emu.so> sizes
    python profiles/codec_plan/workspace_compare.py <libsamaudio_emu.so> passes <mode>

`run.sh sizes` runs both on the parent commit's library and on this tree's and diffs them: workspace_compare.txt.

`sizes`: samaudio_workspace_bytes for every precision mode {fp32, fp32 with OPT_X3_CLASSES (codec and the DiT classes) and the codec's
.x3 / .fly twins registered, bf16} x dims preset {tiny, large*} x samples {hop, 3 hop, 250 hop} x items {1, 2, 3, 5, 16, 64}: the codec
plan alone (rows = 0), the DiT plan of as many rows alone - without and with the folded cross-attention operands - and both as a
separate() of items / 2 clips asks for them.  Host arithmetic only.  The same rows carry the refusals at the plan's edges, which launch
nothing: one byte below workspace_bytes(1) encode and decode return SAMAUDIO_ERR_WORKSPACE (-3), one byte below workspace_bytes(2) so
does decode of pairs.

`passes`: the pass partition as the engine runs it, observed as the profiled launches of a call over those of a one-pass call, in a
workspace of exactly workspace_bytes(capacity) inside 0xFF bytes: encode, decode and decode of pairs at samples hop and 3 hop (the
codec's dims are the same for every preset).  The emulation computes every launch, so 250 hop and 64 items are left to the sizes - the
partition is (bytes - 64 KiB) / per_item of them - and to the GPU benchmark, whose codec launch counts pin it at that size.
"""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["SAMAUDIO_NO_FOLD"] = "1"   # (the fold kernels are not emulated; it sizes the DiT plan of both builds alike)
from sam_audio_amd import hip, preset_config  # noqa: E402
from sam_audio_amd.synthetic import init_state_dict  # noqa: E402
from sam_audio_amd.weights import convert_codec, convert_codec_fly16, convert_codec_x3  # noqa: E402

MODES = ("fp32", "fp32+x3codec", "bf16")   # (fp32+x3codec: OPT_X3_CLASSES on, see engine())


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in hip._PROTOS.items():
        if not name.startswith(("samaudio_vit_", "samaudio_t5_", "samaudio_mbert_")):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def engine(lib, mode, preset, keep):
    cfg = preset_config(preset)
    t, c = cfg.transformer, cfg.audio_codec
    hc = hip.Config(precision=hip.BF16 if mode == "bf16" else hip.F32, dim=t.dim, n_heads=t.n_heads, n_layers=t.n_layers,
                    ffn_hidden=t.ffn_hidden, latent_channels=t.out_channels, text_dim=cfg.text_encoder.dim,
                    video_dim=cfg.vision_encoder.dim, freq_dim=t.frequency_embedding_dim, anchor_dim=cfg.anchor_embedding_dim,
                    anchor_vocab=cfg.num_anchors + 1, max_positions=t.max_positions, norm_eps=t.norm_eps, codec_dim=c.codebook_dim,
                    codec_latent=c.latent_dim, enc_dim=c.encoder_dim, dec_dim=c.decoder_dim,
                    enc_rates=(C.c_int32 * 4)(*c.encoder_rates), dec_rates=(C.c_int32 * 4)(*c.decoder_rates))
    ctx = C.c_void_p()
    assert lib.samaudio_create(C.byref(hc), C.byref(ctx)) == 0
    sd = {k: v for k, v in init_state_dict(preset_config("tiny"), seed=3).items() if k.startswith("audio_codec.")}
    codec = convert_codec(sd, cfg, torch.bfloat16 if mode == "bf16" else torch.float32, "cpu")
    tensors = dict(codec)
    if mode == "fp32+x3codec":   # as SAMAudio.load_state_dict registers them
        x3 = sum(hip.CLS[c] for c in ("codec", "qkv", "wo", "cwq", "cwo", "w13", "w2", "patch", "ckv"))   # (the DiT's: sized, never run)
        assert lib.samaudio_set_option(ctx, hip.OPT_X3_CLASSES, x3) == 0
        tensors.update(convert_codec_x3(codec, torch.bfloat16))
        tensors.update(convert_codec_fly16(codec, torch.bfloat16))
    for name, tt in tensors.items():
        keep.append(tt)
        dt = hip.DT_BF16 if tt.dtype == torch.bfloat16 else hip.DT_F32
        assert lib.samaudio_set_tensor(ctx, name.encode(), hip.ptr(tt), dt, tt.dim(), hip.shape_array(tt.shape)) == 0
    assert lib.samaudio_finalize(ctx, 1) == 0, lib.samaudio_last_error().decode()
    return ctx, cfg


def workspace(lib, ctx, nbytes):
    buf = torch.full((nbytes + 512,), 255, dtype=torch.uint8)
    aligned = (buf.data_ptr() + 255) // 256 * 256
    assert lib.samaudio_set_workspace(ctx, C.c_void_p(aligned), nbytes) == 0
    return buf


def call(lib, ctx, cfg, what, items, frames):
    """(return code, profiled launches) of one encode | decode | pairs call over `items` waveforms"""
    c = cfg.audio_codec
    g = torch.Generator().manual_seed(1)
    lib.samaudio_profile_begin(ctx)
    if what == "encode":
        wav, z = 0.1 * torch.randn(items, frames * c.hop_length, generator=g), torch.empty(items, frames, c.codebook_dim)
        rc = lib.samaudio_codec_encode(ctx, hip.ptr(wav), items, frames * c.hop_length, hip.ptr(z), None)
    else:
        wav = torch.empty(items, frames * c.hop_length)
        if what == "pairs":
            lat = torch.randn(items // 2, frames, 2 * c.codebook_dim, generator=g)
            rc = lib.samaudio_codec_decode_pairs(ctx, hip.ptr(lat), items // 2, frames, hip.ptr(wav), None)
        else:
            lat = torch.randn(items, frames, c.codebook_dim, generator=g)
            rc = lib.samaudio_codec_decode(ctx, hip.ptr(lat), items, frames, hip.ptr(wav), None)
    st, n = (hip.KernelStat * 64)(), C.c_int()
    lib.samaudio_profile_end(ctx, st, 64, C.byref(n))
    return rc, sum(st[i].launches for i in range(n.value))


def sizes(lib):
    for mode in MODES:
        for preset in ("tiny", "large*"):
            keep = []
            ctx, cfg = engine(lib, mode, preset, keep)
            hop = cfg.audio_codec.hop_length
            for frames in (1, 3, 250):
                S = frames * hop
                edge = []
                for what, n in (("encode", 1), ("decode", 1), ("pairs", 2)):   # one byte short of the plan: refused, nothing launched
                    buf = workspace(lib, ctx, lib.samaudio_workspace_bytes(ctx, 0, 0, 0, n, S) - 1)
                    edge.append(f"{what}@ws({n})-1:rc={call(lib, ctx, cfg, what, n, frames)[0]}")
                for items in (1, 2, 3, 5, 16, 64):
                    codec = lib.samaudio_workspace_bytes(ctx, 0, 0, 0, items, S)
                    dit = lib.samaudio_workspace_bytes(ctx, items, frames, 8, 0, 0)   # the DiT plan of `items` rows alone
                    del os.environ["SAMAUDIO_NO_FOLD"]   # ... and with the folds' operands (16-bit contexts, x3 class CWO)
                    fold = lib.samaudio_workspace_bytes(ctx, items, frames, 8, 0, 0)
                    os.environ["SAMAUDIO_NO_FOLD"] = "1"
                    joint = lib.samaudio_workspace_bytes(ctx, max(1, items // 2), frames, 8, items, S)
                    print(f"{mode:13s} {preset:7s} samples={S:7d} items={items:3d} codec_ws={codec:12d} dit_ws={dit:11d} dit_fold_ws={fold:11d} both_ws={joint:12d} "
                          + " ".join(edge))
            lib.samaudio_destroy(ctx)


def passes(lib, mode):
    keep = []
    ctx, cfg = engine(lib, mode, "tiny", keep)
    hop = cfg.audio_codec.hop_length
    cases = {1: [("encode", 1, 1), ("encode", 3, 3), ("encode", 3, 2), ("encode", 5, 2), ("encode", 5, 4),
                 ("decode", 1, 1), ("decode", 3, 3), ("decode", 3, 2), ("decode", 5, 2), ("decode", 5, 4),
                 ("pairs", 2, 2), ("pairs", 4, 2), ("pairs", 4, 3), ("pairs", 4, 1)],
             3: [("encode", 1, 1), ("encode", 3, 2), ("decode", 1, 1), ("decode", 3, 2), ("pairs", 2, 2), ("pairs", 4, 3)]}
    for frames, rows in cases.items():
        one = {}
        for what, items, cap in rows:
            need = lib.samaudio_workspace_bytes(ctx, 0, 0, 0, cap, frames * hop)
            buf = workspace(lib, ctx, need)
            rc, launches = call(lib, ctx, cfg, what, items, frames)
            one.setdefault(what, launches)   # (the first case of each kind is a single pass)
            off = (buf.data_ptr() + 255) // 256 * 256 - buf.data_ptr()
            clean = bool((buf[off + need:] == 255).all())
            print(f"{mode:13s} samples={frames * hop:5d} {what:6s} items={items} capacity={cap} ws={need} rc={rc} launches={launches} "
                  f"passes={launches / one[what] if one[what] else 0:g} bytes_behind_untouched={clean}", flush=True)
    lib.samaudio_destroy(ctx)


if __name__ == "__main__":
    lib = load(os.path.abspath(sys.argv[1]))
    sizes(lib) if sys.argv[2] == "sizes" else passes(lib, sys.argv[3])
