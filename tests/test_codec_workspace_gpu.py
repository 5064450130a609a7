"""The DAC-VAE passes under the workspace guard (tests/util.py workspace_guard): encode and decode over more than one pass, and
decode of (target, residual) pairs, each in exactly the workspace samaudio_workspace_bytes asks for, followed by bytes the test owns.

tests/test_text_edges_gpu.py runs separate() under the guard without the codec; here the codec plan (engine.hip plan_codec /
codec_chunk) runs under it on its own: 'tiny' dims, 2 frames, SAMAUDIO_CODEC_CHUNK small enough that a call needs several passes.
Each call must leave the guard alone, equal the same call outside the guard bit for bit, and stay within the bound the codec parity
tests hold that precision to against the oracle (tests/test_path_gpu.py::test_codec_roundtrip_pieces: fp32, and its 16-bit bound for
bf16 and - a finer format under the same bound - fp16; tests/test_x3_gpu.py::test_codec_roundtrip_in_x3_context: the x3 precisions).
On the simulator builds (SAMAUDIO_EMU_DRYRUN: bfloat16 library only) fp32, bf16 and bf16x3 run.
"""
import os

import pytest
import torch

from oracle import samaudio_oracle as O
from sam_audio_amd import SAMAudio, preset_config
from sam_audio_amd.synthetic import init_state_dict, synthetic_clip
from tests import util

pytestmark = pytest.mark.gpu
SIM = os.environ.get("SAMAUDIO_EMU_DRYRUN", "") != ""
PRECS = ["fp32", "bf16", "bf16x3"] if SIM else ["fp32", "bf16", "fp16", "fp16x3"]
# (encode latent, decoded waveform) max-abs against the oracle, as the parity tests named above state them
TOL = {"fp32": (1e-3, 1e-3), "bf16": (3e-3, 2e-3), "fp16": (3e-3, 2e-3), "fp16x3": (2e-5, 2e-5), "bf16x3": (5e-4, 5e-4)}
FRAMES = 2
_REF = {}


def _reference():
    """4 clips of 2 frames, the oracle's latents of them and the oracle's decode of those latents - computed once"""
    if not _REF:
        cfg = preset_config("tiny")
        sd = {k: v for k, v in init_state_dict(cfg, seed=6).items() if k.startswith("audio_codec.")}
        wav = torch.stack([synthetic_clip(i, FRAMES * cfg.audio_codec.hop_length) for i in range(4)])   # [4, 1, 3840]
        with torch.inference_mode():
            z = O.dac_encode(sd, cfg.audio_codec, wav)                      # [4, 128, 2]
            w = O.dac_decode(sd, cfg.audio_codec, z).squeeze(1)             # [4, 3840]
        _REF.update(cfg=cfg, sd=sd, wav=wav, z=z.transpose(1, 2).contiguous(), w=w)
    return _REF


def _calls(model, r, gpu):
    """the calls of this file: (name, chunk, function, items of the passes it must take, reference, bound index)"""
    z = r["z"].to(gpu)
    state = torch.cat([z[0::2], z[1::2]], 2).contiguous()   # the ODE state layout: row b = (waveform 2b | waveform 2b + 1)
    return [("encode 3", 2, lambda: model.encode_audio(r["wav"][:3].to(gpu)), (2, 1), r["z"][:3], 0),
            ("decode 3", 2, lambda: model.decode_audio(z[:3]), (2, 1), r["w"][:3], 1),
            ("decode 4 as pairs, chunk 2", 2, lambda: model.decode_audio(state, pairs=True), (2, 2), r["w"], 1),
            ("decode 4 as pairs, chunk 3", 3, lambda: model.decode_audio(state, pairs=True), (2, 2), r["w"], 1)]   # 3 -> whole pairs


def _launches(model, fn):
    model.profile_begin()
    out = fn().clone()
    return out, sum(k["launches"] for k in model.profile_end())


@pytest.mark.parametrize("prec", PRECS)
def test_codec_passes_stay_inside_their_workspace(gpu, prec, monkeypatch):
    r = _reference()
    model = SAMAudio(r["cfg"], precision=prec, device=str(gpu), codec_decode="32")
    model.load_state_dict(r["sd"], strict=False)
    z = r["z"].to(gpu)
    # launches of a call that runs as ONE pass over 1 and over 2 items, per kind of call (a split launch counts twice, and whether a
    # launch is split depends on its size: a pass is compared with a single pass of its own size)
    monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", "16")
    one = {("encode", n): _launches(model, lambda: model.encode_audio(r["wav"][:n].to(gpu)))[1] for n in (1, 2)}
    one.update({("decode", n): _launches(model, lambda: model.decode_audio(z[:n]))[1] for n in (1, 2)})
    for name, chunk, fn, passes, want, which in _calls(model, r, gpu):
        monkeypatch.setenv("SAMAUDIO_CODEC_CHUNK", str(chunk))
        model._workspace = None          # outside the guard: a workspace of the model's own, sized for this chunk
        free, n_free = _launches(model, fn)
        with util.workspace_guard(model):
            held, n_held = _launches(model, fn)
        model._workspace = None
        util.report(f"codec {name} {prec}", held, want, TOL[prec][which])
        assert torch.equal(held, free), f"{name}: the result under the guard differs from the one outside it"
        assert n_held == n_free == sum(one[name.split()[0], n] for n in passes), (name, n_held, n_free, one)
