"""The CPU side of the CLAP ranker: tests/clap_ref.py - the float64 statement the log-mel kernel is held to -
pinned to transformers' ClapFeatureExtractor itself; the config / create_ranker wiring; the checkpoint loader's refusals; the BatchNorm
fold and the relative-position index against the module's; the header against the Python binding; the library's argument checks; the
front-end kernel on the SIMT simulator.

What "equal to the extractor" can mean: the extractor is not a float64 computation end to end - `audio_utils.spectrogram` stores the STFT
as complex64 and returns float32.  complex64 moves |X|^2 by at most 2.4e-7 relative (1.0e-6 dB), the float32 result by half an ulp of a
value below 128 (3.8e-6 dB); the statement reads the window and the bank rounded to float32, as the kernel does (6e-8 relative each:
below 1e-6 dB on clips whose bins all sit within 40 dB of the frame's energy).  EXTRACTOR_DB = 1e-5 covers their sum; a wrong window,
padding, repeat count, bank or floor moves values by whole dB.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from sam_audio_amd import clap, hip, synthetic
from sam_audio_amd.config import ClapRankerConfig, SAMAudioConfig, parse_ranker_config
from sam_audio_amd.ranking import ClapRanker, EnsembleRanker, Ranker, create_ranker
from sam_audio_amd.synthetic import synthetic_clip
from tests import clap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRACTOR_DB = 1e-5
# name -> (fft_size, hop, max_length, n_mels)
PARAMS = {"mini": (64, 8, 2_000, 16), "real": (1024, 480, 480_000, 64)}


def _extractor(name):
    from transformers import ClapFeatureExtractor
    fft, hop, _, n_mels = PARAMS[name]
    return ClapFeatureExtractor(feature_size=n_mels, sampling_rate=48_000, hop_length=hop, fft_window_size=fft,
                                truncation="rand_trunc", padding="repeatpad")


def _extract(name, wav):
    _, _, L, _ = PARAMS[name]
    out = _extractor(name)(wav.numpy(), sampling_rate=48_000, max_length=L, return_tensors="pt")
    return out["input_features"][0, 0].double()


@pytest.mark.parametrize("name", list(PARAMS))
def test_statement_equals_the_feature_extractor(name):
    """shorter than half max_length (two repeats + zeros), between half and full (one copy + zeros), exactly max_length; and a longer
    clip cropped at an offset against the extractor on the sliced waveform"""
    fft, hop, L, n_mels = PARAMS[name]
    kw = dict(max_length=L, fft_size=fft, hop=hop, bank=clap.mel_bank(fft, n_mels), quantise=False)
    for index, n in enumerate((int(0.37 * L), int(0.8 * L), L)):
        wav = synthetic_clip(index, n)[0]
        got, want = R.logmel(wav, **kw)[0], _extract(name, wav)
        assert got.shape == want.shape == (1 + L // hop, n_mels)
        err = (got - want).abs().max().item()
        print(f"{name} n = {n}: |statement - extractor| <= {err:.3e} dB")
        assert err <= EXTRACTOR_DB, (name, n, err)
    long = synthetic_clip(5, L + L // 2)[0]
    offset = 345 if name == "mini" else 12_345
    got = R.logmel(long, offsets=[offset], **kw)[0]
    assert (got - _extract(name, long[offset: offset + L])).abs().max().item() <= EXTRACTOR_DB
    assert (R.logmel(long, **kw)[0] - _extract(name, long[:L])).abs().max().item() <= EXTRACTOR_DB   # the default: the head
    # the int16 round trip is laion_clap's two float32 expressions, and it is a quantisation to multiples of 1 / 32767
    x = synthetic_clip(7, 1_000)[0]
    q = R.int16_round_trip(x)
    assert q.dtype == torch.float32 and (q - x).abs().max() <= 1 / 32767 and torch.equal(q, R.int16_round_trip(q))
    assert torch.equal(R.int16_round_trip(torch.tensor([2.0, -3.0, 0.99999])), torch.tensor([1.0, -1.0, 32766 / 32767.0]))


def test_tables_and_bank_are_the_extractors():
    from transformers.audio_utils import window_function
    ex = _extractor("real")
    assert np.array_equal(clap.mel_bank().numpy(), ex.mel_filters_slaney)
    assert np.array_equal(clap.mel_bank(form="htk").numpy(), ex.mel_filters)
    tables = clap.logmel_tables(1024)
    assert tables.dtype == torch.float32 and tables.shape == (2048,)
    assert np.abs(tables[:1024].double().numpy() - window_function(1024, "hann")).max() < 1e-7
    t = 2 * np.pi * np.arange(512) / 1024
    assert np.abs(tables[1024::2].double().numpy() - np.cos(t)).max() < 1e-7 and np.abs(tables[1025::2].double().numpy() + np.sin(t)).max() < 1e-7
    for bad in (32, 4096, 1000):
        with pytest.raises(ValueError):
            clap.logmel_tables(bad)
    assert clap.frames(480_000, 480) == 1001 and clap.frames(2_000, 8) == 251


def test_config_and_create_ranker(tmp_path):
    d = str(tmp_path)
    rc = parse_ranker_config({"kind": "clap", "checkpoint": d})
    assert isinstance(rc, ClapRankerConfig) and rc.checkpoint == d and rc.kind == "clap"
    assert parse_ranker_config({"kind": "clap"}) == ClapRankerConfig(checkpoint=None)
    assert isinstance(SAMAudioConfig(text_ranker={"kind": "clap", "checkpoint": d}).text_ranker, ClapRankerConfig)
    for cfg in ({"kind": "clap"}, ClapRankerConfig()):
        with pytest.raises(NotImplementedError, match="third-party") as e:
            create_ranker(cfg)
        assert "local" in str(e.value) and "directory" in str(e.value)
    with pytest.raises(NotImplementedError, match="third-party"):      # ImageBind: as before
        create_ranker({"kind": "imagebind"})
    # the model and the tokenizer injected: nothing is loaded, so this runs without a GPU
    model, tok = object(), object()
    r = create_ranker(rc, model=model, tokenizer=tok, device="cuda:0", precision="fp16x3")
    assert isinstance(r, ClapRanker) and r.model is model and r.tokenizer is tok and r.config is rc and r.truncation == "head"
    const = type("Const", (Ranker,), {"forward": lambda self, **kw: torch.zeros(1, 1)})()
    ens = create_ranker({"kind": "ensemble", "rankers": {"clap": ({"kind": "clap", "checkpoint": d}, 0.4), "other": (const, 0.6)}},
                        model=model, tokenizer=tok)
    assert isinstance(ens, EnsembleRanker) and ens.weights == [0.4, 0.6] and not ens.needs_spans
    assert isinstance(ens.rankers[0], ClapRanker) and ens.rankers[0].config.checkpoint == d and ens.rankers[1] is const
    with pytest.raises(ValueError, match="truncation"):
        ClapRanker(rc, model=model, tokenizer=tok, truncation="fusion")
    # a directory that is no checkpoint is said so, not turned into "third-party"
    with pytest.raises(FileNotFoundError, match="config.json"):
        create_ranker(rc)
    import sam_audio_amd
    assert sam_audio_amd.ClapRanker is ClapRanker and sam_audio_amd.ClapRankerConfig is ClapRankerConfig
    assert sam_audio_amd.ClapTower is clap.ClapTower


def test_pt_checkpoints_are_refused(tmp_path):
    pt = tmp_path / "630k-best.pt"
    torch.save({"state_dict": {}}, pt)
    for path in (str(pt), str(tmp_path / "missing.pt")):
        with pytest.raises(ValueError, match="convert"):
            clap.load_checkpoint(path)
        with pytest.raises(ValueError, match="convert"):
            clap.ClapTower.from_pretrained(path)
    (tmp_path / "config.json").write_text("{}")
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        clap.load_checkpoint(str(tmp_path))


def test_checkpoint_directory_round_trip(tmp_path):
    """ClapModel.save_pretrained -> load_checkpoint -> convert_clap: every engine tensor the tower asks for, by Hugging Face key names"""
    model = synthetic.init_clap_model(synthetic.clap_config("mini"), seed=2)
    model.save_pretrained(str(tmp_path))
    (tmp_path / "preprocessor_config.json").write_text(__import__("json").dumps(synthetic.CLAP_MINI_FRONTEND))
    config, frontend, sd = clap.load_checkpoint(str(tmp_path))
    assert frontend == synthetic.CLAP_MINI_FRONTEND and set(sd) <= set(model.state_dict())
    c = clap.tower_config(config, frontend)
    assert (c.fft_size, c.hop, c.max_length, c.spec_size, c.num_mel_bins, c.embed_dim, c.num_stages, c.window_size) == (64, 8, 2_000, 64, 16, 96, 3, 4)
    assert list(c.depths)[:3] == [2, 2, 2] and list(c.heads)[:3] == [4, 8, 16] and (c.text_hidden, c.text_max_positions, c.text_pad_id) == (64, 40, 1)
    assert (c.mlp_ratio, c.patch_norm, c.enable_fusion, c.projection_dim, c.text_layers) == (4, 1, 0, 64, 2)
    t = clap.convert_clap(sd, c, frontend, "cpu")
    assert t["a.S1.B1.wqkv"].shape == (576, 192) and t["a.S1.B1.rpb"].shape == (49, 8) and t["a.S0.merge.w"].shape == (192, 384)
    assert t["t.L1.wqkv"].shape == (192, 64) and t["t.type"].shape == (64,) and t["fe.bank"].shape == (33, 16) and t["a.patch.w"].shape == (96, 16)
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in t.values())
    real = clap.tower_config(synthetic.clap_config("real"))
    assert (real.fft_size, real.hop, real.max_length, real.spec_size, real.embed_dim, real.num_stages) == (1024, 480, 480_000, 256, 96, 4)
    assert list(real.depths) == [2, 2, 6, 2] and list(real.heads) == [4, 8, 16, 32] and real.text_max_positions == 514


def test_batch_norm_fold_and_relative_position_index_are_the_modules():
    model = synthetic.init_clap_model(synthetic.clap_config("mini"), seed=4).double()
    enc = model.audio_model.audio_encoder
    bn = enc.batch_norm
    scale, shift = clap.fold_batch_norm(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    x = 40 * torch.randn(2, 1, 251, 16, dtype=torch.float64) - 30
    with torch.no_grad():
        want = bn(x.transpose(1, 3)).transpose(1, 3)            # modeling_clap.py:812-814
    assert (x * scale + shift - want).abs().max() < 1e-12
    assert bn.running_var.std() > 10 and bn.running_mean.abs().mean() > 5       # (the synthetic statistics are not the identity)
    for stage in enc.layers:
        for block in stage.blocks:
            att = block.attention.self
            assert torch.equal(clap.relative_position_index(4), att.relative_position_index)
            assert att.relative_position_bias_table.abs().mean() > 0.1            # (nor are the bias tables zeros)
    from transformers.models.clap.modeling_clap import ClapAudioSelfAttention
    att8 = ClapAudioSelfAttention(synthetic.clap_config("real").audio_config, 96, 4, 8)
    assert torch.equal(clap.relative_position_index(8), att8.relative_position_index)


def test_header_and_python_wiring():
    header = open(os.path.join(ROOT, "include", "samaudio.h")).read()
    new = ["samaudio_op_logmel", "samaudio_logmel_frames"] + list(hip._CLAP_PROTOS)
    assert len(new) == 14
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, header) and name in hip.EXPORTED_SYMBOLS, name
    for name in ("samaudio_clap_create", "samaudio_clap_destroy", "samaudio_clap_set_tensor", "samaudio_clap_finalize",
                 "samaudio_clap_workspace_bytes", "samaudio_clap_set_workspace", "samaudio_clap_audio_embed", "samaudio_clap_text_embed",
                 "samaudio_clap_score"):
        assert name in hip._CLAP_PROTOS
    assert "SAMAUDIO_CLAP_INT16_SCALE 32767.0f" in header and "unpinned" in header and "pinned to ClapFeatureExtractor" in header
    fields = header[: header.index("} samaudio_clap_config;")].rsplit("typedef struct {", 1)[1]
    declared = re.findall(r"\b([a-z_0-9]+)(?:\[4\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert declared == [f[0] for f in hip.ClapConfig._fields_]
    kernels_h = open(os.path.join(ROOT, "sam_audio_amd", "csrc", "kernels.h")).read()
    for name in ("launch_clap_logmel", "launch_clap_patch_embed", "launch_swin_window_attn", "launch_swin_patch_merge",
                 "launch_clap_text_embed", "launch_clap_score"):
        assert re.search(r"__attribute__\(\(weak\)\)\s+hipError_t\s+%s\(" % name, kernels_h)
    csrc = os.path.join(ROOT, "sam_audio_amd", "csrc")
    assert re.search(r"__global__[^;{]*\bclap_logmel_kernel\(", open(os.path.join(csrc, "kernels.hip")).read())
    kernels = open(os.path.join(csrc, "clap_kernels.hip")).read()
    for name in ("clap_patch_embed_kernel", "swin_window_attn_kernel", "swin_patch_merge_kernel", "clap_text_embed_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % name, kernels)
    build = open(os.path.join(csrc, "build.sh")).read()
    assert " clap_kernels " in build and " clap " in build and "clap.h -nt" in build
    for operands in ("bf16", "fp16"):          # both builds carry the same fp32 towers
        assert all(hasattr(hip.lib(operands), name) for name in new)
    x = torch.zeros(2, 800)
    with pytest.raises(hip.SamAudioHipError, match="no CPU fallback"):
        clap.logmel(x)


def test_library_refuses_bad_logmel_arguments_without_a_gpu():
    """argument validation happens before any launch, so it is checked on the real library here"""
    lib = hip.lib()
    buf = (C.c_float * 4096)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)
    assert lib.samaudio_logmel_frames(480_000, 480) == 1001 and lib.samaudio_logmel_frames(2_000, 8) == 251
    assert lib.samaudio_logmel_frames(0, 8) == -1 and lib.samaudio_logmel_frames(100, 0) == -1

    def call(wav=p, rows=2, row_stride=3_000, lengths=(1_000, 3_000), offsets=(0, 1_000), max_length=2_000, fft=64, hop=8, n_mels=16,
             tables=p, bank=p, scale=p, shift=p, out=p):
        lens = (C.c_int64 * len(lengths))(*lengths) if lengths is not None else None
        offs = (C.c_int64 * len(offsets))(*offsets) if offsets is not None else None
        return lib.samaudio_op_logmel(wav, rows, row_stride, lens, offs, max_length, 1, fft, hop, n_mels, tables, bank, scale, shift,
                                      out, None)

    for kw in (dict(wav=null), dict(lengths=None), dict(tables=null), dict(bank=null), dict(out=null), dict(scale=null),
               dict(shift=null), dict(rows=0), dict(rows=70_000, lengths=(1,) * 70_000, offsets=None), dict(hop=0), dict(n_mels=0),
               dict(fft=32), dict(fft=4096), dict(fft=96), dict(max_length=32), dict(max_length=1 << 30), dict(lengths=(0, 3_000)),
               dict(lengths=(1_000, 3_001)), dict(offsets=(0, 1_001)), dict(offsets=(0, -1))):
        assert call(**kw) == hip.ERR_ARG, kw
        assert b"logmel" in lib.samaudio_last_error(), kw
    h = C.c_void_p()
    cfg = clap.tower_config(synthetic.clap_config("mini"), synthetic.CLAP_MINI_FRONTEND)
    cfg.enable_fusion = 1
    assert hip.clap_lib().samaudio_clap_create(C.byref(cfg), C.byref(h)) == hip.ERR_ARG


def test_frontend_kernel_on_the_simulator():
    """the front-end tests of tests/test_clap_gpu.py at clap-mini on the SIMT simulator (the real kernel code compiled for the host, as
    tests/test_simt_cpu.py runs its selections).  The towers' kernels live in sources of their own, which the simulator library - built
    from a fixed list of files - does not contain; they run on the GPU only."""
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt")
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_clap_gpu.py",
                        "-k", "frontend and not real and not 2048"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail
