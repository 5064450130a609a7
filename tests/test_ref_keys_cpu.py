"""State-dict key bookkeeping against the REFERENCE's own module tree (pinned in tests/golden/ref_keys_tiny.json, minted by
oracle/gen_golden.py from the reference's own classes) plus the prefixes a genuine checkpoint carries that the separate()
engine ignores.

The reference SAMAudio cannot be instantiated offline (dacvae / perception_models are absent), but its DiT, AlignModalities,
EmbedAnchors and the two Linear layers can: their state-dict keys under the attribute names of reference model.py:80-93
must be exactly this build's expected non-codec keys."""
import json
import os

from sam_audio_amd import preset_config
from sam_audio_amd.weights import expected_keys, split_missing_unexpected

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_expected_keys_equal_the_reference_module_tree():
    with open(os.path.join(GOLDEN, "ref_keys_tiny.json")) as f:
        ref_keys = set(json.load(f))
    assert ref_keys, "empty key fixture"
    cfg = preset_config("tiny")
    ours = {k for k in expected_keys(cfg) if not k.startswith("audio_codec.")}
    assert ours == ref_keys, (sorted(ours - ref_keys)[:5], sorted(ref_keys - ours)[:5])


def test_a_genuine_checkpoint_key_set_loads_strictly():
    """reference model.py:82-83,346-359: checkpoint.pt carries `vision_encoder.model.*` (PerceptionEncoder is a
    submodule and not in the skip regex) and none of text_encoder / rankers / span_predictor."""
    cfg = preset_config("tiny")
    keys = list(expected_keys(cfg))
    genuine = keys + ["vision_encoder.model.visual.conv1.weight", "vision_encoder.model.visual.proj",
                      "vision_encoder.model.logit_scale"]
    assert split_missing_unexpected(genuine, cfg) == ([], [])
    assert split_missing_unexpected(genuine + ["vision_encoderX.w"], cfg) == ([], ["vision_encoderX.w"])


def test_judge_strict_load_tolerates_the_whole_quantizer_and_a_decoder():
    """reference codec.py:62-63: DACVAEEncoder keeps `model.quantizer` entirely (in_proj AND out_proj); a state dict saved
    from a full DACVAE also holds `decoder.*`.  Both are present-but-unused for the Judge and must not fail strict."""
    import re
    src = open(__import__("sam_audio_amd.judge", fromlist=["x"]).__file__).read()
    m = re.search(r'unused = re\.compile\(r"(.+?)"\)', src)
    assert m, "judge.load_state_dict lost its tolerated-key rule"
    unused = re.compile(m.group(1))
    assert unused.search("audio_codec.quantizer.out_proj.weight_g")
    assert unused.search("audio_codec.quantizer.out_proj.bias")
    assert unused.search("audio_codec.decoder.model.0.weight_v")
    assert not unused.search("audio_codec.quantizer.in_proj.weight_g")
    assert not unused.search("audio_codec.encoder.block.0.weight")
    assert not unused.search("transformer.layers.0.self_attn.q_proj.weight")
