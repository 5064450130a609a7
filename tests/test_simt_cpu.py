"""Runs a light subset of the `-m gpu` tests on the functional SIMT simulator (oracle/simt/: every product source,
kernels included, compiled unchanged for the host; one fiber per GPU thread, lane-exact MFMA / DMA / DPP emulation).

This is what stands in for hardware in the CPU suite: the kernels' FUNCTION (indexing, fragment layouts, swizzles,
masks, epilogues) is exercised through the same C ABI and the same test bodies that run on MI355X.  The simulator
itself is calibrated by the GPU-verified kernels: all of tests/test_kernels_gpu.py, test_gemm_gpu.py and
test_gemm2_gpu.py pass on it.  It models no timing and no asynchrony - races and performance stay with the GPU runs.
The full sweep (incl. the codec-heavy end-to-end tests, ~80 min) is run by hand:
    SAMAUDIO_EMU_DRYRUN=simt python -m pytest tests -m gpu -q
"""
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout, **extra):
    env = dict(os.environ, SAMAUDIO_EMU_DRYRUN="simt", **extra)
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    return tail


def test_every_non_gemm_kernel_on_the_simulator():
    out = _run(["tests/test_kernels_gpu.py"], 600)
    assert " passed" in out and "failed" not in out


def test_no_kernel_consumes_lds_it_never_wrote():
    """SAMAUDIO_SIMT_POISON=1: every LDS array is filled with 0xFF bytes (NaN as fp32 and bf16) before each workgroup,
    as a real CU's LDS holds whatever ran there before - the class of bug behind DESIGN.md section 8 (an MFMA operand
    of padding lanes read past the rows the kernel had written: 0 x NaN).  All non-GEMM kernels, both candidates and
    the new streaming kernels; the GEMM sweep with poison is part of the by-hand run."""
    out = _run(["tests/test_kernels_gpu.py", "tests/test_zz_next_rows_gpu.py", "-k",
                "not (judge or separate or predict or frame_logits or peav_transformer or visual_prompt)"], 900,
               SAMAUDIO_SIMT_POISON="1")
    assert " passed" in out and "failed" not in out


def test_gemm_kernels_on_the_simulator():
    """One pass over every shipped tile variant and epilogue of gemm2.hip plus the fp32 / bf16 kernels of gemm.hip."""
    out = _run(["tests/test_gemm2_gpu.py", "tests/test_gemm_gpu.py", "-k", "not conv_forms"], 900)
    assert " passed" in out and "failed" not in out


def test_pipelined_gemm_kernels_with_dma_landing_as_late_as_the_isa_allows():
    """SAMAUDIO_SIMT_DMA=late: a global_load_lds lands only when the issuing wave's s_waitcnt vmcnt(N) / __syncthreads
    retires it, so a kernel whose counted waits let a wave read a slab too early reads stale LDS here.  (Mutation check
    done by hand: loosening gemm2.hip's counts by 8 fails all 43 tests of this file in this mode and none in the
    default one.)  Covers the ring tiles, conv7h / the fused residual units and the 8-phase kernels."""
    env_extra = {"SAMAUDIO_SIMT_DMA": "late"}
    old = {k: os.environ.get(k) for k in env_extra}
    os.environ.update(env_extra)
    try:
        out = _run(["tests/test_gemm2_gpu.py", "-k", "not conv_forms"], 1200)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert " passed" in out and "failed" not in out


def test_new_streaming_kernels_and_the_peav_transformer_on_the_simulator():
    out = _run(["tests/test_zz_next_rows_gpu.py", "-k",
                "masked_groupnorm or layernorm_rows or peav_transformer or frame_logits"], 900)
    assert "10 passed" in out


def test_round2_policy_tail_split_and_vision_tower_on_the_simulator():
    """The shipped (round-2) tile policy end to end on small shapes: the 8-phase launch split into whole rounds + 128x128
    quadrant tail must be bitwise invisible, and the PE-Core vision tower (tests/test_vit_gpu.py: every structural switch,
    fp32 and bf16, uint8 video -> resize -> tower) must match its oracle with the real kernel code."""
    out = _run(["tests/test_gemm2_gpu.py", "tests/test_vit_gpu.py", "-k",
                "tail_split or 8phase_family or (test_vit_gpu and not checkpoint)"], 900)
    assert " passed" in out and "failed" not in out


def test_t5_prompt_encoder_on_the_simulator():
    """The T5 encoder stack (tests/test_t5_gpu.py: ragged masks, > 64 keys per row, 16 / 32 / 128-wide heads, ReLU and
    gelu_new, error paths, the T5TextEncoder wrapper) against transformers' T5EncoderModel with the real kernel code."""
    out = _run(["tests/test_t5_gpu.py"], 600)
    assert " passed" in out and "failed" not in out


def test_modernbert_text_tower_on_the_simulator():
    """The Judge's / PE-A-Frame's ModernBERT text tower (tests/test_mbert_gpu.py: every hidden state, ragged masks, sequences
    longer than the local window, both layer patterns, error paths) against transformers' ModernBertModel with the real
    kernel code."""
    out = _run(["tests/test_mbert_gpu.py"], 600)
    assert " passed" in out and "failed" not in out


def test_operand_sharing_x3_kernel_with_dma_landing_as_late_as_the_isa_allows():
    """gemm8x_kernel (round 6: the 8-phase kernel that shares operand tiles and fragments between the three products of the compensated
    mode's K-concatenated operands, GemmParams.flags bit 15) against the plain walk and - bit for bit - against gemm8s_kernel's walk of
    the same order, in both weight layouts, with every DMA landing only when its hand-counted wait retires it (vmcnt(4) / vmcnt(8) /
    vmcnt(0) per product: a wait placed behind the wrong barrier in an experimental two-phase form failed exactly here)."""
    env_extra = {"SAMAUDIO_SIMT_DMA": "late"}
    old = {k: os.environ.get(k) for k in env_extra}
    os.environ.update(env_extra)
    try:
        out = _run(["tests/test_x3_gpu.py", "-k", "sharing_the_operand_tiles"], 600)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert "3 passed" in out and "failed" not in out


def test_layer_kernels_on_the_simulator_plain_and_with_poisoned_lds():
    """A light subset of tests/test_layer_kernels_gpu.py (the kernels a DiT layer launches, each against float64 through its own hook):
    the norm family at D = 512 / 3072, all of qkv_prep, cross-attention and the probability kernels (both head widths, 8- and 16-token
    slots), three fold3 shapes, and the three self-attention kernels at both head widths with T = 1, 65 (64-row workgroups, incl. a
    first key tile masked whole) and 128 (128-row workgroups) under every mask kind - once plain and once with every LDS array full
    of NaN patterns before each workgroup: the fully masked tile and T = 1 are where a kernel could consume LDS it never wrote.
    141 tests; measured 105 s of wall time for the two runs inside the CPU suite on an 8-core host (the whole file by hand: 70 s plain,
    4.5 min poisoned)."""
    subset = ["tests/test_layer_kernels_gpu.py", "-k",
              "(self_attention and (-1- or -65- or -128-)) or (not self_attention and not fold3 and not 2816) or "
              "(fold3 and (3-8-3-4 or 11-16-3-4 or 16-16-5-2))"]
    for extra in ({}, {"SAMAUDIO_SIMT_POISON": "1"}):
        out = _run(subset, 600, **extra)
        assert "141 passed" in out and "failed" not in out and "skipped" not in out, out


def test_tower_kernels_on_the_simulator_plain_and_with_poisoned_lds():
    """All of tests/test_tower_kernels_gpu.py (the kernels only the towers launch, each against float64 through its own hook; bfloat16
    library, so every case but the fp16 ones - Lt = 512 and the 129 x 8200 GEGLU included: nothing is left out) - once plain and once with
    every LDS array full of NaN patterns before each workgroup: the pooling kernel's waves without a token (T < 4) and the attention
    rows without an allowed key are where a kernel could consume LDS it never wrote.  125 tests; measured 10 s plain and 30 s poisoned
    on an 8-core host."""
    for extra in ({}, {"SAMAUDIO_SIMT_POISON": "1"}):
        out = _run(["tests/test_tower_kernels_gpu.py"], 600, **extra)
        assert "125 passed" in out and "failed" not in out and "skipped" not in out, out


def test_x3_launch_form_flags_on_the_simulator_plain_and_with_poisoned_lds():
    """tests/test_x3_invariance_gpu.py case (d) in bf16x3 (the whole-path bitwise invariances of the compensated modes): 3 rows of 40
    frames, here on a 'tiny' model with one evaluation of the field per flag - 256 x 256 tiles wherever N allows (gemm8x at M = 120:
    every tile mostly padding rows), the three wave-role settings of the pipelined 128 x 128 kernel and the three epilogue forms (the
    general one sends w2 through the stand-alone split3 into x3u), each bit-identical to the run with all flags at 0 - once plain and
    once with every LDS array full of NaN patterns before each workgroup: the padding rows of a 256-row tile and the LDS-staged epilogue
    are where such a launch could consume LDS it never wrote.  1 test (9 evaluations) per run; measured 93 s of wall time for the two
    runs on an 8-core host (at the hardware's 'mini' dims: 41 s plain, 3.5 min poisoned - too long for this suite).
    Left out: every other case of the file that can run here at all (layout (c) at one stream, codec (e), candidates (f), reload (g) at
    one stream) goes through the DAC-VAE, minutes per separate() on the simulator - (d) at 'mini' dims, (f) and the first case of (g)
    together did not finish in 20 minutes; (a), (b) and the D = 2048 flags are hardware only (4000 rows; streams)."""
    for extra in ({}, {"SAMAUDIO_SIMT_POISON": "1"}):
        out = _run(["tests/test_x3_invariance_gpu.py", "-k", "launch_form_flags_leave_the_latent_bit_identical"], 600, **extra)
        assert "1 passed" in out and "failed" not in out, out


def test_glue_kernels_on_the_simulator_plain_and_with_poisoned_lds():
    """All of tests/test_glue_kernels_gpu.py (the small kernels between the compute kernels, each against float64 or bit for bit through
    its own hook; bfloat16 library and no CLAP kernels, so every case but the fp16 and CLAP ones - the cases above a grid cap
    included: nothing is left out) - once plain and once with every LDS array full of NaN patterns before each workgroup: the
    sentinel's and the checksum's tree reductions are where a kernel could fold LDS it never wrote.  206 tests; measured 4 s plain and
    12 s poisoned on an 8-core host."""
    for extra in ({}, {"SAMAUDIO_SIMT_POISON": "1"}):
        out = _run(["tests/test_glue_kernels_gpu.py"], 600, **extra)
        assert "206 passed" in out and "failed" not in out and "skipped" not in out, out


def test_norm_kernels_on_the_simulator_plain_and_with_poisoned_lds():
    """All of tests/test_norm_kernels_gpu.py (the norm kernels everything else stands on - rmsnorm_mod, layernorm_rows, layernorm_accum,
    groupnorm_silu, masked_groupnorm_silu - each against float64 through its own hook, with eps in reach; bfloat16 library, so every
    case but the fp16 ones, the 129 x 4096 cases above the apply kernels' grid cap included: nothing is left out) - once plain and once
    with every LDS array full of NaN patterns before each workgroup: the fp64 tree reductions of gn_partial_kernel and
    mgn_partial_kernel, whose chunks behind the data fold nothing but what the threads themselves stored, are where LDS could be
    folded unwritten.  200 tests; measured 11 s plain and 82 s poisoned on an 8-core host (the six 129 x 4096 cases: 6.5 s each
    poisoned)."""
    for extra in ({}, {"SAMAUDIO_SIMT_POISON": "1"}):
        out = _run(["tests/test_norm_kernels_gpu.py"], 600, **extra)
        assert "200 passed" in out and "failed" not in out and "skipped" not in out, out
