"""The numbers behind the GEMM selection layer are a debugging ABI (no GPU): GemmVariant ids (samaudio_debug_force_gemm_variant,
the logs under profiles/), the bits of GemmParams.flags (hip.py builds launches from them), the debug switches
(SAMAUDIO_DEBUG_FLAGS=N=V is parsed numerically) and the profile names of the variants (keys of the profile records and of bench.py's
attribution).  The C++ side is read from the source text; sam_audio_amd/hip.py must mirror it name for name, and a renumbering or a
renamed kernel string must fail here."""
import os
import re

from sam_audio_amd import hip

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sam_audio_amd", "csrc")


def _src(name):
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", text)   # (no string of these files holds "//")


def _assignments(body, known=None):
    """'A = 1, B = A | 2' -> {A: 1, B: 3}"""
    out = dict(known or {})
    for name, expr in re.findall(r"(\w+)\s*=\s*([^,;{}]+)", body):
        out[name] = int(eval(expr, {"__builtins__": {}}, out))
    return {k: v for k, v in out.items() if not known or k not in known}


def _enum(text, head):
    m = re.search(re.escape(head) + r"\s*\{([^}]*)\}", text)
    assert m, head
    return _assignments(m.group(1))


def _gemm_flags():
    out = {}
    for body in re.findall(r"constexpr int ((?:GEMM_FLAG|GEMM_QUANT)_\w+\s*=[^;]+);", _src("common.h")):
        out.update(_assignments(body, out))
    return out


def _debug_values():
    out = {}
    for body in re.findall(r"enum : int \{([^}]*)\}", _src("kernels.h")):
        vals = _assignments(body)
        if all(k.startswith("DBG_") for k in vals):
            out.update(vals)
    return out


def _variant_table():
    m = re.search(r"kGemmVariantTable\[\] = \{(.*?)\n\};", _src("kernels.h"), re.S)
    assert m
    return re.findall(r'\{(GV_\w+), (FAM_\w+), "([^"]*)", "([^"]*)"\}', m.group(1))


# today's values: what the tests, the tools and the logs under profiles/ use
VARIANT_IDS = {0, 1, 2, 22, 25, 26, 27, 28, 29, 32, 33, 34, 35, 36, 37, 38, 39}
DEBUG_FLAGS = {11, 16, 18, 19, 21, 24, 26, 27, 29, 30, 31, 33, 35, 36, 38}
FLAG_BITS = {0, 1, 6, 7, 9, 10, 11, 12, 13, 14, 15}   # single-bit switches; bits 2-3 / 4-5 are the two rounding fields, bit 8 is free
NAMES_16 = {0: "gemm_bf16_128x128", 1: "gemm_bf16_128x64", 2: "gemm_bf16_128x32", 22: "gemm8_bf16_256x256_8phase",
            25: "gemm2_bf16_128x128_s2", 26: "gemm2_bf16_64x128_s3", 27: "gemm8s_bf16_128x128", 28: "gemm2_bf16_256x64_s2",
            29: "gemm2_bf16_128x128_k32_s3", 32: "gemm2_bf16_128x64_k32_s2", 33: "gemm2_bf16_64x128_k32_s3",
            34: "gemm2_bf16_128x192_k32_s3", 35: "conv7h_bf16"}
NAMES_32 = {0: "gemm_f32_128x128", 1: "gemm_f32_128x64", 2: "gemm_f32_128x32", 36: "gemm_f32x3_128x96", 37: "gemm_f32x3_128x128",
            38: "gemm_f32x3_128x64", 39: "gemm_f32x3_128x32"}


def _mirrored(prefixes):
    return {k: v for k, v in vars(hip).items() if k.startswith(prefixes) and isinstance(v, int)}


def test_gemm_variant_ids_and_their_mirror():
    ids = _enum(_src("kernels.h"), "enum GemmVariant : int")
    assert set(ids.values()) == VARIANT_IDS and len(ids) == len(VARIANT_IDS)
    m = re.search(r"constexpr int kGemmVariants = (\d+);", _src("kernels.h"))
    assert m and int(m.group(1)) == 40 and max(ids.values()) < 40
    assert _mirrored("GV_") == ids


def test_gemm_flag_bits_and_their_mirror():
    flags = _gemm_flags()
    single = {k: v for k, v in flags.items() if k.startswith("GEMM_FLAG_") and not k.endswith(("_SHIFT", "_MASK", "_EPI_LEAN"))}
    assert sorted(single.values()) == sorted(1 << b for b in FLAG_BITS), single
    want = dict(GEMM_FLAG_EPI_ACC=1, GEMM_FLAG_NO_TAIL_SPLIT=2, GEMM_FLAG_EPI_LINEAR=64, GEMM_FLAG_EPI_ROWS=128, GEMM_FLAG_EPI_LEAN=192,
                GEMM_FLAG_OUT_ALT=512, GEMM_FLAG_OPND_ALT=1024, GEMM_FLAG_W_KTM=2048, GEMM_FLAG_OUT_SPLIT3=4096, GEMM_FLAG_X3_FLY=8192,
                GEMM_FLAG_W_FLY16=16384, GEMM_FLAG_X3_SHARE=32768, GEMM_FLAG_QUANT_A_SHIFT=2, GEMM_FLAG_QUANT_W_SHIFT=4,
                GEMM_FLAG_QUANT_MASK=3, GEMM_QUANT_NONE=0, GEMM_QUANT_BF16=1, GEMM_QUANT_FP16=2)
    assert flags == want
    assert _mirrored(("GEMM_FLAG_", "GEMM_QUANT_")) == flags


def test_debug_switches_and_their_mirror():
    switches = _enum(_src("kernels.h"), "enum DebugFlag : int")
    assert set(switches.values()) == DEBUG_FLAGS and len(switches) == len(DEBUG_FLAGS)
    assert list(switches.values()) == sorted(switches.values()), "one enumerator per switch, in numeric order"
    values = _debug_values()
    assert values == dict(DBG_WS_ALWAYS=1, DBG_WS_NEVER=2, DBG_WS_ALWAYS_GRID3=3, DBG_EPI_GENERAL=1, DBG_EPI_LINEAR=2, DBG_EPI_ROWS=3,
                          DBG_ROLES_NONE=1, DBG_ROLES_PROD0=2, DBG_ROLES_PROD2=3)
    assert _mirrored("DBG_") == {**switches, **values}


def test_variant_table_has_one_row_per_id_and_todays_names():
    ids = _enum(_src("kernels.h"), "enum GemmVariant : int")
    rows = _variant_table()
    assert sorted(r[0] for r in rows) == sorted(ids), "one row per GemmVariant"
    assert {ids[r[0]]: r[2] for r in rows if r[2]} == NAMES_16
    assert {ids[r[0]]: r[3] for r in rows if r[3]} == NAMES_32
    assert {ids[r[0]] for r in rows if r[1] == "FAM_8PHASE"} == {22, 27}
    # every name string lives in the table and nowhere else in the library's sources
    every = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h")))
    for name in list(NAMES_16.values()) + list(NAMES_32.values()) + ["gemm8s_bf16_128x128_tail"]:
        assert every.count('"' + name + '"') == 1, name
