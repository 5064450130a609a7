"""Kernel-level parity of the norm kernels everything else stands on, one C-ABI hook each (include/samaudio.h, csrc/api.hip):

    rmsnorm_mod_reg_kernel<., 12> (D <= 3072), rmsnorm_mod_kernel (wider)            samaudio_op_rmsnorm_mod
    layernorm_rows_reg_kernel<., 4> (D <= 1024), layernorm_rows_kernel (wider)       samaudio_op_layernorm_rows
    layernorm_accum_kernel                                                           samaudio_op_layernorm_accum
    gn_partial_kernel + gn_apply_kernel                                              samaudio_op_groupnorm_silu
    mgn_partial_kernel + mgn_apply_kernel                                            samaudio_op_masked_groupnorm_silu

and one eps-visible case each for samaudio_op_rmsnorm_gs, _headnorm_layers and _qkv_prep_hd, which their own files pin on O(1) data.

Conventions, helpers and the bound are those of tests/test_tower_kernels_gpu.py (imported, not copied).  Every reference is the
operation written out in float64 torch on the fp32 inputs (all five kernels read fp32); _cmp is given that statement and the same
statement evaluated in float32 and allows 8 x the float32 statement's largest error (floor 2^-23 max|ref|), plus half a storage-type ulp
per element for a 16-bit output.  Outputs start as NaN with a guard row or item behind them; owned elements come back finite (a NaN
fails _cmp); the guard, the halo rows and the inputs - the bytes behind D in a strided row included - keep their bits.

Data: an "ordinary" block randn * 2 + 0.3 at eps 1e-5, an "offset" block randn + 8 at eps 1e-6 for the mean-subtracting norms, and an
"eps-visible" block randn * 3e-3 (+ 0.05 for the mean-subtracting norms) whose variance / mean square is about 1e-5: it is run at eps
1e-5 AND 1e-6, each against its own statement, and _eps_visible asserts that the two float64 statements differ by more than 100 x the
bound (10 x the bound plus the half ulp for a 16-bit output) - a property of the inputs alone.  Weights and biases are random per column.

Passed counts: 292 on MI355X (both libraries), 200 on the SIMT simulator plain and with poisoned LDS (SAMAUDIO_EMU_DRYRUN=simt: bfloat16
library only, so the fp16 / fp16x3 cases are hardware only; nothing else is left out, the 129 x 4096 cases included), 196 passed + 4
skipped under the launcher emulation (SAMAUDIO_EMU_DRYRUN=1: its own C++ versions of the five launchers meet the same statements; head
width 64 is not in that build).  Measured figures and the seeded faults: profiles/norm_kernels/.
"""
import pytest
import torch

from sam_audio_amd import hip
from tests import test_glue_kernels_gpu as G
from tests import test_layer_kernels_gpu as L
from tests import util
from tests.test_tower_kernels_gpu import (FACTOR, LAUNCHER_EMU, NAN, SIM, STORAGE, _act, _all_nan, _at, _bit_zero, _cmp, _code, _dev,
                                          _lib, _mk, _nan, _ok, _rnd, _same_bits, _ulp16)

pytestmark = pytest.mark.gpu
EPS_PAIR = (1e-5, 1e-6)


def _bound(want, f32):
    """the bound _cmp prints and asserts (without the half ulp of a 16-bit output)"""
    return max(FACTOR * (f32.double() - want).abs().max().item(), 2.0 ** -23 * want.abs().max().item())


def _eps_visible(tag, wants, f32s, dtype):
    """`wants`, `f32s`: the statement at eps 1e-5 and at 1e-6 in float64 and float32.  The two float64 statements are further apart than
    100 x the larger of the two bounds - and, for a 16-bit output, than 10 x (bound + half a storage ulp at the largest |ref|: bfloat16's
    half ulp at 2 is 2^-8, a hundred of them would be above any normalised output)."""
    gap = (wants[0] - wants[1]).abs().max().item()
    bound = max(_bound(w, f) for w, f in zip(wants, f32s))
    print(f"{tag}: the statements at eps 1e-5 and 1e-6 differ by {gap:.3e} = {gap / bound:.0f} x the bound {bound:.3e}")
    assert gap > 100 * bound, f"{tag}: eps is not visible in this data ({gap} against a bound of {bound})"
    if dtype != torch.float32:
        top = max(w.abs().max().item() for w in wants)
        room = bound + 0.5 * _ulp16(torch.tensor(top), dtype).item()
        assert gap > 10 * room, f"{tag}: eps is not visible in {dtype} ({gap} against {room})"


def _wb(D, seed):
    """weight and bias per column: never all ones / all zeros"""
    return _mk((D,), seed, 0.3) + 1, _mk((D,), seed + 1, 0.5)


def _block(kind, shape, seed, centred):
    """`centred`: the norm subtracts a mean"""
    if kind == "ordinary":
        return _mk(shape, seed, 2.0) + 0.3
    if kind == "offset":
        return _mk(shape, seed) + 8
    return _mk(shape, seed, 3e-3) + (0.05 if centred else 0.0)   # "visible"


# what each mean-subtracting test runs: (block, eps); the two "visible" entries also go through _eps_visible
RUNS_CENTRED = [("ordinary", 1e-5), ("offset", 1e-6), ("visible", 1e-5), ("visible", 1e-6)]
RUNS_RMS = [("ordinary", 1e-5), ("visible", 1e-5), ("visible", 1e-6)]


# ---------------------------------------------------------------------------------------------------------------------
# rmsnorm_mod
# ---------------------------------------------------------------------------------------------------------------------
def _rms_stmt(x, w, eps, dtype, shift=None, scale=None):
    """x [rows, D]; shift / scale: (table [D], time-vector part [rows, D]) or None (plain RMSNorm)"""
    x = x.to(dtype)
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.to(dtype)
    if shift is None:
        return y
    return y * (1 + (scale[0].to(dtype) + scale[1].to(dtype))) + (shift[0].to(dtype) + shift[1].to(dtype))


# form -> (time-vector items, floats per time-vector row / D, tvec_ld / D, shift_off / D, scale_off / D, rows_per_batch, rows)
RMS_FORMS = {
    "none": (0, 0, 0, 0, 0, 2, (1, 5, 9)),
    "shared": (3, 2, 0, 1, 0, 2, (1, 5, 9)),      # tvec_ld = 0: every row takes item 0; items 1, 2 hold NaN
    "item1": (3, 2, 2, 0, 1, 1, (3,)),            # rows = 3 items of rows_per_batch rows
    "item3": (3, 2, 2, 0, 1, 3, (9,)),
    "engine": (3, 6, 6, 3, 4, 3, (1, 5, 9)),      # a 6 D row per item, this norm's shift / scale at 3 D / 4 D, the other columns NaN
}


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("form", list(RMS_FORMS))
@pytest.mark.parametrize("D", [4, 256, 260, 3072, 3076, 3328])
def test_rmsnorm_mod(gpu, prec, form, D):
    """D = 4: one float4, one lane; 256 / 260: n4 = 64 / 65, the first register slot full and the second begun; 3072: the last of the
    12 slots full; 3076: the first width of the two-pass kernel; 3328: its 14th pass.  rows 1 / 5 / 9: a partial workgroup, one and a
    row, two and a row.  Time-vector forms: see RMS_FORMS ("none" passes tvec and both tables as null: T5's and PE-AV's plain RMSNorm)."""
    items, width, ld, s_off, c_off, rpb, rows_list = RMS_FORMS[form]
    dt = _act(prec)
    w, _ = _wb(D, 300 + D)
    tabs = _mk((2, D), 302 + D, 0.2)
    tvec = _mk((max(items, 1), max(width, 1) * D), 303 + D, 0.2)
    held = tvec.clone()
    if form == "shared":
        held[1:] = NAN
    if form == "engine":
        held[:] = NAN
        for off in (s_off, c_off):
            held[:, off * D:(off + 1) * D] = tvec[:, off * D:(off + 1) * D]
    wd, td, tv = _dev(w, gpu), _dev(tabs, gpu), _dev(held, gpu)
    for rows in rows_list:
        item = torch.zeros(rows, dtype=torch.long) if form == "shared" else torch.arange(rows) // rpb
        shift = scale = None
        if items:
            shift = (tabs[0], tvec[item, s_off * D:(s_off + 1) * D])
            scale = (tabs[1], tvec[item, c_off * D:(c_off + 1) * D])
        seen = {}
        for kind, eps in RUNS_RMS:
            x = _block(kind, (rows, D), 310 + rows + D, False)
            xd = _dev(x, gpu)
            out = _nan((rows + 1, D), dt, gpu)
            _ok(prec, _lib(prec).samaudio_op_rmsnorm_mod(hip.ptr(xd), hip.ptr(wd), _at(td[0]) if items else None,
                                                         _at(td[1]) if items else None, hip.ptr(tv) if items else None, ld * D,
                                                         s_off * D, c_off * D, hip.ptr(out), _code(prec), rows, D, rpb, eps,
                                                         util.stream()))
            o = out.cpu()
            assert _all_nan(o[rows]), "the row behind the output was written"
            assert _same_bits(xd, x), "the kernel changed its input"
            want, f32 = _rms_stmt(x, w, eps, torch.float64, shift, scale), _rms_stmt(x, w, eps, torch.float32, shift, scale)
            _cmp(f"rmsnorm_mod {prec} {form} D={D} rows={rows} {kind} eps={eps:g}", o[:rows], want, f32, dt)
            if kind == "visible":
                seen[eps] = (want, f32)
        _eps_visible(f"rmsnorm_mod {form} D={D} rows={rows}", [seen[e][0] for e in EPS_PAIR], [seen[e][1] for e in EPS_PAIR], dt)


# ---------------------------------------------------------------------------------------------------------------------
# layernorm_rows, layernorm_accum
# ---------------------------------------------------------------------------------------------------------------------
def _ln_stmt(x, w, b, eps, dtype):
    x = x.to(dtype)
    c = x - x.mean(-1, keepdim=True)
    return c * torch.rsqrt((c * c).mean(-1, keepdim=True) + eps) * w.to(dtype) + b.to(dtype)


def _ln_launch(gpu, prec, xd, ld, wd, bd, rows, D, eps, f32, act):
    """-> (fp32 output or None, storage-type output or None), guard rows checked; an output that is not asked for is passed as null"""
    o32 = _nan((rows + 1, D), torch.float32, gpu) if f32 else None
    oact = _nan((rows + 1, D), _act(prec), gpu) if act else None
    _ok(prec, _lib(prec).samaudio_op_layernorm_rows(hip.ptr(xd), ld, hip.ptr(wd), hip.ptr(bd), hip.ptr(o32), hip.ptr(oact), _code(prec),
                                                    rows, D, eps, util.stream()))
    res = []
    for o in (o32, oact):
        if o is not None:
            o = o.cpu()
            assert _all_nan(o[rows]), "the row behind the output was written"
            o = o[:rows]
        res.append(o)
    return res


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("stride", ["dense", "gap", "third"])
@pytest.mark.parametrize("D", [4, 256, 260, 1024, 1028, 2048])
def test_layernorm_rows(gpu, prec, stride, D):
    """D = 4; 256 / 260: n4 = 64 / 65; 1024: the last of the 4 register slots full; 1028: the first width of the two-pass kernel; 2048:
    its 8th pass.  x_ld = D, D + 12 (NaN in the gap) and 3 D (every third token of a wider buffer, the others NaN).  Both outputs at once:
    the fp32 one against float64, the storage-type one against float64 and bit for bit the fp32 one rounded; then each output alone
    (the other pointer null): the same bits as in the launch with both.  At D = 1024 and 2048 in the 16-bit libraries, one cross-check:
    the hi block of layernorm_rows_split3 carries the storage-type output's bits (2048: register kernel against two-pass kernel)."""
    dt = _act(prec)
    ld = {"dense": D, "gap": D + 12, "third": 3 * D}[stride]
    w, b = _wb(D, 400 + D)
    wd, bd = _dev(w, gpu), _dev(b, gpu)
    for rows in (1, 5, 9):
        seen = {}
        for kind, eps in RUNS_CENTRED:
            x = _block(kind, (rows, D), 410 + rows + D, True)
            buf = torch.full((rows, ld), NAN)
            buf[:, :D] = x
            xd = _dev(buf, gpu)
            tag = f"layernorm_rows {prec} x_ld={ld} D={D} rows={rows} {kind} eps={eps:g}"
            o32, oact = _ln_launch(gpu, prec, xd, ld, wd, bd, rows, D, eps, True, True)
            want, f32 = _ln_stmt(x, w, b, eps, torch.float64), _ln_stmt(x, w, b, eps, torch.float32)
            _cmp(f"{tag} fp32 output", o32, want, f32)
            _cmp(f"{tag} storage-type output", oact, want, f32, dt)
            assert _same_bits(oact, o32.to(dt)), "the storage-type output is not the fp32 output rounded to nearest even"
            only32, none = _ln_launch(gpu, prec, xd, ld, wd, bd, rows, D, eps, True, False)
            assert none is None and _same_bits(only32, o32), "the fp32 output alone differs from the launch with both"
            none, onlyact = _ln_launch(gpu, prec, xd, ld, wd, bd, rows, D, eps, False, True)
            assert none is None and _same_bits(onlyact, oact), "the storage-type output alone differs from the launch with both"
            assert _same_bits(xd, buf), "the kernel changed its input or the bytes behind D"
            if kind == "visible":
                seen[eps] = (want, f32)
            if kind == "ordinary" and prec != "fp32" and D in (1024, 2048):
                out3 = _nan((rows + 1, 3 * D), dt, gpu)
                rc = _lib(prec).samaudio_op_layernorm_rows_split3(hip.ptr(xd), ld, hip.ptr(wd), hip.ptr(bd), hip.ptr(out3), rows, D, eps,
                                                                  util.stream())
                if not (LAUNCHER_EMU and rc == hip.ERR_STATE):
                    hip.check(rc)
                    assert _same_bits(out3.cpu()[:rows, D:2 * D], oact), "layernorm_rows_split3's hi block is not this kernel's output"
        _eps_visible(f"layernorm_rows x_ld={ld} D={D} rows={rows}", [seen[e][0] for e in EPS_PAIR], [seen[e][1] for e in EPS_PAIR], dt)


def _accum_stmt(x, w, b, gate, acc, eps, dtype):
    return acc.to(dtype) + torch.tanh(torch.tensor(gate, dtype=dtype)) * _ln_stmt(x, w, b, eps, dtype)


@pytest.mark.parametrize("gate", [0.7, -0.3, 20.0, 0.0])
@pytest.mark.parametrize("D", [4, 256, 260, 1028])
def test_layernorm_accum(gpu, gate, D):
    """acc += tanh(gate) LayerNorm(x) in place, fp32 only: gate 0.7 and -0.3, 20 (tanh saturated at 1) and 0 (acc comes back with its
    bits).  acc is random and every launch starts from a fresh copy with a guard row of NaN behind it."""
    w, b = _wb(D, 500 + D)
    wd, bd, gd = _dev(w, gpu), _dev(b, gpu), _dev(torch.tensor([gate]), gpu)
    lib = _lib("fp32")
    for rows in (1, 5, 9):
        acc = _mk((rows, D), 520 + rows + D, 1.5)
        seen = {}
        for kind, eps in RUNS_CENTRED:
            x = _block(kind, (rows, D), 510 + rows + D, True)
            xd = _dev(x, gpu)
            ad = _nan((rows + 1, D), torch.float32, gpu)
            ad[:rows] = acc.to(gpu)
            _ok("fp32", lib.samaudio_op_layernorm_accum(hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(gd), hip.ptr(ad), rows, D, eps,
                                                        util.stream()))
            o = ad.cpu()
            assert _all_nan(o[rows]), "the row behind acc was written"
            assert _same_bits(xd, x), "the kernel changed its input"
            want, f32 = _accum_stmt(x, w, b, gate, acc, eps, torch.float64), _accum_stmt(x, w, b, gate, acc, eps, torch.float32)
            _cmp(f"layernorm_accum gate={gate} D={D} rows={rows} {kind} eps={eps:g}", o[:rows], want, f32)
            if gate == 0.0:
                assert _same_bits(o[:rows], acc), "gate 0 changed acc"
            if kind == "visible":
                seen[eps] = (want, f32)
        if gate != 0.0:
            _eps_visible(f"layernorm_accum gate={gate} D={D} rows={rows}", [seen[e][0] for e in EPS_PAIR], [seen[e][1] for e in EPS_PAIR],
                         torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# groupnorm_silu, masked_groupnorm_silu
# ---------------------------------------------------------------------------------------------------------------------
def _gn_stmt(x, w, b, eps, dtype, mask=None):
    """x [B, T, C]; statistics per item over its valid (frame, channel) entries (all of them without a mask; an item without a valid
    frame has n clamped to 1: mean 0, variance 0); masked frames of the result are zero.  Masked frames of x never enter."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    B, T, Cc = x.shape
    on = torch.ones(B, T, dtype=torch.bool) if mask is None else mask.bool()
    xz = torch.where(on[:, :, None], x, torch.zeros((), dtype=dtype))
    n = (on.sum(1).to(dtype) * Cc).clamp_min(1.0)[:, None, None]
    mean = xz.sum((1, 2), keepdim=True) / n
    c = torch.where(on[:, :, None], xz - mean, torch.zeros((), dtype=dtype))
    var = (c * c).sum((1, 2), keepdim=True) / n
    y = c * torch.rsqrt(var + eps) * w + b
    return torch.where(on[:, :, None], y * torch.sigmoid(y), torch.zeros((), dtype=dtype))


def _gn_items(kind, B, T, Cc, seed):
    """items of one launch differ in scale and offset (a kernel that reads item 0's partials for every item fails)"""
    x = _block(kind, (B, T, Cc), seed, True)
    for i in range(1, B):
        x[i] = x[i] * (1 + 0.5 * i) + (0.02 if kind == "visible" else 0.7) * i
    return x


def _gn_launch(gpu, prec, xd, wd, bd, B, T, Cc, halo, eps, part=None, mask=None):
    """-> out [B + 1, T + 2 halo, C] on the CPU (the item behind the last is a guard), and the partials buffer"""
    out = _nan((B + 1, T + 2 * halo, Cc), _act(prec), gpu)
    if part is None:
        part = torch.zeros(B * 64 * (2 if mask is None else 3), dtype=torch.float64, device=gpu)
    if mask is None:
        rc = _lib(prec).samaudio_op_groupnorm_silu(hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(part), hip.ptr(out), _code(prec), B, T,
                                                   Cc, halo, eps, util.stream())
    else:
        rc = _lib(prec).samaudio_op_masked_groupnorm_silu(hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(mask), hip.ptr(part),
                                                          hip.ptr(out), _code(prec), B, T, Cc, halo, eps, util.stream())
    _ok(prec, rc)
    o = out.cpu()
    assert _all_nan(o[B]), "the item behind the output was written"
    assert _all_nan(o[:B, :halo]) and _all_nan(o[:B, halo + T:]), "halo rows were written"
    return o, part


GN_CASES = ([(T, Cc, B, halo) for T, Cc in ((1, 4), (1, 256), (3, 100), (50, 256)) for B in (1, 3) for halo in (0, 1, 3)]
            + [(129, 4096, 2, 1)])


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("T,Cc,B,halo", GN_CASES)
def test_groupnorm_silu(gpu, prec, T, Cc, B, halo):
    """gn_partial: 64 chunks of ceil(n4 / 64) float4 - (1, 4): one float4, chunks 1 .. 63 empty (lo > hi); (1, 256): one float4 per
    chunk; (3, 100): 75 float4 in chunks of 2, the 38th partial, 26 empty; (50, 256): 50 per chunk; (129, 4096): 132 096 float4, above
    gn_apply's cap of 512 workgroups x 256 (131 072), so its last 1024 float4 come from the second pass of the grid-stride loop.  Item b
    launched alone is item b of the batch bit for bit, and so is a second launch into a partials buffer preset to NaN."""
    dt = _act(prec)
    w, b = _wb(Cc, 600 + Cc)
    wd, bd = _dev(w, gpu), _dev(b, gpu)
    seen = {}
    for kind, eps in RUNS_CENTRED:
        x = _gn_items(kind, B, T, Cc, 610 + T + Cc)
        xd = _dev(x, gpu)
        o, _ = _gn_launch(gpu, prec, xd, wd, bd, B, T, Cc, halo, eps)
        assert _same_bits(xd, x), "the kernel changed its input"
        want, f32 = _gn_stmt(x, w, b, eps, torch.float64), _gn_stmt(x, w, b, eps, torch.float32)
        _cmp(f"groupnorm_silu {prec} T={T} C={Cc} B={B} halo={halo} {kind} eps={eps:g}", o[:B, halo:halo + T], want, f32, dt)
        if kind == "visible":
            seen[eps] = (want, f32)
        if kind != "ordinary":
            continue
        again, _ = _gn_launch(gpu, prec, xd, wd, bd, B, T, Cc, halo, eps, part=_nan((B * 64 * 2,), torch.float64, gpu))
        assert _same_bits(again[:B, halo:halo + T], o[:B, halo:halo + T]), "a launch into NaN partials differs: a partial is read unwritten"
        for i in range(B if B > 1 else 0):
            alone, _ = _gn_launch(gpu, prec, _dev(x[i:i + 1], gpu), wd, bd, 1, T, Cc, halo, eps)
            assert _same_bits(alone[0, halo:halo + T], o[i, halo:halo + T]), f"item {i} alone differs from item {i} of the batch"
    _eps_visible(f"groupnorm_silu T={T} C={Cc} B={B}", [seen[e][0] for e in EPS_PAIR], [seen[e][1] for e in EPS_PAIR], dt)


def _mgn_masks(S):
    """item 0: all valid | 1: a prefix | 2: holes (first and last frame valid, every third inside) | 3: the last frame alone | 4: none.
    Valid bytes are 1 in the even items and 255 in the odd ones."""
    m = torch.zeros(5, S, dtype=torch.uint8)
    m[0] = 1
    m[1, :max(1, S // 2)] = 255
    m[2, ::3] = 1
    m[2, 0] = m[2, S - 1] = 1
    m[3, S - 1] = 255
    return m


MGN_CASES = [(S, Cc, halo) for S, Cc in ((1, 4), (63, 256), (64, 256), (65, 256), (129, 1028), (129, 4096)) for halo in (0, 1)]


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("S,Cc,halo", MGN_CASES)
def test_masked_groupnorm_silu(gpu, prec, S, Cc, halo):
    """mgn_partial: 64 chunks of ceil(S / 64) frames - S = 1: chunks 1 .. 63 empty; 63: one frame per chunk and one empty; 64: every
    chunk full; 65: chunks of 2, the 33rd partial, 31 empty; 129: chunks of 3; C = 1028: 257 float4 per frame, the 256 threads take a
    second pass; (129, 4096) is above mgn_apply's cap of 512 workgroups (grid-stride loop).  Five items per launch (_mgn_masks); every
    masked frame of x is NaN: it may enter neither the statistics nor the output, whose masked rows are bit-zero - the item without a
    valid frame is bit-zero as a whole.  Item b alone is item b of the batch bit for bit."""
    dt = _act(prec)
    B = 5
    w, b = _wb(Cc, 700 + Cc)
    wd, bd = _dev(w, gpu), _dev(b, gpu)
    mask = _mgn_masks(S)
    md = _dev(mask, gpu)
    seen = {}
    for kind, eps in RUNS_CENTRED:
        x = _gn_items(kind, B, S, Cc, 710 + S + Cc)
        x[~mask.bool()] = NAN
        xd = _dev(x, gpu)
        o, _ = _gn_launch(gpu, prec, xd, wd, bd, B, S, Cc, halo, eps, mask=md)
        assert _same_bits(xd, x), "the kernel changed its input"
        own = o[:B, halo:halo + S]
        assert _bit_zero(own[~mask.bool()]), "a masked frame of the output is not bit-zero"
        assert _bit_zero(own[4]), "the item without a valid frame is not bit-zero"
        want, f32 = _gn_stmt(x, w, b, eps, torch.float64, mask), _gn_stmt(x, w, b, eps, torch.float32, mask)
        _cmp(f"masked_groupnorm_silu {prec} S={S} C={Cc} halo={halo} {kind} eps={eps:g}", own, want, f32, dt)
        if kind == "visible":
            seen[eps] = (want, f32)
        if kind != "ordinary":
            continue
        for i in range(B):
            alone, _ = _gn_launch(gpu, prec, _dev(x[i:i + 1], gpu), wd, bd, 1, S, Cc, halo, eps, mask=_dev(mask[i:i + 1], gpu))
            assert _same_bits(alone[0, halo:halo + S], own[i]), f"item {i} alone differs from item {i} of the batch"
    _eps_visible(f"masked_groupnorm_silu S={S} C={Cc}", [seen[e][0] for e in EPS_PAIR], [seen[e][1] for e in EPS_PAIR], dt)


# ---------------------------------------------------------------------------------------------------------------------
# the hooks' refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_norm_hooks_refuse_what_the_kernels_do_not_cover(gpu):
    """Every refusal of the five hooks by its message (SAMAUDIO_ERR_ARG): null required pointers, counts <= 0, halo < 0, dim % 4,
    x_ld % 4, x_ld < dim, tvec_ld / shift_off / scale_off % 4, shift_tab / scale_tab / tvec given in part, both outputs of
    layernorm_rows null, base pointers off their alignment.  A refused call launches nothing: the outputs keep their NaN."""
    lib = _lib("bf16")
    D = 8
    f = _dev(_mk((4, 4 * D), 800), gpu)          # any fp32 operand: 16 floats and more behind every pointer used below
    out = _nan((4, 4 * D), torch.float32, gpu)
    part = _nan((3 * 64,), torch.float64, gpu)
    m = _dev(torch.ones(8, dtype=torch.uint8), gpu)
    p, o, q, mk, z, st = hip.ptr(f), hip.ptr(out), hip.ptr(part), hip.ptr(m), None, util.stream()
    off = lambda t, n: _at(t, n)                  # a pointer n bytes behind the base
    F32, B16 = hip.F32, hip.BF16

    def refused(rc, text):
        msg = lib.samaudio_last_error().decode()
        assert rc == hip.ERR_ARG and text in msg, (rc, text, msg)

    rms = lambda x=p, w=p, st_=p, ct=p, tv=p, ld=2 * D, so=0, co=D, out_=o, prec=F32, rows=2, dim=D, rpb=1: \
        lib.samaudio_op_rmsnorm_mod(x, w, st_, ct, tv, ld, so, co, out_, prec, rows, dim, rpb, 1e-5, st)
    for kw in (dict(x=z), dict(w=z), dict(out_=z)):
        refused(rms(**kw), "rmsnorm_mod: null x / w / out")
    refused(rms(rows=0), "rmsnorm_mod: rows <= 0")
    refused(rms(dim=0), "rmsnorm_mod: dim % 4")
    refused(rms(dim=6), "rmsnorm_mod: dim % 4")
    refused(rms(rpb=0), "rmsnorm_mod: rows_per_batch <= 0")
    for kw in (dict(st_=z), dict(ct=z), dict(tv=z), dict(st_=z, ct=z), dict(ct=z, tv=z), dict(st_=z, tv=z)):
        refused(rms(**kw), "rmsnorm_mod: shift_tab, scale_tab and tvec are given together or not at all")
    refused(rms(ld=2 * D + 2), "rmsnorm_mod: tvec_ld % 4")
    refused(rms(so=2), "rmsnorm_mod: shift_off % 4")
    refused(rms(co=D + 1), "rmsnorm_mod: scale_off % 4")
    for kw in (dict(x=off(f, 4)), dict(w=off(f, 8)), dict(st_=off(f, 4)), dict(ct=off(f, 4)), dict(tv=off(f, 12)), dict(out_=off(out, 8)),
               dict(out_=off(out, 4), prec=B16)):
        refused(rms(**kw), "rmsnorm_mod: x, w, shift_tab, scale_tab and tvec must be aligned to 16 bytes")

    for name, text, fn in (("groupnorm", "groupnorm: ", lib.samaudio_op_groupnorm_silu),
                           ("masked_groupnorm", "masked_groupnorm: ", lib.samaudio_op_masked_groupnorm_silu)):
        masked = name == "masked_groupnorm"

        def gn(x=p, w=p, b=p, mask=mk, part_=q, out_=o, prec=F32, batch=1, frames=2, ch=D, halo=0):
            head = (x, w, b, mask) if masked else (x, w, b)
            return fn(*head, part_, out_, prec, batch, frames, ch, halo, 1e-5, st)
        nulls = [dict(x=z), dict(w=z), dict(b=z), dict(part_=z), dict(out_=z)] + ([dict(mask=z)] if masked else [])
        for kw in nulls:
            refused(gn(**kw), text + "null x / w / b /")
        refused(gn(batch=0), text + "batch <= 0")
        refused(gn(frames=0), text + "frames <= 0")
        refused(gn(ch=0), text + "channels % 4")
        refused(gn(ch=6), text + "channels % 4")
        refused(gn(halo=-1), text + "halo < 0")
        for kw in (dict(x=off(f, 4)), dict(w=off(f, 4)), dict(b=off(f, 8)), dict(part_=off(part, 4)), dict(out_=off(out, 8)),
                   dict(out_=off(out, 4), prec=B16)):
            refused(gn(**kw), text + "x, w and b must be aligned to 16 bytes")

    acc = lambda x=p, w=p, b=p, g=p, a=o, rows=2, dim=D: lib.samaudio_op_layernorm_accum(x, w, b, g, a, rows, dim, 1e-5, st)
    for kw in (dict(x=z), dict(w=z), dict(b=z), dict(g=z), dict(a=z)):
        refused(acc(**kw), "layernorm_accum: null x / w / b / gate / acc")
    refused(acc(rows=0), "layernorm_accum: rows <= 0")
    refused(acc(dim=0), "layernorm_accum: dim % 4")
    refused(acc(dim=6), "layernorm_accum: dim % 4")   # (the kernel would silently skip the last two columns)
    for kw in (dict(x=off(f, 4)), dict(w=off(f, 4)), dict(b=off(f, 4)), dict(a=off(out, 4))):
        refused(acc(**kw), "layernorm_accum: x, w, b and acc must be aligned to 16 bytes")

    rows_ = lambda x=p, ld=D, w=p, b=p, o32=o, oa=z, prec=F32, rows=2, dim=D: \
        lib.samaudio_op_layernorm_rows(x, ld, w, b, o32, oa, prec, rows, dim, 1e-5, st)
    for kw in (dict(x=z), dict(w=z), dict(b=z)):
        refused(rows_(**kw), "layernorm_rows: null x / w / b")
    refused(rows_(o32=z, oa=z), "layernorm_rows: out_f32 and out_act are both null")
    refused(rows_(rows=0), "layernorm_rows: rows <= 0")
    refused(rows_(dim=0), "layernorm_rows: dim % 4")
    refused(rows_(dim=6, ld=8), "layernorm_rows: dim % 4")
    refused(rows_(ld=D + 2), "layernorm_rows: x_ld % 4")
    refused(rows_(ld=D - 4), "layernorm_rows: x_ld < dim")
    for kw in (dict(x=off(f, 4)), dict(w=off(f, 4)), dict(b=off(f, 4)), dict(o32=off(out, 4)), dict(oa=off(out, 8)),
               dict(oa=off(out, 4), prec=B16)):
        refused(rows_(**kw), "layernorm_rows: x, w, b and out_f32 must be aligned to 16 bytes")

    if not SIM:
        torch.cuda.synchronize()
    assert _all_nan(out.cpu()) and _all_nan(part.cpu()), "a refused call wrote something"
    assert _same_bits(f, _mk((4, 4 * D), 800)), "a refused call changed an input"


# ---------------------------------------------------------------------------------------------------------------------
# eps-visible cases of the norms that are pinned on O(1) data in their own files
# ---------------------------------------------------------------------------------------------------------------------
def _small(x, prec):
    """mean square about 1e-5; where the kernel reads 16-bit values, every magnitude stays inside IEEE half's normal range (>= 2^-14)"""
    if prec == "fp32":
        return x * 3.16e-3
    return torch.sign(x) * (x.abs() * 3.0e-3 + 2e-4)


def _gap(tag, a, b, bound, factor):
    gap = (a - b).abs().max().item()
    print(f"{tag}: the statements at eps 1e-5 and 1e-6 differ by {gap:.3e} = {gap / bound:.0f} x the bound {bound:.1e}")
    assert gap > factor * bound, f"{tag}: eps is not visible in this data"


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("shared_time", [False, True])
def test_rmsnorm_gs_with_eps_in_reach(gpu, prec, shared_time):
    """tests/test_layer_kernels_gpu.py test_rmsnorm_gs at D = 512 on its own data scaled to a mean square of 1e-5, at eps 1e-5 and 1e-6
    against that file's float64 statement and bounds (1e-5 fp32, 4e-2 16-bit).  The two statements differ by more than 100 x the fp32
    bound and more than 10 x the 16-bit one: a hundred times 4e-2 is beyond what a change of eps can do to an O(1) output."""
    D, M = 512, L.B_N * L.T_N
    x, w, tabs, tvec = L._norm_case(D, shared_time)
    x = x * 3.16e-3
    nt = tvec.shape[0]
    gs_d, _ = L._mod_tables(gpu, prec, D, w, tabs, tvec)
    gs_n = gs_d.view(-1)[L.USED * nt * 2 * D:]
    xd = _dev(x, gpu)
    tol = 1e-5 if prec == "fp32" else 4e-2
    wants = []
    for eps in EPS_PAIR:
        out = _nan((M + 1, D), _act(prec), gpu)
        hip.check(_lib(prec).samaudio_op_rmsnorm_gs(hip.ptr(xd), _at(gs_n), 0 if nt == 1 else 2 * D, hip.ptr(out), _code(prec), 0, M, D,
                                                    L.T_N, eps, util.stream()))
        o = out.cpu()
        assert _all_nan(o[M]), "the row behind the output was written"
        wants.append(L._norm_want(D, x, w, tabs, tvec, eps))
        L._err(f"rmsnorm_gs {prec} D={D} nt={nt} eps={eps:g}", o[:M], wants[-1], tol)
    _gap(f"rmsnorm_gs {prec} nt={nt}", wants[0], wants[1], tol, 100 if prec == "fp32" else 10)


@pytest.mark.parametrize("prec", STORAGE)
@pytest.mark.parametrize("hd", [64, 128])
def test_headnorm_layers_with_eps_in_reach(gpu, prec, hd):
    """tests/test_glue_kernels_gpu.py test_headnorm_layers at rows 3, L 3, H 2 on inputs of mean square about 1e-5, at eps 1e-5 and
    1e-6, against that file's statement under its bound (_cmp)."""
    if LAUNCHER_EMU and hd == 64:
        pytest.skip("headnorm_layers with head_dim 64: not in this build of the library (the launcher emulation has head_dim 128 only)")
    rows, Ln, H = 3, 3, 2
    dt = _act(prec)
    x = _small(_mk((rows + 1, Ln, 2, H, hd), 900 + hd), prec)
    w = _mk((Ln, hd), 901) + 1.5 * torch.arange(1, Ln + 1)[:, None]
    seen = _rnd(x[:rows, :, 0], prec)
    wants, f32s = [], []
    for eps in EPS_PAIR:
        xd, wd = _dev(x.to(dt), gpu), _dev(w, gpu)
        _ok(prec, _lib(prec).samaudio_op_headnorm_layers(hip.ptr(xd), hip.ptr(wd), _code(prec), rows, Ln, H, hd, eps, util.stream()))
        got = xd.cpu()
        assert _same_bits(got[rows], x[rows].to(dt)), "the row behind the last was changed"
        assert _same_bits(got[:rows, :, 1], x[:rows, :, 1].to(dt)), "a V half was changed"
        wants.append(G._headnorm_stmt(seen, w, torch.float64, eps))
        f32s.append(G._headnorm_stmt(seen, w, torch.float32, eps))
        _cmp(f"headnorm_layers {prec} hd={hd} eps={eps:g}", got[:rows, :, 0], wants[-1], f32s[-1], dt)
    _eps_visible(f"headnorm_layers {prec} hd={hd}", wants, f32s, dt)


@pytest.mark.parametrize("prec,hd", [(p, hd) for p in STORAGE for hd in (64, 128)] + [("f32x:" + p, 128) for p in L.X3])
def test_qkv_prep_with_eps_in_reach(gpu, prec, hd):
    """tests/test_layer_kernels_gpu.py test_qkv_prep at T = 12 (the general kernel at both head widths and types, the 16-byte fast path
    of the 16-bit types at 128, the fp32 fast path "f32x") on inputs of mean square about 1e-5, at eps 1e-5 and 1e-6 against that
    file's statement and bounds (2e-5 fp32, 4e-2 16-bit; 100 x resp. 10 x apart, as for rmsnorm_gs).  V^T is a copy: its bits."""
    f32x = prec.startswith("f32x:")
    lib_prec = prec[5:] if f32x else prec
    prec = "fp32" if f32x else prec
    if hd == 64:
        L._no_launcher_emu("64-wide heads")
    B, H, T = 2, 3, 12
    D, Tp = H * hd, 64
    qkv = _small(_mk((B, T, 3 * D), 950 + hd), prec)
    qw, kw = _mk((hd,), 11, 0.1) + 1, _mk((hd,), 12, 0.1) + 1
    cos, sin = L.O.rope_tables(hd, T, 20000.0)
    dt = _act(prec)
    xd, qwd, kwd, cd, sd = _dev(qkv, gpu, dt), _dev(qw, gpu), _dev(kw, gpu), _dev(cos, gpu), _dev(sin, gpu)
    tol = 2e-5 if prec == "fp32" else 4e-2
    tag = f"qkv_prep {'f32x ' + lib_prec if f32x else prec} hd={hd}"
    wants = []
    for eps in EPS_PAIR:
        q, k, vt = _nan((B + 1, H, Tp, hd), dt, gpu), _nan((B + 1, H, Tp, hd), dt, gpu), _nan((B + 1, H, hd, Tp), dt, gpu)
        hip.check(_lib(lib_prec).samaudio_op_qkv_prep_hd(hip.ptr(xd), hip.ptr(qwd), hip.ptr(kwd), hip.ptr(cd), hip.ptr(sd), hip.ptr(q),
                                                         hip.ptr(k), hip.ptr(vt), _code(prec), 1 if f32x else 0, B, T, Tp, H, hd, eps,
                                                         util.stream()))
        q, k, vt = q.cpu(), k.cpu(), vt.cpu()
        qr, kr, vr = L._qkv_want(_rnd(qkv, prec), B, T, H, hd, qw, kw, cos, sin, eps)
        L._err(f"{tag} eps={eps:g} q", q[:B, :, :T], qr, tol)
        L._err(f"{tag} eps={eps:g} k", k[:B, :, :T], kr, tol)
        assert _same_bits(vt[:B, :, :, :T].contiguous(), vr.to(dt).contiguous()), "V^T is not a copy of v"
        assert _bit_zero(q[:B, :, T:]) and _bit_zero(k[:B, :, T:]) and _bit_zero(vt[:B, :, :, T:]), "padding must be zero"
        assert _all_nan(q[B]) and _all_nan(k[B]) and _all_nan(vt[B]), "the slab behind the last batch item was written"
        wants.append((qr, kr))
    for i, name in enumerate("qk"):
        _gap(f"{tag} {name}", wants[0][i], wants[1][i], tol, 100 if prec == "fp32" else 10)
