"""Every kernel that writes e4m3 bytes, or measures the scale for them, outside the GEMM epilogue, one launch each through the operator entry
points (vima_op_fp8_quant, vima_op_fp8_amax, vima_op_norm_fp8, vima_op_vit_attention_fp8, _cls_fp8 -- include/vima_hip.h), against
tests/fp8_producer_reference.py (the reference conversion, cases and inputs; tests/test_fp8_producer_reference.py pins them on the CPU).

A  quant_fp8_kernel bit for bit: all 65 536 bf16 bit patterns at five scales, four geometries with hostile pad columns, refusals;
B  amax_kernel exact: max(slot, max |x|) by bit pattern, every slot / position combination, past the grid cap, inf and NaN;
C  the out8 path of LayerNorm bit for bit against the fp32 output of the SAME launch, with and without the other outputs;
D  the out8 path of the four ViT attention kernels inside the code interval of the fp64 reference, and bit-identical across kernels;
E  what a NaN activation becomes after calibration.
Codes are compared with 0x00 and 0x80 taken as equal (the same number to the consuming MFMA); the share of such elements is printed. Every output
buffer is pre-filled with the canary byte 0x7F (e4m3 NaN, which no producer can emit) and followed by a guard tail."""
import ctypes

import pytest
import torch

from tests import fp8_producer_reference as R
from tests import seq_norm_reference as N
from tests import vit_front_reference as V
from tests.gpu_common import bare_policy, ptr
from vima_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
_stats = {}                         # family -> [cases, elements, signed-zero elements, lo != hi elements, of those: took hi]


def _note(family, n, zeros=0, straddle=0, took_hi=0):
    s = _stats.setdefault(family, [0, 0, 0, 0, 0])
    for i, v in enumerate((1, n, zeros, straddle, took_hi)):
        s[i] += int(v)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _call(fn, pol, *args):
    rc = fn(pol._handle, *args, pol._stream())
    torch.cuda.synchronize()
    return rc, (pol._lib.vima_last_error().decode("utf-8", "replace") if rc else "")


def _ok(fn, pol, *args):
    rc, msg = _call(fn, pol, *args)
    assert rc == 0, msg


def _guarded(rows, ld):
    """A canary-filled device byte buffer of rows * ld bytes and a guard tail -> (buffer, [rows, ld] view)."""
    buf = torch.full((rows * ld + R.TAIL,), R.CANARY_U8, dtype=torch.uint8, device=DEV)
    return buf, buf[: rows * ld].view(rows, ld)


def _tail_intact(buf, n):
    assert (buf[n:] == R.CANARY_U8).all(), "a kernel wrote past the end of its output"


def _untouched(buf):
    assert (buf == R.CANARY_U8).all(), "a refused or empty call wrote to its output"


def _same_codes(family, cid, got, want):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (cid, got.shape, want.shape)
    ok = R.same_codes(got, want)
    zeros = int(((got != want) & ok).sum())
    _note(family, got.numel(), zeros)
    print(f"[fp8-producers] {family} {cid}: signed-zero share {zeros / max(got.numel(), 1):.5f}")
    if not ok.all():
        at = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(f"{cid} [{family}]: {int((~ok).sum())} of {ok.numel()} codes differ, first at {at}: got 0x{int(got[at]):02X}, want 0x{int(want[at]):02X}")


# ================================================================================================================== A  quant_fp8
def run_quant(x, rows, cols, ldin, ldo, inv, prec="bf16", out_rows=None):
    """One vima_op_fp8_quant call on x fp32 [*, ldin] -> (out8 [rows, ldo] on the CPU, rc, msg); the guard tail is checked here."""
    pol = bare_policy(prec)
    n_rows = rows if out_rows is None else out_rows
    buf, out = _guarded(n_rows, ldo)
    xd = dev(x)
    rc, msg = _call(pol._lib.vima_op_fp8_quant, pol, ptr(xd), ldin, rows, cols, inv, ptr(buf), ldo)
    _tail_intact(buf, n_rows * ldo)
    return out.cpu(), rc, msg


@pytest.mark.parametrize("inv", R.QUANT_INVS, ids=lambda v: f"inv{v:.6g}")
def test_a_quant_every_bf16_bit_pattern(inv):
    """Normals, the e4m3 subnormals (steps of 2^-9), ties, saturation at +-448 (0x7E / 0xFE), +-inf -> +-448, -0. Would fail: truncation,
    saturation one code early (240), the odd and even element of a pair swapped, a vector's words out of order."""
    x = R.all_bf16_patterns()
    out, rc, msg = run_quant(x, 8, 8192, 8192, 8192, inv)
    assert rc == 0, msg
    want = R.e4m3_codes(x, inv)
    _same_codes("A quant exhaustive", f"inv {inv:.6g}", out, want)
    inf = torch.isinf(x)
    assert inf.sum() == 2 and set(out[inf].tolist()) == {0x7E, 0xFE}


@pytest.mark.parametrize("g", R.QUANT_GEOMS, ids=lambda g: "r{}-c{}-ldin{}-ldo{}".format(*g))
def test_a_quant_geometry(g):
    """Pad columns of the input hold +-3e38 and those of the output the canary: the pad is neither read into the result nor written."""
    rows, cols, ldin, ldo = g
    x = R.quant_geom_inputs(rows, cols, ldin)
    for inv in (1.0, R.QUANT_INVS[1]):
        out, rc, msg = run_quant(x, rows, cols, ldin, ldo, inv)
        assert rc == 0, msg
        _same_codes("A quant geometry", "r{}-c{}-ldin{}-ldo{} inv {:.3g}".format(*g, inv), out[:, :cols], R.e4m3_codes(x[:, :cols].contiguous(), inv))
        assert (out[:, cols:] == R.CANARY_U8).all(), "a pad column of the output was written"


def test_a_quant_refusals_and_empty():
    x = torch.ones(64, 16)
    for rows, cols, ldin, ldo in R.QUANT_REFUSED:
        out, rc, msg = run_quant(x, rows, cols, ldin, ldo, 1.0)
        assert rc != 0 and "quant_fp8" in msg, (rows, cols, ldin, ldo, msg)
        _untouched(out)
    out, rc, msg = run_quant(x, 0, 8, 16, 16, 1.0, out_rows=4)
    assert rc == 0, msg
    _untouched(out)
    out, rc, msg = run_quant(x, 4, 8, 16, 16, 1.0, prec="fp32")
    assert rc != 0 and "bf16" in msg
    _untouched(out)


# ================================================================================================================== B  amax
def run_amax(x, rows, cols, ldin, slot0):
    pol = bare_policy("bf16")
    slot = torch.full((1 + 16,), -77.0, device=DEV)              # the slot and a guard
    slot[0] = slot0
    xd = dev(x)
    _ok(pol._lib.vima_op_fp8_amax, pol, ptr(xd), ldin, rows, cols, ptr(slot))
    assert (slot[1:] == -77.0).all()
    return slot[:1].cpu()


def _slot_is(cid, got, want):
    _note("B amax", 1)
    want = torch.as_tensor(want, dtype=torch.float32).reshape(1)
    if torch.isnan(want).all():
        assert torch.isnan(got).all(), f"{cid}: slot {got.item()} where a NaN in the data must reach it"
    else:
        assert got.view(torch.int32).item() == want.view(torch.int32).item(), f"{cid}: slot {got.item()!r}, want {want.item()!r}"


@pytest.mark.parametrize("neg", [False, True], ids=["pos", "neg"])
@pytest.mark.parametrize("place", R.AMAX_PLACES)
@pytest.mark.parametrize("g", [(1, 8, 8), (7, 24, 40), (33, 768, 768), (257, 3072, 3080)], ids=lambda g: "r{}-c{}-ld{}".format(*g))
def test_b_amax_exact(g, place, neg):
    """slot = max(slot0, max |x[:, :cols]|) by bit pattern: slot0 zero, above and below the data's maximum; the maximum first, last, and alone in
    the odd half of a vector (both `<< 16` and `& 0xffff0000`); 3e38 in the pad columns must not count."""
    rows, cols, ldin = g
    x = R.amax_inputs(rows, cols, ldin, place, neg)
    for slot0 in (0.0, 9.0, 0.5):
        _slot_is(f"{g} {place} slot0 {slot0}", run_amax(x, rows, cols, ldin, slot0), R.amax_ref(slot0, x, cols))


def test_b_amax_all_zero_leaves_the_slot():
    x = R.padded(torch.zeros(7, 24), 40)
    x[3, 5] = -0.0
    for slot0 in (0.0, 2.5):
        _slot_is(f"zeros slot0 {slot0}", run_amax(x, 7, 24, 40, slot0), slot0)


def test_b_amax_past_the_grid_cap():
    """rows x cols / 8 vectors > 2048 x 256 x 8: the grid-stride loop runs a ninth, partial round, and the maximum sits in the very last vector."""
    rows, cols = R.AMAX_BIG
    x = R.amax_inputs(rows, cols, cols, "last")
    _slot_is("big last", run_amax(x, rows, cols, cols, 0.0), R.amax_ref(0.0, x, cols))
    assert R.amax_ref(0.0, x, cols) == R.AMAX_PEAK and R.amax_ref(0.0, x[:-1], cols) <= 1.0


def test_b_amax_carries_inf_and_nan():
    """The calibration contract (iii): a non-finite activation must reach the slot so that the freeze refuses it. inf orders above every finite
    magnitude; a NaN would be dropped by fmaxf -- the kernel takes the maximum over the magnitude bit patterns, where NaN orders above inf."""
    for place, bad in (("first", float("inf")), ("last", float("-inf")), ("odd_half", NAN), ("first", -NAN)):
        x = R.amax_inputs(33, 768, 776, place)
        x[17, 301] = bad
        _slot_is(f"{bad} {place}", run_amax(x, 33, 768, 776, 0.5), abs(bad))
    x = R.amax_inputs(33, 768, 768, "last")
    x[0, 0], x[32, 767] = float("inf"), NAN
    _slot_is("inf and NaN", run_amax(x, 33, 768, 768, 0.0), NAN)


# ================================================================================================================== C  LayerNorm out8
def run_norm8(c, inv8, want32=True, wantT=True):
    """One vima_op_norm_fp8 call -> (out8 [rows, E], out32 or None, outT or None) on the CPU."""
    kind, prec, E, rows, pad, rms, regime = c
    full, g, b, _, _ = N.norm_inputs(E, rows, pad, regime)
    pol = bare_policy(prec)
    d = _lib.VimaNormDesc()
    keep = {"x": dev(full), "gamma": dev(g), "beta": None if rms else dev(b)}
    outs = {"out32": torch.full((rows, E), NAN, device=DEV) if want32 else None, "outT": torch.full((rows, E), NAN, device=DEV) if wantT else None}
    for k, t in list(keep.items()) + list(outs.items()):
        setattr(d, k, t.data_ptr() if t is not None else None)
    d.ldin, d.kind, d.rms, d.rows, d.E, d.eps = E + pad, _lib.NORM_KIND[kind], rms, rows, E, (N.RMS_EPS if rms else N.LN_EPS)
    buf, out8 = _guarded(rows, E)
    _ok(pol._lib.vima_op_norm_fp8, pol, ctypes.byref(d), ptr(buf), inv8)
    _tail_intact(buf, rows * E)
    return out8.cpu(), (outs["out32"].cpu() if want32 else None), (outs["outT"].cpu() if wantT else None)


@pytest.mark.parametrize("c", R.LN8_CASES, ids=R.ln8_case_id)
def test_c_layernorm_out8_is_the_code_of_the_fp32_output(c):
    """The kernel converts the fp32 register value it also stores to out32: out8 == e4m3_codes(out32, inv8) exactly, no gate (whether out32 itself
    is right is tests/test_seq_norm_gpu.py's business). Would fail: the bf16-rounded result converted instead, a row or column misplaced in
    out8, the rows of a rows2 pair swapped in out8 only, an odd last row or a grid-stride round left out. The same call without out32 and
    without outT must give the same bytes."""
    kind, prec, E, rows, pad, rms, regime = c
    fam = f"C out8 {N.norm_kernel_of(kind, prec, E, E + pad)}"
    first = None
    for name, inv8 in R.ln8_inv8(c):
        out8, out32, outT = run_norm8(c, inv8)
        assert torch.isfinite(out32).all()
        assert torch.equal(outT, N.bf(out32)), "the operand-type output next to out8 is still the bf16 rounding of out32"
        want = R.e4m3_codes(out32, inv8)
        _same_codes(fam, f"{R.ln8_case_id(c)} {name}", out8, want)
        if name == "sat":
            assert ((out8 & 0x7F) == 0x7E).any(), "inv8 x 16 saturates a visible share"
        if first is None:
            first = (inv8, out8)
    inv8, out8 = first
    assert torch.equal(run_norm8(c, inv8, want32=False)[0], out8), "out8 changes when out32 is not asked for"
    assert torch.equal(run_norm8(c, inv8, wantT=False)[0], out8), "out8 changes when outT is not asked for"
    assert torch.equal(run_norm8(c, inv8, want32=False, wantT=False)[0], out8), "out8 alone"


def test_c_norm_fp8_refusals():
    """Another kind, an fp32 handle, and a row stride the launcher refuses (258: no multiple of 4): an error, and neither out8 nor out32 written."""
    keep = [torch.ones(2 * 264, device=DEV), torch.ones(256, device=DEV), torch.zeros(256, device=DEV)]
    for prec, kind, ldin, word in (("bf16", "ln", 256, "kind"), ("fp32", "ln_T", 256, "bf16"), ("bf16", "ln_T", 258, "layernorm_T")):
        pol = bare_policy(prec)
        d = _lib.VimaNormDesc()
        d.x, d.gamma, d.beta = (t.data_ptr() for t in keep)
        out32 = torch.full((2, 256), -77.0, device=DEV)
        d.out32 = out32.data_ptr()
        d.ldin, d.kind, d.rms, d.rows, d.E, d.eps = ldin, _lib.NORM_KIND[kind], 0, 2, 256, N.LN_EPS
        buf, out8 = _guarded(2, 256)
        rc, msg = _call(pol._lib.vima_op_norm_fp8, pol, ctypes.byref(d), ptr(buf), 1.0)
        assert rc != 0 and word in msg, msg
        _untouched(buf)
        assert (out32 == -77.0).all()


# ================================================================================================================== D  ViT attention out8
def run_attn8(c, inv8, impl=None, qkv=None):
    """One vima_op_vit_attention_fp8 / _cls_fp8 call of a case -> out8 [M * Sq, W] on the CPU."""
    kern, prec, W, S, M, regime = c
    pol = bare_policy(prec)
    qkv = R.attn8_inputs(c) if qkv is None else qkv
    rows = M if kern == "vit_attn_cls" else M * S
    buf, out8 = _guarded(rows, W)
    if kern == "vit_attn_cls":
        q, kv = (dev(t) for t in V.cls_operands(qkv, M, S, W))
        _ok(pol._lib.vima_op_vit_attention_cls_fp8, pol, ptr(q), ptr(kv), M, S, W, W // 32, inv8, ptr(buf))
    else:
        qd = dev(qkv)
        _ok(pol._lib.vima_op_vit_attention_fp8, pol, ptr(qd), M, S, W, W // 32, V.ATTN_IMPL[kern] if impl is None else impl, inv8, ptr(buf))
    _tail_intact(buf, rows * W)
    return out8.cpu()


@pytest.mark.parametrize("c", R.ATTN8_CASES, ids=R.attn8_case_id)
def test_d_attention_out8_inside_the_code_interval(c):
    """The operand-type output is not written on this path, so the fp32 value the kernel converts is not observable: y = the fp64 attention of the
    bf16-rounded operands x inv8, delta = the fp32 handle's gate of the case x inv8, and the code must lie in [e4m3(y - delta), e4m3(y + delta)]
    (one code on >= 99 % of the elements: the CPU test's condition). Would fail: everything the fp64 test of the operand-type output catches, a
    wrong inv8, a head's 32 bytes misplaced, the four bytes of a word out of order, truncation, saturation at 240."""
    fam = f"D {c[0]} {c[5]}"
    for name, inv8, lo, hi in R.attn8_intervals(c):
        out8 = run_attn8(c, inv8)
        ok = R.inside(out8, lo, hi)
        wide = ~R.same_codes(lo, hi)
        _note(fam + " " + name, out8.numel(), ((out8 != lo) & R.same_codes(out8, lo) & ~wide).sum(), wide.sum(), (wide & R.same_codes(out8, hi)).sum())   # signed zeros: where lo == hi
        print(f"[fp8-producers] {fam} {R.attn8_case_id(c)} {name}: lo != hi share {wide.double().mean().item():.5f}")
        if not ok.all():
            at = tuple((~ok).nonzero()[0].tolist())
            raise AssertionError(f"{R.attn8_case_id(c)} {name}: {int((~ok).sum())} of {ok.numel()} codes outside their interval, first at {at}: "
                                 f"got 0x{int(out8[at]):02X}, interval 0x{int(lo[at]):02X} .. 0x{int(hi[at]):02X}")
        if name == "sat":
            assert ((out8 & 0x7F) == 0x7E).any()


@pytest.mark.parametrize("c", [c for c in R.ATTN8_CASES if c[0] != "vit_attn_cls" and c[5] == "normal"], ids=R.attn8_case_id)
def test_d_attention_out8_is_identical_across_kernels(c):
    """impl 0 / 1 / 2 wherever more than one applies (every S <= 16; at the hot shape impl 0 is the LDS-staged kernel), both regimes."""
    for regime in V.REGIMES:
        cc = c[:5] + (regime,)
        inv8 = R.attn8_intervals(cc)[0][1]
        a = run_attn8(cc, inv8, impl=0)
        assert not (a == R.CANARY_U8).any()
        for impl in (1, 2):
            assert torch.equal(run_attn8(cc, inv8, impl=impl), a), f"{R.attn8_case_id(cc)}: impl {impl} differs from impl 0"
        _note("D across impl", a.numel())


@pytest.mark.parametrize("c", [c for c in R.ATTN8_CASES if c[0] == "vit_attn_cls"], ids=R.attn8_case_id)
def test_d_cls_out8_is_row_zero_of_the_full_form(c):
    kern, prec, W, S, M, regime = c
    for name, inv8, _, _ in R.attn8_intervals(c):
        qkv = R.attn8_inputs(c)
        full = run_attn8(("vit_attn8", prec, W, S, M, regime), inv8, impl=0, qkv=qkv).view(M, S, W)
        assert torch.equal(run_attn8(c, inv8), full[:, 0]), f"{R.attn8_case_id(c)} {name}"
    _note("D cls = row 0", M * W)


def test_d_attention_fp8_refusals():
    x = torch.randn(17 * 3 * 768, device=DEV)
    for prec, fn, args, word in (
            ("bf16", "vima_op_vit_attention_fp8", (1, 17, 768, 24, 0), "vit_attn"),          # S = 17: more than the 16 score registers
            ("bf16", "vima_op_vit_attention_fp8", (1, 5, 768, 12, 0), "head dim"),
            ("bf16", "vima_op_vit_attention_fp8", (1, 5, 768, 24, 3), "impl"),
            ("fp32", "vima_op_vit_attention_fp8", (1, 5, 768, 24, 0), "bf16"),
            ("bf16", "vima_op_vit_attention_cls_fp8", (1, 9, 768, 24), "vit_attn_cls"),       # S = 9: more than the cls kernel's 8
            ("fp32", "vima_op_vit_attention_cls_fp8", (1, 5, 768, 24), "bf16")):
        pol = bare_policy(prec)
        buf, _ = _guarded(17, 768)
        ins = (ptr(x), ptr(x)) if "cls" in fn else (ptr(x),)
        rc, msg = _call(getattr(pol._lib, fn), pol, *ins, *args, 1.0, ptr(buf))
        assert rc != 0 and word in msg, (fn, args, msg)
        _untouched(buf)


# ================================================================================================================== E  NaN after calibration
NAN_BYTE = 0xFE


def test_e_nan_activation_becomes_minus_448():
    """A NaN in a non-calibrating pass is NOT detected: fmed3(NaN, -448, 448) returns the minimum of the other two operands and the conversion
    makes it 0xFE, -448 (include/vima_hip.h, calibration contract (iii), states the byte). The neighbours of the NaN are converted as usual."""
    x = torch.arange(16, dtype=torch.float32).reshape(1, 16) - 8
    x[0, 3], x[0, 10] = NAN, -NAN
    out, rc, msg = run_quant(x, 1, 16, 16, 16, 1.0)
    assert rc == 0, msg
    print(f"[fp8-producers] E: a NaN activation becomes 0x{int(out[0, 3]):02X} (+NaN) / 0x{int(out[0, 10]):02X} (-NaN)")
    assert int(out[0, 3]) == NAN_BYTE and int(out[0, 10]) == NAN_BYTE
    fin = torch.isfinite(x)
    assert torch.equal(out[fin], R.e4m3_codes(x, 1.0)[fin])


def test_zz_print_the_record():
    """Last in the file: the figures profiles/fp8_producer_checks.txt records."""
    for fam in sorted(_stats):
        cases, n, zeros, wide, hi = _stats[fam]
        line = f"[fp8-producers] {fam}: {cases} checks, {n} elements, signed-zero share {zeros / max(n, 1):.6f}"
        if fam.startswith("D vit"):
            line += f", lo != hi share {wide / max(n, 1):.6f} (cap {R.LOHI_CAP}), of those at hi {hi} / at lo {wide - hi}, outside 0"
        print(line)
