"""CPU pins of tests/fp8_producer_reference.py: the reference conversion against an independent fp64 nearest-even search on every finite bf16
bit pattern, the named edge codes, the mutations the GPU tests must catch (so the references can tell them apart), the interval form and its
1 % condition on every attention case, and the case tables' reach."""
import pytest
import torch

from tests import fp8_producer_reference as R
from tests import seq_norm_reference as N
from tests import vit_front_reference as V

PIN_INVS = (1.0, R.f32(1 / 3), R.f32(0.0123), 37.0) + R.QUANT_INVS[2:]


def test_decode_table_is_the_format():
    t = R.decode_table()
    assert t[0x00] == 0 and t[0x80] == 0 and torch.signbit(t[0x80])
    assert t[0x01] == 2.0 ** -9 and t[0x07] == 7 * 2.0 ** -9 and t[0x08] == 2.0 ** -6     # subnormal step, first normal
    assert t[0x38] == 1.0 and t[0x7E] == 448.0 and t[0xFE] == -448.0
    assert torch.isnan(t[0x7F]) and torch.isnan(t[0xFF]) and torch.isfinite(t).sum() == 254
    assert (t[1:0x7F] > t[0:0x7E]).all(), "the non-negative codes ascend with their values"
    # torch's own decode of the same bytes
    assert torch.equal(torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().nan_to_num(nan=-1.0), t.nan_to_num(nan=-1.0))


@pytest.mark.parametrize("inv", PIN_INVS, ids=lambda v: f"inv{v:.6g}")
def test_e4m3_codes_is_round_to_nearest_even_on_every_finite_bf16(inv):
    """The product is stated independently too: the fp64 product of two fp32 numbers is exact, its rounding to fp32 is the fp32 product."""
    x = R.finite_bf16_patterns()
    got = R.e4m3_codes(x, inv)
    p = (x.double() * torch.tensor(inv, dtype=torch.float32).double()).float()
    want = R.nearest_codes64(p.double())
    assert R.same_codes(got, want).all(), f"{int((~R.same_codes(got, want)).sum())} codes differ from the fp64 nearest-even search"
    nz = (want & 0x7F) != 0
    assert torch.equal(got[nz], want[nz])
    print(f"[fp8-producers] e4m3_codes vs fp64 search, inv {inv:.6g}: signed-zero share {R.signed_zero_share(got, want):.5f}")
    assert not ((got & 0x7F) == 0x7F).any(), "no NaN code from clamped finite input"


def test_e4m3_codes_named_edges():
    one = lambda v, inv=1.0: int(R.e4m3_codes(torch.tensor([v], dtype=torch.float32), inv)[0])
    assert one(2.0 ** -10) == 0x00                           # tie between 0 and 2^-9: to even
    assert one(3 * 2.0 ** -10) == 0x02                       # tie between 2^-9 and 2^-8: to even
    assert one(2.0 ** -10 * 1.0078125) == 0x01
    assert one(-0.0) == 0x80
    assert one(-2.0 ** -11) in (0x80, 0x00)                  # the sign of a result that rounds to zero is the one freedom
    assert one(448.0) == 0x7E and one(1e30) == 0x7E and one(float("inf")) == 0x7E
    assert one(-449.0) == 0xFE and one(float("-inf")) == 0xFE
    assert one(432.0) == 0x7E and one(400.0) == 0x7C         # ties 416 | 448 and 384 | 416: to the even code
    assert one(1.0) == 0x38 and one(3.0, R.f32(1 / 3)) == 0x38


def test_references_tell_the_mutations_apart():
    """Each mutation of the issue's list changes codes of the exhaustive input (A) beyond the signed-zero excuse."""
    x = R.all_bf16_patterns()
    for inv in R.QUANT_INVS[:3]:
        ref = R.e4m3_codes(x, inv)
        p = (x * torch.tensor(inv, dtype=torch.float32)).double()
        assert not R.same_codes(R.nearest_codes64(p, truncate=True), ref).all(), "truncation"
        assert not R.same_codes(R.nearest_codes64(p, limit=240.0), ref).all(), "saturation at 240"
        swapped = ref.view(8, 4096, 2).flip(-1).reshape(8, 8192)
        assert not R.same_codes(swapped, ref).all(), "odd and even element of a pair swapped"
    # ldin / ldo ignored: a geometry case whose pad is read lands the +-3e38 of the pad in the result
    rows, cols, ldin, ldo = R.QUANT_GEOMS[1]
    full = R.quant_geom_inputs(rows, cols, ldin)
    dense = full.reshape(-1)[: rows * cols].view(rows, cols)
    assert not R.same_codes(R.e4m3_codes(dense, 1.0), R.e4m3_codes(full[:, :cols], 1.0)).all()
    # the bf16-rounded LayerNorm result instead of the fp32 one
    c = ("ln_T", "bf16", 256, 7, 0, 0, "plain")
    y = N.ln_reference(c)[0].float()
    inv8 = R.ln8_inv8(c)[0][1]
    assert not R.same_codes(R.e4m3_codes(N.bf(y), inv8), R.e4m3_codes(y, inv8)).all()


def test_quant_inputs_reach_every_code_class():
    x = R.all_bf16_patterns()
    codes = R.e4m3_codes(x, 1.0)
    assert set(codes.unique().tolist()) == set(range(256)) - {0x7F, 0xFF}, "every finite code is produced at inv = 1"
    for rows, cols, ldin, ldo in R.QUANT_GEOMS:
        assert cols % 8 == 0 and ldin % 8 == 0 and ldo % 8 == 0 and ldin >= cols and ldo >= cols
        full = R.quant_geom_inputs(rows, cols, ldin)
        assert torch.equal(N.bf(full), full), "bf16-exact: the cast in front of the kernel is exact"
        assert ldin == cols or (full[:, cols:].abs() > 2.9e38).all()
    for rows, cols, ldin, ldo in R.QUANT_REFUSED:
        assert (cols % 8 or ldin % 8 or ldo % 8) and rows * ldin % 4 == 0


def test_amax_inputs_and_reference():
    for place in R.AMAX_PLACES:
        for neg in (False, True):
            x = R.amax_inputs(7, 24, 40, place, neg)
            assert torch.equal(N.bf(x), x)
            body = x[:, :24]
            assert (body.abs() == R.AMAX_PEAK).sum() == 1 and (body.abs().flatten().sort().values[-2] <= 1.0)
            assert R.amax_ref(0.0, x, 24) == R.AMAX_PEAK and R.amax_ref(9.0, x, 24) == 9.0 and R.amax_ref(0.5, x, 24) == R.AMAX_PEAK
    x = R.amax_inputs(7, 24, 24, "odd_half")
    r, c = (x.abs() == R.AMAX_PEAK).nonzero()[0].tolist()
    assert c % 2 == 1 and (x[r, c - c % 8:c - c % 8 + 8] != 0).sum() == 1
    x = R.amax_inputs(7, 24, 24, "last")
    assert x[-1, -1] == R.AMAX_PEAK
    rows, cols = R.AMAX_BIG
    assert rows * cols // 8 > 2048 * 256 * 8, "past the grid cap of launch_amax"
    x[3, 3] = float("nan")
    assert torch.isnan(R.amax_ref(0.0, x, 24))


def test_interval_form():
    y = torch.tensor([0.0, 1.0, 1.0625, 1.0625, -1.0625, 500.0, -3e-4, 0.3], dtype=torch.float64)
    d = torch.tensor([0.0, 1e-6, 1e-6, 0.0, 1e-6, 10.0, 1e-6, 1e-5], dtype=torch.float64)
    lo, hi = R.interval_codes(y, d)
    assert lo.tolist()[:2] == [0x00, 0x38] and hi.tolist()[:2] == [0x00, 0x38]
    assert (lo[2], hi[2]) == (0x38, 0x39) and lo[3] == hi[3] == 0x38           # 1.0625: the tie between 1 and 1.125, straddled / to even
    assert (lo[4], hi[4]) == (0xB9, 0xB8)
    assert lo[5] == hi[5] == 0x7E
    assert R.lohi_share(lo, hi) == 2 / 8
    for code in (0x38, 0x39):
        assert R.inside(torch.tensor([code], dtype=torch.uint8), lo[2:3], hi[2:3]).all()
    for code in (0x37, 0x3A, 0x7F, 0xB8):
        assert not R.inside(torch.tensor([code], dtype=torch.uint8), lo[2:3], hi[2:3]).any()
    z = torch.tensor([0x00, 0x80], dtype=torch.uint8)
    assert R.inside(z, z.flip(0), z).all(), "0x00 and 0x80 are the same number"


def test_ln8_cases_reach_every_out8_kernel():
    kernels = {N.norm_kernel_of(k, p, E, E + pad) for k, p, E, rows, pad, rms, regime in R.LN8_CASES}
    assert kernels == {"rows2<1>", "rows2<2>", "rows2<3>", "rows2<4>", "layernorm_T"}
    assert ("ln_T", "bf16", 768, 33, 4, 0, "plain") in R.LN8_CASES and any(c[2] == 320 for c in R.LN8_CASES)
    assert sum(c[3] == N.BIG_ROWS for c in R.LN8_CASES) == 1
    for c in R.LN8_CASES[:: 7]:
        y = N.ln_reference(c)[0].float()
        (_, fit), (_, sat), (_, sub) = R.ln8_inv8(c)
        top = y.abs().max().item()
        assert abs(top * fit - 448 / 1.25) < 1e-3 * 448
        assert ((y * sat).abs() > 448).any(), "x 16 saturates"
        small = R.e4m3_codes(y, sub) & 0x7F
        assert small.max() <= 0x20, "/ 4096: max |out| lands at 0.0875"
        assert c[6] != "plain" or ((small < 0x08).any() and (small == 0).any()), "... and a plain row reaches the subnormal codes and zero"


@pytest.mark.parametrize("c", R.ATTN8_CASES, ids=R.attn8_case_id)
def test_attention_intervals_are_tight(c):
    """The condition of test D: at most 1 % of a case's elements may have two admissible codes."""
    ref, gate = R.attn8_reference(c)
    assert (gate > 0).all() and ref.dtype == torch.float64
    for name, inv8, lo, hi in R.attn8_intervals(c):
        share = R.lohi_share(lo, hi)
        assert (R.decode(lo) <= R.decode(hi)).all()
        assert share <= R.LOHI_CAP, f"{R.attn8_case_id(c)} {name}: lo != hi on {share:.4%} of the elements"
        # the exact value's own code lies inside, and a code one step outside does not pass where the interval is a point
        mid = R.nearest_codes64((ref.reshape(lo.shape) * inv8).float().double())
        assert R.inside(mid, lo, hi).all()


def test_attention_seed_table_is_the_first_seed_that_meets_the_condition():
    shapes = {}
    for c in R.ATTN8_CASES:
        shapes.setdefault(tuple(c[2:]), []).append(c)
    assert set(R.ATTN8_SEEDS) <= set(shapes)
    for shape, seed in R.ATTN8_SEEDS.items():
        for s in range(seed):
            shares = [R.lohi_share(lo, hi) for c in shapes[shape] for _, _, lo, hi in R.attn8_intervals(c, s)]
            assert max(shares) > R.LOHI_CAP, f"{shape}: seed {s} already meets the condition"


def test_attention_interval_shares_summary():
    worst = {}
    for c in R.ATTN8_CASES:
        for name, inv8, lo, hi in R.attn8_intervals(c):
            key = (c[0], c[5], name)
            worst[key] = max(worst.get(key, 0.0), R.lohi_share(lo, hi))
    for key in sorted(worst):
        print(f"[fp8-producers] lo != hi share, worst case of {' '.join(key)}: {worst[key]:.5%} (cap {R.LOHI_CAP:.0%})")
    assert {c[0] for c in R.ATTN8_CASES} == {"vit_attn8", "vit_attn16", "vit_attn_lds", "vit_attn_cls"} and {c[5] for c in R.ATTN8_CASES} == set(V.REGIMES)
