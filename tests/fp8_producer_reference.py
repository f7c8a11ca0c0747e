"""CPU references, input builders and case tables shared by tests/test_fp8_producer_reference.py (which pins all of this on the CPU) and
tests/test_fp8_producers_gpu.py (which holds every kernel that writes e4m3 bytes, or measures the scale for them, outside the GEMM epilogue):

  quant_fp8_kernel, amax_kernel                                                                  (vima_op_fp8_quant, vima_op_fp8_amax)
  the out8 path of layernorm_kernel<bf16, bf16> and layernorm_rows2_kernel<1..4>                 (vima_op_norm_fp8)
  vit_store_head's e4m3 branch in vit_attn_kernel<bf16, 8 | 16>, vit_attn_lds_kernel, vit_attn_cls_kernel
                                                                                                 (vima_op_vit_attention_fp8, _cls_fp8)

All of them end in fmed3(v * inv, -448, 448) and cvt_pk_fp8_f32 on an fp32 value v, so given v the output is ONE definite byte:

  e4m3_codes(v32, inv)      the reference conversion: fp32 product (one rounding), clamp to +-448, torch.float8_e4m3fn (round to nearest even),
                            as uint8. test_fp8_producer_reference.py pins it against `nearest_codes64`, an independent fp64 nearest-even search
                            over the decodes of the 256 codes, on every finite bf16 bit pattern.
  interval_codes(y64, d)    for an output whose fp32 pre-image is not observable: lo = e4m3(clamp(fl32(y - d))), hi = e4m3(clamp(fl32(y + d))).
                            fp32 rounding, the clamp and round-to-nearest are all monotone, so a kernel whose value lies within d of y must
                            emit a code c with decode(lo) <= decode(c) <= decode(hi). The share of elements with lo != hi is a CONDITION
                            (at most LOHI_CAP per case, asserted on the CPU from the reference alone): a looser share would make the check vacuous.

Every comparison of codes treats 0x00 and 0x80 as equal (`same_codes`): +0 and -0 are one number to the consuming MFMA, and which of the two a
result that rounds to zero keeps is the only freedom of the conversion. Nothing else is excused.
The LayerNorm and attention inputs, references and gates are those of tests/seq_norm_reference.py and tests/vit_front_reference.py.
No GPU and no vima_amd import here."""
import functools

import torch

from tests import seq_norm_reference as N
from tests import vit_front_reference as V

CANARY_U8 = 0x7F                    # e4m3 NaN: no producer can emit it from clamped input
TAIL = 64                           # guard bytes behind every output buffer
E4M3_MAX = 448.0
LOHI_CAP = 0.01
PAD_IN = 3e38                       # pad columns of quant / amax inputs (+-): a kernel that reads them saturates or reports them


def f32(v):
    """A Python float as the fp32 the C ABI hands the kernel."""
    return torch.tensor(v, dtype=torch.float32).item()


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ================================================================================================================== the conversion
@functools.lru_cache(maxsize=None)
def decode_table():
    """fp64 [256]: the value of every OCP e4m3 code (0x7F / 0xFF: NaN). Written from the format's definition: sign, 4 exponent bits (bias 7),
    3 mantissa bits, subnormals m / 8 * 2^-6, no infinities."""
    c = torch.arange(256)
    e, m = ((c >> 3) & 15).double(), (c & 7).double()
    mag = torch.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * 2.0 ** (e - 7))
    val = torch.where(c >= 128, -mag, mag)
    val[0x7F] = val[0xFF] = float("nan")
    return val


def decode(codes):
    return decode_table()[codes.long()]


def e4m3_codes(v32, inv):
    """uint8 codes of e4m3(clamp(v32 * inv, +-448)): ONE fp32 rounding of the product, as in the kernels, then round to nearest even."""
    assert v32.dtype == torch.float32
    p = v32 * torch.tensor(inv, dtype=torch.float32)
    return p.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def nearest_codes64(y64, truncate=False, limit=E4M3_MAX):
    """The independent statement: clamp, then the nearest of the finite non-negative decodes (codes 0x00 .. 0x7E, ascending with the code) to
    |y|, a tie to the even code, the sign bit on top. truncate / limit are the mutations 'round toward zero' and 'saturate at 240'."""
    assert y64.dtype == torch.float64
    grid = decode_table()[:0x7F]
    a = y64.abs().clamp(max=limit)
    hi = torch.searchsorted(grid, a).clamp(1, 0x7E)             # grid[hi - 1] <= a <= grid[hi] (a = 0: hi = 1)
    lo = hi - 1
    dlo, dhi = a - grid[lo], grid[hi] - a
    up = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    if truncate:
        up = dhi == 0
    code = torch.where(up, hi, lo)
    return (code + 128 * torch.signbit(y64).long()).to(torch.uint8)


def same_codes(a, b):
    """Elementwise: equal, or 0x00 against 0x80."""
    return (a == b) | (((a | b) & 0x7F) == 0)


def signed_zero_share(a, b):
    return ((a != b) & same_codes(a, b)).double().mean().item()


def interval_codes(y64, delta):
    """-> (lo, hi) uint8. y64 is the exact scaled output, delta >= 0 what the kernel's fp32 value may be away from it (both already x inv)."""
    assert y64.dtype == torch.float64
    return e4m3_codes((y64 - delta).float(), 1.0), e4m3_codes((y64 + delta).float(), 1.0)


def lohi_share(lo, hi):
    return (~same_codes(lo, hi)).double().mean().item()


def inside(codes, lo, hi):
    """Elementwise decode(lo) <= decode(codes) <= decode(hi); a NaN code (the canary) is outside."""
    d = decode(codes)
    return (decode(lo) <= d) & (d <= decode(hi))


def inv8_set(max_abs):
    """The three scales of a case (C, D): max |out| lands at 448 / 1.25 (the calibrated headroom); x 16 saturates a visible share; / 4096 lands in
    the subnormal and zero range."""
    base = f32(E4M3_MAX / 1.25 / max_abs)
    return (("fit", base), ("sat", f32(base * 16)), ("sub", f32(base / 4096)))


# ================================================================================================================== A  quant_fp8
QUANT_INVS = (1.0, f32(1 / 3), f32(448 / 3.7), 2.0 ** -20, 2.0 ** 20)
# (rows, cols, ldin, ldo)
QUANT_GEOMS = ((1, 8, 8, 8), (7, 24, 40, 32), (33, 768, 768, 768), (257, 3072, 3080, 3088))
QUANT_REFUSED = ((4, 12, 16, 16), (4, 8, 12, 16), (4, 8, 16, 12))      # cols, ldin, ldo no multiple of 8 (rows * ldin stays a multiple of 4: the cast runs)


def all_bf16_patterns():
    """fp32 [8, 8192]: every bf16 bit pattern once, in order (element i = pattern i), the NaN patterns replaced by finite values of their own."""
    bits = torch.arange(65536, dtype=torch.int32)
    nan = ((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0)
    bits = torch.where(nan, bits & ~0x4000, bits)                # exponent 0xFF -> 0x7F: magnitudes in [1, 2), the sign kept
    x = (bits << 16).view(torch.float32).reshape(8, 8192)
    assert torch.isfinite(x).sum() == 65536 - 2
    return x


def finite_bf16_patterns():
    """fp32 [65280]: every FINITE bf16 bit pattern."""
    bits = torch.arange(65536, dtype=torch.int32)
    return (bits[(bits & 0x7F80) != 0x7F80] << 16).view(torch.float32)


def padded(x, ld, fill=PAD_IN):
    """[rows, cols] -> [rows, ld] with +-fill (bf16-exact, alternating sign) in the pad columns."""
    rows, cols = x.shape
    full = torch.empty(rows, ld)
    full[:, :cols] = x
    if ld > cols:
        sign = 1.0 - 2.0 * ((torch.arange(rows)[:, None] + torch.arange(ld - cols)[None, :]) % 2)
        full[:, cols:] = N.bf(torch.tensor(fill)) * sign
    return full


@functools.lru_cache(maxsize=None)
def quant_geom_inputs(rows, cols, ldin):
    """x fp32 [rows, ldin], bf16-exact: log-uniform magnitudes over 2^-12 .. 2^10 with random signs (zeros, subnormal results, normals and
    saturation at inv = 1), +-3e38 in the pad columns."""
    gen = _gen(81, rows, cols, ldin)
    mag = 2.0 ** (torch.rand(rows, cols, generator=gen) * 22 - 12)
    sign = 1.0 - 2.0 * torch.randint(0, 2, (rows, cols), generator=gen)
    return padded(N.bf(mag * sign), ldin)


# ================================================================================================================== B  amax
AMAX_SLOTS = ("zero", "above", "below")
AMAX_PLACES = ("first", "last", "odd_half")
AMAX_BIG = (8200, 4096)             # rows x cols / 8 = 4 198 400 vectors > 2048 x 256 x 8: one grid-stride round more, with a partial tail
AMAX_PEAK = 7.5


def amax_inputs(rows, cols, ldin, place, negative=False):
    """x fp32 [rows, ldin], bf16-exact: |x| <= 1 everywhere (a repeated tile of random values) except ONE element of magnitude 7.5 at `place`
    ("first": [0, 0]; "last": [rows - 1, cols - 1], which sits in the last 8-element vector; "odd_half": an odd column of a vector whose other
    seven elements are zero); 3e38 in the pad columns."""
    tile = N.bf(torch.rand(64, 64, generator=_gen(82, rows, cols)) * 2 - 1)
    x = tile.repeat((rows + 63) // 64, (cols + 63) // 64)[:rows, :cols].clone()
    r, c = {"first": (0, 0), "last": (rows - 1, cols - 1), "odd_half": (rows // 2, (cols // 2 // 8) * 8 + 5)}[place]
    if place == "odd_half":
        x[r, c - 5:c + 3] = 0.0
    x[r, c] = -AMAX_PEAK if negative else AMAX_PEAK
    return padded(x, ldin, fill=PAD_IN) if ldin > cols else x


def amax_ref(slot0, x, cols):
    """max(slot0, max |x[:, :cols]|) as fp32; a NaN in the data makes it NaN."""
    body = x[:, :cols]
    if torch.isnan(body).any():
        return torch.tensor(float("nan"))
    return torch.maximum(torch.tensor(slot0, dtype=torch.float32), body.abs().max())


# ================================================================================================================== C  LayerNorm out8
LN8_REGIMES = ("plain", "offset", "spike")
# (E, pad): rows2<1..4> at ldin % 8 == 0, the one-wave kernel at E = 320 and at E = 768 with ldin = 772
LN8_LAYOUTS = ((256, 0), (512, 8), (768, 0), (1024, 8), (320, 0), (768, 4))
LN8_CASES = ([("ln_T", "bf16", E, rows, pad, rms, regime) for E, pad in LN8_LAYOUTS for rows in (1, 2, 7, 33) for rms in (0, 1) for regime in LN8_REGIMES] +
             [("ln_T", "bf16", 256, N.BIG_ROWS, 0, 0, "plain")])


def ln8_case_id(c):
    return "out8-" + N.norm_case_id(c)


def ln8_inv8(c):
    """The three inv8 of a case, from the fp64 reference's max |out| (not from any kernel output)."""
    return inv8_set(N.ln_reference(c)[0].abs().max().item())


# ================================================================================================================== D  ViT attention out8
ATTN8_CASES = [c for c in V.ATTN_CASES if c[1] == "bf16"]
attn8_case_id = V.attn_case_id


# The input seed of a shape (W, S, M, regime) where it is not 0. The smallest cls cases have 64 outputs, so ONE element whose exact value sits
# within the gate of a rounding boundary already exceeds the 1 % condition (the peaked one-crop case at W = 768 drew 10 of 768). Such a shape
# takes the first seed at which every case of the shape meets the condition at all three inv8 -- found from the reference alone
# (test_fp8_producer_reference.py asserts the condition for every case and that every smaller seed misses it); the cap is not touched.
ATTN8_SEEDS = {(64, 5, 1, "normal"): 1, (64, 5, 3, "normal"): 1, (64, 8, 1, "normal"): 1, (64, 8, 1, "peaked"): 1, (768, 8, 1, "peaked"): 1}


def attn8_seed(c):
    return ATTN8_SEEDS.get(tuple(c[2:]), 0)


def attn8_inputs(c):
    """qkv fp32 [M*S, 3W] of a case: vit_front_reference.attn_inputs at the shape's seed."""
    _, _, W, S, M, regime = c
    return V.attn_inputs(W, S, M, regime, attn8_seed(c))


@functools.lru_cache(maxsize=None)
def _attn8_reference(cls, W, S, M, regime, seed):
    q, k, v = V.split_qkv(V.rounded("bf16", V.attn_inputs(W, S, M, regime, seed)), M, S, W)
    if cls:
        q = q[:, :1]
    ref, rowscale = V.attn_ref64(q, k, v)
    return ref, V.attn_gate(regime, "fp32", q, k, ref, rowscale)


def attn8_reference(c, seed=None):
    """-> (ref fp64 [M, Sq, H, 32] of the bf16-rounded operands, gate): the gate an fp32 handle gets for the same case, i.e. attn_gate without the
    bf16 output-rounding term, which the out8 path does not have (it converts the fp32 head output)."""
    kern, _, W, S, M, regime = c
    return _attn8_reference(kern == "vit_attn_cls", W, S, M, regime, attn8_seed(c) if seed is None else seed)


def attn8_intervals(c, seed=None):
    """-> [(name, inv8, lo, hi)] with lo, hi uint8 [rows, W] in the layout of out8."""
    kern, _, W, S, M, _ = c
    ref, gate = attn8_reference(c, seed)
    ref, gate = ref.reshape(-1, W), gate.reshape(-1, W)
    out = []
    for name, inv8 in inv8_set(ref.abs().max().item()):
        lo, hi = interval_codes(ref * inv8, gate * inv8)
        out.append((name, inv8, lo, hi))
    return out
