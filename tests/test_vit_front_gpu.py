"""The non-GEMM kernels of the ViT front end, one launch each through the operator entry points (vima_op_vit_attention, _cls, vima_op_patchify,
vima_op_vit_embed, vima_op_bbox_l1), per output element against fp64 (tests/vit_front_reference.py: references, cases and derived gates;
tests/test_vit_front_reference.py pins them on the CPU).

Which kernel runs (launch_vit_attn / the entry points; there is no per-kernel record in `prof`, so `_kernel_of` restates the rule and the case
tables are checked against it):
  vima_op_vit_attention  impl 0, bf16 handle, S = 5, W = 768, heads = 24 (and VIMA_VIT_ATTN_LDS not 0)   vit_attn_lds_kernel
                         otherwise S > 8 or impl 2                                                       vit_attn_kernel<T, 16>
                         otherwise                                                                       vit_attn_kernel<T, 8>
  vima_op_vit_attention_cls                                                                              vit_attn_cls_kernel
  vima_op_patchify       impl 0 at (H, W, P) = (32, 32, 16): patchify_kernel, else patchify_rect_kernel
  vima_op_vit_embed      impl 0 with cls, S = 5, n_patch = 4: vit_embed_kernel, else vit_embed_rect_kernel

A  every case per element against fp64 inside the derived gate;  B  exact selection: softmax weights of exactly 0 and 1, the output must BE
the selected V row;  C  the equalities the code claims in comments, bit for bit;  D  crops (rows) do not see each other;  E  refusals.
Every output buffer is pre-filled with NaN."""
import os

import pytest
import torch

from tests import vit_front_reference as R
from tests.gpu_common import bare_policy, ptr
from vima_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
_worst = {}


def _kernel_of(op, prec, impl=0, S=0, W=0, heads=0, H=0, P=0, n_patch=0, has_cls=False):
    if op == "vit_attention":
        assert (os.environ.get("VIMA_VIT_ATTN_LDS") or "1")[0] != "0", "VIMA_VIT_ATTN_LDS=0 takes the LDS-staged kernel out of the launcher"
        if impl == 0 and prec == "bf16" and (S, W, heads) == (5, 768, 24):
            return "vit_attn_lds"
        return "vit_attn16" if S > 8 or impl == 2 else "vit_attn8"
    if op == "vit_attention_cls":
        return "vit_attn_cls"
    if op == "patchify":
        return "patchify" if impl == 0 and (H, W, P) == (32, 32, 16) else "patchify_rect"
    assert op == "vit_embed"
    return "vit_embed" if impl == 0 and has_cls and (S, n_patch) == (5, 4) else "vit_embed_rect"


def _call(fn, pol, *args):
    """-> (return code, message)."""
    rc = fn(pol._handle, *args, pol._stream())
    torch.cuda.synchronize()
    return rc, (pol._lib.vima_last_error().decode("utf-8", "replace") if rc else "")


def _ok(fn, pol, *args):
    rc, msg = _call(fn, pol, *args)
    assert rc == 0, msg


def run_attention(prec, qkv, M, S, W, impl):
    pol = bare_policy(prec)
    out = torch.full((M * S, W), NAN, device=DEV)
    qd = qkv.to(DEV)
    _ok(pol._lib.vima_op_vit_attention, pol, ptr(qd), M, S, W, W // 32, impl, ptr(out))
    return out.cpu()


def run_attention_cls(prec, qkv, M, S, W):
    pol = bare_policy(prec)
    out = torch.full((M, W), NAN, device=DEV)
    q, kv = (t.to(DEV) for t in R.cls_operands(qkv, M, S, W))
    _ok(pol._lib.vima_op_vit_attention_cls, pol, ptr(q), ptr(kv), M, S, W, W // 32, ptr(out))
    return out.cpu()


def run_attn_case(c, qkv=None):
    """The launch of an attention case (on other values of the same shape if qkv is given) -> fp32 [M, Sq, heads, 32] on the CPU."""
    kern, prec, W, S, M, regime = c
    qkv = R.attn_inputs(W, S, M, regime) if qkv is None else qkv
    if kern == "vit_attn_cls":
        assert _kernel_of("vit_attention_cls", prec) == kern
        return run_attention_cls(prec, qkv, M, S, W).view(M, 1, W // 32, 32)
    impl = R.ATTN_IMPL[kern]
    assert _kernel_of("vit_attention", prec, impl, S, W, W // 32) == kern
    return run_attention(prec, qkv, M, S, W, impl).view(M, S, W // 32, 32)


def run_patchify(prec, img, P, impl):
    pol = bare_policy(prec)
    M, _, H, W = img.shape
    out = torch.full((M * (H // P) * (W // P), 3 * P * P), NAN, device=DEV)
    d = img.to(DEV)
    _ok(pol._lib.vima_op_patchify, pol, ptr(d), M, H, W, P, impl, ptr(out))
    return out.cpu()


def run_embed(prec, pre, cls, pos, g, b, M, S, n_patch, impl):
    pol = bare_policy(prec)
    out = torch.full((M * S, R.EW), NAN, device=DEV)
    d = [None if t is None else t.to(DEV) for t in (pre, cls, pos, g, b)]
    _ok(pol._lib.vima_op_vit_embed, pol, *(ptr(t) for t in d), M, S, n_patch, impl, ptr(out))
    return out.cpu()


def run_bbox(prec, bbox, W, b):
    pol = bare_policy(prec)
    Rn, N = bbox.shape[0], W.shape[0]
    out = torch.full((Rn, N), NAN, device=DEV)
    d = [t.to(DEV) for t in (bbox, W, b)]
    _ok(pol._lib.vima_op_bbox_l1, pol, *(ptr(t) for t in d), Rn, N, ptr(out))
    return out.cpu()


def _check(family, cid, out, ref, gate):
    """isfinite, then |out - ref64| <= gate for every element; keeps the worst err / gate of the family."""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{cid}: {int((~torch.isfinite(out)).sum())} non-finite outputs"
    ratio = (out.double() - ref).abs() / gate
    worst = ratio.max().item()
    if worst > _worst.get(family, (-1.0, ""))[0]:
        _worst[family] = (worst, cid)
    bad = ratio > 1.0
    assert not bad.any(), f"{cid}: {int(bad.sum())} elements beyond the gate, worst {worst:.3f} x at {tuple(bad.nonzero()[0].tolist())}"


# ================================================================================================================== A
def test_a_case_tables_reach_every_kernel():
    assert {c[0] for c in R.ATTN_CASES} == {"vit_attn8", "vit_attn16", "vit_attn_lds", "vit_attn_cls"}
    for kern, prec, W, S, M, regime in R.ATTN_CASES:
        if kern != "vit_attn_cls":
            assert _kernel_of("vit_attention", prec, R.ATTN_IMPL[kern], S, W, W // 32) == kern
    assert {(k, p) for k, p, *_ in R.ATTN_CASES} == {(k, p) for k in ("vit_attn8", "vit_attn16", "vit_attn_cls") for p in R.PRECS} | {("vit_attn_lds", "bf16")}
    for cases, op in ((R.PATCHIFY_CASES, "patchify"), (R.EMBED_CASES, "vit_embed")):
        assert {(c[0], c[1]) for c in cases} == {(k, p) for k in (op, op + "_rect") for p in R.PRECS}
    for k, p, H, W, P, M, impl in R.PATCHIFY_CASES:
        assert _kernel_of("patchify", p, impl, H=H, W=W, P=P) == k
    for k, p, S, n, cl, M, r, impl in R.EMBED_CASES:
        assert _kernel_of("vit_embed", p, impl, S=S, n_patch=n, has_cls=cl) == k


@pytest.mark.parametrize("c", R.ATTN_CASES, ids=R.attn_case_id)
def test_a_attention_against_fp64_per_element(c):
    """Would fail: a key row of another crop or head, a dropped or phantom key, a wrong scale, chunks of a head out of order (the mutations
    tests/test_vit_front_reference.py holds the gates against), and any fp32 accumulation looser than the dot product's own forward error."""
    ref, _, gate = R.attn_reference(c)
    _check(f"{c[0]} {c[1]} {c[5]}", R.attn_case_id(c), run_attn_case(c), ref, gate)


@pytest.mark.parametrize("c", R.PATCHIFY_CASES, ids=R.patchify_case_id)
def test_a_patchify_against_fp64_per_element(c):
    kern, prec, H, W, P, M, impl = c
    ref, gate = R.patchify_reference(c)
    _check(f"{kern} {prec}", R.patchify_case_id(c), run_patchify(prec, R.patchify_inputs(H, W, M), P, impl), ref, gate)


@pytest.mark.parametrize("c", R.EMBED_CASES, ids=R.embed_case_id)
def test_a_embed_against_fp64_per_element(c):
    kern, prec, S, n, has_cls, M, regime, impl = c
    ref, gate = R.embed_reference(c)
    _check(f"{kern} {prec} {regime}", R.embed_case_id(c), run_embed(prec, *R.embed_inputs(S, n, has_cls, M, regime), M, S, n, impl), ref, gate)


@pytest.mark.parametrize("c", R.BBOX_CASES, ids=R.bbox_case_id)
def test_a_bbox_against_fp64_per_element(c):
    prec, Rn, N = c
    ref, gate = R.bbox_reference(c)
    _check(f"bbox_l1 {prec}", R.bbox_case_id(c), run_bbox(prec, *R.bbox_inputs(Rn, N)), ref, gate)


# ================================================================================================================== B
SELECT = ([("vit_attn8", p, W, S, M) for p in R.PRECS for W, S, M in ((64, 1, 3), (64, 2, 3), (768, 5, 107), (64, 8, 107), (768, 8, 3))] +
          [("vit_attn16", p, W, S, M) for p in R.PRECS for W, S, M in ((64, 9, 11), (768, 13, 1), (768, 16, 11), (768, 5, 3))] +
          [("vit_attn_lds", "bf16", 768, 5, M) for M in (1, 2, 3, 55)] +
          [("vit_attn_cls", p, W, S, M) for p in R.PRECS for W, S, M in ((64, 1, 3), (768, 5, 107), (64, 8, 3), (768, 8, 3))])


@pytest.mark.parametrize("c", SELECT, ids=lambda c: "-".join(str(x) for x in c))
def test_b_exact_selection(c):
    """Every softmax weight is exactly 0 or 1 (tests/vit_front_reference.select_inputs), every value exact in bf16: the output must BE row
    pi(m, i, h) of V, bit for bit, in both precisions. A row, head, chunk or swizzle misplacement returns other integers; q and k chunks
    that disagree make every score 0 and return the mean of V."""
    kern, prec, W, S, M = c
    qkv, want = R.select_inputs(W, S, M)
    if kern == "vit_attn_cls":
        got, want = run_attention_cls(prec, qkv, M, S, W), want.view(M, S, W)[:, 0]
    else:
        impl = 2 if kern == "vit_attn16" else R.ATTN_IMPL[kern]
        assert _kernel_of("vit_attention", prec, impl, S, W, W // 32) == kern
        got = run_attention(prec, qkv, M, S, W, impl)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} elements are not the selected V value; first at {tuple((got != want).nonzero()[0].tolist())}"


# ================================================================================================================== C
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("M", [1, 2, 3, 55])
def test_c_lds_kernel_is_the_register_kernel_bit_for_bit(M, regime):
    """attention.hip: "Same per-head body as the other two kernels: bit-identical results" (LDS-DMA staging and the per-head XOR swizzle
    change where the operands are read from, not the arithmetic)."""
    qkv = R.attn_inputs(768, 5, M, regime)
    assert _kernel_of("vit_attention", "bf16", 0, 5, 768, 24) == "vit_attn_lds" and _kernel_of("vit_attention", "bf16", 1, 5, 768, 24) == "vit_attn8"
    lds, reg = run_attention("bf16", qkv, M, 5, 768, 0), run_attention("bf16", qkv, M, 5, 768, 1)
    assert torch.isfinite(lds).all() and torch.equal(lds, reg)


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("S", [1, 5, 8])
def test_c_sixteen_score_instantiation_is_the_eight_score_one_bit_for_bit(S, prec):
    """vit_head_attention: "Rows j >= S contribute exp = 0.f to the sum and nothing else, so the result does not depend on SM"."""
    for W, M in ((64, 107), (768, 3)):
        for regime in R.REGIMES:
            qkv = R.attn_inputs(W, S, M, regime)
            a, b = run_attention(prec, qkv, M, S, W, 1), run_attention(prec, qkv, M, S, W, 2)
            assert torch.isfinite(a).all() and torch.equal(a, b), (W, M, regime)


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("S", [1, 5, 8])
def test_c_cls_kernel_is_row_zero_of_the_full_kernel_bit_for_bit(S, prec):
    """vit_chunk's pruned last block: "identical values for that row". At the bf16 hot shape against the LDS-staged kernel and the register one."""
    for W, M in ((64, 107), (768, 3), (768, 55)):
        for regime in R.REGIMES:
            qkv = R.attn_inputs(W, S, M, regime)
            cls = run_attention_cls(prec, qkv, M, S, W)
            assert torch.isfinite(cls).all()
            impls = (0, 1) if _kernel_of("vit_attention", prec, 0, S, W, W // 32) == "vit_attn_lds" else (1,)
            for impl in impls:
                full = run_attention(prec, qkv, M, S, W, impl)
                assert torch.equal(cls, full.view(M, S, W)[:, 0]), (W, M, regime, impl)


@pytest.mark.parametrize("prec", R.PRECS)
def test_c_rect_kernels_are_the_crop_kernels_bit_for_bit(prec):
    img = R.patchify_inputs(32, 32, 43)
    a, b = run_patchify(prec, img, 16, 0), run_patchify(prec, img, 16, 1)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    for regime in R.EMBED_REGIMES:
        x = R.embed_inputs(5, 4, True, 51, regime)
        a, b = run_embed(prec, *x, 51, 5, 4, 0), run_embed(prec, *x, 51, 5, 4, 1)
        assert torch.isfinite(a).all() and torch.equal(a, b), regime


# ================================================================================================================== D
ISOLATION = ([("vit_attn8", p, W, S, M, keep) for p in R.PRECS for W, S, M in ((64, 5, 107), (768, 8, 3)) for keep in (0, M - 1)] +
             [("vit_attn16", p, 768, 13, 11, keep) for p in R.PRECS for keep in (0, 10)] +
             [("vit_attn_cls", p, W, S, M, keep) for p in R.PRECS for W, S, M in ((64, 5, 107), (768, 8, 3)) for keep in (0, M - 1)] +
             # LDS kernel, two crops per workgroup: first, last, the partner inside a workgroup (crop 1 of 0 | 1, crop 52 of 52 | 53), the single crop of an odd tail
             [("vit_attn_lds", "bf16", 768, 5, M, keep) for M, keep in ((55, 0), (55, 54), (55, 1), (55, 52), (3, 2), (2, 1), (54, 53))])


@pytest.mark.parametrize("c", ISOLATION, ids=lambda c: "-".join(str(x) for x in c))
def test_d_crops_do_not_see_each_other(c):
    """Every crop but one redrawn: the kept crop's output does not move by a bit, every other crop's does."""
    kern, prec, W, S, M, keep = c
    case = (kern, prec, W, S, M, "normal")
    a, b = R.attn_inputs(W, S, M, "normal"), R.attn_inputs(W, S, M, "normal", seed=1)
    sel = torch.zeros(M, 1, dtype=torch.bool)
    sel[keep] = True
    mixed = torch.where(sel.repeat_interleave(S, dim=0), a, b)
    base, got = run_attn_case(case, a), run_attn_case(case, mixed)
    assert torch.isfinite(base).all() and torch.isfinite(got).all()
    assert torch.equal(got[keep], base[keep])
    moved = (got != base).flatten(1).any(dim=1)
    assert moved.sum().item() == M - 1 and not moved[keep]


@pytest.mark.parametrize("prec", R.PRECS)
def test_d_patchify_and_embed_rows_do_not_see_each_other(prec):
    M = 3
    for keep in (0, M - 1):
        sel = torch.zeros(M, dtype=torch.bool)
        sel[keep] = True
        for H, W, P, impl in ((32, 32, 16, 0), (32, 32, 16, 1), (64, 128, 32, 0)):
            a, b = R.patchify_inputs(H, W, M), R.patchify_inputs(H, W, M, seed=1)
            base = run_patchify(prec, a, P, impl).view(M, -1)
            got = run_patchify(prec, torch.where(sel[:, None, None, None], a, b), P, impl).view(M, -1)
            assert torch.isfinite(got).all() and torch.equal(got[keep], base[keep])
            assert (got != base).any(dim=1).sum().item() == M - 1
        for S, n, has_cls, impl in ((5, 4, True, 0), (5, 4, True, 1), (9, 8, True, 0), (8, 8, False, 0)):
            pre, cls, pos, g, b = R.embed_inputs(S, n, has_cls, M, "plain")
            pre2 = R.embed_inputs(S, n, has_cls, M, "plain", seed=1)[0]
            base = run_embed(prec, pre, cls, pos, g, b, M, S, n, impl).view(M, S, -1)
            got = run_embed(prec, torch.where(sel.repeat_interleave(n)[:, None], pre, pre2), cls, pos, g, b, M, S, n, impl).view(M, S, -1)
            assert torch.isfinite(got).all() and torch.equal(got[keep], base[keep])
            first = 1 if has_cls else 0                            # the cls row does not depend on the crop
            assert torch.equal(got[:, :first], base[:, :first])
            assert (got[:, first:] != base[:, first:]).flatten(1).any(dim=1).sum().item() == M - 1


# ================================================================================================================== E
def _refused(fn, prec, out, *args):
    pol = bare_policy(prec)
    rc, msg = _call(fn, pol, *args, ptr(out))
    assert rc != 0 and msg, (rc, msg)
    assert torch.isnan(out).all(), "a refused call wrote to its output"
    return msg


@pytest.mark.parametrize("prec", R.PRECS)
def test_e_refusals(prec):
    lib = bare_policy(prec)._lib
    out = torch.full((17 * 768,), NAN, device=DEV)
    x = torch.randn(17 * 3 * 768, device=DEV)
    img = torch.zeros(3 * 96 * 96, dtype=torch.uint8, device=DEV)
    assert "vit_attn" in _refused(lib.vima_op_vit_attention, prec, out, ptr(x), 1, 17, 768, 24, 0)             # S = 17: more than the 16 score registers
    assert "vit_attn" in _refused(lib.vima_op_vit_attention, prec, out, ptr(x), 1, 17, 64, 2, 2)
    assert "vit_attn_cls" in _refused(lib.vima_op_vit_attention_cls, prec, out, ptr(x), ptr(x), 1, 9, 768, 24)  # S = 9: more than the cls kernel's 8
    assert "head dim" in _refused(lib.vima_op_vit_attention, prec, out, ptr(x), 1, 5, 768, 12, 0)
    assert "impl" in _refused(lib.vima_op_vit_attention, prec, out, ptr(x), 1, 5, 768, 24, 3)
    assert "patchify_rect" in _refused(lib.vima_op_patchify, prec, out, ptr(img), 1, 48, 48, 24, 0)              # P = 24: no multiple of 16
    assert "patchify_rect" in _refused(lib.vima_op_patchify, prec, out, ptr(img), 1, 32, 40, 16, 0)              # W no multiple of P
    assert "patchify_rect" in _refused(lib.vima_op_patchify, prec, out, ptr(img), 1, 40, 32, 16, 0)              # H no multiple of P
    assert "positive" in _refused(lib.vima_op_patchify, prec, out, ptr(img), 1, 32, 32, 0, 0)
    assert "n_patch" in _refused(lib.vima_op_vit_embed, prec, out, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), 1, 6, 4, 0)   # 5 patch rows needed, 4 there
    assert "null" in _refused(lib.vima_op_vit_embed, prec, out, ptr(x), ptr(x), None, ptr(x), ptr(x), 1, 5, 4, 0)
    assert "positive" in _refused(lib.vima_op_bbox_l1, prec, out, ptr(x), ptr(x), ptr(x), 0, 768)


def test_zz_print_the_worst_ratios():
    """Last in the file: the worst err / gate per family and kernel (profiles/vit_front_errors.txt records them)."""
    for family in sorted(_worst):
        ratio, cid = _worst[family]
        print(f"[vit-front] worst err / gate, {family}: {ratio:.3f} at {cid}")
