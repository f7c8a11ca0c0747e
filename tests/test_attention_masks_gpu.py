"""Structured key masks in every attention kernel, per output element against fp64 (tests/attn_mask_reference.py).

The op-level tests draw one kind of mask (80 % iid, key 0 valid). Here each of the 15 samples of a launch carries one STRUCTURE (valid prefixes and
suffixes around the key-tile size T, a dead tile between two clean ones, single masked keys on sub-tile boundaries, one valid key, none, and
the iid mask as a control), so that clean, partly masked and dead tiles, a dead FIRST tile and a fully masked row meet in one launch. H = 2.

Which kernel runs (launch_attn_mfma / Run::attn; there is no per-kernel attention record in `prof`, so `_kernel_of` restates the rule and
the case table is checked against it):
  impl 0                                        attn_generic (any precision, head dims 16 / 64 here)
  impl 1, bf16x3 handle                         attn_x3 (launch_attn_x3: attn_mfma's one-wave kernel with X3 = true, fp32 operands)
  impl 1, bf16 handle, Lq <= 32, Lk >= 64, not T5  attn_split (128-key tiles, a 32-key quarter per wave; Lk = 300: waves 2, 3 of the last tile see no key)
  impl 1, bf16 handle, Lq >= attn4_min_lq (64)  attn_mfma4 (64-key tiles); 64 queries per wave with attn_qg 2 from Lq = 256 on, not in causal mode
  impl 1, bf16 handle, otherwise                attn_mfma (32-key tiles, one wave per 32 queries)

Gates (attn_mask_reference.gate_of): bf16 kernels 3 * 2^-8 of rowscale = sum p |v| (probabilities rounded, output rounded, normalisation by
the unrounded sum: u each), fp32 generic 1e-5 of rowscale, bf16x3 2e-5 absolute on inputs uniform in [-1, 1]."""
import math

import pytest
import torch

from tests import attn_mask_reference as R
from tests.gpu_common import bare_policy, ptr
from vima_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULTS = {"attn4_min_lq": 64, "attn_qg": 1}
STRUCTURED = slice(1, 13)      # rows 1-12: at least one valid key, at least one masked


def _kernel_of(prec, impl, opts, mode, Lq, Lk, D):
    if impl == 0 or D not in (32, 64):
        return "generic"
    if prec == "bf16x3":
        return "attn_x3"
    assert prec == "bf16"
    if Lq <= 32 and mode != 0 and Lk >= 64:
        return "attn_split"
    if Lq >= opts.get("attn4_min_lq", 64):
        return "attn_mfma4_qg2" if opts.get("attn_qg", 1) == 2 and Lq >= 256 and mode != 2 else "attn_mfma4_qg1"
    return "attn_mfma"


def _run(c, q, k, v, kmask, relbias, scale):
    """One launch of case c's kernel on fp32 host tensors -> fp32 [B, Lq, H, D] on the CPU."""
    name, mode, Lq, Lk, q_off, D = c
    prec, impl, opts, _, _, _ = R.KERNELS[name]
    assert _kernel_of(prec, impl, {**DEFAULTS, **opts}, mode, Lq, Lk, D) == name.replace("generic_fp32", "generic").replace("generic_bf16", "generic")
    pol = bare_policy(prec)
    B = q.shape[0]
    out = torch.full((B, Lq, R.H, D), float("nan"), device=DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    md = kmask.to(DEV) if kmask is not None else None
    rd = relbias.to(DEV) if relbias is not None else None
    try:
        for o, val in {**DEFAULTS, **opts}.items():
            pol.set_option(o, val)
        if q_off is None:
            _lib.check(pol._lib.vima_op_attention(pol._handle, ptr(qd), ptr(kd), ptr(vd), ptr(md), ptr(rd), B, R.H, Lq, Lk, D, scale, mode, impl,
                                                  ptr(out), pol._stream()))
        else:
            assert mode == 2
            _lib.check(pol._lib.vima_op_attention_window(pol._handle, ptr(qd), ptr(kd), ptr(vd), ptr(md), B, R.H, Lq, Lk, D, scale, impl, q_off,
                                                         ptr(out), pol._stream()))
        torch.cuda.synchronize()
    finally:
        for o, val in DEFAULTS.items():
            pol.set_option(o, val)
    return out.cpu()


_outs = {}


def _structured_out(c):
    """The launch with the 15 structures as key masks; Tests A and B share it."""
    if c not in _outs:
        q, k, v, relbias, scale = R.inputs(*c)
        _outs[c] = _run(c, q, k, v, R.structures(c[3], R.KERNELS[c[0]][3]), relbias, scale)
    return _outs[c]


def _which(flags, rows):
    return sorted({rows[i] for i in flags.nonzero()[:, 0].tolist()})


def _check_against_ref64(tag, c, out, ref, rowscale, rows=None):
    """isfinite, |out - ref64| <= gate * rowscale + abs for every element; prints the worst err / rowscale, where, and the iid control row's."""
    rel_gate, abs_gate = R.gate_of(c[0])
    rows = list(range(out.shape[0])) if rows is None else rows
    assert torch.isfinite(out).all(), f"{R.case_id(c)}: non-finite output in structures {_which(~torch.isfinite(out), rows)}"
    err = (out.double() - ref).abs()
    rel = (err / rowscale).flatten(1).max(dim=1).values                     # per structure
    worst = int(rel.argmax())
    line = f"[attn-mask] {tag} {R.case_id(c)}: worst err/rowscale {rel[worst].item():.2e} at structure {rows[worst]}"
    if rel_gate:
        line += f" (gate {rel_gate:.2e})"
    else:
        line += f", worst abs err {err.max().item():.2e} at structure {rows[int(err.flatten(1).max(dim=1).values.argmax())]} (gate {abs_gate:.0e} abs)"
    if R.IID in rows:
        line += f"; iid control row {rel[rows.index(R.IID)].item():.2e}"
    print(line)
    bad = err > rel_gate * rowscale + abs_gate
    assert not bad.any(), f"{R.case_id(c)}: {int(bad.sum())} elements beyond the gate, structures {_which(bad, rows)}: {line}"


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_a_every_structure_against_fp64_per_element(c):
    """Would fail: row 13 if the kernel wrote zeros or averaged over the padded tile instead of Lk keys (error ~ |mean v|, far beyond 3u of
    rowscale); rows 6-9 if the running maximum kept the masked first tile's sentinel (the valid keys would underflow to weight 0 -> NaN or the
    masked keys' mean)."""
    ref, rowscale = R.reference(*c)
    _check_against_ref64("A", c, _structured_out(c), ref, rowscale)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_b_a_masked_key_weighs_exactly_nothing(c):
    """K and V redrawn at every masked position (same distribution): structures 1-12 must not move by a bit. Any non-zero weight of a masked
    key, however small, multiplies a changed V row (or changes the normalising sum) and shows."""
    name, mode, Lq, Lk, q_off, D = c
    q, k, v, relbias, scale = R.inputs(*c)
    _, k2, v2, _, _ = R.inputs(*c, seed=1)
    kmask = R.structures(Lk, R.KERNELS[name][3])
    assert not torch.equal(k, k2) and not torch.equal(v, v2)
    sel = kmask[:, :, None, None]
    got = _run(c, q, torch.where(sel, k, k2), torch.where(sel, v, v2), kmask, relbias, scale)
    base = _structured_out(c)
    assert torch.isfinite(got[STRUCTURED]).all()
    assert torch.equal(got[STRUCTURED], base[STRUCTURED]), \
        f"structures {sorted(set((got[STRUCTURED] != base[STRUCTURED]).nonzero()[:, 0].add(1).tolist()))} moved"
    assert not torch.equal(got[R.NOTHING], base[R.NOTHING])     # (there the masked values ARE the answer: the redraw did reach the kernel)


@pytest.mark.parametrize("c", [c for c in R.CASES if c[3] in (72, 200, 300)], ids=R.case_id)
def test_c_samples_do_not_see_each_other(c):
    """All keys valid, ragged last tile (Lk = 72, 200, 300: its clamped re-reads sit next to the neighbouring sample's rows): a sample's
    output does not move by a bit when every OTHER sample is redrawn -- the first sample, then the last."""
    name, mode, Lq, Lk, q_off, D = c
    q, k, v, relbias, scale = R.inputs(*c)
    q2, k2, v2, _, _ = R.inputs(*c, seed=2)
    kmask = torch.ones(R.N_STRUCT, Lk, dtype=torch.bool)
    base = _run(c, q, k, v, kmask, relbias, scale)
    assert torch.isfinite(base).all()
    for keep in (0, R.N_STRUCT - 1):
        sel = torch.zeros(R.N_STRUCT, 1, 1, 1, dtype=torch.bool)
        sel[keep] = True
        got = _run(c, torch.where(sel, q, q2), torch.where(sel, k, k2), torch.where(sel, v, v2), kmask, relbias, scale)
        assert torch.equal(got[keep], base[keep]), keep
        assert not torch.equal(got, base)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_d_no_mask_is_the_all_ones_mask(c):
    """kmask = NULL against an all-True array, bit for bit, and both against fp64 (structure 0 of Test A is the same thing inside a launch
    whose other samples take the masked path)."""
    name, mode, Lq, Lk, q_off, D = c
    q, k, v, relbias, scale = R.inputs(*c)
    none = _run(c, q, k, v, None, relbias, scale)
    ones = _run(c, q, k, v, torch.ones(R.N_STRUCT, Lk, dtype=torch.bool), relbias, scale)
    assert torch.isfinite(none).all()
    assert torch.equal(none, ones)
    assert torch.equal(none[R.ALL_VALID], _structured_out(c)[R.ALL_VALID])


def test_e_large_scale_keeps_a_fully_masked_row_finite():
    """Cross mode on attn_mfma4 at scale 4 (q divided by 4 sqrt(D): the scores stay O(1)), structures 6, 10, 13. The mask enters that kernel as
    the S^T accumulators' initial value and is multiplied by scale * log2(e) with the score: the stored -1e38 overflowed to -inf from a scale of
    2.36 on, and a row without a valid key computed exp2(-inf - -inf) = NaN. The table now holds -1e38 / max(scale * log2(e), 1)."""
    c = ("attn_mfma4_qg1", 1, 70, 200, None, 64)
    rows = [6, 10, 13]
    q, k, v, _, scale = R.inputs(*c, q_div=4.0 * math.sqrt(64))
    assert scale == 4.0
    kmask = R.structures(200, 64)[rows]
    q, k, v = q[rows], k[rows], v[rows]
    out = _run(c, q, k, v, kmask, None, scale)
    ref, rowscale = R.ref64(*R.operands(c[0], q, k, v), kmask, None, scale, 1)
    _check_against_ref64("E", c, out, ref, rowscale, rows)
