"""Pins tests/attn_mask_reference.py on the CPU: `ref64` against a literal fp32 restatement of the reference's three score pipelines and
against closed forms that need no softmax over masked keys, on the inputs, shapes and mask structures of tests/test_attention_masks_gpu.py."""
import pytest
import torch

from tests import attn_mask_reference as R

# one head dim per shape is enough for the reference (the kernels' head dims are a matter of tests/test_attention_masks_gpu.py);
# generic_bf16 has generic_fp32's inputs
REF_CASES = [c for c in R.CASES if c[5] == R.KERNELS[c[0]][4][-1] and c[0] != "generic_bf16"]


def attn_ref32(q, k, v, kmask, relbias, scale, mode, q_off=0, win=None):
    """`attn_ref` (tests/test_ops_gpu.py) and `attn_ref_window` (tests/test_rollout_gpu.py) in one: fp32, the mask as the ADD (1 - mask) * finfo.min,
    the causal fill as w * b + -1e4 * (1 - b)."""
    Lq, Lk = q.shape[1], k.shape[1]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k)
    madd = (1.0 - kmask[:, None, None, :].float()) * R.FMIN
    if mode == 0:
        idx = (torch.arange(Lk)[None, :] - torch.arange(Lq)[:, None]) + Lk - 1
        s = s + (relbias[:, idx][None] + madd)
    elif mode == 1:
        s = s * scale + madd
    else:
        tri = (~R.future(Lq, Lk, q_off, win)).float()
        s = (s * scale) * tri + -1e4 * (1 - tri)
        s = s + madd
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v)


def _case(c):
    name, mode, Lq, Lk, q_off, D = c
    q, k, v, relbias, scale = R.inputs(*c)
    q, k, v = R.operands(name, q, k, v)
    kmask = R.structures(Lk, R.KERNELS[name][3])
    win = None if q_off is None else q_off + Lq
    return q, k, v, kmask, relbias, scale, mode, (q_off or 0), win


def test_structures_are_what_the_table_says():
    for Lk, T in ((40, 32), (72, 32), (200, 64), (260, 64), (300, 128)):
        m = R.structures(Lk, T)
        assert m.shape == (15, Lk) and m.dtype == torch.bool
        assert m[0].all() and not m[13].any()
        assert [int(m[i].sum()) for i in range(1, 6)] == [1, T - 1, T, T + 1, Lk - 1]
        assert all(bool(m[i, :int(m[i].sum())].all()) for i in range(1, 6))                   # prefixes
        assert [int(m[i].sum()) for i in R.SUFFIXES] == [Lk - 1, Lk - T, Lk - T - 1, 1]
        assert all(bool(m[i, Lk - int(m[i].sum()):].all()) and not bool(m[i, 0]) for i in R.SUFFIXES)
        assert not m[7, :T].any() and not m[8, :T].any() and not m[9, :T].any()              # a dead first tile
        assert m[10, :T].all() and not m[10, T:2 * T].any() and m[10, 2 * T:].all()
        assert sorted((~m[11]).nonzero().flatten().tolist()) == sorted({x for x in (0, 31, 32, 63, T, Lk - 1) if x < Lk})
        assert m[12].nonzero().flatten().tolist() == [Lk - 1]
        assert bool(m[14, 0]) and 0.6 < m[14].float().mean() < 0.95
        assert torch.equal(m, R.structures(Lk, T))                                           # seeded


@pytest.mark.parametrize("c", REF_CASES, ids=R.case_id)
def test_ref64_against_the_literal_fp32_pipeline_and_closed_forms(c):
    q, k, v, kmask, relbias, scale, mode, q_off, win = _case(c)
    out, rowscale = R.ref64(q, k, v, kmask, relbias, scale, mode, q_off, win)
    assert out.dtype == torch.float64 and torch.isfinite(out).all() and torch.isfinite(rowscale).all()
    assert (out.abs() <= rowscale * (1 + 1e-12)).all()
    # the literal fp32 pipeline, per element
    r32 = attn_ref32(q, k, v, kmask, relbias, scale, mode, q_off, win)
    assert torch.isfinite(r32).all()
    rel = ((r32.double() - out).abs() / rowscale).max().item()
    print(f"[attn-mask ref] {R.case_id(c)}: fp32 attn_ref vs ref64, worst err / rowscale {rel:.2e} (bound 1e-5)")
    assert rel <= 1e-5
    # nothing valid: uniform over exactly the Lk keys, in every mode (the future keys of the causal mode are masked as well)
    err13 = (out[R.NOTHING] - v[R.NOTHING].double().mean(dim=0)[None]).abs().max().item()
    assert err13 <= 1e-12, err13
    if mode == 1:
        # cross mode: attention over the gathered valid keys, without any mask
        for b in range(R.N_STRUCT):
            if b == R.NOTHING:
                continue
            sel = kmask[b]
            o, _ = R.ref64(q[b:b + 1], k[b:b + 1, sel], v[b:b + 1, sel], None, None, scale, 1)
            assert (o[0] - out[b]).abs().max().item() <= 1e-12, b
    if mode == 2:
        # a query without a valid visible key that is not future attends uniformly to the valid future keys of its window (at the literal -1e4)
        fut = R.future(q.shape[1], k.shape[1], q_off, win)
        checked = set()
        for b in range(R.N_STRUCT):
            for i in range(q.shape[1]):
                past, ahead = kmask[b] & ~fut[i], kmask[b] & fut[i]
                if not past.any() and ahead.any():
                    want = v[b, ahead].double().mean(dim=0)
                    assert (out[b, i] - want).abs().max().item() <= 1e-12, (b, i)
                    checked.add((b, i))
        if win is None:
            assert (6, 0) in checked      # key 0 masked: query 0 of the plain causal rule has no past at all
