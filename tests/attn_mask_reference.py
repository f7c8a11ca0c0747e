"""CPU reference, key-mask structures and the case table shared by tests/test_attn_mask_reference.py (which pins the reference itself)
and tests/test_attention_masks_gpu.py (which holds every attention kernel against it, per output element).

`ref64` is the fp64 form of `attn_ref` (tests/test_ops_gpu.py) and `attn_ref_window` (tests/test_rollout_gpu.py): a masked key's score IS
finfo(float32).min (torch.where, not an add: in fp32 the fill absorbs the score, in fp64 it would not), the causal fill is the literal -1e4.
`structures` builds one key mask per sample, so that all structures share one launch. No GPU and no vima_amd import here."""
import functools
import math

import torch

FMIN = torch.finfo(torch.float32).min
H = 2
N_STRUCT = 15
ALL_VALID, HOLE, SINGLES, ONLY_LAST, NOTHING, IID = 0, 10, 11, 12, 13, 14
SUFFIXES = (6, 7, 8, 9)


def future(Lq, Lk, q_off=0, win=None):
    """[Lq, Lk] bool: key j is "future" for query i (which sits at position i + q_off) iff i + q_off < j < win. win = None is the plain causal
    rule (the window ends with the keys); vima_op_attention_window has win = q_off + Lq, the rows behind it hold older, visible history."""
    win = Lk if win is None else win
    i = torch.arange(Lq)[:, None] + q_off
    j = torch.arange(Lk)[None, :]
    return (j > i) & (j < win)


def ref64(q, k, v, kmask, relbias, scale, mode, q_off=0, win=None):
    """q [B, Lq, H, D], k / v [B, Lk, H, D], kmask [B, Lk] bool or None, relbias [H, 2 Lk - 1] (mode 0), mode 0 T5 / 1 cross / 2 causal.
    -> (out, rowscale) in fp64, both [B, Lq, H, D]; rowscale = softmax(s) @ |v|, the magnitude an output element's error is measured against."""
    q, k, v = q.double(), k.double(), v.double()
    Lq, Lk = q.shape[1], k.shape[1]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k)
    if mode == 0:
        idx = (torch.arange(Lk)[None, :] - torch.arange(Lq)[:, None]) + Lk - 1
        s = s + relbias.double()[:, idx][None]
    elif mode == 1:
        s = s * scale
    else:
        s = torch.where(future(Lq, Lk, q_off, win)[None, None], -1e4, s * scale)
    if kmask is not None:
        s = torch.where(kmask[:, None, None, :], s, FMIN)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v), torch.einsum("bhqk,bkhd->bqhd", p, v.abs())


def structures(Lk, T):
    """[15, Lk] bool, True = valid key, for key-tile size T (ranges are cut to [0, Lk)):
      0      all valid
      1-5    valid prefix of length n = 1, T-1, T, T+1, Lk-1
      6-9    valid suffix starting at n = 1, T, T+1, Lk-1 (key 0 masked; from n = T on the whole first tile is masked)
      10     hole: keys [T, 2T) masked (clean tile, dead tile, clean tile)
      11     single masked keys 0, 31, 32, 63, T, Lk-1 (sub-tile and lane-half boundaries)
      12     only key Lk-1 valid
      13     nothing valid
      14     iid 80 % with key 0 valid (seeded): the regime of the op-level tests"""
    j = torch.arange(Lk)
    rows = [torch.ones(Lk, dtype=torch.bool)]
    rows += [j < n for n in (1, T - 1, T, T + 1, Lk - 1)]
    rows += [j >= n for n in (1, T, T + 1, Lk - 1)]
    rows.append(~((j >= T) & (j < 2 * T)))
    single = torch.ones(Lk, dtype=torch.bool)
    single[[x for x in (0, 31, 32, 63, T, Lk - 1) if 0 <= x < Lk]] = False
    rows.append(single)
    rows.append(j == Lk - 1)
    rows.append(torch.zeros(Lk, dtype=torch.bool))
    iid = torch.rand(Lk, generator=torch.Generator().manual_seed(7919 * Lk + T)) > 0.2
    iid[0] = True
    rows.append(iid)
    m = torch.stack(rows)
    assert m.shape == (N_STRUCT, Lk)
    return m


# ---------------------------------------------------------------------------------------------- the cases
# kernel -> (precision of the handle, impl, options, key tile T, head dims, [(mode, Lq, Lk, q_off)]); q_off None = the plain entry point
# (vima_op_attention), a number = vima_op_attention_window (causal, window [q_off, q_off + Lq)).
_ONE_WAVE = [(0, 40, 72, None), (1, 40, 72, None), (1, 40, 200, None), (2, 40, 40, None)]
KERNELS = {
    "generic_fp32": ("fp32", 0, {}, 32, (16, 64), [(0, 40, 72, None), (1, 40, 72, None), (2, 40, 72, None)]),
    "generic_bf16": ("bf16", 0, {}, 32, (16, 64), [(0, 40, 72, None), (1, 40, 72, None), (2, 40, 72, None)]),
    "attn_mfma": ("bf16", 1, {"attn4_min_lq": 64}, 32, (32, 64), _ONE_WAVE),
    "attn_x3": ("bf16x3", 1, {}, 32, (32, 64), _ONE_WAVE),
    "attn_mfma4_qg1": ("bf16", 1, {"attn4_min_lq": 64, "attn_qg": 1}, 64, (32, 64), [(0, 70, 200, None), (1, 70, 200, None), (2, 200, 200, None)]),
    "attn_mfma4_qg2": ("bf16", 1, {"attn4_min_lq": 64, "attn_qg": 2}, 64, (32, 64), [(0, 260, 260, None), (1, 260, 200, None)]),
    "attn_split": ("bf16", 1, {"attn4_min_lq": 64}, 128, (32, 64), [(1, 8, 300, None), (2, 8, 300, 0), (2, 8, 300, 120), (2, 8, 300, 292)]),
}
CASES = [(name, mode, Lq, Lk, q_off, D) for name, (_, _, _, _, dims, shapes) in KERNELS.items() for (mode, Lq, Lk, q_off) in shapes for D in dims]
U_BF16 = 2.0 ** -8          # unit roundoff of bfloat16


def case_id(c):
    name, mode, Lq, Lk, q_off, D = c
    return f"{name}-mode{mode}-{Lq}x{Lk}" + ("" if q_off is None else f"-off{q_off}") + f"-D{D}"


def gate_of(name):
    """(relative to rowscale, absolute). bf16: 3 u of sum p |v| -- the flash kernels round the probabilities (<= u sum p |v|), round the output
    (<= u |out|) and, in attn_mfma4 / attn_split, normalise by the sum of the unrounded probabilities (<= u |out|); fp32: the project's 1e-5,
    per element; bf16x3: 2e-5 absolute on inputs uniform in [-1, 1] (test_attention_split_bf16_against_fp64's bound)."""
    prec = KERNELS[name][0]
    if prec == "bf16":
        return 3 * U_BF16, 1e-6
    if prec == "fp32":
        return 1e-5, 1e-6
    return 0.0, 2e-5


@functools.lru_cache(maxsize=None)
def inputs(name, mode, Lq, Lk, q_off, D, seed=0, q_div=1.0):
    """q, k, v (fp32, as handed to the entry point), relbias, scale. q, k scaled as in test_attention (0.4 in T5 mode, which has no 1/sqrt(d));
    bf16x3: uniform in [-1, 1]. B = 15, one sample per structure. q_div: Test E divides q by it and multiplies the scale."""
    B = N_STRUCT
    g = torch.Generator().manual_seed(100000 * seed + 10000 * mode + 1000 * (D // 16) + Lq + Lk + (0 if q_off is None else q_off))
    if KERNELS[name][0] == "bf16x3":
        q, k, v = (torch.rand(B, L, H, D, generator=g) * 2 - 1 for L in (Lq, Lk, Lk))
    else:
        sc = 1.0 if mode else 0.4
        q = torch.randn(B, Lq, H, D, generator=g) * sc
        k = torch.randn(B, Lk, H, D, generator=g) * sc
        v = torch.randn(B, Lk, H, D, generator=g)
    relbias = torch.randn(H, 2 * Lk - 1, generator=g) if mode == 0 else None
    scale = 1.0 if mode == 0 else 1.0 / math.sqrt(D)
    return q / q_div, k, v, relbias, scale * q_div


def bf(x):
    return x.bfloat16().float()


def operands(name, q, k, v):
    """What the kernel computes on: the bf16-rounded inputs on a bf16 handle, the raw ones on fp32 / bf16x3 handles."""
    return (bf(q), bf(k), bf(v)) if KERNELS[name][0] == "bf16" else (q, k, v)


@functools.lru_cache(maxsize=None)
def reference(name, mode, Lq, Lk, q_off, D):
    """(out, rowscale) of ref64 for a case with the structures as its key masks; computed once, shared, never written to."""
    q, k, v, relbias, scale = inputs(name, mode, Lq, Lk, q_off, D)
    kmask = structures(Lk, KERNELS[name][3])
    win = None if q_off is None else q_off + Lq
    return ref64(*operands(name, q, k, v), kmask, relbias, scale, mode, q_off or 0, win)
