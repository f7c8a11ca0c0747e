"""Pins tests/vit_front_reference.py on the CPU: every fp64 reference against an independent torch form, every gate against a torch fp32
restatement of the operation (it must stay well inside: the gates are derived, not fitted), every gate against the mutations it is there to
catch (each must land more than 10x beyond it), and the five operator entry points of tests/test_vit_front_gpu.py against header and binding."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import vit_front_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEETH = 10.0
_worst = {}


def _note(family, ratio, cid):
    if ratio > _worst.get(family, (-1.0, ""))[0]:
        _worst[family] = (ratio, cid)


def _dedup(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


# the kernels of one shape share operands, reference and gate: one case per (precision, shape, regime) is enough on the CPU
ATTN = _dedup(R.ATTN_CASES, lambda c: (c[0] == "vit_attn_cls",) + c[1:])
PATCH = _dedup(R.PATCHIFY_CASES, lambda c: c[1:6])
EMBED = _dedup(R.EMBED_CASES, lambda c: c[1:7])


def _gate32(prec, gate, ref):
    return gate - 1.01 * R.U_BF16 * ref.abs() if prec == "bf16" else gate


def _restatement(family, cid, prec, r32, ref, gate):
    """The fp32 restatement under 0.5 of the fp32 gate; on a bf16 case its bf16 rounding under 1.0 of the bf16 gate."""
    assert r32.dtype == torch.float32 and torch.isfinite(r32).all()
    a = ((r32.double() - ref).abs() / _gate32(prec, gate, ref)).max().item()
    _note(family + " fp32 restatement / fp32 gate", a, cid)
    assert a < 0.5, f"{cid}: fp32 restatement at {a:.3f} of the fp32 gate"
    if prec == "bf16":
        b = ((R.bf(r32).double() - ref).abs() / gate).max().item()
        _note(family + " bf16(restatement) / bf16 gate", b, cid)
        assert b < 1.0, f"{cid}: bf16-rounded restatement at {b:.3f} of the bf16 gate"


def _teeth(cid, name, mut, ref, gate):
    assert mut.shape == ref.shape
    r = ((mut - ref).abs() / gate).max().item()
    assert r > TEETH, f"{cid}: mutation '{name}' reaches only {r:.2f} x the gate"


# ================================================================================================================== attention
@pytest.mark.parametrize("c", [c for c in ATTN if c[1] == "fp32" and c[5] == "normal" and c[4] in (1, 3, 11)], ids=R.attn_case_id)
def test_attention_ref64_against_independent_forms(c):
    kern, prec, W, S, M, regime = c
    q, k, v = R.attn_qkv_of(c)
    ref, rowscale = R.attn_ref64(q, k, v)
    assert ref.dtype == torch.float64 and (ref.abs() <= rowscale * (1 + 1e-12)).all()
    sdpa = F.scaled_dot_product_attention(q.double().transpose(1, 2), k.double().transpose(1, 2), v.double().transpose(1, 2)).transpose(1, 2)
    assert (sdpa - ref).abs().max().item() <= 1e-12
    if kern != "vit_attn_cls":
        # OraclePolicy._vit's own lines on the packed projection output
        heads, d = W // 32, 32
        qq, kk, vv = R.attn_inputs(W, S, M, regime).double().view(M, S, 3 * W).split(W, dim=-1)
        qq = qq.view(M, -1, heads, d).transpose(1, 2)
        kk = kk.view(M, -1, heads, d).transpose(1, 2)
        vv = vv.view(M, -1, heads, d).transpose(1, 2)
        att = torch.softmax(qq @ kk.transpose(-1, -2) / math.sqrt(d), dim=-1) @ vv
        assert (att.transpose(1, 2).reshape(M * S, W) - ref.reshape(M * S, W)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("c", ATTN, ids=R.attn_case_id)
def test_attention_gate_holds_the_fp32_restatement(c):
    kern, prec, W, S, M, regime = c
    q, k, v = R.attn_qkv_of(c)
    ref, _, gate = R.attn_reference(c)
    r32 = (torch.softmax(q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2) / math.sqrt(32), dim=-1) @ v.transpose(1, 2)).transpose(1, 2)
    _restatement(f"attention {regime}", R.attn_case_id(c), prec, r32, ref, gate)


def _attn_mutations(c, q, k, v):
    """name -> mutated output, the mutations that can show on this case. The phantom key has score 0: next to scores of O(1) it takes an O(1)
    share of every row, next to a peaked row's maximum of ~35 it weighs e^-35 and is rightly invisible -- normal regime only."""
    kern, prec, W, S, M, regime = c
    H = W // 32
    out = {}
    if S >= 2:
        out["scale 1/sqrt(64)"] = R.attn_ref64(q, k, v, scale=1.0 / 8.0)[0]
        # dropping a key shows on the rows that give it weight: a near one-hot row that selects another key rightly does not move. It applies
        # where some row gives the last key 1 % (the few-row launches of the cls kernel in the peaked regime may have none)
        p_last = torch.softmax(torch.einsum("mihd,mjhd->mhij", q.double(), k.double()) * R.SCALE, dim=-1)[..., -1].max().item()
        assert p_last >= 0.01 or (regime == "peaked" and kern == "vit_attn_cls" and M <= 3), p_last
        if p_last >= 0.01:
            out["last key dropped"] = R.attn_ref64(q, k[:, :-1], v[:, :-1])[0]
    if regime == "normal":
        z = torch.zeros_like(k[:, :1])
        out["phantom zero-score key"] = R.attn_ref64(q, torch.cat([k, z], dim=1), torch.cat([v, z], dim=1))[0]
    out["V of heads h, h ^ 1 swapped"] = R.attn_ref64(q, k, v[:, :, torch.arange(H) ^ 1])[0]
    out["V chunks rotated inside the head"] = R.attn_ref64(q, k, v.reshape(*v.shape[:-1], 4, 8).roll(1, dims=-2).reshape(v.shape))[0]
    if M >= 2:
        other = torch.arange(M) ^ 1
        other = torch.where(other < M, other, torch.arange(M))
        out["crop m reads the keys of crop m ^ 1"] = R.attn_ref64(q, k[other], v[other])[0]
    return out


@pytest.mark.parametrize("c", ATTN, ids=R.attn_case_id)
def test_attention_gate_has_teeth(c):
    q, k, v = R.attn_qkv_of(c)
    ref, _, gate = R.attn_reference(c)
    muts = _attn_mutations(c, q, k, v)
    assert len(muts) >= 2
    for name, mut in muts.items():
        _teeth(R.attn_case_id(c), name, mut, ref, gate)


@pytest.mark.parametrize("W,S,M", [(64, 1, 3), (64, 5, 3), (768, 5, 55), (768, 8, 3), (64, 13, 11), (768, 16, 2)])
def test_exact_selection_inputs_select_exactly(W, S, M):
    """The inputs of the GPU file's test B: in fp32 every probability is exactly 0 or 1 and the output is the selected V row, bit for bit;
    every value is exact in bf16; each key is selected by some query and the targets differ between heads and crops."""
    qkv, want = R.select_inputs(W, S, M)
    assert torch.equal(R.bf(qkv), qkv) and torch.equal(R.bf(want), want)
    q, k, v = R.split_qkv(qkv, M, S, W)
    s = torch.einsum("mihd,mjhd->mhij", q, k) * torch.tensor(R.SCALE, dtype=torch.float32)
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    assert set(p.unique().tolist()) <= {0.0, 1.0} and torch.equal(p.sum(dim=-1), torch.ones_like(p[..., 0]))
    assert torch.equal(torch.einsum("mhij,mjhd->mihd", p, v).reshape(M * S, W), want)
    assert (R.attn_ref64(q, k, v)[0].reshape(M * S, W) - want).abs().max().item() < 1e-300
    pi = R.select_target(M, S, W // 32)
    assert set(pi.unique().tolist()) == set(range(S))
    if S > 1:
        assert not torch.equal(pi[:, :, 0], pi[:, :, 1]) and (M == 1 or not torch.equal(pi[0], pi[1]))
        # a kernel whose q and k chunks disagree sees only zero scores and returns the mean of V, which is not the target
        assert not torch.equal(v.mean(dim=1, keepdim=True).expand_as(v).reshape(M * S, W), want)


# ================================================================================================================== patchify
@pytest.mark.parametrize("c", [c for c in PATCH if c[1] == "fp32" and c[5] <= 3], ids=R.patchify_case_id)
def test_patchify_ref64_against_conv2d_with_an_identity_basis(c):
    _, _, H, W, P, M, _ = c
    img = R.patchify_inputs(H, W, M)
    ref, _ = R.patchify_ref64(img, P)
    mean = torch.tensor(R.IMG_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(R.IMG_STD, dtype=torch.float32).view(1, 3, 1, 1)
    x = (img.double() / 255.0 - mean.double()) / std.double()                     # OraclePolicy._vit's line, in fp64
    n = 3 * P * P
    y = F.conv2d(x, torch.eye(n, dtype=torch.float64).view(n, 3, P, P), None, stride=P)   # [M, n, gh, gw]
    assert (y.permute(0, 2, 3, 1).reshape(-1, n) - ref).abs().max().item() <= 1e-12
    assert (F.unfold(x, P, stride=P).transpose(1, 2).reshape(-1, n) - ref).abs().max().item() <= 1e-12


def test_patchify_inputs_hold_every_byte_value():
    for _, _, H, W, P, M, _ in PATCH:
        img = R.patchify_inputs(H, W, M)
        assert img.dtype == torch.uint8 and all(len(img[0, ch].unique()) == 256 for ch in range(3))


def _patchify32(img, P, mean=R.IMG_MEAN):
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(R.IMG_STD, dtype=torch.float32).view(1, 3, 1, 1)
    return R.to_patches((img.float() / 255.0 - m) / s, P)


@pytest.mark.parametrize("c", PATCH, ids=R.patchify_case_id)
def test_patchify_gate_holds_the_fp32_restatement_and_has_teeth(c):
    _, prec, H, W, P, M, _ = c
    cid = R.patchify_case_id(c)
    img = R.patchify_inputs(H, W, M)
    ref, gate = R.patchify_reference(c)
    _restatement("patchify", cid, prec, _patchify32(img, P), ref, gate)
    mean, sd = (t.double() for t in (torch.tensor(R.IMG_MEAN, dtype=torch.float32), torch.tensor(R.IMG_STD, dtype=torch.float32)))
    x = (img.double() / 255.0 - mean.view(1, 3, 1, 1)) / sd.view(1, 3, 1, 1)
    gh, gw = H // P, W // P
    _teeth(cid, "gx / gy swapped", x.reshape(M, 3, gh, P, gw, P).permute(0, 4, 2, 1, 3, 5).reshape(ref.shape), ref, gate)
    _teeth(cid, "py / px transposed", x.reshape(M, 3, gh, P, gw, P).permute(0, 2, 4, 1, 5, 3).reshape(ref.shape), ref, gate)
    xm = (img.double() / 255.0 - mean[[1, 0, 2]].view(1, 3, 1, 1)) / sd.view(1, 3, 1, 1)
    _teeth(cid, "means of channels 0 and 1 swapped", R.to_patches(xm, P), ref, gate)


def test_patchify_gate_at_every_byte_value():
    """All 256 byte values in every channel, alone: the ratio the gate's constant rests on."""
    img = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).expand(1, 3, 16, 16).contiguous()
    ref, g32 = R.patchify_ref64(img, 16)
    r32 = _patchify32(img, 16)
    a = ((r32.double() - ref).abs() / g32).max().item()
    b = ((R.bf(r32).double() - ref).abs() / R.with_bf16_term("bf16", g32, ref)).max().item()
    _note("patchify, all 256 bytes: fp32 restatement / fp32 gate", a, "1x3x16x16")
    _note("patchify, all 256 bytes: bf16(restatement) / bf16 gate", b, "1x3x16x16")
    assert a < 0.5 and b < 1.0, (a, b)


# ================================================================================================================== vit_embed
@pytest.mark.parametrize("c", [c for c in EMBED if c[1] == "fp32" and c[5] <= 3], ids=R.embed_case_id)
def test_embed_ref64_against_layer_norm(c):
    _, _, S, n, has_cls, M, regime, _ = c
    pre, cls, pos, g, b = R.embed_inputs(S, n, has_cls, M, regime)
    ref, _ = R.embed_ref64(pre, cls, pos, g, b, M, S, n)
    x = pre.double().view(M, n, R.EW)
    if has_cls:
        x = torch.cat([cls.double().view(1, 1, -1).expand(M, 1, -1), x], dim=1) + pos.double()          # OraclePolicy._vit's lines
    else:
        x = x + pos.double()
    want = F.layer_norm(x, (R.EW,), g.double(), b.double(), 1e-5).reshape(M * S, R.EW)
    assert (want - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("c", EMBED, ids=R.embed_case_id)
def test_embed_gate_holds_the_fp32_restatement_and_has_teeth(c):
    _, prec, S, n, has_cls, M, regime, _ = c
    cid = R.embed_case_id(c)
    pre, cls, pos, g, b = R.embed_inputs(S, n, has_cls, M, regime)
    ref, gate = R.embed_reference(c)
    r32 = F.layer_norm(R.embed_tokens(pre, cls, pos, M, S, n), (R.EW,), g, b, 1e-5).reshape(M * S, R.EW)
    _restatement(f"vit_embed {regime}", cid, prec, r32, ref, gate)
    _teeth(cid, "pos[t + 1] instead of pos[t]", R.embed_ref64(pre, cls, pos.roll(-1, dims=0), g, b, M, S, n)[0], ref, gate)
    if has_cls:
        shifted = pre.view(M, n, R.EW).roll(-1, dims=1).reshape(M * n, R.EW)
        _teeth(cid, "patch t instead of t - 1", R.embed_ref64(shifted, cls, pos, g, b, M, S, n)[0], ref, gate)
        every = pos.clone()
        every[1:] += cls
        _teeth(cid, "cls added on every row", R.embed_ref64(pre, cls, every, g, b, M, S, n)[0], ref, gate)
    if regime == "lowvar":
        _teeth(cid, "eps 1e-6", R.embed_ref64(pre, cls, pos, g, b, M, S, n, eps=1e-6)[0], ref, gate)


@pytest.mark.parametrize("offset", [0.0, 1.0, 30.0, 1000.0])
@pytest.mark.parametrize("sigma", [1e-3, 0.02, 1.0])
def test_embed_gate_over_offsets_and_variances(offset, sigma):
    """Rows N(offset, sigma^2), beyond the regimes of the case table: the ratio the gate's tol rests on."""
    gen = torch.Generator().manual_seed(int(offset) * 7 + int(sigma * 1000))
    pre = torch.randn(8, R.EW, generator=gen) * sigma
    pos = torch.zeros(8, R.EW) + offset
    g, b = 1.0 + 0.2 * torch.randn(R.EW, generator=gen), 0.2 * torch.randn(R.EW, generator=gen)
    ref, g32 = R.embed_ref64(pre, None, pos, g, b, 1, 8, 8)
    r32 = F.layer_norm(pre + pos, (R.EW,), g, b, 1e-5)
    a = ((r32.double() - ref).abs() / g32).max().item()
    _note("vit_embed, offsets 0 .. 1000, sigma 1e-3 .. 1: fp32 restatement / fp32 gate", a, f"offset {offset} sigma {sigma}")
    assert a < 0.5, a


# ================================================================================================================== bbox_l1
@pytest.mark.parametrize("c", R.BBOX_CASES, ids=R.bbox_case_id)
def test_bbox_reference_gate_and_teeth(c):
    prec, Rn, N = c
    cid = R.bbox_case_id(c)
    bbox, W, b = R.bbox_inputs(Rn, N)
    assert bbox.dtype == torch.int64 and 0 <= bbox.min() and bbox.max() <= 255
    if Rn >= 3:
        assert (bbox[-2] == 0).all() and (bbox[-1] == 255).all()
    ref, gate = R.bbox_reference(c)
    norm = torch.tensor([256.0, 128.0, 128.0, 256.0])                                             # OraclePolicy.obj_encoder's lines
    want = torch.relu(F.linear(bbox.double() / norm.double(), W.double(), b.double()))
    assert (want - ref).abs().max().item() <= 1e-12
    _restatement("bbox_l1", cid, prec, torch.relu(F.linear(bbox.float() / norm, W, b)), ref, gate)
    _teeth(cid, "divisors [256, 256, 128, 128]", R.bbox_ref64(bbox, W, b, norm=(256.0, 256.0, 128.0, 128.0))[0], ref, gate)
    _teeth(cid, "relu dropped", R.bbox_ref64(bbox, W, b, relu=False)[0], ref, gate)
    _teeth(cid, "W indexed transposed", R.bbox_ref64(bbox, W.flatten().view(4, N).t(), b)[0], ref, gate)


# ================================================================================================================== tables, binding
def test_case_tables_hold_what_the_gpu_file_needs():
    assert {c[0] for c in R.ATTN_CASES} == set(R.ATTN_IMPL)
    assert {c[0] for c in R.PATCHIFY_CASES} == {"patchify", "patchify_rect"} and {c[0] for c in R.EMBED_CASES} == {"vit_embed", "vit_embed_rect"}
    for cases, cid in ((R.ATTN_CASES, R.attn_case_id), (R.PATCHIFY_CASES, R.patchify_case_id), (R.EMBED_CASES, R.embed_case_id), (R.BBOX_CASES, R.bbox_case_id)):
        assert len({cid(c) for c in cases}) == len(cases)
        assert {c[1] if cases is not R.BBOX_CASES else c[0] for c in cases} == set(R.PRECS)
    assert all(c[1:4] == ("bf16", 768, 5) for c in R.ATTN_CASES if c[0] == "vit_attn_lds")
    assert {c[4] for c in R.ATTN_CASES if c[0] == "vit_attn_lds"} == {1, 2, 3, 55}
    assert 107 * 5 * 24 % 256 and 107 * 24 % 256                      # partial last workgroups of the register and cls kernels


VIT_OPS = {"vima_op_vit_attention": 9, "vima_op_vit_attention_cls": 9, "vima_op_patchify": 9, "vima_op_vit_embed": 12, "vima_op_bbox_l1": 8}


def test_header_library_and_binding_agree_on_the_vit_front_entry_points():
    from vima_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vima_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in VIT_OPS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} not declared in include/vima_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == nargs and params[0] == "VimaHandle* h" and params[-1] == "vima_stream_t stream" and params[-2] == "float* out"
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.ctypes.c_int and len(args) == nargs
        for p, a in zip(params, args):
            assert (a is _lib.ctypes.c_int) == p.startswith("int "), (name, p)
            assert (a is _lib.vp) == ("*" in p or p.startswith("vima_stream_t")), (name, p)
        assert hasattr(lib, name)
    assert lib.vima_abi_version() == _lib.ABI_VERSION == 5


def test_zz_print_the_worst_ratios():
    """Last in the file: the CPU-measured ratios the gates rest on (profiles/vit_front_errors.txt records them)."""
    for family in sorted(_worst):
        ratio, cid = _worst[family]
        print(f"[vit-front ref] {family}: worst {ratio:.3f} at {cid}")
