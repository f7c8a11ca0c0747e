"""CPU references, input builders, case tables and gates shared by tests/test_vit_front_reference.py (which pins all of this on the CPU) and
tests/test_vit_front_gpu.py (which holds every non-GEMM kernel of the ViT front end against it, per output element):

  vit_attn_kernel<T, 8> / <T, 16>, vit_attn_lds_kernel, vit_attn_cls_kernel     (vima_op_vit_attention, vima_op_vit_attention_cls)
  patchify_kernel, patchify_rect_kernel                                         (vima_op_patchify)
  vit_embed_kernel, vit_embed_rect_kernel                                       (vima_op_vit_embed)
  bbox_l1_kernel                                                                (vima_op_bbox_l1)

Every reference is fp64 and written without the kernels' index arithmetic (einsum / softmax over [M, S, heads, 32] views, reshape / permute,
torch.cat + a two-pass LayerNorm, a matmul). On a bf16 handle q | k | v are what launch_cast hands the kernel, the bf16-rounded values; the
fp32 side inputs (pre, cls, pos, g, b, the bbox weights) are read by the kernels as they are and are never rounded here.

Gates (u = 2^-8, the unit roundoff of bf16; every term derived here and measured on the CPU by test_vit_front_reference.py, none taken from
a GPU run):
  attention, fp32, regime "normal" (q, k, v ~ N(0,1))   |err| <= 1e-5 rowscale + 1e-6, rowscale = p @ |v| (attn_mask_reference.gate_of)
  attention, fp32, regime "peaked" (q x 6)              |err| <= (2 delta + 64 2^-24) rowscale + 1e-7 with delta = (D + 2) 2^-24 scale
        max_j sum_d |q_d| |k_jd| per (crop, query, head): the forward error of the fp32 dot product (D products and sums, the scaling, the
        subtraction of the maximum) moves every score by <= delta, exp carries it into every probability relatively, twice through the
        normalisation; 64 2^-24 covers expf, the sum, the reciprocal, the products and the weighted sum of <= 16 keys
  attention, bf16                                       the fp32 gate of the regime + 1.01 u |ref|: ONE rounding, at the output
  vit_embed, per row (sigma^2 the biased variance, mx = max |x| of the summed row)
        tol = 2^-23 (4 + 4 mx / sqrt(sigma^2 + 1e-5)); |err| <= tol |g_c| (|xhat_c| + 1) + 2^-23 |ref| + 1e-7   [bf16: + 1.01 u |ref|]
  patchify   |err| <= 2^-23 ((x / 255 + mean_c) / sd_c + |ref|): three correctly rounded operations                [bf16: + 1.01 u |ref|]
  bbox_l1    |err| <= 8 2^-24 S, S = sum_i |x_i| |w_i| + |b|: five roundings (the divisions by 256 / 128 are exact, relu is 1-Lipschitz)
                                                                                                                   [bf16: + 1.01 u |ref|]
No GPU and no vima_amd import here."""
import functools
import math

import torch

D = 32                              # head dim of every ViT here
SCALE = 1.0 / math.sqrt(D)
U_BF16 = 2.0 ** -8
IMG_MEAN = (0.3471, 0.3429, 0.3383)   # vit.py:9
IMG_STD = (0.3011, 0.2961, 0.2956)    # vit.py:10
EW = 768                            # width of vit_embed
PRECS = ("fp32", "bf16")


def bf(x):
    return x.bfloat16().float()


def rounded(prec, x):
    """What launch_cast hands the kernel."""
    return bf(x) if prec == "bf16" else x


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ================================================================================================================== attention
ATTN_WIDTHS = ((64, 2), (768, 24))
REGIMES = ("normal", "peaked")
PEAK = 6.0
ATTN_IMPL = {"vit_attn8": 1, "vit_attn16": 1, "vit_attn_lds": 0, "vit_attn_cls": None}   # the impl argument that reaches the kernel
# (kernel, prec, W, S, M, regime); heads = W / 32
ATTN_CASES = (
    [("vit_attn8", p, W, S, M, r) for p in PRECS for W, _ in ATTN_WIDTHS for S in (1, 2, 5, 8) for M in (1, 3, 107) for r in REGIMES] +
    [("vit_attn16", p, W, S, M, r) for p in PRECS for W, _ in ATTN_WIDTHS for S in (9, 13, 16) for M in (1, 11) for r in REGIMES] +
    [("vit_attn_lds", "bf16", 768, 5, M, r) for M in (1, 2, 3, 55) for r in REGIMES] +
    [("vit_attn_cls", p, W, S, M, r) for p in PRECS for W, _ in ATTN_WIDTHS for S in (1, 5, 8) for M in (1, 3, 107) for r in REGIMES])


def attn_case_id(c):
    k, p, W, S, M, r = c
    return f"{k}-{p}-W{W}-S{S}-M{M}-{r}"


@functools.lru_cache(maxsize=None)
def attn_inputs(W, S, M, regime, seed=0):
    """qkv fp32 [M*S, 3W] as handed to vima_op_vit_attention: iid N(0,1), so every crop, token and head has data of its own; q x 6 in the
    peaked regime (max |score| about 35, the softmax close to one-hot)."""
    qkv = torch.randn(M * S, 3 * W, generator=_gen(1, W, S, M, seed))
    if regime == "peaked":
        qkv[:, :W] *= PEAK
    else:
        assert regime == "normal"
    return qkv


def split_qkv(qkv, M, S, W):
    """[M*S, 3W] -> q, k, v views [M, S, heads, 32]."""
    x = qkv.view(M, S, 3, W // D, D)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


def cls_operands(qkv, M, S, W):
    """The arguments of vima_op_vit_attention_cls on the values of a full launch: q [M, W] = the q part of token 0, kv [M*S, 2W]."""
    return qkv.view(M, S, 3 * W)[:, 0, :W].contiguous(), qkv[:, W:].contiguous()


def attn_ref64(q, k, v, scale=SCALE):
    """q [M, Sq, H, 32], k / v [M, S, H, 32] -> (out, rowscale) fp64 [M, Sq, H, 32]; rowscale = softmax(s) @ |v|."""
    q, k, v = q.double(), k.double(), v.double()
    p = torch.softmax(torch.einsum("mihd,mjhd->mhij", q, k) * scale, dim=-1)
    return torch.einsum("mhij,mjhd->mihd", p, v), torch.einsum("mhij,mjhd->mihd", p, v.abs())


def attn_qkv_of(c):
    """q, k, v [M, Sq, H, 32] fp32 the kernel of case c computes on (Sq = 1 for the cls kernel)."""
    kern, prec, W, S, M, regime = c
    q, k, v = split_qkv(rounded(prec, attn_inputs(W, S, M, regime)), M, S, W)
    return (q[:, :1] if kern == "vit_attn_cls" else q), k, v


def attn_gate(regime, prec, q, k, ref, rowscale):
    """Per element, the shape of ref."""
    if regime == "normal":
        g = 1e-5 * rowscale + 1e-6
    else:
        delta = (D + 2) * 2.0 ** -24 * SCALE * torch.einsum("mihd,mjhd->mhij", q.double().abs(), k.double().abs()).max(dim=-1).values   # [M, H, Sq]
        g = (2 * delta.permute(0, 2, 1)[..., None] + 64 * 2.0 ** -24) * rowscale + 1e-7
    return g + 1.01 * U_BF16 * ref.abs() if prec == "bf16" else g


@functools.lru_cache(maxsize=None)
def _attn_reference(prec, W, S, M, regime, cls):
    q, k, v = attn_qkv_of(("vit_attn_cls" if cls else "vit_attn8", prec, W, S, M, regime))
    ref, rowscale = attn_ref64(q, k, v)
    return ref, rowscale, attn_gate(regime, prec, q, k, ref, rowscale)


def attn_reference(c):
    """(ref, rowscale, gate) fp64 [M, Sq, H, 32] of a case; computed once, shared (the kernels of a shape share it), never written to."""
    kern, prec, W, S, M, regime = c
    return _attn_reference(prec, W, S, M, regime, kern == "vit_attn_cls")


# ---- exact selection (test B of the GPU file): every probability is exactly 0 or 1, the output IS one V row
def select_target(M, S, H):
    """pi [M, S, H]: the key that query i of head h of crop m selects."""
    m, i, h = torch.arange(M)[:, None, None], torch.arange(S)[None, :, None], torch.arange(H)[None, None, :]
    return (19 * m + i + 17 * h) % S        # 17 and 19 are coprime to every S <= 16: neighbouring heads and crops select different keys


def select_inputs(W, S, M):
    """qkv [M*S, 3W] and the expected output [M*S, W]. Query (m, i, h) is 64 e_a with the carrier component a = (7 h + i) % 32, a different
    one for every query of a head; key j of the head holds -64 on the carrier of every query that does NOT select j and 0 on the carrier
    of those that do. Scores: 0 for the selected key, -4096 / sqrt(32) = -724 for the others, whose exp underflows to exactly 0 in fp32.
    V holds integers in [-128, 127] (exact in bf16) that differ between neighbouring crops, keys, heads and columns:
    (31 m + 17 j + 11 h + c) % 256 - 128."""
    H = W // D
    assert S <= D
    pi = select_target(M, S, H)
    q = torch.zeros(M, S, H, D)
    k = torch.zeros(M, S, H, D)
    m, i, h = torch.meshgrid(torch.arange(M), torch.arange(S), torch.arange(H), indexing="ij")
    a = (7 * h + i) % D
    q[m, i, h, a] = 64.0
    for j in range(S):
        sel = pi != j                                   # queries (m, i, h) that must not see key j
        k[m[sel], j, h[sel], a[sel]] = -64.0
    c = torch.arange(D)
    jj = torch.arange(S)
    v = ((31 * torch.arange(M)[:, None, None, None] + 17 * jj[None, :, None, None] + 11 * torch.arange(H)[None, None, :, None] + c) % 256 - 128).float()
    want = v[m, pi, h]                                  # [M, S, H, 32]
    qkv = torch.stack([q, k, v], dim=2).reshape(M * S, 3 * W)
    return qkv, want.reshape(M * S, W)


# ================================================================================================================== patchify
# (kernel, prec, H, W, P, M, impl)
PATCHIFY_CASES = [c for p in PRECS for c in (
    [("patchify", p, 32, 32, 16, M, 0) for M in (1, 3, 43)] +
    [("patchify_rect", p, 64, 128, 32, M, 0) for M in (1, 5)] +
    [("patchify_rect", p, 32, 48, 16, 2, 0), ("patchify_rect", p, 96, 64, 32, 2, 0), ("patchify_rect", p, 32, 32, 16, 3, 1)])]


def patchify_case_id(c):
    k, p, H, W, P, M, impl = c
    return f"{k}-{p}-{H}x{W}-P{P}-M{M}" + ("-forced" if impl else "")


@functools.lru_cache(maxsize=None)
def patchify_inputs(H, W, M, seed=0):
    """u8 [M, 3, H, W]: iid uniform bytes; every channel of image 0 also holds every value 0 .. 255 (at shuffled positions)."""
    g = _gen(2, H, W, M, seed)
    img = torch.randint(0, 256, (M, 3, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    for ch in range(3):
        where = torch.randperm(H * W, generator=g)[:256]
        img[0, ch].view(-1)[where] = torch.arange(256, dtype=torch.uint8)
    return img


def _img_consts():
    """mean, sd as the fp32 tensors the reference builds them as (preprocess.py:38-43), widened."""
    return (torch.tensor(IMG_MEAN, dtype=torch.float32).double().view(1, 3, 1, 1), torch.tensor(IMG_STD, dtype=torch.float32).double().view(1, 3, 1, 1))


def to_patches(x, P):
    """[M, 3, H, W] -> [M * gh * gw, 3 P P]: row = image, gy, gx; column = c, py, px (the im2col of the P x P stride-P conv)."""
    M, C, H, W = x.shape
    return x.reshape(M, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(M * (H // P) * (W // P), C * P * P)


def patchify_ref64(img, P):
    """-> (ref, gate32) fp64 [M * gh * gw, 3 P P]; gate32 is the fp32 gate, patchify_gate adds the bf16 term."""
    mean, sd = _img_consts()
    x = img.double() / 255.0
    ref = to_patches((x - mean) / sd, P)
    return ref, 2.0 ** -23 * (to_patches((x + mean) / sd, P) + ref.abs())


def with_bf16_term(prec, gate32, ref):
    return gate32 + 1.01 * U_BF16 * ref.abs() if prec == "bf16" else gate32


@functools.lru_cache(maxsize=None)
def _patchify_reference(H, W, P, M):
    return patchify_ref64(patchify_inputs(H, W, M), P)


def patchify_reference(c):
    """(ref, gate) of a case."""
    _, prec, H, W, P, M, _ = c
    ref, g32 = _patchify_reference(H, W, P, M)
    return ref, with_bf16_term(prec, g32, ref)


# ================================================================================================================== vit_embed
EMBED_REGIMES = ("plain", "offset", "lowvar")
# (kernel, prec, S, n_patch, has_cls, M, regime, impl)
EMBED_CASES = [c for p in PRECS for r in EMBED_REGIMES for c in (
    [("vit_embed", p, 5, 4, True, M, r, 0) for M in (1, 3, 51)] +
    [("vit_embed_rect", p, S, n, cl, M, r, 0) for S, n, cl in ((9, 8, True), (8, 8, False)) for M in (1, 3, 51)] +
    [("vit_embed_rect", p, 5, 4, True, 3, r, 1)])]


def embed_case_id(c):
    k, p, S, n, cl, M, r, impl = c
    return f"{k}-{p}-S{S}-n{n}-{'cls' if cl else 'nocls'}-M{M}-{r}" + ("-forced" if impl else "")


@functools.lru_cache(maxsize=None)
def embed_inputs(S, n_patch, has_cls, M, regime, seed=0):
    """pre [M * n_patch, 768], cls [768] or None, pos [S, 768], g, b [768], all fp32. plain: pre, pos, cls ~ N(0,1); offset: pos + 30 (the
    mean is 20 standard deviations of the row away from 0); lowvar: pre, pos, cls x 0.02 (the variance of a summed row is 8e-4, eps = 1e-5
    is 1.25 % of it). g ~ N(1, 0.2), b ~ N(0, 0.2) in every regime."""
    gen = _gen(3, S, n_patch, has_cls, M, seed)           # (the regimes share the draws)
    pre = torch.randn(M * n_patch, EW, generator=gen)
    cls = torch.randn(EW, generator=gen)
    pos = torch.randn(S, EW, generator=gen)
    g = 1.0 + 0.2 * torch.randn(EW, generator=gen)
    b = 0.2 * torch.randn(EW, generator=gen)
    if regime == "offset":
        pos = pos + 30.0
    elif regime == "lowvar":
        pre, cls, pos = pre * 0.02, cls * 0.02, pos * 0.02
    else:
        assert regime == "plain"
    return pre, (cls if has_cls else None), pos, g, b


def embed_tokens(pre, cls, pos, M, S, n_patch):
    """The summed rows [M, S, 768] (vit.py:176-179), in the dtype of the inputs."""
    x = pre.view(M, n_patch, EW)[:, :S - (1 if cls is not None else 0)]
    if cls is not None:
        x = torch.cat([cls.view(1, 1, EW).expand(M, 1, EW), x], dim=1)
    return x + pos


def embed_ref64(pre, cls, pos, g, b, M, S, n_patch, eps=1e-5):
    """-> (ref, gate32) fp64 [M * S, 768]: explicit two-pass LayerNorm."""
    x = embed_tokens(pre.double(), None if cls is None else cls.double(), pos.double(), M, S, n_patch).reshape(M * S, EW)
    mean = x.sum(dim=1, keepdim=True) / EW
    var = ((x - mean) ** 2).sum(dim=1, keepdim=True) / EW
    xhat = (x - mean) / torch.sqrt(var + eps)
    ref = xhat * g.double() + b.double()
    tol = 2.0 ** -23 * (4 + 4 * x.abs().max(dim=1, keepdim=True).values / torch.sqrt(var + 1e-5))
    return ref, tol * g.double().abs() * (xhat.abs() + 1) + 2.0 ** -23 * ref.abs() + 1e-7


@functools.lru_cache(maxsize=None)
def _embed_reference(S, n_patch, has_cls, M, regime):
    return embed_ref64(*embed_inputs(S, n_patch, has_cls, M, regime), M, S, n_patch)


def embed_reference(c):
    _, prec, S, n_patch, has_cls, M, regime, _ = c
    ref, g32 = _embed_reference(S, n_patch, has_cls, M, regime)
    return ref, with_bf16_term(prec, g32, ref)


# ================================================================================================================== bbox_l1
BBOX_NORM = (256.0, 128.0, 128.0, 256.0)     # obj_encoder.py:12-13, 80-85
# (prec, R, N)
BBOX_CASES = [(p, R, N) for p in PRECS for R, N in ((1, 768), (7, 768), (300, 768), (5, 36))]


def bbox_case_id(c):
    return f"bbox_l1-{c[0]}-R{c[1]}-N{c[2]}"


@functools.lru_cache(maxsize=None)
def bbox_inputs(R, N, seed=0):
    """bbox i64 [R, 4] uniform in [0, 256), from R = 3 on the last two rows all zeros and all 255; W [N, 4] ~ N(0, 1), b [N] ~ N(0, 0.5)."""
    gen = _gen(4, R, N, seed)
    bbox = torch.randint(0, 256, (R, 4), generator=gen, dtype=torch.int64)
    if R >= 3:
        bbox[-2] = 0
        bbox[-1] = 255
    return bbox, torch.randn(N, 4, generator=gen), 0.5 * torch.randn(N, generator=gen)


def bbox_ref64(bbox, W, b, norm=BBOX_NORM, relu=True):
    """-> (ref, gate32) fp64 [R, N]."""
    x = bbox.double() / torch.tensor(norm, dtype=torch.float64)
    y = x @ W.double().t() + b.double()
    return (torch.relu(y) if relu else y), 8 * 2.0 ** -24 * (x.abs() @ W.double().abs().t() + b.double().abs())


@functools.lru_cache(maxsize=None)
def _bbox_reference(R, N):
    return bbox_ref64(*bbox_inputs(R, N))


def bbox_reference(c):
    prec, R, N = c
    ref, g32 = _bbox_reference(R, N)
    return ref, with_bf16_term(prec, g32, ref)
