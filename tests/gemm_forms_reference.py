"""fp64 references of the structured launch forms of launch_gemm (GemmArgs, vima_amd/csrc/kernels.h), their cases, and ONE checker.

Plain torch on the CPU. A `Case` names a form at one geometry; `make_inputs` draws its operands (padding poisoned), `expected`
returns, for EVERY output buffer, the fp64 image of the whole allocation (guard bands, padding columns, skipped rows included),
a per-element error bound and the written set; `check` holds a launch's buffers against them:

    inside the written set   finite and |out - ref| <= bound, element by element
    outside it               bit-equal to the canary the buffer was filled with

Rounding points are the ones kernels.h declares, and only those: operands are bf16 values (bf16 mode), the GEGLU gate is stored in
bf16 before the multiply, the statistics come from the final fp32 values (with out32) or from the stored bf16 values (outT only),
the output is rounded once where it is bf16. The reference itself is unrounded fp64 of the rounded OPERANDS; every rounding point
appears as a term of the bound (2^-8 |value| per bf16 rounding, 2^-24 |value| per fp32 operation), next to the accumulation term
C_ACC * 2^-24 * S with S = sum_k |a_k| |w_k| (+ |bias|), carried through the epilogue by the activation's Lipschitz constant and
|mul| / |gate|. C_ACC and the activation terms are MEASURED on the CPU (measure_c / measure_act_error, pinned by
tests/test_gemm_forms_reference.py, recorded in profiles/gemm_form_errors.txt), never taken from what the GPU gives.
"""
import math

import torch

U24 = 2.0 ** -24          # fp32 unit roundoff
UBF = 2.0 ** -8           # bf16 unit roundoff: 8 significant bits, round to nearest is off by up to 2^-8 |value| / (1 + 2^-8)
CANARY = -24576.0         # bf16-exact sentinel every output buffer is filled with
GUARD = 512               # guard band (elements) at both ends of every output buffer
# accumulation constant: 4 x the worst measured ratio (CPU fp32 matmul and a 16-wide exact-block fp32 chain, against fp64, in units
# of 2^-24 S) over the cases' own operands -- the factor 4 for the unknown order inside the matrix instruction -- rounded up to a
# whole number. Measured over every case shape (tests/test_gemm_forms_reference.py asserts it): worst 3.36, from the fp32 matmul; the block
# chain stays below 1.6. 4 x 3.36 = 13.4.
C_ACC = 14.0
X3_REL = 3e-5             # precision bf16x3: the per-GEMM bound of tests/test_bf16x3_gpu.py (error / sum_k |a_k w_k|), unchanged
LIPSCHITZ = {0: 1.0, 1: 1.0, 2: 1.13, 3: 1.10}   # sup |act'|: GELU 1.129, x sigmoid(1.702 x) 1.0998
# error of evaluating the activation's formula as written in common.h, fp32 against fp64 over [-8, 8], per max(|v|, 1): 4 x measured
ACT_ERR = {("bf16", 2): 4 * 1.8e-7, ("fp32", 2): 4 * 1.1e-7, ("bf16", 3): 4 * 1.5e-7, ("fp32", 3): 4 * 1.5e-7}   # measured 1.79e-7, 1.06e-7, 1.42e-7
ACT_NONE, ACT_RELU, ACT_GELU, ACT_QUICKGELU = 0, 1, 2, 3


def act64(v, act):
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))
    if act == ACT_QUICKGELU:
        return v * torch.sigmoid(1.702 * v)
    return v


def act_formula_fp32(v, act, bf16_kernel):
    """The activation as common.h writes it, evaluated in fp32 on the CPU (v: fp32 tensor)."""
    f = torch.float32
    if act == ACT_GELU and bf16_kernel:   # gelu_erf_bf16: Abramowitz-Stegun 7.1.26
        x = v.abs() * torch.tensor(0.70710678118654752440, dtype=f)
        t = 1.0 / (torch.tensor(0.3275911, dtype=f) * x + 1.0)
        q = torch.tensor(1.061405429, dtype=f) * t + torch.tensor(-1.453152027, dtype=f)
        q = q * t + torch.tensor(1.421413741, dtype=f)
        q = q * t + torch.tensor(-0.284496736, dtype=f)
        q = q * t + torch.tensor(0.254829592, dtype=f)
        e = (q * t) * torch.exp2((x * x) * torch.tensor(-1.44269504088896340736, dtype=f))
        return (0.5 * v) * torch.where(v < 0, e, 2.0 - e)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * torch.tensor(0.70710678118654752440, dtype=f)))
    if act == ACT_QUICKGELU:
        return v * (1.0 / (1.0 + torch.exp(torch.tensor(-1.702, dtype=f) * v)))
    return act64(v, act)


def measure_act_error(act, bf16_kernel, n=400001):
    """max over [-8, 8] of |formula in fp32 - exact fp64| / max(|v|, 1)."""
    v = torch.linspace(-8.0, 8.0, n, dtype=torch.float64).float()
    got = act_formula_fp32(v, act, bf16_kernel).double()
    return ((got - act64(v.double(), act)).abs() / v.double().abs().clamp_min(1.0)).max().item()


def block16_chain_fp32(a, w):
    """CPU emulation of a matrix-core K loop: exact 16-wide blocks of products, added sequentially in fp32 (a, w: fp64 operands)."""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k in range(0, a.shape[1], 16):
        acc = (acc.double() + a[:, k:k + 16] @ w[:, k:k + 16].T).float()
    return acc


def measure_c(a, w):
    """Worst |fp32 result - fp64| / (2^-24 S) of the CPU fp32 matmul and of the 16-wide block chain (a, w: operand values)."""
    a64, w64 = a.double(), w.double()
    ref = a64 @ w64.T
    s = (a64.abs() @ w64.abs().T).clamp_min(1e-300) * U24
    r_mm = ((a.float() @ w.float().T).double() - ref).abs().div(s).max().item()
    r_bl = (block16_chain_fp32(a64, w64).double() - ref).abs().div(s).max().item()
    return r_mm, r_bl


class Case:
    """One structured launch: a form of GemmArgs at one geometry. Everything not given is the plain dense form."""

    def __init__(self, name, M, N, K, prec="bf16", batch=1, lda=None, ldw=None, ld32=None, ldT=None, ldmul=None, ldres=None, ldresT=None,
                 bias=False, act=0, mul=False, res=False, resT=False, out32=False, outT=False, gap=0, grp=None, remap=None, split_n=0,
                 ldT_lo=None, hm=None, pair32=False, dual=None, lda2=None, ldw2=None, ssq=False, sumo=False, rs=None, rs_parts=0, seed=0):
        self.name, self.M, self.N, self.K, self.prec, self.batch = name, M, N, K, prec, batch
        self.lda, self.ldw = lda or K, ldw or K
        self.Nout = N // 2 if pair32 else N
        self.ld32, self.ldT = ld32 or self.Nout, ldT or (self.Nout - split_n if split_n else self.Nout)
        self.ldmul, self.ldres, self.ldresT = ldmul or N, ldres or N, ldresT or N
        self.bias, self.act, self.mul, self.res, self.resT, self.out32, self.outT = bias, act, mul, res, resT, out32, outT
        self.gap = gap                      # extra rows between the batches of every batched buffer (the bs* strides)
        self.grp = grp                      # grouped form: column starts [batch + 1]
        self.remap = remap                  # (rb, s_hi, s_lo, ro)
        self.split_n, self.ldT_lo = split_n, ldT_lo or split_n
        self.hm = hm                        # (hm_D, hm_L)
        self.pair32, self.dual = pair32, dual   # dual: "same" (A2 = A) or "sep" (its own A2)
        self.lda2, self.ldw2 = lda2 or self.lda, ldw2 or K
        self.ssq, self.sumo = ssq, sumo     # producers: ssq_out / sum_out
        self.rs, self.rs_parts = rs, rs_parts   # consumers: "rms" / "ln"
        self.rs_invk, self.rs_eps = 1.0 / K, 1e-5
        self.seed = seed
        if grp is not None:
            assert len(grp) == batch + 1 and N == max(b - a for a, b in zip(grp, grp[1:]))

    @property
    def tdtype(self):
        return torch.bfloat16 if self.prec == "bf16" else torch.float32

    def orow(self, r):
        if not self.remap:
            return r
        rb, s_hi, s_lo, ro = self.remap
        return (r // rb) * s_hi + (r % rb) * s_lo + ro

    def __repr__(self):
        return self.name


def _padded(vals, rows_alloc, ld, fill, dtype):
    """[b, r, c] values in the top-left corner of a [b, rows_alloc, ld] buffer of `fill`."""
    b, r, c = vals.shape
    out = torch.full((b, rows_alloc, ld), fill, dtype=torch.float32)
    out[:, :r, :c] = vals
    return out.to(dtype).contiguous()


def make_inputs(case, poison=0):
    """Operands of a case as CPU tensors [batch, rows (+ gap), ld] in the dtype the launch reads. The VALUES depend on the seed only;
    the padding (columns beyond K / N up to the leading dimension, the gap rows between batches) is NaN (poison 0) or another
    finite pattern (poison 1): no output may depend on it."""
    c = case
    g = torch.Generator().manual_seed(1000 + c.seed)
    fill = float("nan") if poison == 0 else 3.0 + poison
    T = c.tdtype
    nb = 1 if c.grp is not None else c.batch
    wrows = c.grp[-1] if c.grp is not None else c.N
    d = {}
    d["A"] = _padded(torch.rand(c.batch, c.M, c.K, generator=g) * 2 - 1, c.M + c.gap, c.lda, fill, T)
    d["W"] = _padded(torch.randn(nb, wrows, c.K, generator=g) * c.K ** -0.5, wrows + c.gap, c.ldw, fill, T)
    if c.dual:
        d["W2"] = _padded(torch.randn(1, c.N, c.K, generator=g) * c.K ** -0.5, c.N, c.ldw2, fill, T)
        if c.dual == "sep":
            d["A2"] = _padded(torch.rand(1, c.M, c.K, generator=g) * 2 - 1, c.M, c.lda2, fill, T)
    if c.bias:
        d["bias"] = _padded(torch.randn(nb, 1, wrows, generator=g) * 0.5, 1, wrows + 4 * (c.gap > 0), fill, torch.float32)
    if c.mul:
        d["mul"] = _padded(torch.rand(c.batch, c.M, c.N, generator=g) * 2 - 1, c.M + c.gap, c.ldmul, fill, T)
    if c.res:
        d["res"] = _padded(torch.randn(c.batch, c.M, c.N, generator=g), c.M + c.gap, c.ldres, fill, torch.float32)
    if c.resT:
        d["resT"] = _padded(torch.randn(1, c.M, c.N, generator=g), c.M, c.ldresT, fill, T)
    if c.rs:
        # the producer's partial statistics of a plausible K-wide input row: sums of 32 values ~ N(0.1, 1) and of their squares
        x = torch.randn(c.M, c.rs_parts, max(c.K // c.rs_parts, 1), generator=g) + 0.1
        d["rs_ssq"] = x.pow(2).sum(-1).float().contiguous()
        if c.rs == "ln":
            d["rs_sum"] = x.sum(-1).float().contiguous()
            w = d["W"][0, :c.N, :c.K].double()
            d["rs_c"] = w.sum(1).float().contiguous()   # sum_k W'[n][k] of the ROUNDED operand values
    if c.grp is not None:
        d["grp_col"] = torch.tensor(c.grp, dtype=torch.int32)
    return d


def strides(case, inp):
    """The element strides a launch of this case passes (what the buffers of make_inputs / expected are laid out with)."""
    c = case
    s = {"bsA": inp["A"].stride(0) if c.batch > 1 else 0, "bsW": inp["W"].stride(0) if (c.batch > 1 and c.grp is None) else 0,
         "bsBias": inp["bias"].stride(0) if (c.bias and c.batch > 1 and c.grp is None) else 0,
         "bsMul": inp["mul"].stride(0) if (c.mul and c.batch > 1) else 0, "bsRes": inp["res"].stride(0) if (c.res and c.batch > 1) else 0}
    rows = max(c.orow(r) for r in range(c.M)) + 1 + c.gap
    batched = c.batch > 1 and c.grp is None
    s["bs32"] = rows * c.ld32 if (batched and c.out32) else 0
    s["bsT"] = rows * c.ldT if (batched and c.outT) else 0
    return s


def _scatter(size, idx, val, bnd):
    img = torch.full((size,), CANARY, dtype=torch.float64)
    b = torch.zeros(size, dtype=torch.float64)
    m = torch.zeros(size, dtype=torch.bool)
    flat = idx.reshape(-1) + GUARD
    assert flat.unique().numel() == flat.numel(), "two output elements map to one address: not a valid geometry"
    img[flat], b[flat], m[flat] = val.reshape(-1), bnd.reshape(-1), True
    return img, b, m


def product_terms(case, inp, z):
    """fp64 product, S = sum_k |a||w| and the accumulation-error term of batch / group z (and of the second product of a dual)."""
    c = case
    A = inp["A"][z, :c.M, :c.K].double()
    if c.grp is not None:
        W = inp["W"][0, c.grp[z]:c.grp[z + 1], :c.K].double()
    else:
        W = inp["W"][z, :c.N, :c.K].double()
    P, S = A @ W.T, A.abs() @ W.abs().T
    e = S * (X3_REL if c.prec == "bf16x3" else C_ACC * U24)
    return P, S, e


def expected(case, inp):
    """{buffer name: (image, bound, written)}: flat fp64 / fp64 / bool tensors over the WHOLE allocation of every output buffer
    (GUARD elements, the launch's extent, GUARD elements). Also returns the launch's strides."""
    c = case
    st = strides(c, inp)
    cacc = X3_REL if c.prec == "bf16x3" else C_ACC * U24
    uT = UBF if c.prec == "bf16" else U24
    vals, errs = [], []
    for z in range(c.batch):
        P, S, e = product_terms(c, inp, z)
        n_z = P.shape[1]
        col0 = c.grp[z] if c.grp is not None else 0
        v = P
        if c.rs == "rms":
            t = inp["rs_ssq"].double().sum(1)
            rsc = (t * c.rs_invk + c.rs_eps).rsqrt()[:, None]
            v = v * rsc
            e = e * rsc + v.abs() * ((c.rs_parts + 4) * U24 + U24)
        elif c.rs == "ln":   # the kernel's declared algebra: rstd * (A.W'^T - mean * rs_c[n])
            qs, qq = inp["rs_sum"].double(), inp["rs_ssq"].double()
            mean = qs.sum(1) * c.rs_invk
            e_mean = c.rs_parts * U24 * qs.abs().sum(1) * c.rs_invk + U24 * mean.abs()
            var = (qq.sum(1) * c.rs_invk - mean * mean).clamp_min(0.0)
            e_var = (c.rs_parts + 1) * U24 * qq.sum(1) * c.rs_invk + 2 * mean.abs() * e_mean + 2 * U24 * mean * mean + U24 * var
            rstd = (var + c.rs_eps).rsqrt()
            d_rstd = 0.5 * e_var / (var + c.rs_eps) + 3 * U24
            mc = mean[:, None] * inp["rs_c"].double()[None, :]
            inner = P - mc
            e_in = e + e_mean[:, None] * inp["rs_c"].double().abs()[None, :] + U24 * (mc.abs() + inner.abs())
            vl = rstd[:, None] * inner
            el = rstd[:, None] * e_in + vl.abs() * (d_rstd[:, None] + U24)
            if c.pair32:   # the GELU'd blocks only; the plain multiplier factor is untouched
                gel = ((torch.arange(c.N) // 32) % 2 == 0)[None, :]
                v, e = torch.where(gel, vl, v), torch.where(gel, el, e)
            else:
                v, e = vl, el
        if c.bias:
            b = inp["bias"][0 if c.grp is not None else z, 0, col0:col0 + n_z].double()[None, :]
            v = v + b
            e = e + cacc * b.abs() + U24 * v.abs()
        if c.pair32:   # blocks of 32 interleaved columns: 2j the GELU'd layer, 2j + 1 its plain multiplier
            vv = v.reshape(c.M, c.N // 64, 2, 32)
            ee = e.reshape(c.M, c.N // 64, 2, 32)
            gate, e_g = vv[:, :, 1].reshape(c.M, -1), ee[:, :, 1].reshape(c.M, -1)
            v, e = vv[:, :, 0].reshape(c.M, -1), ee[:, :, 0].reshape(c.M, -1)
        if c.act:
            assert v.abs().max() <= 8.0, "activation error measured over [-8, 8] only"
            e = LIPSCHITZ[c.act] * e + ACT_ERR.get(("bf16" if c.prec == "bf16" else "fp32", c.act), 0.0) * v.abs().clamp_min(1.0)
            v = act64(v, c.act)
            e = e + U24 * v.abs()
        if c.mul:
            m = inp["mul"][z, :c.M, :c.N].double()
            v = v * m
            e = e * m.abs() + U24 * v.abs()
        if c.dual:
            A2 = (inp["A2"] if c.dual == "sep" else inp["A"])[0, :c.M, :c.K].double()
            W2 = inp["W2"][0, :c.N, :c.K].double()
            gate, e_g = A2 @ W2.T, (A2.abs() @ W2.abs().T) * cacc
        if c.dual or c.pair32:   # the gate is stored in bf16 before the multiply
            e_g = e_g + UBF * gate.abs()
            e = e * (gate.abs() + e_g) + v.abs() * e_g
            v = v * gate
            e = e + U24 * v.abs()
        if c.res:
            v = v + inp["res"][z, :c.M, :c.N].double()
            e = e + U24 * v.abs()
        if c.resT:
            v = v + inp["resT"][0, :c.M, :c.N].double()
            e = e + U24 * v.abs()
        vals.append(v)
        errs.append(e)
    out = {}
    M, r = c.M, torch.arange(c.M)
    orow = torch.tensor([c.orow(int(i)) for i in r])
    rows_ext = int(orow.max()) + 1 + max(c.gap, 2)   # rows before `ro`, the rows a remap skips and rows after the last one stay canary

    def image(name, ld, bs, bound_of):
        idx, val, bnd = [], [], []
        for z in range(c.batch):
            v, e = vals[z], errs[z]
            n = torch.arange(v.shape[1])
            col0 = c.grp[z] if c.grp is not None else 0
            idx.append(z * bs + orow[:, None] * ld + col0 + n[None, :])
            val.append(v)
            bnd.append(bound_of(v, e))
        size = 2 * GUARD + (c.batch - 1) * bs + rows_ext * ld
        out[name] = _scatter(size, torch.cat([i.reshape(-1) for i in idx]), torch.cat([x.reshape(-1) for x in val]),
                             torch.cat([x.reshape(-1) for x in bnd]))

    b32 = lambda v, e: e + U24 * v.abs()          # noqa: E731
    bT = lambda v, e: e + uT * v.abs()            # noqa: E731  (one rounding to the operand type)
    if c.out32:
        image("out32", c.ld32, st["bs32"], b32)
    if c.outT and c.hm:
        D, L = c.hm
        n = torch.arange(c.N)
        idx = ((r[:, None] // L) * (c.N // D) + n[None, :] // D) * (L * D) + (r[:, None] % L) * D + n[None, :] % D
        out["outT"] = _scatter(2 * GUARD + M * c.N, idx, vals[0], bT(vals[0], errs[0]))
    elif c.outT and c.split_n:
        v, e, n = vals[0], errs[0], torch.arange(c.N)
        lo, hi = n < c.split_n, n >= c.split_n
        out["outT_lo"] = _scatter(2 * GUARD + (M + 2) * c.ldT_lo, r[:, None] * c.ldT_lo + n[None, lo], v[:, lo], bT(v[:, lo], e[:, lo]))
        out["outT"] = _scatter(2 * GUARD + rows_ext * c.ldT, orow[:, None] * c.ldT + (n[None, hi] - c.split_n), v[:, hi], bT(v[:, hi], e[:, hi]))
    elif c.outT:
        image("outT", c.ldT, st["bsT"], bT)
    if c.ssq or c.sumo:   # [M, N / 32] partials of row r (not remapped): 32-term fp32 sums of values that carry the bound above
        v = vals[0]
        ex = b32(v, errs[0]) if c.out32 else bT(v, errs[0])   # statistics of the fp32 values / of the STORED bf16 values
        v3, e3 = v.reshape(M, c.N // 32, 32), ex.reshape(M, c.N // 32, 32)
        idx = r[:, None] * (c.N // 32) + torch.arange(c.N // 32)[None, :]
        size = 2 * GUARD + (M + 2) * (c.N // 32)
        if c.ssq:
            q = v3.pow(2).sum(-1)
            out["ssq_out"] = _scatter(size, idx, q, (2 * v3.abs() * e3 + e3 * e3).sum(-1) + 33 * U24 * q)
        if c.sumo:
            out["sum_out"] = _scatter(size, idx, v3.sum(-1), e3.sum(-1) + 32 * U24 * v3.abs().sum(-1))
    return out, st


def buffer_dtype(case, name):
    return case.tdtype if name in ("outT", "outT_lo") else torch.float32


def canary_buffers(case, exp, device="cpu"):
    """Every output buffer of the case, canary-filled, at its full allocation."""
    return {k: torch.full((img.numel(),), CANARY, dtype=buffer_dtype(case, k), device=device) for k, (img, _, _) in exp.items()}


def untouched(bufs):
    return all(bool((b == CANARY).all()) for b in bufs.values())


def _region(case, name, i, size):
    if i < GUARD:
        return "guard band in front of the buffer"
    if i >= size - GUARD:
        return "guard band behind the buffer"
    return "padding column / skipped row inside the buffer"


def check(case, exp, bufs):
    """Holds every buffer of a launch against its expected image; raises AssertionError naming the worst element (flat index without
    the guard, region, ratio to its bound) on the first failing buffer. Returns {buffer: worst |err| / bound over its written set};
    a bf16 buffer has a second entry "<buffer>:fp32 part", the share of the error that the final rounding cannot explain,
    max(|err| - 2^-8 |ref|, 0) over the bound without its rounding term (correct rounding alone takes the plain ratio to 0.996)."""
    worst = {}
    assert set(bufs) == set(exp), (sorted(bufs), sorted(exp))
    for name, (img, bnd, wr) in exp.items():
        got = bufs[name].detach().cpu().double().reshape(-1)
        assert got.numel() == img.numel(), (name, got.numel(), img.numel())
        stray = (~wr) & ((got != CANARY) | ~torch.isfinite(got))
        if bool(stray.any()):
            i = int(stray.nonzero()[0])
            raise AssertionError(f"{case.name}: {name}[{i - GUARD}] = {got[i].item()} written OUTSIDE the form's written set "
                                 f"({_region(case, name, i, got.numel())}); {int(stray.sum())} such elements")
        fin = torch.isfinite(got) | ~wr
        if not bool(fin.all()):
            i = int((~fin).nonzero()[0])
            raise AssertionError(f"{case.name}: {name}[{i - GUARD}] = {got[i].item()} is not finite (written set)")
        err = torch.where(wr, (got - img).abs(), torch.zeros_like(got))
        ratio = err / bnd.clamp_min(1e-300)
        i = int(ratio.argmax())
        w = ratio[i].item()
        if w > 1.0:
            raise AssertionError(f"{case.name}: {name}[{i - GUARD}] = {got[i].item()!r}, reference {img[i].item()!r}: |err| = "
                                 f"{abs(got[i].item() - img[i].item()):.3e} is {w:.2f} x its bound {bnd[i].item():.3e} (written set); "
                                 f"{int((ratio > 1).sum())} elements over their bound")
        worst[name] = w
        if buffer_dtype(case, name) == torch.bfloat16:
            rnd = UBF * img.abs()
            worst[name + ":fp32 part"] = torch.where(wr, (err - rnd).clamp_min(0.0) / (bnd - rnd).clamp_min(1e-300), torch.zeros_like(got)).max().item()
    return worst


def worst_ratio(w, fp32_part=False):
    """The largest entry of check()'s result; with fp32_part the bf16 buffers count by their "fp32 part" only."""
    if fp32_part:
        return max(v for k, v in w.items() if k.endswith(":fp32 part") or (k + ":fp32 part") not in w)
    return max(v for k, v in w.items() if not k.endswith(":fp32 part"))


def ideal_buffers(case, exp):
    """What a correct launch leaves behind, as far as the reference knows: the fp64 image rounded once to each buffer's dtype."""
    return {k: img.to(buffer_dtype(case, k)) for k, (img, _, _) in exp.items()}


# ------------------------------------------------------------------------------------------------ the cases
# kernel families by GemmArgs::kernel_id / 1000
PP, PERSIST, TILE256, TILE128, TILE64, TILE32, SPLITK = 1, 2, 4, 5, 6, 7, 8
RES32, RES64X32, RES64, DUAL32, DUAL64, SKINNY, SKINNY_DUAL, X3, SPLITK_X3 = 10, 11, 12, 15, 16, 17, 18, 21, 23
RES = (RES32, RES64X32, RES64)
BIG_ROUTES = [(128, {"gemm_tile": 2}, PP), (320, {"gemm_tile": 2}, PERSIST), (128, {"gemm_tile": 2, "gemm_pp": 0}, PERSIST),
              (320, {"gemm_tile": 2, "gemm_pp": 0}, PERSIST)]   # (K, options, family) of a full-tile problem on the persistent 256x256 kernels
REMAPS = [(3, 11, 1, 4), (5, 12, 2, 1)]


def _routes(M):
    """(options, kernel families allowed) through which a small bf16 problem of M rows reaches every family that takes it."""
    return [({}, (SKINNY,) if M <= 32 else RES), ({"gemm_tile": 1}, (TILE128,)), ({"gemm_tile": 8}, (TILE64,)), ({"gemm_tile": 7}, (TILE32,)),
            ({"gemm_tile": 10}, (RES32,)), ({"gemm_tile": 11}, (RES64X32,)), ({"gemm_tile": 12}, (RES64,)),
            ({"gemm_tile": 2, "gemm_persist": 0}, (TILE256,))]


def gpu_cases():
    """[(form, Case, options, allowed kernel families)]: every row of the table of forms, at the smallest shapes at which the path can
    still go wrong (more than one tile each way, ragged last tiles, K of one slice / more slices than ring stages / an odd count)."""
    out = []
    sd = [0]

    def add(form, opts, kinds, name, *a, **kw):
        sd[0] += 1
        tag = ",".join(f"{k[5:]}={v}" for k, v in opts.items()) or "default"
        out.append((form, Case(f"{form}:{name}[{tag}]", *a, seed=sd[0], **kw), opts, tuple(kinds)))

    # ---- independent leading dimensions and batch strides
    for (M, N, K) in [(70, 136, 320), (21, 136, 64)]:
        for opts, kinds in _routes(M):
            add("strides", opts, kinds, f"T16B {M}x{N}x{K}x3", M, N, K, batch=3, lda=K + 8, ldw=K + 16, ldT=N + 8, ldmul=N + 8, bias=True,
                act=ACT_RELU, mul=True, outT=True, gap=1)
            add("strides", opts, kinds, f"T8B+f32 {M}x{N}x{K}x3", M, N, K, batch=3, lda=K + 8, ldw=K + 16, ld32=N + 4, ldT=N + 4, ldres=N + 4,
                bias=True, act=ACT_GELU, res=True, out32=True, outT=True, gap=1)
    for K in (1088, 2112):   # the skinny kernel's 8- and 16-wave K splits (K / 16 > 64, > 128)
        add("strides", {}, (SKINNY,), f"T16B 21x136x{K}x3", 21, 136, K, batch=3, lda=K + 8, ldw=K + 16, ldT=144, ldmul=144, bias=True, act=ACT_RELU,
            mul=True, outT=True, gap=1)
    for K, opts, kinds in [(128, {"gemm_tile": 2}, (PP,)), (320, {"gemm_tile": 2}, (PERSIST,)), (128, {"gemm_tile": 2, "gemm_pp": 0}, (PERSIST,)),
                           (320, {"gemm_tile": 2, "gemm_persist": 0}, (TILE256,))]:
        add("strides", opts, kinds, f"T16B 512x512x{K}", 512, 512, K, lda=K + 8, ldw=K + 16, ldT=520, bias=True, act=ACT_RELU, outT=True)
        add("strides", opts, kinds, f"f32+T 512x512x{K}", 512, 512, K, lda=K + 8, ldw=K + 16, ld32=516, ldT=516, ldres=516, bias=True, res=True,
            out32=True, outT=True)
    for prec, kinds in [("fp32", (TILE128,)), ("bf16x3", (X3,))]:
        add("strides", {}, kinds, f"{prec} 70x136x320x3", 70, 136, 320, prec=prec, batch=3, lda=324, ldw=328, ld32=140, ldT=140, ldres=140,
            bias=True, act=ACT_GELU, res=True, out32=True, outT=True, gap=1)
    for prec, kinds in [("bf16", (SPLITK,)), ("bf16x3", (SPLITK_X3,))]:   # the two-pass split-K and its reduce kernel (K >= 1536, underfilled grid)
        add("strides", {"gemm_splitk": 1}, kinds, f"{prec} split-K 70x136x1536", 70, 136, 1536, prec=prec, lda=1544, ldw=1552, ld32=140, ldT=140, ldres=140,
            bias=True, act=ACT_GELU, res=True, out32=True, outT=True)
    # ---- grouped
    for M in (5, 70):
        for K in (64, 320):
            for opts, kinds in [({}, (RES32,)), ({"gemm_res_maxwg": 8}, (RES32,) if M <= 32 else (RES64,))]:
                add("grouped", opts, kinds, f"{M}x[100,50,7,1]x{K}", M, 100, K, batch=4, grp=[0, 100, 150, 157, 158], ld32=160, bias=True,
                    out32=True, lda=K + 8, gap=1)
    # ---- output-row remap; the persistent kernels must decline (gemm_tile 2 alone lands on the one-tile 256x256 kernel)
    for i, rm in enumerate(REMAPS):
        for M in (21, 69, 300):
            routes = _routes(M) + [({"gemm_tile": 2}, (TILE256,))] if M == 69 else [({}, (SKINNY,) if M <= 32 else RES), ({"gemm_tile": 1}, (TILE128,))]
            for opts, kinds in routes:
                if i == 0:
                    add("remap", opts, kinds, f"f32 {M}x136x320 {rm}", M, 136, 320, remap=rm, ld32=140, ldres=140, bias=True, res=True, out32=True)
                else:
                    add("remap", opts, kinds, f"bf16 {M}x136x64 {rm}", M, 136, 64, remap=rm, ldT=144, bias=True, act=ACT_RELU, outT=True)
    add("remap", {}, (SKINNY,), f"f32 21x136x2112 {REMAPS[0]}", 21, 136, 2112, remap=REMAPS[0], ld32=140, ldres=140, bias=True, res=True, out32=True)
    add("remap", {}, (SKINNY,), f"bf16 21x136x1088 {REMAPS[1]}", 21, 136, 1088, remap=REMAPS[1], ldT=144, bias=True, act=ACT_RELU, outT=True)
    # full 256x256 tiles: launch_persistent / launch_pp see the problem and must hand a remap on to the one-tile kernel
    for K, opts, _ in BIG_ROUTES:
        add("remap", opts, (TILE256,), f"f32 512x256x{K} {REMAPS[0]}", 512, 256, K, remap=REMAPS[0], ld32=260, ldres=260, bias=True, res=True, out32=True)
        add("remap", opts, (TILE256,), f"bf16 512x256x{K} {REMAPS[1]}", 512, 256, K, remap=REMAPS[1], ldT=264, bias=True, act=ACT_RELU, outT=True)
    # ---- column split (+ remap on the hi part)
    for (N, sn) in [(264, 128), (384, 256)]:
        for M in (21, 70, 300):
            for opts, kinds in [({}, (SKINNY,) if M <= 32 else RES), ({"gemm_tile": 1}, (TILE128,)), ({"gemm_tile": 8}, (TILE64,))]:
                add("split", opts, kinds, f"{M}x{N}x320 split {sn}", M, N, 320, split_n=sn, ldT_lo=sn + 8, ldT=N - sn + 8, remap=REMAPS[M % 2],
                    bias=True, outT=True)
    # ---- head-major output
    for L, Ds in [(256, (8, 128)), (512, (32, 256))]:
        for D in Ds:
            for K, opts, kinds in [(128, {"gemm_tile": 2}, (PP,)), (320, {"gemm_tile": 2}, (PERSIST,)), (128, {"gemm_tile": 2, "gemm_pp": 0}, (PERSIST,))]:
                add("headmajor", opts, kinds, f"1024x256x{K} D{D} L{L}", 1024, 256, K, hm=(D, L), bias=True, outT=True)
    # ---- GEGLU pair over block-interleaved weights, with and without the folded LayerNorm
    for fold in (None, "ln"):
        for K in (64, 320):
            add("pair32", {"gemm_small": 0}, (TILE128,), f"70x2*192x{K} fold={fold}", 70, 384, K, pair32=True, bias=True, act=ACT_GELU, outT=True,
                ldT=200, rs=fold, rs_parts=K // 32)
        add("pair32", {}, (PP,), f"2560x2*2048x128 fold={fold}", 2560, 4096, 128, pair32=True, bias=True, act=ACT_GELU, outT=True, rs=fold, rs_parts=4)
    # ---- dual (W2, A2 != A, lda2 != lda)
    for fold in (None, "ln"):
        for M in (5, 21, 70):
            for K in (64, 320, 1088):
                routes = [({}, (SKINNY_DUAL,)), ({"gemm_skinny": 0}, (DUAL32,))] if M <= 32 else [({}, (DUAL64,))]
                for opts, kinds in routes:
                    add("dual", opts, kinds, f"{M}x100x{K} fold={fold}", M, 100, K, dual="sep" if K != 320 else "same", lda=K + 8, lda2=K + 24,
                        ldw2=K + 8, ldT=104, bias=True, act=ACT_GELU, outT=True, rs=fold, rs_parts=K // 32)
    # ---- RMS producer (statistics of the fp32 stream / of the stored bf16 values) and the LN-fold producer
    for M in (21, 70, 300):
        for opts, kinds in [({}, (SKINNY,) if M <= 32 else RES), ({"gemm_tile": 1}, (TILE128,)), ({"gemm_tile": 8}, (TILE64,))]:
            add("rms_producer", opts, kinds, f"f32 stream {M}x96x320", M, 96, 320, bias=True, res=True, out32=True, outT=True, ssq=True, ld32=100, ldres=100)
            add("rms_producer", opts, kinds, f"bf16 stream {M}x96x320", M, 96, 320, bias=True, resT=True, outT=True, ssq=True, ldT=104, ldresT=104)
            add("ln_producer", opts, kinds, f"{M}x96x320", M, 96, 320, bias=True, res=True, out32=True, outT=True, ssq=True, sumo=True, ld32=100, ldres=100)
    for K in (1088, 2112):   # skinny 8- / 16-wave
        add("rms_producer", {}, (SKINNY,), f"f32 stream 21x96x{K}", 21, 96, K, bias=True, res=True, out32=True, outT=True, ssq=True, ld32=100, ldres=100)
        add("rms_producer", {}, (SKINNY,), f"bf16 stream 21x96x{K}", 21, 96, K, bias=True, resT=True, outT=True, ssq=True, ldT=104, ldresT=104)
    for K, opts, fam in BIG_ROUTES:   # the persistent 256x256 kernels' stream epilogues: fp32 stream (epilogue 3) and bf16 stream (epilogue 4)
        add("rms_producer", opts, (fam,), f"f32 stream 512x256x{K}", 512, 256, K, bias=True, res=True, out32=True, outT=True, ssq=True, ld32=260, ldres=260)
        add("rms_producer", opts, (fam,), f"bf16 stream 512x256x{K}", 512, 256, K, bias=True, resT=True, outT=True, ssq=True)
    # (gemm_q4_kernel and gemm_wide_kernel are not in this table: they take a problem only at gemm_tile 0 once it is `large` -- 160 tiles of 256x256 with
    # < 15 % padding -- and N % 384 == 0; the smallest such problem, about 2816 x 3840 x 128, is above the 2560 x 4096 x 128 cap on this file's problem
    # sizes. Their epilogues are held by the whole-model gates; the gemm_q4 / gemm_wide entries of SWEEP only show that the knobs re-route nothing here.)
    # ---- RMS consumer: every family that accepts it
    for parts in (1, 10):
        for M in (21, 70, 300):
            routes = _routes(M) if M == 70 else [({}, (SKINNY,) if M <= 32 else RES), ({"gemm_tile": 1}, (TILE128,)), ({"gemm_tile": 8}, (TILE64,))]
            for opts, kinds in routes:
                add("rms_consumer", opts, kinds, f"{M}x136x320 parts {parts}", M, 136, 320, rs="rms", rs_parts=parts, bias=True, act=ACT_RELU, outT=True, ldT=144)
        for K, opts, fam in BIG_ROUTES:
            add("rms_consumer", opts, (fam,), f"512x256x{K} parts {parts}", 512, 256, K, rs="rms", rs_parts=parts, bias=True, act=ACT_RELU, outT=True)
        add("rms_consumer", {"gemm_splitk": 1}, (SPLITK,), f"split-K 70x136x1536 parts {parts}", 70, 136, 1536, rs="rms", rs_parts=parts, bias=True,
            act=ACT_RELU, outT=True, ldT=144)
        add("rms_consumer", {}, (SKINNY,), f"21x136x1088 parts {parts}", 21, 136, 1088, rs="rms", rs_parts=parts, bias=True, act=ACT_RELU, outT=True, ldT=144)
    return out


# (B) the knob settings that change routing, swept over one small case per form
SWEEP = ([{"gemm_tile": t} for t in (0, 1, 2, 7, 8, 10, 11, 12)] +
         [{k: 0} for k in ("gemm_persist", "gemm_pp", "gemm_small", "gemm_resident", "gemm_skinny", "gemm_variant", "gemm_epi")] +
         [{"gemm_splitk": 1}, {"gemm_q4": 0}, {"gemm_q4": 1}, {"gemm_q4": 2}, {"gemm_wide": 1}, {"gemm_tile": 2, "gemm_persist": 0}, {"gemm_tile": 2, "gemm_pp": 0}])


def sweep_cases():
    """One small case per form (the first of gpu_cases() that is not a large-tile shape)."""
    seen, out = set(), []
    for form, case, opts, kinds in gpu_cases():
        if form not in seen and (case.M < 512 or form == "headmajor"):
            seen.add(form)
            out.append((form, case, opts))
    return out
