"""CPU-only: pins tests/gemm_forms_reference.py (the fp64 references, bounds and checker the GPU file tests/test_gemm_forms_gpu.py
relies on) against independent restatements in fp64, to 1e-12, and shows that `check` rejects every single-defect mutation of a
correct output image."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_forms_reference as R
from tests.gemm_forms_reference import Case, GUARD, CANARY

TOL = 1e-12


def _case_of(form, pred=lambda c: True):
    for f, c, _, _ in R.gpu_cases():
        if f == form and c.M <= 1024 and pred(c):
            return c
    raise KeyError(form)


def _written(exp, name):
    img, bnd, wr = exp[name]
    return img[GUARD:-GUARD], bnd[GUARD:-GUARD], wr[GUARD:-GUARD]


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _dyadic(shape, g, den, lim):
    """Values k / den, |k| <= lim: exact in bf16, with exactly representable squares and short sums."""
    return torch.randint(-lim, lim + 1, shape, generator=g).double() / den


# ------------------------------------------------------------------------------------------------ the measured constants
def test_accumulation_constant_is_four_times_the_measured_worst():
    """Over the operands of EVERY case shape (the issue's rule): C_ACC is 4 x the worst measured ratio, rounded up to a whole number."""
    worst, seen = 0.0, set()
    for form, c, _, _ in R.gpu_cases():
        key = (c.M, c.N, c.K, c.prec)
        if key in seen:
            continue
        seen.add(key)
        inp = R.make_inputs(c)
        r_mm, r_bl = R.measure_c(inp["A"][0, :c.M, :c.K], inp["W"][0, :(c.grp[-1] if c.grp else c.N), :c.K])
        print(f"[gemm forms] {key}: |fp32 - fp64| / (2^-24 S): matmul {r_mm:.2f}, 16-wide block chain {r_bl:.2f}")
        worst = max(worst, r_mm, r_bl)
    print(f"[gemm forms] worst {worst:.2f}, C_ACC {R.C_ACC}")
    assert 4 * worst <= R.C_ACC <= 4 * worst + 1.0 and R.C_ACC <= 64   # 64 = the rigorous K of the shortest case


def test_activation_error_terms_are_four_times_the_measured_ones():
    for (prec, act), term in R.ACT_ERR.items():
        m = R.measure_act_error(act, prec == "bf16")
        print(f"[gemm forms] activation {act} ({prec} kernels): max |fp32 formula - fp64| / max(|v|, 1) over [-8, 8] = {m:.3e}")
        assert 4 * m <= term <= 8 * m + 1e-7


def test_bf16_rounding_term_is_the_format_unit_roundoff():
    x = torch.linspace(1.0, 2.0, 100001, dtype=torch.float64)
    rel = ((x.bfloat16().double() - x).abs() / x).max().item()
    assert 0.99 * R.UBF <= rel * (1 + R.UBF) <= R.UBF * (1 + 1e-9)   # half an ulp of 8 significant bits, reached just above 1


# ------------------------------------------------------------------------------------------------ restatements
def test_check_accepts_the_correctly_rounded_image_of_every_case_and_ignores_padding():
    for form, c, _, _ in R.gpu_cases():
        if c.M > 600:
            continue
        inp = R.make_inputs(c)
        exp, _ = R.expected(c, inp)
        w = R.check(c, exp, R.ideal_buffers(c, exp))
        assert R.worst_ratio(w) <= 1.0 and all(v == 0.0 for k, v in w.items() if k.endswith(":fp32 part"))   # correct rounding leaves no fp32 part
        assert not R.untouched(R.ideal_buffers(c, exp)) and R.untouched(R.canary_buffers(c, exp))
    c = _case_of("strides")
    e0, _ = R.expected(c, R.make_inputs(c, poison=0))
    e1, _ = R.expected(c, R.make_inputs(c, poison=1))
    for k in e0:
        assert all(torch.equal(a, b) for a, b in zip(e0[k], e1[k]))


def test_remap_formula_against_loops():
    c = _case_of("remap", lambda c: c.out32 and c.M == 21)
    inp = R.make_inputs(c)
    exp, _ = R.expected(c, inp)
    v = inp["A"][0, :, :c.K].double() @ inp["W"][0, :, :c.K].double().T + inp["bias"][0, 0].double() + inp["res"][0, :, :c.N].double()
    rb, s_hi, s_lo, ro = c.remap
    img, _, wr = _written(exp, "out32")
    want = torch.full_like(img, CANARY)
    for r in range(c.M):
        row = (r // rb) * s_hi + (r % rb) * s_lo + ro
        for n in range(c.N):
            want[row * c.ld32 + n] = v[r, n]
    _close(img, want)
    assert int(wr.sum()) == c.M * c.N and not bool(wr[:ro * c.ld32].any())


def test_headmajor_index_against_reshape_permute():
    c = Case("hm", 512, 256, 128, hm=(32, 256), bias=True, outT=True, seed=3)
    inp = R.make_inputs(c)
    exp, _ = R.expected(c, inp)
    v = inp["A"][0].double() @ inp["W"][0].double().T + inp["bias"][0, 0].double()
    D, L = c.hm
    want = v.reshape(c.M // L, L, c.N // D, D).permute(0, 2, 1, 3).reshape(-1)
    img, _, wr = _written(exp, "outT")
    _close(img, want)
    assert bool(wr.all())


def test_pair32_interleave_against_plain_geglu():
    c = _case_of("pair32", lambda c: c.rs is None and c.K == 64)
    inp = R.make_inputs(c)
    exp, _ = R.expected(c, inp)
    W, b, A = inp["W"][0, :, :c.K].double(), inp["bias"][0, 0].double(), inp["A"][0, :, :c.K].double()
    blk = torch.arange(c.N) // 32
    W1, Wg, b1, bg = W[blk % 2 == 0], W[blk % 2 == 1], b[blk % 2 == 0], b[blk % 2 == 1]
    want = F.gelu(A @ W1.T + b1) * (A @ Wg.T + bg)
    img, _, wr = _written(exp, "outT")
    got = img.reshape(-1, c.ldT)[:c.M, :c.N // 2]
    _close(got, want)
    assert int(wr.sum()) == c.M * c.N // 2


def test_grouped_against_per_group_matmul():
    c = _case_of("grouped", lambda c: c.M == 70 and c.K == 320)
    inp = R.make_inputs(c)
    exp, _ = R.expected(c, inp)
    img, _, wr = _written(exp, "out32")
    img = img.reshape(-1, c.ld32)
    for z in range(c.batch):
        a, b = c.grp[z], c.grp[z + 1]
        want = inp["A"][z, :c.M, :c.K].double() @ inp["W"][0, a:b, :c.K].double().T + inp["bias"][0, 0, a:b].double()
        _close(img[:c.M, a:b], want)
    assert bool((img[:, c.grp[-1]:] == CANARY).all()) and bool((img[c.M:] == CANARY).all())


def test_rms_consumer_against_rmsnorm_then_matmul():
    c = Case("rmsc", 21, 136, 320, rs="rms", rs_parts=10, outT=True, seed=5)
    inp = R.make_inputs(c)
    g = torch.Generator().manual_seed(1)
    x = _dyadic((c.M, c.K), g, 16, 16)
    inp["A"] = x.to(c.tdtype)[None].contiguous()
    inp["rs_ssq"] = x.pow(2).reshape(c.M, 10, 32).sum(-1).float()   # exact in fp32
    exp, _ = R.expected(c, inp)
    xn = x * (x.pow(2).mean(-1, keepdim=True) + c.rs_eps).rsqrt()
    want = xn @ inp["W"][0, :, :c.K].double().T
    _close(_written(exp, "outT")[0].reshape(-1, c.ldT)[:c.M, :c.N], want)


def test_ln_fold_against_layer_norm_then_matmul():
    K, M, N = 64, 21, 100
    c = Case("lnfold", M, N, K, dual="sep", rs="ln", rs_parts=2, bias=True, act=R.ACT_GELU, outT=True, ldT=104, seed=6)
    inp = R.make_inputs(c)
    g = torch.Generator().manual_seed(2)
    x, W = _dyadic((M, K), g, 16, 16), _dyadic((N, K), g, 64, 8)
    gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (K,), generator=g)].double()
    beta, b = _dyadic((K,), g, 4, 4), _dyadic((N,), g, 8, 8)
    Wf = W * gamma[None, :]                                      # W' = W diag(gamma): bf16-exact
    inp["A"], inp["W"] = x.to(c.tdtype)[None].contiguous(), Wf.to(c.tdtype)[None].contiguous()
    assert torch.equal(inp["W"][0].double(), Wf)
    inp["bias"] = (W @ beta + b).float()[None, None].contiguous()   # beta folded into the bias: exact in fp32
    inp["rs_c"] = Wf.sum(1).float()
    inp["rs_sum"], inp["rs_ssq"] = x.reshape(M, 2, 32).sum(-1).float(), x.pow(2).reshape(M, 2, 32).sum(-1).float()
    exp, _ = R.expected(c, inp)
    gate = inp["A2"][0, :, :K].double() @ inp["W2"][0, :, :K].double().T
    want = F.gelu(F.layer_norm(x, (K,), gamma, beta, c.rs_eps) @ W.T + b) * gate
    _close(_written(exp, "outT")[0].reshape(-1, c.ldT)[:M, :N], want)


def test_statistics_against_blocked_sums():
    c = _case_of("ln_producer", lambda c: c.M == 21)
    inp = R.make_inputs(c)
    exp, _ = R.expected(c, inp)
    v = inp["A"][0, :, :c.K].double() @ inp["W"][0, :, :c.K].double().T + inp["bias"][0, 0].double() + inp["res"][0, :, :c.N].double()
    _close(_written(exp, "ssq_out")[0][:c.M * 3].reshape(c.M, 3), v.pow(2).reshape(c.M, 3, 32).sum(-1))
    _close(_written(exp, "sum_out")[0][:c.M * 3].reshape(c.M, 3), v.reshape(c.M, 3, 32).sum(-1))
    assert bool((_written(exp, "ssq_out")[0][c.M * 3:] == CANARY).all())


# ------------------------------------------------------------------------------------------------ mutations
def _setup(c):
    inp = R.make_inputs(c)
    exp, _ = R.expected(c, inp)
    bufs = R.ideal_buffers(c, exp)
    R.check(c, exp, bufs)   # the unmutated image passes
    return inp, exp, bufs


def _rejected(c, exp, bufs, what):
    with pytest.raises(AssertionError, match=what):
        R.check(c, exp, bufs)


def test_mutation_one_product_term_dropped():
    """The element and the term are chosen so that the reference alone guarantees rejection: |a_k w_k| >= 2 x the element's bound
    (plus the fp32 rounding of the stored value). Holds for every K of the cases (the bound is C_ACC * 2^-24 * S, one term of S / K)."""
    for c in (_case_of("strides", lambda c: c.out32 and c.prec == "bf16" and c.M == 70), _case_of("dual", lambda c: c.K == 1088 and c.M == 70 and not c.rs)):
        inp, exp, bufs = _setup(c)
        name = "out32" if c.out32 else "outT"
        if c.out32:
            A, W = inp["A"][0, :c.M, :c.K].double(), inp["W"][0, :c.N, :c.K].double()
            r, n = 3, 5
            k = int((A[r] * W[n]).abs().argmax())
            term = float(A[r, k] * W[n, k])
            i = GUARD + c.orow(r) * c.ld32 + n
            img, bnd, _ = exp[name]
            # d out / d acc of gelu(acc + b) + res is gelu'(.) >= 0.5 for a non-negative pre-activation: choose such an element
            pre = float(A[r] @ W[n] + inp["bias"][0, 0, n].double())
            while pre < 0.2 or pre - abs(term) < 0.0:
                n += 1
                k = int((A[r] * W[n]).abs().argmax())
                term = float(A[r, k] * W[n, k])
                pre = float(A[r] @ W[n] + inp["bias"][0, 0, n].double())
                i = GUARD + c.orow(r) * c.ld32 + n
            dropped = float(R.act64(torch.tensor(pre - term, dtype=torch.float64), c.act)) + float(inp["res"][0, r, n])
            assert abs(dropped - float(img[i])) >= 2 * float(bnd[i]), (abs(dropped - float(img[i])), float(bnd[i]))
            bufs[name][i] = dropped
        else:   # bf16 output of a dual at K = 1088: the stored value moves by more than twice its bound (bf16 rounding included)
            img, bnd, wr = exp[name]
            A, W = inp["A"][0, :c.M, :c.K].double(), inp["W"][0, :c.N, :c.K].double()
            gate = inp["A2"][0, :c.M, :c.K].double() @ inp["W2"][0, :c.N, :c.K].double().T
            best = None
            for r in range(c.M):
                for n in range(c.N):
                    k = int((A[r] * W[n]).abs().argmax())
                    pre = float(A[r] @ W[n] + inp["bias"][0, 0, n].double())
                    mut = float(R.act64(torch.tensor(pre - float(A[r, k] * W[n, k]), dtype=torch.float64), c.act)) * float(gate[r, n])
                    i = GUARD + r * c.ldT + n
                    ratio = abs(mut - float(img[i])) / float(bnd[i])
                    if best is None or ratio > best[0]:
                        best = (ratio, i, mut)
                if best[0] >= 4:
                    break
            assert best[0] >= 4, best   # 4 x: twice the bound after the mutated value's own bf16 rounding (<= 1 x the bound)
            bufs[name][best[1]] = best[2]
        _rejected(c, exp, bufs, "x its bound")


def test_mutation_remapped_row_one_row_off():
    c = _case_of("remap", lambda c: c.out32 and c.M == 21)
    inp, exp, bufs = _setup(c)
    r = 2
    src, dst = GUARD + c.orow(r) * c.ld32, GUARD + (c.orow(r) + 1) * c.ld32
    assert not bool(exp["out32"][2][dst:dst + c.N].any())   # the row below is one the remap skips
    bufs["out32"][dst:dst + c.N] = bufs["out32"][src:src + c.N].clone()
    bufs["out32"][src:src + c.N] = CANARY
    _rejected(c, exp, bufs, "OUTSIDE the form's written set")


def test_mutation_pair_blocks_swapped():
    c = _case_of("pair32", lambda c: c.rs is None and c.K == 64)
    inp, exp, bufs = _setup(c)
    A, W, b = inp["A"][0, :, :c.K].double(), inp["W"][0, :, :c.K].double(), inp["bias"][0, 0].double()
    pre = (A @ W.T + b).reshape(c.M, c.N // 64, 2, 32)
    swapped = (F.gelu(pre[:, :, 1]) * pre[:, :, 0]).reshape(c.M, -1)   # the multiplier block GELU'd, the GELU block plain
    img, bnd, _ = exp["outT"]
    view = bufs["outT"][GUARD:-GUARD].reshape(-1, c.ldT)
    ref = img[GUARD:-GUARD].reshape(-1, c.ldT)[:c.M, :c.N // 2]
    assert float(((swapped - ref).abs() / bnd[GUARD:-GUARD].reshape(-1, c.ldT)[:c.M, :c.N // 2]).max()) >= 4
    view[:c.M, :c.N // 2] = swapped.to(view.dtype)
    _rejected(c, exp, bufs, "x its bound")


def test_mutation_group_columns_shifted_by_one():
    c = _case_of("grouped", lambda c: c.M == 5 and c.K == 64)
    inp, exp, bufs = _setup(c)
    view = bufs["out32"][GUARD:-GUARD].reshape(-1, c.ld32)
    a, b = c.grp[1], c.grp[2]
    view[:c.M, a + 1:b + 1] = view[:c.M, a:b].clone()
    _rejected(c, exp, bufs, "x its bound")
    inp, exp, bufs = _setup(c)   # the LAST group shifted: its column lands in the padding of the row
    view = bufs["out32"][GUARD:-GUARD].reshape(-1, c.ld32)
    view[:c.M, c.grp[-1]] = view[:c.M, c.grp[-2]]
    _rejected(c, exp, bufs, "OUTSIDE the form's written set")


def test_mutation_split_hi_part_without_its_offset():
    c = _case_of("split", lambda c: c.M == 21 and c.N == 264)
    inp, exp, bufs = _setup(c)
    img = exp["outT"][0]
    hi = c.N - c.split_n
    good = bufs["outT"].clone()
    bufs["outT"][:] = CANARY
    for r in range(c.M):   # columns n >= split_n stored at n instead of n - split_n
        src = GUARD + c.orow(r) * c.ldT
        dst = src + c.split_n
        if dst + hi <= bufs["outT"].numel():
            bufs["outT"][dst:dst + hi] = good[src:src + hi]
    _rejected(c, exp, bufs, "OUTSIDE the form's written set|x its bound")


def test_mutation_headmajor_head_stride_n():
    c = Case("hm", 512, 256, 128, hm=(32, 256), bias=True, outT=True, seed=3)
    inp, exp, bufs = _setup(c)
    D, L = c.hm
    good = bufs["outT"][GUARD:-GUARD].clone()
    r, n = torch.arange(c.M)[:, None], torch.arange(c.N)[None, :]
    right = ((r // L) * (c.N // D) + n // D) * (L * D) + (r % L) * D + n % D
    wrong = ((r // L) * (c.N // D) + n // D) * c.N + (r % L) * D + n % D      # head stride N instead of hm_L * hm_D
    assert int(wrong.max()) < c.M * c.N and wrong.unique().numel() < c.M * c.N   # heads overlap: some element is lost
    out = torch.full_like(good, CANARY)
    out[wrong.reshape(-1)] = good[right.reshape(-1)]
    bufs["outT"][GUARD:-GUARD] = out
    _rejected(c, exp, bufs, "x its bound")


def test_mutation_canary_overwritten_and_written_element_left_at_canary():
    c = _case_of("strides", lambda c: c.out32)
    for name in ("out32", "outT"):
        for i in (0, GUARD - 1, -1, -GUARD):
            inp, exp, bufs = _setup(c)
            bufs[name][i] = 0.0
            _rejected(c, exp, bufs, "guard band")
        inp, exp, bufs = _setup(c)
        i = GUARD + c.N   # the first padding column of row 0
        assert not bool(exp[name][2][i])
        bufs[name][i] = 1.0
        _rejected(c, exp, bufs, "padding column")
        inp, exp, bufs = _setup(c)
        i = int(exp[name][2].nonzero()[37])
        bufs[name][i] = CANARY
        _rejected(c, exp, bufs, "x its bound")


def test_mutation_statistics_partial_in_the_next_slot():
    c = _case_of("rms_producer", lambda c: c.out32 and c.M == 21)
    inp, exp, bufs = _setup(c)
    img, bnd, _ = exp["ssq_out"]
    parts = c.N // 32
    ok = False
    for r in range(c.M):   # a row whose neighbouring partials differ by more than twice the bound: the reference guarantees rejection
        i = GUARD + r * parts
        if abs(float(img[i] - img[i + 1])) >= 2 * float(bnd[i + 1]) + 1e-6 * abs(float(img[i])):
            ok = True
            break
    assert ok
    bufs["ssq_out"][i + 1] = bufs["ssq_out"][i]
    _rejected(c, exp, bufs, "x its bound")
