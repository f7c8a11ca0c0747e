"""The fused-RMSNorm consumer form of gemm_q4_kernel's 256x384 tile (gemm_q4_kernel<ACT, 7, 2>, option gemm_q4_rs) through vima_op_gemm.

A lane of that form carries the four row scales of its rows through the K loop in registers, and fetches the NEXT tile's 24 partials per row
while the current tile's epilogue runs. What can go wrong is therefore a scale that belongs to another row, another tile or the previous
launch-state of a register, so the inputs make every such mix-up large: row r of A is scaled by 2^e, e from a permuted cycle of -3 .. 3 with
period 7 -- neighbouring rows, and rows 32, 64, 128 or 256 apart, differ by at least a factor of 2 -- and the partials are those of the
bf16-rounded A, so that a correct launch normalises every row back to O(1) and a wrong scale is off by 2x or more.

Shapes (K = 768 is fixed by the 24 partials; gemm_q4 = 1 lets small problems reach the tile), the smallest that run each path on 256 CUs:
  12 288 x 2304            288 tiles: 32 workgroups take two (prologue, prefetch across an epilogue, no successor), the others one
  8 448 x 3072, ReLU       264 tiles
  33 024 x 2304            774 tiles, three or four per workgroup: a scale that survives a tile too long
  12 288 x 2304, pad rows  the last 256 rows carry all-zero partials (scale = rsqrt(eps))

Checks per case: the output bytes equal the knob-off launch (gemm_pp_kernel) on the same buffers; every element against fp64 with the bound
of tests/gemm_forms_reference.expected (its rms-consumer lines, evaluated on the GPU in fp64 for the whole output and held to
gemm_forms_reference.expected / check themselves on the first and last 64 rows); the canaries around the output stay, the partial buffer
and its canaries are unchanged."""
import ctypes

import pytest
import torch

from vima_amd import _lib
from tests import gemm_forms_reference as R
from tests.gpu_common import bare_policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, PARTS = 768, 24
CYCLE = (3, 0, 5, 1, 6, 2, 4)   # exponent + 3 of row r: CYCLE[r % 7]
CASES = [("12288x2304", 12288, 2304, R.ACT_NONE, 0), ("8448x3072 relu", 8448, 3072, R.ACT_RELU, 0), ("33024x2304", 33024, 2304, R.ACT_NONE, 0),
         ("12288x2304 pad rows", 12288, 2304, R.ACT_NONE, 256)]


def _inputs(M, N, pad, seed):
    g = torch.Generator().manual_seed(seed)
    e = torch.tensor(CYCLE, dtype=torch.float32)[torch.arange(M) % 7] - 3.0
    A = ((torch.rand(M, K, generator=g) * 2 - 1) * torch.exp2(e)[:, None]).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    ssq = A.float().reshape(M, PARTS, K // PARTS).pow(2).sum(-1)
    if pad:
        ssq[M - pad:] = 0.0
        A[M - pad:] = (A[M - pad:].float() * 2.0 ** -11).to(torch.bfloat16)   # rsqrt(eps) = 316: keeps the pad rows' outputs O(1)
    return A.to(DEV), W.to(DEV), ssq.to(DEV)


def _expected_gpu(A, W, ssq, act):
    """gemm_forms_reference.expected for Case(rs="rms", outT=True, act) without bias: fp64 image and per-element bound, on the GPU."""
    a, w = A.double(), W.double()
    P, S = a @ w.T, a.abs() @ w.abs().T
    e = S * (R.C_ACC * R.U24)
    rsc = (ssq.double().sum(1) * (1.0 / K) + 1e-5).rsqrt()[:, None]
    v = P * rsc
    e = e * rsc + v.abs() * ((PARTS + 4) * R.U24 + R.U24)
    if act:
        e = R.LIPSCHITZ[act] * e + R.ACT_ERR.get(("bf16", act), 0.0) * v.abs().clamp_min(1.0)
        v = R.act64(v, act)
        e = e + R.U24 * v.abs()
    return v, e + R.UBF * v.abs()


def _launch(pol, A, W, part_buf, out_buf, M, N, act):
    d = _lib.VimaGemmDesc()
    d.A, d.W = A.data_ptr(), W.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldw, d.batch, d.act = M, N, K, K, K, 1, act
    d.rs_ssq = part_buf.data_ptr() + R.GUARD * 4
    d.rs_parts, d.rs_invk, d.rs_eps = PARTS, 1.0 / K, 1e-5
    d.outT, d.ldT = out_buf.data_ptr() + R.GUARD * 2, N
    kid = ctypes.c_int(0)
    rc = pol._lib.vima_op_gemm(pol._handle, ctypes.byref(d), ctypes.byref(kid), pol._stream())
    torch.cuda.synchronize()
    return rc, kid.value


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_rms_consumer_on_the_256x384_tile(i):
    name, M, N, act, pad = CASES[i]
    pol = bare_policy("bf16")
    A, W, ssq = _inputs(M, N, pad, 77 + i)
    part_buf = torch.full((2 * R.GUARD + M * PARTS,), R.CANARY, dtype=torch.float32, device=DEV)
    part_buf[R.GUARD:R.GUARD + M * PARTS] = ssq.reshape(-1)
    part_ref = part_buf.clone()
    outs = {}
    try:
        pol.set_option("gemm_q4", 1)
        for knob in (0, 1):
            pol.set_option("gemm_q4_rs", knob)
            out = torch.full((2 * R.GUARD + M * N,), R.CANARY, dtype=torch.bfloat16, device=DEV)
            rc, kid = _launch(pol, A, W, part_buf, out, M, N, act)
            assert rc == 0, f"{name}: refused with gemm_q4_rs = {knob}: {pol._lib.vima_last_error().decode()}"
            assert kid == (19000 + (act + 1) * 10 + 7 if knob else 1000 + (act + 1) * 10 + 1), (name, knob, kid)
            outs[knob] = out
    finally:
        pol.set_option("gemm_q4_rs", -1)
        pol.set_option("gemm_q4", -1)
    assert torch.equal(part_buf.view(torch.int32), part_ref.view(torch.int32)), f"{name}: the partial buffer or its canaries changed"
    got = outs[1]
    for knob, out in outs.items():
        guards = torch.cat([out[:R.GUARD], out[-R.GUARD:]])
        assert bool((guards == R.CANARY).all()), f"{name}: gemm_q4_rs = {knob} wrote outside the output"
    body = got[R.GUARD:-R.GUARD].reshape(M, N)
    ref_body = outs[0][R.GUARD:-R.GUARD].reshape(M, N)
    diff = body.view(torch.int16) != ref_body.view(torch.int16)
    if bool(diff.any()):
        r, c = [int(x) for x in diff.nonzero()[0]]
        raise AssertionError(f"{name}: {int(diff.sum())} elements differ from gemm_pp_kernel's, first at row {r} (tile row {r // 256}, row in tile "
                             f"{r % 256}), column {c}: {body[r, c].item()} vs {ref_body[r, c].item()}; rows affected {int(diff.any(1).sum())}")
    v, bnd = _expected_gpu(A, W, ssq, act)
    assert bool(torch.isfinite(body).all()), name
    ratio = (body.double() - v).abs() / bnd.clamp_min(1e-300)
    worst = ratio.max().item()
    print(f"[q4 rms consumer] {name}: worst |err| / bound {worst:.3f} over {M * N} elements, max |out| {body.abs().max().item():.3g}")
    if worst > 1.0:
        r, c = divmod(int(ratio.argmax()), N)
        raise AssertionError(f"{name}: out[{r}][{c}] = {body[r, c].item()!r}, reference {v[r, c].item()!r}: {worst:.2f} x its bound; "
                             f"{int((ratio > 1).sum())} elements over their bound")
    # the GPU-side image and bound ARE gemm_forms_reference's: its own expected / check on the first and the last 64 rows
    for r0 in (0, M - 64):
        c = R.Case(f"{name} rows {r0}..", 64, N, K, rs="rms", rs_parts=PARTS, act=act, outT=True)
        inp = {"A": A[r0:r0 + 64].cpu()[None], "W": W.cpu()[None], "rs_ssq": ssq[r0:r0 + 64].cpu()}
        exp, _ = R.expected(c, inp)
        img, b, wr = exp["outT"]
        sl = slice(R.GUARD, R.GUARD + 64 * N)
        assert torch.allclose(img[sl], v[r0:r0 + 64].reshape(-1).cpu(), rtol=1e-12, atol=1e-300)
        assert torch.allclose(b[sl], bnd[r0:r0 + 64].reshape(-1).cpu(), rtol=1e-9, atol=1e-300)
        buf = torch.full((img.numel(),), R.CANARY, dtype=torch.bfloat16)
        buf[sl] = body[r0:r0 + 64].reshape(-1).cpu()   # (expected() allots two canary rows behind the last one)
        R.check(c, exp, {"outT": buf})
