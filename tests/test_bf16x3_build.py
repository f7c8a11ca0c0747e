"""Precision "bf16x3" (split-bf16 matrix products on fp32 operands) without a GPU: the public surface accepts it, the Python
enum matches the header, and the two split kernels cross-compile for gfx950 scratch-free, within their register budget, on
the bf16 matrix instruction and never on the fp32 one -- while the fp32 instantiations of the same GEMM body stay on the fp32 one."""
import os
import re
import shutil
import subprocess

import pytest

from vima_amd import _lib
from vima_amd.policy import VIMAPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")


def test_policy_accepts_bf16x3():
    pol = VIMAPolicy(embed_dim=256, xf_n_layers=1, sattn_n_heads=8, xattn_n_heads=8, precision="bf16x3")
    assert pol.precision == "bf16x3"


def test_python_precision_matches_header():
    with open(os.path.join(ROOT, "include", "vima_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"VIMA_PRECISION_BF16X3\s*=\s*(\d+)", hdr)
    assert m, "VIMA_PRECISION_BF16X3 missing from include/vima_hip.h"
    assert _lib.PRECISION["bf16x3"] == int(m.group(1))
    assert len(set(_lib.PRECISION.values())) == len(_lib.PRECISION)


_compiled = {}


def _compile(src):
    if src not in _compiled:
        out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result",
                              "--cuda-device-only", "-S", os.path.join(ROOT, "vima_amd", "csrc", src), "-o", "-",
                              "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        _compiled[src] = (out.stdout, out.stderr)
    return _compiled[src]


def _usage(remarks):
    res, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return res


def _body(asm, name):
    start = re.search(r"^" + re.escape(name) + r":", asm, flags=re.M)
    assert start, name
    return asm[start.end():asm.index("s_endpgm", start.end())]


# The split GEMM is gemm_kernel<float, ..., X3>: the fp32 instantiations (mangled gemm_kernelIf...) whose last two template
# arguments W8, X3 are false, true; X3 = false ends in ...ELb0EEEv.
_GEMM_F32 = r"gemm_kernelIf\S*ELb[01]EEEvNS0_7GemmDevE$"
_GEMM_X3 = r"gemm_kernelIf\S*ELb0ELb1EEEvNS0_7GemmDevE$"
# Likewise the split attention is attn_mfma_kernel<D, MODE, X3 = true>, the single-wave flash kernel (groups: D, X3).
_ATTN_1W = r"16attn_mfma_kernelILi(\d+)ELi\dELb([01])EEEvNS0_7AttnDevE$"
_ATTN_X3 = r"16attn_mfma_kernelILi\d+ELi\dELb1EEEvNS0_7AttnDevE$"


# (source, kernel (regular expression on the mangled name), expected instantiations, VGPR + AGPR budget per lane: 2 waves / SIMD
# for the 256-thread GEMM tile (two workgroups per CU), 2 / SIMD for the single-wave attention kernel)
@needs_hipcc
@pytest.mark.parametrize("src,kernel,count,budget", [pytest.param("gemm.hip", _GEMM_X3, 10, 256, id="gemm.hip-gemm_kernel_X3-10-256"),
                                                     pytest.param("attention.hip", _ATTN_X3, 6, 256, id="attention.hip-attn_mfma_kernel_X3-6-256")])
def test_split_kernels_compile_on_the_bf16_matrix_instruction(src, kernel, count, budget):
    asm, remarks = _compile(src)
    res = {k: v for k, v in _usage(remarks).items() if re.search(kernel, k)}
    assert len(res) == count, sorted(res)
    for name, v in res.items():
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v.get("VGPRs", 0) + v.get("AGPRs", 0) <= budget, (name, v)
        body = _body(asm, name)
        assert "v_mfma_f32_32x32x16_bf16" in body, name
        assert "v_mfma_f32_32x32x2_f32" not in body, name


@needs_hipcc
def test_single_wave_attention_lds_is_one_plane_for_bf16_two_for_x3():
    """X3 is a flag of the one single-wave attention body; its second V^T plane (lo_plane) must exist in the X3 instantiations only.
    Static LDS = D rows of VT_STRIDE = 36 bf16 per plane: 2304 / 4608 bytes for D = 32 / 64, twice that with X3."""
    _, remarks = _compile("attention.hip")
    found = {False: [], True: []}
    for name, v in _usage(remarks).items():
        m = re.search(_ATTN_1W, name)
        if not m:
            continue
        d, x3 = int(m.group(1)), m.group(2) == "1"
        found[x3].append(name)
        assert v.get("ScratchSize") == 0, (name, v)
        assert v.get("LDS") == d * 36 * 2 * (2 if x3 else 1), (name, v)
    assert len(found[False]) == 6 and len(found[True]) == 6, found


@needs_hipcc
def test_fp32_ring_kernels_stay_on_the_fp32_matrix_instruction():
    """The converse: X3 is a flag of the one ring-tile body, so every fp32 instantiation WITHOUT it must still be the exact
    fp32 product."""
    asm, remarks = _compile("gemm.hip")
    f32 = [k for k in _usage(remarks) if re.search(_GEMM_F32, k) and not re.search(_GEMM_X3, k)]
    assert f32, "no fp32 gemm_kernel instantiation found"
    for name in f32:
        body = _body(asm, name)
        assert "v_mfma_f32_32x32x2_f32" in body, name
        assert "v_mfma_f32_32x32x16_bf16" not in body, name
