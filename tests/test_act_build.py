"""On-device action selection (vima_action_select / vima_act, act_select_kernel) without a GPU: the C ABI declares, exports and
binds the two functions, the kernel cross-compiles for gfx950 scratch-free inside its register budget, and the comparisons of
tests/test_act_gpu.py leave out at most 1 % of their (row, dimension) pairs on the inputs they use."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vima_amd import _lib
from tests import act_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
NEW = ("vima_action_select", "vima_act")


def _declaration(name):
    with open(os.path.join(ROOT, "include", "vima_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/vima_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW)
def test_header_library_and_binding_agree(name):
    params = _declaration(name)
    assert name in _lib.PROTOTYPES, f"{name} missing from _lib.PROTOTYPES"
    res, args = _lib.PROTOTYPES[name]
    assert res is ctypes.c_int and len(args) == len(params), (params, args)
    for p, a in zip(params, args):       # ints are ints, everything else a pointer-sized argument
        is_int = re.match(r"^int\s+\w+$", p) is not None
        assert (a is ctypes.c_int) == is_int, (name, p, a)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), f"{_lib.LIB_PATH} does not export {name}"
    assert _lib.load().vima_abi_version() == 5 == _lib.ABI_VERSION       # additive: the version stays


def test_policy_classes_have_act():
    from vima_amd.policy import VIMAPolicy
    from vima_amd import baselines, actions
    assert callable(getattr(VIMAPolicy, "act", None))
    for cls in baselines.BASELINES.values():
        assert cls.act is VIMAPolicy.act
    assert callable(actions.select_actions)
    pol = VIMAPolicy(embed_dim=256, xf_n_layers=1, sattn_n_heads=8, xattn_n_heads=8)
    with pytest.raises(RuntimeError):      # no weights (and no GPU here): refuses, no fallback
        pol.act(np.zeros((1, 256), dtype=np.float32))


def test_bounds_argument():
    from vima_amd.actions import bounds_array
    assert bounds_array(None) is None
    b = bounds_array({"low": np.array([0.25, -0.5], dtype=np.float32), "high": [0.75, 0.5]})
    assert list(b) == [0.25, -0.5, 0.75, 0.5]
    with pytest.raises(ValueError):
        bounds_array({"low": [0.0, 0.0, 0.0], "high": [1.0, 1.0, 1.0]})


@needs_hipcc
def test_act_select_kernel_resources():
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result",
                          "--cuda-device-only", "-S", os.path.join(ROOT, "vima_amd", "csrc", "action_select.hip"), "-o", "-",
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    res = {k: v for k, v in res.items() if "act_select_kernel" in k}
    assert len(res) == 2, sorted(res)                       # operand types float and bf16
    for name, v in res.items():
        assert v.get("ScratchSize", 0) == 0, (name, v)
        assert v.get("VGPRs", 0) + v.get("AGPRs", 0) <= 64, (name, v)
        assert v.get("LDS", 0) <= 1024, (name, v)
    asm = out.stdout
    for name in res:                                        # wave reductions only: no atomics, no scratch traffic
        start = re.search(r"^" + re.escape(name) + r":", asm, flags=re.M)
        body = asm[start.end():asm.index("s_endpgm", start.end())]
        assert "atomic" not in body and "scratch_" not in body, name
        assert body.count("s_barrier") == 1, name


def test_mode_exemption_budget():
    """Pairs whose two largest golden logits are within 1e-6 of each other are left out of the comparison with the reference's
    argmax(probs): at most 1 % of the golden pairs, none of the random ones."""
    total = exempt = 0
    for name in ref.GOLDENS:
        x, _ = ref.golden_logits(name)
        e = ref.mode_exempt(x)
        total += e.size
        exempt += int(e.sum())
    print(f"[act] mode comparison: {exempt} of {total} golden (row, dimension) pairs exempt")
    assert exempt <= 0.01 * total
    for s in ref.SCALES:
        assert not ref.mode_exempt(ref.random_logits(s)).any()


@pytest.mark.parametrize("scale", ref.SCALES)
def test_sampling_exemption_budget_and_fp32_cumsum(scale):
    """u within 1e-5 of an fp64 cumulative boundary is left out: at most 1 % of the pairs; everywhere else a sequential fp32
    cumulative sum already gives the fp64 bin, so an fp32 kernel can be held to it."""
    x, u = ref.random_logits(scale), ref.random_uniforms()
    b64, exempt = ref.sample_bins64(x, u)
    b32 = ref.sample_bins32_sequential(x, u)
    print(f"[act] sampling at logit scale {scale}: {int(exempt.sum())} of {exempt.size} pairs exempt ({100.0 * exempt.mean():.3f} %), "
          f"fp32 sequential cumsum differs on {int((b32 != b64).sum())} pairs, {int(((b32 != b64) & ~exempt).sum())} of them outside")
    assert exempt.mean() <= 0.01
    assert not ((b32 != b64) & ~exempt).any()
    assert b64.min() >= 0 and (b64 < np.array(ref.BINS)).all()
