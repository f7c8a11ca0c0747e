"""Sampling controls and action scoring (vima_action_select_ex / vima_act_ex, act_sample_kernel) without a GPU: the C ABI declares,
exports and binds the two functions, the Python surface exists, the fp64 reference of tests/act_sampling_reference.py checks itself,
the comparisons of tests/test_act_sampling_gpu.py leave out at most 1 % of their (row, dimension) pairs on each of the 192 input
combinations, an fp32 emulation of the kernel's arithmetic stays within a quarter of the statistics gate, and the kernel
cross-compiles for gfx950 without scratch."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vima_amd import _lib
from tests import act_reference as ref
from tests import act_sampling_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
NEW = ("vima_action_select_ex", "vima_act_ex")
CONTROLS = ("temperature", "top_k", "top_p", "n_samples")


def _header():
    with open(os.path.join(ROOT, "include", "vima_hip.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", NEW)
def test_header_library_and_binding_agree(name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.M | re.S)
    assert m, f"{name} is not declared in include/vima_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    assert name in _lib.PROTOTYPES, f"{name} missing from _lib.PROTOTYPES"
    res, args = _lib.PROTOTYPES[name]
    assert res is ctypes.c_int and len(args) == len(params), (params, args)
    for p, a in zip(params, args):       # ints are ints, everything else a pointer-sized argument
        is_int = re.match(r"^int\s+\w+$", p) is not None
        assert (a is ctypes.c_int) == is_int, (name, p, a)
        if "VimaSampleOpts" in p:
            assert a is ctypes.POINTER(_lib.VimaSampleOpts)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), f"{_lib.LIB_PATH} does not export {name}"
    assert _lib.load().vima_abi_version() == 5 == _lib.ABI_VERSION       # additive: the version stays


def test_sample_opts_struct_mirrors_the_header():
    m = re.search(r"typedef struct VimaSampleOpts \{(.*?)\} VimaSampleOpts;", _header(), flags=re.S)
    assert m, "VimaSampleOpts is not declared in include/vima_hip.h"
    fields = re.findall(r"^\s*(const float\*|int|float)\s+(\w+);", m.group(1), flags=re.M)
    ctype = {"const float*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.VimaSampleOpts._fields_)
    assert [n for _, n in fields] == ["temperature", "top_k", "top_p", "n_samples", "given"]


def test_python_surface():
    from vima_amd.policy import VIMAPolicy
    from vima_amd import baselines, actions
    sig = inspect.signature(VIMAPolicy.act)
    for name in CONTROLS:
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert (sig.parameters["temperature"].default, sig.parameters["top_k"].default, sig.parameters["top_p"].default,
            sig.parameters["n_samples"].default) == (None, 0, 1.0, 1)
    ev = inspect.signature(VIMAPolicy.evaluate_actions)
    assert list(ev.parameters)[:3] == ["self", "predicted_action_tokens", "actions"]
    for name in CONTROLS[:3]:
        assert ev.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    for cls in baselines.BASELINES.values():
        assert cls.act is VIMAPolicy.act and cls.evaluate_actions is VIMAPolicy.evaluate_actions
    sel = inspect.signature(actions.select_actions)
    assert list(sel.parameters)[:3] == ["logits", "uniforms", "action_bounds"]
    for name in CONTROLS:
        assert sel.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    sc = inspect.signature(actions.score_actions)
    assert list(sc.parameters)[:2] == ["logits", "actions"]
    for name in CONTROLS[:3] + ("action_bounds",):
        assert sc.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert actions.sample_opts(None, 0, 1.0, 1, (3,), "cpu") == (None, None)      # all defaults: the old entry points
    pol = VIMAPolicy(embed_dim=256, xf_n_layers=1, sattn_n_heads=8, xattn_n_heads=8)
    with pytest.raises(RuntimeError):      # no weights (and no GPU here): refuses, no fallback
        pol.evaluate_actions(np.zeros((1, 256), dtype=np.float32), {})


def test_exemption_budget_on_every_combination():
    """At most 1 % of the (row, dimension) pairs of each of the 192 combinations are left out of the comparisons."""
    worst, where, total = 0.0, None, 0
    for c in sref.combinations():
        e = sref.combination(*c)["exempt"]
        total += int(e.sum())
        if e.mean() > worst:
            worst, where = float(e.mean()), c
        assert e.mean() <= 0.01, (c, e.mean())
    print(f"[act-sampling] exemptions: {total} pairs over {len(sref.combinations())} combinations of {sref.ROWS * 12}; "
          f"worst {100 * worst:.3f} % at {where}")
    assert len(sref.combinations()) == 192


@pytest.mark.parametrize("scale", sref.SCALES)
def test_reference_defaults_are_the_act_reference(scale):
    x, u = sref.logits("random", scale), sref.uniforms()
    r = sref.reference(x, u)
    b64, exempt = ref.sample_bins64(x, u)
    assert np.array_equal(r["bins"], b64) and np.array_equal(r["exempt"], exempt)
    lp, en = ref.stats64(x, b64)
    assert np.abs(r["log_prob"] - lp).max() <= 1e-12 and np.abs(r["entropy"] - en).max() <= 1e-12
    assert all(k.all() for k in r["keep"])
    m = sref.reference(x)                                  # no uniforms: the mode
    assert np.array_equal(m["bins"], ref.argmax_bins(x))
    g = sref.reference(x, given=b64 + 1000)                # given bins are clamped
    assert np.array_equal(g["bins"], np.broadcast_to(np.array(ref.BINS) - 1, b64.shape))


@pytest.mark.parametrize("kind,scale", sref.INPUTS)
def test_reference_top1_is_the_argmax_and_kept_sets_are_monotone(kind, scale):
    x, u = sref.logits(kind, scale), sref.uniforms()
    for tname in sref.TEMPERATURES:
        T = sref.temperature(tname)
        assert np.array_equal(sref.combination(kind, scale, tname, 1, 1.0)["bins"], ref.argmax_bins(sref.scaled(x, T)))
        if tname != "mix":
            continue
        for d, zs in list(enumerate(ref.segments(sref.scaled(x, T))))[:2]:      # one 50-bin and one 100-bin segment
            prev = None
            for k in (1, 2, 5, 10, 49, 50, 99, 100, 0):    # growing k (0 = everything)
                keep, _ = sref.kept_set(zs, k, 1.0)
                assert keep.sum(axis=1).min() == keep.sum(axis=1).max() == (zs.shape[1] if k <= 0 or k >= zs.shape[1] else k)
                assert prev is None or not (prev & ~keep).any(), (d, k)
                prev = keep
            prev = None
            for p in (1e-6, 1e-3, 0.3, 0.5, 0.77, 0.9, 0.999, 1.0):
                keep, _ = sref.kept_set(zs, 10, p)
                assert keep.any(axis=1).all() and (prev is None or not (prev & ~keep).any()), (d, p)
                prev = keep
    for k, p in sref.KP:                                    # every selected bin is in the kept set
        r = sref.combination(kind, scale, "mix", k, p)
        for d in range(12):
            assert np.take_along_axis(r["keep"][d], r["bins"][:, d:d + 1], axis=1).all()


@pytest.mark.parametrize("scale", sref.SCALES)
def test_reference_kept_set_is_the_sorted_one_without_ties(scale):
    x = sref.logits("random", scale)
    for tname in sref.TEMPERATURES:
        z = sref.scaled(x, sref.temperature(tname))
        for d, zs in enumerate(ref.segments(z)):
            assert all(len(np.unique(row)) == len(row) for row in zs), "the random inputs are tie-free"
            for k, p in sref.KP:
                assert np.array_equal(sref.kept_set(zs, k, p)[0], sref.kept_set_by_sorting(zs, k, p)), (tname, d, k, p)


def test_quantised_inputs_have_ties():
    for s in sref.SCALES:
        zs = ref.segments(sref.logits("quantised", s))[1]
        assert any(len(np.unique(row)) < len(row) for row in zs)


@pytest.mark.parametrize("kind,scale", sref.INPUTS)
def test_fp32_arithmetic_stays_within_a_quarter_of_the_statistics_gate(kind, scale):
    """exp, sums, division and log in float32 (the kernel's arithmetic, another summation order) against fp64, per dimension,
    on pairs whose kept set is not decided below fp32 resolution: error <= 0.25 * 2e-5 * max(1, |ref|, max |z|)."""
    x = sref.logits(kind, scale)
    worst = 0.0
    for tname in sref.TEMPERATURES:
        T = sref.temperature(tname)
        for k, p in sref.KP:
            r = sref.combination(kind, scale, tname, k, p)             # shared with the budget test; its exemptions include u's
            lp32, en32, keeps = sref.emulate32(x, T, k, p)
            ok = ~r["exempt"]
            for d in range(12):
                assert np.array_equal(keeps[d][ok[:, d]], r["keep"][d][ok[:, d]]), (tname, k, p, d)
            lp_mode = np.stack([np.log(pi.max(axis=1)) for pi in r["pi"]], axis=1)   # the mode is in K and has the largest pi
            for got, want in ((lp32, lp_mode), (en32, r["entropy_dim"])):
                rel = np.abs(got - want) / (sref.stat_bound(want, r["zmax"]) / sref.STAT_GATE)
                worst = max(worst, float(rel[ok].max()))
    print(f"[act-sampling] fp32 emulation, {kind} scale {scale}: max error {worst:.3e} relative to max(1, |ref|, max |z|) per dimension "
          f"(bound {0.25 * sref.STAT_GATE:.1e})")
    assert worst <= 0.25 * sref.STAT_GATE


@needs_hipcc
def test_act_sample_kernel_compiles_without_scratch():
    """Both instantiations (operand types float and bf16) cross-compile for gfx950 with scratch size 0. Figures of this record
    (ROCm 7.2 hipcc): float 44 VGPRs, bf16 51 VGPRs, 0 AGPRs, 2192 bytes of LDS per block, occupancy 8 waves per SIMD."""
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result",
                          "--cuda-device-only", "-S", os.path.join(ROOT, "vima_amd", "csrc", "action_sample.hip"), "-o", os.devnull,
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
    res = {k: v for k, v in res.items() if "act_sample_kernel" in k}
    assert len(res) == 2, sorted(res)
    assert not any("act_select_kernel" in k for k in res)
    for name, v in res.items():
        print(f"[act-sampling] {name}: {v}")
        assert v.get("ScratchSize", 0) == 0, (name, v)
