"""Episode prefill of the decoder-only baselines (vima_seq_decode_chunk, vima_seq_decode_restart_history, vima_seq_history_room) without a GPU:
the C ABI declares, exports and binds the three functions and the two operator entries, the Python surface exists, the bookkeeping restatement
of tests/seq_prefill_reference.py checks itself, the chunked ring schedule of tests/test_seq_prefill_gpu.py has what that test is about, and the
new kernels cross-compile for gfx950 without scratch."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from oracle.cases import BASELINE_CASES
from tests import seq_prefill_reference as sp
from tests import seq_ring_reference as rr
from vima_amd import _lib
from vima_amd.policy import build_prompt_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
NEW = ("vima_seq_decode_chunk", "vima_seq_decode_restart_history", "vima_seq_history_room", "vima_op_seq_embed_chunk", "vima_op_seq_history_install")


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
    for p, a in zip(params, args):       # ints are ints, strides 64-bit, everything else a pointer-sized argument
        is_int = re.match(r"^int\s+\w+$", p) is not None
        assert (a is ctypes.c_int) == is_int, (name, p, a)
        if p.startswith("int64_t "):
            assert a is ctypes.c_int64, (name, p, a)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), f"{_lib.LIB_PATH} does not export {name}"
    assert _lib.load().vima_abi_version() == 5 == _lib.ABI_VERSION       # additive: the version stays


def test_arities():
    assert [len(_lib.PROTOTYPES[n][1]) for n in NEW] == [8, 13, 2, 17, 13]
    assert len(_lib.PROTOTYPES["vima_seq_decode_chunk"][1]) == len(_lib.PROTOTYPES["vima_seq_decode_step"][1]) + 1                    # + T
    assert len(_lib.PROTOTYPES["vima_seq_decode_restart_history"][1]) == len(_lib.PROTOTYPES["vima_seq_decode_restart"][1]) + 4      # + obs, act, T, out
    assert len(_lib.PROTOTYPES["vima_op_seq_embed_chunk"][1]) == len(_lib.PROTOTYPES["vima_op_seq_embed_step"][1]) + 1               # + T


def test_python_surface():
    from vima_amd import baselines
    base = baselines.VIMAFlamingoPolicy.__mro__[1]
    assert list(inspect.signature(base.seq_steps).parameters) == ["self", "obs_token", "action_token"]
    assert inspect.signature(base.seq_steps).parameters["action_token"].default is None
    rs = inspect.signature(base.seq_restart)
    assert list(rs.parameters) == ["self", "restart", "prompt_token", "prompt_token_mask", "history"] and rs.parameters["history"].default is None
    assert list(inspect.signature(base.seq_history_room).parameters) == ["self"]
    for cls in baselines.BASELINES.values():
        assert cls.seq_steps is base.seq_steps and cls.seq_restart is base.seq_restart and cls.seq_history_room is base.seq_history_room
    fl = object.__new__(baselines.VIMAFlamingoPolicy)          # Flamingo decodes with XAttnGPT: the three refuse through _seq_only
    for call in (lambda: fl.seq_steps(None), lambda: fl.seq_restart(None, None, None, history=(None, None)), lambda: fl.seq_history_room()):
        with pytest.raises(NotImplementedError, match="decoder-only"):
            call()
    for cls in (baselines.VIMAGPTPolicy, baselines.VIMAGatoPolicy):   # the XAttnGPT names still refuse and now name their seq_* twins
        stub = object.__new__(cls)
        with pytest.raises(NotImplementedError, match="seq_steps"):
            stub.forward_steps(None, None, None, None, 0)
        with pytest.raises(NotImplementedError, match=r"seq_restart\(history=\)"):
            stub.restart_samples(None, None, None, history=(None, None))
        with pytest.raises(NotImplementedError, match="seq_history_room"):
            stub.history_room()
        for call in (lambda: stub.forward_steps(None, None, None, None, 0), lambda: stub.restart_samples(None, None, None, history=(None, None)),
                     lambda: stub.history_room()):
            with pytest.raises(NotImplementedError, match="seq_"):
                call()


def test_the_bookkeeping_restatement_checks_itself():
    """T = 1 units reproduce Ring.step, install ages equal a restarted sample's, the room never maps a history onto a row overwritten or skipped
    since, a history's rows are distinct (300 random schedules, ring and linear)."""
    n = sp.selfcheck(seed=0, schedules=300)
    print(f"[seq_prefill] bookkeeping restatement: {n} installs checked over 300 schedules")
    assert n > 1000


def test_a_chunk_can_be_refused_where_single_steps_pass():
    """The chunk is one unit: its skipped tail is longer than a step's. Lp = 3: P0 = 4, R = 48."""
    book = sp.SeqBook(3, 52, 4, 1, True)
    for _ in range(8):
        book.advance(1)            # rows 4 .. 42, age 39
    assert book.steps_left() == [1] and book.plan(1) == (43, 5, 5)
    with pytest.raises(IndexError, match="sample 0"):
        book.plan(2)               # 43 + 10 > 52: skip 9, write 10 -> 39 + 19 > 48
    lin = sp.SeqBook(3, 52, 4, 1, False)
    for _ in range(7):
        lin.advance(1)
    assert lin.plan(2) == (38, 10, 10)
    with pytest.raises(IndexError, match="room for 2 more steps"):
        lin.plan(3)


@pytest.mark.parametrize("kind,wraps", [("gato", 3), ("gpt", 4)])
def test_the_chunked_ring_schedule_has_what_its_test_is_about(kind, wraps):
    """tests/test_seq_prefill_gpu.py, test 3: every call legal, the wraps, 4 chunks, one of which skips the tail, each right behind a restart; on the
    rings of tests/seq_ring_reference.py (90 / 9) the same schedule is refused at step 7."""
    Lp = build_prompt_index(BASELINE_CASES["baseline_gato"]["layout"], sp.Q[kind])[1]
    u = sp.units()
    assert sum(T for _, T in u) == sp.STEPS and [t for t, _ in u] == [sum(T for _, T in u[:i]) for i in range(len(u))]
    assert not any(any(sp.restarts(t + j)) for t, T in u for j in range(1, T))
    p = sp.chunked_ring_properties(kind, Lp)
    assert p["legal"] and (p["wraps"], p["chunks"], p["chunk_skips"], p["chunk_fresh"]) == (wraps, 4, 1, 4), p
    old = sp.chunked_ring_properties(kind, Lp, rr.RING[kind])
    assert not old["legal"] and old["refused_at"] == 7


@needs_hipcc
def test_new_kernels_compile_without_scratch():
    """The kernels of the baselines' episode prefill cross-compile for gfx950 with scratch size 0: those of baseline_kernels.hip and the history
    install both policy families share (episode_rows.hip). Figures of this record (ROCm 7.2 hipcc), VGPRs / LDS bytes per block:
    seq_embed_chunk_kernel 31 / 0 (float and bf16); episode_install_kernel 32 / 16; seq_embed_kernel (with the list and the episode-state
    arguments: it is the prefill too) 26 / 0 (float and bf16)."""
    res = {}
    for src in ("baseline_kernels.hip", "episode_rows.hip"):
        out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result",
                              "--cuda-device-only", "-S", os.path.join(ROOT, "vima_amd", "csrc", src), "-o", os.devnull,
                              "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        name = None
        for line in out.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                res[name] = {}
                continue
            m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and name:
                res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    want = {"seq_embed_chunk_kernel": 2, "episode_install_kernel": 1, "16seq_embed_kernel": 2}
    for kernel, n in want.items():
        found = {k: v for k, v in res.items() if kernel in k}
        assert len(found) == n, (kernel, sorted(found))
        for name, v in found.items():
            print(f"[seq_prefill] {name}: {v}")
            assert v.get("ScratchSize", 0) == 0, (name, v)
            assert v.get("LDS", 0) <= 64, (name, v)
