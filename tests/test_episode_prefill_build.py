"""Episode prefill (vima_decode_chunk, vima_decode_restart_history, vima_decode_history_room) without a GPU: the C ABI declares, exports and
binds the three functions, the Python surface exists, the bookkeeping restatement of tests/episode_prefill_reference.py checks itself, the
schedule of the chunked ring rollout of tests/test_episode_prefill_gpu.py has what the test is about, and the new kernels cross-compile for
gfx950 without scratch."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from vima_amd import _lib
from tests import episode_prefill_reference as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
NEW = ("vima_decode_chunk", "vima_decode_restart_history", "vima_decode_history_room")


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
    assert [len(_lib.PROTOTYPES[n][1]) for n in NEW] == [15, 14, 2]
    assert len(_lib.PROTOTYPES["vima_decode_chunk"][1]) == len(_lib.PROTOTYPES["vima_decode_step"][1]) + 1          # + T
    assert len(_lib.PROTOTYPES["vima_decode_restart_history"][1]) == len(_lib.PROTOTYPES["vima_decode_restart"][1]) + 5


def test_python_surface():
    from vima_amd.policy import VIMAPolicy
    from vima_amd import baselines
    fs = inspect.signature(VIMAPolicy.forward_steps)
    assert list(fs.parameters) == ["self", "obs_token", "obs_mask", "action_token", "prompt_token", "prompt_token_mask", "step"]
    rs = inspect.signature(VIMAPolicy.restart_samples)
    assert list(rs.parameters) == ["self", "restart", "prompt_token", "prompt_token_mask", "history"] and rs.parameters["history"].default is None
    assert list(inspect.signature(VIMAPolicy.history_room).parameters) == ["self"]
    # the baselines: Flamingo through the all-ones-mask wrappers, GPT / Gato refuse and point to seq_*
    base = baselines.VIMAFlamingoPolicy.__mro__[1]
    assert list(inspect.signature(base.forward_steps).parameters) == ["self", "obs_token", "action_token", "prompt_token", "prompt_token_mask", "step"]
    assert inspect.signature(base.restart_samples).parameters["history"].default is None
    for cls in baselines.BASELINES.values():
        assert cls.forward_steps is base.forward_steps and cls.restart_samples is base.restart_samples and cls.history_room is base.history_room
    for cls in (baselines.VIMAGPTPolicy, baselines.VIMAGatoPolicy):
        stub = object.__new__(cls)
        with pytest.raises(NotImplementedError, match="seq_"):
            stub.forward_steps(None, None, None, None, 0)
        with pytest.raises(NotImplementedError, match="seq_"):
            stub.restart_samples(None, None, None, history=(None, None))
        with pytest.raises(NotImplementedError, match="seq_"):
            stub.history_room()
    pol = VIMAPolicy(embed_dim=256, xf_n_layers=1, sattn_n_heads=8, xattn_n_heads=8)
    with pytest.raises(RuntimeError):      # no weights (and no GPU here): refuses, no fallback
        pol.history_room()


def test_the_bookkeeping_restatement_checks_itself():
    """Chunk units reproduce single steps at T = 1, install ages equal a restarted sample's, the room never exceeds what the age rule allows
    (300 random schedules, ring and linear)."""
    n = eref.selfcheck(seed=0, schedules=300)
    print(f"[prefill] bookkeeping restatement: {n} installs checked over 300 schedules")
    assert n > 1000


def test_a_chunk_can_be_refused_where_single_steps_pass():
    """The chunk is one unit: its skipped tail is longer than a step's."""
    book = eref.EpisodeBook(1, 4, 48, True)
    for _ in range(8):
        book.advance(1)            # rows 0 .. 38, age 39
    assert book.steps_left() == [1] and book.plan(1) == (39, 5, 5)
    with pytest.raises(IndexError, match="sample 0"):
        book.plan(2)               # 39 + 10 > 48: skip 9, write 10
    lin = eref.EpisodeBook(1, 4, 48, False)
    for _ in range(7):
        lin.advance(1)
    assert lin.plan(2) == (34, 10, 10)
    with pytest.raises(IndexError, match="room for 2 more steps"):
        lin.plan(3)


def test_the_chunked_ring_schedule_has_what_its_test_is_about():
    """tests/test_episode_prefill_gpu.py, test 3: every call legal, >= 3 wraps, a chunk that skips the tail, a restart right before a chunk."""
    B, Q, npos, steps = 3, 4, 48, 40

    def restarts(t):
        return [t > 0 and t % (3 + b) == 0 for b in range(B)]
    units = eref.chunk_schedule(steps, restarts, every=3, T=2)
    assert sum(T for _, T in units) == steps and [t for t, _ in units] == [sum(T for _, T in units[:i]) for i in range(len(units))]
    book = eref.EpisodeBook(B, Q, npos, True)
    wraps = skip = fresh = 0
    for t, T in units:
        assert not any(any(restarts(t + j)) for j in range(1, T))
        if t > 0:
            book.restart(restarts(t))
        row, lq, adv = book.advance(T)
        wraps, skip, fresh = wraps + (adv > lq), skip + (T > 1 and adv > lq), fresh + (T > 1 and any(restarts(t)))
    assert wraps >= 3 and skip >= 1 and fresh >= 1 and sum(T > 1 for _, T in units) >= 7


@needs_hipcc
def test_new_kernels_compile_without_scratch():
    """Every kernel of the episode prefill, both operand types where it has them, cross-compiles for gfx950 with scratch size 0: those of
    elementwise.hip and the ones the two policy families share (episode_rows.hip; kv_rows_kernel knows no operand type, so it has ONE
    instantiation for the gather, the scatter and the row-map scatter alike). Figures of this record (ROCm 7.2 hipcc), VGPRs / LDS bytes per
    block, all at occupancy 8 waves per SIMD: dec_embed_chunk_kernel 22 / 3072 (float and bf16), gather_pred_kernel (with the lead argument)
    14 / 0, mask_rows_gather_kernel 4 / 0, kv_rows_kernel 8 / 0, episode_restart_kernel 32 / 0, episode_install_kernel 32 / 16."""
    res = {}
    for src in ("elementwise.hip", "episode_rows.hip"):
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
    want = {"dec_embed_chunk_kernel": 2, "gather_pred_kernel": 1, "mask_rows_gather_kernel": 1, "kv_rows_kernel": 1, "episode_restart_kernel": 1,
            "episode_install_kernel": 1}
    for kernel, n in want.items():
        found = {k: v for k, v in res.items() if kernel in k}
        assert len(found) == n, (kernel, sorted(found))
        for name, v in found.items():
            print(f"[prefill] {name}: {v}")
            assert v.get("ScratchSize", 0) == 0, (name, v)
            assert v.get("LDS", 0) <= 3072, (name, v)
