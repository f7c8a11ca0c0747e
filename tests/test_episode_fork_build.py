"""Branch rollouts (vima_decode_fork / vima_seq_decode_fork / vima_op_episode_fork, episode_fork_kernel) without a GPU: the fork bookkeeping of
vima_amd/csrc/episode_book.h (fork_ok, fork, live_ranges) in a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/episode_book_driver.cpp, built by tests/episode_driver.py) against the brute-force restatement of
tests/episode_fork_reference.py over 300 random schedules; the C ABI declares, exports and binds the three functions; the Python surface; the
kernel cross-compiles for gfx950 without scratch; and the scenario of tests/test_episode_fork_gpu.py contains the forks it is about."""
import ctypes
import functools
import inspect
import os
import random
import re
import shutil
import subprocess

import pytest

from vima_amd import _lib
from tests import episode_driver
from tests import episode_fork_reference as fref
from tests.episode_driver import ROOT, _ints, driver  # noqa: F401

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
NEW = ("vima_decode_fork", "vima_seq_decode_fork", "vima_op_episode_fork")
_run = functools.partial(episode_driver._run, brief=True)


class _Script:
    """Operations for the driver next to what the restatement expects: an exact line, or a check of the `ranges` line against the book's state"""

    def __init__(self):
        self.ops, self.want = [], []

    def add(self, op, want):
        self.ops.append(op)
        self.want.append(want)

    def after(self, bk):
        """what the issue compares after every fork and unit: ranges vs live rows, ages and steps_left"""
        snap = dict(P0=bk.P0, hw=bk.hw, wp=bk.wp, ring=bk.ring, age=list(bk.age), live=[bk.live_rows(b) for b in range(bk.B)])
        self.add("ranges", snap)
        self.add("state", f"state {bk.wp} {bk.hw} {bk.next} {bk.hw if bk.ring else bk.wp} ages " + _ints(bk.age))
        self.add("left", "left " + _ints(bk.steps_left(b) for b in range(bk.B)))

    def check(self, exe):
        got = _run(exe, self.ops)
        stats = dict(two_ranges=0, ranges=0, superset_rows=0)
        for i, (op, want, g) in enumerate(zip(self.ops, self.want, got)):
            where = f"operation {i} `{op}`: the program says `{g}`; before it: {self.ops[max(0, i - 10):i]}"
            if isinstance(want, str):
                assert g == want, where + f"; the restatement `{want}`"
                continue
            parts = g.split("|")
            assert parts[0].strip() == "ranges" and len(parts) == 1 + len(want["age"]), where
            for b, part in enumerate(parts[1:]):
                v = [int(x) for x in part.split()]
                rg = list(zip(v[0::2], v[1::2]))
                assert len(v) % 2 == 0 and len(rg) <= 2, where
                covered = set()
                for lo, hi in rg:
                    assert want["P0"] <= lo < hi <= (want["hw"] if want["ring"] else want["wp"]), (where, b, rg, want)   # inside [P0, written_end)
                    assert not (covered & set(range(lo, hi))), (where, b, rg)                                        # disjoint
                    covered |= set(range(lo, hi))
                assert covered >= want["live"][b], (where, b, rg, sorted(want["live"][b]))
                assert len(covered) <= want["age"][b], (where, b, rg, want["age"][b])
                assert want["age"][b] > 0 or not rg, (where, b)
                stats["two_ranges"] += len(rg) == 2
                stats["ranges"] += len(rg)
                stats["superset_rows"] += len(covered - want["live"][b])
        return stats


def _random_source(rng, B):
    """a legal source map: some samples are sources of some of the others"""
    order = list(range(B))
    rng.shuffle(order)
    n_src = rng.randint(1, max(1, B // 2))
    srcs, source = order[:n_src], list(range(B))
    for b in order[n_src:]:
        if rng.random() < 0.6:
            source[b] = rng.choice(srcs)
    return source


def _schedules(seq, seed=0, schedules=300):
    rng = random.Random(seed + (1000 if seq else 0))
    sc = _Script()
    seen = dict(ring=0, linear=0, forks=0, multi_dst=0, installs=0, wraps=0, fork_age0=0)
    for k in range(schedules):
        B, Q, ring = rng.randint(1, 5), rng.randint(1, 6), k % 4 != 0
        if seq:
            Lp = rng.randint(1, 9)
            P0, Lmax = Lp + 1, Lp + 1 + rng.randint(3 * (Q + 1), 96)
        else:
            P0, Lmax = 0, rng.randint(24, 96)
        bk = fref.Book(B, Q, P0, Lmax, ring)
        seen["ring" if ring else "linear"] += 1
        sc.add(f"begin {B} {Q} {P0} {Lmax} {int(ring)}", "ok")
        sc.after(bk)
        for _ in range(rng.randint(5, 60)):
            flags = [rng.random() < 0.2 for _ in range(B)]
            if ring:
                flags = [f or bk.steps_left(b) == 0 for b, f in enumerate(flags)]
            if any(flags):
                bk.restart(flags)
                sc.add("restart " + _ints(flags), "ok")
                sc.after(bk)
            if bk.room() >= 1 and rng.random() < 0.3:
                T, fl = rng.randint(1, bk.room()), [rng.random() < 0.5 for _ in range(B)]
                bk.install(fl, T)
                sc.add(f"install {T} " + _ints(fl), f"install {sum(bk.adv[len(bk.adv) - T:])}")
                sc.after(bk)
                seen["installs"] += 1
            if rng.random() < 0.5:
                source = _random_source(rng, B)
                seen["fork_age0"] += any(s != b and bk.age[s] == 0 for b, s in enumerate(source))
                seen["multi_dst"] += any(sum(1 for b, s in enumerate(source) if s == x and b != x) >= 2 for x in range(B))
                bk.fork(source)
                sc.add("fork " + _ints(source), "ok")
                sc.after(bk)
                seen["forks"] += 1
            out = [ring and bk.steps_left(b) == 0 for b in range(B)]     # an install or a fork may have brought an old episode back
            if any(out):
                bk.restart(out)
                sc.add("restart " + _ints(out), "ok")
            T = rng.choice([1, 1, 2, 3])
            p = bk.step(T)
            sc.add(f"step {T}", "refused" if p is None else f"plan {p[0]} {p[1]} {p[2]}")
            sc.after(bk)
            if p is None:
                if T == 1:
                    assert not ring, "ring: every sample out of steps was restarted, a single step must pass"
                    break
                continue
            seen["wraps"] += p[2] > p[1]
    return sc, seen


@pytest.mark.parametrize("seq", [False, True], ids=["P0=0", "P0=Lp+1"])
def test_random_schedules_with_forks(driver, seq):
    sc, seen = _schedules(seq)
    stats = sc.check(driver)                                    # all 300 schedules through one child process
    print(f"[episode-fork] {seen}, {stats}")
    assert seen["ring"] == 225 and seen["linear"] == 75
    assert seen["forks"] > 1000 and seen["multi_dst"] >= 50 and seen["installs"] >= 100 and seen["wraps"] >= 50 and seen["fork_age0"] >= 20, seen
    assert stats["two_ranges"] >= 50, stats


def test_fork_ok(driver):
    ops = ["begin 4 2 0 40 1",
           "forkok 0 1 2 3",            # identity
           "forkok 0 0 0 3",            # one source, two destinations
           "forkok 1 1 3 3",            # two groups
           "forkok 1 2 2 3",            # chain: 0 <- 1 <- 2
           "forkok 1 0 2 3",            # swap
           "forkok 0 1 2 4",            # out of range
           "forkok 0 -1 2 3",
           "forkok 0 1 2",              # wrong length
           "forkok 0 1 2 3 0",
           "fork 1 0 2 3", "state",     # a refused map changes nothing
           "fork 3 3 3 3", "state"]
    got = _run(driver, ops)
    assert got[1:10] == ["forkok 1", "forkok 1", "forkok 1", "forkok 0", "forkok 0", "forkok 0", "forkok 0", "forkok 0", "forkok 0"]
    assert got[10] == "refused" and got[11] == "state 0 0 0 0 ages 0 0 0 0" and got[12] == "ok"
    bk = fref.Book(4, 2, 0, 40, True)
    for src, ok in (([0, 1, 2, 3], True), ([0, 0, 0, 3], True), ([1, 1, 3, 3], True), ([1, 2, 2, 3], False), ([1, 0, 2, 3], False), ([0, 1, 2, 4], False),
                    ([0, -1, 2, 3], False), ([0, 1, 2], False)):
        assert bk.fork_ok(src) == ok, src


def test_the_smallest_case_of_every_range_rule(driver):
    """Q = 4, Lmax = 24 + P0: 4 rows, then 5 per step; the step at wp = 24 + P0 - 5 + ... wraps. One sample restarted in front of step 3."""
    for P0 in (0, 3):
        for ring in (1, 0):
            ops = [f"begin 2 4 {P0} {P0 + 24} {ring}", "step 1", "step 1", "step 1", "restart 0 1", "ranges", "step 1", "ranges"]
            got = _run(driver, ops)
            assert got[5] == f"ranges | {P0} {P0 + 14} |"                                  # sample 1: age 0, no range
            assert got[7] == f"ranges | {P0} {P0 + 19} | {P0 + 14} {P0 + 19}"
            if not ring:
                continue
            # step 4 does not fit (19 + 5 = 24 fits exactly: no skip); step 5 wraps behind an empty tail: sample 0 (age 24) must restart
            got = _run(driver, ops + ["step 1", "restart 1 0", "step 1", "ranges", "fork 1 1", "ranges", "left"])
            assert got[8] == f"plan {P0 + 19} 5 5" and got[10] == f"plan {P0} 5 5"
            assert got[11] == f"ranges | {P0} {P0 + 5} | {P0} {P0 + 5} {P0 + 14} {P0 + 24}"      # sample 1: steps 3, 4 at the end, step 5 at the start
            assert got[13] == f"ranges | {P0} {P0 + 5} {P0 + 14} {P0 + 24} | {P0} {P0 + 5} {P0 + 14} {P0 + 24}"
            assert len(set(got[14].split()[1:])) == 1


# ---------------------------------------------------------------------------------------------- the GPU scenario contains what it is about
def test_the_gpu_scenario_contains_the_forks_it_is_about(driver):
    forks, bk = fref.replay(ring=True)
    assert [f["t"] for f in forks] == sorted(fref.FORKS)
    two_ranges = [f for f in forks if any(len(fref.ranges_of(rows)) == 2 for rows in f["live"].values())]
    age0 = [f for f in forks if any(a == 0 for a in f["ages"].values())]
    installed = [f for f in forks if any(f["installed"].values())]
    multi = [f for f in forks if any(n >= 2 for n in f["n_dst"].values())]
    after_skip = [f for f in forks if f["skipped_tails"] >= 1 and any(f["ages"].values())]
    groups2 = [f for f in forks if len(f["n_dst"]) >= 2]
    assert two_ranges and age0 and installed and multi and after_skip and groups2, forks
    assert any(f in multi for f in two_ranges), "a fork to two destinations whose source lies behind a wrap"
    assert all(rows for f in installed for s, rows in f["live"].items() if f["installed"][s])
    # a destination's prompt differs from its source's: in front of every fork the two are in different episodes of different samples -- prompts
    # are drawn per (sample, episode number) -- unless the destination is itself a copy of that source
    lin, _ = fref.replay(ring=False)
    assert len(lin) == 1 and lin[0]["ages"] == {0: 24} and lin[0]["n_dst"] == {0: 2}
    # the same scenario through the C++ book: ages, ranges and steps_left agree with the restatement at every fork
    sc = _Script()
    ref = fref.Book(fref.B, fref.Q, 0, fref.NPOS, True)
    sc.add(f"begin {fref.B} {fref.Q} 0 {fref.NPOS} 1", "ok")
    for t in range(fref.STEPS):
        flags, inst, source = fref.events(t)
        if any(flags):
            ref.restart(flags)
            sc.add("restart " + _ints(flags), "ok")
        if inst:
            b, T = inst
            fl = [x == b for x in range(fref.B)]
            ref.restart(fl)
            ref.install(fl, T)
            sc.add("restart " + _ints(fl), "ok")
            sc.add(f"install {T} " + _ints(fl), f"install {ref.age[b]}")
        if source:
            ref.fork(source)
            sc.add("fork " + _ints(source), "ok")
            sc.after(ref)
        p = ref.step(1)
        sc.add("step 1", f"plan {p[0]} {p[1]} {p[2]}")
        sc.after(ref)
    sc.check(driver)


# ---------------------------------------------------------------------------------------------- ABI, Python surface, kernel build
def _header():
    with open(os.path.join(ROOT, "include", "vima_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


@pytest.mark.parametrize("name", NEW)
def test_header_library_and_binding_agree(name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.M | re.S)
    assert m, f"{name} is not declared in include/vima_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    assert name in _lib.PROTOTYPES, f"{name} missing from _lib.PROTOTYPES"
    res, args = _lib.PROTOTYPES[name]
    assert res is ctypes.c_int and len(args) == len(params), (params, args)
    for p, a in zip(params, args):       # ints are ints, host int32 arrays are int32 pointers, everything else a pointer-sized argument
        is_int = re.match(r"^int\s+\w+$", p) is not None
        assert (a is ctypes.c_int) == is_int, (name, p, a)
        assert (a is ctypes.POINTER(ctypes.c_int32)) == p.startswith("const int32_t*"), (name, p, a)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), f"{_lib.LIB_PATH} does not export {name}"
    assert _lib.load().vima_abi_version() == 5 == _lib.ABI_VERSION       # additive: the version stays


def test_python_surface():
    import torch
    from vima_amd.policy import VIMAPolicy
    from vima_amd import baselines
    assert list(inspect.signature(VIMAPolicy.fork_samples).parameters) == ["self", "source", "prompt_token", "prompt_token_mask"]
    assert list(inspect.signature(baselines._BaselinePolicy.seq_fork).parameters) == ["self", "source"]
    for text in (VIMAPolicy.fork_samples.__doc__, baselines._BaselinePolicy.seq_fork.__doc__):
        assert "steps_left" in text and "bit for bit" in text
    x, m = torch.zeros(3, 2, 256), torch.ones(2, 3, dtype=torch.bool)
    for cls, kw in ((baselines.VIMAGPTPolicy, {}), (baselines.VIMAGatoPolicy, {})):
        pol = cls(embed_dim=256, vocab_size=16, n_positions=64, n_layer=1, n_head=8, **kw)
        with pytest.raises(NotImplementedError, match="seq_fork"):
            pol.fork_samples([0, 0], x, m)
    fl = baselines.VIMAFlamingoPolicy(embed_dim=256, dt_n_layers=1, dt_n_heads=8, xattn_n_heads=8)
    assert type(fl).fork_samples is baselines._BaselinePolicy.fork_samples
    with pytest.raises(NotImplementedError, match="fork_samples"):
        fl.seq_fork([0, 0])
    pol = VIMAPolicy(embed_dim=256, xf_n_layers=1, sattn_n_heads=8, xattn_n_heads=8)
    with pytest.raises(RuntimeError):      # no weights (and no GPU here): refuses, no fallback
        pol.fork_samples([0, 0], x, m)


@needs_hipcc
def test_episode_fork_kernels_compile_without_scratch():
    """Both instantiations of episode_fork_kernel (operand types float and bf16) and the state kernel cross-compile for gfx950 with scratch size 0.
    Figures of this record (ROCm 7.2 hipcc): episode_fork_kernel 32 VGPRs for either type, episode_fork_state_kernel 6 VGPRs; 0 AGPRs and
    0 bytes of LDS everywhere."""
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result",
                          "--cuda-device-only", "-S", os.path.join(ROOT, "vima_amd", "csrc", "episode_fork.hip"), "-o", os.devnull,
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
    assert len([k for k in res if "episode_fork_kernel" in k]) == 2 and len([k for k in res if "episode_fork_state_kernel" in k]) == 1, sorted(res)
    for name, v in res.items():
        print(f"[episode-fork] {name}: {v}")
        assert v.get("ScratchSize", 0) == 0 and v.get("LDS", 0) == 0, (name, v)
