"""Episode snapshots (vima_decode_snapshot / vima_decode_restore, the vima_seq_* pair, vima_op_episode_pack / _unpack) without a GPU: the
bookkeeping of vima_amd/csrc/episode_book.h (steps_of, history_rows, install) in a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/episode_book_driver.cpp, built by tests/episode_driver.py) against the brute-force
restatement of tests/episode_snapshot_reference.py over 300 random schedules per cache family; the C ABI declares, exports and binds the new
functions; the Python surface; the kernels cross-compile for gfx950 without scratch and LDS; and the scenario of
tests/test_episode_snapshot_gpu.py contains the snapshots and restores it is about."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import pytest

from vima_amd import _lib
from tests import episode_snapshot_reference as sref
from tests.episode_driver import ROOT, _ints, driver  # noqa: F401
from tests.test_episode_fork_build import HIPCC, _random_source, _run, needs_hipcc

NEW = ("vima_decode_snapshot_size", "vima_decode_snapshot", "vima_decode_restore", "vima_seq_decode_snapshot_size", "vima_seq_decode_snapshot",
       "vima_seq_decode_restore", "vima_op_episode_pack", "vima_op_episode_unpack")


class _Script:
    """operations for the driver next to the exact line the restatement expects"""

    def __init__(self):
        self.ops, self.want = [], []

    def add(self, op, want):
        self.ops.append(op)
        self.want.append(want)

    def after(self, bk):
        """after every operation: write pointer, high-water mark, ages, and steps_left of every sample"""
        self.add("state", f"state {bk.wp} {bk.hw} {bk.next} {bk.hw if bk.ring else bk.wp} ages " + _ints(bk.age))
        self.add("left", "left " + _ints(bk.steps_left(b) for b in range(bk.B)))

    def check(self, exe):
        for i, (op, want, g) in enumerate(zip(self.ops, self.want, _run(exe, self.ops))):
            assert g == want, f"operation {i} `{op}`: the program says `{g}`, the restatement `{want}`; before it: {self.ops[max(0, i - 10):i]}"


def _rows(rows):
    return " |" + "".join(f" {r}" for r in rows)


def _schedules(seq, seed=0, schedules=300):
    rng = random.Random(seed + (1000 if seq else 0))
    sc = _Script()
    seen = dict(ring=0, linear=0, snapshots=0, two_ranges=0, restores=0, straddle=0, n0=0, two_slots=0, refusals=0, later=0, installs=0, forks=0, wraps=0)
    for k in range(schedules):
        B, Q, ring = rng.randint(1, 5), rng.randint(1, 6), k % 4 != 0
        if seq:
            Lp = rng.randint(1, 9)
            P0, Lmax = Lp + 1, Lp + 1 + rng.randint(3 * (Q + 1), 96)
        else:
            P0, Lmax = 0, rng.randint(24, 96)
        bk = sref.SnapBook(B, Q, P0, Lmax, ring)
        seen["ring" if ring else "linear"] += 1
        sc.add(f"begin {B} {Q} {P0} {Lmax} {int(ring)}", "ok")
        sc.after(bk)
        held = []                                                    # (n, batch step it was taken at)
        for _ in range(rng.randint(5, 60)):
            flags = [rng.random() < 0.2 for _ in range(B)]
            if ring:
                flags = [f or bk.steps_left(b) == 0 for b, f in enumerate(flags)]
            if any(flags):
                bk.restart(flags)
                sc.add("restart " + _ints(flags), "ok")
                sc.after(bk)
            if bk.room() >= 1 and rng.random() < 0.2:
                T, fl = rng.randint(1, bk.room()), [rng.random() < 0.5 for _ in range(B)]
                bk.install(fl, T)
                sc.add(f"install {T} " + _ints(fl), f"install {sum(bk.adv[len(bk.adv) - T:])}")
                sc.after(bk)
                seen["installs"] += 1
            if rng.random() < 0.3:
                source = _random_source(rng, B)
                bk.fork(source)
                sc.add("fork " + _ints(source), "ok")
                sc.after(bk)
                seen["forks"] += 1
            if rng.random() < 0.5:                                    # a snapshot: n and the compact -> cache row map of this moment
                b = rng.randrange(B)
                n, rows = bk.snapshot(b)
                live = bk.live_rows(b)                                # the episode's written rows: the compact rows and, at most, the first step's masked action row
                assert set(rows) <= live and len(rows) == len(set(rows)) and len(live) - len(rows) in (0, 1), (rows, live)
                sc.add(f"snap {b}", f"snap {n}" + _rows(rows))
                held.append((n, bk.next))
                seen["snapshots"] += 1
                seen["two_ranges"] += len(sref.ranges_of(bk.live_rows(b))) == 2
                seen["n0"] += n == 0
            if held and rng.random() < 0.5:                           # a restore, usually at a later step, into one or two slots
                n, taken = max(held) if rng.random() < 0.3 else rng.choice(held)   # the longest one often: it may no longer fit
                slots = rng.sample(range(B), min(B, rng.choice([1, 1, 2])))
                before = (list(bk.age), [bk.steps_left(b) for b in range(B)])
                got = bk.restore(slots, n)
                if got is None:
                    sc.add(f"restore {n} " + _ints(slots), f"refused room {bk.room()}")
                    assert before == (list(bk.age), [bk.steps_left(b) for b in range(B)])
                    seen["refusals"] += 1
                else:
                    age, rows = got
                    sc.add(f"restore {n} " + _ints(slots), f"restore {age}" + _rows(rows))
                    seen["restores"] += 1
                    seen["straddle"] += sref.straddles(rows)
                    seen["two_slots"] += len(slots) == 2
                    seen["later"] += bk.next > taken
                    for d in slots:                                   # the restored slot is a sample restarted n batch steps ago
                        assert bk.steps_of(d) == n
                sc.after(bk)                                          # a refusal changes nothing: the same state and steps_left lines
            out = [ring and bk.steps_left(b) == 0 for b in range(B)]
            if any(out):
                bk.restart(out)
                sc.add("restart " + _ints(out), "ok")
            T = rng.choice([1, 1, 2, 3])
            p = bk.step(T)
            sc.add(f"step {T}", "refused" if p is None else f"plan {p[0]} {p[1]} {p[2]}")
            sc.after(bk)
            # EpisodeBook::history as the entries call it, for the longest history that fits (the identity over the prefix, then the rows; any other
            # line is its range check failing) and for one step more (refused with the room)
            room = bk.room()
            sc.add(f"hist {room}", f"hist {sum(bk.adv[len(bk.adv) - room:]) if room else 0}" + _rows(list(range(P0)) + bk.rows_of_last(room)))
            sc.add(f"hist {room + 1}", f"refused room {room}")
            if p is None:
                if T == 1:
                    assert not ring, "ring: every sample out of steps was restarted, a single step must pass"
                    break
                continue
            seen["wraps"] += p[2] > p[1]
    return sc, seen


@pytest.mark.parametrize("seq", [False, True], ids=["P0=0", "P0=Lp+1"])
def test_random_schedules_with_snapshots_and_restores(driver, seq):
    sc, seen = _schedules(seq)
    sc.check(driver)                                                  # all 300 schedules through one child process
    print(f"[episode-snapshot] {seen}")
    assert seen["ring"] == 225 and seen["linear"] == 75
    assert seen["snapshots"] > 1000 and seen["restores"] > 500 and seen["later"] > 300 and seen["installs"] >= 100 and seen["forks"] >= 100, seen
    assert seen["straddle"] >= 30 and seen["two_ranges"] >= 30 and seen["n0"] >= 100 and seen["two_slots"] >= 100 and seen["refusals"] >= 15, seen


def test_steps_of_and_the_room_rule_in_the_smallest_case(driver):
    """Q = 4, Lmax = 24: 4 rows, then 5 per step; sample 1 restarted in front of step 2. A snapshot of 3 steps is refused while the book holds 2."""
    ops = ["begin 2 4 0 24 1", "snap 0", "step 1", "step 1", "restart 0 1", "snap 1", "step 1", "snap 0", "snap 1", "restore 4 1", "state",
           "restore 1 0 1", "state", "snap 0"]
    got = _run(driver, ops)
    assert got[1] == "snap 0 |" and got[5] == "snap 0 |"
    assert got[7] == "snap 3 |" + "".join(f" {r}" for r in range(14)) and got[8] == "snap 1 | 10 11 12 13"
    assert got[9] == "refused room 3" and got[10] == "state 14 14 3 14 ages 14 5"
    assert got[11] == "restore 5 | 10 11 12 13" and got[12] == "state 14 14 3 14 ages 5 5" and got[13] == "snap 1 | 10 11 12 13"
    bk = sref.SnapBook(1, 2, 0, 40, True)
    bk.age[0] = 1                                                     # no run of steps adds up to this age
    assert bk.steps_of(0) == -1


# ---------------------------------------------------------------------------------------------- the GPU scenario contains what it is about
def test_the_gpu_scenario_contains_the_cases_it_is_about(driver):
    snaps, rests, left, bk = sref.replay(ring=True)
    by = {s["name"]: s for s in snaps}
    assert any(len(s["ranges"]) == 2 for s in snaps), "a snapshot taken behind a wrap"
    assert any(sref.straddles(r["rows"]) for r in rests), "a restore whose rows straddle the wrap"
    assert any(r["own_slot"] and r["t"] > r["taken"] for r in rests), "a restore into its own slot k steps later"
    assert any(len(r["slots"]) == 2 and sref.straddles(r["rows"]) for r in rests), "a restore into two slots"
    assert any(s["n"] == 0 and s["restarted_now"] for s in snaps) and any(r["n"] == 0 for r in rests), "a just-restarted sample"
    assert any(s["installed"] and s["n"] > 0 for s in snaps), "a sample with an installed history"
    assert any(s["forked"] and s["n"] > 0 for s in snaps), "a forked destination"
    assert any(r["after_chunk"] == 2 for r in rests), "a restore after a forward_steps chunk of T = 2"
    assert any(not r["with_prompt"] and r["own_slot"] for r in rests), "a prompt-less snapshot restored inside its prompt group"
    assert all(r["rows"] != by[r["name"]]["rows"] for r in rests if r["n"]), "every restore lands at other rows than the snapshot was taken from"
    assert {r["name"] for r in rests} == set(by)
    lin_s, lin_r, _, lin = sref.replay(ring=False)
    assert len(lin_s) == 1 and lin_s[0]["n"] == 3 and lin_r[0]["slots"] == [0, 2] and [lin.steps_left(b) for b in range(sref.B)] == [0] * sref.B
    # the same scenario through the C++ book: maps, ages and steps_left agree with the restatement at every operation
    sc = _Script()
    ref = sref.SnapBook(sref.B, sref.Q, 0, sref.NPOS, True)
    sc.add(f"begin {sref.B} {sref.Q} 0 {sref.NPOS} 1", "ok")
    held, t = {}, 0
    while t < sref.STEPS:
        flags, inst, source, T, snap, rest = sref.events(t)
        if any(flags):
            ref.restart(flags)
            sc.add("restart " + _ints(flags), "ok")
        if inst:
            b, n = inst
            fl = [x == b for x in range(sref.B)]
            ref.restart(fl)
            ref.install(fl, n)
            sc.add("restart " + _ints(fl), "ok")
            sc.add(f"install {n} " + _ints(fl), f"install {ref.age[b]}")
        if source:
            ref.fork(source)
            sc.add("fork " + _ints(source), "ok")
        for name, (b, _) in snap.items():
            n, rows = ref.snapshot(b)
            held[name] = n
            sc.add(f"snap {b}", f"snap {n}" + _rows(rows))
        for name, slots in rest:
            age, rows = ref.restore(slots, held[name])
            sc.add(f"restore {held[name]} " + _ints(slots), f"restore {age}" + _rows(rows))
            sc.after(ref)
        assert [ref.steps_left(b) for b in range(sref.B)] == left[t]
        p = ref.step(T)
        sc.add(f"step {T}", f"plan {p[0]} {p[1]} {p[2]}")
        sc.after(ref)
        t += T
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


def test_info_struct_matches_the_header():
    m = re.search(r"typedef struct VimaEpisodeSnapshotInfo \{(.*?)\} VimaEpisodeSnapshotInfo;", _header(), flags=re.S)
    assert m, "VimaEpisodeSnapshotInfo is not declared in include/vima_hip.h"
    fields = re.findall(r"(int32_t|int64_t)\s+(\w+)\s*;", m.group(1))
    want = [(n, {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t"}[t]) for n, t in _lib.VimaEpisodeSnapshotInfo._fields_]
    assert [(n, t) for t, n in fields] == want
    assert ctypes.sizeof(_lib.VimaEpisodeSnapshotInfo) == 40
    assert re.search(r"#define\s+VIMA_SNAPSHOT_PROMPT\s+1\b", _header()) and _lib.SNAPSHOT_PROMPT == 1


def test_python_surface():
    import torch
    from vima_amd.policy import VIMAPolicy
    from vima_amd import baselines
    from vima_amd.episodes import EpisodeSnapshot
    assert list(inspect.signature(VIMAPolicy.snapshot_samples).parameters) == ["self", "samples", "prompt_token", "prompt_token_mask", "with_prompt"]
    assert inspect.signature(VIMAPolicy.snapshot_samples).parameters["with_prompt"].default is True
    assert list(inspect.signature(VIMAPolicy.restore_samples).parameters) == ["self", "slots", "snapshots", "prompt_token", "prompt_token_mask"]
    assert list(inspect.signature(baselines._BaselinePolicy.seq_snapshot).parameters) == ["self", "samples"]
    assert list(inspect.signature(baselines._BaselinePolicy.seq_restore).parameters) == ["self", "slots", "snapshots"]
    for text in (VIMAPolicy.restore_samples.__doc__, baselines._BaselinePolicy.seq_restore.__doc__):
        assert "steps_left" in text and "IndexError" in text and "ValueError" in text
    x, m = torch.zeros(3, 2, 256), torch.ones(2, 3, dtype=torch.bool)
    for cls in (baselines.VIMAGPTPolicy, baselines.VIMAGatoPolicy):
        pol = cls(embed_dim=256, vocab_size=16, n_positions=64, n_layer=1, n_head=8)
        with pytest.raises(NotImplementedError, match="seq_snapshot"):
            pol.snapshot_samples([0], x, m)
        with pytest.raises(NotImplementedError, match="seq_restore"):
            pol.restore_samples([0], [], x, m)
    fl = baselines.VIMAFlamingoPolicy(embed_dim=256, dt_n_layers=1, dt_n_heads=8, xattn_n_heads=8)
    with pytest.raises(NotImplementedError, match="snapshot_samples"):
        fl.seq_snapshot([0])
    with pytest.raises(NotImplementedError, match="restore_samples"):
        fl.seq_restore([0], [])
    pol = VIMAPolicy(embed_dim=256, xf_n_layers=1, sattn_n_heads=8, xattn_n_heads=8)
    with pytest.raises(RuntimeError):      # no weights (and no GPU here): refuses, no fallback
        pol.snapshot_samples([0], x, m)
    assert EpisodeSnapshot.__module__ == "vima_amd.episodes"


def test_snapshot_state_dict_round_trips_on_the_cpu(tmp_path):
    import torch
    from vima_amd.episodes import EpisodeSnapshot
    info = dict(steps=3, Q=4, embed_dim=256, layers=2, prompt_len=5, elem_bytes=2, flags=1, policy_kind=0, bytes=96)
    g = torch.Generator().manual_seed(3)
    snap = EpisodeSnapshot(torch.randint(0, 256, (96,), generator=g, dtype=torch.uint8), info, torch.randn(5, 256, generator=g),
                           torch.tensor([1, 1, 0, 1, 1], dtype=torch.bool))
    assert snap.steps == 3 and snap.nbytes == 96 and snap.has_prompt and snap.cpu() is snap and snap.to("cpu") is snap
    sd = snap.state_dict()
    assert all(isinstance(v, (int, torch.Tensor)) for v in sd.values()), {k: type(v) for k, v in sd.items()}
    torch.save(sd, tmp_path / "snap.pt")
    back = EpisodeSnapshot.from_state_dict(torch.load(tmp_path / "snap.pt", weights_only=True))
    assert back.info == snap.info and torch.equal(back.payload, snap.payload) and torch.equal(back.prompt_token, snap.prompt_token)
    assert torch.equal(back.prompt_token_mask, snap.prompt_token_mask) and back.has_prompt and back.steps == 3
    bare = EpisodeSnapshot(snap.payload[:32].clone(), dict(info, flags=0, bytes=32))
    again = EpisodeSnapshot.from_state_dict(bare.state_dict())
    assert not again.has_prompt and again.prompt_token is None and again.nbytes == 32
    with pytest.raises(ValueError):
        EpisodeSnapshot(snap.payload[:31], info)
    with pytest.raises(KeyError):
        EpisodeSnapshot.from_state_dict({"payload": snap.payload})


def test_snapshot_kernels_live_in_their_own_file():
    """episode_fork.hip keeps its kernels (tests/test_episode_fork_build.py counts them); build.sh compiles and links the new file"""
    with open(os.path.join(ROOT, "vima_amd", "csrc", "build.sh")) as f:
        sh = f.read()
    assert "episode_snapshot;" in sh and "obj/episode_snapshot.o" in sh
    with open(os.path.join(ROOT, "vima_amd", "csrc", "episode_fork.hip")) as f:
        assert "episode_pack" not in f.read()


@needs_hipcc
def test_episode_snapshot_kernels_compile_without_scratch_and_lds():
    """Both instantiations of episode_pack_kernel and episode_unpack_kernel (operand types float and bf16) and the two state kernels cross-compile
    for gfx950 with scratch size 0 and no LDS. Figures of this record: episode_pack_kernel 40 VGPRs and episode_unpack_kernel 48 for either type,
    episode_pack_state_kernel 53, episode_unpack_state_kernel 32; 0 AGPRs everywhere."""
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result",
                          "--cuda-device-only", "-S", os.path.join(ROOT, "vima_amd", "csrc", "episode_snapshot.hip"), "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    for stem, count in (("episode_pack_kernel", 2), ("episode_unpack_kernel", 2), ("episode_pack_state_kernel", 1), ("episode_unpack_state_kernel", 1)):
        assert len([k for k in res if stem in k]) == count, (stem, sorted(res))
    for name, v in res.items():
        print(f"[episode-snapshot] {name}: {v}")
        assert v.get("ScratchSize", 0) == 0 and v.get("LDS", 0) == 0, (name, v)
