"""The host bookkeeping of the episode caches itself (vima_amd/csrc/episode_book.h, the one EpisodeBook behind vima_decode_* and vima_seq_*) on the
CPU: tests/episode_book_driver.cpp is compiled (tests/episode_driver.py) as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, run in a child
process, and compared line for line with the three Python restatements (tests/episode_prefill_reference.EpisodeBook for the prefix P0 = 0,
tests/seq_prefill_reference.SeqBook on top of tests/seq_ring_reference.Ring for P0 = Lp + 1), which stay independent of it.

What the C++ adds to the restatements and the test derives by the stated rule: hw = max(hw, row + Lq); ring: win_end = row + Lq, Lk = hw; linear:
win_end = 0, Lk = row + Lq; a refusal carries the steps that still fit for the offending sample (= its steps_left). The restatements name a unit
longer than the whole ring by its first victim ("sample 0"; EpisodeBook at batch step 0: "longer than n_positions"); the C++ has a kind of its own
for it ("long", sample 0), so that pair is the one place where the two are matched by rule and not by text."""
import random
import re

import pytest

from tests import episode_prefill_reference as eref
from tests import seq_prefill_reference as sref
from tests.episode_driver import _flags, _run, driver  # noqa: F401


class _Twin:
    """One Python restatement behind the driver's vocabulary: every method returns (operation line, expected result line)."""

    def __init__(self, seq, B, Q, P0, Lmax, ring):
        self.seq, self.B, self.Q, self.P0, self.Lmax, self.ring = seq, B, Q, P0, Lmax, bool(ring)
        self.R = Lmax - P0
        if seq:
            self.book = sref.SeqBook(P0 - 1, Lmax, Q, B, ring)
            self.book.prefill()
        else:
            assert P0 == 0
            self.book = eref.EpisodeBook(B, Q, Lmax, ring)
        self.hw = P0

    def begin(self):
        return f"begin {self.B} {self.Q} {self.P0} {self.Lmax} {int(self.ring)}", "ok"

    # ---- the restatements' state under common names
    next = property(lambda s: s.book.r.next if s.seq else s.book.step + 1)
    wp = property(lambda s: s.book.r.wp if s.seq else s.book.wp)
    ages = property(lambda s: s.book.r.age if s.seq else s.book.age)

    def room_now(self):
        return self.book.room() if self.seq else self.book.history_room()

    def left_now(self):
        if self.seq or self.book.step >= 0:
            return self.book.steps_left()
        # EpisodeBook restates steps_left only for a batch that has taken step 0; in front of it: the fresh batch of the other restatement, no prefix
        if self.ring:
            return sref.rr.Ring(-1, self.Lmax, self.Q, self.B).steps_left()
        return [sref.rr.linear_steps_left(self.Lmax, 0, self.Q, True)] * self.B

    def _lq(self, T):
        return T * (self.Q + 1) - (1 if self.next == 0 else 0)

    # ---- operations
    def unit(self, T, commit):
        """plan T / step T -> (op, expected, compare the expected line as a prefix only, (row, lq, adv) or None). A refusal reads `refused kind sample
        fit age`; the age is compared where the restatements keep one: for the sample over age"""
        op = f"{'step' if commit else 'plan'} {T}"
        try:
            row, lq, adv = self.book.plan(T)
        except IndexError as e:
            m = re.search(r"room for (\d+) more steps", str(e))
            if m:                                                    # linear
                fit = int(m.group(1))
                assert self.left_now() == [fit] * self.B
                return op, f"refused full 0 {fit}", True, None
            if self.ring and self._lq(T) > self.R:                   # longer than the whole ring (docstring)
                assert "sample 0" in str(e) or "longer than n_positions" in str(e)
                return op, f"refused long 0 {self.left_now()[0]}", True, None
            b = int(re.search(r"sample (\d+)", str(e)).group(1))
            return op, f"refused age {b} {self.left_now()[b]} {self.ages[b]}", False, None
        hw = max(self.hw, row + lq)
        want = f"plan {row} {lq} {adv} {hw if self.ring else row + lq} {row + lq if self.ring else 0} {hw}"
        if commit:
            assert self.book.advance(T) == (row, lq, adv)
            self.hw = hw
            if self.seq:
                assert self.book.r.hw == hw
        return op, want, False, (row, lq, adv)

    def restart(self, flags):
        self.book.restart(flags)
        return "restart " + _flags(flags), "ok"

    def room(self):
        return "room", f"room {self.room_now()}"

    def _age(self, T):
        return sum(adv for _, adv in self.book.slots[len(self.book.slots) - T:])

    def rows(self, T):
        if T > self.room_now():
            return f"rows {T}", f"refused room {self.room_now()}"
        return f"rows {T}", " ".join(map(str, ["rows", self._age(T)] + self.book.history_rows(T)))

    def hist(self, T):
        """EpisodeBook::history as the library's entries call it: the identity over the prefix, then the rows. Any other line is its range check
        ([P0, written_end()) for every history row) failing; a history beyond the room is refused with the room"""
        if T > self.room_now():
            return f"hist {T}", f"refused room {self.room_now()}"
        return f"hist {T}", " ".join(map(str, ["hist", self._age(T), "|"] + list(range(self.P0)) + self.book.history_rows(T)))

    def install(self, T, flags):
        op = f"install {T} " + _flags(flags)
        try:
            self.book.install(flags, T)
        except IndexError as e:
            assert f"room for {self.room_now()}" in str(e)
            return op, f"refused room {self.room_now()}"
        assert all(a == self._age(T) for f, a in zip(flags, self.ages) if f)
        return op, " ".join(map(str, ["install", self._age(T)] + self.book.history_rows(T)))

    def left(self):
        return "left", "left " + " ".join(map(str, self.left_now()))

    def state(self):
        """write pointer, high-water mark, next step, written_end, slot count (the C++ trims the record to Lmax entries; EpisodeBook keeps all), ages
        (SeqBook keeps them under the ring only)"""
        n = min(len(self.book.slots), self.Lmax)
        head = f"state {self.wp} {self.hw} {self.next} {self.hw if self.ring else self.wp} {n} ages"
        if self.seq and not self.ring:
            return "state", head, True
        return "state", " ".join([head] + list(map(str, self.ages))), False


class _Script:
    def __init__(self):
        self.ops, self.want, self.prefix_only = [], [], []

    def add(self, op, want, prefix_only=False):
        self.ops.append(op)
        self.want.append(want)
        self.prefix_only.append(prefix_only)

    def after(self, twin):
        """everything the issue compares after an operation: room, steps_left, ages and slot count"""
        self.add(*twin.room())
        self.add(*twin.left())
        self.add(*twin.state())

    def check(self, exe):
        got = _run(exe, self.ops)
        for i, (op, want, g, pre) in enumerate(zip(self.ops, self.want, got, self.prefix_only)):
            assert (g.startswith(want + " ") or g == want) if pre else g == want, \
                f"operation {i} `{op}`: the program says `{g}`, the restatement `{want}`; before it: {self.ops[max(0, i - 12):i]}"


def _schedules(seq, seed=0, schedules=300):
    """The generator of the two selfcheck functions (restarts with probability 1 / 4 and of every sample out of steps, units of 1, 1, 2 or 3 steps,
    every third schedule single steps only, every fourth linear), with real installs of 1, the room and a random T after every unit, each behind the table the library builds for it."""
    rng = random.Random(seed)
    sc = _Script()
    seen = dict(wrap_skips=0, chunk_refused_step_passes=0, installs=0, refused_installs=0, ring=0, linear=0)
    for k in range(schedules):
        B, Q, ring = rng.randint(1, 4), rng.randint(1, 6), k % 4 != 0
        if seq:
            Lp = rng.randint(1, 9)
            P0, Lmax = Lp + 1, Lp + 1 + rng.randint(3 * (Q + 1), 96)
        else:
            P0, Lmax = 0, rng.randint(24, 96)
        twin = _Twin(seq, B, Q, P0, Lmax, ring)
        seen["ring" if ring else "linear"] += 1
        only1 = k % 3 == 0
        sc.add(*twin.begin())
        sc.after(twin)
        for _ in range(rng.randint(5, 60)):
            flags = [rng.random() < 0.25 for _ in range(B)]
            if ring:
                flags = [f or n == 0 for f, n in zip(flags, twin.left_now())]
            if twin.next > 0 or seq:
                sc.add(*twin.restart(flags))
                sc.after(twin)
            T = 1 if only1 else rng.choice([1, 1, 2, 3])
            sc.add(*twin.unit(T, False)[:3])
            *line, unit = twin.unit(T, True)
            sc.add(*line)
            sc.after(twin)
            if unit is None:
                if T == 1:
                    assert not ring, "ring: every sample out of steps was restarted, a single step must pass"
                    break
                *line, one = twin.unit(1, False)
                sc.add(*line)
                seen["chunk_refused_step_passes"] += one is not None
                continue
            row, lq, adv = unit
            seen["wrap_skips"] += adv > lq
            room = twin.room_now()
            for Th in sorted({1, room, rng.randint(1, max(1, room))}):
                if Th < 1 or Th > room:
                    continue
                sc.add(*twin.rows(Th))
                sc.add(*twin.hist(Th))
                sc.add(*twin.install(Th, [rng.random() < 0.5 for _ in range(B)]))
                sc.after(twin)
                seen["installs"] += 1
            sc.add(*twin.hist(room + 1))                            # one step more than the room: refused with the room, whatever the record holds
            if room < min(len(twin.book.slots), Lmax):
                sc.add(*twin.rows(room + 1))
                sc.add(*twin.install(room + 1, [True] * B))
                sc.after(twin)
                seen["refused_installs"] += 1
    return sc, seen


@pytest.mark.parametrize("seq", [False, True], ids=["P0=0-vs-EpisodeBook", "P0=Lp+1-vs-SeqBook"])
def test_random_schedules_line_for_line(driver, seq):
    sc, seen = _schedules(seq)
    sc.check(driver)                                            # all 300 schedules through one child process
    assert seen["ring"] == 225 and seen["linear"] == 75
    assert seen["wrap_skips"] >= 1 and seen["chunk_refused_step_passes"] >= 1 and seen["installs"] > 1000 and seen["refused_installs"] >= 1, seen


# ---------------------------------------------------------------------------------------------- the smallest cases of every rule
def _steps(twin, sc, n, restart_before=()):
    for t in range(n):
        if t in restart_before:
            sc.add(*twin.restart([True] * twin.B))
        *line, unit = twin.unit(1, True)
        assert unit is not None, (t, line)
        sc.add(*line)


def test_ring_chunk_refused_where_a_step_passes(driver):
    twin, sc = _Twin(True, 1, 4, 4, 52, True), _Script()        # SeqBook(3, 52, 4, 1, ring)
    sc.add(*twin.begin())
    _steps(twin, sc, 8)
    assert twin.book.plan(1) == (43, 5, 5)
    sc.add("plan 1", "plan 43 5 5 48 48 48")
    sc.add("plan 2", "refused age 0 1 39")                      # 43 + 10 > 52: skips 9 rows and writes 10, 39 + 19 > 48; one single step fits
    assert twin.unit(2, False)[1] == "refused age 0 1 39"
    sc.after(twin)
    sc.check(driver)


def test_linear_chunk_room(driver):
    twin, sc = _Twin(True, 1, 4, 4, 52, False), _Script()
    sc.add(*twin.begin())
    _steps(twin, sc, 7)
    assert twin.book.plan(2) == (38, 10, 10)
    sc.add("plan 2", "plan 38 10 10 48 0 48")
    sc.add("plan 3", "refused full 0 2", True)                  # 38 + 15 > 52; room for (52 - 38) // 5 = 2
    assert twin.unit(3, False)[1] == "refused full 0 2"
    sc.after(twin)
    sc.check(driver)


@pytest.mark.parametrize("P0", [0, 4])
def test_a_unit_that_ends_exactly_at_lmax_is_not_skipped(driver, P0):
    Q, n = 4, 10                                                # Q rows, then 9 x (Q + 1): the last one ends at Lmax = P0 + 49 = the whole ring
    twin, sc = _Twin(P0 > 0, 2, Q, P0, P0 + 49, True), _Script()
    sc.add(*twin.begin())
    _steps(twin, sc, n - 1)
    op, want, _, unit = twin.unit(1, True)
    assert unit == (P0 + 44, 5, 5)                              # no skip: advance = Lq
    sc.add(op, f"plan {P0 + 44} 5 5 {P0 + 49} {P0 + 49} {P0 + 49}")
    assert want == sc.want[-1]
    sc.add("state", f"state {P0 + 49} {P0 + 49} {n} {P0 + 49} {n} ages 49 49")
    sc.add("left", "left 0 0")
    sc.add("plan 1", "refused age 0 0 49")                      # the next unit wraps behind an empty tail: 5 more rows than the ring has
    sc.add(*twin.restart([True, False]))
    sc.add("plan 1", "refused age 1 0 49")
    sc.add(*twin.restart([False, True]))
    sc.add("step 1", f"plan {P0} 5 5 {P0 + 49} {P0 + 5} {P0 + 49}")
    assert twin.unit(1, True)[1] == sc.want[-1]
    sc.after(twin)
    sc.check(driver)


@pytest.mark.parametrize("P0", [0, 4])
def test_a_unit_as_long_as_the_whole_ring_and_one_row_longer(driver, P0):
    Q, T = 4, 3                                                 # 3 steps of a fresh batch: 14 rows
    for R, legal in ((14, True), (13, False)):
        twin, sc = _Twin(P0 > 0, 2, Q, P0, P0 + R, True), _Script()
        sc.add(*twin.begin())
        op, want, pre, unit = twin.unit(T, True)
        assert (unit is not None) == legal
        sc.add(op, f"plan {P0} 14 14 {P0 + 14} {P0 + 14} {P0 + 14}" if legal else "refused long 0 2", pre)   # 4 + 5 rows fit, 14 do not
        assert want == sc.want[-1]
        sc.add("state", f"state {P0 + 14} {P0 + 14} 3 {P0 + 14} 3 ages 14 14" if legal else f"state {P0} {P0} 0 {P0} 0 ages 0 0")
        sc.after(twin)
        sc.check(driver)


def test_the_slot_record_is_trimmed_and_the_room_is_not_affected(driver):
    twin, sc = _Twin(False, 1, 1, 0, 24, True), _Script()       # Lmax = 24, Q = 1: a step advances 2 rows, the ring holds 12 steps
    sc.add(*twin.begin())
    for t in range(30):
        if t and t % 5 == 0:
            sc.add(*twin.restart([True]))
        elif twin.left_now() == [0]:
            sc.add(*twin.restart([True]))
        *line, unit = twin.unit(1, True)
        assert unit is not None
        sc.add(*line)
        sc.after(twin)                                          # the room of the untrimmed restatement at every step
    assert len(twin.book.slots) == 30
    sc.add("state", "state", True)
    sc.check(driver)
    assert _run(driver, sc.ops)[-1].split()[5] == "24"


def test_a_history_across_a_skipped_tail_has_the_skipped_rows_in_its_age(driver):
    twin, sc = _Twin(True, 2, 4, 4, 52, True), _Script()        # rows 4 .. 8, then 5 per step: step 8 ends at 48, step 9 does not fit in front of 52
    sc.add(*twin.begin())
    _steps(twin, sc, 10, restart_before=(5,))
    assert twin.book.slots[-2:] == [(44, 5), (5, 9)]            # step 9: 4 skipped rows + 5, action row 4, obs rows 5 .. 8
    sc.add("rows 2", "rows 14 44 45 46 47 4 5 6 7 8")
    assert twin.rows(2)[1] == sc.want[-1]
    sc.add(*twin.install(2, [False, True]))
    sc.add("state", "state 9 48 10 48 10 ages 29 14")
    assert twin.state()[1] == sc.want[-1]
    sc.after(twin)
    sc.check(driver)


@pytest.mark.parametrize("seq", [False, True])
def test_a_refused_install_changes_nothing(driver, seq):
    P0 = 4 if seq else 0
    twin, sc = _Twin(seq, 2, 4, P0, P0 + 24, True), _Script()   # a ring of 24 rows: 4 whole steps
    sc.add(*twin.begin())
    _steps(twin, sc, 9, restart_before=(4, 8))
    room = twin.room_now()
    assert 1 <= room < len(twin.book.slots)
    sc.add(*twin.state())
    before = sc.want[-1]
    sc.add(*twin.rows(room + 1))
    sc.add(*twin.install(room + 1, [True, True]))
    assert sc.want[-1] == sc.want[-2] == f"refused room {room}"
    sc.add(*twin.state())
    assert sc.want[-1] == before
    sc.after(twin)
    sc.check(driver)
