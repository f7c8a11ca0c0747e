"""The host bookkeeping of the episode prefill of the decoder-only baselines (vima_seq_decode_chunk, vima_seq_decode_restart_history,
vima_seq_history_room; include/vima_hip.h) restated in Python on top of tests/seq_ring_reference.Ring: chunk units, the slot record, the
room, installs and steps_left. No GPU, no library: tests/test_seq_prefill_build.py holds the properties, tests/test_seq_prefill_gpu.py holds
the library against this file.

Rows [0, P0), P0 = Lp + 1, are the fixed prefix; the rows behind it are one row index space for the batch, linear or (option seq_ring) a ring
of R = Lmax - P0 rows. A call of T env steps is ONE unit of Lq = T (Q + 1) rows (one fewer at batch step 0: its first slot has no action
row). Every batch step leaves a slot (first obs row, rows advanced; a chunk's skipped tail counts with its first step). An installed history
of T steps takes the last T slots and the age of a sample restarted right in front of them."""
from __future__ import annotations

from tests import episode_prefill_reference as eref
from tests import seq_ring_reference as rr

B, STEPS = rr.B, rr.STEPS
Q = rr.Q
# R of the chunked ring rollout: the schedule below is refused at step 7 on the rings of tests/seq_ring_reference.py (90 / 9): a chunk of two
# steps skips a longer tail. 140 = 8 * 17 + 4, 11 = 5 * 2 + 1.
RING = {"gato": 140, "gpt": 11}
restarts = rr.restarts


def units():
    """[(t, T)]: the 26 steps, every third unit a chunk of 2 steps where no restart falls inside it"""
    return eref.chunk_schedule(STEPS, restarts, every=3, T=2)


class SeqBook:
    def __init__(self, Lp, Lmax, Qn, Bn, ring):
        self.ring = bool(ring)
        self.r = rr.Ring(Lp, Lmax, Qn, Bn)      # wp / hw / age / next; linear: wp = the rows in use, age unused
        self.P0, self.Lmax, self.Q, self.B, self.R = Lp + 1, Lmax, Qn, Bn, Lmax - Lp - 1
        self.slots = []                          # per batch step since the prefill: (first obs row, rows advanced)

    def prefill(self):
        self.r.prefill()
        self.slots = []

    # ------------------------------------------------------------------ units
    def plan(self, T=1):
        """(row, Lq, advance) of the next unit of T steps; IndexError (nothing changes) when it is refused"""
        r = self.r
        lq = T * (self.Q + 1) - (1 if r.next == 0 else 0)
        if not self.ring:
            if r.wp + lq > self.Lmax:
                raise IndexError(f"room for {(self.Lmax - r.wp + (1 if r.next == 0 else 0)) // (self.Q + 1)} more steps")
            return r.wp, lq, lq
        row, adv = rr.plan(r.wp, lq, self.P0, self.Lmax)
        for b in range(self.B):
            if r.age[b] + adv > self.R:
                raise IndexError(f"sample {b}")
        return row, lq, adv

    def advance(self, T=1):
        row, lq, adv = self.plan(T)
        r = self.r
        has_act = 1 if r.next > 0 else 0
        if self.ring and T == 1:
            s = r.step()                         # the single step IS Ring.step
            assert (s["row"], s["Lq"], s["advance"]) == (row, lq, adv)
        else:
            if self.ring:
                r.age = [a + adv for a in r.age]
            r.wp = row + lq
            r.hw = max(r.hw, r.wp)
            r.next += T
        for u in range(T):
            self.slots.append((row + u * (self.Q + 1) + has_act, adv - (T - 1) * (self.Q + 1) if u == 0 else self.Q + 1))
        self.slots = self.slots[-self.Lmax:]
        return row, lq, adv

    # ------------------------------------------------------------------ restarts, installs
    def restart(self, flags):
        self.r.restart(flags)

    def room(self):
        if not self.ring:
            return len(self.slots)
        room, total = 0, 0
        for _, adv in reversed(self.slots):
            if total + adv > self.R:
                break
            total, room = total + adv, room + 1
        return room

    def history_rows(self, T):
        """cache rows of the compact history rows [o_0 (Q), a_0, o_1 (Q), a_1 ..]: step s in the slot of batch step t - T + s"""
        S = self.slots[len(self.slots) - T:]
        rows = []
        for s in range(T):
            rows += [S[s][0] + q for q in range(self.Q)]
            if s + 1 < T:
                rows.append(S[s + 1][0] - 1)
        return rows

    def rowmap(self, T):
        """row l of [prompt | sep | history] -> cache row"""
        return list(range(self.P0)) + self.history_rows(T)

    def install(self, flags, T):
        if T > self.room():
            raise IndexError(f"room for {self.room()}")
        age = sum(adv for _, adv in self.slots[len(self.slots) - T:]) if T else 0
        self.r.age = [age if f else a for f, a in zip(flags, self.r.age)]

    def steps_left(self):
        if self.ring:
            return self.r.steps_left()
        return [rr.linear_steps_left(self.Lmax, self.r.wp, self.Q, self.r.next == 0)] * self.B


def selfcheck(seed=0, schedules=300):
    """Random schedules of restarts, single steps and chunks, ring and linear: (1) T = 1 units reproduce Ring.step (a twin Ring stepped alongside;
    linear: the rows restated inline); (2) an installed age equals that of a sample restarted right before step t - T; (3) the room never maps a
    history onto a row that has been overwritten or skipped since (a stamp per row) and a history's rows are distinct and behind the prefix.
    Returns the number of installs checked."""
    import copy
    import random
    rng = random.Random(seed)
    checked = 0
    for k in range(schedules):
        Bn, Qn, Lp, ring = rng.randint(1, 4), rng.randint(1, 6), rng.randint(1, 9), k % 4 != 0
        Lmax = Lp + 1 + rng.randint(3 * (Qn + 1), 96)
        book = SeqBook(Lp, Lmax, Qn, Bn, ring)
        only1 = k % 3 == 0
        twin = rr.Ring(Lp, Lmax, Qn, Bn)
        used = Lp + 1
        stamp = [-1] * Lmax
        unit_of, marks = {}, {}
        for _ in range(rng.randint(5, 60)):
            flags = [rng.random() < 0.25 for _ in range(Bn)]
            if ring:
                flags = [f or n == 0 for f, n in zip(flags, book.steps_left())]
            book.restart(flags)
            twin.restart(flags)
            T = 1 if only1 else rng.choice([1, 1, 2, 3])
            before = copy.deepcopy(book.__dict__)
            try:
                row, lq, adv = book.plan(T)
            except IndexError:
                assert book.r.__dict__ == before["r"].__dict__ and book.slots == before["slots"]
                if T == 1:
                    assert not ring, "ring: every sample out of steps was restarted, a single step must pass"
                    break
                continue
            t0, wp0 = book.r.next, book.r.wp
            assert book.advance(T) == (row, lq, adv) and book.r.next == t0 + T
            for r in (list(range(wp0, Lmax)) + list(range(book.P0, book.P0 + lq)) if adv > lq else range(row, row + lq)):
                stamp[r] = t0
            for u in range(T):
                unit_of[t0 + u] = t0
            marks[t0] = 0
            marks = {t: a + adv for t, a in marks.items()}
            if only1:
                if ring:
                    s = twin.step()
                    assert (s["row"], s["Lq"], s["advance"]) == (row, lq, adv)
                    assert (twin.wp, twin.hw, twin.age, twin.next) == (book.r.wp, book.r.hw, book.r.age, book.r.next)
                    assert twin.steps_left() == book.steps_left()
                else:
                    lq1 = Qn + (1 if t0 > 0 else 0)
                    assert (row, lq, adv) == (used, lq1, lq1)
                    used += lq1
                    assert book.steps_left() == [rr.linear_steps_left(Lmax, used, Qn, False)] * Bn
            room = book.room()
            assert 0 <= room <= len(book.slots) == min(book.r.next, Lmax)      # the record is trimmed to the last Lmax steps
            if not ring:
                assert room == book.r.next
            for Th in sorted({1, room, rng.randint(1, max(1, room))}):
                if Th < 1 or Th > room:
                    continue
                rows = book.history_rows(Th)
                first = book.r.next - Th
                assert len(rows) == Th * (Qn + 1) - 1 == len(set(rows)) and all(book.P0 <= r < Lmax for r in rows)
                assert all(stamp[r] == unit_of[first + (i + 1) // (Qn + 1)] for i, r in enumerate(rows)), \
                    "a history row was overwritten or skipped after its step"
                assert book.rowmap(Th)[:book.P0] == list(range(Lp + 1))
                probe = copy.deepcopy(book)
                probe.install([True] + [False] * (Bn - 1), Th)
                if ring:
                    assert probe.r.age[0] <= book.R and probe.r.age[1:] == book.r.age[1:]
                    if unit_of[first] == first:
                        assert probe.r.age[0] == marks[first], (probe.r.age[0], marks[first])
                checked += 1
            if room < len(book.slots):
                try:
                    copy.deepcopy(book).install([True] * Bn, room + 1)
                except IndexError:
                    pass
                else:
                    raise AssertionError("an install beyond the room was accepted")
    return checked


def chunked_ring_properties(kind, Lp, R=None):
    """The chunked ring schedule through the restatement -> dict(wraps, chunks, chunk_skips, chunk_fresh, legal, refused_at, log): log[i] = (t, T,
    row, Lq, advance, flags) per unit."""
    R = RING[kind] if R is None else R
    book = SeqBook(Lp, Lp + 1 + R, Q[kind], B, True)
    out = dict(wraps=0, chunks=0, chunk_skips=0, chunk_fresh=0, legal=True, refused_at=None, log=[])
    for t, T in units():
        flags = restarts(t)
        if any(flags):
            book.restart(flags)
        try:
            row, lq, adv = book.advance(T)
        except IndexError:
            out["legal"], out["refused_at"] = False, t
            break
        out["wraps"] += adv > lq
        out["chunks"] += T > 1
        out["chunk_skips"] += T > 1 and adv > lq
        out["chunk_fresh"] += T > 1 and any(flags)
        out["log"].append((t, T, row, lq, adv, flags))
    out["book"] = book
    return out
