"""The host bookkeeping of the episode caches restated in Python, for the tests of the episode prefill (vima_decode_chunk,
vima_decode_restart_history): `_steps_left_model` of tests/test_rollout_gpu.py extended with chunk units and history ages.

One row index space of `lmax` rows for the batch. A call of T env steps is ONE unit of lq = T (Q + 1) rows (one fewer at batch step 0).
Linear: the unit goes behind the rows written so far and must end in front of lmax. Ring: it goes to the write pointer, or to row 0 after
skipping the tail when it does not fit; legal iff age[b] + advance <= lmax for every b. Every batch step leaves a slot (first obs row,
rows advanced); an installed history of T steps takes the last T slots and the age of a sample restarted right in front of them."""
from __future__ import annotations


def ring_next(wp, lq, lmax):
    """-> (row, advance): a unit's rows are never split across the wrap"""
    return (0, lmax - wp + lq) if wp + lq > lmax else (wp, lq)


class EpisodeBook:
    def __init__(self, B, Q, lmax, ring):
        self.B, self.Q, self.lmax, self.ring = B, Q, lmax, bool(ring)
        self.step = -1          # the last batch step taken
        self.wp = 0             # next row to write (ring: the write pointer; linear: the rows in use)
        self.age = [0] * B
        self.slots = []         # per batch step: (first obs row, rows advanced)

    # ------------------------------------------------------------------ units
    def plan(self, T=1):
        """(row, lq, advance) of the next unit of T steps; IndexError (nothing changes) when it is refused"""
        t = self.step + 1
        lq = T * (self.Q + 1) - (1 if t == 0 else 0)
        if not self.ring:
            row = t * (self.Q + 1) - 1 if t > 0 else 0
            if row + lq > self.lmax:
                raise IndexError(f"room for {max(0, (self.lmax + 1) // (self.Q + 1) - t)} more steps")
            return row, lq, lq
        if t == 0:
            if lq > self.lmax:
                raise IndexError("longer than n_positions")
            return 0, lq, lq
        row, adv = ring_next(self.wp, lq, self.lmax)
        for b in range(self.B):
            if self.age[b] + adv > self.lmax:
                raise IndexError(f"sample {b}")
        return row, lq, adv

    def advance(self, T=1):
        row, lq, adv = self.plan(T)
        t = self.step + 1
        if t == 0:
            self.age, self.slots = [0] * self.B, []
        has_act = 1 if t > 0 else 0
        for u in range(T):
            rows = self.Q if (t == 0 and u == 0) else self.Q + 1
            self.slots.append((row + u * (self.Q + 1) + has_act, adv - (T - 1) * (self.Q + 1) if u == 0 else rows))
        self.age = [a + adv for a in self.age]
        self.wp, self.step = row + lq, self.step + T
        return row, lq, adv

    # ------------------------------------------------------------------ restarts
    def restart(self, flags):
        self.age = [0 if f else a for f, a in zip(flags, self.age)]

    def history_room(self):
        if not self.ring:
            return len(self.slots)
        room, total = 0, 0
        for _, adv in reversed(self.slots):
            if total + adv > self.lmax:
                break
            total, room = total + adv, room + 1
        return room

    def history_rows(self, T):
        """cache rows of the compact history rows [o_0 (Q), a_0, o_1 (Q), a_1 ...]: step s in the slot of batch step t - T + s"""
        S = self.slots[len(self.slots) - T:]
        rows = []
        for s in range(T):
            rows += [S[s][0] + q for q in range(self.Q)]
            if s + 1 < T:
                rows.append(S[s + 1][0] - 1)
        return rows

    def install(self, flags, T):
        if T > self.history_room():
            raise IndexError(f"room for {self.history_room()}")
        age = sum(adv for _, adv in self.slots[len(self.slots) - T:]) if T else 0
        self.age = [age if f else a for f, a in zip(flags, self.age)]

    # ------------------------------------------------------------------ steps_left
    def steps_left(self):
        """per sample: how many further single steps would succeed if that sample alone were never restarted"""
        if not self.ring:
            return [max(0, (self.lmax + 1) // (self.Q + 1) - 1 - self.step)] * self.B
        out = []
        for b in range(self.B):
            n, wp, age = 0, self.wp, self.age[b]
            while True:
                row, adv = ring_next(wp, self.Q + 1, self.lmax)
                if age + adv > self.lmax:
                    break
                age, wp, n = age + adv, row + self.Q + 1, n + 1
            out.append(n)
        return out


def steps_left_single(ring, wp, age, step, lq, lmax):
    """`_steps_left_model` of tests/test_rollout_gpu.py, verbatim in meaning: the single-step bookkeeping EpisodeBook must reproduce at T = 1"""
    if not ring:
        return max(0, (lmax + 1) // lq - 1 - step)
    n = 0
    while True:
        adv, row = (lmax - wp + lq, 0) if wp + lq > lmax else (lq, wp)
        if age + adv > lmax:
            return n
        age, wp, n = age + adv, row + lq, n + 1


def chunk_schedule(steps, restarts, every=3, T=2):
    """[(t, T)] covering `steps` env steps: every `every`-th unit is a chunk of T steps where no restart falls inside it (restarts(t) ->
    flags of the restart right before step t) and it ends within `steps`; every other unit is one step"""
    units, t, due = [], 0, 0
    while t < steps:
        due += 1   # a chunk that is due waits for the first step where it is possible
        n = T if (due >= every and t + T <= steps and not any(any(restarts(t + j)) for j in range(1, T))) else 1
        due = 0 if n > 1 else due
        units.append((t, n))
        t += n
    return units


def selfcheck(seed=0, schedules=300):
    """The restatement checks itself on random schedules of restarts, single steps and chunks, ring and linear: (1) T = 1 units reproduce the
    single-step bookkeeping (`steps_left_single`, rows and advances restated inline); (2) an installed history has the age of a sample restarted
    right in front of those steps (kept independently per unit boundary); (3) the room never exceeds what the age rule allows: the installed age is
    at most lmax, the history's rows are distinct, and none of them has been overwritten or skipped since its step (a stamp per row). Returns the
    number of installs checked."""
    import copy
    import random
    rng = random.Random(seed)
    checked = 0
    for k in range(schedules):
        B, Q, lmax, ring = rng.randint(1, 4), rng.randint(1, 6), rng.randint(24, 96), k % 4 != 0
        book = EpisodeBook(B, Q, lmax, ring)
        only1 = k % 3 == 0                   # single steps only: against the single-step restatement
        wp, age = 0, [0] * B
        stamp = [-1] * lmax                  # the batch step (first of its unit) that last wrote or skipped the row
        unit_of = {}                         # batch step -> first step of its unit
        marks = {}                           # unit's first step -> age of a sample restarted right before it
        for _ in range(rng.randint(5, 60)):
            flags = [rng.random() < 0.25 for _ in range(B)]
            if ring and book.step >= 0:
                flags = [f or n == 0 for f, n in zip(flags, book.steps_left())]
            if book.step >= 0:
                book.restart(flags)
                age = [0 if f else a for f, a in zip(flags, age)]
                if only1:
                    assert book.steps_left() == [steps_left_single(ring, wp, a, book.step, Q + 1, lmax) for a in age]
            T = 1 if only1 else rng.choice([1, 1, 2, 3])
            before = copy.deepcopy(book.__dict__)
            try:
                row, lq, adv = book.plan(T)
            except IndexError:
                assert book.__dict__ == before
                if T == 1:
                    assert not ring, "ring: every sample out of steps was restarted, a single step must pass"
                    break
                continue
            t0, wp0 = book.step + 1, book.wp
            assert book.advance(T) == (row, lq, adv) and book.step == t0 + T - 1
            if t0 == 0:
                stamp, marks, unit_of = [-1] * lmax, {}, {}
            for r in (list(range(wp0, lmax)) + list(range(lq)) if adv > lq else range(row, row + lq)):
                stamp[r] = t0
            for u in range(T):
                unit_of[t0 + u] = t0
            marks[t0] = 0
            marks = {t: a + adv for t, a in marks.items()}
            if only1:
                lq1 = Q + 1 if t0 > 0 else Q
                if not ring:
                    r1, a1 = (t0 * (Q + 1) - 1 if t0 > 0 else 0), lq1
                else:
                    a1, r1 = (lmax - wp + lq1, 0) if (t0 > 0 and wp + lq1 > lmax) else (lq1, wp if t0 > 0 else 0)
                assert (row, lq, adv) == (r1, lq1, a1)
                age = [a + a1 for a in age] if t0 > 0 else [a1] * B
                wp = r1 + lq1
                if ring:
                    assert book.age == age
            room = book.history_room()
            assert 0 <= room <= len(book.slots) == book.step + 1
            for Th in sorted({1, room, rng.randint(1, max(1, room))}):
                if Th < 1 or Th > room:
                    continue
                rows = book.history_rows(Th)
                first = book.step + 1 - Th
                assert len(rows) == Th * (Q + 1) - 1 == len(set(rows)) and all(0 <= r < lmax for r in rows)
                # compact row i: obs rows of history step i // (Q + 1), or (i % (Q + 1) == Q) the action row of the NEXT step's slot
                assert all(stamp[r] == unit_of[first + (i + 1) // (Q + 1)] for i, r in enumerate(rows)), \
                    "a history row was overwritten or skipped after its step"
                probe = copy.deepcopy(book)
                probe.install([True] + [False] * (B - 1), Th)
                if ring:
                    assert probe.age[0] <= lmax and probe.age[1:] == book.age[1:]
                    if unit_of[first] == first:
                        assert probe.age[0] == marks[first], (probe.age[0], marks[first])
                checked += 1
            if room < len(book.slots):
                try:
                    copy.deepcopy(book).install([True] * B, room + 1)
                except IndexError:
                    pass
                else:
                    raise AssertionError("an install beyond the room was accepted")
    return checked
