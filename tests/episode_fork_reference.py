"""Brute-force restatement of the episode-cache bookkeeping with forks, independent of vima_amd/csrc/episode_book.h, and the fork scenario the GPU
tests run (tests/test_episode_fork_gpu.py), so that tests/test_episode_fork_build.py can assert on the CPU what that scenario contains.

The restatement keeps a LOG of every row advanced since `begin`: the row number, or None for a row of a skipped tail. A sample's live rows are the
written rows among the last age[b] log entries; a fork copies the age. Nothing else is derived from the C++."""


class Book:
    def __init__(self, B, Q, P0, Lmax, ring):
        self.B, self.Q, self.P0, self.Lmax, self.ring = B, Q, P0, Lmax, bool(ring)
        self.wp = self.hw = P0
        self.next = 0
        self.age = [0] * B
        self.log = []          # one entry per advanced row
        self.adv = []          # rows advanced per batch step (a chunk's skipped tail counts with its first step)

    def _place(self, wp, lq):
        """-> (first row, rows advanced)"""
        return (self.P0, self.Lmax - wp + lq) if wp + lq > self.Lmax else (wp, lq)

    def _legal(self, age, wp, lq):
        row, adv = self._place(wp, lq)
        return age + adv <= self.Lmax - self.P0 if self.ring else wp + lq <= self.Lmax

    def plan(self, T):
        """-> (row, lq, advance), or None when the unit is refused"""
        lq = T * (self.Q + 1) - (1 if self.next == 0 else 0)
        if (lq > self.Lmax - self.P0) if self.ring else (self.wp + lq > self.Lmax):
            return None
        if not all(self._legal(a, self.wp, lq) for a in self.age):
            return None
        row, adv = self._place(self.wp, lq)
        return row, lq, adv

    def step(self, T=1):
        p = self.plan(T)
        if p is None:
            return None
        row, lq, adv = p
        self.log += [None] * (adv - lq) + list(range(row, row + lq))
        self.adv += [adv - (T - 1) * (self.Q + 1)] + [self.Q + 1] * (T - 1)
        self.age = [a + adv for a in self.age]
        self.wp, self.hw, self.next = row + lq, max(self.hw, row + lq), self.next + T
        return p

    def restart(self, flags):
        self.age = [0 if f else a for f, a in zip(flags, self.age)]

    def room(self):
        r = s = 0
        for a in reversed(self.adv):
            if s + a > self.Lmax - self.P0:
                break
            r, s = r + 1, s + a
        return r

    def install(self, flags, T):
        assert 1 <= T <= self.room()
        a = sum(self.adv[len(self.adv) - T:])
        self.age = [a if f else x for f, x in zip(flags, self.age)]

    def fork_ok(self, source):
        return len(source) == self.B and all(0 <= s < self.B for s in source) and all(source[s] == s for s in source)

    def fork(self, source):
        assert self.fork_ok(source)
        self.age = [self.age[s] for s in source]

    def live_rows(self, b):
        a = self.age[b]
        return {r for r in self.log[len(self.log) - a:] if r is not None} if a else set()

    def steps_left(self, b):
        n, wp, a, lq = 0, self.wp, self.age[b], self.Q + (1 if self.next > 0 else 0)
        while self._legal(a, wp, lq):
            row, adv = self._place(wp, lq)
            n, wp, a, lq = n + 1, row + lq, a + adv, self.Q + 1
        return n


# ---------------------------------------------------------------------------------------------------- the GPU scenario
# model 4M, n_positions 48, B = 4, Q = 4 (2 per view): 4 ring rows at step 0, 5 per step after it; the write pointer runs 4, 9 .. 44, step 9 skips
# the tail [44, 48) and goes to row 0; from then on a lap is 9 steps (wp 5 .. 45, a skip of 3), wrapping at steps 18, 27 and 36.
NPOS, B, Q, STEPS = 48, 4, 4, 40
LINEAR_STEPS = 9                      # the linear cache holds steps 0 .. 8


def restarts(t):
    """sample b starts a new episode (new prompt) in front of every step t > 0 with t % (3 + b) == 0, as in tests/test_rollout_gpu.py"""
    return [t > 0 and t % (3 + b) == 0 for b in range(B)]


# in front of step t, after the step's restarts: sample -> number of its own last steps it is re-installed with (restart_samples(history=))
INSTALLS = {14: (1, 2)}
# in front of step t, after restarts and installs: the source map
FORKS = {
    10: [3, 1, 2, 3],    # source 3: episode of steps 6 .. 9, behind the wrap of step 9 -> two live ranges, in a lap that began with a skipped tail
    12: [0, 1, 0, 3],    # source 0 restarted in front of this very step: age 0
    14: [0, 1, 2, 1],    # source 1 carries the history installed in front of this step
    22: [0, 2, 2, 2],    # two destinations
    28: [3, 1, 3, 3],    # two destinations; source 3: steps 24 .. 27, behind the wrap of step 27
    33: [0, 0, 2, 2],    # two groups in one call; source 0 of age 0
}
LINEAR_FORKS = {5: [0, 0, 2, 0]}     # the linear cache: mid-episode, two destinations


def events(t, ring=True):
    """-> (restart flags, (sample, T) or None, source map or None) in front of step t"""
    if not ring:
        return [False] * B, None, LINEAR_FORKS.get(t)
    return restarts(t), INSTALLS.get(t), FORKS.get(t)


def replay(ring=True):
    """The scenario on the restatement. -> one record per fork: dict(t, source, book ages before, live rows of every source, wraps so far),
    and the final book. Asserts that every restart, install, fork and step of the scenario is legal."""
    bk = Book(B, Q, 0, NPOS, ring)
    forks, skipped = [], 0
    installed = [False] * B            # the sample's current episode carries an installed history
    for t in range(STEPS if ring else LINEAR_STEPS):
        flags, inst, source = events(t, ring)
        if any(flags):
            bk.restart(flags)
            installed = [i and not f for i, f in zip(installed, flags)]
        if inst:
            b, T = inst
            assert bk.age[b] == sum(bk.adv[len(bk.adv) - T:]), "the scenario re-installs a sample with exactly its own episode"
            bk.restart([x == b for x in range(B)])
            bk.install([x == b for x in range(B)], T)
            installed[b] = True
        if source:
            assert bk.fork_ok(source)
            srcs = sorted({s for b, s in enumerate(source) if s != b})
            forks.append(dict(t=t, source=source, ages={s: bk.age[s] for s in srcs}, live={s: bk.live_rows(s) for s in srcs},
                              installed={s: installed[s] for s in srcs}, skipped_tails=skipped,
                              n_dst={s: sum(1 for b, x in enumerate(source) if x == s and b != s) for s in srcs}))
            bk.fork(source)
            installed = [installed[s] for s in source]
        p = bk.step(1)
        assert p is not None, f"step {t} of the scenario is refused"
        skipped += p[2] > p[1]
    return forks, bk


def ranges_of(rows):
    """a set of rows -> its maximal runs [(lo, hi)]"""
    out = []
    for r in sorted(rows):
        if out and out[-1][1] == r:
            out[-1][1] = r + 1
        else:
            out.append([r, r + 1])
    return [tuple(x) for x in out]
