"""Brute-force restatement of the snapshot / restore bookkeeping on top of the row log of tests/episode_fork_reference.py::Book, independent of
vima_amd/csrc/episode_book.h, and the snapshot scenario the GPU tests run (tests/test_episode_snapshot_gpu.py), so that
tests/test_episode_snapshot_build.py can assert on the CPU what that scenario contains.

The restatement derives everything from the LOG of advanced rows: the episode of a sample that has taken n steps is the last R = n (Q + 1) - 1
WRITTEN rows of the log (a step writes [action row, Q obs rows], the action of step s in front of the obs rows of step s + 1; the compact order
[o_0, a_0, o_1, ..] is the write order minus the leading action row), and n is found by trying every suffix of the per-step advances."""
from tests.episode_fork_reference import Book, ranges_of  # noqa: F401


class SnapBook(Book):
    def steps_of(self, b):
        hits = [n for n in range(len(self.adv) + 1) if sum(self.adv[len(self.adv) - n:]) == self.age[b]]
        return hits[0] if hits else -1

    def rows_of_last(self, n):
        """cache rows of the compact rows of the last n batch steps, in compact order"""
        R = max(n * (self.Q + 1) - 1, 0)
        written = [r for r in self.log if r is not None]
        assert R <= len(written)
        return written[len(written) - R:] if R else []

    def snapshot(self, b):
        """-> (n, rows at this moment)"""
        n = self.steps_of(b)
        assert n >= 0 and n <= self.room()
        return n, self.rows_of_last(n)

    def restore(self, slots, n):
        """-> (age, rows), or None when the snapshot does not fit (nothing changes)"""
        if n > self.room():
            return None
        age = sum(self.adv[len(self.adv) - n:]) if n else 0
        for d in slots:
            self.age[d] = age
        return age, self.rows_of_last(n)


def straddles(rows):
    """the rows of a restore go down somewhere: they lie on both sides of a wrap"""
    return any(b < a for a, b in zip(rows, rows[1:]))


# ---------------------------------------------------------------------------------------------------- the GPU scenario
# model 4M, n_positions 48, B = 4, Q = 4 (tests/episode_fork_reference.py): 4 ring rows at step 0, 5 per step after it; steps 9, 18, 27 and 36 skip
# the tail and go to row 0. Sample b restarts in front of every step t > 0 with t % (3 + b) == 0. Slot b is fed column b of the step's data.
NPOS, B, Q, STEPS = 48, 4, 4, 40
LINEAR_STEPS = 9


def restarts(t):
    return [t > 0 and t % (3 + b) == 0 for b in range(B)]


INSTALLS = {14: (1, 2)}             # in front of step 14 sample 1 is re-installed with its own last 2 steps (restart_samples(history=))
FORKS = {21: [0, 1, 1, 3]}          # slot 2 continues the episode of slot 1 (restarted in front of step 20)
CHUNKS = {22: 2}                    # steps 22 and 23 run as one forward_steps chunk
# in front of step t, after restarts, installs and forks: name -> (sample, with_prompt)
SNAPSHOTS = {
    9: {"fresh": (0, True)},        # sample 0 restarted in front of this very step: n = 0
    10: {"wrapped": (3, True)},     # sample 3: steps 6 .. 9, behind the wrap of step 9 -> two live ranges
    12: {"back": (2, False)},       # sample 2: steps 10, 11; prompt-less, for the backtrack inside its own episode
    14: {"installed": (1, True)},   # sample 1 carries the history installed in front of this step
    22: {"forked": (2, True)},      # slot 2 is the destination of the fork in front of step 21
}
# in front of step t, after the snapshots: (name, slots)
RESTORES = {
    10: [("fresh", [1])],           # n = 0: only the prompt and fresh = 1 travel
    14: [("back", [2])],            # into its own slot two steps later, without the prompt: a backtrack inside the prompt group
    16: [("installed", [3])],
    19: [("wrapped", [0, 1])],      # two slots; the last 4 steps 15 .. 18 straddle the wrap of step 18
    24: [("forked", [3])],          # right after the chunk of T = 2: the rows go to the chunk's slots
    37: [("installed", [2])],       # three laps later; steps 35, 36 straddle the wrap of step 36
}
LINEAR_SNAPSHOTS = {3: {"lin": (1, True)}}
LINEAR_RESTORES = {6: [("lin", [0, 2])]}


def events(t, ring=True):
    """-> (restart flags, install, source map, chunk length, snapshots, restores) in front of step t"""
    if not ring:
        return [False] * B, None, None, 1, LINEAR_SNAPSHOTS.get(t, {}), LINEAR_RESTORES.get(t, [])
    return restarts(t), INSTALLS.get(t), FORKS.get(t), CHUNKS.get(t, 1), SNAPSHOTS.get(t, {}), RESTORES.get(t, [])


def replay(ring=True):
    """The scenario on the restatement -> (snapshot records, restore records, steps_left in front of every step, final book). Asserts that every
    operation of the scenario is legal."""
    bk = SnapBook(B, Q, 0, NPOS, ring)
    held, snaps, rests, left = {}, [], [], {}
    installed, forked = [False] * B, [False] * B
    last_chunk = 1
    t, steps = 0, STEPS if ring else LINEAR_STEPS
    while t < steps:
        flags, inst, source, T, snap, rest = events(t, ring)
        if any(flags):
            bk.restart(flags)
            installed = [i and not f for i, f in zip(installed, flags)]
            forked = [i and not f for i, f in zip(forked, flags)]
        if inst:
            b, n = inst
            assert bk.steps_of(b) == n, "the scenario re-installs a sample with exactly its own episode"
            bk.restart([x == b for x in range(B)])
            bk.install([x == b for x in range(B)], n)
            installed[b] = True
        if source:
            assert bk.fork_ok(source)
            bk.fork(source)
            installed = [installed[s] for s in source]
            forked = [forked[s] or s != b for b, s in enumerate(source)]
        for name, (b, with_prompt) in snap.items():
            n, rows = bk.snapshot(b)
            held[name] = dict(name=name, t=t, sample=b, n=n, rows=rows, ranges=ranges_of(bk.live_rows(b)), with_prompt=with_prompt,
                              installed=installed[b], forked=forked[b], restarted_now=flags[b])
            snaps.append(held[name])
        for name, slots in rest:
            s = held[name]
            got = bk.restore(slots, s["n"])
            assert got is not None, f"the restore of {name} in front of step {t} does not fit"
            rests.append(dict(name=name, t=t, slots=slots, n=s["n"], rows=got[1], age=got[0], taken=s["t"], own_slot=slots == [s["sample"]],
                              with_prompt=s["with_prompt"], after_chunk=last_chunk))
            for d in slots:
                installed[d], forked[d] = s["installed"], s["forked"]
        left[t] = [bk.steps_left(b) for b in range(B)]
        assert bk.step(T) is not None, f"step {t} of the scenario is refused"
        last_chunk = T
        t += T
    return snaps, rests, left, bk
