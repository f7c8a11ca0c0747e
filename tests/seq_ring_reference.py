"""Pure-Python restatement of the ring bookkeeping of the decoder-only episode cache (option "seq_ring" of vima_seq_prefill /
vima_seq_decode_step / vima_seq_decode_restart; include/vima_hip.h), the schedules the GPU tests drive, and an fp64 restatement of the
windowed causal attention the ring stands on. No GPU, no library: tests/test_seq_ring_reference.py holds the properties of the schedules,
tests/test_seq_ring_gpu.py holds the library against this file.

Rows [0, P0), P0 = Lp + 1, of every sample's cache block are the fixed prefix (prompt + separator); rows [P0, Lmax) are the ring, R = Lmax - P0
rows, one row index space for the whole batch. wp = next row, hw = one past the highest row written since the prefill, age[b] = ring rows
advanced (skipped tail rows included) since sample b's episode began."""
import torch

# the scenario of the GPU tests: B samples, STEPS env steps, sample b restarted at every t > 0 with t % (2 + b) == 0
B, STEPS = 3, 26
Q = {"gato": 16, "gpt": 1}
RING = {"gato": 90, "gpt": 9}      # R: 90 = 5 * 17 + 5 (five whole steps and a tail per lap); 9 = 4 * 2 + 1


def restarts(t, never=()):
    return [t > 0 and t % (2 + b) == 0 and b not in never for b in range(B)]


class Refused(Exception):
    """The step is not legal: sample `sample` is the first with age + advance > R. Nothing has changed."""

    def __init__(self, sample, age, advance):
        super().__init__(f"sample {sample}: {age} + {advance} ring rows")
        self.sample, self.age, self.advance = sample, age, advance


def plan(wp, Lq, P0, Lmax):
    """(row, advance) of a step of Lq rows at write pointer wp: a step's rows are never split across the wrap."""
    if wp + Lq > Lmax:
        return P0, Lmax - wp + Lq
    return wp, Lq


class Ring:
    def __init__(self, Lp, Lmax, Q, B):
        self.P0, self.Lmax, self.Q, self.B = Lp + 1, Lmax, Q, B
        self.R = Lmax - self.P0
        self.prefill()

    def prefill(self):
        self.wp = self.hw = self.P0
        self.age = [0] * self.B
        self.next = 0              # the step number the next call carries

    def _lq(self, step):
        return self.Q + (1 if step > 0 else 0)

    def step(self):
        """Plan + legality + commit of one env step. Returns dict(row, Lq, advance, hw, has_act, wrap, tail): the step writes rows [row, row + Lq)
        and its attention reads [0, hw) with q_off = row, win_end = row + Lq; wrap: it skipped `tail` rows and went to P0."""
        Lq = self._lq(self.next)
        wrap = self.wp + Lq > self.Lmax
        row, adv = plan(self.wp, Lq, self.P0, self.Lmax)
        for b in range(self.B):
            if self.age[b] + adv > self.R:
                raise Refused(b, self.age[b], adv)
        self.age = [a + adv for a in self.age]
        self.wp = row + Lq
        self.hw = max(self.hw, self.wp)
        self.next += 1
        return dict(row=row, Lq=Lq, advance=adv, hw=self.hw, has_act=int(Lq > self.Q), wrap=wrap, tail=adv - Lq)

    def restart(self, flags):
        """A restart consumes no ring rows: the flagged samples' ages return to 0."""
        self.age = [0 if f else a for f, a in zip(flags, self.age)]

    def steps_left(self):
        """out[b]: further steps that would succeed if sample b alone were never restarted (the bookkeeping run forward)."""
        out = []
        for b in range(self.B):
            n, wp, age, Lq = 0, self.wp, self.age[b], self._lq(self.next)
            while True:
                row, adv = plan(wp, Lq, self.P0, self.Lmax)
                if age + adv > self.R:
                    break
                age, wp, Lq, n = age + adv, row + Lq, self.Q + 1, n + 1
            out.append(n)
        return out


def linear_steps_left(Lmax, used, Q, before_step0):
    """Ring off (the formula of tests/test_seq_step_gpu.py): every step takes Q + 1 rows, step 0 of the batch Q."""
    return (Lmax - used + (1 if before_step0 else 0)) // (Q + 1)


def run_schedule(kind, Lp, steps=STEPS, never=(), R=None):
    """The scenario through the restatement: returns (ring, [step dicts]). A refused step raises Refused with `.step` set, ring untouched."""
    R = RING[kind] if R is None else R
    ring = Ring(Lp, Lp + 1 + R, Q[kind], B)
    log = []
    for t in range(steps):
        flags = restarts(t, never)
        if any(flags):
            ring.restart(flags)
        try:
            log.append(ring.step())
        except Refused as e:
            e.step, e.ring, e.log = t, ring, log
            raise
    return ring, log


def episode_starts(steps=STEPS, never=()):
    """{(b, t0): t1}: sample b's episode that begins at step t0 ends one before t1."""
    ends = {}
    for b in range(B):
        starts = [0] + [t for t in range(1, steps) if restarts(t, never)[b]]
        for t0, t1 in zip(starts, starts[1:] + [steps]):
            ends[(b, t0)] = t1
    return ends


def lap_of_step(log):
    """1-based lap number of every step: a new lap begins at every step that wrapped to P0 (and at step 0)."""
    laps, lap = [], 0
    for i, s in enumerate(log):
        if i == 0 or s["wrap"]:
            lap += 1
        laps.append(lap)
    return laps


def graph_keys(log):
    """What a captured launch sequence of a step bakes in besides shapes and pointers."""
    return [(s["row"], s["hw"], s["has_act"]) for s in log]


# ---- the windowed causal rule, fp64 ----------------------------------------------------------------------------------------------------
def attn_window_f64(q, k, v, kmask, scale, q_off):
    """q [B, Lq, H, D], k / v [B, Lk, H, D], kmask bool [B, Lk] -> [B, Lq, H, D] in fp64. The step's rows are [q_off, win_end = q_off + Lq): key j is
    "future" for query i iff i + q_off < j < win_end and scores -1e4 (the reference's causal fill); keys below q_off (prefix and this lap's
    earlier rows) and from win_end on (older laps) are visible; a masked key's score is finfo(fp32).min."""
    q, k, v = q.double(), k.double(), v.double()
    Bq, Lq, H, D = q.shape
    Lk = k.shape[1]
    win_end = q_off + Lq
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    i = torch.arange(Lq)[:, None]
    j = torch.arange(Lk)[None, :]
    future = (j > i + q_off) & (j < win_end)
    s = torch.where(future[None, None], torch.full_like(s, -1e4), s)
    s = torch.where(kmask[:, None, None, :], s, torch.full_like(s, float(torch.finfo(torch.float32).min)))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v)
