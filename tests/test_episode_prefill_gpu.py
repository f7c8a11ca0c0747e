"""Episode prefill on the MI355X: `VIMAPolicy.forward_steps` (vima_decode_chunk: T env steps as one pass of the incremental branch) and
`restart_samples(..., history=)` / `history_room()` (vima_decode_restart_history: an in-flight episode joins a running batch).

Scenario and yardstick of tests/test_rollout_gpu.py: model 4M, n_positions 48, B = 3, Q = 4 (5 cache rows per step, 4 at step 0), prompts of
3 segments x 3 words, make_state_dict(cfg, 5); a second configuration with n_positions 128 for the chunk sizes that reach the other causal
attention kernels. Reference: the full-history `forward` of one (sample, episode) alone on a policy with the ring off; gates: that file's TOL
(error / max(1, |ref|) <= 2e-5 fp32, 3e-2 bf16, 2e-5 bf16x3). Every test prints its worst observed value (profiles/episode_prefill_pytest.txt).
The host bookkeeping is held against its restatement in tests/episode_prefill_reference.py."""
import dataclasses

import pytest
import torch

from tests.episode_prefill_reference import EpisodeBook, chunk_schedule
from tests.gpu_common import max_abs
from tests.test_rollout_gpu import B, CFG, DEV, NPOS, Q, QV, STEPS, TOL, X3, _data, _policy, _prompt, _restarts, _state_dict
from vima_amd.baselines import VIMAGPTPolicy
from vima_amd.policy import VIMAPolicy
from vima_testing import synthetic as syn
from oracle.vima_oracle import OraclePolicy

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "bf16", X3]


class Run:
    """A batch stepping through the scenario's token streams. Sample b at batch step t is fed otok[t + delta, sb] with (sb, delta) = feed[b]
    (its own stream, (b, 0), unless a history from another stream was installed) and, from its second step on, atok[t - 1 + delta, sb]."""

    def __init__(self, pol, otok, omask, atok, static=False):
        self.pol, self.otok, self.omask, self.atok = pol, otok, omask, atok
        self.t = 0
        pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
        self.pt, self.pm = pt.clone(), pm.clone()
        self.episode = [0] * B
        self.episodes = {(b, 0): (self.pt[:, b:b + 1].clone(), self.pm[b:b + 1].clone()) for b in range(B)}
        self.feed = [(b, 0) for b in range(B)]
        self.outs = {}
        self.static = static
        if static:   # graph replay needs the step's inputs and output at fixed addresses: fixed input buffers, and nothing else allocated per step
            self.so, self.sm, self.sa = torch.empty_like(otok[0]), torch.empty_like(omask[0]), torch.empty_like(atok[0])
            self.kept = torch.empty(otok.shape[0], B, otok.shape[-1], device=DEV)
            # ... every later episode's prompt up front, as _rollout of tests/test_rollout_gpu.py does: between two steps nothing is allocated and kept
            self.prompts = {(b, e): pol.forward_prompt_assembly(syn.to_device(syn.cut_prompt(_prompt(e), [b]), DEV)) for b in range(B) for e in range(1, 16)}
            self.prompts = {k: (nt.clone(), nm.clone()) for k, (nt, nm) in self.prompts.items()}

    def set_prompt(self, b, ptok, pmask):
        self.pt[:, b], self.pm[b] = ptok[:, 0], pmask[0]

    def restart(self, flags):
        """the plain restart of the scenario: every flagged sample starts its next episode's prompt"""
        if not any(flags):
            return
        for b in range(B):
            if flags[b]:
                self.episode[b] += 1
                if self.static:
                    self.episodes[(b, self.t)] = nt, nm = self.prompts[(b, self.episode[b])]
                else:
                    nt, nm = self.pol.forward_prompt_assembly(syn.to_device(syn.cut_prompt(_prompt(self.episode[b]), [b]), DEV))
                    self.episodes[(b, self.t)] = (nt.clone(), nm.clone())
                self.set_prompt(b, nt, nm)
                self.feed[b] = (b, 0)
        self.pol.restart_samples(torch.tensor(flags), self.pt, self.pm)

    def install(self, targets, sources, T, ptoks):
        """samples `targets` (increasing) take the last T steps of streams `sources` = [(sb, i1)]: tokens otok[i1 - T : i1, sb]; they go on at i1"""
        flags = [b in targets for b in range(B)]
        for b, (sb, i1), (ptok, pmask) in zip(targets, sources, ptoks):
            self.set_prompt(b, ptok, pmask)
        h_obs = torch.stack([self.otok[i1 - T:i1, sb] for sb, i1 in sources], dim=1).contiguous()
        h_mask = torch.stack([self.omask[i1 - T:i1, sb] for sb, i1 in sources], dim=1).contiguous()
        h_act = torch.stack([self.atok[i1 - T:i1 - 1, sb] for sb, i1 in sources], dim=1).contiguous() if T > 1 else None
        out = self.pol.restart_samples(torch.tensor(flags), self.pt, self.pm, history=(h_obs, h_mask, h_act))
        for b, (sb, i1) in zip(targets, sources):
            self.feed[b] = (sb, i1 - self.t)
        return out

    def _inputs(self, t, static=False):
        if static:
            o, m, a = self.so, self.sm, (self.sa if t > 0 else None)
            o.copy_(self.otok[t]); m.copy_(self.omask[t])
            if t > 0:
                a.copy_(self.atok[t - 1])
        else:
            o, m, a = self.otok[t].clone(), self.omask[t].clone(), self.atok[t - 1].clone() if t > 0 else None
        for b, (sb, d) in enumerate(self.feed):
            if (sb, d) != (b, 0):
                o[b], m[b] = self.otok[t + d, sb], self.omask[t + d, sb]
                a[b] = self.atok[t - 1 + d, sb]
        return o, m, a

    def run(self, T=1):
        t = self.t
        if T == 1 and self.static:   # like _rollout(static=True) of tests/test_rollout_gpu.py: the output block is freed before the next step asks for it
            o, m, a = self._inputs(t, static=True)
            out = self.pol.forward_step(o, m, a, self.pt, self.pm, step=t)
            self.kept[t].copy_(out)
            del out
            self.outs[t] = self.kept[t]
            self.t += 1
            return None
        ins = [self._inputs(t + j) for j in range(T)]
        if T == 1:
            o, m, a = ins[0]
            out = self.pol.forward_step(o, m, a, self.pt, self.pm, step=t).unsqueeze(0)
        else:
            acts = [a for _, _, a in ins if a is not None]
            out = self.pol.forward_steps(torch.stack([o for o, _, _ in ins]), torch.stack([m for _, m, _ in ins]), torch.stack(acts),
                                         self.pt, self.pm, step=t)
        for j in range(T):
            if self.static:
                self.kept[t + j].copy_(out[j])
            self.outs[t + j] = self.kept[t + j] if self.static else out[j].clone()
        self.t += T
        return None if self.static else out


def _reference(ref_pol, otok, omask, atok, sb, i0, i1, ptok, pmask):
    """[i1 - i0, E]: the full-history forward of stream sb, rows i0 .. i1 - 1, alone"""
    act = atok[i0:i1 - 1, sb:sb + 1].contiguous() if i1 - i0 > 1 else None
    return ref_pol.forward(otok[i0:i1, sb:sb + 1].contiguous(), omask[i0:i1, sb:sb + 1].contiguous(), act, ptok, pmask)[:, 0]


def _err(got, ref):
    assert torch.isfinite(got).all()
    return max_abs(got, ref) / max(1.0, ref.abs().max().item())


def _check_episodes(ref_pol, run, tol, steps):
    """every (sample, episode) of a run that only restarted plainly, against its full history"""
    worst = 0.0
    for b in range(B):
        starts = sorted(t for (bb, t) in run.episodes if bb == b)
        for t0, t1 in zip(starts, starts[1:] + [steps]):
            full = _reference(ref_pol, run.otok, run.omask, run.atok, b, t0, t1, *run.episodes[(b, t0)])
            for t in range(t0, t1):
                e = _err(run.outs[t][b], full[t - t0])
                worst = max(worst, e)
                assert e <= tol, (b, t0, t, e)
    return worst


# ------------------------------------------------------------------------------------------ 1. chunk = steps
@pytest.mark.parametrize("prec", PRECS)
def test_chunks_equal_the_steps_they_replace(prec):
    """Linear cache: T = 3 at step 0, T = 2 at step 3, then single steps to the end of the cache (step 8)."""
    pol, ref_pol = _policy(prec), _policy(prec)
    obs, acts, otok, omask, atok = _data(pol, 10)
    run = Run(pol, otok, omask, atok)
    for T in (3, 2, 1, 1, 1, 1):
        run.run(T)
        assert pol.steps_left().tolist() == [9 - run.t] * B
    assert run.t == 9
    worst = _check_episodes(ref_pol, run, TOL[prec], 9)
    print(f"[prefill] chunk = steps, {prec}: worst error / max(1, |ref|) {worst:.3e} (bound {TOL[prec]:.0e})")
    if prec == "fp32":   # one episode's logits against the CPU oracle's own pipeline (the bound of the rollout test's third-lap check)
        b = 1
        orc = OraclePolicy(_state_dict(), **CFG.ctor_kwargs())
        o = obs["objects"]
        cut = {"objects": type(o)({k: type(o[k])({v: o[k][v][0:9, b:b + 1] for v in o[k]}) for k in o}), "ee": obs["ee"][0:9, b:b + 1]}
        ptok, pmask = orc.forward_prompt_assembly(syn.cut_prompt(_prompt(0), [b]))
        o_otok, o_omask = orc.forward_obs_token(cut)
        o_atok = orc.forward_action_token({k: v[0:8, b:b + 1] for k, v in acts.items()})
        want = orc.action_logits(orc.forward(o_otok, o_omask, o_atok, ptok, pmask))[:, 0]
        got = pol.action_logits(torch.stack([run.outs[t][b] for t in range(9)]))
        err = max_abs(got, want)
        print(f"[prefill] fp32 logits of a chunked episode vs the oracle: {err:.3e} (bound 2e-5), max |logit| {want.abs().max().item():.3g}")
        assert err < 2e-5, err


@pytest.mark.parametrize("ring", [0, 1])
def test_a_chunk_of_one_step_is_forward_step(ring):
    pol, twin = _policy("bf16", decode_ring=ring), _policy("bf16", decode_ring=ring)
    _, _, otok, omask, atok = _data(pol, 4)
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    for t in range(4):
        a = atok[t - 1:t] if t > 0 else None
        got = pol.forward_steps(otok[t:t + 1], omask[t:t + 1], a, pt, pm, step=t)
        want = twin.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t > 0 else None, pt, pm, step=t)
        assert got.shape == (1, B, otok.shape[-1]) and torch.equal(got[0], want), t


# ------------------------------------------------------------------------------------------ 2. every causal kernel behind a chunk
NPOS2 = 128
CFG2 = dataclasses.replace(syn.config("4M"), n_positions=NPOS2)
# (T, first step s): Lq = 5 T rows against s * 5 - 1 + Lq >= 64 keys -- Lq 15: the split-key kernel, 35: the one-wave kernel, 65: the four-wave kernel
CHUNKS2 = [(3, 10), (7, 6), (13, 2)]
STEPS2 = 16
_ref2 = {}


def _policy2(prec, **opts):
    pol = VIMAPolicy(**CFG2.ctor_kwargs(), n_positions=NPOS2, precision=prec, device=DEV)
    if "sd" not in _ref2:
        _ref2["sd"] = syn.make_state_dict(CFG2, 5)
    pol.load_state_dict(_ref2["sd"], strict=True)
    for k, v in opts.items():
        pol.set_option(k, v)
    return pol


def _reference2(prec, otok, omask, atok, pt, pm):
    """computed once per precision and shared: [STEPS2, B, E], each sample alone"""
    if prec not in _ref2:
        ref_pol = _policy2(prec)
        _ref2[prec] = torch.stack([_reference(ref_pol, otok, omask, atok, b, 0, STEPS2, pt[:, b:b + 1].contiguous(), pm[b:b + 1].contiguous())
                                   for b in range(B)], dim=1)
    return _ref2[prec]


@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("prec", PRECS)
def test_every_causal_kernel_behind_a_chunk(prec, impl, ring):
    assert all(s * (Q + 1) - 1 + T * (Q + 1) >= 64 and s + T < STEPS2 for T, s in CHUNKS2)
    pol = _policy2(prec, attn_impl=impl, decode_ring=ring)
    _, _, otok, omask, atok = _data(pol, STEPS2)
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    ref = _reference2(prec, otok, omask, atok, pt, pm)
    single = [pol.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t > 0 else None, pt, pm, step=t).clone() for t in range(STEPS2)]
    worst, worst_kv = 0.0, 0.0
    for T, s in CHUNKS2:
        for t in range(s):
            pol.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t > 0 else None, pt, pm, step=t)
        out = pol.forward_steps(otok[s:s + T].contiguous(), omask[s:s + T].contiguous(), atok[s - 1:s + T - 1].contiguous(), pt, pm, step=s)
        for j in range(T):
            for b in range(B):
                e = _err(out[j, b], ref[s + j, b])
                worst = max(worst, e)
                assert e <= TOL[prec], (T, s, j, b, e)
        # the chunk's K / V rows, through the next step: it reads them all
        t = s + T
        nxt = pol.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1], pt, pm, step=t)
        for b in range(B):
            e = _err(nxt[b], ref[t, b])
            worst = max(worst, e)
            assert e <= TOL[prec], (T, s, "next", b, e)
        kv = (nxt - single[t]).abs().max().item() / single[t].abs().max().item()
        worst_kv = max(worst_kv, kv)
        if prec != "bf16":
            assert kv <= 2e-5, (T, s, kv)
    print(f"[prefill] kernels behind a chunk, {prec} impl {impl} ring {ring}: worst error / max(1, |ref|) {worst:.3e} (bound {TOL[prec]:.0e}); "
          f"next step after the chunk vs after single steps, relative {worst_kv:.3e}" + (" (bound 2e-5)" if prec != "bf16" else " (not gated in bf16)"))


# ------------------------------------------------------------------------------------------ 3. chunks in a ring rollout
@pytest.mark.parametrize("prec", PRECS)
def test_ring_rollout_with_chunks_matches_every_episode_alone(prec):
    """The 40-step staggered-restart scenario with every third unit a 2-step chunk (where no restart falls inside it)."""
    units = chunk_schedule(STEPS, _restarts, every=3, T=2)
    pol, ref_pol = _policy(prec, decode_ring=1), _policy(prec)
    _, _, otok, omask, atok = _data(pol)
    run, book = Run(pol, otok, omask, atok), EpisodeBook(B, Q, NPOS, True)
    wraps = skipped_by_chunk = restarted_before_chunk = 0
    for t, T in units:
        flags = _restarts(t)
        run.restart(flags)
        if t > 0:
            book.restart(flags)
            assert pol.steps_left().tolist() == book.steps_left(), t
        row, lq, adv = book.advance(T)
        wraps += adv > lq
        skipped_by_chunk += T > 1 and adv > lq
        restarted_before_chunk += T > 1 and any(flags)
        run.run(T)
        assert pol.steps_left().tolist() == book.steps_left() and pol.history_room() == book.history_room(), t
    assert run.t == STEPS and wraps >= 3 and skipped_by_chunk >= 1 and restarted_before_chunk >= 1 and sum(T > 1 for _, T in units) >= 7
    worst = _check_episodes(ref_pol, run, TOL[prec], STEPS)
    print(f"[prefill] ring rollout with {sum(T > 1 for _, T in units)} chunks, {wraps} wraps, {prec}: {len(run.episodes)} episodes, worst error / "
          f"max(1, |ref|) {worst:.3e} (bound {TOL[prec]:.0e})")


# ------------------------------------------------------------------------------------------ 4. / 5. install
def _scenario_to(run, book, t_end, skip=()):
    """single steps with the scenario's restarts up to (not including) batch step t_end; samples in `skip` are not restarted"""
    while run.t < t_end:
        flags = [f and b not in skip for b, f in enumerate(_restarts(run.t))]
        run.restart(flags)
        if run.t > 0:
            book.restart(flags)
        book.advance(1)
        run.run(1)


def _install_case(prec, ring, tB, T, n_after, label):
    """Stream 2's episode that began at step 5 (policy A ran it for T steps) joins batch B as sample 0 right before batch step tB, and goes on there
    for n_after steps. The twin never hears of it."""
    src, i0 = 2, 5
    polA, polB, twin = (_policy(prec, decode_ring=ring) for _ in range(3))
    ref_pol = _policy(prec)
    _, _, otok, omask, atok = _data(polA)
    A, bookA = Run(polA, otok, omask, atok), EpisodeBook(B, Q, NPOS, ring)
    _scenario_to(A, bookA, i0 + T)
    assert (src, i0) in A.episodes and not any((src, t) in A.episodes for t in range(i0 + 1, i0 + T))
    ptok, pmask = A.episodes[(src, i0)]
    ref = _reference(ref_pol, otok, omask, atok, src, i0, i0 + T + n_after, ptok, pmask)
    runs = []
    for pol, inst in ((polB, True), (twin, False)):
        run, book = Run(pol, otok, omask, atok), EpisodeBook(B, Q, NPOS, ring)
        _scenario_to(run, book, tB)
        flags = [f and b != 0 for b, f in enumerate(_restarts(tB))]   # the others' restarts of batch step tB, in both runs
        run.restart(flags)
        book.restart(flags)
        if inst:
            assert pol.history_room() == book.history_room() >= T
            rows = book.history_rows(T)
            pred = run.install([0], [(src, i0 + T)], T, [(ptok, pmask)])
            book.install([True, False, False], T)
            assert pred.shape == (T, 1, otok.shape[-1])
            worst = max(_err(pred[j, 0], ref[j]) for j in range(T))
            assert worst <= TOL[prec], worst
            worstA = max(_err(pred[j, 0], A.outs[i0 + j][src]) for j in range(T))   # what policy A itself predicted for these steps
            assert worstA <= 2 * TOL[prec], worstA
            assert pol.steps_left().tolist() == book.steps_left()
            # ... which is the entry of a sample plainly restarted T batch steps earlier (and not since)
            probe = Run(_policy(prec, decode_ring=ring), otok, omask, atok)   # a twin run of the policy itself
            while probe.t < tB:
                t = probe.t
                probe.restart([t > 0 and (t == tB - T if (b == 0 and t >= tB - T) else _restarts(t)[b]) for b in range(B)])
                probe.run(1)
            assert pol.steps_left()[0].item() == probe.pol.steps_left()[0].item()
        for _ in range(n_after):
            if run.t > tB:
                f = [f and b != 0 for b, f in enumerate(_restarts(run.t))]
                run.restart(f)
                book.restart(f)
            book.advance(1)
            run.run(1)
            assert pol.steps_left().tolist() == book.steps_left()
        runs.append((run, book))
    (rb, bookB), (rt, _) = runs
    for j in range(n_after):
        e = _err(rb.outs[tB + j][0], ref[T + j])
        worst = max(worst, e)
        assert e <= TOL[prec], (j, e)
        for b in (1, 2):   # untouched, bit for bit
            assert torch.equal(rb.outs[tB + j][b], rt.outs[tB + j][b]), (j, b)
    print(f"[prefill] install {label}, {prec} ring {ring}: T {T} at batch step {tB}, cache rows {rows}, {n_after} further steps; worst error / "
          f"max(1, |ref|) {worst:.3e} (bound {TOL[prec]:.0e}); predictions vs the source policy's own {worstA:.3e}")
    return rows


@pytest.mark.parametrize("ring", [1, 0])
@pytest.mark.parametrize("prec", PRECS)
def test_an_installed_episode_continues_as_if_it_had_run_here(prec, ring):
    """Ring: batch B is past its first wrap (step 9); the history takes the slots of batch steps 13 .. 15 (rows 20 .. 34) and the episode goes on over
    the wrap of step 18. Linear: installed at batch step 4 >= T, to the end of the cache."""
    if ring:
        rows = _install_case(prec, 1, 16, 3, 5, "behind the first wrap")
        assert rows[0] == 21 and max(rows) == 34
    else:
        _install_case(prec, 0, 4, 3, 5, "linear")


@pytest.mark.parametrize("prec", PRECS)
def test_a_history_across_the_wrap(prec):
    """The slots of batch steps 16, 17 (rows 35 .. 44) and 18 (rows 0 .. 4 behind the skipped tail 45 .. 47)."""
    rows = _install_case(prec, 1, 19, 3, 4, "across the wrap")
    assert max(rows) == 44 and min(rows) == 0 and rows[-1] < rows[0]


def test_two_samples_in_one_call_equal_two_calls():
    """T = 7: 34 history rows, so that one sample alone is already beyond the 32 rows of gemm_skinny_kernel, whose summation order differs from the
    tile kernels' (the header's option gemm_skinny): every GEMM of both routes then runs on tile kernels, which agree bit for bit at every row count."""
    T, tB = 7, 17
    outs = []
    for together in (True, False):
        pol = _policy("bf16", decode_ring=1)
        _, _, otok, omask, atok = _data(pol)
        run, book = Run(pol, otok, omask, atok), EpisodeBook(B, Q, NPOS, True)
        _scenario_to(run, book, tB)
        assert pol.history_room() == book.history_room() >= T
        pr = [(run.pt[:, b:b + 1].clone(), run.pm[b:b + 1].clone()) for b in (1, 2)]
        if together:
            pred = run.install([0, 2], [(1, 20), (2, 30)], T, pr)
        else:
            pred = torch.cat([run.install([0], [(1, 20)], T, pr[:1]), run.install([2], [(2, 30)], T, pr[1:])], dim=1)
        book.install([True, False, True], T)
        assert pol.steps_left().tolist() == book.steps_left() and min(book.steps_left()) >= 2
        run.run(1)
        run.run(1)
        outs.append((pred, run.outs[tB], run.outs[tB + 1]))
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 6. refusals
def _twins(ring, t_end, skip=()):
    out = []
    for _ in range(2):
        pol = _policy("fp32", decode_ring=ring)
        _, _, otok, omask, atok = _data(pol, 12)
        run, book = Run(pol, otok, omask, atok), EpisodeBook(B, Q, NPOS, ring)
        _scenario_to(run, book, t_end, skip)
        out.append((run, book))
    return out


def _same_next_step(a, b):
    a.run(1)
    b.run(1)
    assert torch.equal(a.outs[a.t - 1], b.outs[b.t - 1])


def test_refused_history_changes_nothing():
    (run, book), (twin, _) = _twins(1, 11)
    room = run.pol.history_room()
    assert room == book.history_room() < run.t
    left = run.pol.steps_left().tolist()
    with pytest.raises(IndexError, match=f"room for {room}"):
        run.install([1], [(1, 11)], room + 1, [(run.pt[:, 1:2].clone(), run.pm[1:2].clone())])
    run.feed[1] = (1, 0)
    assert run.pol.steps_left().tolist() == left and run.pol.history_room() == room
    _same_next_step(run, twin)


def test_refused_chunk_in_the_linear_cache_changes_nothing():
    (run, _), (twin, _) = _twins(0, 7)
    with pytest.raises(IndexError, match="room for 2 more steps"):
        run.run(3)
    assert run.pol.steps_left().tolist() == [2] * B
    _same_next_step(run, twin)


def test_a_call_of_more_than_512_rows_is_refused_and_changes_nothing():
    """The position scan of the incremental embedding holds 512 rows, so every incremental call is bounded by its T slots of Q + 1 rows,
    T (Q + 1) <= 512: a single step (Q = 512: a slot of 513; at batch step 0, whose slot lacks the action row, the same T and Q are refused
    although the call has 512 rows) like a chunk (T = 2, Q = 256: 514). The refusal names the call and comes before anything changes: step 0
    would otherwise end the running episode batch."""
    (run, _), (twin, _) = _twins(0, 7)
    left = run.pol.steps_left().tolist()
    E = run.otok.shape[-1]
    wide, wmask = torch.zeros(B, 512, E, device=DEV), torch.ones(B, 512, dtype=torch.bool, device=DEV)
    for step, act in ((0, None), (run.t, run.atok[run.t - 1])):
        with pytest.raises(RuntimeError, match="vima_decode_step: .*at most 512 rows"):
            run.pol.forward_step(wide, wmask, act, run.pt, run.pm, step)
    with pytest.raises(RuntimeError, match="vima_decode_chunk: .*at most 512 rows"):
        run.pol.forward_steps(torch.stack([wide[:, :256]] * 2), torch.stack([wmask[:, :256]] * 2), run.atok[run.t - 1:run.t + 1], run.pt, run.pm, run.t)
    assert run.pol.steps_left().tolist() == left
    _same_next_step(run, twin)


def test_refused_chunk_in_the_ring_changes_nothing():
    """Sample 2 is never restarted: at batch step 8 it has age 39 and one step left (it would write rows 39 .. 43); a 2-step chunk does not fit in
    front of row 48, would skip 9 rows and write 10."""
    (run, book), (twin, _) = _twins(1, 8, skip=(2,))
    assert book.steps_left()[2] == 1 == run.pol.steps_left()[2].item()
    with pytest.raises(IndexError, match="sample 2"):
        run.run(2)
    assert run.pol.steps_left().tolist() == book.steps_left()
    _same_next_step(run, twin)


def test_decoder_only_policies_point_to_seq():
    pol = VIMAGPTPolicy(embed_dim=64, n_layer=1, n_head=2, n_positions=64, precision="fp32", device=DEV)
    x = torch.zeros(2, 1, 1, 64, device=DEV)
    with pytest.raises(NotImplementedError, match="seq_"):
        pol.forward_steps(x, None, None, None, 0)
    with pytest.raises(NotImplementedError, match="seq_"):
        pol.restart_samples([True], None, None, history=(x, None))


@pytest.mark.parametrize("ring", [1, 0])
def test_no_history_is_the_plain_restart(ring):
    runs = _twins(ring, 4) + _twins(ring, 4)[:1]
    E = runs[0][0].otok.shape[-1]
    empty = (torch.empty(0, 1, Q, E, device=DEV), torch.empty(0, 1, Q, dtype=torch.bool, device=DEV), None)
    for (run, _), hist in zip(runs, ("plain", None, empty)):
        flags = torch.tensor([False, True, False])
        if hist == "plain":
            got = run.pol.restart_samples(flags, run.pt, run.pm)
        else:
            got = run.pol.restart_samples(flags, run.pt, run.pm, history=hist)
        assert got is None or got.shape == (0, 1, E)
        run.run(1)
        run.run(1)
    for run, _ in runs[1:]:
        for t in (4, 5):
            assert torch.equal(run.outs[t], runs[0][0].outs[t])


# ------------------------------------------------------------------------------------------ 7. graphs
def test_chunk_and_install_inside_a_graphed_ring_rollout():
    """The 40 steps of the scenario; replays begin in the fourth lap (step 27: the third lap captured the graphs of the settled ring). The 2-step
    chunk of steps 28, 29 (rows 5 .. 14, the rows of two steps, so the write pointers of the later steps stay those of the captured graphs) and,
    right before step 34, stream 1's last 3 steps installed as sample 0, which then runs to the last step its age allows (39)."""
    results = []
    for graphs in (0, 1):
        pol = _policy("bf16", decode_ring=1, graphs=graphs)
        _, _, otok, omask, atok = _data(pol)
        run, book = Run(pol, otok, omask, atok, static=True), EpisodeBook(B, Q, NPOS, True)
        stats = {}
        _scenario_to(run, book, 28)
        run.restart(_restarts(28))
        book.restart(_restarts(28))
        stats["chunk"] = pol.graph_stats()
        assert not any(_restarts(29)) and book.plan(2)[0] == 5
        run.run(2)
        book.advance(2)
        _scenario_to(run, book, 34)
        stats["install"] = pol.graph_stats()
        run.install([0], [(1, 34)], 3, [(run.pt[:, 1:2].clone(), run.pm[1:2].clone())])
        book.install([True, False, False], 3)
        _scenario_to(run, book, STEPS, skip=(0,))
        stats["end"] = pol.graph_stats()
        assert pol.steps_left().tolist() == book.steps_left() and book.steps_left()[0] == 0
        results.append((run, stats))
    (eager, _), (graphed, stats) = results
    for t in range(STEPS):
        assert torch.equal(eager.outs[t], graphed.outs[t]), t
    print(f"[prefill] graphs (replays, captures): before the chunk {stats['chunk']}, before the install {stats['install']}, at the end {stats['end']}")
    assert stats["chunk"][0] > 0 and stats["install"][0] > stats["chunk"][0] and stats["end"][0] > stats["install"][0]


# ------------------------------------------------------------------------------------------ 8. launch counts
def _launches(pol, fn):
    pol.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    n = sum(v["launches"] for v in pol.prof_read().values())
    pol.prof_enable(False)
    return n


def test_launch_counts():
    """Prompts of 6 segments x 6 words (more than 32 tokens: the restart itself is then batched, tests/test_rollout_gpu.py): an install takes the
    same launches for 1 and for 2 samples; a chunk of 4 steps takes fewer launches than 4 steps (those of one step)."""
    long_prompt = syn.make_prompt(B, n_segments=6, words_per_segment=6, q_per_view=QV, seed=77)
    install, plain = {}, {}
    for who in ([0], [0, 2]):
        pol = _policy("bf16", decode_ring=1)
        _, _, otok, omask, atok = _data(pol, 8)
        pt, pm = pol.forward_prompt_assembly(syn.to_device(long_prompt, DEV))
        assert pt.shape[0] > 32
        for t in range(5):
            pol.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t > 0 else None, pt, pm, step=t)
        flags = torch.tensor([b in who for b in range(B)])
        hist = (otok[:3, who].contiguous(), omask[:3, who].contiguous(), atok[:2, who].contiguous())
        install[len(who)] = _launches(pol, lambda: pol.restart_samples(flags, pt, pm, history=hist))
        plain[len(who)] = _launches(pol, lambda: pol.restart_samples(flags, pt, pm))
    pol = _policy("bf16", decode_ring=1)
    _, _, otok, omask, atok = _data(pol)
    run = Run(pol, otok, omask, atok)
    run.run(1)
    chunk = _launches(pol, lambda: run.run(4))                      # steps 1 .. 4
    singles = [_launches(pol, lambda: run.run(1)) for _ in range(4)]  # steps 5 .. 8
    one, steps = singles[0], sum(singles)
    print(f"[prefill] launches: install of 1 sample {install[1]}, of 2 samples {install[2]} (the plain restart: {plain[1]}, {plain[2]}); one step {one}, "
          f"a chunk of 4 steps {chunk}, 4 single steps {steps}")
    assert install[1] == install[2] and plain[1] == plain[2] == 2 + 2 * CFG.xf_n_layers
    assert chunk < steps == 4 * one and chunk < 2 * one   # one pass: the launches of one step, give or take a GEMM form that splits at another row count
