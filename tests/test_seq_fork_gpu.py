"""Branch rollouts of the decoder-only baselines on the MI355X: `seq_fork` (vima_seq_decode_fork) on GPT and Gato, with option "seq_ring" and on
the linear cache.

The models, prompts and data are those of tests/test_seq_ring_gpu.py (B = 3, Gato Q = 16 on a ring of 90 rows, GPT Q = 1 on 9; sample b restarted
with a new prompt at every t > 0 with t % (2 + b) == 0; ragged prompts, so a destination's prefix differs from its source's before every fork).
Ring scenario, 14 steps (the ring wraps at steps 5 and 10 for Gato, 5, 9 and 13 for GPT): a fork behind the wrap in front of step 6, a
`seq_restart(history=)` of the forked slot in front of step 7, a fork of a just-restarted source in front of step 8, a fork to two destinations
behind the second wrap in front of step 11. The bookkeeping is followed with the brute-force restatement of tests/episode_fork_reference.py
(every step legal, steps_left equal at every step). Slot b is fed column b of the data; on the step right after a fork a destination is fed its
source's column and must return its source's bits. Every (slot, lineage) is compared with `forward` of the lineage's full history alone on a
ring-off policy, at the gates of tests/test_seq_ring_gpu.py."""
import ctypes

import pytest
import torch

from tests import episode_fork_reference as fref
from tests import seq_ring_reference as rr
from tests.test_seq_ring_gpu import _close, _data, _lp, _model, _policy, _raw_prompt
from vima_amd import _lib
from vima_amd.baselines import build_baseline
from vima_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = rr.B
RING_STEPS, LINEAR_STEPS = 14, 5
FORKS = {6: [2, 1, 2], 8: [0, 0, 2], 11: [1, 1, 1]}
INSTALLS = {7: (0, 3)}                 # slot 0, forked in front of step 6, re-joins with its lineage's 3 steps
LINEAR_FORKS = {2: [0, 0, 2], 3: [2, 1, 2]}
LINEAR_RESTARTS = {3: [False, False, True]}


class _Lineage:
    def __init__(self, slot, prompt, steps=(), own_from=0):
        self.slot, self.prompt, self.steps, self.own_from = slot, prompt, list(steps), own_from


def _rollout(pol, kind, otok, atok, ring):
    Lp, steps = _lp(kind), RING_STEPS if ring else LINEAR_STEPS
    bk = fref.Book(B, rr.Q[kind], Lp + 1, Lp + 1 + rr.RING[kind], ring)
    ptoks = {}

    def prompt(e):
        if e not in ptoks:
            with torch.no_grad():
                t, m = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(e), DEV))
            ptoks[e] = (t.contiguous().clone(), m.clone())
        return ptoks[e]

    number = [0] * B
    pt, pm = (x.clone() for x in prompt(0))
    live = [_Lineage(b, (pt[:, b:b + 1].clone(), pm[b:b + 1].clone())) for b in range(B)]
    done, seen = [], dict(two_ranges=0, age0=0, multi=0, installed=0)
    outs = torch.empty(steps, B, atok.shape[-1], device=DEV)
    pol.seq_prefill(pt, pm)
    for t in range(steps):
        flags = rr.restarts(t) if ring else LINEAR_RESTARTS.get(t, [False] * B)
        if any(flags):
            for b in range(B):
                if flags[b]:
                    number[b] += 1
                    nt, nm = prompt(number[b])
                    pt[:, b], pm[b] = nt[:, b], nm[b]
                    done.append(live[b])
                    live[b] = _Lineage(b, (nt[:, b:b + 1].clone(), nm[b:b + 1].clone()))
            pol.seq_restart(flags, pt, pm)
            bk.restart(flags)
        inst = INSTALLS.get(t) if ring else None
        if inst:   # a forked slot restarted with its own lineage as the history: the lineage stays
            b, T = inst
            ln = live[b]
            assert len(ln.steps) == T and ln.own_from > 0
            pt[:, b], pm[b] = ln.prompt[0][:, 0], ln.prompt[1][0]
            h_obs = torch.stack([otok[s, c] for s, c in ln.steps]).unsqueeze(1).contiguous()
            h_act = torch.stack([atok[s - 1, c] for s, c in ln.steps[1:]]).unsqueeze(1).contiguous()
            fl = [x == b for x in range(B)]
            assert T <= pol.seq_history_room() == bk.room()
            pol.seq_restart(fl, pt, pm, history=(h_obs, h_act))
            bk.restart(fl)
            bk.install(fl, T)
            seen["installed"] += 1
        cols, pairs = list(range(B)), []
        source = (FORKS if ring else LINEAR_FORKS).get(t)
        if source:
            srcs = {s for b, s in enumerate(source) if s != b}
            seen["two_ranges"] += any(len(fref.ranges_of(bk.live_rows(s))) == 2 for s in srcs)
            seen["age0"] += any(bk.age[s] == 0 for s in srcs)
            seen["multi"] += any(sum(1 for b, x in enumerate(source) if x == s and b != s) >= 2 for s in srcs)
            for b, s in enumerate(source):
                if s != b:
                    assert not (torch.equal(live[b].prompt[0], live[s].prompt[0]) and torch.equal(live[b].prompt[1], live[s].prompt[1])), (t, b, s)
            pol.seq_fork(source)
            bk.fork(source)
            left = pol.steps_left().tolist()
            for b, s in enumerate(source):
                assert left[b] == left[s]
                if s != b:
                    pairs.append((b, s))
                    done.append(live[b])
                    live[b] = _Lineage(b, live[s].prompt, live[s].steps, own_from=len(live[s].steps))
                    cols[b] = s
        assert pol.steps_left().tolist() == [bk.steps_left(b) for b in range(B)], t
        assert bk.step(1) is not None, f"step {t} of the scenario is refused"
        idx = torch.tensor(cols, device=DEV)
        out = pol.seq_step(otok[t].index_select(0, idx).contiguous(), atok[t - 1].index_select(0, idx).contiguous() if t > 0 else None)
        outs[t].copy_(out)
        for b, s in pairs:   # fed the source's inputs, the destination returns the source's output bit for bit
            assert torch.equal(out[b], out[s]), (t, b, s, (out[b] - out[s]).abs().max().item())
        for b in range(B):
            live[b].steps.append((t, cols[b]))
    torch.cuda.synchronize()
    return outs, done + live, seen


def _check_lineages(ref_pol, outs, lineages, otok, atok, prec):
    worst_a = worst_r = 0.0
    n = 0
    for ln in lineages:
        if ln.own_from >= len(ln.steps):
            continue
        obs = torch.stack([otok[s, c] for s, c in ln.steps]).unsqueeze(1).contiguous()
        act = torch.stack([atok[s - 1, c] for s, c in ln.steps[1:]]).unsqueeze(1).contiguous() if len(ln.steps) > 1 else None
        full = ref_pol.forward(obs, act, *ln.prompt)[:, 0]
        for i in range(ln.own_from, len(ln.steps)):
            t = ln.steps[i][0]
            a, r = _close(outs[t][ln.slot], full[i], prec, (ln.slot, ln.steps[0], t))
            worst_a, worst_r, n = max(worst_a, a), max(worst_r, r), n + 1
    return worst_a, worst_r, n


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("ring", [1, 0], ids=["seq_ring", "linear"])
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_seq_fork_matches_every_lineage_alone(kind, ring, prec):
    cfg, sd = _model(kind, 256, 8, 2)
    pol = _policy(cfg, sd, prec, seq_ring=ring)
    ref_pol = _policy(cfg, sd, prec, seq_ring=0)
    steps = RING_STEPS if ring else LINEAR_STEPS
    _, _, otok, atok = _data(pol, steps)
    outs, lineages, seen = _rollout(pol, kind, otok, atok, bool(ring))
    if ring:
        assert seen["age0"] >= 1 and seen["multi"] >= 1 and seen["installed"] == 1, seen
        assert seen["two_ranges"] >= (2 if kind == "gato" else 1), seen
    else:
        assert seen["age0"] >= 1 and pol.steps_left().tolist() == [0] * B
    wa, wr, n = _check_lineages(ref_pol, outs, lineages, otok, atok, prec)
    assert n == steps * B
    print(f"[seq_fork] {kind} {'ring' if ring else 'linear'} {prec}: {len(lineages)} lineages, {n} (slot, step) outputs, worst max_abs {wa:.3e} "
          f"max_rel {wr:.3e}; destinations equal their sources bit for bit after every fork")


def test_seq_fork_refusals():
    cfg, sd = _model("gato", 256, 8, 2)
    pol, twin = _policy(cfg, sd, "fp32", seq_ring=1), _policy(cfg, sd, "fp32", seq_ring=1)
    _, _, otok, atok = _data(pol, 3)
    with torch.no_grad():
        pt, pm = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(0), DEV))
    pt, pm = pt.contiguous(), pm.contiguous()
    with pytest.raises(_lib.VimaError, match="no running episode"):
        pol.seq_fork([0, 0, 2])
    for p in (pol, twin):
        p.seq_prefill(pt, pm)
        for t in range(2):
            p.seq_step(otok[t].contiguous(), atok[t - 1] if t else None)
    left = pol.steps_left().tolist()
    with pytest.raises(ValueError, match=r"source\[0\] = 1 is itself a destination"):
        pol.seq_fork([1, 2, 2])
    with pytest.raises(ValueError, match=r"source\[2\] = 3 is not a sample"):
        pol.seq_fork([0, 1, 3])
    with pytest.raises(_lib.VimaError, match="vima_seq_decode_fork"):
        _lib.check(pol._lib.vima_decode_fork(pol._handle, (ctypes.c_int32 * 3)(0, 0, 2), 3, pol._stream()))
    pol.seq_fork([0, 1, 2])
    assert pol.steps_left().tolist() == left
    assert torch.equal(pol.seq_step(otok[2].contiguous(), atok[1]), twin.seq_step(otok[2].contiguous(), atok[1]))
    fl = build_baseline(syn.BaselineConfig("flamingo", 256, 1, 8, xattn_n_heads=8), device=DEV)
    with pytest.raises(NotImplementedError, match="fork_samples"):
        fl.seq_fork([0, 0])
