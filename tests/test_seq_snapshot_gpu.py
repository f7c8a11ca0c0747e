"""Episode snapshots of the decoder-only baselines on the MI355X: `seq_snapshot` / `seq_restore` (vima_seq_decode_snapshot /
vima_seq_decode_restore) on GPT and Gato, with option "seq_ring" and on the linear cache.

The models, prompts and data are those of tests/test_seq_ring_gpu.py (B = 3, Gato Q = 16 on a ring of 90 rows, GPT Q = 1 on 9; sample b restarted
with a new prompt at every t > 0 with t % (2 + b) == 0; ragged prompts, so a slot's prefix differs from the snapshot's before every restore).
Ring scenario, 14 steps (the ring wraps at steps 5 and 10 for Gato, 5, 9 and 13 for GPT): a snapshot behind the wrap in front of step 6, restored
into two slots in front of step 7, into a slot right after its `seq_restart` in front of step 8, and behind the second wrap in front of step 11; a
second snapshot in front of step 11, restored in front of step 13. The bookkeeping is followed with the brute-force restatement of
tests/episode_snapshot_reference.py (every step legal, steps_left equal at every step). Slot b is fed column b of the data. Every (slot, lineage)
is compared with `forward` of the lineage's full history alone on a ring-off policy, at the gates of tests/test_seq_ring_gpu.py."""
import pytest
import torch

from tests import episode_snapshot_reference as sref
from tests import seq_ring_reference as rr
from tests.test_seq_fork_gpu import _check_lineages, _Lineage
from tests.test_seq_ring_gpu import _data, _lp, _model, _policy, _raw_prompt
from vima_amd import _lib
from vima_amd.baselines import build_baseline
from vima_amd.episodes import EpisodeSnapshot
from vima_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = rr.B
RING_STEPS, LINEAR_STEPS = 14, 5
SNAPSHOTS = {6: ("A", 2), 11: ("B", 1)}                 # in front of step t: name, sample
RESTORES = {7: ("A", [0, 1]), 8: ("A", [0]), 11: ("A", [2]), 13: ("B", [0])}
LINEAR_SNAPSHOTS = {2: ("L", 1)}
LINEAR_RESTORES = {3: ("L", [0, 2])}


def _rollout(pol, kind, otok, atok, ring):
    Lp, steps = _lp(kind), RING_STEPS if ring else LINEAR_STEPS
    bk = sref.SnapBook(B, rr.Q[kind], Lp + 1, Lp + 1 + rr.RING[kind], ring)
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
    done, held = [], {}
    seen = dict(two_ranges=0, straddle=0, two_slots=0, after_restart=0, later=0)
    outs = torch.empty(steps, B, atok.shape[-1], device=DEV)
    pol.seq_prefill(pt, pm)
    for t in range(steps):
        flags = rr.restarts(t) if ring else [False] * B
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
        snap = (SNAPSHOTS if ring else LINEAR_SNAPSHOTS).get(t)
        if snap:
            name, b = snap
            (s,) = pol.seq_snapshot([b])
            n, _ = bk.snapshot(b)
            assert s.steps == n == len(live[b].steps) and s.has_prompt and s.prompt_token is None
            seen["two_ranges"] += len(sref.ranges_of(bk.live_rows(b))) == 2
            held[name] = (s, live[b].prompt, list(live[b].steps), t)
        rest = (RESTORES if ring else LINEAR_RESTORES).get(t)
        if rest:
            name, slots = rest
            s, prm, hist, taken = held[name]
            for d in slots:
                assert not (torch.equal(live[d].prompt[0], prm[0]) and torch.equal(live[d].prompt[1], prm[1])), (t, d)
            assert s.steps <= pol.seq_history_room() == bk.room()
            pol.seq_restore(slots, [s if t % 2 else s.cpu()] * len(slots))        # every other restore goes through the host
            age, rows = bk.restore(slots, s.steps)
            seen["straddle"] += sref.straddles(rows)
            seen["two_slots"] += len(slots) == 2
            seen["after_restart"] += any(flags[d] for d in slots)
            seen["later"] += t > taken
            for d in slots:
                done.append(live[d])
                live[d] = _Lineage(d, prm, hist, own_from=len(hist))
        assert pol.steps_left().tolist() == [bk.steps_left(b) for b in range(B)], t
        assert bk.step(1) is not None, f"step {t} of the scenario is refused"
        outs[t].copy_(pol.seq_step(otok[t].contiguous(), atok[t - 1].contiguous() if t > 0 else None))
        for b in range(B):
            live[b].steps.append((t, b))
    torch.cuda.synchronize()
    return outs, done + live, seen


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("ring", [1, 0], ids=["seq_ring", "linear"])
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_seq_snapshots_match_every_lineage_alone(kind, ring, prec):
    cfg, sd = _model(kind, 256, 8, 2)
    pol = _policy(cfg, sd, prec, seq_ring=ring)
    ref_pol = _policy(cfg, sd, prec, seq_ring=0)
    steps = RING_STEPS if ring else LINEAR_STEPS
    _, _, otok, atok = _data(pol, steps)
    outs, lineages, seen = _rollout(pol, kind, otok, atok, bool(ring))
    if ring:
        assert seen["two_ranges"] >= 1 and seen["two_slots"] == 1 and seen["after_restart"] == 1 and seen["later"] == 4, seen
        assert seen["straddle"] >= (1 if kind == "gato" else 0), seen
    else:
        assert seen["two_slots"] == 1 and seen["later"] == 1 and pol.steps_left().tolist() == [0] * B
    wa, wr, n = _check_lineages(ref_pol, outs, lineages, otok, atok, prec)
    assert n == steps * B
    print(f"[seq_snapshot] {kind} {'ring' if ring else 'linear'} {prec}: {len(lineages)} lineages, {n} (slot, step) outputs, worst max_abs {wa:.3e} "
          f"max_rel {wr:.3e}; {seen}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,E,heads", [("gato", 768, 12),    # head dim 64
                                          ("gpt", 320, 20)])    # head dim 16; E % 128 != 0
def test_seq_snapshots_on_the_other_head_dims(kind, E, heads, prec):
    cfg, sd = _model(kind, E, heads, 1)
    pol = _policy(cfg, sd, prec, seq_ring=1)
    ref_pol = _policy(cfg, sd, prec, seq_ring=0)
    _, _, otok, atok = _data(pol, RING_STEPS)
    outs, lineages, seen = _rollout(pol, kind, otok, atok, True)
    wa, wr, n = _check_lineages(ref_pol, outs, lineages, otok, atok, prec)
    assert n == RING_STEPS * B
    print(f"[seq_snapshot] {kind} E {E} head dim {E // heads} ring {prec}: worst max_abs {wa:.3e} max_rel {wr:.3e}")


def test_seq_snapshot_same_moment_refusals_and_launch_counts():
    cfg, sd = _model("gato", 256, 8, 2)
    pol, twin = _policy(cfg, sd, "fp32", seq_ring=1), _policy(cfg, sd, "fp32", seq_ring=1)
    _, _, otok, atok = _data(pol, 5)
    with torch.no_grad():
        pt, pm = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(0), DEV))
    pt, pm = pt.contiguous(), pm.contiguous()
    with pytest.raises(_lib.VimaError, match="no running episode"):
        pol.seq_snapshot([0])
    for p in (pol, twin):
        p.seq_prefill(pt, pm)
        for t in range(2):
            p.seq_step(otok[t].contiguous(), atok[t - 1] if t else None)
    left = pol.steps_left().tolist()
    counts = {}
    for samples in ([1], [0, 1, 2]):
        pol.prof_enable(True)
        snaps = pol.seq_snapshot(samples)
        torch.cuda.synchronize()
        a = sum(v["launches"] for v in pol.prof_read().values())
        pol.prof_enable(False)
        pol.prof_enable(True)
        pol.seq_restore(samples, snaps)                                   # every sample into its own slot: the identity
        torch.cuda.synchronize()
        counts[len(samples)] = (a, sum(v["launches"] for v in pol.prof_read().values()))
        pol.prof_enable(False)
    print(f"[seq_snapshot] launches of one (snapshot, restore) call by pairs: {counts}")
    assert counts == {1: (2, 2), 3: (2, 2)}, counts
    s = snaps[1]
    assert s.steps == 2 and pol.steps_left().tolist() == left
    with pytest.raises(ValueError, match="listed twice"):
        pol.seq_restore([0, 0], [s, s])
    with pytest.raises(ValueError, match="Q = 3"):
        pol.seq_restore([0], [EpisodeSnapshot(s.payload, dict(s.info, Q=3))])
    with pytest.raises(ValueError, match="another policy kind"):
        pol.seq_restore([0], [EpisodeSnapshot(s.payload, dict(s.info, policy_kind=0))])
    ahead = twin.seq_step(otok[2].contiguous(), atok[1])                    # the twin is one step ahead: its snapshot holds 3 steps, the room here is 2
    (s3,) = twin.seq_snapshot([0])
    with pytest.raises(IndexError, match="holds 3 steps and does not fit: room for 2"):
        pol.seq_restore([0], [s3])
    with pytest.raises(_lib.VimaError, match="vima_seq_decode"):
        _lib.check(pol._lib.vima_decode_snapshot_size(pol._handle, (_lib.c_i32 * 1)(0), 1, 1, None))
    with pytest.raises(NotImplementedError, match="seq_snapshot"):
        pol.snapshot_samples([0], pt, pm)
    assert pol.steps_left().tolist() == left
    # after the identity restores and the refusals the next step equals the untouched twin's bit for bit; then slot 2 := the snapshot of slot 1
    assert torch.equal(pol.seq_step(otok[2].contiguous(), atok[1]), ahead)
    (s1,) = pol.seq_snapshot([1])
    pol.seq_restore([2], [s1])
    twin.seq_fork([0, 1, 1])
    idx = torch.tensor([0, 1, 1], device=DEV)
    got = pol.seq_step(otok[3].index_select(0, idx).contiguous(), atok[2].index_select(0, idx).contiguous())
    want = twin.seq_step(otok[3].index_select(0, idx).contiguous(), atok[2].index_select(0, idx).contiguous())
    assert torch.equal(got[2], got[1]) and torch.equal(got, want)          # restored at once: what seq_fork gives, to the bit
    fl = build_baseline(syn.BaselineConfig("flamingo", 256, 1, 8, xattn_n_heads=8), device=DEV)
    with pytest.raises(NotImplementedError, match="snapshot_samples"):
        fl.seq_snapshot([0])
