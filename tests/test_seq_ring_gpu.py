"""Continuous batched rollouts of the decoder-only baselines on the MI355X: option "seq_ring" of `seq_prefill` / `seq_step` / `seq_restart`
(vima_seq_prefill / vima_seq_decode_step / vima_seq_decode_restart) and `steps_left`.

The scenario (tests/seq_ring_reference.py, whose properties tests/test_seq_ring_reference.py holds on the CPU): B = 3, 26 env steps, sample b
restarted with a new prompt at every t > 0 with t % (2 + b) == 0; Gato Q = 16 on a ring of R = 90 rows (5 wraps, tails 6, 5, 5, 5, 5, rows that
are never written), GPT Q = 1 on R = 9 (6 wraps). Every prompt comes from the ragged layout of BASELINE_CASES["baseline_gato"] with its own seed:
one Lp, a different number of valid tokens per sample. n_positions = Lp + 1 + R. References: `forward` on the full history of one
(sample, episode) alone, on a second policy with the ring off; the CPU oracle for one episode of a late lap."""
import functools
import math

import pytest
import torch

from oracle.baseline_oracle import build_baseline_oracle
from oracle.cases import BASELINE_CASES, run_baseline
from tests import seq_ring_reference as rr
from tests.gpu_common import bare_policy, bf, max_abs, max_rel, ptr
from vima_amd import _lib
from vima_amd.baselines import build_baseline
from vima_amd.policy import build_prompt_index
from vima_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X3 = "bf16x3"
B = rr.B
_LAYOUT = BASELINE_CASES["baseline_gato"]["layout"]


def _lp(kind):
    return build_prompt_index(_LAYOUT, rr.Q[kind])[1]


@functools.lru_cache(maxsize=None)
def _model(kind, E, heads, layers):
    """(cfg, state dict): Lp is computed BEFORE the policy is built, n_positions sizes its position table"""
    cfg = syn.BaselineConfig(kind, E, layers, heads, vocab_size=16, n_positions=_lp(kind) + 1 + rr.RING[kind])
    return cfg, syn.make_baseline_state_dict(cfg, 4100 + E + heads, head_gain=0.5)


def _policy(cfg, sd, prec, **opts):
    pol = build_baseline(cfg, precision=prec, device=DEV)
    pol.load_state_dict(sd, strict=True)
    for k, v in opts.items():
        pol.set_option(k, v)
    return pol


def _raw_prompt(e):
    """the raw prompts of every sample's episode number e"""
    return syn.make_rgb_prompt(B, layout=_LAYOUT, seed=700 + e)


def _cut_prompt(prompts, b):
    layout, words, img = prompts
    w0 = sum(t == 0 for p in layout[:b] for t in p)
    i0 = sum(t == 1 for p in layout[:b] for t in p)
    nw, ni = sum(t == 0 for t in layout[b]), sum(t == 1 for t in layout[b])
    return [layout[b]], words[w0:w0 + nw], syn.MapDict(rgb=syn.MapDict({v: img["rgb"][v][i0:i0 + ni] for v in syn.VIEWS}))


def _cut(obs, actions, t0, t1, b):   # as tests/test_seq_step_gpu.py
    o = syn.MapDict(rgb=syn.MapDict({v: obs["rgb"][v][t0:t1, b:b + 1] for v in syn.VIEWS}), ee=obs["ee"][t0:t1, b:b + 1])
    return o, ({k: v[t0:t1 - 1, b:b + 1] for k, v in actions.items()} if t1 - t0 > 1 else None)


def _data(pol, steps):
    obs, acts = syn.make_rgb_obs(steps, B, seed=811), syn.make_actions(steps, B, seed=911)
    with torch.no_grad():
        otok = pol.forward_obs_token(syn.to_device(obs, DEV))       # [steps, B, Q, E] (gato) / [steps, B, E] (gpt)
        atok = pol.forward_action_token(syn.to_device(acts, DEV))   # [steps, B, E]: the action of step t is fed at step t + 1
    return obs, acts, otok, atok


def _rollout(pol, otok, atok, steps, never=(), static=False, on_step=None):
    """`steps` env steps of the batch with the staggered restarts. Returns the outputs [steps][B, E], the episodes {(b, first step): (prompt
    tokens [Lp, 1, E], mask [1, Lp], episode number)} and the current batch prompt (tokens, mask)."""
    ptoks = {}

    def prompt(e):
        if e not in ptoks:
            with torch.no_grad():
                t, m = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(e), DEV))
            ptoks[e] = (t.contiguous().clone(), m.clone())
        return ptoks[e]

    number = [0] * B
    pt, pm = (x.clone() for x in prompt(0))
    episodes = {(b, 0): (pt[:, b:b + 1].clone(), pm[b:b + 1].clone(), 0) for b in range(B)}
    for t in range(steps):   # every episode's prompt up front: the stepping loop below allocates nothing but seq_step's output
        for b in range(B):
            if rr.restarts(t, never)[b]:
                number[b] += 1
                nt, nm = prompt(number[b])
                episodes[(b, t)] = (nt[:, b:b + 1].clone(), nm[b:b + 1].clone(), number[b])
    if static:
        so, sa = torch.empty_like(otok[0]), torch.empty_like(atok[0])
    outs = torch.empty(steps, B, atok.shape[-1], device=DEV)
    pol.seq_prefill(pt, pm)
    for t in range(steps):
        flags = rr.restarts(t, never)
        if any(flags):
            for b in range(B):
                if flags[b]:
                    pt[:, b], pm[b] = episodes[(b, t)][0][:, 0], episodes[(b, t)][1][0]
            pol.seq_restart(flags, pt, pm)
        if on_step:
            on_step(t)
        prev = atok[t - 1] if t > 0 else None
        if static:
            so.copy_(otok[t])
            if t > 0:
                sa.copy_(prev)
            out = pol.seq_step(so, sa if t > 0 else None)
        else:
            out = pol.seq_step(otok[t].contiguous(), prev)
        outs[t].copy_(out)
        del out
    torch.cuda.synchronize()
    return list(outs), episodes, (pt, pm)


def _alone(ref_pol, episodes, key, t1, otok, atok):
    """`forward` of the ring-off policy on the full history of one (sample, episode) alone -> [t1 - t0, E]"""
    b, t0 = key
    ptok, pmask, _ = episodes[key]
    act = atok[t0:t1 - 1, b:b + 1].contiguous() if t1 - t0 > 1 else None
    return ref_pol.forward(otok[t0:t1, b:b + 1].contiguous(), act, ptok, pmask)[:, 0]


def _close(got, ref, prec, tag):
    """The project's gates for two routes of the same sample: fp32 max abs < 2e-4 (test_seq_step_matches_forward_fp32), bf16 max_rel < 4e-2
    (tests/test_baselines_gpu.py::_compare)."""
    assert torch.isfinite(got).all(), tag
    a, r = max_abs(got, ref), max_rel(got, ref)
    if prec == "fp32":
        assert a < 2e-4, (tag, a)
    else:
        assert r < 4e-2, (tag, r)
    return a, r


def _check_against_every_episode_alone(ref_pol, outs, episodes, otok, atok, prec, steps, never=()):
    worst_a = worst_r = 0.0
    for key, t1 in rr.episode_starts(steps, never).items():
        full = _alone(ref_pol, episodes, key, t1, otok, atok)
        for t in range(key[1], t1):
            a, r = _close(outs[t][key[0]], full[t - key[1]], prec, (key, t))
            worst_a, worst_r = max(worst_a, a), max(worst_r, r)
    return worst_a, worst_r


def _gate_oracle(got, ref, tag):   # `_gate` of tests/test_seq_step_gpu.py, fp32
    got, ref = got.cpu(), ref.cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape), tuple(ref.shape))
    a, r = max_abs(got, ref), max_rel(got, ref)
    print(f"[{tag}] fp32: max_abs {a:.3e} max_rel {r:.3e} (max|ref| {ref.abs().max().item():.3g})")
    assert a < 1e-3 * max(1.0, ref.abs().max().item()), (tag, a)
    assert r < 2e-4, (tag, r)


# ---- 1. many laps / 2. other kernel routes -------------------------------------------------------------------------------------------
def _run_scenario(kind, E, heads, layers, prec, steps, oracle):
    cfg, sd = _model(kind, E, heads, layers)
    Lp = _lp(kind)
    sched, log = rr.run_schedule(kind, Lp, steps)          # legal throughout (tests/test_seq_ring_reference.py)
    pol = _policy(cfg, sd, prec, seq_ring=1)
    ref_pol = _policy(cfg, sd, prec, seq_ring=0)
    obs, acts, otok, atok = _data(pol, steps)
    outs, episodes, (pt, _) = _rollout(pol, otok, atok, steps)
    assert pt.shape[0] == Lp and cfg.n_positions == Lp + 1 + rr.RING[kind]
    assert len(episodes) == len(rr.episode_starts(steps))
    assert pol.steps_left().tolist() == sched.steps_left()
    # the two sides of the attention launcher's choice by key count
    if kind == "gato":
        assert max(s["hw"] for s in log) > 64
    else:
        assert cfg.n_positions < 64
    wa, wr = _check_against_every_episode_alone(ref_pol, outs, episodes, otok, atok, prec, steps)
    laps = rr.lap_of_step(log)
    print(f"[seq_ring] {kind} E {E} heads {heads} {prec}: {len(episodes)} episodes over {steps} steps and {max(laps)} laps, worst max_abs {wa:.3e} "
          f"max_rel {wr:.3e} against every episode alone")
    if oracle:
        # the longest episode that lies wholly in lap >= 3, against the CPU oracle on its raw inputs
        ends = rr.episode_starts(steps)
        (b, t0), t1 = max(((k, v) for k, v in ends.items() if laps[k[1]] >= 3), key=lambda kv: (kv[1] - kv[0][1], -kv[0][1]))
        assert t1 - t0 >= 2 and laps[t0] >= 3
        orc = build_baseline_oracle(cfg, sd)
        o, a = _cut(obs, acts, t0, t1, b)
        want = run_baseline(orc, _cut_prompt(_raw_prompt(episodes[(b, t0)][2]), b), o, a)["predicted"][:, 0]
        _gate_oracle(torch.stack([outs[t][b] for t in range(t0, t1)]), want, f"seq_ring {kind} sample {b} steps {t0}..{t1 - 1} (lap {laps[t0]}) vs oracle")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_rollout_over_many_laps_matches_every_episode_alone(kind, prec):
    """No bit identity is asked for: the ring reads a sample's keys in a different order than the linear cache."""
    _run_scenario(kind, 256, 8, 2, prec, rr.STEPS, oracle=prec == "fp32")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,E,heads", [("gato", 768, 12),    # head dim 64
                                          ("gpt", 320, 20)])    # head dim 16: the generic attention kernel; E % 128 != 0: the two-launch c_attn append
def test_rollout_on_the_other_kernel_routes(kind, E, heads, prec):
    log = rr.run_schedule(kind, _lp(kind), 12)[1]
    assert sum(s["wrap"] for s in log) >= 2
    _run_scenario(kind, E, heads, 1, prec, 12, oracle=False)


# ---- 3. bounds -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_a_sample_that_is_never_restarted_stops_the_ring_until_it_is(kind):
    cfg, sd = _model(kind, 256, 8, 2)
    pol = _policy(cfg, sd, "fp32", seq_ring=1)
    ref_pol = _policy(cfg, sd, "fp32", seq_ring=0)
    _, _, otok, atok = _data(pol, 6)
    with pytest.raises(rr.Refused) as ei:
        rr.run_schedule(kind, _lp(kind), 6, never=(2,))
    model = ei.value.ring                                          # the restatement as the fifth successful step left it
    assert ei.value.step == 5 and ei.value.sample == 2
    sim = rr.Ring(_lp(kind), cfg.n_positions, rr.Q[kind], B)
    left = {}

    def on_step(t):                                                 # after the restarts of step t, before its seq_step
        sim.restart(rr.restarts(t, (2,)))
        left[t] = (pol.steps_left().tolist(), sim.steps_left())
        sim.step()

    outs, episodes, (pt, pm) = _rollout(pol, otok, atok, 5, never=(2,), on_step=on_step)
    assert all(got == want for got, want in left.values()), left
    assert not any(rr.restarts(5, (2,)))
    sl = pol.steps_left()
    assert sl.dtype == torch.int32 and sl.device.type == "cpu" and sl.tolist() == model.steps_left() and sl[2].item() == 0 and min(sl[:2].tolist()) > 0, sl
    for _ in range(2):   # a failing call leaves the state as it was
        with pytest.raises(IndexError, match="sample 2"):
            pol.seq_step(otok[5].contiguous(), atok[4])
        assert pol.steps_left().tolist() == sl.tolist()
    with torch.no_grad():
        nt, nm = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(9), DEV))
    pt[:, 2], pm[2] = nt[:, 2], nm[2]
    pol.seq_restart([False, False, True], pt, pm)
    model.restart([False, False, True])
    assert pol.steps_left().tolist() == model.steps_left() and pol.steps_left()[2].item() > 0
    out = pol.seq_step(otok[5].contiguous(), atok[4])
    model.step()
    assert pol.steps_left().tolist() == model.steps_left()
    fresh = ref_pol.forward(otok[5:6, 2:3].contiguous(), None, nt[:, 2:3].contiguous(), nm[2:3])[0, 0]     # sample 2: a fresh episode
    _close(out[2], fresh, "fp32", "restarted sample 2")
    cont = _alone(ref_pol, episodes, (1, 3), 6, otok, atok)[2]                                              # sample 1: its episode of steps 3 .. 5
    _close(out[1], cont, "fp32", "continuing sample 1")


# ---- 4. ring off is untouched --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_without_the_ring_the_batch_still_ends_at_the_same_step(kind):
    cfg, sd = _model(kind, 256, 8, 2)
    Lp, Q, N = _lp(kind), rr.Q[kind], cfg.n_positions
    pol = _policy(cfg, sd, "fp32", seq_ring=0)
    _, _, otok, atok = _data(pol, 8)
    with torch.no_grad():
        pt, pm = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(0), DEV))
    pol.seq_prefill(pt, pm)
    used, t = Lp + 1, 0
    assert pol.steps_left().tolist() == [(N - used + 1) // (Q + 1)] * B    # the formula of tests/test_seq_step_gpu.py
    while used + Q + (1 if t else 0) <= N:
        pol.seq_step(otok[t].contiguous(), atok[t - 1] if t else None)
        used += Q + (1 if t else 0)
        t += 1
        if t in (2, 3):
            pol.seq_restart([t == 2, False, True], pt, pm)                 # restarts give no rows back
        assert pol.steps_left().tolist() == [(N - used) // (Q + 1)] * B
    assert t == 1 + (rr.RING[kind] - Q) // (Q + 1) == 5 and pol.steps_left().tolist() == [0] * B
    with pytest.raises(IndexError, match="n_positions"):
        pol.seq_step(otok[t].contiguous(), atok[t - 1])
    # setting the option ends a running episode, either way
    for first, second in ((0, 1), (1, 0)):
        pol.set_option("seq_ring", first)
        pol.seq_prefill(pt, pm)
        pol.seq_step(otok[0].contiguous())
        pol.set_option("seq_ring", second)
        with pytest.raises(_lib.VimaError, match="does not continue the episode state"):
            pol.seq_step(otok[1].contiguous(), atok[0])
    # decode_ring stays VIMAPolicy's ring
    pol.set_option("decode_ring", 1)
    for call in (lambda: pol.seq_prefill(pt, pm), lambda: pol.seq_step(otok[1].contiguous(), atok[0]), lambda: pol.seq_restart([True, False, False], pt, pm)):
        with pytest.raises(_lib.VimaError, match="decode_ring"):
            call()
    torch.cuda.synchronize()


# ---- 5. graph replay -----------------------------------------------------------------------------------------------------------------
def test_ring_rollout_under_graph_replay_is_exact_and_bounded():
    """A captured step bakes in (row, hw, action slot). In this schedule hw moves for the last time at the end of lap 2 (step 9: the first lap is one
    row shorter, step 0 has no action slot), so steps 10 .. 13 of lap 3 carry keys that laps 1 and 2 did not have and are captured then; from lap 4
    (step 15) on everything replays. The restatement predicts the number of captures: every key with an action slot when first seen, except the
    one eager step that warms the family."""
    cfg, sd = _model("gato", 256, 8, 2)
    log = rr.run_schedule("gato", _lp("gato"))[1]
    laps, keys = rr.lap_of_step(log), rr.graph_keys(log)
    assert [laps.index(n) for n in (3, 4, 5)] == [10, 15, 20]

    def predicted(upto):
        return max(0, len({k for k in keys[:upto] if k[2]}) - 1)

    eager = _policy(cfg, sd, "bf16", seq_ring=1)
    _, _, otok, atok = _data(eager, rr.STEPS)
    want = _rollout(eager, otok, atok, rr.STEPS, static=True)[0]
    pol = _policy(cfg, sd, "bf16", seq_ring=1, graphs=1)
    stats = {}
    got = _rollout(pol, otok, atok, rr.STEPS, static=True, on_step=lambda t: stats.__setitem__(t, pol.graph_stats()))[0]
    for t, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), t
    replays, captures = pol.graph_stats()
    print(f"[seq_ring] graphs: {captures} captures, {replays} replays over {rr.STEPS} steps; captures at the start of laps 3, 4, 5: "
          f"{[stats[t][1] for t in (10, 15, 20)]}, predicted {[predicted(t) for t in (10, 15, 20)]}")
    assert captures > 0 and replays > 0
    assert stats[15][1] == stats[20][1] == captures, "from lap 4 on every step must run on the graphs of the laps before it"
    assert [stats[t][1] for t in (10, 15)] == [predicted(10), predicted(15)] and captures == predicted(rr.STEPS)
    assert stats[15][1] - stats[10][1] == 4 and replays == rr.STEPS - 2 - captures


# ---- 6. restart launches -------------------------------------------------------------------------------------------------------------
def test_restart_launches_do_not_depend_on_the_count_or_the_ring():
    cfg, sd = _model("gato", 256, 8, 2)
    launches = {}
    for ring in (1, 0):
        pol = _policy(cfg, sd, "bf16", seq_ring=ring)
        _, _, otok, atok = _data(pol, 2)
        with torch.no_grad():
            pt, pm = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(0), DEV))
            nt, nm = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(1), DEV))
        for flagged in ([1], [1, 2]):
            pol.seq_prefill(pt, pm)
            pol.seq_step(otok[0].contiguous())
            pol.seq_step(otok[1].contiguous(), atok[0])
            pol.prof_enable(True)
            pol.seq_restart([b in flagged for b in range(B)], nt, nm)
            torch.cuda.synchronize()
            launches[(ring, len(flagged))] = sum(v["launches"] for v in pol.prof_read().values())
            pol.prof_enable(False)
    print(f"[seq_ring] launches of one seq_restart (ring, flagged samples): {launches}")
    assert launches[(1, 1)] == launches[(1, 2)] == launches[(0, 1)] == launches[(0, 2)] > 0, launches


# ---- 7. the window rule at these shapes (passes without the feature: it pins the kernel path the feature stands on) -------------------
@pytest.mark.parametrize("prec,impl", [("fp32", 0), ("bf16", 0), ("bf16", 1), (X3, 1)])
@pytest.mark.parametrize("Lq,D", [(17, 32), (17, 64), (2, 16), (2, 32)])
@pytest.mark.parametrize("Lk,P0", [(40, 8), (150, 38)])
def test_window_rule_at_the_ring_shapes(prec, impl, Lq, D, Lk, P0):
    """A visible prefix below q_off, the step's rows [q_off, win_end), older laps in [win_end, Lk), random key masks with at least one whole
    older-lap block masked out per sample (a restarted sample's dead rows). Per element against fp64 (tests/seq_ring_reference.py); tolerances
    of tests/test_rollout_gpu.py::test_window_rule_in_every_attention_kernel for the same precision / impl pairs: fp32 1e-5 and bf16 1.5e-2 of
    max |ref| (bf16: on the bf16-rounded inputs), bf16x3 2e-5 absolute on inputs uniform in [-1, 1]. impl 1 at D = 16 is the generic kernel."""
    pol = bare_policy(prec)
    pol.set_option("attn4_min_lq", 64)
    Bq, H = 2, 4
    scale = 1.0 / math.sqrt(D)
    ring = Lk - P0
    for q_off in (P0, P0 + (ring - Lq) // 2):                    # the first ring row; mid-ring, with this lap's rows below and older ones above
        win_end = q_off + Lq
        assert P0 <= q_off and win_end < Lk
        g = torch.Generator().manual_seed(7000 + 100 * Lq + 10 * D + Lk + q_off)
        if prec == X3:
            q, k, v = (torch.rand(Bq, L, H, D, generator=g) * 2 - 1 for L in (Lq, Lk, Lk))
        else:
            q, k, v = (torch.randn(Bq, L, H, D, generator=g) for L in (Lq, Lk, Lk))
        kmask = torch.rand(Bq, Lk, generator=g) > 0.2
        kmask[:, 0] = True                                        # no sample has a fully masked row
        kmask[:, q_off] = True
        blk = min(Lq, Lk - win_end)
        kmask[0, Lk - blk:] = False                               # a whole block of an older lap: the last one ...
        kmask[1, win_end:win_end + blk] = False                   # ... and the one right behind the window
        kmask[1, P0:q_off] = False                                # sample 1 restarted at this lap's start: nothing else in the ring is its own
        assert bool(kmask.any(dim=1).all())
        out = torch.full((Bq, Lq, H, D), float("nan"), device=DEV)
        qd, kd, vd, md = q.to(DEV), k.to(DEV), v.to(DEV), kmask.to(DEV)
        _lib.check(pol._lib.vima_op_attention_window(pol._handle, ptr(qd), ptr(kd), ptr(vd), ptr(md), Bq, H, Lq, Lk, D, scale, impl, q_off, ptr(out),
                                                     pol._stream()))
        torch.cuda.synchronize()
        out = out.cpu()
        assert torch.isfinite(out).all()
        ref = rr.attn_window_f64(bf(q), bf(k), bf(v), kmask, scale, q_off) if prec == "bf16" else rr.attn_window_f64(q, k, v, kmask, scale, q_off)
        err = (out.double() - ref).abs()
        bound = 2e-5 if prec == X3 else (1.5e-2 if prec == "bf16" else 1e-5) * ref.abs().max().item()
        print(f"[seq_ring window] {prec} impl {impl} Lq {Lq} D {D} Lk {Lk} q_off {q_off}: max err vs fp64 {err.max().item():.2e} (bound {bound:.2e})")
        assert bool((err <= bound).all()), (q_off, err.max().item(), bound)
