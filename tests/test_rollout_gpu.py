"""Continuous batched rollouts on the MI355X: the ring mode of the episode caches (option "decode_ring"), the windowed causal rule of
every attention kernel behind it (vima_op_attention_window), `VIMAPolicy.steps_left`, and the batched `restart_samples`.

The rollout scenario (model 4M, n_positions 48, B = 3, Q = 4 -> 5 ring rows per step, 4 at step 0): the write pointer runs 4, 9 .. 44,
the step after that does not fit (44 + 5 > 48), skips the tail and goes to row 0; from then on a lap is the 9 steps 0, 5 .. 40. Sample b
restarts every 3 + b steps with a new prompt; 40 env steps are four laps and a bit. The worst age + advance is 25 + 9 = 34 <= 48, so
every call is legal. References: full-history `forward` of one (sample, episode) alone on a policy with the ring off, and the CPU oracle."""
import dataclasses
import math

import pytest
import torch

from tests.gpu_common import bare_policy, bf, max_abs, max_rel, ptr
from vima_amd import _lib
from vima_amd.policy import VIMAPolicy
from vima_testing import synthetic as syn
from oracle.vima_oracle import OraclePolicy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X3 = "bf16x3"


# ------------------------------------------------------------------------------------------ 1. the window rule, every kernel
def attn_ref_window(q, k, v, kmask, scale, q_off, f64=False):
    """`attn_ref` of tests/test_ops_gpu.py, mode 2, restated with the window: tri[i, j] = 0 iff q_off <= j < q_off + Lq and j - q_off > i.
    f64: the fp64 form of tests/test_bf16x3_gpu.py (a masked key's score IS finfo(fp32).min)."""
    if f64:
        q, k, v = q.double(), k.double(), v.double()
    B, Lq, H, D = q.shape
    Lk = k.shape[1]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k)
    tri = torch.ones(Lq, Lk, dtype=s.dtype)
    tri[:, q_off:q_off + Lq] = torch.tril(torch.ones(Lq, Lq, dtype=s.dtype))
    s = (s * scale) * tri + -1e4 * (1 - tri)
    fmin = torch.finfo(torch.float32).min
    if f64:
        s = torch.where(kmask[:, None, None, :], s, fmin)
    else:
        s = s + (1.0 - kmask[:, None, None, :].float()) * fmin
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v)


# (B, H, Lq, Lk, D): split-key kernel (Lq <= 32, Lk >= 64), one-wave kernel, four-wave kernel (Lq >= 64); impl 0 is the generic kernel at every shape
WINDOW_SHAPES = [(2, 8, 9, 128, 32), (2, 4, 17, 192, 64), (2, 8, 9, 48, 32), (2, 4, 40, 128, 64), (2, 8, 65, 192, 32), (1, 4, 65, 192, 64)]


def _window(pol, q, k, v, kmask, scale, impl, q_off):
    B, Lq, H, D = q.shape
    out = torch.full((B, Lq, H, D), float("nan"), device=DEV)
    qd, kd, vd, md = q.to(DEV), k.to(DEV), v.to(DEV), kmask.to(DEV)
    _lib.check(pol._lib.vima_op_attention_window(pol._handle, ptr(qd), ptr(kd), ptr(vd), ptr(md), B, H, Lq, k.shape[1], D, scale, impl, q_off,
                                                 ptr(out), pol._stream()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("prec,impl", [("fp32", 0), ("bf16", 0), ("bf16", 1), (X3, 1)])
@pytest.mark.parametrize("B,H,Lq,Lk,D", WINDOW_SHAPES)
def test_window_rule_in_every_attention_kernel(prec, impl, B, H, Lq, Lk, D):
    """The window at the start of the ring image, straddling a 64-key tile (q_off 60; not at Lk = 48, where it does not fit) and at its end.
    Tolerances: those of test_attention (tests/test_ops_gpu.py) for the same kernels; bf16x3: 2e-5 absolute against fp64 on inputs uniform in
    [-1, 1], as test_attention_split_bf16_against_fp64 (tests/test_bf16x3_gpu.py)."""
    pol = bare_policy(prec)
    pol.set_option("attn4_min_lq", 64)
    scale = 1.0 / math.sqrt(D)
    for q_off in sorted({o for o in (0, 60, Lk - Lq) if o + Lq <= Lk}):
        g = torch.Generator().manual_seed(1000 * Lq + Lk + q_off)
        if prec == X3:
            q, k, v = (torch.rand(B, L, H, D, generator=g) * 2 - 1 for L in (Lq, Lk, Lk))
        else:
            q, k, v = (torch.randn(B, L, H, D, generator=g) for L in (Lq, Lk, Lk))
        kmask = torch.rand(B, Lk, generator=g) > 0.2
        kmask[:, q_off] = True
        if B > 1:   # a freshly restarted sample: nothing outside the window is its own
            kmask[1, :q_off] = False
            kmask[1, q_off + Lq:] = False
        out = _window(pol, q, k, v, kmask, scale, impl, q_off)
        assert torch.isfinite(out).all()
        if prec == X3:
            err = (out.double() - attn_ref_window(q, k, v, kmask, scale, q_off, f64=True)).abs().max().item()
            print(f"[window] {prec} impl {impl} {(B, H, Lq, Lk, D)} q_off {q_off}: max err vs fp64 {err:.2e} (bound 2e-5)")
            assert err <= 2e-5, (q_off, err)
        else:
            ref = attn_ref_window(bf(q), bf(k), bf(v), kmask, scale, q_off) if prec == "bf16" else attn_ref_window(q, k, v, kmask, scale, q_off)
            err = max_rel(out, ref)
            print(f"[window] {prec} impl {impl} {(B, H, Lq, Lk, D)} q_off {q_off}: max_rel {err:.2e}")
            assert err < (1.5e-2 if prec == "bf16" else 1e-5), (q_off, err)


@pytest.mark.parametrize("prec,impl", [("fp32", 0), ("bf16", 0), ("bf16", 1), (X3, 1)])
@pytest.mark.parametrize("B,H,L,D", [(2, 8, 9, 32), (2, 4, 40, 64), (2, 8, 65, 32), (1, 4, 200, 64)])
def test_window_over_everything_is_the_plain_causal_mode(prec, impl, B, H, L, D):
    """q_off = 0, Lq = Lk: the legacy rule, bit for bit (vima_op_attention mode 2 on the same inputs)."""
    pol = bare_policy(prec)
    pol.set_option("attn4_min_lq", 64)
    g = torch.Generator().manual_seed(L + D)
    q, k, v = (torch.randn(B, L, H, D, generator=g) for _ in range(3))
    kmask = torch.rand(B, L, generator=g) > 0.2
    kmask[:, 0] = True
    scale = 1.0 / math.sqrt(D)
    got = _window(pol, q, k, v, kmask, scale, impl, 0)
    out = torch.full((B, L, H, D), float("nan"), device=DEV)
    qd, kd, vd, md = q.to(DEV), k.to(DEV), v.to(DEV), kmask.to(DEV)
    _lib.check(pol._lib.vima_op_attention(pol._handle, ptr(qd), ptr(kd), ptr(vd), ptr(md), None, B, H, L, L, D, scale, 2, impl, ptr(out), pol._stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, out.cpu())


# ------------------------------------------------------------------------------------------ the rollout scenario
NPOS, B, Q, QV, STEPS = 48, 3, 4, 2, 40
CFG = dataclasses.replace(syn.config("4M"), n_positions=NPOS)
TOL = {"fp32": 2e-5, "bf16": 3e-2, X3: 2e-5}   # test_per_sample_episode_restart_in_incremental_decoding / test_episode_restart_bf16x3
_sd = {}


def _state_dict():
    if not _sd:
        _sd["sd"] = syn.make_state_dict(CFG, 5)   # the default head gain: logits of ~0.1, the magnitude the 2e-5 logit gate of tests/test_policy_gpu.py is for
    return _sd["sd"]


def _policy(prec, **opts):
    pol = VIMAPolicy(**CFG.ctor_kwargs(), n_positions=NPOS, precision=prec, device=DEV)
    pol.load_state_dict(_state_dict(), strict=True)
    for k, v in opts.items():
        pol.set_option(k, v)
    return pol


def _prompt(e):
    """the prompts of every sample's episode number e"""
    return syn.make_prompt(B, n_segments=3, words_per_segment=3, q_per_view=QV, seed=300 + e)


def _data(pol, steps=STEPS):
    obs = syn.make_obs(steps, B, QV, seed=401)
    acts = syn.make_actions(steps, B, seed=601)
    otok, omask = pol.forward_obs_token(syn.to_device(obs, DEV))            # [steps, B, Q, E], [steps, B, Q]
    atok = pol.forward_action_token(syn.to_device(acts, DEV))              # [steps, B, E]: the action of step t is fed at step t + 1
    if steps == STEPS:   # the scenario needs invalid object tokens, in every sample
        assert not any(bool(omask[:, b].all()) for b in range(B))
    return obs, acts, otok, omask, atok


def _restarts(t, never=()):
    return [t > 0 and t % (3 + b) == 0 and b not in never for b in range(B)]


def _rollout(pol, otok, omask, atok, steps=STEPS, never=(), static=False, on_step=None):
    """`steps` env steps of the batch with the staggered restarts; returns the outputs [steps][B, E] and the episodes
    {(b, first step): (prompt tokens [Lp, 1, E], mask [1, Lp])}. static: the step's inputs go through fixed buffers (what graph replay needs)."""
    episode = [0] * B
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    pt, pm = pt.clone(), pm.clone()
    episodes = {(b, 0): (pt[:, b:b + 1].clone(), pm[b:b + 1].clone()) for b in range(B)}
    for t in range(steps):   # every episode's prompt up front: the stepping loop below allocates nothing but forward_step's output
        for b in range(B):
            if _restarts(t, never)[b]:
                episode[b] += 1
                nt, nm = pol.forward_prompt_assembly(syn.to_device(syn.cut_prompt(_prompt(episode[b]), [b]), DEV))
                episodes[(b, t)] = (nt.clone(), nm.clone())
    if static:
        so, sm, sa = torch.empty_like(otok[0]), torch.empty_like(omask[0]), torch.empty_like(atok[0])
    outs = torch.empty(steps, B, otok.shape[-1], device=DEV)
    for t in range(steps):
        flags = _restarts(t, never)
        if any(flags):
            for b in range(B):
                if flags[b]:
                    pt[:, b], pm[b] = episodes[(b, t)][0][:, 0], episodes[(b, t)][1][0]
            pol.restart_samples(torch.tensor(flags), pt, pm)
        if on_step:
            on_step(t)
        prev = atok[t - 1] if t > 0 else None
        if static:
            so.copy_(otok[t]); sm.copy_(omask[t])
            if t > 0:
                sa.copy_(prev)
            out = pol.forward_step(so, sm, sa if t > 0 else None, pt, pm, step=t)
        else:
            out = pol.forward_step(otok[t].contiguous(), omask[t].contiguous(), prev, pt, pm, step=t)
        outs[t].copy_(out)
        del out
    torch.cuda.synchronize()
    return list(outs), episodes


def _episode_ends(episodes, steps=STEPS):
    """(b, t0) -> t1, one past the episode's last step"""
    ends = {}
    for b in range(B):
        starts = sorted(t for (bb, t) in episodes if bb == b)
        for t0, t1 in zip(starts, starts[1:] + [steps]):
            ends[(b, t0)] = t1
    return ends


def _check_against_full_history(ref_pol, outs, episodes, otok, omask, atok, tol, steps=STEPS):
    worst = 0.0
    for (b, t0), t1 in _episode_ends(episodes, steps).items():
        ptok, pmask = episodes[(b, t0)]
        act = atok[t0:t1 - 1, b:b + 1].contiguous() if t1 - t0 > 1 else None
        full = ref_pol.forward(otok[t0:t1, b:b + 1].contiguous(), omask[t0:t1, b:b + 1].contiguous(), act, ptok, pmask)   # [T, 1, E]
        for t in range(t0, t1):
            ref = full[t - t0, 0]
            err = max_abs(outs[t][b], ref) / max(1.0, ref.abs().max().item())
            worst = max(worst, err)
            assert torch.isfinite(outs[t][b]).all() and err <= tol, (b, t0, t, err)
    return worst


@pytest.mark.parametrize("prec", ["fp32", "bf16", X3])
def test_rollout_over_four_laps_matches_every_episode_alone(prec):
    pol = _policy(prec, decode_ring=1)
    ref_pol = _policy(prec)
    obs, acts, otok, omask, atok = _data(pol)
    outs, episodes = _rollout(pol, otok, omask, atok)
    assert len(episodes) == 3 + 13 + 9 + 7
    worst = _check_against_full_history(ref_pol, outs, episodes, otok, omask, atok, TOL[prec])
    print(f"[rollout] {prec}: {len(episodes)} episodes over {STEPS} steps, worst error / max(1, |ref|) {worst:.3e} (bound {TOL[prec]:.0e})")
    if prec == "fp32":
        # sample 0's episode of steps 18 .. 20 lies wholly in the third lap (steps 18 .. 26): logits against the CPU oracle's own pipeline
        b, t0, t1 = 0, 18, 21
        assert _episode_ends(episodes)[(b, t0)] == t1
        orc = OraclePolicy(_state_dict(), **CFG.ctor_kwargs())
        o = obs["objects"]
        cut = {"objects": type(o)({k: type(o[k])({v: o[k][v][t0:t1, b:b + 1] for v in o[k]}) for k in o}), "ee": obs["ee"][t0:t1, b:b + 1]}
        ptok, pmask = orc.forward_prompt_assembly(syn.cut_prompt(_prompt(t0 // 3), [b]))
        o_otok, o_omask = orc.forward_obs_token(cut)
        o_atok = orc.forward_action_token({k: v[t0:t1 - 1, b:b + 1] for k, v in acts.items()})
        want = orc.action_logits(orc.forward(o_otok, o_omask, o_atok, ptok, pmask))[:, 0]                    # [3, 700]
        got = pol.action_logits(torch.stack([outs[t][b] for t in range(t0, t1)]))
        err = max_abs(got, want)
        print(f"[rollout] fp32 logits of the third-lap episode vs the oracle: {err:.3e} (bound 2e-5), max |logit| {want.abs().max().item():.3g}")
        assert err < 2e-5, err


# ------------------------------------------------------------------------------------------ 3. bounds
def test_a_sample_that_is_never_restarted_stops_the_ring_until_it_is():
    pol = _policy("fp32", decode_ring=1)
    ref_pol = _policy("fp32")
    _, _, otok, omask, atok = _data(pol, 10)
    left = {}
    outs, episodes = _rollout(pol, otok, omask, atok, steps=9, never=(2,), on_step=lambda t: left.__setitem__(t, pol.steps_left().tolist() if t > 0 else None))
    assert [left[t][2] for t in range(1, 9)] == [8, 7, 6, 5, 4, 3, 2, 1]
    # step 9: sample 0 restarts (9 % 3 == 0), sample 2 has age 44 and the step would skip 4 rows and write 5
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    pt, pm = pt.clone(), pm.clone()
    for b, t0 in ((0, 6), (1, 8)):
        pt[:, b], pm[b] = episodes[(b, t0)][0][:, 0], episodes[(b, t0)][1][0]
    nt, nm = pol.forward_prompt_assembly(syn.to_device(syn.cut_prompt(_prompt(3), [0]), DEV))
    pt[:, 0], pm[0] = nt[:, 0], nm[0]
    pol.restart_samples(torch.tensor([True, False, False]), pt, pm)
    sl = pol.steps_left()
    assert sl.dtype == torch.int32 and sl.device.type == "cpu" and sl[2].item() == 0 and sl[0].item() > 0 and sl[1].item() > 0, sl
    for _ in range(2):   # a failing call leaves the state as it was
        with pytest.raises(IndexError, match="sample 2"):
            pol.forward_step(otok[9].contiguous(), omask[9].contiguous(), atok[8], pt, pm, step=9)
        assert pol.steps_left().tolist() == sl.tolist()
    n2, m2 = pol.forward_prompt_assembly(syn.to_device(syn.cut_prompt(_prompt(7), [2]), DEV))
    pt[:, 2], pm[2] = n2[:, 0], m2[0]
    pol.restart_samples(torch.tensor([False, False, True]), pt, pm)
    assert pol.steps_left()[2].item() > 0
    out = pol.forward_step(otok[9].contiguous(), omask[9].contiguous(), atok[8], pt, pm, step=9)
    ref = ref_pol.forward(otok[9:10, 2:3].contiguous(), omask[9:10, 2:3].contiguous(), None, n2, m2)[0, 0]
    assert max_abs(out[2], ref) <= TOL["fp32"] * max(1.0, ref.abs().max().item())
    ref1 = ref_pol.forward(otok[8:10, 1:2].contiguous(), omask[8:10, 1:2].contiguous(), atok[8:9, 1:2].contiguous(), *episodes[(1, 8)])[1, 0]
    assert max_abs(out[1], ref1) <= TOL["fp32"] * max(1.0, ref1.abs().max().item())


def test_without_the_ring_the_batch_still_ends_at_the_same_step():
    """Ring off: (s + 1) (Q + 1) - 1 <= 48 holds up to step 8; step 9 raises code 34 whatever was restarted, as it always did."""
    pol = _policy("fp32")
    _, _, otok, omask, atok = _data(pol, 10)
    left = {}
    _rollout(pol, otok, omask, atok, steps=9, on_step=lambda t: left.__setitem__(t, pol.steps_left().tolist() if t > 0 else None))
    assert all(left[t] == [9 - t] * B for t in range(1, 9)), left
    assert pol.steps_left().tolist() == [0] * B
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    pol.restart_samples(torch.tensor([True] * B), pt, pm)
    with pytest.raises(IndexError, match="n_positions"):
        pol.forward_step(otok[9].contiguous(), omask[9].contiguous(), atok[8], pt, pm, step=9)


# ------------------------------------------------------------------------------------------ 4. graphs
def test_ring_rollout_under_graph_replay_is_exact_and_bounded():
    eager = _policy("bf16", decode_ring=1)
    _, _, otok, omask, atok = _data(eager)
    want, _ = _rollout(eager, otok, omask, atok, static=True)
    pol = _policy("bf16", decode_ring=1, graphs=1)
    stats = {}
    got, _ = _rollout(pol, otok, omask, atok, static=True, on_step=lambda t: stats.__setitem__(t, pol.graph_stats()))
    for t, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), t
    replays, captures = pol.graph_stats()
    print(f"[rollout] graphs: {captures} captures, {replays} replays over {STEPS} steps; captures at the start of laps 2..5: "
          f"{[stats[t][1] for t in (9, 18, 27, 36)]}")
    assert captures > 0 and replays > 0
    assert stats[36][1] == stats[27][1], "the fourth lap (steps 27 .. 35) must run on the graphs of the laps before it"
    assert captures == stats[27][1]


# ------------------------------------------------------------------------------------------ 5. batched restart
def test_batched_restart_gives_the_loops_bits_with_launches_independent_of_the_count():
    """The setting of test_head_major_prompt_kv_cache_is_bit_identical (tests/test_policy_gpu.py): 2M, B = 40, Lp = 512, bf16."""
    cfg = syn.config("2M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 11, head_gain=0.5)
    Bb, Lp, Qb, E = 40, 512, 4, cfg.embed_dim
    g = torch.Generator().manual_seed(3)
    ptok = torch.randn(Lp, Bb, E, generator=g).to(DEV)
    pmask = (torch.rand(Bb, Lp, generator=g) > 0.1)
    pmask[:, 0] = True
    pmask = pmask.to(DEV)
    ptok2 = torch.randn(Lp, Bb, E, generator=g).to(DEV)
    step_o = [torch.randn(1, Bb, Qb, E, generator=g).to(DEV) for _ in range(4)]
    step_a = [torch.randn(1, Bb, E, generator=g).to(DEV) for _ in range(4)]
    ones = torch.ones(1, Bb, Qb, dtype=torch.bool, device=DEV)

    def run(hm, batched, who):
        pol = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=512, precision="bf16", device=DEV)
        pol.load_state_dict(sd, strict=True)
        pol.set_option("kv_headmajor", hm)
        pol.set_option("restart_batched", batched)
        outs, launches, pt = [], None, ptok
        for k in range(4):
            if k == 2:
                flags = torch.zeros(Bb, dtype=torch.bool)
                flags[who] = True
                pt = ptok.clone()
                pt[:, who] = ptok2[:, who]
                pol.prof_enable(True)
                pol.restart_samples(flags, pt, pmask)
                torch.cuda.synchronize()
                launches = sum(v["launches"] for v in pol.prof_read().values())
                pol.prof_enable(False)
            outs.append(pol.forward_step(step_o[k], ones, step_a[k - 1] if k > 0 else None, pt, pmask, step=k).clone())
        torch.cuda.synchronize()
        return outs, launches

    for hm in (0, 1):
        loop3, n_loop3 = run(hm, 0, [1, 17, 30])
        bat3, n_bat3 = run(hm, 1, [1, 17, 30])
        _, n_bat1 = run(hm, 1, [17])
        for k, (a, b) in enumerate(zip(bat3, loop3)):
            assert torch.isfinite(a).all() and torch.equal(a, b), (hm, k, (a - b).abs().max().item())
        print(f"[restart] kv_headmajor {hm}: launches of one restart call: loop, 3 samples {n_loop3}; batched, 3 samples {n_bat3}; batched, 1 sample {n_bat1}")
        assert n_bat1 == n_bat3 == 2 + 2 * cfg.xf_n_layers and n_bat3 < n_loop3


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_restart_of_short_prompts_matches_the_fresh_episode(prec):
    """4M, the prompts of syn.make_prompt(B, 3, 3, 2) (21 tokens: the per-sample form is kept up to 32), two samples restarted together."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 5, head_gain=0.5)
    pol = VIMAPolicy(**cfg.ctor_kwargs(), precision=prec, device=DEV)
    pol.load_state_dict(sd, strict=True)
    pt, pm = pol.forward_prompt_assembly(syn.to_device(syn.make_prompt(B, n_segments=3, words_per_segment=3, q_per_view=QV, seed=31), DEV))
    nt, nm = pol.forward_prompt_assembly(syn.to_device(syn.make_prompt(B, n_segments=3, words_per_segment=3, q_per_view=QV, seed=32), DEV))
    otok, omask = pol.forward_obs_token(syn.to_device(syn.make_obs(5, B, QV, seed=40), DEV))
    atok = pol.forward_action_token(syn.to_device(syn.make_actions(5, B, seed=60), DEV))
    pt, pm = pt.clone(), pm.clone()
    first = [pt.clone(), pm.clone()]
    outs = []
    for t in range(5):
        if t == 2:
            pt[:, 0], pm[0], pt[:, 2], pm[2] = nt[:, 0], nm[0], nt[:, 2], nm[2]
            pol.restart_samples(torch.tensor([True, False, True]), pt, pm)
        outs.append(pol.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t > 0 else None, pt, pm, step=t).clone())
    ref_pol = VIMAPolicy(**cfg.ctor_kwargs(), precision=prec, device=DEV)
    ref_pol.load_state_dict(sd, strict=True)
    for b, t0, ptok, pmask in ((0, 2, nt, nm), (2, 2, nt, nm), (1, 0, *first)):
        full = ref_pol.forward(otok[t0:, b:b + 1].contiguous(), omask[t0:, b:b + 1].contiguous(), atok[t0:4, b:b + 1].contiguous(),
                               ptok[:, b:b + 1].contiguous(), pmask[b:b + 1].contiguous())
        for t in range(t0, 5):
            ref = full[t - t0, 0]
            assert max_abs(outs[t][b], ref) <= TOL[prec] * max(1.0, ref.abs().max().item()), (b, t)


# ------------------------------------------------------------------------------------------ 6. steps_left
def _steps_left_model(ring, wp, age, step, lq=Q + 1, lmax=NPOS):
    """The bookkeeping restated: ring -- run (write pointer, age) forward until age + advance > lmax; linear -- steps up to (lmax + 1) // lq - 1."""
    if not ring:
        return max(0, (lmax + 1) // lq - 1 - step)
    n = 0
    while True:
        adv, row = (lmax - wp + lq, 0) if wp + lq > lmax else (lq, wp)
        if age + adv > lmax:
            return n
        age, wp, n = age + adv, row + lq, n + 1


@pytest.mark.parametrize("ring", [1, 0])
def test_steps_left_against_a_restatement_of_the_bookkeeping(ring):
    pol = _policy("fp32", decode_ring=ring)
    _, _, otok, omask, atok = _data(pol, 8)
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    g = torch.Generator().manual_seed(17 + ring)
    wp, age, done = 0, [0] * B, 0
    for t in range(60):
        flags = (torch.rand(B, generator=g) < 0.25).tolist() if t > 0 else [False] * B
        model = [_steps_left_model(ring, wp, a, t - 1) for a in age] if t > 0 else None
        if t > 0 and min(model) == 0:       # somebody (ring off: everybody) is out of rows: restart them; without the ring start over
            if not ring:
                break
            flags = [f or m == 0 for f, m in zip(flags, model)]
        if any(flags):
            pol.restart_samples(torch.tensor(flags), pt, pm)
            age = [0 if f else a for f, a in zip(flags, age)]
        if t > 0:
            assert pol.steps_left().tolist() == [_steps_left_model(ring, wp, a, t - 1) for a in age], t
        lq = Q + 1 if t > 0 else Q
        adv, row = (NPOS - wp + lq, 0) if wp + lq > NPOS else (lq, wp)
        pol.forward_step(otok[t % 8].contiguous(), omask[t % 8].contiguous(), atok[(t - 1) % 8] if t > 0 else None, pt, pm, step=t)
        wp, age, done = row + lq, [a + adv for a in age], done + 1
    assert done == (60 if ring else 9)
