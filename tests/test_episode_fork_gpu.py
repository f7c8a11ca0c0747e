"""Branch rollouts on the MI355X: `VIMAPolicy.fork_samples` (vima_decode_fork) and the copy kernel alone (vima_op_episode_fork).

The scenario is tests/episode_fork_reference.py (model 4M, n_positions 48, B = 4, Q = 4, 40 steps, staggered restarts as in
tests/test_rollout_gpu.py, one history install, six forks); tests/test_episode_fork_build.py asserts on the CPU that it contains a fork behind a
wrap (two live ranges), one of a just-restarted source, one of a source with an installed history, forks with two destinations and two groups.
Slot b is fed column b of the step's data, so branches diverge by themselves; on the step right after a fork a destination is fed its source's
column and must return its source's bits. Every (slot, lineage) is compared with `forward(<the lineage's full history>)` of a ring-off policy."""
import ctypes
import dataclasses

import pytest
import torch

from tests import episode_fork_reference as fref
from tests.gpu_common import bare_policy, max_abs, ptr
from vima_amd import _lib
from vima_amd.baselines import build_baseline
from vima_amd.policy import VIMAPolicy
from vima_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X3 = "bf16x3"
NPOS, B, Q, QV, STEPS = fref.NPOS, fref.B, fref.Q, 2, fref.STEPS
CFG = dataclasses.replace(syn.config("4M"), n_positions=NPOS)
TOL = {"fp32": 2e-5, "bf16": 3e-2, X3: 2e-5}   # the gates of tests/test_rollout_gpu.py, error / max(1, |ref|)
_sd = {}


def _state_dict(cfg=CFG):
    if cfg not in _sd:
        _sd[cfg] = syn.make_state_dict(cfg, 5)
    return _sd[cfg]


def _policy(prec, cfg=CFG, **opts):
    pol = VIMAPolicy(**cfg.ctor_kwargs(), n_positions=NPOS, precision=prec, device=DEV)
    pol.load_state_dict(_state_dict(cfg), strict=True)
    for k, v in opts.items():
        pol.set_option(k, v)
    return pol


def _prompt(e):
    """the prompts of every sample's episode number e"""
    return syn.make_prompt(B, n_segments=3, words_per_segment=3, q_per_view=QV, seed=300 + e)


def _data(pol, steps=STEPS):
    otok, omask = pol.forward_obs_token(syn.to_device(syn.make_obs(steps, B, QV, seed=401), DEV))      # [steps, B, Q, E], [steps, B, Q]
    atok = pol.forward_action_token(syn.to_device(syn.make_actions(steps, B, seed=601), DEV))         # [steps, B, E]: the action of step t is fed at step t + 1
    return otok, omask, atok


def _i32(xs):
    a = (ctypes.c_int32 * max(len(xs), 1))(*xs)
    return a


# ------------------------------------------------------------------------------------------ 1. the kernel alone
def _op_fork(cache, groups):
    """groups: [(source, [destinations], [(row0, row1)])] -> vima_op_episode_fork in place on `cache` [NL, B, L, N]"""
    pol = bare_policy("fp32")
    NL, Bc, L, N = cache.shape
    gs, gp, ds, rp, rg = [], [0], [], [0], []
    for s, d, r in groups:
        gs.append(s)
        ds += d
        gp.append(len(ds))
        for lo, hi in r:
            rg += [lo, hi]
        rp.append(len(rg) // 2)
    return pol._lib.vima_op_episode_fork(pol._handle, ptr(cache), cache.element_size(), NL, Bc, L, N, _i32(gs), _i32(gp), _i32(ds), _i32(rp), _i32(rg),
                                         len(groups), pol._stream())


OP_CASES = {
    "empty": [(0, [1], [(5, 5)])],
    "one-row": [(2, [0], [(7, 8)])],
    "ending-at-L": [(1, [3], [(40, 48)])],
    "two-ranges": [(4, [2], [(0, 5), (29, 44)])],
    "one-to-three": [(0, [4, 1, 3], [(3, 17)])],
    "two-groups": [(1, [0], [(0, 48)]), (3, [2, 4], [(10, 11), (47, 48)])],
    "eleven-destinations": None,   # more than kForkMaxDst: the group is split over two jobs
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("NL,N", [(1, 128), (3, 640), (3, 128), (1, 640)])
@pytest.mark.parametrize("case", list(OP_CASES))
def test_copy_kernel_alone_is_exact_and_touches_nothing_else(case, NL, N, dtype):
    L, Bc = 48, 5
    groups = OP_CASES[case]
    if groups is None:
        Bc, groups = 13, [(6, [b for b in range(13) if b != 6 and b != 9], [(1, 48)])]
    g = torch.Generator().manual_seed(NL * 1000 + N)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (NL * Bc * L * N * dtype.itemsize // 4,), generator=g, dtype=torch.int64).to(torch.int32)
    cache = bits.view(dtype).view(NL, Bc, L, N).to(DEV)                   # distinctive: random BITS in every element (NaN patterns included)
    want = cache.clone().view(torch.int32 if dtype == torch.float32 else torch.int16)
    for s, dsts, ranges in groups:
        for d in dsts:
            for lo, hi in ranges:
                want[:, d, lo:hi] = want[:, s, lo:hi]
    _lib.check(_op_fork(cache, groups))
    torch.cuda.synchronize()
    got = cache.view(want.dtype)
    assert torch.equal(got, want), (case, (got != want).nonzero()[:4].tolist())


def test_copy_kernel_refusals():
    cache = torch.zeros(1, 4, 8, 128, device=DEV)
    for groups in ([(0, [0], [(0, 1)])], [(0, [1], [(0, 1)]), (1, [2], [(0, 1)])], [(0, [1, 1], [(0, 1)])], [(0, [4], [(0, 1)])], [(0, [1], [(0, 9)])],
                   [(0, [1], [(3, 2)])]):
        assert _op_fork(cache, groups) != 0, groups
    odd = torch.zeros(1, 2, 8, 6, device=DEV)                                # 24-byte rows
    with pytest.raises(ValueError, match="16 bytes"):
        _lib.check(_op_fork(odd, [(0, [1], [(0, 1)])]))
    torch.cuda.synchronize()
    assert not cache.any() and not odd.any()


# ------------------------------------------------------------------------------------------ the rollout scenario
class _Lineage:
    def __init__(self, slot, prompt, steps=(), own_from=0, pure=True):
        self.slot, self.prompt, self.steps, self.own_from, self.pure = slot, prompt, list(steps), own_from, pure


def _rollout(pol, otok, omask, atok, ring=True, forks=True, static=False, check_bits=True):
    """The scenario. -> outputs [steps, B, E], the closed lineages, and the (slot, step) pairs whose lineage was never forked ("pure")."""
    steps = STEPS if ring else fref.LINEAR_STEPS
    number = [0] * B
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    pt, pm = pt.clone(), pm.clone()
    pt0, pm0 = pt, pm
    live = [_Lineage(b, (pt[:, b:b + 1].clone(), pm[b:b + 1].clone())) for b in range(B)]
    done, pure_steps = [], set()
    new_prompts = {}
    for t in range(steps):   # every episode's prompt up front
        for b in range(B):
            if fref.events(t, ring)[0][b]:
                number[b] += 1
                nt, nm = pol.forward_prompt_assembly(syn.to_device(syn.cut_prompt(_prompt(number[b]), [b]), DEV))
                new_prompts[(b, t)] = (nt.clone(), nm.clone())
    if static:
        so, sm, sa = torch.empty_like(otok[0]), torch.empty_like(omask[0]), torch.empty_like(atok[0])
    outs = torch.empty(steps, B, otok.shape[-1], device=DEV)
    for t in range(steps):
        flags, inst, source = fref.events(t, ring)
        if not forks:
            source = None
        if any(flags):
            for b in range(B):
                if flags[b]:
                    pt[:, b], pm[b] = new_prompts[(b, t)][0][:, 0], new_prompts[(b, t)][1][0]
                    done.append(live[b])
                    live[b] = _Lineage(b, new_prompts[(b, t)])
            pol.restart_samples(torch.tensor(flags), pt, pm)
        if inst:   # the sample re-joins with its own last T steps: its lineage stays, its state is rebuilt by the history pass
            b, T = inst
            hist = live[b].steps[-T:]
            assert len(live[b].steps) == T
            h_obs = torch.stack([otok[s, c] for s, c in hist]).unsqueeze(1).contiguous()
            h_mask = torch.stack([omask[s, c] for s, c in hist]).unsqueeze(1).contiguous()
            h_act = torch.stack([atok[s - 1, c] for s, c in hist[1:]]).unsqueeze(1).contiguous() if T > 1 else None
            pol.restart_samples(torch.tensor([x == b for x in range(B)]), pt, pm, history=(h_obs, h_mask, h_act))
        cols = list(range(B))
        pairs = []
        if source:
            before = pol.steps_left().tolist()
            differs = [not (torch.equal(pt[:, b], pt[:, s]) and torch.equal(pm[b], pm[s])) for b, s in enumerate(source)]
            rt, rm = pol.fork_samples(source, pt, pm)
            assert rt is pt and rm is pm, "the prompt tensors are updated in place"
            after = pol.steps_left().tolist()
            for b, s in enumerate(source):
                assert after[b] == before[s], (t, b, s, before, after)
                if s != b:
                    assert torch.equal(pt[:, b], pt[:, s]) and torch.equal(pm[b], pm[s])
                    pairs.append((b, s, differs[b]))
                    done.append(live[b])
                    live[b] = _Lineage(b, live[s].prompt, live[s].steps, own_from=len(live[s].steps), pure=False)
                    cols[b] = s
        idx = torch.tensor(cols, device=DEV)
        o, m = otok[t].index_select(0, idx), omask[t].index_select(0, idx)
        a = atok[t - 1].index_select(0, idx) if t > 0 else None
        if static:
            so.copy_(o); sm.copy_(m)
            if t > 0:
                sa.copy_(a)
            o, m, a = so, sm, (sa if t > 0 else None)
        out = pol.forward_step(o, m, a, pt, pm, step=t)
        outs[t].copy_(out)
        if check_bits:
            for b, s, _ in pairs:   # fed the source's inputs, the destination returns the source's output bit for bit
                assert torch.equal(out[b], out[s]), (t, b, s, (out[b] - out[s]).abs().max().item())
        del out
        for b in range(B):
            live[b].steps.append((t, cols[b]))
            if live[b].pure:
                pure_steps.add((b, t))
    torch.cuda.synchronize()
    assert pt is pt0 and pm is pm0
    return outs, done + live, pure_steps


def _check_lineages(ref_pol, outs, lineages, otok, omask, atok, tol):
    worst, n = 0.0, 0
    for ln in lineages:
        if ln.own_from >= len(ln.steps):
            continue
        obs = torch.stack([otok[s, c] for s, c in ln.steps]).unsqueeze(1).contiguous()
        msk = torch.stack([omask[s, c] for s, c in ln.steps]).unsqueeze(1).contiguous()
        act = torch.stack([atok[s - 1, c] for s, c in ln.steps[1:]]).unsqueeze(1).contiguous() if len(ln.steps) > 1 else None
        full = ref_pol.forward(obs, msk, act, *ln.prompt)               # [T, 1, E]
        for i in range(ln.own_from, len(ln.steps)):
            t, ref = ln.steps[i][0], full[i, 0]
            err = max_abs(outs[t][ln.slot], ref) / max(1.0, ref.abs().max().item())
            worst, n = max(worst, err), n + 1
            assert torch.isfinite(outs[t][ln.slot]).all() and err <= tol, (ln.slot, ln.steps[0], t, err)
    return worst, n


# ------------------------------------------------------------------------------------------ 2. ring rollout with forks
@pytest.mark.parametrize("hm", [0, 1])
@pytest.mark.parametrize("prec", ["fp32", "bf16", X3])
def test_ring_rollout_with_forks_matches_every_lineage_alone(prec, hm):
    pol = _policy(prec, decode_ring=1, kv_headmajor=hm)
    ref_pol = _policy(prec)
    otok, omask, atok = _data(pol)
    outs, lineages, _ = _rollout(pol, otok, omask, atok)              # asserts the bit-for-bit equality on the step after every fork
    worst, n = _check_lineages(ref_pol, outs, lineages, otok, omask, atok, TOL[prec])
    assert n == STEPS * B
    print(f"[fork] {prec} kv_headmajor {hm}: {len(lineages)} lineages, {n} (slot, step) outputs, worst error / max(1, |ref|) {worst:.3e} "
          f"(bound {TOL[prec]:.0e}); destinations equal their sources bit for bit after each of the {len(fref.FORKS)} forks")


# ------------------------------------------------------------------------------------------ 3. bystanders keep their bits
def test_samples_outside_a_fork_keep_their_bits():
    pol, twin = _policy("fp32", decode_ring=1), _policy("fp32", decode_ring=1)
    otok, omask, atok = _data(pol)
    got, _, pure = _rollout(pol, otok, omask, atok)
    want, _, all_pure = _rollout(twin, otok, omask, atok, forks=False)
    assert len(all_pure) == STEPS * B and STEPS * B // 3 < len(pure) < STEPS * B
    for b, t in sorted(pure):
        assert torch.equal(got[t][b], want[t][b]), (b, t)
    bystanders = [(b, t) for t, source in fref.FORKS.items() for b in range(B) if source[b] == b and source.count(b) == 1 and (b, t) in pure]
    assert len(bystanders) >= 4, bystanders                            # samples that were neither source nor destination of a fork, on the step after it


# ------------------------------------------------------------------------------------------ 4. linear cache
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fork_on_the_linear_cache(prec):
    pol, ref_pol = _policy(prec, decode_ring=0), _policy(prec)
    otok, omask, atok = _data(pol, fref.LINEAR_STEPS)
    outs, lineages, _ = _rollout(pol, otok, omask, atok, ring=False)  # steps_left of every pair is compared inside
    worst, n = _check_lineages(ref_pol, outs, lineages, otok, omask, atok, TOL[prec])
    assert n == fref.LINEAR_STEPS * B and pol.steps_left().tolist() == [0] * B
    print(f"[fork] linear cache {prec}: worst error / max(1, |ref|) {worst:.3e} (bound {TOL[prec]:.0e})")


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_change_nothing():
    pol, twin = _policy("fp32", decode_ring=1), _policy("fp32", decode_ring=1)
    otok, omask, atok = _data(pol, 4)
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    with pytest.raises(_lib.VimaError, match="no running episode"):
        pol.fork_samples([0, 0, 2, 3], pt, pm)
    for t in range(3):
        for p in (pol, twin):
            p.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t else None, pt, pm, step=t)
    keep_t, keep_m, left = pt.clone(), pm.clone(), pol.steps_left().tolist()
    with pytest.raises(ValueError, match=r"source\[0\] = 1 is itself a destination"):
        pol.fork_samples([1, 2, 2, 3], pt, pm)                           # a chain
    with pytest.raises(ValueError, match=r"source\[0\] = 1 is itself a destination"):
        pol.fork_samples([1, 0, 2, 3], pt, pm)                           # a swap
    with pytest.raises(ValueError, match=r"source\[3\] = 4 is not a sample"):
        pol.fork_samples([0, 1, 2, 4], pt, pm)
    with pytest.raises(AssertionError):
        pol.fork_samples([0, 1, 2], pt, pm)
    with pytest.raises(_lib.VimaError, match="no running episode"):
        _lib.check(pol._lib.vima_decode_fork(pol._handle, _i32([0, 0]), 2, pol._stream()))   # wrong B
    with pytest.raises(_lib.VimaError, match="vima_decode_fork"):
        _lib.check(pol._lib.vima_seq_decode_fork(pol._handle, _i32([0, 0, 2, 3]), 4, pol._stream()))
    assert torch.equal(pt, keep_t) and torch.equal(pm, keep_m) and pol.steps_left().tolist() == left
    pol.fork_samples(list(range(B)), pt, pm)                             # the identity: a no-op
    a = pol.forward_step(otok[3].contiguous(), omask[3].contiguous(), atok[2], pt, pm, step=3)
    b = twin.forward_step(otok[3].contiguous(), omask[3].contiguous(), atok[2], pt, pm, step=3)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 6. graphs
def test_forked_rollout_under_graph_replay_is_exact():
    otok, omask, atok = _data(_policy("bf16"))
    want, _, _ = _rollout(_policy("bf16", decode_ring=1), otok, omask, atok, static=True)
    pol = _policy("bf16", decode_ring=1, graphs=1)
    got, _, _ = _rollout(pol, otok, omask, atok, static=True)
    for t in range(STEPS):
        assert torch.equal(got[t], want[t]), t
    plain = _policy("bf16", decode_ring=1, graphs=1)
    _rollout(plain, otok, omask, atok, static=True, forks=False)
    (replays, captures), (p_replays, p_captures) = pol.graph_stats(), plain.graph_stats()
    print(f"[fork] graphs: {captures} captures / {replays} replays with forks, {p_captures} / {p_replays} without")
    assert captures == p_captures > 0 and replays == p_replays > 0


# ------------------------------------------------------------------------------------------ 7. launch count
def test_launch_count_does_not_depend_on_pairs_or_layers():
    """The 4M config has 2 decoder layers itself, so the other layer count is a 4-layer variant of it."""
    counts = {}
    for layers in (CFG.xf_n_layers, 4):
        cfg = dataclasses.replace(CFG, xf_n_layers=layers)
        for source in ([0, 0, 2, 3], [0, 0, 0, 0]):
            pol = _policy("bf16", cfg=cfg, decode_ring=1)
            otok, omask, atok = _data(pol, 2)
            pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
            pt, pm = pt.clone(), pm.clone()
            for t in range(2):
                pol.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t else None, pt, pm, step=t)
            pol.prof_enable(True)
            pol.fork_samples(source, pt, pm)
            torch.cuda.synchronize()
            counts[(layers, source.count(0) - 1)] = sum(v["launches"] for v in pol.prof_read().values())
            pol.prof_enable(False)
    print(f"[fork] launches of one fork call by (layers, destinations): {counts}")
    assert CFG.xf_n_layers == 2 and len(counts) == 4 and len(set(counts.values())) == 1 and 1 <= next(iter(counts.values())) <= 3, counts


# ------------------------------------------------------------------------------------------ 8. Flamingo
def test_flamingo_fork_samples():
    cfg = syn.BaselineConfig("flamingo", 256, 2, 8, xattn_n_heads=8)
    sd = syn.make_baseline_state_dict(cfg, seed=51)
    pol = build_baseline(cfg, precision="fp32", device=DEV)
    pol.load_state_dict(sd, strict=True)
    T, Bf = 4, 3
    prompts = syn.to_device(syn.make_rgb_prompt(Bf, layout=[[0, 1, 0], [1, 0, 0, 1], [0, 0, 1]], seed=52), DEV)
    with torch.no_grad():
        ptok, pmask = pol.forward_prompt_assembly(prompts)
        otok = pol.forward_obs_token(syn.to_device(syn.make_rgb_obs(T, Bf, seed=53), DEV))
        atok = pol.forward_action_token(syn.to_device(syn.make_actions(T, Bf, seed=54), DEV))
        ptok, pmask = ptok.contiguous().clone(), pmask.clone()
        p1 = (ptok[:, 1:2].clone(), pmask[1:2].clone())
        for t in range(2):
            pol.forward_step(otok[t], None if t == 0 else atok[t - 1], ptok, pmask, t)
        assert not torch.equal(ptok[:, 2], ptok[:, 1])
        pol.fork_samples([0, 1, 1], ptok, pmask)
        cols = torch.tensor([0, 1, 1], device=DEV)
        out2 = pol.forward_step(otok[2].index_select(0, cols), atok[1].index_select(0, cols), ptok, pmask, 2)
        assert torch.equal(out2[2], out2[1])
        out3 = pol.forward_step(otok[3], atok[2], ptok, pmask, 3)                 # the branches diverge
        assert not torch.equal(out3[2], out3[1])
        obs = torch.stack([otok[0, 1], otok[1, 1], otok[2, 1], otok[3, 2]]).unsqueeze(1).contiguous()
        act = torch.stack([atok[0, 1], atok[1, 1], atok[2, 2]]).unsqueeze(1).contiguous()
        full = pol.forward(obs, act, *p1)
        for got, ref in ((out2[2], full[2, 0]), (out3[2], full[3, 0])):
            assert max_abs(got, ref) < 2e-5 * max(1.0, full.abs().max().item())
