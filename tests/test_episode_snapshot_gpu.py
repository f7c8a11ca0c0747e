"""Episode snapshots on the MI355X: `VIMAPolicy.snapshot_samples` / `restore_samples` (vima_decode_snapshot / vima_decode_restore) and the pack /
unpack kernels alone (vima_op_episode_pack / vima_op_episode_unpack).

The scenario is tests/episode_snapshot_reference.py (model 4M, n_positions 48, B = 4, Q = 4, 40 steps, staggered restarts as in
tests/test_rollout_gpu.py, one history install, one fork, one chunk of T = 2, five snapshots, six restores); tests/test_episode_snapshot_build.py
asserts on the CPU that it contains a snapshot behind a wrap, restores whose rows straddle the wrap, a backtrack into the own slot, a restore into
two slots, a just-restarted sample, an installed history, a forked destination, a restore after a chunk and a prompt-less snapshot. Slot b is fed
column b of the step's data. Every (slot, lineage) is compared with `forward(<the lineage's full history>)` of a ring-off policy.

Same moment: a snapshot restored at once lands at the row numbers it was taken from (asserted on the restatement), so the destination holds its
source's bits in every row its attention reads with a non-zero weight; it returned its source's output bit for bit in fp32, bf16 and bf16x3."""
import ctypes
import dataclasses

import pytest
import torch

from tests import episode_snapshot_reference as sref
from tests.gpu_common import bare_policy, max_abs, ptr
from tests.test_episode_fork_gpu import CFG, DEV, QV, TOL, X3, _check_lineages, _data, _i32, _Lineage, _policy, _prompt
from vima_amd import _lib
from vima_amd.baselines import build_baseline
from vima_amd.episodes import EpisodeSnapshot
from vima_testing import synthetic as syn

pytestmark = pytest.mark.gpu
NPOS, B, Q, STEPS = sref.NPOS, sref.B, sref.Q, sref.STEPS


# ------------------------------------------------------------------------------------------ 1. the kernels alone
def _ptrs(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[t.data_ptr() if isinstance(t, torch.Tensor) else t for t in ts])


def _op(name, cache, D, rowmap, n_map, jobs, payloads):
    """jobs: [(sample, nrows)] -> vima_op_episode_pack / _unpack on `cache` [NL, B, L, N]"""
    pol = bare_policy("fp32")
    NL, Bc, L, N = cache.shape
    fn = getattr(pol._lib, name)
    return fn(pol._handle, ptr(cache), cache.element_size(), NL, Bc, L, N, D, _i32(rowmap) if rowmap is not None else None, n_map,
              _i32([s for s, _ in jobs]), _i32([n for _, n in jobs]), ctypes.cast(_ptrs(payloads), ctypes.c_void_p), len(jobs), pol._stream())


def _bits(shape, dtype, seed):
    """random BITS in every element (NaN patterns included), viewed as integers for exact comparison"""
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(-2 ** 31, 2 ** 31 - 1, (n * dtype.itemsize // 4,), generator=g, dtype=torch.int64).to(torch.int32)
    return raw.view(dtype).view(*shape).to(DEV)


def _ints_view(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _logical(cache, D):
    """[NL, B, L, N] as stored -> a VIEW-free copy of the logical rows [NL, B, L, N] (head-major blocks [N / D][L][D] transposed back)"""
    NL, Bc, L, N = cache.shape
    return cache if not D else cache.reshape(NL, Bc, N // D, L, D).permute(0, 1, 3, 2, 4).reshape(NL, Bc, L, N)


def _stored(logical, D):
    NL, Bc, L, N = logical.shape
    return logical if not D else logical.reshape(NL, Bc, L, N // D, D).permute(0, 1, 3, 2, 4).reshape(NL, Bc, L, N)


WRAP = list(range(40, 48)) + list(range(0, 5))
OP_CASES = {   # (row map or None = identity, n_map, jobs [(sample, nrows)], D)
    "empty-map": ([], 0, [(0, 0)], 0),
    "one-row": ([7], 1, [(2, 1)], 0),
    "ending-at-L-1": (list(range(40, 48)), 8, [(1, 8)], 0),
    "crossing-the-wrap": (WRAP, 13, [(3, 13)], 0),
    "two-suffixes": (WRAP, 13, [(0, 13), (4, 5)], 0),
    "head-major-32": (None, 48, [(1, 48), (3, 48)], 32),
    "head-major-64": (None, 48, [(2, 48)], 64),
    "head-major-64-mapped": (WRAP, 13, [(2, 13), (0, 2)], 64),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("NL,N", [(1, 128), (3, 640)])
@pytest.mark.parametrize("case", list(OP_CASES))
def test_pack_and_unpack_alone_are_exact_and_touch_nothing_else(case, NL, N, dtype):
    L, Bc = 48, 5
    rowmap, n_map, jobs, D = OP_CASES[case]
    table = list(range(n_map)) if rowmap is None else rowmap
    cache = _bits((NL, Bc, L, N), dtype, NL * 1000 + N)
    keep = cache.clone()
    pays = [torch.zeros(NL, max(n, 1), N, dtype=dtype, device=DEV) for _, n in jobs]
    _lib.check(_op("vima_op_episode_pack", cache, D, rowmap, n_map, jobs, pays))
    torch.cuda.synchronize()
    assert torch.equal(_ints_view(cache), _ints_view(keep)), "pack writes nothing into the cache"
    rows_logical = _logical(keep, D)
    for (s, n), p in zip(jobs, pays):
        want = rows_logical[:, s, table[len(table) - n:]] if n else p[:, :0]
        assert torch.equal(_ints_view(p[:, :n].contiguous()), _ints_view(want.contiguous())), (case, s, n)
        assert n > 0 or not p.any()
    # unpack into ANOTHER sample of another buffer: the rows arrive, everything else stays
    other = _bits((NL, Bc, L, N), dtype, NL * 1000 + N + 1)
    shifted = [((s + 1) % Bc, n) for s, n in jobs]
    want = _logical(other, D).clone()
    for (d, n), p in zip(shifted, pays):
        if n:
            want[:, d, table[len(table) - n:]] = p[:, :n]
    want = _stored(want, D).contiguous()
    _lib.check(_op("vima_op_episode_unpack", other, D, rowmap, n_map, shifted, pays))
    torch.cuda.synchronize()
    got, exp = _ints_view(other), _ints_view(want)
    assert torch.equal(got, exp), (case, (got != exp).nonzero()[:4].tolist())


def test_pack_and_unpack_refusals_touch_nothing():
    cache = _bits((1, 4, 8, 128), torch.float32, 5)
    keep = cache.clone()
    pay = torch.zeros(1, 4, 128, device=DEV)
    wide = torch.zeros(1 * 4 * 128 + 4, device=DEV)
    host = torch.zeros(1, 4, 128)
    for name in ("vima_op_episode_pack", "vima_op_episode_unpack"):
        assert _op(name, cache, 0, [0, 1, 2, 8], 4, [(0, 4)], [pay]) != 0                     # a map entry >= L
        assert _op(name, cache, 0, [0, 1, 2, -1], 4, [(0, 4)], [pay]) != 0
        assert _op(name, cache, 0, [0, 1, 2, 3], 4, [(4, 4)], [pay]) != 0                     # not a sample
        assert _op(name, cache, 0, [0, 1, 2, 3], 4, [(0, 5)], [pay]) != 0                     # more rows than the map holds
        assert _op(name, cache, 48, [0, 1, 2, 3], 4, [(0, 4)], [pay]) != 0                    # D does not divide N
        with pytest.raises(ValueError, match="not 16-byte aligned"):
            _lib.check(_op(name, cache, 0, [0, 1, 2, 3], 4, [(0, 4)], [wide.data_ptr() + 4]))
        with pytest.raises(ValueError, match="not device memory"):
            _lib.check(_op(name, cache, 0, [0, 1, 2, 3], 4, [(0, 4)], [host]))
        odd = torch.zeros(1, 2, 8, 6, device=DEV)                                             # 24-byte rows
        with pytest.raises(ValueError, match="16 bytes"):
            _lib.check(_op(name, odd, 0, [0], 1, [(0, 1)], [pay]))
    with pytest.raises(ValueError, match="listed twice"):
        _lib.check(_op("vima_op_episode_unpack", cache, 0, [0, 1], 2, [(1, 2), (1, 1)], [pay, pay]))
    torch.cuda.synchronize()
    assert torch.equal(_ints_view(cache), _ints_view(keep)) and not pay.any() and not wide.any() and not host.any()


# ------------------------------------------------------------------------------------------ the rollout scenario
def _history(ln, T, otok, omask, atok):
    hist = ln.steps[-T:]
    h_obs = torch.stack([otok[s, c] for s, c in hist]).unsqueeze(1).contiguous()
    h_mask = torch.stack([omask[s, c] for s, c in hist]).unsqueeze(1).contiguous()
    h_act = torch.stack([atok[s - 1, c] for s, c in hist[1:]]).unsqueeze(1).contiguous() if T > 1 else None
    return h_obs, h_mask, h_act


def _rollout(pol, otok, omask, atok, ring=True, restores=True, static=False):
    """The scenario. -> outputs [steps, B, E], every lineage, and the (slot, step) pairs of lineages no restore has touched ("pure")."""
    steps = STEPS if ring else sref.LINEAR_STEPS
    left_ref = sref.replay(ring)[2]
    number = [0] * B
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    pt, pm = pt.clone(), pm.clone()
    pt0, pm0 = pt, pm
    live = [_Lineage(b, (pt[:, b:b + 1].clone(), pm[b:b + 1].clone())) for b in range(B)]
    done, pure_steps, held = [], set(), {}
    new_prompts = {}
    for t in range(steps):   # every episode's prompt up front
        for b in range(B):
            if sref.events(t, ring)[0][b]:
                number[b] += 1
                nt, nm = pol.forward_prompt_assembly(syn.to_device(syn.cut_prompt(_prompt(number[b]), [b]), DEV))
                new_prompts[(b, t)] = (nt.clone(), nm.clone())
    if static:
        so, sm, sa = torch.empty_like(otok[0]), torch.empty_like(omask[0]), torch.empty_like(atok[0])
    outs = torch.empty(steps, B, otok.shape[-1], device=DEV)
    t = 0
    while t < steps:
        flags, inst, source, T, snap, rest = sref.events(t, ring)
        if any(flags):
            for b in range(B):
                if flags[b]:
                    pt[:, b], pm[b] = new_prompts[(b, t)][0][:, 0], new_prompts[(b, t)][1][0]
                    done.append(live[b])
                    live[b] = _Lineage(b, new_prompts[(b, t)])
            pol.restart_samples(torch.tensor(flags), pt, pm)
        if inst:   # the sample re-joins with its own last n steps: its lineage stays, its state is rebuilt by the history pass
            b, n = inst
            assert len(live[b].steps) == n
            pol.restart_samples(torch.tensor([x == b for x in range(B)]), pt, pm, history=_history(live[b], n, otok, omask, atok))
        if source:
            pol.fork_samples(source, pt, pm)
            for b, s in enumerate(source):
                if s != b:
                    done.append(live[b])
                    live[b] = _Lineage(b, live[s].prompt, live[s].steps, own_from=len(live[s].steps), pure=live[s].pure)
        if restores:
            for name, (b, with_prompt) in snap.items():
                (s,) = pol.snapshot_samples([b], pt, pm, with_prompt=with_prompt)
                assert s.steps == len(live[b].steps) and s.has_prompt == with_prompt and s.nbytes == s.payload.numel()
                held[name] = (s, live[b].prompt, list(live[b].steps))
            for name, slots in rest:
                s, prompt, hist = held[name]
                assert s.steps <= pol.history_room()
                rt, rm = pol.restore_samples(slots, [s] * len(slots), pt, pm)
                assert rt is pt and rm is pm, "the prompt tensors are updated in place"
                for d in slots:
                    assert torch.equal(pt[:, d], prompt[0][:, 0]) and torch.equal(pm[d], prompt[1][0]), (t, name, d)
                    done.append(live[d])
                    live[d] = _Lineage(d, prompt, hist, own_from=len(hist), pure=False)
            assert t == 0 or pol.steps_left().tolist() == left_ref[t], (t, pol.steps_left().tolist(), left_ref[t])
        if T == 1:
            o, m, a = otok[t], omask[t], (atok[t - 1] if t > 0 else None)
            if static:
                so.copy_(o); sm.copy_(m)
                if t > 0:
                    sa.copy_(a)
                o, m, a = so, sm, (sa if t > 0 else None)
            outs[t].copy_(pol.forward_step(o.contiguous(), m.contiguous(), a, pt, pm, step=t))
        else:
            outs[t:t + T].copy_(pol.forward_steps(otok[t:t + T].contiguous(), omask[t:t + T].contiguous(), atok[t - 1:t + T - 1].contiguous(), pt, pm, step=t))
        for u in range(t, t + T):
            for b in range(B):
                live[b].steps.append((u, b))
                if live[b].pure:
                    pure_steps.add((b, u))
        t += T
    torch.cuda.synchronize()
    assert pt is pt0 and pm is pm0
    return outs, done + live, pure_steps


# ------------------------------------------------------------------------------------------ 2. same moment
@pytest.mark.parametrize("prec", ["fp32", "bf16", X3])
def test_restored_at_once_a_snapshot_is_a_fork_and_the_identity(prec):
    """A snapshot of b restored at once into d != b: fed b's inputs, d returns b's output bit for bit on the next step -- what fork_samples gives on
    a twin, to the bit. Restored into b itself, the next step equals an untouched twin's bit for bit in every slot."""
    pol, forked, twin = (_policy(prec, decode_ring=1) for _ in range(3))
    otok, omask, atok = _data(pol, 5)
    pts = []
    for p in (pol, forked, twin):
        pt, pm = p.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
        pts.append((pt.clone(), pm.clone()))
        for t in range(3):
            p.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t else None, *pts[-1], step=t)
    (s,) = pol.snapshot_samples([1], *pts[0])
    assert s.steps == 3 and s.has_prompt
    pol.restore_samples([3], [s], *pts[0])
    forked.fork_samples([0, 1, 2, 1], *pts[1])
    assert torch.equal(pts[0][0], pts[1][0]) and torch.equal(pts[0][1], pts[1][1]) and pol.steps_left().tolist() == forked.steps_left().tolist()
    idx = torch.tensor([0, 1, 2, 1], device=DEV)
    o, m, a = otok[3].index_select(0, idx), omask[3].index_select(0, idx), atok[2].index_select(0, idx)
    got, want = pol.forward_step(o, m, a, *pts[0], step=3), forked.forward_step(o, m, a, *pts[1], step=3)
    assert torch.equal(got[3], got[1]), (got[3] - got[1]).abs().max().item()
    assert torch.equal(got, want)
    # into its own slot: nothing changes
    (s2,) = pol.snapshot_samples([2], *pts[0], with_prompt=False)
    pol.restore_samples([2], [s2], *pts[0])
    plain = twin.forward_step(otok[3].contiguous(), omask[3].contiguous(), atok[2], *pts[2], step=3)
    assert torch.equal(got[:3], plain[:3])
    a4, b4 = (p.forward_step(otok[4].contiguous(), omask[4].contiguous(), atok[3], *q, step=4) for p, q in ((pol, pts[0]), (twin, pts[2])))
    assert torch.equal(a4[:3], b4[:3])


# ------------------------------------------------------------------------------------------ 3. later
@pytest.mark.parametrize("hm", [0, 1])
@pytest.mark.parametrize("prec", ["fp32", "bf16", X3])
def test_ring_rollout_with_snapshots_matches_every_lineage_alone(prec, hm):
    pol = _policy(prec, decode_ring=1, kv_headmajor=hm)
    ref_pol = _policy(prec)
    otok, omask, atok = _data(pol)
    outs, lineages, _ = _rollout(pol, otok, omask, atok)               # steps_left equals the restatement in front of every step
    worst, n = _check_lineages(ref_pol, outs, lineages, otok, omask, atok, TOL[prec])
    assert n == STEPS * B
    print(f"[snapshot] ring {prec} kv_headmajor {hm}: {len(lineages)} lineages, {n} (slot, step) outputs, worst error / max(1, |ref|) {worst:.3e} "
          f"(bound {TOL[prec]:.0e}); {len(sref.SNAPSHOTS)} snapshots, {sum(len(s) for _, s in sum(sref.RESTORES.values(), []))} restored slots")


def test_samples_outside_a_restore_keep_their_bits():
    pol, twin = _policy("fp32", decode_ring=1), _policy("fp32", decode_ring=1)
    otok, omask, atok = _data(pol)
    got, _, pure = _rollout(pol, otok, omask, atok)
    want, _, all_pure = _rollout(twin, otok, omask, atok, restores=False)
    assert len(all_pure) == STEPS * B and STEPS * B // 3 < len(pure) < STEPS * B
    for b, t in sorted(pure):
        assert torch.equal(got[t][b], want[t][b]), (b, t)
    bystanders = [(b, t) for t, rs in sref.RESTORES.items() for b in range(B) if all(b not in slots for _, slots in rs) and (b, t) in pure]
    assert len(bystanders) >= 8, bystanders                             # slots no restore wrote, on the step right after one


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_snapshots_on_the_linear_cache(prec):
    pol, ref_pol = _policy(prec, decode_ring=0), _policy(prec)
    otok, omask, atok = _data(pol, sref.LINEAR_STEPS)
    outs, lineages, _ = _rollout(pol, otok, omask, atok, ring=False)
    worst, n = _check_lineages(ref_pol, outs, lineages, otok, omask, atok, TOL[prec])
    assert n == sref.LINEAR_STEPS * B and pol.steps_left().tolist() == [0] * B
    print(f"[snapshot] linear cache {prec}: worst error / max(1, |ref|) {worst:.3e} (bound {TOL[prec]:.0e})")


# ------------------------------------------------------------------------------------------ 4. across handles and through the host
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("dest", ["ring", "other-layout", "linear"])
def test_a_snapshot_travels_through_the_host_into_another_batch(dest, prec, tmp_path):
    """Taken from slot 2 of a B = 4 ring policy after 6 steps; .cpu(), state_dict, torch.save / load, from_state_dict; restored into slot 1 of a
    B = 2 policy that is 11 steps into its own rollout (behind its first wrap), or has the other prompt K/V layout, or a linear cache."""
    src = _policy(prec, decode_ring=1, kv_headmajor=0)
    otok, omask, atok = _data(src, 14)
    pt, pm = src.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    pt, pm = pt.clone(), pm.clone()
    for t in range(6):
        src.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t else None, pt, pm, step=t)
    (snap,) = src.snapshot_samples([2], pt, pm)
    torch.save(snap.cpu().state_dict(), tmp_path / "episode.pt")
    del snap
    back = EpisodeSnapshot.from_state_dict(torch.load(tmp_path / "episode.pt", weights_only=True))
    assert back.device.type == "cpu" and back.steps == 6 and back.has_prompt
    opts = dict(ring=dict(decode_ring=1), linear=dict(decode_ring=0))
    opts["other-layout"] = dict(decode_ring=1, kv_headmajor=1)
    dst = _policy(prec, **opts[dest])
    t0 = 6 if dest == "linear" else 11
    qt, qm = dst.forward_prompt_assembly(syn.to_device(syn.cut_prompt(_prompt(1), [0, 1]), DEV))
    qt, qm = qt.clone(), qm.clone()
    for t in range(t0):
        if dest != "linear" and t == 6:                                 # the ring gives rows back on a restart
            dst.restart_samples(torch.tensor([True, True]), qt, qm)
        dst.forward_step(otok[t, :2].contiguous(), omask[t, :2].contiguous(), atok[t - 1, :2].contiguous() if t else None, qt, qm, step=t)
    assert dst.history_room() >= 6
    dst.restore_samples([1], [back], qt, qm)
    assert torch.equal(qt[:, 1], pt[:, 2]) and torch.equal(qm[1], pm[2])
    outs = []
    for k in range(2):                                                  # slot 1 continues the episode of the source's sample 2: its steps 6 and 7
        o = torch.stack([otok[t0 + k, 0], otok[6 + k, 2]])
        m = torch.stack([omask[t0 + k, 0], omask[6 + k, 2]])
        a = torch.stack([atok[t0 + k - 1, 0], atok[5 + k, 2]])
        outs.append(dst.forward_step(o, m, a, qt, qm, step=t0 + k)[1])
    full = _policy(prec).forward(otok[:8, 2:3].contiguous(), omask[:8, 2:3].contiguous(), atok[:7, 2:3].contiguous(), pt[:, 2:3].contiguous(), pm[2:3])
    worst = 0.0
    for k in range(2):
        ref = full[6 + k, 0]
        err = max_abs(outs[k], ref) / max(1.0, ref.abs().max().item())
        worst = max(worst, err)
        assert torch.isfinite(outs[k]).all() and err <= TOL[prec], (dest, k, err)
    print(f"[snapshot] through the host into B = 2 ({dest}) {prec}: worst error / max(1, |ref|) {worst:.3e} (bound {TOL[prec]:.0e})")


def test_flamingo_snapshot_and_restore():
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
        (s,) = pol.snapshot_samples([1], ptok, pmask)
        pol.forward_step(otok[2], atok[1], ptok, pmask, 2)
        assert s.steps == 2 and not torch.equal(ptok[:, 2], ptok[:, 1])
        pol.restore_samples([2], [s.cpu()], ptok, pmask)                  # one step later, through the host
        assert torch.equal(ptok[:, 2], ptok[:, 1]) and torch.equal(pmask[2], pmask[1])
        out3 = pol.forward_step(otok[3], atok[2], ptok, pmask, 3)
        obs = torch.stack([otok[0, 1], otok[1, 1], otok[3, 2]]).unsqueeze(1).contiguous()
        act = torch.stack([atok[0, 1], atok[2, 2]]).unsqueeze(1).contiguous()
        full = pol.forward(obs, act, *p1)
        assert max_abs(out3[2], full[2, 0]) < 2e-5 * max(1.0, full.abs().max().item())


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_change_nothing():
    donor, donor16 = _policy("fp32", decode_ring=1), _policy("bf16", decode_ring=1)
    pol, twin = _policy("fp32", decode_ring=1), _policy("fp32", decode_ring=1)
    otok, omask, atok = _data(pol, 16)
    pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
    pt, pm = pt.clone(), pm.clone()
    with pytest.raises(_lib.VimaError, match="no running episode"):
        pol.snapshot_samples([0], pt, pm)
    for t in range(4):
        donor.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t else None, pt, pm, step=t)
    donor16.forward_step(otok[0].contiguous(), omask[0].contiguous(), None, pt, pm, step=0)
    (s4,), (s16,) = donor.snapshot_samples([1], pt, pm), donor16.snapshot_samples([1], pt, pm)
    (s1,) = donor.snapshot_samples([1], pt, pm, with_prompt=False)
    with pytest.raises(_lib.VimaError, match="no running episode"):
        pol.restore_samples([0], [s4], pt, pm)
    step = [0]

    def both():
        """one step of pol and twin (every sample restarted in front of every fourth step) -> equal bit for bit"""
        t = step[0]
        outs = []
        for p in (pol, twin):
            if t and t % 4 == 0:
                p.restart_samples(torch.tensor([True] * B), pt, pm)
            outs.append(p.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t else None, pt, pm, step=t))
        step[0] += 1
        assert torch.equal(*outs), t
        assert pol.steps_left().tolist() == twin.steps_left().tolist()

    def fake(**kw):
        return EpisodeSnapshot(s1.payload, dict(s1.info, **kw))

    both()
    keep_t, keep_m, host = pt.clone(), pm.clone(), s1.payload.cpu()
    padded = EpisodeSnapshot(torch.zeros(s1.nbytes + 16, dtype=torch.uint8, device=DEV), dict(s1.info, bytes=s1.nbytes + 16))
    refusals = [
        (IndexError, "does not fit: room for 1", lambda: pol.restore_samples([0], [s4], pt, pm)),          # n = 4 > history_room() = 1
        (ValueError, "precision", lambda: pol.restore_samples([0], [s16], pt, pm)),
        (ValueError, "Q = 2", lambda: pol.restore_samples([0], [fake(Q=2)], pt, pm)),
        (ValueError, r"prompt of \d+ rows", lambda: pol.restore_samples([0], [fake(prompt_len=s1.info["prompt_len"] + 1)], pt, pm)),
        (ValueError, "another policy kind", lambda: pol.restore_samples([0], [fake(policy_kind=3)], pt, pm)),
        (ValueError, "embed_dim", lambda: pol.restore_samples([0], [fake(layers=3)], pt, pm)),
        (ValueError, "not one this library wrote", lambda: pol.restore_samples([0], [padded], pt, pm)),
        (ValueError, "slot 2 is listed twice", lambda: pol.restore_samples([2, 2], [s1, s1], pt, pm)),
        (ValueError, "slot 4 is not a sample", lambda: pol.restore_samples([4], [s1], pt, pm)),
        (ValueError, "sample 4 is not a sample", lambda: pol.snapshot_samples([4], pt, pm)),
        (ValueError, "not device memory", lambda: _lib.check(pol._lib.vima_decode_restore(
            pol._handle, _i32([0]), 1, ctypes.cast(_ptrs([host]), ctypes.c_void_p), ctypes.byref(s1._c_info()), pol._stream()))),
        (_lib.VimaError, "vima_seq_decode_restore", lambda: _lib.check(pol._lib.vima_seq_decode_restore(
            pol._handle, _i32([0]), 1, ctypes.cast(_ptrs([s1.payload]), ctypes.c_void_p), ctypes.byref(s1._c_info()), pol._stream()))),
        (AssertionError, "2 slots but 1 snapshots", lambda: pol.restore_samples([0, 1], [s1], pt, pm)),
    ]
    for exc, match, call in refusals:
        left = pol.steps_left().tolist()
        with pytest.raises(exc, match=match):
            call()
        assert torch.equal(pt, keep_t) and torch.equal(pm, keep_m) and pol.steps_left().tolist() == left, match
        both()                                                           # the next step equals the twin's bit for bit
    assert step[0] == len(refusals) + 1 <= 16


# ------------------------------------------------------------------------------------------ 6. graphs
def test_rollout_with_restores_under_graph_replay_is_exact():
    otok, omask, atok = _data(_policy("bf16"))
    want, _, _ = _rollout(_policy("bf16", decode_ring=1), otok, omask, atok, static=True)
    pol = _policy("bf16", decode_ring=1, graphs=1)
    got, _, _ = _rollout(pol, otok, omask, atok, static=True)
    for t in range(STEPS):
        assert torch.equal(got[t], want[t]), t
    plain = _policy("bf16", decode_ring=1, graphs=1)
    _rollout(plain, otok, omask, atok, static=True, restores=False)
    (replays, captures), (p_replays, p_captures) = pol.graph_stats(), plain.graph_stats()
    print(f"[snapshot] graphs: {captures} captures / {replays} replays with snapshots and restores, {p_captures} / {p_replays} without")
    assert captures == p_captures > 0 and replays == p_replays > 0


# ------------------------------------------------------------------------------------------ 7. launch count
def test_launch_counts_do_not_depend_on_pairs_or_layers():
    """The 4M config has 2 decoder layers itself, so the other layer count is a 4-layer variant of it."""
    counts = {}
    for layers in (CFG.xf_n_layers, 4):
        cfg = dataclasses.replace(CFG, xf_n_layers=layers)
        for samples in ([1], [0, 1, 3]):
            for with_prompt in (True, False):
                pol = _policy("bf16", cfg=cfg, decode_ring=1)
                otok, omask, atok = _data(pol, 2)
                pt, pm = pol.forward_prompt_assembly(syn.to_device(_prompt(0), DEV))
                pt, pm = pt.clone(), pm.clone()
                for t in range(2):
                    pol.forward_step(otok[t].contiguous(), omask[t].contiguous(), atok[t - 1] if t else None, pt, pm, step=t)
                pol.prof_enable(True)
                snaps = pol.snapshot_samples(samples, pt, pm, with_prompt=with_prompt)
                torch.cuda.synchronize()
                n = [sum(v["launches"] for v in pol.prof_read().values())]
                pol.prof_enable(False)
                pol.prof_enable(True)
                pol.restore_samples(samples[::-1], snaps, pt, pm)
                torch.cuda.synchronize()
                n.append(sum(v["launches"] for v in pol.prof_read().values()))
                pol.prof_enable(False)
                counts[(layers, len(samples), with_prompt)] = tuple(n)
    print(f"[snapshot] launches of one (snapshot, restore) call by (layers, pairs, with_prompt): {counts}")
    assert CFG.xf_n_layers == 2 and len(counts) == 8
    assert {v for k, v in counts.items() if k[2]} == {(3, 3)} and {v for k, v in counts.items() if not k[2]} == {(2, 2)}, counts
