"""Incremental decoding of the decoder-only baselines (VIMAGPTPolicy / VIMAGatoPolicy: `seq_prefill` / `seq_step` / `seq_restart`,
C entry points vima_seq_prefill / vima_seq_decode_step / vima_seq_decode_restart) on a real MI355X.

The expected values come from the oracle (`oracle.baseline_oracle`, pinned to the unmodified reference by tests/golden/baseline_*.npz)
run on the FULL history; step t of the incremental path is compared with `predicted[t]`. Gates are those of
tests/test_baselines_gpu.py::_compare: fp32 max_abs < 1e-3 max(1, max|ref|) and max_rel < 2e-4; bf16 max_rel < 4e-2."""
import ctypes
import functools

import pytest
import torch

from oracle.baseline_oracle import build_baseline_oracle
from oracle.cases import BASELINE_CASES, baseline_state_dict, build_baseline_case, run_baseline
from vima_amd import _lib
from vima_amd.baselines import build_baseline
from vima_testing import synthetic as syn
from tests.gpu_common import loaded_policy, max_abs, max_rel, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_RAGGED = BASELINE_CASES["baseline_gato"]["layout"]


def _gate(got, ref, prec, tag):
    got, ref = got.cpu(), ref.cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape), tuple(ref.shape))
    a, r = max_abs(got, ref), max_rel(got, ref)
    print(f"[{tag}] {prec}: max_abs {a:.3e} max_rel {r:.3e} (max|ref| {ref.abs().max().item():.3g})")
    if prec == "fp32":
        assert a < 1e-3 * max(1.0, ref.abs().max().item()), (tag, a)
        assert r < 2e-4, (tag, r)
    else:
        assert r < 4e-2, (tag, r)


# ---- cases: (cfg, state dict, prompts, obs, actions) and the oracle's full-history rows, computed once per case ----------------------
def _case_inputs(name):
    if name in BASELINE_CASES:
        cfg, prompts, obs, actions = build_baseline_case(name)
        return cfg, baseline_state_dict(name, cfg), prompts, obs, actions
    if name == "gato_T3":       # baseline_gato with a third step: the last step's row offset is Lp + 1 + 2 (Q + 1) - 1
        c = BASELINE_CASES["baseline_gato"]
        cfg = build_baseline_case("baseline_gato")[0]
        prompts = syn.make_rgb_prompt(c["batch"], layout=c["layout"], seed=c["iseed"])
        return (cfg, baseline_state_dict("baseline_gato", cfg), prompts, syn.make_rgb_obs(3, c["batch"], seed=c["iseed"] + 100),
                syn.make_actions(2, c["batch"], seed=c["iseed"] + 200))
    kind, E, heads, layers, T = {"gato_768": ("gato", 768, 12, 1, 2), "gato_320": ("gato", 320, 20, 2, 2), "gpt_320": ("gpt", 320, 20, 1, 3),
                                 "gato_T4": ("gato", 256, 8, 2, 4), "gpt_T4": ("gpt", 256, 8, 2, 4)}[name]
    cfg = syn.BaselineConfig(kind, E, layers, heads, vocab_size=16)
    seed = 3100 + sum(map(ord, name))
    return (cfg, syn.make_baseline_state_dict(cfg, seed, head_gain=0.5), syn.make_rgb_prompt(3, layout=_RAGGED, seed=seed + 1),
            syn.make_rgb_obs(T, 3, seed=seed + 2), syn.make_actions(T - 1, 3, seed=seed + 3))


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg, sd, prompts, obs, actions = _case_inputs(name)
    orc = build_baseline_oracle(cfg, sd)
    ref = run_baseline(orc, prompts, obs, actions)["predicted"]
    return cfg, sd, prompts, obs, actions, orc, ref


def _policy(cfg, sd, prec, **opts):
    pol = build_baseline(cfg, precision=prec, device=DEV)
    pol.load_state_dict(sd, strict=True)
    for k, v in opts.items():
        pol.set_option(k, v)
    return pol


def _tokens(pol, prompts, obs, actions):
    with torch.no_grad():
        ptok, pmask = pol.forward_prompt_assembly(syn.to_device(prompts, DEV))
        otok = pol.forward_obs_token(syn.to_device(obs, DEV))
        atok = pol.forward_action_token(syn.to_device(actions, DEV))
    return ptok, pmask, otok, atok


def _episode(pol, ptok, pmask, otok, atok):
    pol.seq_prefill(ptok, pmask)
    return torch.stack([pol.seq_step(otok[t], None if t == 0 else atok[t - 1]) for t in range(otok.shape[0])])


# ---- 1. parity with the oracle / 2. kernel routes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["baseline_gpt", "baseline_gato", "gato_T3",
                                  "gato_768",    # head dim 64
                                  # E = 320: E % 128 != 0 takes the two-launch c_attn append; 20 heads of 16 take the generic attention kernel (the
                                  # library has head dims 16 / 32 / 64 / 128 only: 8 heads of 40 are refused by vima_create, see the bounds test)
                                  "gato_320",
                                  "gpt_320"])
def test_seq_step_matches_oracle_full_history(name, prec):
    """Ragged prompts (nv differs per sample, padding keys sit inside the cache); step t against predicted[t] of the full history."""
    cfg, sd, prompts, obs, actions, _, ref = _case(name)
    pol = _policy(cfg, sd, prec)
    got = _episode(pol, *_tokens(pol, prompts, obs, actions))
    torch.cuda.synchronize()
    for t in range(ref.shape[0]):
        _gate(got[t], ref[t], prec, f"{name} step {t}")


# ---- 3. consistency with the full-history entry point ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["baseline_gpt", "gato_T3", "gato_320"])
def test_seq_step_matches_forward_fp32(name):
    """The same sample through a different route (prefix cached, new rows only) against `forward` on the whole history: 2e-4 absolute,
    the gate of test_baseline_matches_oracle_other_shapes. Observed on MI355X: 0.0 at all three shapes (the two routes agree bit for bit there);
    profiles/seq_step_pytest.txt."""
    cfg, sd, prompts, obs, actions = _case(name)[:5]
    pol = _policy(cfg, sd, "fp32")
    ptok, pmask, otok, atok = _tokens(pol, prompts, obs, actions)
    full = pol.forward(otok, atok, ptok, pmask)
    got = _episode(pol, ptok, pmask, otok, atok)
    torch.cuda.synchronize()
    worst = max(max_abs(got[t], full[t]) for t in range(full.shape[0]))
    print(f"[{name}] seq_step vs forward, fp32: max_abs {worst:.3e} (max|forward| {full.abs().max().item():.3g})")
    assert worst < 2e-4, worst


# ---- 4. restart ---------------------------------------------------------------------------------------------------------------------
def _cut(obs, actions, t0, t1, b):
    o = syn.MapDict(rgb=syn.MapDict({v: obs["rgb"][v][t0:t1, b:b + 1] for v in syn.VIEWS}), ee=obs["ee"][t0:t1, b:b + 1])
    return o, {k: v[t0:t1 - 1, b:b + 1] for k, v in actions.items()}


@functools.lru_cache(maxsize=None)
def _restart_refs(name):
    """Oracle rows of FRESH B = 1 episodes of samples 1 and 2 that begin at env step 2 with new prompts."""
    cfg, sd, prompts, obs, actions, orc, ref = _case(name)
    new = {1: syn.make_rgb_prompt(1, layout=[[0, 1, 0]], seed=77), 2: syn.make_rgb_prompt(1, layout=[[1]], seed=78)}
    refs = {}
    for b, p in new.items():
        o, a = _cut(obs, actions, 2, 4, b)
        refs[b] = run_baseline(orc, p, o, a)["predicted"][:, 0]
    return new, refs


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["gato_T4", "gpt_T4"])
def test_seq_restart_rebuilds_flagged_samples(name, prec):
    cfg, sd, prompts, obs, actions, _, ref = _case(name)
    new, new_ref = _restart_refs(name)
    pol = _policy(cfg, sd, prec)
    ptok, pmask, otok, atok = _tokens(pol, prompts, obs, actions)
    Lp, E = ptok.shape[0], cfg.embed_dim
    ptok, pmask = ptok.contiguous(), pmask.clone()
    launches = {}
    for flagged in ([1], [1, 2]):
        ptok2, pmask2 = ptok.clone(), pmask.clone()
        for b in flagged:     # the new prompt, padded to the episode's Lp
            nt, nm = pol.forward_prompt_assembly(syn.to_device(new[b], DEV))
            assert nt.shape[0] < Lp
            ptok2[:, b] = 0
            ptok2[:nt.shape[0], b] = nt[:, 0]
            pmask2[b] = False
            pmask2[b, :nt.shape[0]] = nm[0]
        flags = torch.tensor([b in flagged for b in range(3)])
        pol.seq_prefill(ptok, pmask)
        got = [pol.seq_step(otok[0]), pol.seq_step(otok[1], atok[0])]
        pol.prof_enable(True)
        pol.seq_restart(flags, ptok2, pmask2)
        launches[len(flagged)] = sum(v["launches"] for v in pol.prof_read().values())
        pol.prof_enable(False)
        a1 = atok[1].clone()
        a1[flagged] = 100.0      # finite garbage in the action rows of the restarted samples: must not be read
        got += [pol.seq_step(otok[2], a1), pol.seq_step(otok[3], atok[2])]
        torch.cuda.synchronize()
        for b in range(3):
            for t in range(4):
                want = new_ref[b][t - 2] if (b in flagged and t >= 2) else ref[t, b]
                _gate(got[t][b], want, prec, f"{name} restart {flagged} sample {b} step {t}")
    print(f"[{name}] launches of seq_restart: {launches}")
    assert launches[1] == launches[2] and launches[1] > 0, launches


# ---- 5. bounds and state (host-side argument checks only) ---------------------------------------------------------------------------
def test_seq_step_bounds_and_state():
    cfg = syn.BaselineConfig("gato", 256, 1, 8, vocab_size=8, n_positions=64)
    pol = _policy(cfg, syn.make_baseline_state_dict(cfg, 5), "bf16")
    g = torch.Generator().manual_seed(9)
    B, Lp, Q, E, N = 3, 18, 16, 256, 64
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    pmask[0, 17:] = False
    obs = torch.randn(B, Q, E, generator=g).to(DEV)
    act = torch.randn(B, E, generator=g).to(DEV)
    with pytest.raises(_lib.VimaError):
        pol.seq_step(obs)                                   # no prefill
    for rep in range(2):                                    # the second pass: the same calls succeed again after a new prefill
        pol.seq_prefill(ptok, pmask)
        used = Lp + 1
        assert pol.steps_left().tolist() == [(N - used + 1) // (Q + 1)] * B == [2] * B
        pol.seq_step(obs)
        used += Q
        assert pol.steps_left().tolist() == [(N - used) // (Q + 1)] * B == [1] * B
        with pytest.raises(_lib.VimaError):
            pol.seq_step(obs[:2], act[:2])                  # wrong B: refused, nothing changes
        pol.seq_step(obs, act)
        used += Q + 1
        assert pol.steps_left().tolist() == [(N - used) // (Q + 1)] * B == [0] * B
        with pytest.raises(IndexError, match="n_positions"):
            pol.seq_step(obs, act)                          # 52 + 17 > 64
        assert pol.steps_left().tolist() == [0] * B
    with pytest.raises(IndexError):                         # a sample without a valid prompt token, like forward
        m0 = pmask.clone()
        m0[1] = False
        pol.seq_prefill(ptok, m0)
    with pytest.raises(IndexError, match="n_positions"):    # prompt + separator longer than the table
        pol.seq_prefill(torch.zeros(64, B, E, device=DEV), torch.ones(B, 64, dtype=torch.bool, device=DEV))
    # the step number is checked by the C entry point, too
    lib = _lib.load()
    pol.seq_prefill(ptok, pmask)
    out = torch.empty(B, E, device=DEV)
    assert lib.vima_seq_decode_step(pol._handle, ptr(obs), ptr(act), 1, B, ptr(out), None) != 0
    assert b"does not continue the episode state" in lib.vima_last_error()
    # decode_ring is not part of this path
    pol.set_option("decode_ring", 1)
    with pytest.raises(_lib.VimaError, match="decode_ring"):
        pol.seq_prefill(ptok, pmask)
    with pytest.raises(_lib.VimaError, match="decode_ring"):
        pol.seq_step(obs)
    with pytest.raises(_lib.VimaError, match="decode_ring"):
        pol.seq_restart([True, False, False], ptok, pmask)
    pol.set_option("decode_ring", 0)
    with pytest.raises(_lib.VimaError):
        pol.seq_step(obs)                                   # the option change ended the episode
    # E = 320 with 8 heads (head dim 40) is no configuration of this library: the generic-attention route is tested at 20 heads of 16
    with pytest.raises(_lib.VimaError, match="head dim"):
        build_baseline(syn.BaselineConfig("gato", 320, 1, 8, vocab_size=8), device=DEV)._ensure_handle()
    # other policy kinds are refused by the mirror and by the C entry points
    fcfg = syn.BaselineConfig("flamingo", 256, 1, 8, xattn_n_heads=8)
    fl = _policy(fcfg, syn.make_baseline_state_dict(fcfg, 6), "bf16")
    with pytest.raises(NotImplementedError):
        fl.seq_prefill(ptok, pmask)
    with pytest.raises(NotImplementedError):
        fl.seq_step(obs)
    vcfg = syn.config("2M")
    vp = loaded_policy(vcfg, syn.make_state_dict(vcfg, 0), "bf16")
    assert not hasattr(vp, "seq_prefill")
    pm8 = pmask.to(torch.uint8)
    for h in (fl._handle, vp._handle):
        assert lib.vima_seq_prefill(h, ptr(ptok), ptok.stride(1), ptok.stride(0), ptr(pm8), B, Lp, None) != 0
        assert lib.vima_seq_decode_step(h, ptr(obs), None, 0, B, ptr(out), None) != 0
        flags = (ctypes.c_uint8 * B)(1, 0, 0)
        assert lib.vima_seq_decode_restart(h, flags, B, ptr(ptok), ptok.stride(1), ptok.stride(0), ptr(pm8), Lp, None) != 0
    torch.cuda.synchronize()


# ---- 6. graph replay ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_seq_step_graph_replay_is_exact(prec):
    cfg = syn.BaselineConfig("gato", 256, 2, 8, vocab_size=8)
    sd = syn.make_baseline_state_dict(cfg, 11)
    g = torch.Generator().manual_seed(12)
    B, Lp, Q, E, T = 3, 21, 16, 256, 3
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    pmask[1, 9:] = False
    otok = torch.randn(T, B, Q, E, generator=g).to(DEV)
    atok = torch.randn(T - 1, B, E, generator=g).to(DEV)

    def loop(pol):
        outs = []
        for rep in range(3):      # eager, capture, replay of every step
            pol.seq_prefill(ptok, pmask)
            for t in range(T):
                outs.append(pol.seq_step(otok[t], None if t == 0 else atok[t - 1]).clone())
        torch.cuda.synchronize()
        return outs

    eager = loop(_policy(cfg, sd, prec))
    polg = _policy(cfg, sd, prec, graphs=1)
    graphed = loop(polg)
    replays, captures = polg.graph_stats()
    print(f"[graphs] {prec}: replays {replays}, captures {captures}")
    assert captures > 0 and replays > 0, (replays, captures)
    for t in range(T):
        assert torch.equal(eager[t], eager[T + t]) and torch.equal(eager[t], eager[2 * T + t])
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)
