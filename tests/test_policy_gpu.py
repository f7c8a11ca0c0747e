"""End-to-end parity of the HIP policy path (through the C ABI and the VIMAPolicy host mirror) on a real MI355X:
  * against the committed golden fixtures that the UNMODIFIED reference produced (tests/golden/, oracle/make_golden.py),
  * against the oracle on the same seeded inputs,
  * at BASELINE.json's full VIMA-200M shapes through size-independent properties.
Tolerances: north_star asks for action logits within 1e-3 (fp32). fp32-operand mode meets 1e-3 on EVERY tensor
(in fact ~1e-5); bf16-operand mode is gated on the logits (abs 1e-3) and on a relative bound for O(1) tokens."""
import os

import numpy as np
import pytest
import torch

from oracle.cases import CASES, SMALL_CASES, BENCH_CASES, build_case, run_policy, case_state_dict, gold_view
from oracle.vima_oracle import OraclePolicy, ACTION_KEYS
from vima_testing import synthetic as syn
from tests.gpu_common import loaded_policy, max_abs, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def native_outputs(pol, prompts, obs, actions):
    out, d = run_policy(pol, syn.to_device(prompts, DEV), syn.to_device(obs, DEV),
                        syn.to_device(actions, DEV) if actions is not None else None)
    out["raw_logits"] = torch.cat([d[k].raw_logits for k in ACTION_KEYS], dim=-1)
    out["norm_logits"] = torch.cat([torch.cat([c.logits for c in d[k]._dists], dim=-1) for k in ACTION_KEYS], dim=-1)
    out["modes"] = torch.cat([d[k].mode() for k in ACTION_KEYS], dim=-1)
    out["mode_action_tokens"] = pol.forward_action_token({k: d[k].mode() for k in ACTION_KEYS})
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(SMALL_CASES))
@pytest.mark.parametrize("prec,attn_impl,gemm_variant", [("fp32", 0, 1), ("fp32", 0, 0), ("bf16", 1, 1), ("bf16", 0, 0)])
def test_matches_reference_golden(name, prec, attn_impl, gemm_variant, golden_dir):
    gold = np.load(os.path.join(golden_dir, f"{name}.npz"))
    cfg, wseed, prompts, obs, actions = build_case(name)
    sd = syn.make_state_dict(cfg, wseed)
    pol = loaded_policy(cfg, sd, prec, attn_impl=attn_impl, gemm_variant=gemm_variant)
    out = native_outputs(pol, prompts, obs, actions)
    for k in gold.files:
        if k.startswith("_"):
            continue
        ref = torch.from_numpy(gold[k])
        got = out[k].cpu()
        assert tuple(got.shape) == tuple(ref.shape), k
        if ref.dtype == torch.bool:
            assert torch.equal(got, ref), k
        elif ref.dtype == torch.int64:
            if prec == "fp32":
                assert torch.equal(got, ref), k           # argmax of the action distributions
        elif prec == "fp32":
            assert max_abs(got, ref) < 1e-3, (k, max_abs(got, ref))
            assert max_rel(got, ref) < 2e-4, (k, max_rel(got, ref))
        elif k == "raw_logits":
            assert max_abs(got, ref) < 1e-3, (k, max_abs(got, ref))   # the north_star gate
        elif k != "mode_action_tokens":                    # modes may legitimately flip on near-ties in bf16
            assert max_rel(got, ref) < 4e-2, (k, max_rel(got, ref))


def _flip_report(got_logits, ref_logits):
    """Per-dimension argmax agreement of two [R,700] logit tensors over the 12 categorical heads; for every disagreement
    returns how far (in the REFERENCE's logits) the chosen bin is below the reference's best bin."""
    agree, total, worst_gap = 0, 0, 0.0
    off = 0
    for k in ACTION_KEYS:
        for bins in syn.ACTION_DIMS[k]:
            g, r = got_logits[:, off:off + bins], ref_logits[:, off:off + bins]
            ga, ra = g.argmax(-1), r.argmax(-1)
            agree += int((ga == ra).sum())
            total += ga.numel()
            gap = (r.gather(1, ra[:, None]) - r.gather(1, ga[:, None])).max().item()
            worst_gap = max(worst_gap, gap)
            off += bins
    return agree, total, worst_gap


@pytest.mark.parametrize("name", list(BENCH_CASES))
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_benchmarked_configs_match_reference_golden(name, prec, golden_dir):
    """the BENCHMARKED configurations themselves against outputs of the unmodified reference --
    VIMA-200M / xattn_n_positions=512 / Lp=512 / Q=8 on samples cut from bench.py's own batch (`bench_200M`), the same with
    O(1) logits (`bench_200M_o1`), BASELINE configs[1] (20M, B=32, Lp=256, Q=4) and the 1024-token prompt of configs[4].
    Every stage tensor is compared. fp32-operand mode: 1e-3 abs / 2e-4 rel on everything, modes exact.
    bf16 mode: raw logits within 1e-3 abs where the logits are O(0.06) (north_star gate); for the O(1)-logit case within
    2 % of max|logit|, argmax agreement >= 90 %, and every disagreement is a near-tie of the reference (gap below twice
    the measured logit error)."""
    gold = np.load(os.path.join(golden_dir, f"{name}.npz"))
    cfg, wseed, prompts, obs, actions = build_case(name)
    sd = case_state_dict(name, cfg)
    pol = loaded_policy(cfg, sd, prec)
    out = native_outputs(pol, prompts, obs, actions)
    o1 = CASES[name].get("head_gain", 0.01) > 0.1
    for k in gold.files:
        if k.startswith("_"):
            continue
        ref = torch.from_numpy(gold[k])
        got = gold_view(name, k, out[k].cpu())
        assert tuple(got.shape) == tuple(ref.shape), k
        if ref.dtype == torch.bool:
            assert torch.equal(got, ref), k
        elif ref.dtype == torch.int64:
            if prec == "fp32":
                assert torch.equal(got, ref), k
        elif prec == "fp32":
            assert max_abs(got, ref) < 1e-3, (k, max_abs(got, ref))
            assert max_rel(got, ref) < 2e-4, (k, max_rel(got, ref))
        elif k == "raw_logits" and not o1:
            assert max_abs(got, ref) < 1e-3, (k, max_abs(got, ref))   # the north_star gate
        elif k != "mode_action_tokens":
            assert max_rel(got, ref) < (2e-2 if k in ("raw_logits", "norm_logits") else 4e-2), (k, max_rel(got, ref))
    got_l, ref_l = out["raw_logits"].cpu().reshape(-1, 700), torch.from_numpy(gold["raw_logits"]).reshape(-1, 700)
    agree, total, gap = _flip_report(got_l, ref_l)
    err = max_abs(got_l, ref_l)
    print(f"[parity] {name} {prec}: max|logit err| {err:.3e} (max|logit| {ref_l.abs().max():.3g}), "
          f"argmax agreement {agree}/{total}, worst reference gap at a disagreement {gap:.3e}")
    assert gap <= 2 * err + 1e-7, "an argmax flip that is not a near-tie of the reference"
    if prec == "fp32":
        assert agree == total
    elif o1:
        assert agree >= 0.9 * total, (agree, total)


def test_bf16_argmax_agreement_o1_logits_live_oracle():
    """Larger sample for the argmax statistic: 32 samples cut from the bench batch, O(1) logits, bf16 path vs the oracle
    run live on the host (about 5 s of CPU). Reported and gated like the golden case."""
    name = "bench_200M_o1"
    c = dict(CASES[name])
    cfg = syn.config(c["model"], xattn_n_positions=c["npos"])
    sd = case_state_dict(name, cfg)
    idx = list(range(8, 40))
    prompts = syn.cut_prompt(syn.make_prompt(256, n_segments=32, words_per_segment=8, q_per_view=4, seed=1236), idx)
    obs = syn.cut_obs(syn.make_obs(1, 256, 4, seed=1336), idx)
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    _, od = run_policy(orc, prompts, obs, None)
    ref_l = torch.cat([od[k]["raw"] for k in ACTION_KEYS], dim=-1).reshape(-1, 700)
    pol = loaded_policy(cfg, sd, "bf16")
    got_l = native_outputs(pol, prompts, obs, None)["raw_logits"].cpu().reshape(-1, 700)
    agree, total, gap = _flip_report(got_l, ref_l)
    err = max_abs(got_l, ref_l)
    print(f"[parity] bf16 vs live oracle, 32 samples, O(1) logits: max err {err:.3e} of max|logit| {ref_l.abs().max():.3g}; "
          f"argmax agreement {agree}/{total} = {agree / total:.3f}; worst gap at a flip {gap:.3e}")
    assert err < 2e-2 * ref_l.abs().max().item()
    assert gap <= 2 * err + 1e-7
    assert agree >= 0.9 * total



@pytest.mark.parametrize("opts", [{"gemm_skinny": 0}, {"gemm_small": 0}, {"gemm_persist": 0}, {"gemm_splitk": 1}, {"t5_fuse_rms": 0}, {"stream_T": 0}, {"attn_qg": 2}, {"gemm_wide": 1}, {"gemm_pp": 0}, {"graphs": 1}, {"gemm_resident": 0},
                                  {"dual_stream": 0}, {"attn_split": 0}, {"gemm_epi": 0}, {"vit_prune_last": 0}, {"ln_fuse": 0}])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_every_option_matches_reference_golden(opts, prec, golden_dir):
    """Each alternative code path (tile choice, one-tile-per-workgroup GEMM, split-K, unfused RMSNorm, graph replay, single
    stream, one-wave cross attention, direct epilogue, full last ViT block) against the reference's golden outputs."""
    name = "e384_long"
    gold = np.load(os.path.join(golden_dir, f"{name}.npz"))
    cfg, wseed, prompts, obs, actions = build_case(name)
    sd = syn.make_state_dict(cfg, wseed)
    pol = loaded_policy(cfg, sd, prec, **opts)
    try:
        for _ in range(3 if "graphs" in opts else 1):          # eager, capture, replay
            out = native_outputs(pol, prompts, obs, actions)
        ref = torch.from_numpy(gold["raw_logits"])
        assert max_abs(out["raw_logits"].cpu(), ref) < 1e-3, (opts, max_abs(out["raw_logits"].cpu(), ref))
        tok = torch.from_numpy(gold["prompt_tokens"])
        assert max_rel(out["prompt_tokens"].cpu(), tok) < (2e-4 if prec == "fp32" else 4e-2)
    finally:
        for k in opts:                                         # (options are per handle; restoring is belt and braces)
            pol.set_option(k, {"gemm_small": 1, "gemm_persist": 1, "gemm_splitk": 0, "t5_fuse_rms": 1, "stream_T": 1, "attn_qg": 1, "gemm_wide": 0, "gemm_pp": 1, "graphs": 0, "dual_stream": 1, "gemm_resident": 1,
                               "attn_split": 1, "gemm_epi": 1, "vit_prune_last": 1, "ln_fuse": 1, "gemm_skinny": 1}[k])


def test_stagewise_against_oracle_fp32():
    """Each native stage fed with the ORACLE's inputs for that stage (isolates stages from each other)."""
    cfg, wseed, prompts, obs, actions = build_case("ragged_4M")
    sd = syn.make_state_dict(cfg, wseed)
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    o, od = run_policy(orc, prompts, obs, actions)
    pol = loaded_policy(cfg, sd, "fp32", attn_impl=0)
    pred = pol.forward(o["obs_tokens"].to(DEV), o["obs_masks"].to(DEV), o["action_tokens"].to(DEV),
                       o["prompt_tokens"].to(DEV), o["prompt_masks"].to(DEV))
    assert max_abs(pred, o["predicted"]) < 2e-4
    logits = pol.action_logits(o["predicted"].to(DEV))
    assert max_abs(logits, orc.action_logits(o["predicted"])) < 1e-5
    feats = pol.obj_encoder(syn.to_device(prompts[2]["cropped_img"], DEV), syn.to_device(prompts[2]["bbox"], DEV))
    assert max_abs(feats, orc.obj_encoder(prompts[2]["cropped_img"], prompts[2]["bbox"])) < 2e-4


def test_invariances_fp32():
    """Self-consistency properties the domain offers: batch-permutation equivariance, invariance to the
    CONTENT of masked prompt tokens, causality of the history."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 3)
    pol = loaded_policy(cfg, sd, "fp32", attn_impl=0)
    g = torch.Generator().manual_seed(0)
    B, Lp, Q, T, E = 4, 24, 4, 3, cfg.embed_dim
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool)
    pmask[:, 18:] = False
    otok = torch.randn(T, B, Q, E, generator=g).to(DEV)
    omask = torch.ones(T, B, Q, dtype=torch.bool)
    omask[1, :, 2] = False
    atok = torch.randn(T - 1, B, E, generator=g).to(DEV)
    base = pol.forward(otok, omask.to(DEV), atok, ptok, pmask.to(DEV))
    perm = torch.tensor([2, 0, 3, 1])
    permuted = pol.forward(otok[:, perm], omask[:, perm].to(DEV), atok[:, perm], ptok[:, perm], pmask[perm].to(DEV))
    assert max_abs(permuted, base[:, perm]) < 1e-5
    ptok2 = ptok.clone()
    ptok2[18:] = 123.0                                        # masked prompt content must not matter
    assert max_abs(pol.forward(otok, omask.to(DEV), atok, ptok2, pmask.to(DEV)), base) < 1e-5
    shorter = pol.forward(otok[:2], omask[:2].to(DEV), atok[:1], ptok, pmask.to(DEV))   # causal: step t ignores t' > t
    assert max_abs(shorter, base[:2]) < 1e-5


def test_dual_stream_and_pruning_are_exact():
    """The two-stream software pipelining (batch halves / ViT chunks / prompt K/V on an auxiliary stream) and the
    cls-only last ViT block only reorder or skip never-read work: results must be bit-identical to the plain path."""
    cfg, wseed, prompts, obs, actions = build_case("e384_long")
    sd = syn.make_state_dict(cfg, wseed)
    outs = []
    for dual, prune, chunk in [(0, 0, 16384), (1, 1, 16384), (1, 0, 7), (0, 1, 5)]:
        # (gemm_skinny = 0: chunks of 5 / 7 crops put the cls-row GEMMs of a chunk below 33 rows, where the K-split kernel sums in another order than
        # the tiles the 16384-crop chunk takes; chunking invariance at the bit level is a property of the tiles)
        pol = loaded_policy(cfg, sd, "bf16", dual_stream=dual, vit_prune_last=prune, vit_chunk=chunk, gemm_skinny=0)
        for _ in range(2):   # second pass exercises the steady-state (consolidated) workspace
            o = native_outputs(pol, prompts, obs, actions)
        outs.append(o)
    for o in outs[1:]:
        for k in ("prompt_tokens", "obs_tokens", "predicted", "raw_logits"):
            assert torch.equal(o[k], outs[0][k]), k


@pytest.mark.parametrize("name", ["e384_long", "ragged_4M"])
def test_resident_gemm_kernel_is_exact_in_the_policy(name):
    """gemm_resident_kernel takes the underfilled GEMM grids of a small-batch step (decoder, action head, T5 / ViT at batch <= 4,
    incl. the fused-RMSNorm producers / consumers and the K/V-cache appends of incremental decoding); it accumulates K in the
    ring tiles' order, so every output of the policy must be BIT-identical with and without it -- also with a grid limit that
    sends the mid-size problems to it."""
    cfg, wseed, prompts, obs, actions = build_case(name)
    sd = syn.make_state_dict(cfg, wseed)
    outs = []
    for res, maxwg in ((0, 256), (1, 256), (1, 4096), (1, 8)):
        # (ln_fuse = 0: the folded LayerNorm of XAttention's feed-forward exists in the resident kernel's pair form only, so switching that kernel
        # off would also switch the fold off -- a different rounding point, tested in test_ln_fuse_*; THIS test is about the kernel's K order)
        pol = loaded_policy(cfg, sd, "bf16", gemm_resident=res, gemm_res_maxwg=maxwg, ln_fuse=0, gemm_skinny=0)
        for _ in range(2):
            o = native_outputs(pol, prompts, obs, actions)
        outs.append(o)
    for o in outs[1:]:
        for k in ("prompt_tokens", "obs_tokens", "predicted", "raw_logits"):
            assert torch.equal(o[k], outs[0][k]), (k, (o[k].float() - outs[0][k].float()).abs().max().item())


def test_t5_fused_rmsnorm_matches_unfused():
    """T5 RMSNorms folded into the neighbouring GEMMs (weight in W, statistics from the producer's epilogue, row scale in
    the consumer's) against the standalone RMSNorm kernel path: same maths, different rounding points. The fused path is
    used from 8192 rows per stream (smaller problems split their GEMMs along K instead), so the stack is run on
    [64, 256, 768]. fp32 operands agree to ~1e-5; bf16 operands within the usual bf16 bounds; the fused path is
    deterministic (no atomics)."""
    cfg = syn.config("2M")
    sd = syn.make_state_dict(cfg, 13)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(64, 256, 768, generator=g)
    mask = torch.ones(64, 256, dtype=torch.bool)
    mask[3, 200:] = False
    for prec, tol in (("fp32", 5e-5), ("bf16", 4e-2)):
        outs = {}
        for fuse in (0, 1):
            pol = loaded_policy(cfg, sd, prec, t5_fuse_rms=fuse)
            outs[fuse] = pol.t5_encode(x, mask)
            if fuse:
                assert torch.equal(pol.t5_encode(x, mask), outs[1]), prec
        assert max_rel(outs[1], outs[0]) < tol, (prec, max_rel(outs[1], outs[0]))


def test_prompt_kv_cache_is_exact_and_invalidates():
    """Cross-step caching of the per-layer prompt K/V: passing the same prompt tensor again reuses
    the cache and must give bit-identical tokens; an in-place edit of the prompt (version counter) or a new tensor
    invalidates it; a stateless policy (cache off) agrees bit for bit."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 5)
    pol = loaded_policy(cfg, sd, "bf16")
    ref = loaded_policy(cfg, sd, "bf16")
    ref.cache_prompt_kv = False
    g = torch.Generator().manual_seed(1)
    B, Lp, Q, E = 3, 40, 4, cfg.embed_dim
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    steps = []
    for T in (1, 2, 3):                                    # a growing history like the eval loop (example.py:135-190)
        otok = torch.randn(T, B, Q, E, generator=g).to(DEV)
        omask = torch.ones(T, B, Q, dtype=torch.bool, device=DEV)
        atok = torch.randn(T - 1, B, E, generator=g).to(DEV) if T > 1 else None
        a = pol.forward(otok, omask, atok, ptok, pmask)    # T=1 builds the cache, T=2,3 reuse it
        b = ref.forward(otok, omask, atok, ptok, pmask)
        assert torch.equal(a, b), T
        steps.append((otok, omask, atok, a))
    otok, omask, atok, last = steps[-1]
    ptok.mul_(1.5)                                         # in-place edit -> stale cache must not be used
    a = pol.forward(otok, omask, atok, ptok, pmask)
    assert torch.equal(a, ref.forward(otok, omask, atok, ptok, pmask))
    assert not torch.equal(a, last)
    ptok2 = ptok.clone()                                   # different storage, same values -> rebuilt, same result
    assert torch.equal(pol.forward(otok, omask, atok, ptok2, pmask), a)


@pytest.mark.parametrize("prec,cfgname,T", [("fp32", "4M", 4), ("bf16", "4M", 4), ("bf16", "20M", 9)])
def test_incremental_decoding_matches_full_history(prec, cfgname, T):
    """env-step-by-env-step decoding against the episode caches (vima_decode_step) reproduces the
    reference-style forward over the re-fed history, including masked observation tokens (position ids skip them) and
    a padded prompt. T = 9 reaches 80 cached keys (split-key MFMA kernel with a causal offset)."""
    cfg = syn.config(cfgname)
    sd = syn.make_state_dict(cfg, 11)
    pol = loaded_policy(cfg, sd, prec)
    g = torch.Generator().manual_seed(5)
    B, Lp, Q, E = 3, 24, 8, cfg.embed_dim
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool)
    pmask[1, 17:] = False
    otok = torch.randn(T, B, Q, E, generator=g).to(DEV)
    omask = torch.rand(T, B, Q, generator=g) > 0.25
    omask[:, :, 0] = True
    atok = torch.randn(T - 1, B, E, generator=g).to(DEV)
    full = pol.forward(otok, omask.to(DEV), atok, ptok, pmask.to(DEV))
    tol = 2e-5 if prec == "fp32" else 4e-2
    for rep in range(2):                                       # a second episode reuses the allocated state
        for t in range(T):
            step = pol.forward_step(otok[t], omask[t], atok[t - 1] if t > 0 else None, ptok, pmask, t)
            assert step.shape == (B, E)
            assert max_rel(step, full[t]) < tol, (prec, t, max_rel(step, full[t]))
    with pytest.raises(RuntimeError):                          # step 5 does not follow the last completed step
        pol.forward_step(otok[0], omask[0], atok[0], ptok, pmask, T + 3)
    # the history-re-feeding path still works afterwards (and rebuilds its prompt cache)
    assert max_rel(pol.forward(otok, omask.to(DEV), atok, ptok, pmask.to(DEV)), full) < 1e-6


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_incremental_decoding_with_64_object_tokens(prec):
    """Q = 64: a step of 64 / 65 rows, the smallest size beyond the 64 rows a step's embedding once held (a step is a chunk of one:
    dec_embed_chunk_kernel, up to 512 rows). Every step against the re-fed history, random object masks with the first token valid;
    forward_steps with one step is forward_step, bit for bit, on a twin policy."""
    cfg = syn.config("2M")
    sd = syn.make_state_dict(cfg, 11)
    pol, twin = loaded_policy(cfg, sd, prec), loaded_policy(cfg, sd, prec)
    g = torch.Generator().manual_seed(6)
    B, Lp, Q, E, T = 2, 8, 64, cfg.embed_dim, 3
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool)
    pmask[1, 5:] = False
    otok = torch.randn(T, B, Q, E, generator=g).to(DEV)
    omask = torch.rand(T, B, Q, generator=g) > 0.25
    omask[:, :, 0] = True
    atok = torch.randn(T - 1, B, E, generator=g).to(DEV)
    full = pol.forward(otok, omask.to(DEV), atok, ptok, pmask.to(DEV))
    tol = 2e-5 if prec == "fp32" else 4e-2
    for t in range(T):
        step = pol.forward_step(otok[t], omask[t], atok[t - 1] if t > 0 else None, ptok, pmask, t)
        assert step.shape == (B, E) and torch.isfinite(step).all()
        assert max_rel(step, full[t]) < tol, (prec, t, max_rel(step, full[t]))
        one = twin.forward_steps(otok[t:t + 1], omask[t:t + 1], atok[t - 1:t] if t > 0 else None, ptok, pmask, t)
        assert one.shape == (1, B, E) and torch.equal(one[0], step)


def test_incremental_decoding_full_size_200m():
    """VIMA-200M, batch 64, 512-token prompt, T = 3: the episode-cache path against the re-fed history at the
    benchmark's model size (persistent / 128x128 / 64x64 GEMM tiles and the split-key attention kernel all take part)."""
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    pol = loaded_policy(cfg, sd, "bf16")
    g = torch.Generator().manual_seed(8)
    B, Lp, Q, E, T = 64, 512, 8, cfg.embed_dim, 3
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    pmask[5, 400:] = False
    otok = torch.randn(T, B, Q, E, generator=g).to(DEV)
    omask = torch.ones(T, B, Q, dtype=torch.bool, device=DEV)
    omask[1, :, 3] = False
    atok = torch.randn(T - 1, B, E, generator=g).to(DEV)
    full = pol.forward(otok, omask, atok, ptok, pmask)
    for t in range(T):
        step = pol.forward_step(otok[t], omask[t], atok[t - 1] if t > 0 else None, ptok, pmask, t)
        assert torch.isfinite(step).all()
        assert max_rel(step, full[t]) < 4e-2, (t, max_rel(step, full[t]))
        assert max_abs(pol.action_logits(step), pol.action_logits(full[t])) < 1e-3


@pytest.mark.parametrize("heads", [16, 2])
def test_other_head_counts_against_oracle(heads):
    """embed_dim 256 with 16 heads (head dim 16) and 2 heads (head dim 128): the head counts are free parameters of
    the checkpoint config; these sizes take the exact generic attention kernel in both precisions."""
    cfg = syn.PolicyConfig(256, 2, heads, heads)
    sd = syn.make_state_dict(cfg, 21)
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    g = torch.Generator().manual_seed(heads)
    B, Lp, Q, T, E = 2, 20, 4, 2, cfg.embed_dim
    ptok = torch.randn(Lp, B, E, generator=g)
    pmask = torch.ones(B, Lp, dtype=torch.bool)
    pmask[1, 15:] = False
    otok = torch.randn(T, B, Q, E, generator=g)
    omask = torch.ones(T, B, Q, dtype=torch.bool)
    atok = torch.randn(T - 1, B, E, generator=g)
    ref = orc.forward(otok, omask, atok, ptok, pmask)
    for prec, tol in (("fp32", 2e-5), ("bf16", 4e-2)):
        pol = loaded_policy(cfg, sd, prec)
        got = pol.forward(otok.to(DEV), omask.to(DEV), atok.to(DEV), ptok.to(DEV), pmask.to(DEV))
        assert max_rel(got, ref) < tol, (prec, max_rel(got, ref))


def test_embed_dim_1024_identity_action_post_layer():
    """embed_dim == 1024: the reference's ActionEmbedding._post_layer is nn.Identity (action_embd.py:16-20), the key is
    absent from the state dict and the concatenated 4 x 256 embedding is the token. Whole policy against the oracle."""
    cfg = syn.PolicyConfig(1024, 1, 16, 16)
    sd = syn.make_state_dict(cfg, 4)
    assert "action_encoder._post_layer.weight" not in sd
    prompts = syn.make_prompt(2, layout=[[0, 1, 0], [1, 0, 0, 0]], q_per_view=2, seed=31)
    obs = syn.make_obs(2, 2, 2, seed=32)
    actions = syn.make_actions(1, 2, seed=33)
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    o, od = run_policy(orc, prompts, obs, actions)
    ref_logits = torch.cat([od[k]["raw"] for k in ACTION_KEYS], dim=-1)
    for prec, tol_tok, tol_logit in (("fp32", 2e-4, 2e-5), ("bf16", 4e-2, 1e-3)):
        pol = loaded_policy(cfg, sd, prec)
        out = native_outputs(pol, prompts, obs, actions)
        assert max_rel(out["action_tokens"], o["action_tokens"]) < tol_tok, prec
        assert max_rel(out["predicted"], o["predicted"]) < tol_tok, prec
        assert max_abs(out["raw_logits"], ref_logits) < tol_logit, prec


def test_options_are_per_handle():
    """Kernel-selection options live in the handle (VERDICT r1 weak item 10 / ADVICE): changing them on one policy must
    not change what another policy in the same process launches, nor invalidate its captured graphs."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 7)
    g = torch.Generator().manual_seed(3)
    B, Lp, Q, E = 2, 24, 8, cfg.embed_dim
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    otok = torch.randn(1, B, Q, E, generator=g).to(DEV)
    omask = torch.ones(1, B, Q, dtype=torch.bool, device=DEV)
    a = loaded_policy(cfg, sd, "fp32", graphs=1)
    b = loaded_policy(cfg, sd, "fp32")
    b.forward(otok, omask, None, ptok, pmask)
    base = [a.forward(otok, omask, None, ptok, pmask).clone() for _ in range(5)]   # eager (cache build), eager, capture, replay, replay
    r0, c0 = a.graph_stats()
    assert c0 >= 1 and r0 >= 1
    for k, v in dict(attn_impl=0, gemm_tile=1, gemm_variant=0, gemm_epi=0, attn_split=0, gemm_splitk=1).items():
        b.set_option(k, v)                                   # options of B change AFTER A captured its graph
    other = b.forward(otok, omask, None, ptok, pmask).clone()
    again = a.forward(otok, omask, None, ptok, pmask).clone()
    r1, c1 = a.graph_stats()
    assert all(torch.equal(x, base[0]) for x in base) and torch.equal(again, base[0])
    assert c1 == c0 and r1 == r0 + 1, "policy A's captured graph must survive option changes on policy B"
    assert max_abs(other, again) < 1e-4


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_graph_replay_is_exact(prec):
    """hipGraph replay of the per-env-step entry points (option "graphs"): the same warm loop and the same incremental
    episode, eager vs captured + replayed, must give bit-identical results; replays must actually happen."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 7)
    g = torch.Generator().manual_seed(3)
    B, Lp, Q, E, T = 2, 24, 8, cfg.embed_dim, 4
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    obs = syn.to_device(syn.make_obs(1, B, Q // 2, seed=5), DEV)
    acts = syn.to_device(syn.make_actions(1, B, seed=6), DEV)

    def loop(pol):
        outs = []
        for rep in range(4):                                  # identical calls: eager, capture, replay, replay
            otok, omask = pol.forward_obs_token(obs)
            pred = pol.forward(otok, omask, None, ptok, pmask)
            outs.append(pol.action_logits(pred[-1]).clone())
        for rep in range(3):                                  # three identical episodes through the incremental path
            for t in range(T):
                otok, omask = pol.forward_obs_token(obs)
                atok = pol.forward_action_token(acts) if t > 0 else None
                outs.append(pol.action_logits(pol.forward_step(otok, omask, atok, ptok, pmask, t)).clone())
        torch.cuda.synchronize()
        return outs

    eager = loop(loaded_policy(cfg, sd, prec))
    polg = loaded_policy(cfg, sd, prec, graphs=1)
    graphed = loop(polg)
    replays, captures = polg.graph_stats()
    assert captures > 0 and replays > captures, (replays, captures)
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)


def test_prompts_with_only_images_and_without_images():
    """Degenerate prompt compositions: a prompt made only of images (against the oracle), and a batch whose prompts are
    pure words -- the reference cannot run that one (`img.max()` of an empty image batch raises inside
    basic_image_tensor_preprocess, preprocess.py:28), the native path skips the object encoder: finite tokens, all-True mask,
    and the word rows equal those of a mixed prompt's T5 input up to attention (checked through determinism only)."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 9)
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    obs = syn.make_obs(1, 2, 2, seed=52)
    prompts = syn.make_prompt(2, layout=[[1, 1], [1, 0]], q_per_view=2, seed=51)
    o, od = run_policy(orc, prompts, obs, None)
    ref_logits = torch.cat([od[k]["raw"] for k in ACTION_KEYS], dim=-1)
    for prec, tol in (("fp32", 2e-5), ("bf16", 1e-3)):
        pol = loaded_policy(cfg, sd, prec)
        out = native_outputs(pol, prompts, obs, None)
        assert torch.equal(out["prompt_masks"].cpu(), o["prompt_masks"])
        assert max_abs(out["raw_logits"], ref_logits) < tol, (prec, max_abs(out["raw_logits"], ref_logits))
        assert max_rel(out["prompt_tokens"], o["prompt_tokens"]) < (2e-4 if prec == "fp32" else 4e-2)
    words_only = syn.make_prompt(2, layout=[[0, 0, 0], [0, 0, 0, 0, 0]], q_per_view=2, seed=51)
    pol = loaded_policy(cfg, sd, "bf16")
    ptok, pmask = pol.forward_prompt_assembly(syn.to_device(words_only, DEV))
    assert ptok.shape == (5, 2, cfg.embed_dim) and torch.isfinite(ptok).all()
    assert pmask.cpu().tolist() == [[True, True, True, False, False], [True] * 5]
    ptok2, _ = pol.forward_prompt_assembly(syn.to_device(words_only, DEV))
    assert torch.equal(ptok, ptok2)


def test_create_policy_from_ckpt_round_trip(tmp_path):
    """write a checkpoint file with the reference's layout ({"cfg": ctor kwargs, "state_dict":
    {"policy.<key>": tensor}}, vima/__init__.py:9-14), load it with vima_amd.create_policy_from_ckpt and compare with a
    policy filled through load_state_dict: bit-identical outputs; a file with a missing key fails strictly."""
    import vima_amd
    cfg, wseed, prompts, obs, actions = build_case("ragged_4M")
    sd = syn.make_state_dict(cfg, wseed)
    path = str(tmp_path / "4M.ckpt")
    torch.save({"cfg": cfg.ctor_kwargs(), "state_dict": {"policy." + k: v for k, v in sd.items()}}, path)
    pol = vima_amd.create_policy_from_ckpt(path, DEV)
    assert isinstance(pol, vima_amd.VIMAPolicy) and not pol.training and pol.embed_dim == cfg.embed_dim
    a = native_outputs(pol, prompts, obs, actions)
    b = native_outputs(loaded_policy(cfg, sd, "bf16"), prompts, obs, actions)
    for k in ("prompt_tokens", "obs_tokens", "predicted", "raw_logits", "modes"):
        assert torch.equal(a[k], b[k]), k
    assert set(pol.state_dict().keys()) == set(sd.keys())
    bad = {"policy." + k: v for k, v in sd.items() if k != "obs_fusion_layer.bias"}
    torch.save({"cfg": cfg.ctor_kwargs(), "state_dict": bad}, path)
    with pytest.raises(RuntimeError):
        vima_amd.create_policy_from_ckpt(path, DEV)


def test_forward_under_inference_mode():
    """inference tensors do not track a version counter; the prompt K/V cache key must not crash `forward`
    under torch.inference_mode() -- such calls run stateless and agree with the cached path bit for bit."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 5)
    pol = loaded_policy(cfg, sd, "bf16")
    prompts = syn.to_device(syn.make_prompt(2, n_segments=2, words_per_segment=3, q_per_view=2, seed=9), DEV)
    obs = syn.to_device(syn.make_obs(1, 2, 2, seed=10), DEV)
    with torch.no_grad():
        ptok, pmask = pol.forward_prompt_assembly(prompts)
        otok, omask = pol.forward_obs_token(obs)
        want = pol.forward(otok, omask, None, ptok, pmask)
        want2 = pol.forward(otok, omask, None, ptok, pmask)      # cached K/V
    with torch.inference_mode():
        ptok_i, pmask_i = pol.forward_prompt_assembly(prompts)
        otok_i, omask_i = pol.forward_obs_token(obs)
        assert ptok_i.is_inference()
        got = pol.forward(otok_i, omask_i, None, ptok_i, pmask_i)
        got2 = pol.forward(otok_i, omask_i, None, ptok_i, pmask_i)
    assert torch.equal(got, want) and torch.equal(got2, want) and torch.equal(want2, want)
    pol.reset_prompt_cache()
    assert torch.equal(pol.forward(otok, omask, None, ptok, pmask), want)
    with pytest.raises(AssertionError):      # fp16 tokens must be rejected on EVERY call, not reinterpreted
        pol.forward(otok.half(), omask, None, ptok, pmask)


def test_errors_mirror_reference():
    cfg = syn.config("2M")
    sd = syn.make_state_dict(cfg, 0)
    pol = loaded_policy(cfg, sd, "bf16")
    E = cfg.embed_dim
    with pytest.raises(AssertionError):      # xattn_gpt.py:110: prompt longer than xattn_n_positions
        pol.forward(torch.zeros(1, 1, 2, E, device=DEV), torch.ones(1, 1, 2, dtype=torch.bool, device=DEV), None,
                    torch.zeros(300, 1, E, device=DEV), torch.ones(1, 300, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):          # vima_policy.py:177: invalid prompt token type
        pol.forward_prompt_assembly(([[0, 2]], torch.zeros(1, dtype=torch.int64), syn.make_prompt(1)[2]))
    bad = dict(sd)
    bad.pop("obs_fusion_layer.bias")
    with pytest.raises(RuntimeError):        # strict load (vima/__init__.py:11-14)
        loaded_policy(cfg, bad, "bf16")


def test_full_size_200m_headline_batch_against_reference(golden_dir):
    """BASELINE.json configs[2] exactly as bench.py runs it (VIMA-200M, B=256, Lp=512, Q=8, same seeds): rows
    0/5/100/255 of the FULL batch are compared with what the unmodified reference computed for those samples
    (tests/golden/bench_200M.npz) -- prompt tokens, obs tokens, predicted action tokens and the raw logits (1e-3 abs,
    the north_star gate). Then size-independent properties: per-sample independence (a sub-batch -- and ONE sample alone, north_star's
    batch 1 -- reproduces its rows bit for bit up to 1e-5), opt-in split-K, and the fp32-operand mode on the sub-batch."""
    gold = np.load(os.path.join(golden_dir, "bench_200M.npz"))
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    pol = loaded_policy(cfg, sd, "bf16")
    B = 256
    prompts = syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1236)
    obs = syn.make_obs(1, B, 4, seed=1336)
    ptok, pmask = pol.forward_prompt_assembly(syn.to_device(prompts, DEV))
    assert ptok.shape == (512, B, 768) and pmask.shape == (B, 512)
    otok, omask = pol.forward_obs_token(syn.to_device(obs, DEV))
    pred = pol.forward(otok, omask, None, ptok, pmask)
    logits = pol.action_logits(pred[-1])
    torch.cuda.synchronize()
    assert logits.shape == (B, 700) and torch.isfinite(logits).all() and torch.isfinite(ptok).all()
    sub = CASES["bench_200M"]["cut"]
    ref_logits = torch.from_numpy(gold["raw_logits"])[0]
    err = max_abs(logits[sub], ref_logits)
    print(f"[parity] headline batch (B=256) rows {sub} vs reference: max|logit err| {err:.3e} (max|logit| {ref_logits.abs().max():.3g})")
    assert err < 1e-3, err
    assert torch.equal(pmask[sub].cpu(), torch.from_numpy(gold["prompt_masks"]))
    assert max_rel(gold_view("bench_200M", "prompt_tokens", ptok[:, sub]), torch.from_numpy(gold["prompt_tokens"])) < 4e-2
    assert max_rel(otok[:, sub], torch.from_numpy(gold["obs_tokens"])) < 4e-2
    assert max_rel(pred[:, sub], torch.from_numpy(gold["predicted"])) < 4e-2
    p_sub = syn.cut_prompt(prompts, sub)
    o_sub = syn.cut_obs(obs, sub)
    ptok_s, pmask_s = pol.forward_prompt_assembly(syn.to_device(p_sub, DEV))
    otok_s, omask_s = pol.forward_obs_token(syn.to_device(o_sub, DEV))
    logits_s = pol.action_logits(pol.forward(otok_s, omask_s, None, ptok_s, pmask_s)[-1])
    # Round 5: GEMMs of at most 32 rows (this sub-batch's decoder: 4 x 8 rows, its action head) run on gemm_skinny_kernel, whose K split sums in
    # another order than the tiles of the batch-256 run: equal to bf16 rounding (a fraction of the 1e-3 gate), and bit-level again with the option off
    d_s = max_abs(logits_s, logits[sub])
    pol.set_option("gemm_skinny", 0)
    ptok_x, pmask_x = pol.forward_prompt_assembly(syn.to_device(p_sub, DEV))
    otok_x, omask_x = pol.forward_obs_token(syn.to_device(o_sub, DEV))
    logits_x = pol.action_logits(pol.forward(otok_x, omask_x, None, ptok_x, pmask_x)[-1])
    pol.set_option("gemm_skinny", 1)
    print(f"[parity] sub-batch of 4 vs its rows of the batch-256 run: {d_s:.3e} (gemm_skinny on) / {max_abs(logits_x, logits[sub]):.3e} (off)")
    assert d_s < 5e-4, "samples of a batch must be independent"
    assert max_abs(logits_x, logits[sub]) < 1e-5, "samples of a batch must be independent"
    # in the DEFAULT configuration (gemm_skinny on) the sub-batch and the full batch must still pick the same action bins, except at
    # near-ties no wider than the rounding difference itself
    agree, total, gap = _flip_report(logits_s.float().cpu(), logits[sub].float().cpu())
    print(f"[parity] default config, sub-batch vs full batch: argmax agreement {agree}/{total}, widest gap at a flip {gap:.3e}")
    assert gap <= 2 * d_s + 1e-7, (agree, total, gap)
    # north_star's batch 1 at full size: sample sub[0] ALONE (M = 9 decoder rows: the 32x32 resident tiles, the grouped action head and
    # the dual GEGLU launch) against the reference's logits for that sample and against its row of the batch-256 run
    one = [sub[0]]
    ptok_1, pmask_1 = pol.forward_prompt_assembly(syn.to_device(syn.cut_prompt(prompts, one), DEV))
    otok_1, omask_1 = pol.forward_obs_token(syn.to_device(syn.cut_obs(obs, one), DEV))
    logits_1 = pol.action_logits(pol.forward(otok_1, omask_1, None, ptok_1, pmask_1)[-1])
    err1 = max_abs(logits_1, ref_logits[:1])
    print(f"[parity] batch 1 (sample {sub[0]} alone) vs reference: max|logit err| {err1:.3e}; vs its row of the batch-256 run: "
          f"{max_abs(logits_1, logits[one]):.3e}")
    assert err1 < 1e-3, err1
    assert max_abs(logits_1, logits[one]) < 5e-4, "a sample alone must reproduce its row of the full batch (to bf16 rounding: gemm_skinny_kernel)"
    # opt-in split-K for underfilled grids: the sub-batch then sums K in a different order than the full batch
    pol.set_option("gemm_splitk", 1)
    ptok_k, pmask_k = pol.forward_prompt_assembly(syn.to_device(p_sub, DEV))
    otok_k, omask_k = pol.forward_obs_token(syn.to_device(o_sub, DEV))
    logits_k = pol.action_logits(pol.forward(otok_k, omask_k, None, ptok_k, pmask_k)[-1])
    pol.set_option("gemm_splitk", 0)
    assert max_abs(logits_k, ref_logits) < 1e-3
    pol32 = loaded_policy(cfg, sd, "fp32", attn_impl=0)
    ptok_f, pmask_f = pol32.forward_prompt_assembly(syn.to_device(p_sub, DEV))
    otok_f, omask_f = pol32.forward_obs_token(syn.to_device(o_sub, DEV))
    logits_f = pol32.action_logits(pol32.forward(otok_f, omask_f, None, ptok_f, pmask_f)[-1])
    assert max_abs(logits_f, ref_logits) < 2e-5, max_abs(logits_f, ref_logits)


def test_headline_batch_every_row_against_live_oracle():
    """The benchmarked batch itself (VIMA-200M, B=256, Lp=512, Q=8, bench.py's seeds), bf16 path, against the oracle run live on
    the host in chunks of 32: every raw logit of ALL 256 rows within the north_star gate (1e-3 abs on logits of ~0.08), and the
    argmax of the 12 categorical heads reported. (VIMA_FAST_PARITY=1 checks every other chunk: 128 rows, half the host time.)"""
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    B = 256
    prompts = syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1236)
    obs = syn.make_obs(1, B, 4, seed=1336)
    pol = loaded_policy(cfg, sd, "bf16")
    got = native_outputs(pol, prompts, obs, None)["raw_logits"].cpu().reshape(B, 700)
    del pol
    torch.cuda.empty_cache()
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    # the oracle costs ~0.3 s of host CPU per sample (~80 s for the batch on the GPU box's 16 usable cores)
    full = os.environ.get("VIMA_FAST_PARITY", "0") != "1"
    rows, ref = [], []
    for lo in range(0, B, 32 if full else 64):
        idx = list(range(lo, lo + 32))
        rows += idx
        ref.append(orc.cold_step(syn.cut_prompt(prompts, idx), syn.cut_obs(obs, idx)))
    ref = torch.cat(ref, dim=0)
    got = got[rows]
    err = max_abs(got, ref)
    agree, total, gap = _flip_report(got, ref)
    print(f"[parity] headline batch, {len(rows)} of 256 rows vs live oracle: max|logit err| {err:.3e} (max|logit| {ref.abs().max():.3g}), "
          f"argmax agreement {agree}/{total} = {agree / total:.4f}, worst reference gap at a flip {gap:.3e}")
    assert err < 1e-3, err
    assert gap <= 2 * err + 1e-7
    assert len(rows) == (B if full else B // 2)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_per_sample_episode_restart_in_incremental_decoding(prec):
    """VERDICT r2 missing item 5: batched environments end their episodes at different steps. A batch of 3 steps together; after global
    step 1, sample 1 restarts with a NEW prompt (`restart_samples`). From then on its predictions must equal those of a fresh
    single-sample episode on the new prompt, and the other samples must be unaffected (their history continues)."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 5, head_gain=0.5)
    pol = loaded_policy(cfg, sd, prec)
    B, Q, qv, steps = 3, 4, 2, 5
    pr_a = syn.to_device(syn.make_prompt(B, n_segments=3, words_per_segment=3, q_per_view=qv, seed=31), DEV)
    pr_b = syn.to_device(syn.make_prompt(B, n_segments=3, words_per_segment=3, q_per_view=qv, seed=32), DEV)
    ptok_a, pmask_a = pol.forward_prompt_assembly(pr_a)
    ptok_b, pmask_b = pol.forward_prompt_assembly(pr_b)
    obs = [syn.to_device(syn.make_obs(1, B, qv, seed=40 + t), DEV) for t in range(steps)]
    acts = [syn.to_device(syn.make_actions(1, B, seed=60 + t), DEV) for t in range(steps)]
    otoks = [pol.forward_obs_token(o) for o in obs]
    atoks = [pol.forward_action_token(a) for a in acts]           # [1, B, E] "previous action" fed at step t + 1

    def run(ptok, pmask, sel, t0, n, restart_at=None, new=None):
        """n steps of forward_step for the samples `sel` (a slice of the batch) starting at data index t0."""
        out = []
        pt, pm = ptok[:, sel].contiguous(), pmask[sel].contiguous()
        for k in range(n):
            t = t0 + k
            if restart_at is not None and k == restart_at:
                flags = torch.zeros(pt.shape[1], dtype=torch.bool)
                flags[1] = True
                pt, pm = pt.clone(), pm.clone()
                pt[:, 1], pm[1] = new[0][:, 1], new[1][1]
                pol.restart_samples(flags, pt, pm)
            ot, om = otoks[t][0][:, sel], otoks[t][1][:, sel]
            prev = atoks[t - 1][:, sel] if k > 0 else None
            out.append(pol.forward_step(ot.contiguous(), om.contiguous(), prev.contiguous() if prev is not None else None, pt, pm, step=k).clone())
        return out

    allb = slice(0, B)
    mixed = run(ptok_a, pmask_a, allb, 0, steps, restart_at=2, new=(ptok_b, pmask_b))      # sample 1 restarts before global step 2
    plain = run(ptok_a, pmask_a, allb, 0, steps)                                               # nobody restarts
    fresh = run(ptok_b, pmask_b, slice(1, 2), 2, steps - 2)                                    # sample 1 alone, new prompt, data of steps 2..4
    tol = 2e-5 if prec == "fp32" else 3e-2
    for t in range(steps):
        for b in (0, 2):
            assert max_abs(mixed[t][b], plain[t][b]) <= tol * max(1.0, plain[t][b].abs().max().item()), (t, b)
    for k in range(steps - 2):
        ref = fresh[k][0]
        assert max_abs(mixed[2 + k][1], ref) <= tol * max(1.0, ref.abs().max().item()), (k, max_abs(mixed[2 + k][1], ref))
    assert max_abs(mixed[3][1], plain[3][1]) > 10 * tol            # the restart really changed sample 1's trajectory


def test_head_major_prompt_kv_cache_is_bit_identical():
    """Round 4: where the decoder's prompt K / V projection runs on the persistent 256x256 GEMM (batch x prompt large enough) its epilogue
    writes the per-layer K / V head-major ([B][2 heads][Lp][head dim], option kv_headmajor, default on) and every attention kernel reads it
    through batch / head strides. Same values, same arithmetic: full-history forward (cache built, then re-used), incremental steps, a
    per-sample restart (whose rows are rebuilt row-major and transposed) and the stateless path must all equal the row-major layout
    bit for bit. 2M model (E 256, 8 heads of 32), 40 samples x 512-token prompt = 160 tiles of 256x256 in the projection."""
    cfg = syn.config("2M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 11, head_gain=0.5)
    B, Lp, Q, E = 40, 512, 4, cfg.embed_dim
    g = torch.Generator().manual_seed(3)
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = (torch.rand(B, Lp, generator=g) > 0.1)
    pmask[:, 0] = True
    pmask = pmask.to(DEV)
    ptok2 = torch.randn(Lp, B, E, generator=g).to(DEV)
    otok = [torch.randn(T, B, Q, E, generator=g).to(DEV) for T in (1, 2, 9)]            # T = 9: 44 queries (the 1-wave MFMA kernel); 1, 2: split-key
    omask = [torch.ones(T, B, Q, dtype=torch.bool, device=DEV) for T in (1, 2, 9)]
    atok = [None] + [torch.randn(T - 1, B, E, generator=g).to(DEV) for T in (2, 9)]
    step_o = [torch.randn(1, B, Q, E, generator=g).to(DEV) for _ in range(4)]
    step_a = [torch.randn(1, B, E, generator=g).to(DEV) for _ in range(4)]

    def run(hm, cache):
        pol = loaded_policy(cfg, sd, "bf16", kv_headmajor=hm)
        pol.cache_prompt_kv = cache
        outs = []
        pol.prof_enable(True)
        outs.append(pol.forward(otok[0], omask[0], atok[0], ptok, pmask).clone())             # builds the cache (or stateless)
        torch.cuda.synchronize()
        kinds = pol.prof_read_gemm_kernels()
        pol.prof_enable(False)
        outs.append(pol.forward(otok[1], omask[1], atok[1], ptok, pmask).clone())             # re-uses it
        outs.append(pol.forward(otok[2], omask[2], atok[2], ptok, pmask).clone())
        pt, pm = ptok, pmask
        for k in range(4):                                                                    # incremental episode with a restart before step 2
            if k == 2:
                flags = torch.zeros(B, dtype=torch.bool)
                flags[[1, 17]] = True
                pt = ptok.clone()
                pt[:, 1], pt[:, 17] = ptok2[:, 1], ptok2[:, 17]
                pol.restart_samples(flags, pt, pm)
            outs.append(pol.forward_step(step_o[k], torch.ones(1, B, Q, dtype=torch.bool, device=DEV), step_a[k - 1] if k > 0 else None, pt, pm, step=k).clone())
        return outs, kinds

    ref, kinds0 = run(0, True)
    got, kinds1 = run(1, True)
    assert any("gemm_pp_kernel" in k or "gemm_persistent_kernel" in k for k in kinds1), kinds1.keys()   # the projection took the kernel that writes head-major
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (i, (a - b).abs().max().item())
    stateless, _ = run(1, False)
    for i in range(3):
        assert torch.equal(stateless[i], ref[i]), i


@pytest.mark.parametrize("size,B,Ts", [("2M", 256, (1, 2)), ("2M", 250, (1,)), ("200M", 256, (1,))])
def test_geglu_pair_over_interleaved_weights_is_bit_identical(size, B, Ts):
    """Round 4: the decoder blocks' MLP (components.py:221-226: c_fc GELU'd x gated_layer, both reading ln_1's output) runs as ONE GEMM launch over
    block-interleaved weights (GemmArgs::pair32, option geglu_pair, default on) where the [rows, 4E] grid is too large for the dual-accumulator
    resident form and too small for the persistent 256x256 kernels -- batch 256 x 8 object tokens = 2048 rows, the warm / incremental step of the
    headline workload. Both factors of an output element sit in one lane's accumulators, and the epilogue applies the operations and roundings of the
    two-launch form: logits must be equal bit for bit (ragged row count: 250 x 8 rows)."""
    cfg = syn.config(size, xattn_n_positions=256)
    sd = syn.make_state_dict(cfg, 5, head_gain=0.5)
    Lp, Q, E = 64, 8, cfg.embed_dim
    g = torch.Generator().manual_seed(9)
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    outs = {}
    for pair in (0, 1):
        pol = loaded_policy(cfg, sd, "bf16", geglu_pair=pair, ln_fuse=0)   # (ln_fuse would route XAttention's GEGLU through the pair form as well: test_ln_fuse_*)
        res = []
        for T in Ts:
            gi = torch.Generator().manual_seed(100 + T)
            otok = torch.randn(T, B, Q, E, generator=gi).to(DEV)
            atok = torch.randn(T - 1, B, E, generator=gi).to(DEV) if T > 1 else None
            pol.prof_enable(True)
            res.append(pol.forward(otok, torch.ones(T, B, Q, dtype=torch.bool, device=DEV), atok, ptok, pmask).clone())
            torch.cuda.synchronize()
            launches = pol.prof_read_gemm_launches()
            pol.prof_enable(False)
            n_pair = sum(1 for l in launches if l["N"] == 8 * E)          # the interleaved weight has 2 x 4E rows
            assert n_pair == (cfg.xf_n_layers if pair else 0), (pair, T, n_pair)
        outs[pair] = res
        del pol
    for a, b in zip(outs[1], outs[0]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("size,B,T", [("4M", 3, 2), ("2M", 256, 1), ("2M", 250, 2), ("200M", 256, 1), ("200M", 4, 1), ("200M", 32, 1)])
def test_ln_fuse_decoder_layernorms(size, B, T):
    """Round 5: option ln_fuse (default on). (1) ln_2 of decoder layer i and the query pre-LN of XAttention in layer i + 1
    (components.py:37,166) are one launch of layernorm2_kernel; (2) the pre-LN in front of XAttention's feed-forward (components.py:220-226) is folded
    into the GEMMs either side: attention_out's epilogue writes per-32-column sums / sums of squares of the new stream, and the GEGLU -- whose two
    products then both read the un-normed stream -- runs as ONE launch (dual-accumulator resident form at small grids, block-interleaved pair32
    form at mid-size ones) applying rstd * (acc - mean * c[n]) + d[n] to the GELU'd factor. (1) is bit-exact; (2) moves a bf16 rounding point (the
    operand is bf16(a) instead of bf16(LN(a))), so the gate is the usual bf16 one against the unfused path, and the launch log must show the
    LayerNorm launches gone: 4 per layer -> 2, and one GEGLU launch per layer where the pair forms exist."""
    cfg = syn.config(size, xattn_n_positions=256)
    sd = syn.make_state_dict(cfg, 7, head_gain=0.5)
    Lp, Q, E, NL = 64, 8, cfg.embed_dim, cfg.xf_n_layers
    g = torch.Generator().manual_seed(19)
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    pmask[0, 50:] = False
    otok = torch.randn(T, B, Q, E, generator=g).to(DEV)
    omask = torch.ones(T, B, Q, dtype=torch.bool, device=DEV)
    atok = torch.randn(T - 1, B, E, generator=g).to(DEV) if T > 1 else None
    outs, other, n8 = {}, {}, {}
    for fuse in (0, 1):
        pol = loaded_policy(cfg, sd, "bf16", ln_fuse=fuse)
        pol.forward(otok, omask, atok, ptok, pmask)
        pol.prof_enable(True)
        outs[fuse] = pol.forward(otok, omask, atok, ptok, pmask).clone()
        torch.cuda.synchronize()
        launches = pol.prof_read_gemm_launches()
        prof = pol.prof_read_ex()
        pol.prof_enable(False)
        other[fuse] = prof["other"]["launches"]
        n8[fuse] = sum(1 for l in launches if l["N"] == 8 * E)
        outs[(fuse, "lg")] = pol.action_logits(outs[fuse][-1]).clone()
        del pol
    rows = B * (T * Q + T - 1)
    err, lerr = max_rel(outs[1], outs[0]), max_abs(outs[(1, "lg")], outs[(0, "lg")])
    print(f"[ln_fuse] VIMA-{size}, {rows} decoder rows: predicted tokens fused vs unfused max rel {err:.3e}; logits max abs {lerr:.3e} "
          f"(max |logit| {outs[(0, 'lg')].abs().max().item():.3g}); elementwise launches {other[0]} -> {other[1]}; N = 8E GEMM launches {n8[0]} -> {n8[1]}")
    assert torch.isfinite(outs[1]).all()
    assert err < 4e-2 and lerr < 2e-2 * outs[(0, "lg")].abs().max().item()
    # 4 LayerNorm launches per layer -> 2 where the fold applies (every size here but the 341 .. 683-row gap between the two pair forms), else 3
    assert other[0] - other[1] >= NL + (NL - 1)


def test_ln_fuse_double_layernorm_is_bit_identical():
    """layernorm2_kernel (ln_2 + the next layer's query pre-LN in one launch) against the two launches it replaces: with the fold of part (2) out of
    reach (fp8w weights: the folded operands are packed for bf16 weights only) the option changes nothing but the launch count."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 7, head_gain=0.5)
    g = torch.Generator().manual_seed(23)
    B, Lp, Q, T, E = 5, 40, 6, 3, cfg.embed_dim
    ptok = torch.randn(Lp, B, E, generator=g).to(DEV)
    pmask = torch.ones(B, Lp, dtype=torch.bool, device=DEV)
    otok = torch.randn(T, B, Q, E, generator=g).to(DEV)
    omask = torch.ones(T, B, Q, dtype=torch.bool, device=DEV)
    atok = torch.randn(T - 1, B, E, generator=g).to(DEV)
    a = loaded_policy(cfg, sd, "fp8w", ln_fuse=1).forward(otok, omask, atok, ptok, pmask)
    b = loaded_policy(cfg, sd, "fp8w", ln_fuse=0).forward(otok, omask, atok, ptok, pmask)
    assert torch.equal(a, b), (a - b).abs().max().item()


def test_t8_history_200m_against_live_oracle():
    """the `t8` line of the bench record (VIMA-200M, T = 8 observation steps re-fed like the reference's eval loop does,
    Lq = 71 decoder tokens per sample: causal self-attention on the >= 64-query 4-wave kernel, cross attention on the MFMA kernel, 512-token
    prompt) had no oracle parity at that size -- policy-level parity stopped at T <= 3 on small models. Batch 32 with bench.py's own generators
    (seeds 1236 / 1336 / 1436), bf16 path, EVERY step's logits of the sampled rows against the oracle run live on the host: 1e-3 abs."""
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    B, T = 32, 8
    prompts = syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1236)
    obs = syn.make_obs(T, B, 4, seed=1336)
    past = syn.make_actions(T - 1, B, seed=1436)
    pol = loaded_policy(cfg, sd, "bf16")
    p, o, a = syn.to_device(prompts, DEV), syn.to_device(obs, DEV), syn.to_device(past, DEV)
    ptok, pmask = pol.forward_prompt_assembly(p)
    otok, omask = pol.forward_obs_token(o)
    atok = pol.forward_action_token(a)
    pol.prof_enable(True)
    pred = pol.forward(otok, omask, atok, ptok, pmask)
    torch.cuda.synchronize()
    prof = pol.prof_read_ex()
    pol.prof_enable(False)
    assert pred.shape == (T, B, cfg.embed_dim)
    got = pol.action_logits(pred).float().cpu()              # [T, B, 700]
    rows = [0, 9, 18, 31]
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        cp, co, ca = syn.cut_prompt(prompts, rows), syn.cut_obs(obs, rows), syn.cut_actions(past, rows)
        r_ptok, r_pmask = orc.forward_prompt_assembly(cp)
        r_otok, r_omask = orc.forward_obs_token(co)
        r_pred = orc.forward(r_otok, r_omask, orc.forward_action_token(ca), r_ptok, r_pmask)
        ref = orc.action_logits(r_pred)                      # [T, 4, 700]
    err = max_abs(got[:, rows], ref)
    agree, total, gap = _flip_report(got[:, rows].reshape(-1, 700), ref.reshape(-1, 700))
    print(f"[parity] VIMA-200M, T = {T} (Lq = {T * 9 - 1}), batch {B}, rows {rows} x {T} steps vs live oracle: max|logit err| {err:.3e} "
          f"(max|logit| {ref.abs().max():.3g}), predicted tokens max rel {max_rel(pred[:, rows], r_pred):.3e}, argmax agreement {agree}/{total}, "
          f"worst reference gap at a flip {gap:.3e}; attention launches {prof['attention']['launches']}")
    assert torch.isfinite(got).all()
    assert err < 1e-3, err
    assert gap <= 2 * err + 1e-7


def _time_slice(obs, lo, hi):
    """Env steps [lo, hi) of a `make_obs` dict (time is dim 0)."""
    return {"objects": type(obs["objects"])({k: type(obs["objects"][k])({v: obs["objects"][k][v][lo:hi] for v in obs["objects"][k]})
                                              for k in obs["objects"]}), "ee": obs["ee"][lo:hi]}


def test_incremental_decoding_benchmarked_shape_against_live_oracle():
    """`incremental_env_step_ms` is VIMA-200M at B = 256, Lp = 512 -- M = 2304 decoder rows: the GEGLU pair on
    gemm_pp_kernel<2, 6> with the flat tile enumeration and the column-split q|k|v launch (GemmArgs::split_n). Those launches had parity only
    against the library's own full-history path at B = 64. Here: bench.py's generators (seeds 1236 / 1336 / 1436), T = 5 env steps through
    `forward_step`, EVERY step's logits of four sampled rows against the oracle run live on the host over the re-fed history (1e-3 abs), one
    sampled row restarting mid-episode with a new prompt (`restart_samples`; its oracle is a fresh episode on the new prompt), and the launch
    log shows that the two launch forms in question really ran."""
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    B, T, E = 256, 5, cfg.embed_dim
    prompts = syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1236)
    prompts_new = syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=2236)
    obs = syn.make_obs(T, B, 4, seed=1336)
    past = syn.make_actions(T - 1, B, seed=1436)
    pol = loaded_policy(cfg, sd, "bf16")
    ptok, pmask = pol.forward_prompt_assembly(syn.to_device(prompts, DEV))
    ptok_n, pmask_n = pol.forward_prompt_assembly(syn.to_device(prompts_new, DEV))
    otok, omask = pol.forward_obs_token(syn.to_device(obs, DEV))            # [T, B, Q, E]
    atok = pol.forward_action_token(syn.to_device(past, DEV))               # [T - 1, B, E]
    rows, r_restart, t_restart = [0, 77, 130, 255], 130, 3
    got = []
    pt, pm = ptok, pmask
    for t in range(T):
        if t == t_restart:
            flags = torch.zeros(B, dtype=torch.bool)
            flags[r_restart] = True
            pt, pm = ptok.clone(), pmask.clone()
            pt[:, r_restart], pm[r_restart] = ptok_n[:, r_restart], pmask_n[r_restart]
            pol.restart_samples(flags, pt, pm)
        if t == 1:
            pol.prof_enable(True)
        step = pol.forward_step(otok[t], omask[t], atok[t - 1] if t > 0 else None, pt, pm, t)
        if t == 1:
            torch.cuda.synchronize()
            launches = pol.prof_read_gemm_launches()
            pol.prof_enable(False)
        got.append(pol.action_logits(step).float().cpu())
    got = torch.stack(got)                                                  # [T, B, 700]
    assert torch.isfinite(got).all()
    m_dec = B * 9
    pair = [l for l in launches if l["kernel"].startswith("vima::gemm_pp_kernel<2, 6") and l["M"] == m_dec]
    split = [l for l in launches if l["M"] == m_dec and l["N"] == 3 * E and l["K"] == E]
    assert len(pair) >= cfg.xf_n_layers, f"the M = {m_dec} GEGLU pair launches on gemm_pp_kernel<2, 6>: {sorted(set(l['kernel'] for l in launches))}"
    assert len(split) == cfg.xf_n_layers, f"one column-split q|k|v launch per decoder layer, got {len(split)}"
    del pol
    torch.cuda.empty_cache()
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        keep = [r for r in rows if r != r_restart]
        r_ptok, r_pmask = orc.forward_prompt_assembly(syn.cut_prompt(prompts, rows))
        r_otok, r_omask = orc.forward_obs_token(syn.cut_obs(obs, rows))
        r_atok = orc.forward_action_token(syn.cut_actions(past, rows))
        ref = orc.action_logits(orc.forward(r_otok, r_omask, r_atok, r_ptok, r_pmask))           # [T, 4, 700]: nobody restarts
        # the restarted row from t_restart on: a fresh episode on the new prompt over the observations / previous actions of steps t_restart ..
        n_ptok, n_pmask = orc.forward_prompt_assembly(syn.cut_prompt(prompts_new, [r_restart]))
        o_cut = _time_slice(syn.cut_obs(obs, [r_restart]), t_restart, T)
        n_otok, n_omask = orc.forward_obs_token(o_cut)
        a_cut = {k: v[t_restart:] for k, v in syn.cut_actions(past, [r_restart]).items()}          # fed at steps t_restart + 1 ..
        n_atok = orc.forward_action_token(a_cut) if T - 1 - t_restart > 0 else None
        ref_new = orc.action_logits(orc.forward(n_otok, n_omask, n_atok, n_ptok, n_pmask))       # [T - t_restart, 1, 700]
    i_restart = rows.index(r_restart)
    ref_plain = ref
    ref = ref.clone()
    ref[t_restart:, i_restart] = ref_new[:, 0]
    err_t = [max_abs(got[t][rows], ref[t]) for t in range(T)]
    agree, total, gap = _flip_report(got[:, rows].reshape(-1, 700), ref.reshape(-1, 700))
    print(f"[parity] incremental decoding at the benchmarked shape (VIMA-200M, B = {B}, Lp = 512, T = {T}), rows {rows} (row {r_restart} restarts at step "
          f"{t_restart}) vs live oracle: max|logit err| per step {['%.2e' % e for e in err_t]} (max|logit| {ref.abs().max():.3g}), argmax agreement "
          f"{agree}/{total}, worst reference gap at a flip {gap:.3e}; pair launches {len(pair)}, split_n launches {len(split)}")
    assert max(err_t) < 1e-3, err_t
    assert gap <= 2 * max(err_t) + 1e-7
    moved = max_abs(got[t_restart][r_restart], ref_plain[t_restart][i_restart])
    print(f"[parity] restarted row vs its no-restart oracle logits at step {t_restart}: {moved:.3e}")
    assert len(keep) == 3 and moved > err_t[t_restart]                   # the restart really changed the row's trajectory


def test_batch32_cold_step_200m_against_live_oracle():
    """north_star's batch 32 at VIMA-200M, T = 1 cold (decoder M = 256 rows: the dual-accumulator GEGLU pair with the
    folded LayerNorm, 192-tile T5 GEMM grids) was compared fused-vs-unfused only. bench.py's generators at batch 32, every row's logits
    against the oracle run live on the host: 1e-3 abs."""
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    B = 32
    prompts = syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1236)
    obs = syn.make_obs(1, B, 4, seed=1336)
    pol = loaded_policy(cfg, sd, "bf16")
    got = native_outputs(pol, prompts, obs, None)["raw_logits"].cpu().reshape(B, 700)
    del pol
    torch.cuda.empty_cache()
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = orc.cold_step(prompts, obs)
    err = max_abs(got, ref)
    agree, total, gap = _flip_report(got, ref)
    print(f"[parity] VIMA-200M batch 32 cold step, all {B} rows vs live oracle: max|logit err| {err:.3e} (max|logit| {ref.abs().max():.3g}), "
          f"argmax agreement {agree}/{total}, worst reference gap at a flip {gap:.3e}")
    assert err < 1e-3, err
    assert gap <= 2 * err + 1e-7


def test_q4_gemm_tile_in_the_headline_batch_is_bit_identical():
    """Round 6: with option gemm_q4 the large bf16 GEMMs whose N is a multiple of 384 (ViT in_proj / fc / out_proj / c_proj, T5 o / wo, the decoder's
    head-major prompt K / V projection) run on gemm_q4_kernel (256x384 tile, four waves, inline-asm MFMAs with accumulators in both register files).
    The headline batch (VIMA-200M, B = 256, Lp = 512, bench.py's seeds) must come out BIT-IDENTICAL to the default kernels -- every tile shape
    accumulates K in the same order -- and the launch log must show that the kernel really ran in every epilogue form it has."""
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    B = 256
    prompts = syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1236), DEV)
    obs = syn.to_device(syn.make_obs(1, B, 4, seed=1336), DEV)
    pol = loaded_policy(cfg, sd, "bf16")

    def step():
        ptok, pmask = pol.forward_prompt_assembly(prompts)
        otok, omask = pol.forward_obs_token(obs)
        return ptok, otok, pol.action_logits(pol.forward(otok, omask, None, ptok, pmask)[-1])

    pol.set_option("gemm_q4", 0)            # the 256x256 kernels everywhere
    ref = step()
    pol.set_option("gemm_q4", 1)            # the 256x384 tile wherever it fits (the default, 6, takes it from 32 768 rows on)
    pol.prof_enable(True)
    got = step()
    torch.cuda.synchronize()
    kinds = sorted(set(l["kernel"] for l in pol.prof_read_gemm_launches() if "gemm_q4_kernel" in l["kernel"]))
    pol.prof_enable(False)
    pol.set_option("gemm_q4", 6)
    print(f"[q4] kernels in the headline step: {kinds}")
    assert any(k.endswith("<0, 4, 2>") for k in kinds) and any(k.endswith("<0, 5, 2>") for k in kinds) and any(k.endswith("<0, 1, 2>") for k in kinds) \
        and any(k.endswith("<3, 1, 2>") for k in kinds), kinds
    for a, b, what in zip(ref, got, ("prompt tokens", "obs tokens", "logits")):
        assert torch.equal(a, b), what


@pytest.mark.gpu
@pytest.mark.parametrize("n,qv,chunk", [(291, 4, 0), (700, 4, 2600)])
def test_vit_padded_chunks_are_bit_identical(n, qv, chunk):
    """Option vit_pad (default on): a ViT pass over a crop count that is not a multiple of 256 is computed on the next multiple (zero-image pad crops whose features
    nobody reads), so that its GEMMs keep the 256-row tile kernels; ObjEncoder.forward (obj_encoder.py:66-95) must return the same bits as the unpadded pass
    (every kernel on the way is row-wise, and the tile kernels are bit-identical to one another). 2 n qv = 2 328 crops in one pass, and 5 600 crops in chunks
    of 2 816 (the last one padded) on two streams."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 5)
    pol = loaded_policy(cfg, sd, "bf16")
    g = torch.Generator().manual_seed(n)
    objs = syn._objects(g, (n,), qv)
    crops, bbox = syn.to_device(objs["cropped_img"], DEV), syn.to_device(objs["bbox"], DEV)
    if chunk:
        pol.set_option("vit_chunk", chunk)
    try:
        pol.set_option("vit_pad", 1)
        a = pol.obj_encoder(crops, bbox).clone()
        pol.set_option("vit_pad", 0)
        b = pol.obj_encoder(crops, bbox).clone()
    finally:
        pol.set_option("vit_pad", 1)
        pol.set_option("vit_chunk", 16384)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), max_abs(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", [(10, 496), (5, 500)])
def test_t5_padded_rows_are_bit_identical(B, L):
    """Option t5_pad (default on): a T5 pass whose row count per stream (2 480 = 5 x 496, or 2 500 on one stream) is not a multiple of 256 is computed on the next
    multiple -- zero pad rows through the GEMM chain, no attention launch sees them -- so that T5PromptEncoder's GEMMs (prompt_encoder.py:681-825) keep the 256-row
    tile kernels; the encoder output must be the same bits as the unpadded pass."""
    cfg = syn.config("4M")
    sd = syn.make_state_dict(cfg, 7)
    pol = loaded_policy(cfg, sd, "bf16")
    g = torch.Generator().manual_seed(B * L)
    x = torch.randn(B, L, 768, generator=g).to(DEV)
    mask = torch.rand(B, L, generator=g) > 0.1
    mask[:, 0] = True
    try:
        if B < 8:
            pol.set_option("dual_stream", 0)
        pol.set_option("t5_pad", 1)
        a = pol.t5_encode(x, mask.to(DEV)).clone()
        pol.set_option("t5_pad", 0)
        b = pol.t5_encode(x, mask.to(DEV)).clone()
    finally:
        pol.set_option("t5_pad", 1)
        pol.set_option("dual_stream", 1)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), max_abs(a, b)


@pytest.mark.gpu
def test_default_tiling_choices_are_bit_identical_at_an_odd_size():
    """VIMA-200M at batch 50 with 496-token prompts (24 800 T5 rows, 25 600 + 400 crops: nothing a multiple of 256): the defaults -- T5 streams and ViT chunks computed on
    padded row counts (t5_pad, vit_pad), the 256x384 GEMM tile from 32 768 rows on (gemm_q4 = 6) -- against the plain run without any of them. Every choice only changes WHICH
    tile kernel multiplies which rows, so the whole policy forward (prompt_encoder.py / vit.py / xattn_gpt.py) must return the same bits."""
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    pol = loaded_policy(cfg, sd, "bf16")
    B = 50
    prompts = syn.to_device(syn.make_prompt(B, n_segments=31, words_per_segment=8, q_per_view=4, seed=1236), DEV)
    obs = syn.to_device(syn.make_obs(1, B, 4, seed=1336), DEV)

    def step():
        ptok, pmask = pol.forward_prompt_assembly(prompts)
        otok, omask = pol.forward_obs_token(obs)
        return ptok, pol.action_logits(pol.forward(otok, omask, None, ptok, pmask)[-1])

    try:
        a = [t.clone() for t in step()]
        for k in ("t5_pad", "vit_pad", "gemm_q4"):
            pol.set_option(k, 0)
        b = [t.clone() for t in step()]
    finally:
        pol.set_option("t5_pad", 1)
        pol.set_option("vit_pad", 1)
        pol.set_option("gemm_q4", 6)
    assert torch.isfinite(a[1]).all()
    for x, y, what in zip(a, b, ("prompt tokens", "logits")):
        assert torch.equal(x, y), (what, max_abs(x, y))
