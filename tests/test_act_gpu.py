"""On-device action selection on the MI355X: vima_action_select (`vima_amd.actions.select_actions`) against torch.argmax, the
reference's golden modes and fp64 statistics; vima_act (`VIMAPolicy.act`) bit for bit against the entry points it chains, under
hipGraph replay, by its launch counts, and in the closed evaluation loop.

References and exemptions are in tests/act_reference.py; tests/test_act_build.py bounds the exempt share on the CPU.

Continuous actions: the kernel divides (float)bin by 50 / 100 like `_de_discretize_actions` does on CPU tensors, which is how the
stored reference run computed the actions it sent to the environment. torch's GPU kernel for tensor / python-scalar multiplies by
the rounded reciprocal instead and differs from the division by one ulp on some bins (5, 9, 10, 15, ... of 50), so the bit-equal
references here are evaluated on CPU tensors; the number of elements the GPU evaluation of the same expression differs on is printed."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from tests import act_reference as ref                       # noqa: E402
from tests.gpu_common import loaded_policy, ptr              # noqa: E402
from vima_testing import synthetic as syn                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOW, HIGH = [0.25, -0.5], [0.75, 0.5]


def _bins(sel):
    return torch.cat([sel.actions[k].reshape(-1, w) for k, w in zip(ref.KEYS, ref.KEY_DIMS)], dim=1).cpu().numpy()


def _cont(sel):
    return torch.cat([sel.continuous[k].reshape(-1, w) for k, w in zip(ref.KEYS, ref.KEY_DIMS)], dim=1).cpu().numpy()


def _per_key(d):
    return torch.stack([d[k].reshape(-1) for k in ref.KEYS], dim=1).cpu().numpy().astype(np.float64)


def _select(x, u=None, bounds=None):
    from vima_amd.actions import select_actions
    return select_actions(torch.from_numpy(x).to(DEV), None if u is None else torch.from_numpy(u).to(DEV), bounds)


def _check_stats(x, sel, bins, tag):
    lp64, en64 = ref.stats64(x, bins)
    for what, got, want in (("log_prob", _per_key(sel.log_prob), lp64), ("entropy", _per_key(sel.entropy), en64)):
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print(f"[act] {tag} {what}: max error {err.max():.3e} relative to max(1, |ref|) (bound 2e-5), max |ref| {np.abs(want).max():.3f}")
        assert np.isfinite(got).all() and err.max() <= 2e-5, (tag, what, err.max())


# ------------------------------------------------------------------------------------------ handle-free selection
@pytest.mark.parametrize("name", ref.GOLDENS)
def test_mode_is_argmax_and_the_reference_mode(name):
    x, modes = ref.golden_logits(name)
    sel = _select(x)
    bins = _bins(sel)
    assert sel.actions["pose0_position"].dtype == torch.int64 and sel.continuous["pose0_rotation"].dtype == torch.float32
    assert np.array_equal(bins, ref.argmax_bins(x))                                         # exact, every pair
    dev_argmax = torch.stack([s.argmax(dim=1) for s in torch.split(torch.from_numpy(x).to(DEV), list(ref.BINS), dim=1)], dim=1)
    assert np.array_equal(bins, dev_argmax.cpu().numpy())
    if modes is not None:                                                                   # the baseline goldens store no modes
        keep = ~ref.mode_exempt(x)
        print(f"[act] {name}: {int((~keep).sum())} of {keep.size} pairs exempt from the golden-mode comparison")
        assert (~keep).mean() <= 0.01
        assert np.array_equal(bins[keep], modes[keep])
    _check_stats(x, sel, bins, name)


@pytest.mark.parametrize("scale", ref.SCALES)
def test_mode_and_statistics_on_random_logits(scale):
    x = ref.random_logits(scale)
    sel = _select(x)
    bins = _bins(sel)
    assert np.array_equal(bins, ref.argmax_bins(x))
    _check_stats(x, sel, bins, f"scale {scale}")


@pytest.mark.parametrize("scale", ref.SCALES)
def test_sampling_is_the_fp64_inverse_cdf(scale):
    x, u = ref.random_logits(scale), ref.random_uniforms()
    b64, exempt = ref.sample_bins64(x, u)
    sel = _select(x, u)
    bins = _bins(sel)
    diff = bins != b64
    print(f"[act] sampling at scale {scale}: {int(exempt.sum())} of {exempt.size} pairs exempt ({100.0 * exempt.mean():.3f} %), "
          f"{int(diff.sum())} bins differ from fp64, {int((diff & ~exempt).sum())} of them outside the exemption")
    assert exempt.mean() <= 0.01
    assert bins.min() >= 0 and (bins < np.array(ref.BINS)).all()
    assert not (diff & ~exempt).any()
    _check_stats(x, sel, bins, f"sampled, scale {scale}")        # log-probability of the SAMPLED bins
    assert len(np.unique(bins[:, 1])) > 50                       # it samples: not the mode everywhere


def test_bins_stay_in_range_whatever_the_inputs_hold():
    x = ref.random_logits(4.0, rows=64)
    x[1, :] = 0.0                                                # all ties: first index
    x[2, 10:20] = np.nan
    x[3, :] = np.nan
    x[4, :] = -np.inf
    x[5, 60:90] = np.inf
    x[6, :] = 1e30
    top = np.array(ref.BINS) - 1
    for uval in (0.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), 1.0, 7.0, -3.0, float("nan")):
        u = np.full((64, 12), uval, dtype=np.float32)
        bins = _bins(_select(x, u))
        assert bins.min() >= 0 and (bins <= top).all(), uval
        if uval == 0.0:
            assert (bins[0] == 0).all()
        if uval >= 0.9999:                                       # flat row: the last bin holds 1 / n of the mass
            assert (bins[1] == top).all()
    bins = _bins(_select(x))
    assert bins.min() >= 0 and (bins <= top).all()
    assert (bins[1] == 0).all()
    keep = [0] + list(range(7, 64))
    assert np.array_equal(bins[keep], ref.argmax_bins(x)[keep])


def _torch_gpu_expression(bins, low=None, high=None):
    """the same expressions evaluated by torch ON THE GPU (figures only)"""
    from vima_amd.policy import VIMAPolicy
    acts = {k: torch.from_numpy(bins[:, f:f + w]).to(DEV) for k, f, w in zip(ref.KEYS, ref.KEY_FIRST, ref.KEY_DIMS)}
    bins_of = types.SimpleNamespace(_n_discrete_x_bins=50, _n_discrete_y_bins=100, _n_discrete_rot_bins=50)
    cont = VIMAPolicy._de_discretize_actions(bins_of, acts)
    if low is not None:
        lo, hi = torch.tensor([low], device=DEV), torch.tensor([high], device=DEV)
        for k in ("pose0_position", "pose1_position"):
            cont[k] = torch.clamp(cont[k] * (hi - lo) + lo, min=lo, max=hi)
        for k in ("pose0_rotation", "pose1_rotation"):
            cont[k] = torch.clamp(cont[k] * 2 - 1, min=-1, max=1)
    return torch.cat([cont[k] for k in ref.KEYS], dim=1).cpu().numpy()


def test_continuous_actions_are_bit_equal_to_the_torch_expressions():
    x, u = ref.random_logits(0.1), ref.random_uniforms()         # flat distributions: the samples visit every bin
    sel = _select(x, u)
    bins = _bins(sel)
    assert all(len(np.unique(bins[:, d])) == ref.BINS[d] for d in range(12))
    want = ref.de_discretize_cpu(bins)
    got = _cont(sel)
    print(f"[act] continuous, no bounds: {int((got != want).sum())} of {got.size} differ from _de_discretize_actions (CPU tensors); "
          f"{int((got != _torch_gpu_expression(bins)).sum())} from its GPU evaluation")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    selb = _select(x, u, {"low": np.array(LOW, dtype=np.float32), "high": np.array(HIGH, dtype=np.float32)})
    assert np.array_equal(_bins(selb), bins)
    wantb, gotb = ref.rescale_cpu(bins, LOW, HIGH), _cont(selb)
    print(f"[act] continuous, bounds {LOW} .. {HIGH}: {int((gotb != wantb).sum())} of {gotb.size} differ from the reference loop's "
          f"expression (CPU tensors); {int((gotb != _torch_gpu_expression(bins, LOW, HIGH)).sum())} from its GPU evaluation")
    assert np.array_equal(gotb.view(np.uint32), wantb.view(np.uint32))
    assert gotb[:, [0, 6]].min() >= 0.25 and gotb[:, [0, 6]].max() <= 0.75 and np.abs(gotb[:, [2, 3, 4, 5, 8, 9, 10, 11]]).max() <= 1.0


# ------------------------------------------------------------------------------------------ vima_act on loaded policies
def _policy(model, prec, **opts):
    if model == "gato":
        from vima_amd.baselines import build_baseline
        cfg = syn.BaselineConfig("gato", 256, 1, 8, vocab_size=8)
        pol = build_baseline(cfg, precision=prec, device=DEV)
        pol.load_state_dict(syn.make_baseline_state_dict(cfg, 3, head_gain=0.5), strict=True)
        for k, v in opts.items():
            pol.set_option(k, v)
        return pol
    cfg = syn.config(model)
    return loaded_policy(cfg, syn.make_state_dict(cfg, 3, head_gain=0.5), prec, **opts)


def _tokens(pol, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, pol.embed_dim, generator=g).to(DEV)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("model", ["2M", "20M", "gato"])
def test_act_is_bit_equal_to_the_entry_points_it_chains(model, prec):
    from vima_amd.actions import select_actions
    pol = _policy(model, prec)
    for shape in ((1, 3), (2, 37)):                             # 3 rows: the skinny GEMMs; 74 rows: the tile kernels
        tok = _tokens(pol, shape, 11)
        logits = pol.action_logits(tok)
        out = pol.act(tok, action_bounds={"low": LOW, "high": HIGH}, return_logits=True)
        assert out.logits.shape == (*shape, 700) and torch.equal(out.logits, logits)
        want = select_actions(logits, action_bounds={"low": LOW, "high": HIGH})
        for k, w in zip(ref.KEYS, ref.KEY_DIMS):
            assert out.actions[k].shape == (*shape, w) and out.actions[k].dtype == torch.int64
            assert torch.equal(out.actions[k], want.actions[k]), k
            assert torch.equal(out.continuous[k], want.continuous[k]), k
            assert torch.equal(out.log_prob[k], want.log_prob[k]) and torch.equal(out.entropy[k], want.entropy[k]), k
            assert out.log_prob[k].shape == shape
        assert np.array_equal(_bins(out), ref.argmax_bins(logits.reshape(-1, 700).cpu().numpy()))
        assert out.action_token.shape == (*shape, pol.embed_dim)
        assert torch.equal(out.action_token, pol.forward_action_token(out.actions))
        # sampled: the same three identities, and the host-side distribution objects agree on log_prob / entropy
        g = torch.Generator(device=DEV).manual_seed(5)
        u = torch.rand(shape[0] * shape[1], 12, generator=g, device=DEV)
        outs = pol.act(tok, uniforms=u)
        wants = select_actions(logits, uniforms=u)
        dists = pol.forward_action_decoder(tok)
        tol = 2 * 2e-5 * 18.5      # two fp32 evaluations, each within 2e-5 max(1, |ref|) of the exact value, |ref| <= 4 ln 100 = 18.4
        for k in ref.KEYS:
            assert torch.equal(outs.actions[k], wants.actions[k]), k
            assert torch.allclose(outs.log_prob[k], dists[k].log_prob(outs.actions[k]), rtol=0, atol=tol), k
            assert torch.allclose(outs.entropy[k], dists[k].entropy(), rtol=0, atol=tol), k
        assert torch.equal(outs.action_token, pol.forward_action_token(outs.actions))
        assert not all(torch.equal(outs.actions[k], out.actions[k]) for k in ref.KEYS)
        g1, g2 = torch.Generator(device=DEV).manual_seed(9), torch.Generator(device=DEV).manual_seed(9)
        a, b = pol.act(tok, sample=True, generator=g1), pol.act(tok, sample=True, generator=g2)
        assert all(torch.equal(a.actions[k], b.actions[k]) for k in ref.KEYS)
        assert a.logits is None
    del pol


def _raw_act(pol, tok, u, bufs, bounds=None):
    """vima_act through ctypes on FIXED buffers (the graph key holds every pointer)."""
    from vima_amd import _lib
    from vima_amd.actions import bounds_array
    logits, idx, cont, logp, ent, token = bufs
    arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in idx])
    _lib.check(pol._lib.vima_act(pol._handle, ptr(tok), tok.shape[0], ptr(u), bounds_array(bounds), ptr(logits), arr, ptr(cont), ptr(logp),
                                 ptr(ent), ptr(token), pol._stream()))
    torch.cuda.synchronize()
    return [t.clone() for t in (logits, *idx, cont, logp, ent, token)]


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("model", ["2M", "gato"])
def test_act_under_graph_replay(model, prec):
    from vima_amd.actions import alloc_outputs
    pol = _policy(model, prec, graphs=1)
    R = 5
    tok = _tokens(pol, (R,), 21)
    g = torch.Generator(device=DEV).manual_seed(1)
    u = torch.rand(R, 12, generator=g, device=DEV)
    idx, cont, logp, ent = alloc_outputs(R, DEV)
    bufs = (torch.empty(R, 700, device=DEV), idx, cont, logp, ent, torch.empty(R, pol.embed_dim, device=DEV))
    bounds = {"low": LOW, "high": HIGH}
    pol.act(tok, uniforms=u.clone(), action_bounds=bounds, return_logits=True)   # sizes the workspace (its generation is part of every key)
    r0, c0 = pol.graph_stats()
    eager = _raw_act(pol, tok, u, bufs, bounds)
    capture = _raw_act(pol, tok, u, bufs, bounds)
    replay = _raw_act(pol, tok, u, bufs, bounds)
    r1, c1 = pol.graph_stats()
    assert c1 == c0 + 1 and r1 == r0 + 1, (r0, c0, r1, c1)
    for a, b, c in zip(eager, capture, replay):
        assert torch.equal(a, b) and torch.equal(a, c)
    u2 = torch.rand(R, 12, generator=g, device=DEV)
    u.copy_(u2)                                                  # new uniforms in place: the replay reads them from memory
    again = _raw_act(pol, tok, u, bufs, bounds)
    r2, c2 = pol.graph_stats()
    assert c2 == c1 and r2 == r1 + 1
    fresh = pol.act(tok, uniforms=u2.clone(), action_bounds=bounds, return_logits=True)
    want = [fresh.logits, *[fresh.actions[k] for k in ref.KEYS]]
    for a, b in zip(again[:5], want):
        assert torch.equal(a, b)
    assert torch.equal(again[-1], fresh.action_token)
    assert not all(torch.equal(a, b) for a, b in zip(again[1:5], replay[1:5]))
    other = _raw_act(pol, tok, u, bufs, {"low": [0.0, 0.0], "high": [1.0, 1.0]})     # other bound VALUES: another key, not the captured graph
    assert pol.graph_stats()[0] == r2
    assert not torch.equal(other[5], again[5]) and torch.equal(other[1], again[1])
    del pol


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("model,rows", [("2M", 1), ("20M", 32), ("gato", 256)])
def test_act_replaces_the_action_l1_launches(model, rows, prec):
    pol = _policy(model, prec)
    tok = _tokens(pol, (1, rows), 31)
    out = pol.act(tok)                                           # warm: workspace, code objects
    pol.prof_enable(True)
    pol.prof_read()
    pol.action_logits(tok)
    head = pol.prof_read()
    pol.forward_action_token(out.actions)
    embed = pol.prof_read()
    pol.act(tok)
    act = pol.prof_read()
    pol.prof_enable(False)
    n = {k: (head[k]["launches"], embed[k]["launches"], act[k]["launches"]) for k in ("gemm", "attention", "other")}
    print(f"[act] {model} {prec} rows {rows}: launches (action_head, action_embed, act) = {n}")
    assert n["other"][2] == n["other"][0] + 1                    # the one act_select launch
    assert n["gemm"][2] == n["gemm"][0] + n["gemm"][1]
    assert n["attention"] == (0, 0, 0)
    assert n["other"][1] > 1                                     # so the chained call launches less than the two calls it replaces
    del pol


# ------------------------------------------------------------------------------------------ closed loop
@pytest.mark.parametrize("incremental", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_eval_loop_with_device_actions_takes_the_reference_actions(precision, incremental):
    """The set-up of tests/test_eval_loop.py::test_reference_eval_loop_on_the_gpu_takes_the_reference_actions with
    device_actions=True: same golden discrete trace, and the continuous actions the environment receives are the stored
    reference run's, array for array."""
    from oracle import eval_loop
    import reference_loop
    from vima_amd.policy import VIMAPolicy
    from vima_amd.preprocess import prepare_obs, prepare_prompt_images
    MODEL, STEPS, N_OBJ, ENV_SEED, WSEED = "20M", 6, 4, 3, 7
    MISSING = {2: (3,), 4: (2, 5)}
    gold = np.load(os.path.join(ROOT, "tests", "golden", "eval_loop_20M.npz"))
    _, actions_ref = eval_loop.load_log(os.path.join(ROOT, "tests", "golden", "eval_loop_20M_calls.npz"))
    cfg = syn.config(MODEL)
    pol = VIMAPolicy(**cfg.ctor_kwargs(), precision=precision, device=DEV)
    pol.load_state_dict(syn.make_state_dict(cfg, WSEED, head_gain=0.5), strict=True)
    env = eval_loop.SyntheticEnv(n_steps=STEPS, n_obj=N_OBJ, seed=ENV_SEED, missing_at=MISSING)
    with torch.no_grad():
        recs = reference_loop.run_episode(pol, env, tokenizer=eval_loop.FixedTokenizer(), placeholders=eval_loop.placeholders(),
                                          prepare_obs=prepare_obs, prepare_prompt_images=prepare_prompt_images, device=DEV,
                                          incremental=incremental, device_actions=True)
    got = {k: np.stack([r["discrete"][k].numpy() for r in recs]) for k in ref.KEYS}
    total = sum(gold[k].size for k in ref.KEYS)
    agree = sum(int((got[k] == gold[k]).sum()) for k in ref.KEYS)
    first_diff = next((t for t in range(STEPS) if any((got[k][t] != gold[k][t]).any() for k in ref.KEYS)), STEPS)
    print(f"[act] eval loop, device actions, {precision} {'forward_step' if incremental else 'forward'}: {agree}/{total} discrete action "
          f"dimensions equal to the reference's; identical for the first {first_diff} steps")
    assert len(env.actions) == STEPS == len(actions_ref)
    if precision == "fp32":
        assert agree == total
        for a, b in zip(actions_ref, env.actions):
            for k in ref.KEYS:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    else:
        assert first_diff >= 1 and agree >= 0.8 * total
    for t, a in enumerate(env.actions):                          # in every precision: what the environment got IS the rescaled bins
        bins = np.concatenate([got[k][t] for k in ref.KEYS])[None]
        assert np.array_equal(np.concatenate([a[k] for k in ref.KEYS]), ref.rescale_cpu(bins, LOW, HIGH)[0])
