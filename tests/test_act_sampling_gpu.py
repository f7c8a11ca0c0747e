"""Sampling controls and action scoring on the MI355X: vima_action_select_ex (`actions.select_actions(..., temperature=, top_k=,
top_p=, n_samples=)`, `actions.score_actions`) and vima_act_ex (`VIMAPolicy.act(...)` with the same keywords,
`VIMAPolicy.evaluate_actions`) against the fp64 restatement of tests/act_sampling_reference.py, and bit for bit against the default
entry points they extend. Inputs, exemptions and gates are in tests/act_sampling_reference.py; tests/test_act_sampling_build.py bounds
the exempt share (at most 1 % of the pairs of each of the 192 combinations) on the CPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import act_reference as ref                       # noqa: E402
from tests import act_sampling_reference as sref             # noqa: E402
from tests.gpu_common import loaded_policy, ptr              # noqa: E402
from vima_testing import synthetic as syn                    # noqa: E402
from vima_amd import _lib                                    # noqa: E402
from vima_amd import actions as A                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDS = {"low": [0.25, -0.5], "high": [0.75, 0.5]}
TOP = np.array(ref.BINS) - 1


def _bins(sel):
    return torch.cat([sel.actions[k].reshape(-1, w) for k, w in zip(ref.KEYS, ref.KEY_DIMS)], dim=1).cpu().numpy()


def _per_key(d):
    return torch.stack([d[k].reshape(-1) for k in ref.KEYS], dim=1).cpu().numpy().astype(np.float64)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # a copy: the shared inputs are read-only


def _actions_of(bins):
    return {k: _dev(bins[:, f:f + w].astype(np.int64)) for k, f, w in zip(ref.KEYS, ref.KEY_FIRST, ref.KEY_DIMS)}


def _same(a, b, what=("actions", "continuous", "log_prob", "entropy")):
    """bit for bit (NaN-free outputs; -inf compares equal to itself)"""
    for field in what:
        for k in ref.KEYS:
            assert torch.equal(getattr(a, field)[k].reshape(-1), getattr(b, field)[k].reshape(-1)), (field, k)


def _raw_select_ex(x, u, opts, bounds=None, idx=None, R=None):
    """vima_action_select_ex through ctypes -> (return code, idx list, cont, log_prob, entropy); outputs pre-filled with sentinels"""
    lib = _lib.load()
    R = x.shape[0] if R is None else R
    S = max(opts.n_samples, 1) if opts is not None else 1
    own = idx is None
    if own:
        idx = [torch.full((R * S, w), -7, dtype=torch.int64, device=DEV) for w in ref.KEY_DIMS]
    cont, logp, ent = (torch.full((R * S, n), -7.0, device=DEV) for n in (12, 4, 4))
    arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in idx])            # idx == []: four null pointers
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.vima_action_select_ex(ptr(x), R, ptr(u), ctypes.byref(opts) if opts is not None else None, A.bounds_array(bounds), arr,
                                   ptr(cont), ptr(logp), ptr(ent), stream)
    torch.cuda.synchronize()
    return rc, idx, cont, logp, ent


def _opts(temp=None, k=0, p=1.0, S=1, given=0):
    return _lib.VimaSampleOpts(temp.data_ptr() if temp is not None else None, k, p, S, given)


# ------------------------------------------------------------------------------------------ 1. defaults are the old path
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("bounds", [None, BOUNDS])
def test_defaults_equal_vima_action_select_bit_for_bit(sampled, bounds):
    x = _dev(sref.logits("random", 1.0))
    u = _dev(sref.uniforms()) if sampled else None
    old = A.select_actions(x, u, bounds)                    # all defaults: vima_action_select
    want = [old.actions[k] for k in ref.KEYS]
    ones = torch.ones(x.shape[0], device=DEV)
    for tag, o in (("NULL", None), ("explicit defaults", _opts()), ("controls that keep every bin", _opts(ones, 100, 1.0))):
        rc, idx, cont, logp, ent = _raw_select_ex(x, u, o, bounds)
        assert rc == 0, tag
        for a, b in zip(idx, want):
            assert torch.equal(a, b), tag
        assert torch.equal(cont, torch.cat([old.continuous[k] for k in ref.KEYS], dim=1)), tag
        assert torch.equal(logp, torch.stack([old.log_prob[k] for k in ref.KEYS], dim=1)), tag
        assert torch.equal(ent, torch.stack([old.entropy[k] for k in ref.KEYS], dim=1)), tag


def _policy(prec, model="4M", **opts):
    cfg = syn.config(model)
    return loaded_policy(cfg, syn.make_state_dict(cfg, 3, head_gain=0.5), prec, **opts)


def _tokens(pol, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, pol.embed_dim, generator=g).to(DEV)


def _raw_act(pol, tok, u, bufs, bounds=None, opts=None, ex=True):
    """vima_act_ex (or vima_act) through ctypes on FIXED buffers (the graph key holds every pointer)"""
    logits, idx, cont, logp, ent, token = bufs
    arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in idx])
    if ex:
        rc = pol._lib.vima_act_ex(pol._handle, ptr(tok), tok.shape[0], ptr(u), ctypes.byref(opts) if opts is not None else None,
                                  A.bounds_array(bounds), ptr(logits), arr, ptr(cont), ptr(logp), ptr(ent), ptr(token), pol._stream())
    else:
        rc = pol._lib.vima_act(pol._handle, ptr(tok), tok.shape[0], ptr(u), A.bounds_array(bounds), ptr(logits), arr, ptr(cont),
                               ptr(logp), ptr(ent), ptr(token), pol._stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    return [t.clone() for t in (logits, *idx, cont, logp, ent, token)]


def _bufs(pol, R, S=1):
    idx, cont, logp, ent = A.alloc_outputs(R * S, DEV)
    return (torch.empty(R, 700, device=DEV), idx, cont, logp, ent, torch.empty(R * S, pol.embed_dim, device=DEV))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_act_ex_defaults_equal_vima_act_bit_for_bit(prec):
    pol = _policy(prec)
    R = 37
    tok = _tokens(pol, (R,), 11)
    g = torch.Generator(device=DEV).manual_seed(5)
    for u in (None, torch.rand(R, 12, generator=g, device=DEV)):
        old = _raw_act(pol, tok, u, _bufs(pol, R), BOUNDS, ex=False)
        for o in (None, _opts()):
            new = _raw_act(pol, tok, u, _bufs(pol, R), BOUNDS, o)
            for a, b in zip(old, new):                      # logits, 4 x idx, cont, log_prob, entropy, token
                assert torch.equal(a, b)
    del pol


# ------------------------------------------------------------------------------------------ 2. / 4. kept set, sampling, statistics
_gpu_cache = {}


def _gpu(kind, scale, tname, k, p):
    """one launch per combination, shared by the tests below: bins [256,12], per-key log_prob / entropy [256,4]"""
    key = (kind, scale, tname, k, p)
    if key not in _gpu_cache:
        sel = A.select_actions(_dev(sref.logits(kind, scale)), _dev(sref.uniforms()), temperature=_dev(sref.temperature(tname)),
                               top_k=k, top_p=p)
        _gpu_cache[key] = (_bins(sel), _per_key(sel.log_prob), _per_key(sel.entropy))
    return _gpu_cache[key]


@pytest.mark.parametrize("kind,scale", sref.INPUTS)
def test_kept_set_and_sampling_equal_the_fp64_reference(kind, scale):
    z_argmax = {t: ref.argmax_bins(sref.scaled(sref.logits(kind, scale), sref.temperature(t))) for t in sref.TEMPERATURES}
    n_exempt = n_diff = 0
    for tname in sref.TEMPERATURES:
        for k, p in sref.KP:
            r = sref.combination(kind, scale, tname, k, p)
            bins, _, _ = _gpu(kind, scale, tname, k, p)
            assert bins.min() >= 0 and (bins <= TOP).all()
            diff = bins != r["bins"]
            n_exempt += int(r["exempt"].sum())
            n_diff += int(diff.sum())
            assert r["exempt"].mean() <= 0.01
            assert not (diff & ~r["exempt"]).any(), (tname, k, p, int((diff & ~r["exempt"]).sum()))
            # every selected bin lies in the reference's kept set: without top-p the set is decided by exact comparisons, so on every
            # pair; with top-p on the pairs whose set is not decided below fp32 resolution
            ok = ~r["exempt"] if p < 1.0 else np.ones_like(r["exempt"])
            for d in range(12):
                inside = np.take_along_axis(r["keep"][d], bins[:, d:d + 1], axis=1)[:, 0]
                assert inside[ok[:, d]].all(), (tname, k, p, d)
            if k == 1:                                      # whatever u
                assert np.array_equal(bins, z_argmax[tname])
    print(f"[act-sampling] {kind} scale {scale}: {n_exempt} of {32 * 3072} pairs exempt over 32 combinations, {n_diff} bins differ from "
          f"fp64, all of them exempt")


@pytest.mark.parametrize("kind,scale", sref.INPUTS)
def test_statistics_of_the_truncated_distribution(kind, scale):
    """per-key log_prob (of the sampled bins) and entropy against fp64 on non-exempt keys:
    |err| <= 2e-5 * max(1, |ref|, sum over the key's dimensions of max |z|)"""
    worst = {"log_prob": 0.0, "entropy": 0.0}
    for tname in sref.TEMPERATURES:
        for k, p in sref.KP:
            r = sref.combination(kind, scale, tname, k, p)
            _, lp, en = _gpu(kind, scale, tname, k, p)
            ok = ~r["exempt_key"]
            for what, got, want in (("log_prob", lp, r["log_prob"]), ("entropy", en, r["entropy"])):
                assert np.isfinite(got[ok]).all() and np.isfinite(want[ok]).all(), (what, tname, k, p)
                ratio = np.abs(got - want)[ok] / sref.stat_bound(want, r["zmax_key"])[ok]
                worst[what] = max(worst[what], float(ratio.max()))
                assert ratio.max() <= 1.0, (what, tname, k, p, float(ratio.max()))
    print(f"[act-sampling] {kind} scale {scale}: max error / gate over 32 combinations: log_prob {worst['log_prob']:.3f}, "
          f"entropy {worst['entropy']:.3f} (gate 2e-5 max(1, |ref|, sum max |z|))")


# ------------------------------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("scale", sref.SCALES)
def test_ties_go_to_the_lower_index(scale):
    """Quantised logits, k = 5: over 4096 fresh uniforms per row (the same for each of the 12 dimensions) the SET of sampled bins is the
    reference's kept set exactly, so among equal logits at the k-th place the lower indices are the ones kept."""
    x = sref.logits("quantised", scale)[:4]
    g = torch.Generator().manual_seed(77)
    # one fresh uniform in each of the 4096 strata [i, i + 1) / 4096: every bin of probability >= 2 / 4096 is drawn, whatever the seed
    u = ((torch.arange(4096)[None, :, None] + torch.rand(4, 4096, 1, generator=g)) / 4096).expand(4, 4096, 12).contiguous()
    sel = A.select_actions(_dev(x), u.to(DEV), top_k=5, n_samples=4096)
    bins = _bins(sel).reshape(4, 4096, 12)
    r = sref.reference(x, None, None, 5, 1.0)
    tied = 0
    for d in range(12):
        zs = ref.segments(x)[d]
        for row in range(4):
            want = np.flatnonzero(r["keep"][d][row])
            assert len(want) == 5 and r["pi"][d][row][want].min() >= 2.0 / 4096
            assert np.array_equal(np.unique(bins[row, :, d]), want), (row, d)
            tied += int((zs[row] == zs[row][want].min()).sum() > (zs[row][want] == zs[row][want].min()).sum())
    print(f"[act-sampling] ties, quantised scale {scale}: {tied} of 48 (row, dimension) pairs have a tie across the k-th place")
    assert tied > 0


# ------------------------------------------------------------------------------------------ 5. given actions
def test_score_actions_defaults_are_the_raw_head_statistics():
    x = sref.logits("random", 1.0)
    bins, _ = ref.sample_bins64(x, sref.uniforms())
    sc = A.score_actions(_dev(x), _actions_of(bins))
    assert np.array_equal(_bins(sc), bins)
    lp64, en64 = ref.stats64(x, bins)
    zmax = sref.reference(x)["zmax_key"]
    for what, got, want in (("log_prob", _per_key(sc.log_prob), lp64), ("entropy", _per_key(sc.entropy), en64)):
        ratio = np.abs(got - want) / sref.stat_bound(want, zmax)
        print(f"[act-sampling] score_actions defaults, {what}: max error / gate {ratio.max():.3f}")
        assert np.isfinite(got).all() and ratio.max() <= 1.0
    assert np.array_equal(torch.cat([sc.continuous[k] for k in ref.KEYS], dim=1).cpu().numpy(), ref.de_discretize_cpu(bins))


@pytest.mark.parametrize("controls", [{}, {"temperature": 0.7, "top_k": 10, "top_p": 0.9}, {"temperature": 3.0, "top_k": 50}])
def test_score_actions_reproduces_the_selection_bit_for_bit(controls):
    x, u = _dev(sref.logits("random", 4.0)), _dev(sref.uniforms())
    for uu in (None, u):
        sel = A.select_actions(x, uu, BOUNDS, **controls)
        sc = A.score_actions(x, sel.actions, action_bounds=BOUNDS, **controls)
        _same(sel, sc)


def test_score_actions_outside_the_kept_set_and_out_of_range():
    x = sref.logits("random", 1.0)
    r = sref.reference(x, None, None, 5, 1.0)
    worst = np.stack([s.argmin(axis=1) for s in ref.segments(x)], axis=1)       # never among the five largest
    sc = A.score_actions(_dev(x), _actions_of(worst), top_k=5)
    lp = _per_key(sc.log_prob)
    assert np.isneginf(lp).all() and np.isfinite(_per_key(sc.entropy)).all()
    mixed = worst.copy()
    mixed[:, 2:] = r["bins"][:, 2:]                                             # only pose0_position holds removed bins
    lp = _per_key(A.score_actions(_dev(x), _actions_of(mixed), top_k=5).log_prob)
    assert np.isneginf(lp[:, 0]).all() and np.isfinite(lp[:, 1:]).all()
    low, high = np.full((256, 12), -5), np.full((256, 12), 1000)
    for given, clamped in ((low, np.zeros((256, 12), dtype=np.int64)), (high, np.broadcast_to(TOP, (256, 12)).copy())):
        acts = _actions_of(given)
        a, b = A.score_actions(_dev(x), acts, action_bounds=BOUNDS), A.score_actions(_dev(x), _actions_of(clamped), action_bounds=BOUNDS)
        _same(a, b, what=("continuous", "log_prob", "entropy"))
        assert np.array_equal(_bins(a), given)                                  # the given bins are left as they are


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("controls", [{}, {"temperature": 0.7, "top_k": 10, "top_p": 0.9}])
def test_evaluate_actions_reproduces_act_bit_for_bit(prec, controls):
    pol = _policy(prec)
    tok = _tokens(pol, (2, 37), 13)
    g = torch.Generator(device=DEV).manual_seed(3)
    for sample in (False, True):
        out = pol.act(tok, sample=sample, generator=g, action_bounds=BOUNDS, **controls)
        ev = pol.evaluate_actions(tok, out.actions, action_bounds=BOUNDS, **controls)
        _same(out, ev)
        assert ev.log_prob["pose0_position"].shape == (2, 37) and ev.action_token.shape == (2, 37, pol.embed_dim)
        assert torch.equal(ev.action_token, out.action_token)
        assert torch.equal(ev.action_token, pol.forward_action_token(out.actions))
    del pol


# ------------------------------------------------------------------------------------------ 6. candidates
def test_candidates_are_single_sample_calls():
    x = _dev(sref.logits("random", 1.0)[:32])
    T = _dev(sref.temperature("mix")[:32])
    g = torch.Generator().manual_seed(9)
    u = torch.rand(32, 4, 12, generator=g).to(DEV)
    many = A.select_actions(x, u, BOUNDS, temperature=T, top_k=10, top_p=0.9, n_samples=4)
    assert many.actions["pose0_rotation"].shape == (32, 4, 4) and many.log_prob["pose0_rotation"].shape == (32, 4)
    for s in range(4):
        one = A.select_actions(x, u[:, s].contiguous(), BOUNDS, temperature=T, top_k=10, top_p=0.9)
        for field in ("actions", "continuous", "log_prob", "entropy"):
            for k in ref.KEYS:
                assert torch.equal(getattr(many, field)[k][:, s], getattr(one, field)[k]), (s, field, k)
    assert not torch.equal(many.actions["pose0_rotation"][:, 0], many.actions["pose0_rotation"][:, 1])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_act_candidates_share_one_pass_of_the_action_head(prec):
    pol = _policy(prec)
    R, S = 6, 4
    tok = _tokens(pol, (2, 3), 17)
    g = torch.Generator(device=DEV).manual_seed(4)
    u = torch.rand(2, 3, S, 12, generator=g, device=DEV)
    kw = dict(temperature=0.7, top_k=10, action_bounds=BOUNDS)
    many = pol.act(tok, uniforms=u, n_samples=S, return_logits=True, **kw)
    assert many.action_token.shape == (2, 3, S, pol.embed_dim) and many.logits.shape == (2, 3, 700)
    assert torch.equal(many.logits, pol.action_logits(tok))
    for s in range(S):
        one = pol.act(tok, uniforms=u[:, :, s].contiguous(), **kw)
        for field in ("actions", "continuous", "log_prob", "entropy"):
            for k in ref.KEYS:
                assert torch.equal(getattr(many, field)[k][:, :, s], getattr(one, field)[k]), (s, field, k)
        acts = {k: many.actions[k][:, :, s].contiguous() for k in ref.KEYS}
        assert torch.equal(many.action_token[:, :, s], pol.forward_action_token(acts))
    drawn = pol.act(tok, sample=True, n_samples=S, generator=g, **kw)      # uniforms drawn on the device
    assert drawn.actions["pose1_rotation"].shape == (2, 3, S, 4)
    pol.prof_enable(True)
    pol.prof_read()
    pol.act(tok, uniforms=u[:, :, 0].contiguous(), **kw)
    single = pol.prof_read_gemm_launches()
    pol.prof_read()
    pol.act(tok, uniforms=u, n_samples=S, **kw)
    cand = pol.prof_read_gemm_launches()
    n_other = pol.prof_read()["other"]["launches"]
    pol.action_logits(tok)
    head = pol.prof_read_gemm_launches()
    pol.prof_read()
    pol.prof_enable(False)
    print(f"[act-sampling] {prec}: GEMM launches: action head {len(head)}, act {len(single)}, act with {S} candidates {len(cand)}")
    assert len(cand) == len(single)                                       # the head runs once, on R rows
    assert [l["M"] for l in cand[:len(head)]] == [R] * len(head) and all(l["M"] == R * S for l in cand[len(head):])
    assert len(cand) > len(head) and n_other >= 1
    del pol


# ------------------------------------------------------------------------------------------ 7. edge inputs
def _edge_logits():
    x = np.zeros((2, 700), dtype=np.float32)
    x[0, 0::2], x[0, 1::2] = 1e4, -1e4
    x[1] = ref.random_logits(4.0, rows=1)[0]
    x[1, 50:150] = 0.5                                       # a segment of equal logits
    return x


@pytest.mark.parametrize("k,p", [(0, 1.0), (1000, 1.0), (3, 1.0), (0, 1e-6), (7, 0.5)])
def test_edge_inputs_keep_bins_in_range_and_outputs_finite(k, p):
    x = _dev(_edge_logits())
    for tval in (0.0, -1.0, float("nan"), 1e-9, 1e9, 1.0):
        T = torch.full((2,), tval, device=DEV)
        for uval in (-1.0, 0.0, 1.0, 2.0, float("nan"), None):
            u = None if uval is None else torch.full((2, 12), uval, device=DEV)
            sel = A.select_actions(x, u, BOUNDS, temperature=T, top_k=k, top_p=p)
            bins = _bins(sel)
            assert bins.min() >= 0 and (bins <= TOP).all(), (tval, uval)
            for field in (sel.log_prob, sel.entropy, sel.continuous):
                assert all(torch.isfinite(v).all() for v in field.values()), (tval, uval)
            if uval in (0.0, -1.0, None) or (uval is not None and uval != uval):
                assert bins[1, 1] == 0                       # equal logits: the first bin (also the first of K)
            elif 0 < k < 100:                                # K is the first bins of the flat segment (top-p 0.5 of 7 keeps 4: 3/7 < 0.5 <= 4/7)
                assert bins[1, 1] == (k - 1 if p >= 1.0 else 3)          # u = 1 takes the last bin of K
            elif p < 1e-3:
                assert bins[1, 1] == 0
            sc = A.score_actions(x, sel.actions, temperature=T, top_k=k, top_p=p, action_bounds=BOUNDS)
            _same(sel, sc)


def test_host_side_refusals_launch_nothing():
    x = _dev(sref.logits("random", 1.0)[:2])
    bad = (_opts(p=0.0), _opts(p=-0.5), _opts(p=float("nan")), _opts(S=0), _opts(S=2, given=1))
    for o in bad:
        rc, idx, cont, logp, ent = _raw_select_ex(x, None, o)
        assert rc != 0 and _lib.load().vima_last_error()
        assert all((t == -7).all() for t in (*idx, cont, logp, ent)), "an output was written"
    rc, _, cont, logp, ent = _raw_select_ex(x, None, _opts(), idx=[])
    assert rc != 0 and all((t == -7).all() for t in (cont, logp, ent))
    with pytest.raises(Exception):
        A.select_actions(x, top_p=0.0)
    with pytest.raises(Exception):
        A.select_actions(x, n_samples=0)
    pol = _policy("fp32", model="2M")
    tok = _tokens(pol, (2,), 1)
    for o in bad:
        bufs = _bufs(pol, 2, max(o.n_samples, 1))
        for t in bufs[2:5]:
            t.fill_(-7.0)
        arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in bufs[1]])
        rc = pol._lib.vima_act_ex(pol._handle, ptr(tok), 2, None, ctypes.byref(o), None, None, arr, ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]),
                                  ptr(bufs[5]), pol._stream())
        torch.cuda.synchronize()
        assert rc != 0 and all((t == -7).all() for t in bufs[2:5])
    del pol


# ------------------------------------------------------------------------------------------ 8. graph replay
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_act_ex_under_graph_replay(prec):
    pol = _policy(prec, model="2M", graphs=1)
    R, S = 5, 2
    tok = _tokens(pol, (R,), 21)
    g = torch.Generator(device=DEV).manual_seed(1)
    u = torch.rand(R * S, 12, generator=g, device=DEV)
    T = torch.full((R,), 0.7, device=DEV)
    bufs = _bufs(pol, R, S)
    kw = dict(top_k=10, top_p=0.9, n_samples=S, action_bounds=BOUNDS, return_logits=True)
    pol.act(tok, uniforms=u.clone(), temperature=T.clone(), **kw)          # sizes the workspace (its generation is part of every key)
    o = _opts(T, 10, 0.9, S)
    r0, c0 = pol.graph_stats()
    eager = _raw_act(pol, tok, u, bufs, BOUNDS, o)
    capture = _raw_act(pol, tok, u, bufs, BOUNDS, o)
    replay = _raw_act(pol, tok, u, bufs, BOUNDS, o)
    r1, c1 = pol.graph_stats()
    assert c1 == c0 + 1 and r1 == r0 + 1, (r0, c0, r1, c1)
    for a, b, c in zip(eager, capture, replay):
        assert torch.equal(a, b) and torch.equal(a, c)
    u2, T2 = torch.rand(R * S, 12, generator=g, device=DEV), torch.tensor([0.3, 1.0, 2.5, 0.7, 5.0], device=DEV)
    u.copy_(u2)                                                            # new values in place: the replay reads them from memory
    T.copy_(T2)
    again = _raw_act(pol, tok, u, bufs, BOUNDS, o)
    r2, c2 = pol.graph_stats()
    assert c2 == c1 and r2 == r1 + 1
    fresh = pol.act(tok, uniforms=u2.clone(), temperature=T2.clone(), **kw)
    for a, b in zip(again[:5], [fresh.logits, *[fresh.actions[k].reshape(R * S, -1) for k in ref.KEYS]]):
        assert torch.equal(a, b)
    assert torch.equal(again[6], torch.stack([fresh.log_prob[k].reshape(-1) for k in ref.KEYS], dim=1))
    assert torch.equal(again[-1], fresh.action_token.reshape(R * S, -1))
    assert not torch.equal(again[6], replay[6])
    r, c = r2, c2
    for other, S2 in ((_opts(T, 11, 0.9, S), S), (_opts(T, 10, 0.8, S), S), (_opts(T, 10, 0.9, 1), 1)):   # k, p, S: other keys
        b2 = bufs if S2 == S else (bufs[0], [t[:R] for t in bufs[1]], bufs[2][:R], bufs[3][:R], bufs[4][:R], bufs[5][:R])
        _raw_act(pol, tok, u, b2, BOUNDS, other)
        assert pol.graph_stats() == (r, c)                                 # seen once: runs eagerly, not the captured graph
        _raw_act(pol, tok, u, b2, BOUNDS, other)
        assert pol.graph_stats() == (r, c + 1)                             # seen twice: captured anew
        c += 1
    del pol
