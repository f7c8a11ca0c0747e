"""The norm and sequence-assembly kernels of elementwise.hip / baseline_kernels.hip / episode_rows.hip, one launch each through the operator entry points
(vima_op_norm, vima_op_prompt_assemble, vima_op_dec_embed, ... -- include/vima_hip.h), per output element against
tests/seq_norm_reference.py (references, cases and gates; tests/test_seq_norm_reference.py pins them on the CPU).

A  LayerNorm / RMSNorm / layernorm2 / rms_stats per element against fp64 inside the derived gates, both the fp32 and the operand-type output,
   every row stride, the routing between the half-wave-per-row and one-wave-per-row kernels, and the bit equalities the comments claim;
B  the exact kernels: outputs, masks and episode state bit for bit / integer for integer against the cumsum references, canaries intact;
C  the incremental forms against the whole-sequence forms, bit for bit;  E  refusals, with nothing written.
Float outputs are pre-filled with NaN or, where a region must stay untouched, with the canary."""
import ctypes
import os

import pytest
import torch

from tests import seq_norm_reference as R
from tests.gpu_common import bare_policy, ptr
from vima_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
_worst = {}


def dev(t, dtype=None):
    return None if t is None else t.to(DEV, dtype=dtype).contiguous()


def i32(seq):
    return torch.tensor(list(seq), dtype=torch.int32, device=DEV)


class _Args:
    """Device copies of the arguments of ONE call, kept alive until the call has returned: a(t) -> pointer (None -> NULL)."""

    def __init__(self):
        self.keep = []

    def __call__(self, t):
        if t is None:
            return ptr(None)
        self.keep.append(i32(t) if isinstance(t, (tuple, list)) else dev(t))
        return ptr(self.keep[-1])


def _call(fn, pol, *args):
    """-> (return code, message)."""
    rc = fn(pol._handle, *args, pol._stream())
    torch.cuda.synchronize()
    return rc, (pol._lib.vima_last_error().decode("utf-8", "replace") if rc else "")


def _ok(fn, pol, *args):
    rc, msg = _call(fn, pol, *args)
    assert rc == 0, msg


def _guarded(shape, fill, dtype=torch.float32, tail=64):
    """A flat device buffer of prod(shape) elements followed by `tail` canary elements -> (buffer, view of the shape)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + tail,), R.CANARY if dtype == torch.float32 else R.CANARY_U8, dtype=dtype, device=DEV)
    buf[:n] = fill.reshape(-1).to(DEV) if torch.is_tensor(fill) else fill
    return buf, buf[:n].view(*shape)


def _tail_intact(buf, n):
    want = R.CANARY if buf.dtype == torch.float32 else R.CANARY_U8
    assert (buf[n:] == want).all(), "a kernel wrote past the end of its output"


def _within(family, cid, out, ref, gate):
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{cid}: {int((~torch.isfinite(out)).sum())} non-finite outputs"
    ratio = (out.double() - ref).abs() / gate
    worst = ratio.max().item()
    if worst > _worst.get(family, (-1.0, ""))[0]:
        _worst[family] = (worst, cid)
    bad = ratio > 1.0
    assert not bad.any(), f"{cid} [{family}]: {int(bad.sum())} elements beyond the gate, worst {worst:.3f} x at {tuple(bad.nonzero()[0].tolist())}"


def _same(cid, what, got, want):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (cid, what, got.shape, want.shape)
    if got.dtype.is_floating_point:
        same = got.view(torch.int32) == want.view(torch.int32)
    else:
        same = got == want
    assert same.all(), f"{cid}: {what}: {int((~same).sum())} of {same.numel()} elements differ, first at {tuple((~same).nonzero()[0].tolist())}"


# ================================================================================================================== A  norms
def run_norm(prec, kind, x, ldin, g, b, eps, rms, rows, E, g2=None, b2=None, eps2=0.0, want32=True, wantT=True):
    """One vima_op_norm call -> dict of CPU tensors (out32, outT, out2T, ssq as requested), rc, msg."""
    pol = bare_policy(prec)
    d = _lib.VimaNormDesc()
    keep = {"x": dev(x), "gamma": dev(g), "beta": dev(b), "gamma2": dev(g2), "beta2": dev(b2)}
    outs = {}
    if kind == "rms_stats":
        outs["outT"], outs["ssq"] = torch.full((rows, E), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    else:
        if want32:
            outs["out32"] = torch.full((rows, E), NAN, device=DEV)
        if wantT:
            outs["outT"] = torch.full((rows, E), NAN, device=DEV)
        if kind == "ln2":
            outs["out2T"] = torch.full((rows, E), NAN, device=DEV)
    for k, t in list(keep.items()) + list(outs.items()):
        setattr(d, k, t.data_ptr() if t is not None else None)
    d.ldin, d.kind, d.rms, d.rows, d.E, d.eps, d.eps2 = ldin, _lib.NORM_KIND[kind], rms, rows, E, eps, eps2
    rc, msg = _call(pol._lib.vima_op_norm, pol, ctypes.byref(d))
    return {k: t.cpu() for k, t in outs.items()}, rc, msg


def run_ln_case(c, **kw):
    kind, prec, E, rows, pad, rms, regime = c
    full, g, b, g2, b2 = R.norm_inputs(E, rows, pad, regime)
    if kind == "ln2":
        out, rc, msg = run_norm(prec, kind, full, E + pad, g, b, R.LN_EPS, 0, rows, E, g2, b2, R.LN_EPS, **kw)
    else:
        out, rc, msg = run_norm(prec, kind, full, E + pad, g, None if rms else b, R.RMS_EPS if rms else R.LN_EPS, rms, rows, E, **kw)
    assert rc == 0, msg
    return out


def test_a_rows2_is_enabled():
    assert (os.environ.get("VIMA_LN_ROWS2") or "1")[0] != "0", "VIMA_LN_ROWS2=0 takes the half-wave-per-row kernel out of launch_layernorm_T"


@pytest.mark.parametrize("c", R.LN_CASES, ids=R.norm_case_id)
def test_a_layernorm_against_fp64_per_element(c):
    """Would fail: unbiased variance, eps dropped, the mean kept in the second pass, beta under rms, the rows of a rows2 pair swapped, an odd
    last row normalised with its neighbour's statistics, a pad column read (the mutations tests/test_seq_norm_reference.py holds the gates
    against), and any fp32 statistic looser than the summation depth allows."""
    kind, prec, E, rows, pad, rms, regime = c
    ref, g32, gT = R.ln_reference(c)
    out = run_ln_case(c)
    fam = f"{R.norm_kernel_of(kind, prec, E, E + pad)} {prec} {'rms' if rms else 'ln'} {regime}"
    _within(fam + " out32", R.norm_case_id(c), out["out32"], ref, g32)
    _within(fam + " outT", R.norm_case_id(c), out["outT"], ref, gT)
    if prec == "bf16":
        _same(R.norm_case_id(c), "outT is the bf16 rounding of out32", out["outT"], R.bf(out["out32"]))
    else:
        _same(R.norm_case_id(c), "outT is out32", out["outT"], out["out32"])


@pytest.mark.parametrize("c", R.LN2_CASES, ids=R.norm_case_id)
def test_a_layernorm2_against_fp64_and_two_launches(c):
    """All three outputs per element; then the kernel's claim: 'bit-identical' to two launches of layernorm_kernel, the second on the fp32 y."""
    kind, prec, E, rows, pad, _, regime = c
    y, g1, g1T, z, gzT = R.ln2_reference(c)
    out = run_ln_case(c)
    cid = R.norm_case_id(c)
    _within(f"layernorm2 {prec} {regime} y out32", cid, out["out32"], y, g1)
    _within(f"layernorm2 {prec} {regime} y outT", cid, out["outT"], y, g1T)
    _within(f"layernorm2 {prec} {regime} z out2T", cid, out["out2T"], z, gzT)
    full, g, b, g2, b2 = R.norm_inputs(E, rows, pad, regime)
    first, rc, msg = run_norm(prec, "ln", full, E + pad, g, b, R.LN_EPS, 0, rows, E)
    assert rc == 0, msg
    second, rc, msg = run_norm(prec, "ln", first["out32"], E, g2, b2, R.LN_EPS, 0, rows, E, want32=False)
    assert rc == 0, msg
    _same(cid, "y (fp32) of layernorm2 and of launch_layernorm", out["out32"], first["out32"])
    _same(cid, "y (operand type)", out["outT"], first["outT"])
    _same(cid, "z of layernorm2 and of the second launch_layernorm", out["out2T"], second["outT"])


@pytest.mark.parametrize("c", R.RMS_STATS_CASES, ids=R.norm_case_id)
def test_a_rms_stats_copy_and_ssq(c):
    _, prec, E, rows, _, _, regime = c
    x = R.norm_inputs(E, rows, 0, regime)[0]
    out, rc, msg = run_norm(prec, "rms_stats", x, E, None, None, 0.0, 1, rows, E)
    assert rc == 0, msg
    _same(R.norm_case_id(c), "operand-type copy", out["outT"], R.rounded(prec, x))
    ref, gate = R.ssq_reference(x)
    if regime == "zero":
        assert (out["ssq"] == 0).all()
    else:
        _within(f"rms_stats {prec} {regime} ssq", R.norm_case_id(c), out["ssq"], ref, gate)


@pytest.mark.parametrize("rms", [0, 1])
@pytest.mark.parametrize("E,rows", [(256, 33), (1024, 33), (768, 7)])
def test_a_routing_of_the_bf16_stream(E, rows, rms):
    """launch_layernorm_T on a bf16 stream: ldin = E + 4 must take the one-wave kernel layernorm_kernel<bf16, bf16>, whose arithmetic is
    layernorm_kernel<bf16, float>'s on the same (bf16-exact) values -- reached through launch_layernorm with no routing rule in the way:
    bit equality. ldin = E and E + 8 take rows2, whose sums run in another order: equal to each other bit for bit (the stride does not
    matter), and not to the one-wave kernel's bits."""
    b = None
    res = {}
    for pad in (0, 8, 4):
        full, g, beta, _, _ = R.norm_inputs(E, rows, pad, "plain")
        x = full.clone()
        x[:, :E] = R.norm_inputs(E, rows, 0, "plain")[0][:, :E]                        # the same rows at every stride
        b = None if rms else R.norm_inputs(E, rows, 0, "plain")[2]
        g = R.norm_inputs(E, rows, 0, "plain")[1]
        eps = R.RMS_EPS if rms else R.LN_EPS
        res[pad], rc, msg = run_norm("bf16", "ln_T", x, E + pad, g, b, eps, rms, rows, E)
        assert rc == 0, msg
        if pad == 4:
            res["one-wave"], rc, msg = run_norm("bf16", "ln", R.bf(x), E + pad, g, b, eps, rms, rows, E)
            assert rc == 0, msg
    assert R.norm_kernel_of("ln_T", "bf16", E, E + 4) == "layernorm_T" and R.norm_kernel_of("ln_T", "bf16", E, E + 8).startswith("rows2")
    for k in ("out32", "outT"):
        _same(f"E{E} rows{rows}", f"{k}: ldin = E + 4 is the one-wave kernel", res[4][k], res["one-wave"][k])
        _same(f"E{E} rows{rows}", f"{k}: rows2 at ldin = E and E + 8", res[0][k], res[8][k])
    if rows >= 33:   # 33 rows of sums taken in two orders: some statistic differs in its last bit
        assert not torch.equal(res[0]["out32"], res[4]["out32"]), "ldin = E gave the one-wave kernel's bits: rows2 was not taken"


# ================================================================================================================== B  exact kernels
def run_prompt_assemble(prec, src, word_ids, wt, ot, om, E, stats):
    pol = bare_policy(prec)
    rows = src.numel()
    xb, x = _guarded((rows, E), NAN)
    mb, m = _guarded((rows,), R.CANARY_U8, torch.uint8)
    ssq = torch.full((rows,), NAN, device=DEV)
    d = [dev(src), dev(word_ids), dev(wt), dev(ot), dev(om)]
    _ok(pol._lib.vima_op_prompt_assemble, pol, *(ptr(t) for t in d), rows, E, stats, ptr(xb), ptr(ssq), ptr(mb))
    _tail_intact(xb, rows * E), _tail_intact(mb, rows)
    return x.cpu(), m.cpu(), ssq.cpu()


@pytest.mark.parametrize("c", R.PA_CASES, ids=R.pa_case_id)
def test_b_prompt_assemble_and_its_stats_form(c):
    """Rows, masks bit for bit; the stats form: 'identical bits' with rms_stats on the assembled rows -- the rows AND ssq."""
    prec, E, B, L = c
    cid = R.pa_case_id(c)
    inp = R.pa_inputs(E, B, L)
    want_x, want_m = R.prompt_assemble_ref(*inp)
    x, m, _ = run_prompt_assemble(prec, *inp, E, 0)
    _same(cid, "rows", x, want_x), _same(cid, "mask", m, want_m)
    xs, ms, ssq = run_prompt_assemble(prec, *inp, E, 1)
    _same(cid, "operand-type rows of the stats form", xs, R.rounded(prec, want_x)), _same(cid, "mask of the stats form", ms, want_m)
    st, rc, msg = run_norm(prec, "rms_stats", x, E, None, None, 0.0, 1, B * L, E)
    assert rc == 0, msg
    _same(cid, "rows: prompt_assemble_stats vs rms_stats(prompt_assemble)", xs, st["outT"])
    _same(cid, "ssq: prompt_assemble_stats vs rms_stats(prompt_assemble)", ssq, st["ssq"])
    ref, gate = R.ssq_reference(want_x)
    nz = ref > 0
    _within(f"prompt_assemble_stats {prec} ssq", cid, ssq[nz], ref[nz], gate[nz])
    assert (ssq[~nz] == 0).all()


def run_dec_embed(prec, obs, mask, act, table, n_pos, T, B, Q, L_act, E):
    pol = bare_policy(prec)
    L = T * Q + L_act
    xb, x = _guarded((B, L, E), NAN)
    tb, xT = _guarded((B, L, E), NAN)
    mb, m = _guarded((B, L), R.CANARY_U8, torch.uint8)
    d = [dev(obs), dev(mask), dev(act), dev(table)]
    rc, msg = _call(pol._lib.vima_op_dec_embed, pol, *(ptr(t) for t in d), n_pos, T, B, Q, L_act, E, ptr(xb), ptr(tb), ptr(mb))
    for buf, n in ((xb, B * L * E), (tb, B * L * E), (mb, B * L)):
        _tail_intact(buf, n)
    return x.cpu(), xT.cpu(), m.cpu(), rc, msg


@pytest.mark.parametrize("c", R.DEC_CASES, ids=R.dec_case_id)
def test_b_dec_embed_and_gather_pred(c):
    """Would fail: position ids off by one, the cumsum restarted per step, a masked token consuming a position, either clamp missing, a
    token of another step / slot / sample. gather_pred on the result: rows Q - 1 + (Q + 1) t."""
    prec, E, B, T, Q, L_act, mkind = c
    cid = R.dec_case_id(c)
    obs, mask, act, table, n_pos = R.dec_inputs(E, B, T, Q, L_act, mkind)
    want, want_m, _ = R.dec_embed_ref(obs, mask, act, table, n_pos, L_act)
    x, xT, m, rc, msg = run_dec_embed(prec, obs, mask, act, table, n_pos, T, B, Q, L_act, E)
    assert rc == 0, msg
    _same(cid, "x32", x, want), _same(cid, "xT", xT, R.rounded(prec, want)), _same(cid, "mask", m, want_m)
    pol = bare_policy(prec)
    a = _Args()
    L = T * Q + L_act
    Tg = T                                                  # the last step's row Q - 1 exists with or without its action
    ob, o = _guarded((Tg, B, E), NAN)
    _ok(pol._lib.vima_op_gather_pred, pol, a(x), Tg, B, Q, L, E, ptr(ob))
    _tail_intact(ob, Tg * B * E)
    _same(cid, "gather_pred", o, R.gather_pred_ref(want, Tg, Q))


class _DecState:
    def __init__(self, B, Lmax):
        self.cpu = R.dec_state(B, Lmax)
        self.dev = {k: dev(v) for k, v in self.cpu.items()}

    def check(self, cid):
        for k in self.cpu:
            _same(cid, k, self.dev[k], self.cpu[k])


def run_dec_step(prec, st, obs, mask, act, table, n_pos, L_hist, Lmax, has_act):
    pol = bare_policy(prec)
    B, Q, E = obs.shape
    Ln = Q + has_act
    xb, x = _guarded((B, Ln, E), NAN)
    tb, xT = _guarded((B, Ln, E), NAN)
    d = [dev(obs), dev(mask), dev(act), dev(table)]
    rc, msg = _call(pol._lib.vima_op_dec_embed_step, pol, *(ptr(t) for t in d), n_pos, L_hist, Lmax, B, Q, has_act, E, ptr(xb), ptr(tb),
                    ptr(st["hist_mask"]), ptr(st["poscnt"]), ptr(st["fresh"]))
    _tail_intact(xb, B * Ln * E), _tail_intact(tb, B * Ln * E)
    return x.cpu(), xT.cpu(), rc, msg


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("E,B,Q,n_pos", [(256, 3, 4, 512), (320, 1, 1, 512), (768, 5, 4, 6)])
def test_b_dec_embed_step_chain_with_a_restart(E, B, Q, n_pos, prec):
    """Four env steps, every second sample restarted before step 2: rows and the episode state (hist_mask with its canary rows, poscnt,
    fresh) after every launch against the cumsum reference."""
    table, steps = R.dec_chain(E, B, Q, n_pos, restart_at=2)
    Lmax = 4 * (Q + 1) + 3
    st = _DecState(B, Lmax)
    pol = bare_policy(prec)
    a = _Args()
    L_hist = 0
    for t, (obs, mask, act, flags) in enumerate(steps):
        cid = f"dec_embed_step-{prec}-E{E}-B{B}-Q{Q}-step{t}"
        has_act = 1 if t else 0
        if flags is not None:
            R.restart_ref(st.cpu, flags)
            _ok(pol._lib.vima_op_restart_samples, pol, a(flags), ptr(st.dev["hist_mask"]), ptr(st.dev["poscnt"]), ptr(st.dev["fresh"]), B, Lmax)
            st.check(cid + " restart")
        want = R.dec_step_ref(st.cpu, obs, mask, act, table, n_pos, L_hist, has_act)
        x, xT, rc, msg = run_dec_step(prec, st.dev, obs, mask, act, table, n_pos, L_hist, Lmax, has_act)
        assert rc == 0, msg
        _same(cid, "x32", x, want), _same(cid, "xT", xT, R.rounded(prec, want))
        st.check(cid)
        L_hist += Q + has_act


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("E,B,Q,n_pos", [(256, 3, 4, 512), (768, 5, 4, 6)])
def test_c_dec_embed_step_rows_are_dec_embed_rows(E, B, Q, n_pos, prec):
    """Without a restart the rows of env step t are the last Q + has_act rows of dec_embed over steps 0 .. t and the history mask is its
    mask: launch against launch, bit for bit."""
    table, steps = R.dec_chain(E, B, Q, n_pos)
    Lmax = 4 * (Q + 1)
    st = _DecState(B, Lmax)
    L_hist = 0
    for t, (obs, mask, act, _) in enumerate(steps):
        cid = f"dec chain-{prec}-E{E}-step{t}"
        has_act = 1 if t else 0
        Ln = Q + has_act
        x, xT, rc, msg = run_dec_step(prec, st.dev, obs, mask, act, table, n_pos, L_hist, Lmax, has_act)
        assert rc == 0, msg
        L_hist += Ln
        obs_all, mask_all = torch.stack([s[0] for s in steps[: t + 1]]), torch.stack([s[1] for s in steps[: t + 1]])
        act_all = torch.stack([s[2] for s in steps[1: t + 1]]) if t else torch.zeros(1, B, E)
        fx, fxT, fm, rc, msg = run_dec_embed(prec, obs_all, mask_all, act_all, table, n_pos, t + 1, B, Q, t, E)
        assert rc == 0, msg
        _same(cid, "x32", x, fx[:, -Ln:]), _same(cid, "xT", xT, fxT[:, -Ln:])
        _same(cid, "hist_mask", st.dev["hist_mask"][:, :L_hist], fm)


@pytest.mark.parametrize("prec", R.PRECS)
def test_b_dec_embed_step_fills_pos_s(prec):
    """Q + has_act = 64: the most rows vima_op_dec_embed_step takes (the chunk kernel at T = 1; one row per thread of its scan up to 256)."""
    E, B, Q, n_pos = 256, 2, 63, 40
    gen = R._gen(81)
    obs, act, table = torch.randn(B, Q, E, generator=gen), torch.randn(B, E, generator=gen), torch.randn(n_pos, E, generator=gen)
    mask = (torch.rand(B, Q, generator=gen) < 0.8).to(torch.uint8)
    st = _DecState(B, 70)
    st.cpu["poscnt"][:] = torch.tensor([0, 5], dtype=torch.int32)
    st.dev["poscnt"].copy_(st.cpu["poscnt"])
    want = R.dec_step_ref(st.cpu, obs, mask, act, table, n_pos, 3, 1)
    x, xT, rc, msg = run_dec_step(prec, st.dev, obs, mask, act, table, n_pos, 3, 70, 1)
    assert rc == 0, msg
    _same("dec_embed_step Q63", "x32", x, want), _same("dec_embed_step Q63", "xT", xT, R.rounded(prec, want))
    st.check("dec_embed_step Q63")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("has_act", [0, 1])
def test_b_dec_embed_step_without_fresh(has_act, prec):
    """fresh = NULL: no sample is fresh. Rows, hist_mask and poscnt against the reference with no restart flag set, bit for bit."""
    E, B, Q, n_pos, L_hist, Lmax = 256, 2, 4, 512, 3, 12
    table, steps = R.dec_chain(E, B, Q, n_pos, seed=3)
    obs, mask, act, _ = steps[1]
    st = _DecState(B, Lmax)
    st.cpu["poscnt"][:] = torch.tensor([0, 5], dtype=torch.int32)
    st.dev["poscnt"].copy_(st.cpu["poscnt"])
    want = R.dec_step_ref(st.cpu, obs, mask, act, table, n_pos, L_hist, has_act)
    x, xT, rc, msg = run_dec_step(prec, {**st.dev, "fresh": None}, obs, mask, act, table, n_pos, L_hist, Lmax, has_act)
    assert rc == 0, msg
    cid = f"dec_embed_step no fresh-{prec}-act{has_act}"
    _same(cid, "x32", x, want), _same(cid, "xT", xT, R.rounded(prec, want))
    st.check(cid)


def run_prompt_pos(prec, store, sb, sl, mask, table, n_pos, lst, B, Lp, E):
    pol = bare_policy(prec)
    a = _Args()
    nb = B if lst is None else len(lst)
    ob, o = _guarded((nb, Lp, E), NAN)
    _ok(pol._lib.vima_op_prompt_pos, pol, a(store), sb, sl, a(mask), a(table), n_pos, a(lst), nb, Lp, E, ptr(ob))
    _tail_intact(ob, nb * Lp * E)
    return o.cpu()


@pytest.mark.parametrize("c", R.PP_CASES, ids=R.pp_case_id)
def test_b_prompt_pos(c):
    """Both slab sizes, the block-wide scan over 1 .. 600 positions, seq-first strides, an all-False sample, a list that permutes and repeats."""
    prec, E, B, Lp, lay, mkind, lst = c
    store, sb, sl, mask, table, n_pos = R.pp_inputs(E, B, Lp, lay, mkind)
    want = R.prompt_pos_ref(R.pp_view(store, lay), mask, table, n_pos, lst)
    _same(R.pp_case_id(c), "out", run_prompt_pos(prec, store, sb, sl, mask, table, n_pos, lst, B, Lp, E), R.rounded(prec, want))


@pytest.mark.parametrize("c", R.ACT_CASES, ids=R.act_case_id)
def test_b_action_l1(c):
    prec, K, Rn, ldo, col0 = c
    idx, W, b = R.act_inputs(K, Rn)
    ref, g32 = R.action_l1_ref(idx, W, b, R.action_bins(K))
    pol = bare_policy(prec)
    a = _Args()
    ob, o = _guarded((Rn, ldo), R.CANARY)
    _ok(pol._lib.vima_op_action_l1, pol, a(idx), K, a(W), a(b), Rn, ldo, col0, ptr(ob))
    _tail_intact(ob, Rn * ldo)
    o = o.cpu()
    _within(f"action_l1 {prec} K{K}", R.act_case_id(c), o[:, col0:col0 + 256], ref, R.with_bf16_term(prec, g32, ref))
    keep = torch.ones(ldo, dtype=torch.bool)
    keep[col0:col0 + 256] = False
    assert (o[:, keep] == R.CANARY).all(), "columns outside [col0, col0 + 256) were written"


@pytest.mark.parametrize("rows,E,group", [(13, 256, 3), (300, 768, 4), (7, 320, 1)])
def test_b_add_row_table(rows, E, group):
    gen = R._gen(91, rows, E, group)
    out, table = torch.randn(rows, E, generator=gen), torch.randn(2, E, generator=gen)
    sel = torch.randint(-1, 4, ((rows + group - 1) // group,), generator=gen, dtype=torch.int64)
    pol = bare_policy("fp32")
    a = _Args()
    ob, o = _guarded((rows, E), out)
    _ok(pol._lib.vima_op_add_row_table, pol, ptr(ob), rows, E, a(table), a(sel), group)
    _tail_intact(ob, rows * E)
    _same(f"add_row_table-{rows}-{E}-{group}", "out", o, R.add_row_table_ref(out, table, sel, group))


COPY_SHAPES = [(5, 128, 32), (37, 192, 64), (70, 520 - 8, 64), (3, 96, 32)]      # L, N, D: L N / 8 and L N / 4 chunks, no multiple of 256


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("L,N,D", COPY_SHAPES)
def test_b_operand_type_copies(L, N, D, prec):
    """rows_to_headmajor, kv_scatter (both layouts) and seq_kv_store (ld_in > N, L < Lmax, lists with gaps, no list): pure copies, bit for
    bit the (operand-type) source; unlisted blocks and rows past L keep the canary."""
    pol = bare_policy(prec)
    a = _Args()
    gen = R._gen(101, L, N, D)
    cid = f"copies-{prec}-L{L}-N{N}-D{D}"
    x = torch.randn(L, N, generator=gen)
    ob, o = _guarded((N // D, L, D), NAN)
    _ok(pol._lib.vima_op_rows_to_headmajor, pol, a(x), L, N, D, ptr(ob))
    _tail_intact(ob, L * N)
    _same(cid, "rows_to_headmajor", o, R.rounded(prec, R.headmajor_ref(x, D)))
    n, lst, nb = 3, (4, 0, 2), 6
    xs = torch.randn(n, L, N, generator=gen)
    for hm in (0, 1):
        ob, o = _guarded((nb, L * N), R.CANARY)
        _ok(pol._lib.vima_op_kv_scatter, pol, a(xs), a(lst), n, L, N, D, hm, nb, ptr(ob))
        _tail_intact(ob, nb * L * N)
        _same(cid, f"kv_scatter hm={hm}", o, R.kv_scatter_ref(R.rounded(prec, xs), lst, nb, L, N, D, hm))
    Lmax = L + 4
    for ld in (N, N + 8):
        xw = torch.randn(n, L, ld, generator=gen)
        for use in (lst, None):
            ob, o = _guarded((nb, Lmax, N), R.CANARY)
            _ok(pol._lib.vima_op_seq_kv_store, pol, a(xw), ld, a(use), n, L, N, Lmax, nb, ptr(ob))
            _tail_intact(ob, nb * Lmax * N)
            _same(cid, f"seq_kv_store ld_in={ld} list={use}", o, R.seq_kv_store_ref(R.rounded(prec, xw), use, nb, L, N, Lmax))


@pytest.mark.parametrize("rows,E,period", [(10, 256, 3), (1000, 320, 7), (5, 768, 8)])
def test_b_broadcast_rows(rows, E, period):
    src = torch.randn(period, E, generator=R._gen(111, rows, E))
    pol = bare_policy("fp32")
    a = _Args()
    ob, o = _guarded((rows, E), NAN)
    _ok(pol._lib.vima_op_broadcast_rows, pol, a(src), rows, E, period, ptr(ob))
    _tail_intact(ob, rows * E)
    _same(f"broadcast_rows-{rows}-{E}-{period}", "out", o, R.broadcast_ref(src, rows))


# ------------------------------------------------------------------------------------------------------------------ seq_embed*
def run_seq_embed(prec, store, pmask, sep, obs, act, table, n_pos, B, L, Lp, Q, E):
    pol = bare_policy(prec)
    xb, x = _guarded((B, L, E), NAN)
    tb, xT = _guarded((B, L, E), NAN)
    mb, m = _guarded((B, L), R.CANARY_U8, torch.uint8)
    d = [dev(store)], [dev(pmask), dev(sep), dev(obs), dev(act), dev(table)]
    _ok(pol._lib.vima_op_seq_embed, pol, ptr(d[0][0]), E, B * E, *(ptr(t) for t in d[1]), n_pos, B, L, Lp, Q, E, ptr(xb), ptr(tb), ptr(mb))
    for buf, n in ((xb, B * L * E), (tb, B * L * E), (mb, B * L)):
        _tail_intact(buf, n)
    return x.cpu(), xT.cpu(), m.cpu()


class _SeqState:
    def __init__(self, B, n_pos):
        self.cpu = R.seq_state(B, n_pos)
        self.dev = {k: dev(v) for k, v in self.cpu.items()}

    def check(self, cid):
        for k in self.cpu:
            _same(cid, k, self.dev[k], self.cpu[k])


def run_seq_prefill(prec, st, store, pmask, sep, table, n_pos, lst, B, Lp, E):
    pol = bare_policy(prec)
    a = _Args()
    n = B if lst is None else len(lst)
    xb, x = _guarded((n, Lp + 1, E), NAN)
    tb, xT = _guarded((n, Lp + 1, E), NAN)
    mb, m = _guarded((n, Lp + 1), R.CANARY_U8, torch.uint8)
    d = [dev(pmask), dev(sep), dev(table)]
    rc, msg = _call(pol._lib.vima_op_seq_embed_prefill, pol, a(store), E, B * E, *(ptr(t) for t in d), n_pos, a(lst), n, Lp, E,
                    ptr(xb), ptr(tb), ptr(mb), ptr(st["cache_mask"]), ptr(st["posbase"]))
    for buf, k in ((xb, n * (Lp + 1) * E), (tb, n * (Lp + 1) * E), (mb, n * (Lp + 1))):
        _tail_intact(buf, k)
    return x.cpu(), xT.cpu(), m.cpu(), rc, msg


def run_seq_step(prec, st, obs, act, table, n_pos, row0, has_act):
    pol = bare_policy(prec)
    a = _Args()
    B, Q, E = obs.shape
    Ln = Q + has_act
    xb, x = _guarded((B, Ln, E), NAN)
    tb, xT = _guarded((B, Ln, E), NAN)
    rc, msg = _call(pol._lib.vima_op_seq_embed_step, pol, a(obs), a(act), a(table), n_pos, row0, B, Q, has_act, E, ptr(xb), ptr(tb),
                    ptr(st["cache_mask"]), ptr(st["posbase"]), ptr(st["fresh"]))
    _tail_intact(xb, B * Ln * E), _tail_intact(tb, B * Ln * E)
    return x.cpu(), xT.cpu(), rc, msg


@pytest.mark.parametrize("c", R.SEQ_CASES, ids=R.seq_case_id)
def test_b_seq_embed_and_c_prefill_plus_steps(c):
    """seq_embed over the whole sequence against the reference; then the same sequence fed in pieces -- prefill, one launch per env step --
    bit for bit the rows of the whole-sequence launch, with the episode state (cache_mask and its canary rows, posbase, fresh) after each."""
    prec, E, B, Lp, nvk, T, Q, L_act, n_pos_c = c
    cid = R.seq_case_id(c)
    store, pmask, sep, obs, act, table, n_pos = R.seq_inputs(E, B, Lp, nvk, T, Q, L_act, n_pos_c)
    prompt = store.transpose(0, 1)
    L = Lp + 1 + T * Q + L_act
    want, want_m = R.seq_embed_ref(prompt, pmask, sep, obs, act, table, n_pos, L_act)
    x, xT, m = run_seq_embed(prec, store, pmask, sep, obs, act, table, n_pos, B, L, Lp, Q, E)
    _same(cid, "x32", x, want), _same(cid, "xT", xT, R.rounded(prec, want)), _same(cid, "mask", m, want_m)
    if Lp + 1 > n_pos:
        return
    st = _SeqState(B, n_pos)
    wp, wm = R.seq_prefill_ref(st.cpu, prompt, pmask, sep, table, n_pos)
    xp, xpT, mp, rc, msg = run_seq_prefill(prec, st.dev, store, pmask, sep, table, n_pos, None, B, Lp, E)
    assert rc == 0, msg
    _same(cid, "prefill x32", xp, wp), _same(cid, "prefill xT", xpT, R.rounded(prec, wp)), _same(cid, "prefill mask", mp, wm)
    _same(cid, "prefill rows are seq_embed's", xp, x[:, : Lp + 1])
    st.check(cid + " prefill")
    row0 = Lp + 1
    for t in range(T):
        has_act = 1 if t else 0
        Ln = Q + has_act
        if t > L_act or row0 + Ln > min(L, n_pos):
            break
        a = act[t - 1] if t else act[0]
        ws = R.seq_step_ref(st.cpu, obs[t], a, table, n_pos, row0, has_act)
        xs, xsT, rc, msg = run_seq_step(prec, st.dev, obs[t], a, table, n_pos, row0, has_act)
        assert rc == 0, msg
        _same(cid, f"step {t} x32", xs, ws), _same(cid, f"step {t} xT", xsT, R.rounded(prec, ws))
        _same(cid, f"step {t} rows are seq_embed's", xs, x[:, row0:row0 + Ln])
        st.check(cid + f" step {t}")
        row0 += Ln


@pytest.mark.parametrize("prec", R.PRECS)
def test_b_seq_prefill_list_restart_and_the_fresh_action_row(prec):
    """A prefill of a list of samples with gaps leaves the other samples' state alone; seq_restart masks [lo, hi) of the listed samples;
    the next step of a restarted sample embeds ZEROS for its action row whatever act_tok holds (here NaN), masks it and gives it no id."""
    E, B, Lp, Q = 256, 5, 5, 4
    store, pmask, sep, obs, act, table, n_pos = R.seq_inputs(E, B, Lp, "mixed", 2, Q, 1, 40)
    prompt = store.transpose(0, 1)
    st = _SeqState(B, n_pos)
    lst = (3, 0)
    cid = f"seq list / restart {prec}"
    wp, wm = R.seq_prefill_ref(st.cpu, prompt, pmask, sep, table, n_pos, lst)
    xp, xpT, mp, rc, msg = run_seq_prefill(prec, st.dev, store, pmask, sep, table, n_pos, lst, B, Lp, E)
    assert rc == 0, msg
    _same(cid, "prefill x32", xp, wp), _same(cid, "prefill xT", xpT, R.rounded(prec, wp)), _same(cid, "prefill mask", mp, wm)
    st.check(cid + " prefill")
    assert (st.cpu["cache_mask"][[1, 2, 4]] == R.CANARY_U8).all() and (st.cpu["posbase"][[1, 2, 4]] == -7).all()
    pol = bare_policy(prec)
    a = _Args()
    R.seq_restart_ref(st.cpu, (4, 0), Lp + 1, 30)
    _ok(pol._lib.vima_op_seq_restart, pol, a((4, 0)), 2, Lp + 1, 30, n_pos, ptr(st.dev["cache_mask"]), ptr(st.dev["fresh"]))
    st.check(cid + " restart")
    for k in ("posbase",):
        st.cpu[k][:] = torch.tensor([3, 9, 2, 38, 1], dtype=torch.int32)          # sample 3 runs into the upper clamp
        st.dev[k].copy_(st.cpu[k])
    poisoned = act[0].clone()
    poisoned[[0, 4]] = NAN
    ws = R.seq_step_ref(st.cpu, obs[1], poisoned, table, n_pos, 12, 1)
    xs, xsT, rc, msg = run_seq_step(prec, st.dev, obs[1], poisoned, table, n_pos, 12, 1)
    assert rc == 0, msg
    assert torch.isfinite(xs).all(), "a fresh sample's act_tok row reached the output"
    _same(cid, "step x32", xs, ws), _same(cid, "step xT", xsT, R.rounded(prec, ws))
    st.check(cid + " step")


# ================================================================================================================== E
def _refused(fn, prec, outs, *args):
    pol = bare_policy(prec)
    before = [o.clone() for o in outs]
    rc, msg = _call(fn, pol, *args)
    assert rc != 0 and msg, (rc, msg)
    for o, b in zip(outs, before):
        assert torch.equal(o.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote to a caller's buffer"
    return msg


@pytest.mark.parametrize("prec", R.PRECS)
def test_e_norm_refusals(prec):
    x, g = torch.randn(8, 1040), torch.ones(1040)
    for kind, E, ldin, why in (("ln", 1028, 1028, "E > 1024"), ("ln_T", 1028, 1028, "E > 1024"), ("ln2", 1028, 1028, "E > 1024"), ("ln", 254, 256, "E % 4"),
                               ("ln_T", 256, 258, "ldin % 4"), ("rms_stats", 254, 254, "E % 4")):
        out, rc, msg = run_norm(prec, kind, x, ldin, g, g, 1e-5, 0, 8, E, g, g, 1e-5)
        assert rc != 0 and msg, (kind, why)
        assert all(torch.isnan(t).all() for t in out.values()), f"{kind} ({why}): a refused call wrote to an output"
    out, rc, msg = run_norm(prec, "ln", x, 256, g, g, 1e-5, 0, 8, 256, want32=False, wantT=False)
    assert rc != 0 and "no output" in msg
    out, rc, msg = run_norm(prec, "ln2", x, 256, g, g, 1e-5, 0, 8, 256, None, None, 1e-5)
    assert rc != 0 and "gamma2" in msg and all(torch.isnan(t).all() for t in out.values())
    out, rc, msg = run_norm(prec, "rms_stats", x, 260, None, None, 0.0, 1, 8, 256)
    assert rc != 0 and "ldin" in msg and all(torch.isnan(t).all() for t in out.values())


@pytest.mark.parametrize("prec", R.PRECS)
def test_e_sequence_refusals(prec):
    lib = bare_policy(prec)._lib
    E = 256
    f = torch.randn(600 * E, device=DEV)
    u8 = torch.ones(4096, dtype=torch.uint8, device=DEV)
    out, out2 = torch.full((520 * E,), NAN, device=DEV), torch.full((520 * E,), NAN, device=DEV)
    mk = torch.full((4096,), R.CANARY_U8, dtype=torch.uint8, device=DEV)
    cnt = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    fr = torch.zeros(8, dtype=torch.uint8, device=DEV)
    outs = [out, out2, mk, cnt, fr]
    T, Q, La = R.DEC_REFUSED
    assert T * Q + La == 513
    assert "dec_embed" in _refused(lib.vima_op_dec_embed, prec, outs, ptr(f), ptr(u8), ptr(f), ptr(f), 512, T, 1, Q, La, E, ptr(out), ptr(out2), ptr(mk))
    assert "L_act" in _refused(lib.vima_op_dec_embed, prec, outs, ptr(f), ptr(u8), ptr(f), ptr(f), 512, 3, 1, 4, 1, E, ptr(out), ptr(out2), ptr(mk))
    assert "null" in _refused(lib.vima_op_dec_embed, prec, outs, ptr(f), None, ptr(f), ptr(f), 512, 2, 1, 4, 2, E, ptr(out), ptr(out2), ptr(mk))
    step = lambda *a: _refused(lib.vima_op_dec_embed_step, prec, outs, ptr(f), ptr(u8), ptr(f), ptr(f), 512, *a, E, ptr(out), ptr(out2), ptr(mk), ptr(cnt), ptr(fr))
    assert "dec_embed_step" in step(0, 128, 1, 64, 1)                      # Q + has_act = 65: one more than the op takes  
    assert "dec_embed_step" in step(10, 14, 1, 4, 1)                       # L_hist + Ln = 15 > Lmax = 14
    assert "gather_pred" in _refused(lib.vima_op_gather_pred, prec, outs, ptr(f), 2, 1, 4, 8, E, ptr(out))       # row 3 + 5 = 8 of 8
    assert "prompt_pos" in _refused(lib.vima_op_prompt_pos, prec, outs, ptr(f), 258, 6, ptr(u8), ptr(f), 8, None, 1, 2, E, ptr(out))   # strides % 4
    assert "K must" in _refused(lib.vima_op_action_l1, prec, outs, ptr(cnt), 3, ptr(f), ptr(f), 1, 256, 0, ptr(out))
    assert "inside ldo" in _refused(lib.vima_op_action_l1, prec, outs, ptr(cnt), 2, ptr(f), ptr(f), 1, 256, 4, ptr(out))
    assert "rows_to_headmajor" in _refused(lib.vima_op_rows_to_headmajor, prec, outs, ptr(f), 4, 96, 36, ptr(out))         # N % D
    assert "kv_scatter" in _refused(lib.vima_op_kv_scatter, prec, outs, ptr(f), ptr(cnt), 1, 4, 96, 36, 1, 1, ptr(out))
    assert "seq_kv_store" in _refused(lib.vima_op_seq_kv_store, prec, outs, ptr(f), 96, None, 1, 9, 96, 8, 1, ptr(out))   # L > Lmax
    assert "broadcast_rows" in _refused(lib.vima_op_broadcast_rows, prec, outs, ptr(f), 4, E, 0, ptr(out))
    pre = lambda n_pos, Lp: _refused(lib.vima_op_seq_embed_prefill, prec, outs, ptr(f), E, E, ptr(u8), ptr(f), ptr(f), n_pos, None, 1, Lp, E,
                                     ptr(out), ptr(out2), ptr(mk), ptr(mk), ptr(cnt))
    assert "seq_embed_prefill" in pre(5, 5)                                # Lp + 1 > n_pos
    sstep = lambda n_pos, row0, Q, ha: _refused(lib.vima_op_seq_embed_step, prec, outs, ptr(f), ptr(f), ptr(f), n_pos, row0, 1, Q, ha, E, ptr(out), ptr(out2),
                                                ptr(mk), ptr(cnt), ptr(fr))
    assert "seq_embed_step" in sstep(12, 8, 4, 1)                          # row0 + Ln = 13 > n_pos = 12
    assert "seq_embed_step" in sstep(512, 0, 64, 1)                        # Q + has_act = 65
    assert "seq_restart" in _refused(lib.vima_op_seq_restart, prec, outs, ptr(cnt), 1, 0, 13, 12, ptr(mk), ptr(fr))       # hi > n_pos
    assert "null" in _refused(lib.vima_op_seq_embed, prec, outs, ptr(f), E, E, ptr(u8), None, ptr(f), ptr(f), ptr(f), 64, 1, 8, 2, 4, E, ptr(out), ptr(out2), ptr(mk))
    assert "positive" in _refused(lib.vima_op_prompt_assemble, prec, outs, ptr(cnt), ptr(cnt), ptr(f), ptr(f), ptr(u8), 0, E, 0, ptr(out), ptr(out2), ptr(mk))
    assert "prompt_assemble" in _refused(lib.vima_op_prompt_assemble, prec, outs, ptr(cnt), ptr(cnt), ptr(f), ptr(f), ptr(u8), 1, 254, 1, ptr(out), ptr(out2), ptr(mk))


def test_zz_print_the_worst_ratios():
    """Last in the file: the worst err / gate per kernel, operand type and regime (profiles/seq_norm_errors.txt records them)."""
    for family in sorted(_worst):
        ratio, cid = _worst[family]
        print(f"[seq-norm] worst err / gate, {family}: {ratio:.3f} at {cid}")
