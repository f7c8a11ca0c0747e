"""Pins tests/seq_norm_reference.py on the CPU: every reference against a second, independently written form (1e-12, or equality for the
exact ones), against oracle/ where it computes the stage (decoder position ids, prompt assembly, the decoder-only sequence), every LN / RMS
gate against a two-pass fp32 restatement in two summation orders (under HALF the fp32 gate; its bf16 rounding under the bf16 gate), every
gate against the mutations it is there to catch (each more than 10x beyond it on a named case), and the entry points of
tests/test_seq_norm_gpu.py against header and binding."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import seq_norm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEETH = 10.0
_worst = {}


def _note(family, ratio, cid):
    if ratio > _worst.get(family, (-1.0, ""))[0]:
        _worst[family] = (ratio, cid)


def _dedup(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


def _stream_is_bf16(c):
    return c[0] == "ln_T" and c[1] == "bf16"


# one case per (values the kernel reads, shape, regime): the kernels of one shape share the reference and the gate
LN = _dedup(R.LN_CASES, lambda c: (_stream_is_bf16(c), c[1]) + c[2:])
LN_SMALL = [c for c in LN if c[3] <= 33]


# ================================================================================================================== norms
def _two_pass32(x, g, b, eps, rms, perm=None):
    """The fp32 restatement: mean, centred squares, one rsqrt -- every sum by torch in fp32, on permuted columns when perm is given."""
    E = x.shape[1]
    if perm is not None:
        x, g, b = x[:, perm], g[perm], (None if b is None else b[perm])
    mean = torch.zeros_like(x[:, :1]) if rms else x.sum(dim=1, keepdim=True) / E
    d = x - mean
    out = d * torch.rsqrt((d * d).sum(dim=1, keepdim=True) / E + eps) * g
    if b is not None:
        out = out + b
    if perm is not None:
        out = out[:, torch.argsort(perm)]
    assert out.dtype == torch.float32
    return out


def _perm(E):
    return torch.randperm(E, generator=torch.Generator().manual_seed(E))


@pytest.mark.parametrize("c", [c for c in LN_SMALL if c[1] == "fp32" and c[4] == 0], ids=R.norm_case_id)
def test_norm_ref64_against_independent_forms(c):
    kind, prec, E, rows, pad, rms, regime = c
    x, g, b, eps = R.norm_operands(c)
    ref, _, _ = R.ln_reference(c)
    if rms:   # OraclePolicy._rms's lines (HF T5LayerNorm), in fp64
        xd = x.double()
        want = g.double() * (xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps))
    else:
        want = F.layer_norm(x.double(), (E,), g.double(), b.double(), eps)
    assert ref.dtype == torch.float64 and (want - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
    if regime == "zero":
        assert torch.equal(ref, torch.zeros_like(ref) if rms else b.double().expand_as(ref))


@pytest.mark.parametrize("c", LN, ids=R.norm_case_id)
def test_ln_gate_holds_the_fp32_restatement_in_two_orders(c):
    kind, prec, E, rows, pad, rms, regime = c
    x, g, b, eps = R.norm_operands(c)
    ref, g32, gT = R.ln_reference(c)
    assert torch.isfinite(ref).all() and (g32 > 0).all()
    fam = f"{'rms' if rms else 'ln'} {regime}"
    for name, perm in (("torch order", None), ("permuted columns", _perm(E))):
        r32 = _two_pass32(x, g, b, eps, rms, perm)
        a = ((r32.double() - ref).abs() / g32).max().item()
        _note(f"{fam}: fp32 restatement / fp32 gate", a, R.norm_case_id(c) + " " + name)
        assert a < 0.5, f"{R.norm_case_id(c)} ({name}): fp32 restatement at {a:.3f} of the fp32 gate"
    bb = ((R.bf(ref.float()).double() - ref).abs() / R.with_bf16_term("bf16", g32, ref)).max().item()
    _note(f"{fam}: bf16(fp64 reference) / bf16 gate", bb, R.norm_case_id(c))
    assert bb < 1.0


@pytest.mark.parametrize("c", _dedup(R.LN2_CASES, lambda c: c[2:]), ids=R.norm_case_id)
def test_ln2_gates_hold_the_fp32_restatement(c):
    _, prec, E, rows, pad, _, regime = c
    full, g, b, g2, b2 = R.norm_inputs(E, rows, pad, regime)
    y, g1, _, z, gz = R.ln2_reference((c[0], "fp32") + c[2:])
    want = F.layer_norm(F.layer_norm(full[:, :E].double(), (E,), g.double(), b.double(), 1e-5), (E,), g2.double(), b2.double(), 1e-5)
    assert (want - z).abs().max().item() <= 1e-12 * max(1.0, z.abs().max().item())
    for name, perm in (("torch order", None), ("permuted columns", _perm(E))):
        y32 = _two_pass32(full[:, :E], g, b, 1e-5, 0, perm)
        z32 = _two_pass32(y32, g2, b2, 1e-5, 0, perm)
        a, a2 = ((y32.double() - y).abs() / g1).max().item(), ((z32.double() - z).abs() / gz).max().item()
        _note(f"ln2 {regime}: second output, fp32 restatement / composed gate", a2, R.norm_case_id(c) + " " + name)
        assert a < 0.5 and a2 < 0.5, (name, a, a2)
    assert ((R.bf(z.float()).double() - z).abs() / R.with_bf16_term("bf16", gz, z)).max().item() < 1.0


@pytest.mark.parametrize("c", _dedup(R.RMS_STATS_CASES, lambda c: c[2:]), ids=R.norm_case_id)
def test_ssq_reference_and_gate(c):
    _, _, E, rows, _, _, regime = c
    x = R.norm_inputs(E, rows, 0, regime)[0]
    ref, gate = R.ssq_reference(x)
    assert (torch.linalg.vector_norm(x.double(), dim=1) ** 2 - ref).abs().max().item() <= 1e-12 * max(1.0, ref.max().item())
    for xs in (x, x[:, _perm(E)]):
        err = ((xs * xs).sum(dim=1).double() - ref).abs()
        assert (err <= 0.5 * gate).all()
        if regime != "zero":
            _note("ssq: fp32 restatement / gate", (err / gate).max().item(), R.norm_case_id(c))
    assert ((1.02 * ref - ref).abs() > gate).all() or regime == "zero"


def _row_pairs_swapped(ref):
    rows = ref.shape[0]
    idx = torch.arange(rows) ^ 1
    return ref[torch.where(idx < rows, idx, torch.arange(rows))]


# mutation -> the case of LN_CASES it is shown on (the fp32 output's gate; a bf16 rounding rightly hides a change of 1 / 2E)
NORM_MUTATIONS = {
    "unbiased variance (E - 1)": ("ln_T", "fp32", 256, 33, 0, 0, "plain"),
    "eps dropped": ("ln", "fp32", 256, 7, 0, 0, "lowvar"),
    "mean not removed in the second pass": ("ln", "fp32", 320, 7, 0, 0, "offset"),
    "beta applied under rms": ("ln_T", "bf16", 768, 33, 0, 1, "plain"),
    "the two rows of a rows2 pair swapped": ("ln_T", "bf16", 512, 2, 0, 0, "plain"),
    "the last odd row takes its neighbour's statistics": ("ln_T", "bf16", 1024, 7, 0, 0, "plain"),
}


@pytest.mark.parametrize("name", list(NORM_MUTATIONS))
def test_norm_gates_have_teeth(name):
    c = NORM_MUTATIONS[name]
    assert c in R.LN_CASES
    kind, prec, E, rows, pad, rms, regime = c
    x, g, b, eps = R.norm_operands(c)
    ref, g32, gT = R.ln_reference(c)
    xd, gd, bd = x.double(), g.double(), (None if b is None else b.double())
    if name.startswith("unbiased"):
        mut = R.norm_ref64(xd, gd, bd, eps, rms, unbiased=True)[0]
    elif name.startswith("eps"):
        mut = R.norm_ref64(xd, gd, bd, eps, rms, drop_eps=True)[0]
    elif name.startswith("mean"):
        mut = R.norm_ref64(xd, gd, bd, eps, rms, keep_mean=True)[0]
    elif name.startswith("beta"):
        mut = ref + R.norm_inputs(E, rows, pad, regime)[2].double()
    elif name.startswith("the two rows"):
        mut = _row_pairs_swapped(ref)
    else:
        assert rows % 2 == 1
        mean = xd.sum(dim=1, keepdim=True) / E
        var = ((xd - mean) ** 2).sum(dim=1, keepdim=True) / E
        mean[-1], var[-1] = mean[-2], var[-2]
        mut = (xd - mean) / torch.sqrt(var + eps) * gd + bd
    gate = g32 if prec == "fp32" else gT
    r = ((mut - ref).abs() / gate).max().item()
    assert r > TEETH, f"{R.norm_case_id(c)}: mutation '{name}' reaches only {r:.2f} x the gate"


# ================================================================================================================== exact kernels
def _differs(cid, name, mut, ref):
    """An exact gate has no width: the mutation must move some element by more than 10 bf16 roundings of it, so that no operand type hides it."""
    assert mut.shape == ref.shape, (cid, name)
    d = (mut.double() - ref.double()).abs()
    r = (d / (R.U_BF16 * ref.double().abs() + 1e-30)).max().item()
    assert r > TEETH and not torch.equal(R.bf(mut), R.bf(ref)), f"{cid}: mutation '{name}' moves no element by more than {r:.2f} bf16 roundings"


class _CapturedDecoder:
    """OraclePolicy.forward (oracle/vima_oracle.py) with the transformer replaced by a recorder: what remains is the oracle's own interleave,
    its cumsum position ids of tokens and prompt, and its gather of the predicted rows."""

    @staticmethod
    def run(obs, mask, act, prompt_lbe, pmask):
        from oracle.vima_oracle import OraclePolicy
        cap = {}

        class P(OraclePolicy):
            def __init__(self):
                pass

            def xattn_gpt(self, tokens, pos_ids, prompt, prompt_mask, prompt_pos_ids, masks):
                cap.update(tokens=tokens, pos=pos_ids, ppos=prompt_pos_ids, masks=masks)
                return tokens

        cap["pred"] = P().forward(obs, mask.bool(), act, prompt_lbe, pmask.bool())
        return cap


@pytest.mark.parametrize("c", [c for c in R.DEC_CASES if c[0] == "fp32" and c[3] <= 3], ids=R.dec_case_id)
def test_dec_embed_ref_against_the_oracle_and_a_loop(c):
    _, E, B, T, Q, L_act, mkind = c
    obs, mask, act, table, n_pos = R.dec_inputs(E, B, T, Q, L_act, mkind)
    x, m, pos = R.dec_embed_ref(obs, mask, act, table, n_pos, L_act)
    L = T * Q + L_act
    cap = _CapturedDecoder.run(obs, mask, act[:L_act] if L_act else None, torch.zeros(1, B, E), torch.ones(B, 1))
    assert torch.equal(cap["tokens"], R.interleave(obs, mask, act[:L_act] if L_act else None, L)[0]) and torch.equal(cap["masks"], m.bool())
    assert torch.equal(cap["pos"].clamp(0, n_pos - 1), pos)                 # the two clamps are this project's, the ids the oracle's
    assert torch.equal(cap["tokens"] + table[pos], x)
    assert torch.equal(cap["pred"], R.gather_pred_ref(cap["tokens"], cap["pred"].shape[0], Q))
    # second form: plain loops
    for b in range(B):
        run = 0
        for l in range(L):
            t, s = divmod(l, Q + 1)
            mk = int(mask[t, b, s]) if s < Q else 1
            run += mk
            p = min(max(run - 1, 0), n_pos - 1)
            tok = obs[t, b, s] if s < Q else act[t, b]
            assert m[b, l] == mk and pos[b, l] == p and torch.equal(x[b, l], tok + table[p])


DEC_MUTATIONS = {
    "position ids off by one": (("fp32", 256, 3, 2, 4, 2, "valid"), dict(shift=1)),
    "cumsum restarted per step": (("fp32", 256, 3, 3, 4, 2, "valid"), dict(per_step=True)),
    "a masked token consumes a position": (("fp32", 768, 5, 2, 4, 1, "first_masked"), dict(count_masked=True)),
    "lower clamp missing": (("fp32", 320, 1, 1, 1, 0, "first_masked"), dict(lower=False)),
    "upper clamp missing": (("fp32", 256, 3, 3, 4, 3, "overflow"), dict(upper=False)),
}


@pytest.mark.parametrize("name", list(DEC_MUTATIONS))
def test_dec_embed_mutations_are_seen(name):
    c, kw = DEC_MUTATIONS[name]
    assert c in R.DEC_CASES
    _, E, B, T, Q, L_act, mkind = c
    obs, mask, act, table, n_pos = R.dec_inputs(E, B, T, Q, L_act, mkind)
    _differs(R.dec_case_id(c), name, R.dec_embed_ref(obs, mask, act, table, n_pos, L_act, **kw)[0], R.dec_embed_ref(obs, mask, act, table, n_pos, L_act)[0])


def test_gather_pred_mutation_is_seen():
    x = torch.randn(3, 14, 256, generator=torch.Generator().manual_seed(3))
    _differs("gather_pred T3 Q4", "row Q instead of Q - 1", R.gather_pred_ref(x, 3, 4, row=4)[:2], R.gather_pred_ref(x, 3, 4)[:2])
    for t in range(3):
        assert torch.equal(R.gather_pred_ref(x, 3, 4)[t], x[:, 3 + 5 * t])


@pytest.mark.parametrize("E,B,Q,n_pos", [(256, 3, 4, 512), (320, 1, 1, 512), (768, 5, 4, 6)])
def test_dec_step_chain_is_dec_embed_over_the_history(E, B, Q, n_pos):
    """Without a restart the rows of step t are the last Q + 1 rows of dec_embed over steps 0 .. t, bit for bit, and the state is its mask /
    its count of valid tokens."""
    table, steps = R.dec_chain(E, B, Q, n_pos)
    Lmax = 4 * (Q + 1) + 3
    st = R.dec_state(B, Lmax)
    L_hist = 0
    for t, (obs, mask, act, _) in enumerate(steps):
        has_act = 1 if t else 0
        x = R.dec_step_ref(st, obs, mask, act, table, n_pos, L_hist, has_act)
        L_hist += Q + has_act
        obs_all = torch.stack([s[0] for s in steps[: t + 1]])
        mask_all = torch.stack([s[1] for s in steps[: t + 1]])
        act_all = torch.stack([s[2] for s in steps[1: t + 1]]) if t else torch.zeros(1, B, E)
        full, m, _ = R.dec_embed_ref(obs_all, mask_all, act_all, table, n_pos, t)
        assert torch.equal(x, full[:, -(Q + has_act):])
        assert torch.equal(st["hist_mask"][:, :L_hist], m) and (st["hist_mask"][:, L_hist:] == R.CANARY_U8).all()
        assert torch.equal(st["poscnt"].long(), m.long().sum(dim=1))


def test_dec_step_restart_against_a_loop():
    E, B, Q, n_pos = 256, 3, 4, 512
    table, steps = R.dec_chain(E, B, Q, n_pos, restart_at=2)
    Lmax = 4 * (Q + 1)
    st = R.dec_state(B, Lmax)
    hist, cnt, fresh = [[R.CANARY_U8] * Lmax for _ in range(B)], [0] * B, [0] * B
    L_hist = 0
    for t, (obs, mask, act, flags) in enumerate(steps):
        has_act = 1 if t else 0
        if flags is not None:
            R.restart_ref(st, flags)
            for b in range(B):
                if flags[b]:
                    hist[b], cnt[b], fresh[b] = [0] * Lmax, 0, 1
        x = R.dec_step_ref(st, obs, mask, act, table, n_pos, L_hist, has_act)
        for b in range(B):
            for i in range(Q + has_act):
                is_act = has_act and i == 0
                mk = (0 if fresh[b] else 1) if is_act else int(mask[b, i - has_act])
                cnt[b] += mk
                hist[b][L_hist + i] = mk
                assert torch.equal(x[b, i], (act[b] if is_act else obs[b, i - has_act]) + table[min(max(cnt[b] - 1, 0), n_pos - 1)])
            fresh[b] = 0
        L_hist += Q + has_act
        assert st["hist_mask"].tolist() == hist and st["poscnt"].tolist() == cnt and st["fresh"].tolist() == fresh


# ------------------------------------------------------------------------------------------------------------------ prompt_pos
@pytest.mark.parametrize("c", [c for c in R.PP_CASES if c[0] == "fp32"], ids=R.pp_case_id)
def test_prompt_pos_ref_against_the_oracle(c):
    _, E, B, Lp, lay, mkind, lst = c
    store, sb, sl, mask, table, n_pos = R.pp_inputs(E, B, Lp, lay, mkind)
    view = R.pp_view(store, lay)
    assert view.shape == (B, Lp, E) and view.stride() == (sb, sl, 1)
    out = R.prompt_pos_ref(view, mask, table, n_pos, lst)
    cap = _CapturedDecoder.run(torch.zeros(1, B, 1, E), torch.ones(1, B, 1), None, view.transpose(0, 1), mask)
    want = view + table[cap["ppos"].clamp(0, n_pos - 1)]
    assert torch.equal(out, want if lst is None else torch.stack([want[i] for i in lst]))
    if mkind == "empty_sample":
        assert torch.equal(out[(lst or list(range(B))).index(B // 2)], view[B // 2] + table[0])


PP_MUTATIONS = {
    "position ids off by one": (("fp32", 256, 3, 256, "BLE", "holes", None), dict(shift=1)),
    "a masked token consumes a position": (("fp32", 320, 1, 255, "LBE", "holes", None), dict(count_masked=True)),
    "lower clamp missing": (("fp32", 768, 5, 257, "LBE", "holes", None), dict(lower=False)),
    "upper clamp missing": (("fp32", 256, 3, 40, "BLE", "overflow", None), dict(upper=False)),
    "list applied to the output block": (("fp32", 256, 3, 40, "BLE", "holes", (2, 0, 1)), dict(scatter=True)),
}


@pytest.mark.parametrize("name", list(PP_MUTATIONS) + ["sl and sb exchanged"])
def test_prompt_pos_mutations_are_seen(name):
    c, kw = PP_MUTATIONS.get(name, (("fp32", 320, 5, 70, "LBE", "empty_sample", (4, 0, 0, 2, 4, 1, 4)), {}))
    assert c in R.PP_CASES
    _, E, B, Lp, lay, mkind, lst = c
    store, sb, sl, mask, table, n_pos = R.pp_inputs(E, B, Lp, lay, mkind)
    ref = R.prompt_pos_ref(R.pp_view(store, lay), mask, table, n_pos, lst)
    mut = R.prompt_pos_ref(R.pp_view(store, lay, swap=not kw), mask, table, n_pos, lst, **kw)
    _differs(R.pp_case_id(c), name, mut, ref)


# ------------------------------------------------------------------------------------------------------------------ prompt_assemble
def test_prompt_assemble_ref_against_the_oracle(monkeypatch):
    """OraclePolicy.forward_prompt_assembly with the encoders replaced by recorders: its python loops place word rows, object rows and masks."""
    from oracle import vima_oracle
    E, Q = 768, 2
    gen = torch.Generator().manual_seed(5)
    token_types = [[0, 1, 0], [1], [0, 0, 1, 1]]
    n_words, n_img = 4, 4
    word_ids = torch.randint(0, 11, (n_words,), generator=gen)
    table, img_emb = torch.randn(11, E, generator=gen), torch.randn(n_img, Q, E, generator=gen)
    view_mask = {v: (torch.rand(n_img, 1, generator=gen) < 0.5) for v in vima_oracle.VIEWS}
    cap = {}

    class P(vima_oracle.OraclePolicy):
        def __init__(self):
            self.sd = {"prompt_embedding._embed_layer.weight": table}

        def obj_encoder(self, crops, bbox, mask=None):
            return img_emb

        def _t5(self, toks, masks):
            cap.update(toks=toks, masks=masks)
            return toks

    monkeypatch.setattr(vima_oracle, "_mlp", lambda sd, prefix, x, n: x)
    P().forward_prompt_assembly((token_types, word_ids, {"cropped_img": None, "bbox": None, "mask": view_mask}))
    B, L = cap["toks"].shape[:2]
    src, wp, ip = torch.full((B, L), -1, dtype=torch.int32), 0, 0           # the host's encoding of the same prompts
    for b, p in enumerate(token_types):
        l = 0
        for t in p:
            if t == 0:
                src[b, l], wp, l = wp, wp + 1, l + 1
            else:
                for q in range(Q):
                    src[b, l + q] = -2 - (ip * Q + q)
                ip, l = ip + 1, l + Q
    obj_mask = torch.cat([view_mask[v] for v in vima_oracle.VIEWS], dim=-1).to(torch.uint8).flatten()
    x, m = R.prompt_assemble_ref(src.flatten(), word_ids, table, img_emb.reshape(-1, E), obj_mask)
    assert torch.equal(x.view(B, L, E), cap["toks"]) and torch.equal(m.view(B, L).float(), cap["masks"])


@pytest.mark.parametrize("c", [c for c in R.PA_CASES if c[0] == "fp32"], ids=R.pa_case_id)
def test_prompt_assemble_ref_against_a_loop(c):
    _, E, B, L = c
    src, word_ids, wt, ot, om = R.pa_inputs(E, B, L)
    x, m = R.prompt_assemble_ref(src, word_ids, wt, ot, om)
    kinds = set()
    for r, s in enumerate(src.tolist()):
        if s >= 0:
            want, mk = wt[word_ids[s]], 1
        elif s == -1:
            want, mk = torch.zeros(E), 0
        else:
            want, mk = ot[-s - 2], int(om[-s - 2] != 0)
        kinds.add((s >= 0, s == -1, mk))
        assert torch.equal(x[r], want) and m[r] == mk
    assert len(kinds) == 4 and len(set(src.tolist())) < len(src) or B * L < 8       # words, pads, objects of both masks; repeated sources


# ------------------------------------------------------------------------------------------------------------------ action_l1, add_row_table
@pytest.mark.parametrize("c", R.ACT_CASES, ids=R.act_case_id)
def test_action_l1_reference_gate_and_teeth(c):
    prec, K, Rn, ldo, col0 = c
    idx, W, b = R.act_inputs(K, Rn)
    ref, g32 = R.action_l1_ref(idx, W, b, R.action_bins(K))
    gate = R.with_bf16_term(prec, g32, ref)
    a = idx.float().clone()                                                        # OraclePolicy._de_discretize_actions' lines
    if K == 2:
        a[..., 0], a[..., 1] = a[..., 0] / 50, a[..., 1] / 100
    else:
        a = a / 50
    assert (torch.relu(F.linear(a.double(), W.double(), b.double())) - ref).abs().max().item() <= 1e-6    # idx / bins is rounded in fp32 there
    exact = torch.relu(F.linear(idx.double() / torch.tensor(R.action_bins(K), dtype=torch.float64), W.double(), b.double()))
    assert (exact - ref).abs().max().item() <= 1e-12
    r32 = torch.relu(F.linear(a, W, b))
    ratio = ((r32.double() - ref).abs() / g32).max().item()
    _note("action_l1: fp32 restatement / fp32 gate", ratio, R.act_case_id(c))
    assert ratio < 0.5 and ((R.bf(r32).double() - ref).abs() / R.with_bf16_term("bf16", g32, ref)).max().item() < 1.0
    if K == 2 and Rn >= 7:
        mut = R.action_l1_ref(idx, W, b, R.action_bins(2, y_bins=50.0))[0]
        r = ((mut - ref).abs() / gate).max().item()
        assert r > TEETH, f"{R.act_case_id(c)}: 'y divided by 50' reaches only {r:.2f} x the gate"


def test_add_row_table_ref_against_a_loop():
    gen = torch.Generator().manual_seed(9)
    out, table = torch.randn(13, 256, generator=gen), torch.randn(2, 256, generator=gen)
    sel = torch.tensor([0, 1, 5, -3, 1])
    got = R.add_row_table_ref(out, table, sel, 3)
    for r in range(13):
        assert torch.equal(got[r], out[r] + table[min(max(int(sel[r // 3]), 0), 1)])


# ------------------------------------------------------------------------------------------------------------------ copies
def test_copy_refs_against_loops_and_mutations():
    gen = torch.Generator().manual_seed(11)
    L, N, D = 5, 128, 32
    x = torch.randn(L, N, generator=gen)
    hm = R.headmajor_ref(x, D)
    for l in range(L):
        for h in range(N // D):
            assert torch.equal(hm[h, l], x[l, h * D:(h + 1) * D])
    _differs("rows_to_headmajor L5 N128 D32", "L and D exchanged", R.headmajor_ref(x, D, swap_ld=True).reshape(-1), hm.reshape(-1))
    n, lst, nb = 3, (4, 0, 2), 6
    xs = torch.randn(n, L, N, generator=gen)
    for flag in (0, 1):
        out = R.kv_scatter_ref(xs, lst, nb, L, N, D, flag)
        for blk in range(nb):
            if blk in lst:
                src = xs[lst.index(blk)]
                assert torch.equal(out[blk], (R.headmajor_ref(src, D) if flag else src).reshape(-1))
            else:
                assert (out[blk] == R.CANARY).all()
    ld, Lmax = N + 8, 9
    xw = torch.randn(n, L, ld, generator=gen)
    for use in (lst, None):
        out = R.seq_kv_store_ref(xw, use, nb, L, N, Lmax)
        for blk in range(nb):
            r = (list(use).index(blk) if blk in use else None) if use else (blk if blk < n else None)
            if r is None:
                assert (out[blk] == R.CANARY).all()
            else:
                assert torch.equal(out[blk, :L], xw[r, :, :N]) and (out[blk, L:] == R.CANARY).all()
    src = torch.randn(3, 64, generator=gen)
    b = R.broadcast_ref(src, 10)
    assert all(torch.equal(b[r], src[r % 3]) for r in range(10))


# ------------------------------------------------------------------------------------------------------------------ seq_embed*
@pytest.mark.parametrize("c", [c for c in R.SEQ_CASES if c[0] == "fp32"], ids=R.seq_case_id)
def test_seq_embed_ref_against_the_oracle_and_the_incremental_chain(c):
    _, E, B, Lp, nvk, T, Q, L_act, n_pos_c = c
    store, pmask, sep, obs, act, table, n_pos = R.seq_inputs(E, B, Lp, nvk, T, Q, L_act, n_pos_c)
    prompt = store.transpose(0, 1)
    x, m = R.seq_embed_ref(prompt, pmask, sep, obs, act, table, n_pos, L_act)
    L = Lp + 1 + T * Q + L_act
    from oracle.baseline_oracle import OracleGatoPolicy
    cap = {}

    class P(OracleGatoPolicy):
        def __init__(self):
            self.sd, self.n_queries, self.embed_dim = {"prompt_sep_token": sep}, Q, E

        def _hfgpt(self, tokens, key_mask, position_ids):
            cap.update(tokens=tokens, mask=key_mask, pos=position_ids)
            return tokens

    P()._decoder_only_forward(obs, act[:L_act] if L_act else None, store, pmask.bool())
    assert cap["tokens"].shape == (B, L, E) and torch.equal(cap["mask"], m.bool())
    assert torch.equal(cap["tokens"] + table[cap["pos"].clamp(0, n_pos - 1)], x)
    # prefill + steps == the whole sequence, bit for bit (the references against each other)
    st = R.seq_state(B, n_pos)
    xp, mp = R.seq_prefill_ref(st, prompt, pmask, sep, table, n_pos)
    assert torch.equal(xp, x[:, : Lp + 1]) and torch.equal(mp, m[:, : Lp + 1]) and torch.equal(st["posbase"].long(), pmask.long().sum(dim=1) + 1)
    row0 = Lp + 1
    for t in range(T):
        has_act = 1 if t else 0
        if t > L_act:
            break
        Ln = Q + has_act
        if row0 + Ln > min(L, n_pos):
            break
        xs = R.seq_step_ref(st, obs[t], act[t - 1] if t else act[0], table, n_pos, row0, has_act)
        assert torch.equal(xs, x[:, row0:row0 + Ln])
        row0 += Ln
    assert torch.equal(st["cache_mask"][:, :row0], m[:, :row0]) and (st["cache_mask"][:, row0:] == R.CANARY_U8).all()
    _differs(R.seq_case_id(c), "position ids off by one", R.seq_embed_ref(prompt, pmask, sep, obs, act, table, n_pos, L_act, shift=1)[0], x)


def test_seq_step_fresh_sample_and_restart_against_a_loop():
    E, B, Q, n_pos = 256, 3, 4, 40
    gen = torch.Generator().manual_seed(13)
    table = torch.randn(n_pos, E, generator=gen)
    st = R.seq_state(B, n_pos)
    st["cache_mask"][:] = 1
    st["posbase"][:] = torch.tensor([5, 9, 38], dtype=torch.int32)
    R.seq_restart_ref(st, [2, 0], 6, 30)
    assert st["fresh"].tolist() == [1, 0, 1] and st["cache_mask"][0, 6:30].sum() == 0 and st["cache_mask"][1].all() and st["cache_mask"][2, 30:].all()
    obs, act = torch.randn(B, Q, E, generator=gen), torch.full((B, E), float("nan"))
    act[1] = torch.randn(E, generator=gen)
    base = st["posbase"].tolist()
    x = R.seq_step_ref(st, obs, act, table, n_pos, 10, 1)
    assert torch.isfinite(x).all(), "a fresh sample's poisoned act_tok row reached the output"
    for b, fr in enumerate((1, 0, 1)):
        run = base[b]
        for i in range(Q + 1):
            mk = 0 if (i == 0 and fr) else 1
            tok = (torch.zeros(E) if fr else act[b]) if i == 0 else obs[b, i - 1]
            assert torch.equal(x[b, i], tok + table[min(run, n_pos - 1)]) and st["cache_mask"][b, 10 + i] == mk
            run += mk
        assert st["posbase"][b] == run
    assert st["fresh"].tolist() == [0, 0, 0]


# ================================================================================================================== tables, binding
def test_case_tables_hold_what_the_gpu_file_needs():
    kern = {(R.norm_kernel_of(c[0], c[1], c[2], c[2] + c[4]), c[1], c[5]) for c in R.LN_CASES}
    for rms in (0, 1):
        assert {(f"rows2<{n}>", "bf16", rms) for n in (1, 2, 3, 4)} | {("layernorm_T", "bf16", rms), ("layernorm", "fp32", rms), ("layernorm", "bf16", rms)} <= kern
    assert {c[2] for c in R.LN_CASES if R.norm_kernel_of(*c[:3], c[2] + c[4]) == "layernorm_T"} >= {256, 320, 384, 1024}    # E + 4 routes E % 256 == 0 there
    assert {c[6] for c in R.LN_CASES} == set(R.NORM_REGIMES) and {c[3] for c in R.LN_CASES} >= {1, 2, 7, 33, R.BIG_ROWS}
    big = (R.BIG_ROWS + 1) // 2
    assert (big + 3) // 4 == 2049                                                  # one workgroup past the cap: the grid-stride loop runs once
    for cases, cid in ((R.LN_CASES, R.norm_case_id), (R.LN2_CASES, R.norm_case_id), (R.RMS_STATS_CASES, R.norm_case_id), (R.DEC_CASES, R.dec_case_id),
                       (R.PP_CASES, R.pp_case_id), (R.PA_CASES, R.pa_case_id), (R.ACT_CASES, R.act_case_id), (R.SEQ_CASES, R.seq_case_id)):
        assert len({cid(c) for c in cases}) == len(cases)
        assert {c[1] if cases[0][0] not in R.PRECS else c[0] for c in cases} == set(R.PRECS)
    assert {R.pp_slab(B if lst is None else len(lst), Lp) for _, _, B, Lp, _, _, lst in R.PP_CASES} == {8, 64}
    assert {c[3] for c in R.PP_CASES} >= {1, 255, 256, 257, 600}
    assert max(T * Q + La for _, _, _, T, Q, La, _ in R.DEC_CASES) == 512           # the largest sequence dec_embed_kernel's pos_s[512] holds


SEQ_NORM_OPS = ("vima_op_norm", "vima_op_prompt_assemble", "vima_op_dec_embed", "vima_op_dec_embed_step", "vima_op_restart_samples",
                "vima_op_prompt_pos", "vima_op_gather_pred", "vima_op_action_l1", "vima_op_add_row_table", "vima_op_rows_to_headmajor",
                "vima_op_kv_scatter", "vima_op_seq_kv_store", "vima_op_broadcast_rows", "vima_op_seq_embed", "vima_op_seq_embed_prefill",
                "vima_op_seq_embed_step", "vima_op_seq_restart")


def test_header_library_and_binding_agree_on_the_entry_points():
    from vima_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vima_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in SEQ_NORM_OPS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} not declared in include/vima_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.ctypes.c_int and len(args) == len(params) and params[0] == "VimaHandle* h" and params[-1] == "vima_stream_t stream"
        for p, a in zip(params, args):
            assert (a is _lib.ctypes.c_int) == p.startswith("int "), (name, p)
            assert (a is _lib.c_i64) == p.startswith("int64_t "), (name, p)
            assert (a in (_lib.vp, _lib.ctypes.POINTER(_lib.VimaNormDesc))) == ("*" in p or p.startswith("vima_stream_t")), (name, p)
        assert hasattr(lib, name)
    m = re.search(r"typedef struct VimaNormDesc \{(.*?)\} VimaNormDesc;", src, flags=re.S)
    fields = [f.strip().lstrip("*") for decl in m.group(1).split(";") if decl.strip() for f in decl.strip().split(",")]
    fields = [f.split()[-1].lstrip("*") for f in fields]
    assert fields == [n for n, _ in _lib.VimaNormDesc._fields_]
    assert _lib.NORM_KIND == {"ln": 0, "ln_T": 1, "ln2": 2, "rms_stats": 3} and all(f"VIMA_NORM_{k}" in src for k in ("LN = 0", "LN_T = 1", "LN2 = 2", "RMS_STATS = 3"))
    assert lib.vima_abi_version() == _lib.ABI_VERSION == 5


def test_zz_print_the_worst_ratios():
    """Last in the file: the CPU-measured ratios the gates rest on (profiles/seq_norm_errors.txt records them)."""
    for family in sorted(_worst):
        ratio, cid = _worst[family]
        print(f"[seq-norm ref] {family}: worst {ratio:.3f} at {cid}")
