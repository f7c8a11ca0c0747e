"""CPU references, input builders, case tables and gates shared by tests/test_seq_norm_reference.py (which pins all of this on the CPU) and
tests/test_seq_norm_gpu.py (which holds the norm and sequence-assembly kernels of elementwise.hip / baseline_kernels.hip / episode_rows.hip
against it, one launch per case, per output element):

  layernorm_kernel<T>, <bf16, bf16>, layernorm_rows2_kernel<1..4>, layernorm2_kernel, rms_stats_kernel              (vima_op_norm)
  prompt_assemble_kernel, prompt_assemble_stats_kernel                                                               (vima_op_prompt_assemble)
  dec_embed_kernel, dec_embed_chunk_kernel at T = 1, prompt_pos_kernel, gather_pred_kernel                           (vima_op_dec_embed, _step ...)
  action_l1_kernel, add_row_table_kernel, broadcast_rows_kernel                                                      (vima_op_action_l1 ...)
  seq_embed_kernel, also as the prefill (vima_op_seq_embed_prefill), seq_embed_chunk_kernel at T = 1 (vima_op_seq_embed_step)
  kv_rows_kernel in three of its forms (vima_op_rows_to_headmajor, vima_op_kv_scatter, vima_op_seq_kv_store), episode_restart_kernel with and
  without a position counter (vima_op_restart_samples, vima_op_seq_restart)

References are fp64 (norms, ssq, action_l1) or exact fp32 (everything else: a gather plus ONE IEEE fp32 add, which torch on the CPU performs
with the same bits), and are written with cumsum / cat / index_select / reshape / permute only -- none of the kernels' index arithmetic.
The semantics are the reference project's (the lines each kernel's header comment cites); where this project diverges ON PURPOSE the
reference mirrors it and says so:
  * position clamps: a position id of -1 (first token masked; the reference project raises) reads row 0, an id >= n_pos (it raises too) reads
    row n_pos - 1 -- `clamp_pos`;
  * the action slot of a `fresh` (just restarted) sample is a masked token that consumes no position id -- `dec_step_ref`, `seq_step_ref`;
  * in the decoder-only (seq) form zeros are embedded for that slot instead of the caller's act_tok row -- `seq_step_ref`.

Gates (every constant derived here or in the issue, measured on the CPU by test_seq_norm_reference.py, none taken from a GPU run):
  exact kernels   fp32 outputs bit-equal to torch fp32 `token + pos_row` (copies: to the source), operand-type outputs to `.bfloat16()` of it,
                  masks and counters equal as integers, everything outside the written region still the canary
  ssq             |err| <= 1.01 (9 + ceil(E / 256)) 2^-24 ssq   (non-negative terms: one product rounding, two adds inside the float4, a
                  per-lane chain of E / 256, six wave_sum levels)
  action_l1       |err| <= (K + 4) 2^-24 (sum_k |x_k| |w_k| + |b|)                                                  [bf16: + 1.01 2^-8 |ref|]
  LayerNorm / RMSNorm, per row (s^2 the biased variance, or the mean square under rms; mx = max |x| of the row)
                  tol = 2^-23 (4 + c_E mx / sqrt(s^2 + eps));  |err| <= tol |g_c| (|xhat_c| + 1) + 2^-23 |ref| + 1e-7   [bf16: + 1.01 2^-8 |ref|]
                  the form pinned for vit_embed at E = 768 with c_E = 4. RE-DERIVED here: c_E = (9 + ceil(E / 256)) / 2 (5 .. 6.5). With
                  c_E = 4 the two-pass fp32 restatement of test_seq_norm_reference.py reaches 0.56 of the gate on exactly constant rows
                  at E = 1024 (0.36 at E = 256), over the half it may use. Cause: the c_E term is the error of the MEAN carried to the
                  output, delta rstd |g_c|. Every kernel sums a row through 8 + ceil(E / 256) levels (2 or 3 inside the lane's vector, a
                  per-lane chain of E / 256, 6 or 5 shuffle levels) and divides once, so |delta| <= (9 + ceil(E / 256)) 2^-24 mx to first
                  order -- the depth count of the ssq gate -- and on a constant row every partial sum of a level rounds the same way, so
                  the roundings add up instead of averaging out; c_E = 4 allowed 8 2^-24 mx. Measured on the CPU against fp64 with the new
                  constant: restatement <= 0.35 of the gate in every regime at E = 256 .. 1024 (layernorm2, second output: 0.36).
  layernorm2      first output y: the gate above. Second output z, against the fp64 LN of the fp64 y: its own gate (of the fp64 y) + the
                  first gate times the second LN's Lipschitz factor |g2_c| / sqrt(var2 + eps2)                    [bf16: + 1.01 2^-8 |ref|]
No GPU and no vima_amd import here."""
import functools
import math

import torch

PRECS = ("fp32", "bf16")
U_BF16 = 2.0 ** -8
CANARY = -77.0                      # exact in bf16; no kernel output below equals it
CANARY_U8 = 0xA5


def ln_c(E):
    """The constant of the LN gate's mean term (module docstring)."""
    return (9 + math.ceil(E / 256)) / 2.0


def bf(x):
    return x.bfloat16().float()


def rounded(prec, x):
    """What launch_cast hands the kernel / what an operand-type store keeps."""
    return bf(x) if prec == "bf16" else x


def with_bf16_term(prec, gate, ref):
    return gate + 1.01 * U_BF16 * ref.abs() if prec == "bf16" else gate


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ================================================================================================================== norms
NORM_REGIMES = ("plain", "offset", "lowvar", "constant", "zero", "spike")
LN_EPS, RMS_EPS = 1e-5, 1e-6        # nn.LayerNorm / HF T5LayerNorm
BIG_ROWS = 16387                    # first row count past the 2048-workgroup cap of rows2: one grid-stride round with an odd tail


def norm_kernel_of(kind, prec, E, ldin):
    """The routing of launch_layernorm / launch_layernorm_T, restated (VIMA_LN_ROWS2 unset)."""
    if kind == "ln2":
        return "layernorm2"
    if kind == "rms_stats":
        return "rms_stats"
    if kind == "ln" or prec == "fp32":
        return "layernorm"
    return f"rows2<{E // 256}>" if E % 256 == 0 and ldin % 8 == 0 else "layernorm_T"


def _ln_cases():
    out = []
    for p in PRECS:
        for rms in (0, 1):
            # ln_T: on a bf16 handle E % 256 == 0 takes rows2<1..4> at ldin % 8 == 0 and the one-wave kernel at ldin = E + 4
            for E in (256, 512, 768, 1024, 320, 384):
                for rows in (1, 2, 7, 33):
                    for pad in (0, 8, 4):
                        if rows in (1, 33) or pad == 0:
                            out.append(("ln_T", p, E, rows, pad, rms, "plain"))
            for E in (256, 320, 768, 1024):
                for rows, pad in ((1, 0), (7, 4), (33, 0)):
                    out.append(("ln", p, E, rows, pad, rms, "plain"))
            for E in (256, 320, 1024):
                for regime in NORM_REGIMES[1:]:
                    out.append(("ln_T", p, E, 7, 0, rms, regime))
                    out.append(("ln", p, E, 7, 0, rms, regime))
    out += [("ln_T", "bf16", 256, BIG_ROWS, 0, 0, "plain"), ("ln_T", "bf16", 256, BIG_ROWS, 4, 1, "plain"), ("ln", "fp32", 256, BIG_ROWS, 0, 0, "plain")]
    return out


LN_CASES = _ln_cases()
LN2_CASES = [("ln2", p, E, rows, pad, 0, r) for p in PRECS for E in (256, 320, 768) for rows, pad in ((1, 0), (7, 4), (33, 0)) for r in ("plain", "offset", "lowvar")]
RMS_STATS_CASES = [("rms_stats", p, E, rows, 0, 1, r) for p in PRECS for E in (256, 320, 768, 1024) for rows in (1, 7, 33) for r in ("plain", "zero", "spike")]


def norm_case_id(c):
    kind, p, E, rows, pad, rms, regime = c
    return f"{kind}-{p}-E{E}-r{rows}-ld+{pad}-{'rms' if rms else 'ln'}-{regime}"


@functools.lru_cache(maxsize=None)
def norm_inputs(E, rows, pad, regime, seed=0):
    """x fp32 [rows, E + pad] (the pad columns hold 1e3: a kernel that reads them is far off), g ~ N(1, 0.2), b ~ N(0, 0.2), and a second
    pair g2, b2 for layernorm2. plain 3 N(0,1) + 0.5; offset 300 + N(0,1); lowvar 0.5 + sqrt(1e-5) N(0,1) (variance of the order of eps);
    constant: every element of a row the same value (a different one per row); zero: all zeros; spike: N(0,1) with one element 1e4."""
    gen = _gen(11, E, min(rows, 64), pad, NORM_REGIMES.index(regime), seed)
    n = torch.randn(rows, E, generator=gen)
    if regime == "plain":
        x = 3 * n + 0.5
    elif regime == "offset":
        x = 300 + n
    elif regime == "lowvar":
        x = 0.5 + math.sqrt(1e-5) * n
    elif regime == "constant":
        x = (0.7 + torch.arange(rows, dtype=torch.float32)[:, None] * 1.3).expand(rows, E).clone()
    elif regime == "zero":
        x = torch.zeros(rows, E)
    else:
        assert regime == "spike"
        x = n.clone()
        x[torch.arange(rows), torch.randint(0, E, (rows,), generator=gen)] = 1e4
    full = torch.full((rows, E + pad), 1e3)
    full[:, :E] = x
    g, b = 1.0 + 0.2 * torch.randn(E, generator=gen), 0.2 * torch.randn(E, generator=gen)
    g2, b2 = 1.0 + 0.2 * torch.randn(E, generator=gen), 0.2 * torch.randn(E, generator=gen)
    return full, g, b, g2, b2


def norm_ref64(x, g, b, eps, rms, unbiased=False, drop_eps=False, keep_mean=False):
    """x fp64 [rows, E] -> (ref, gate32, rstd): explicit two-pass LayerNorm (rms: no mean, the mean square). The keyword arguments are the
    mutations of test_seq_norm_reference.py."""
    E = x.shape[1]
    mean = torch.zeros_like(x[:, :1]) if rms else x.sum(dim=1, keepdim=True) / E
    var = ((x - mean) ** 2).sum(dim=1, keepdim=True) / (E - 1 if unbiased else E)
    rstd = 1.0 / torch.sqrt(var + (0.0 if drop_eps else eps))
    xhat = (x if keep_mean else x - mean) * rstd
    ref = xhat * g
    if b is not None:
        ref = ref + b
    tol = 2.0 ** -23 * (4 + ln_c(E) * x.abs().max(dim=1, keepdim=True).values / torch.sqrt(var + eps))
    return ref, tol * g.abs() * (xhat.abs() + 1) + 2.0 ** -23 * ref.abs() + 1e-7, rstd


def norm_operands(c):
    """(x [rows, E] as the kernel reads it, g, b or None, eps) of an LN case: a bf16 stream (ln_T on a bf16 handle) is rounded first."""
    kind, prec, E, rows, pad, rms, regime = c
    full, g, b, _, _ = norm_inputs(E, rows, pad, regime)
    x = full[:, :E]
    if kind == "ln_T":
        x = rounded(prec, x)
    return x, g, (None if rms else b), (RMS_EPS if rms else LN_EPS)


@functools.lru_cache(maxsize=None)
def _ln_reference(kind, bf_in, E, rows, pad, rms, regime):
    x, g, b, eps = norm_operands((kind, "bf16" if bf_in else "fp32", E, rows, pad, rms, regime))
    ref, g32, _ = norm_ref64(x.double(), g.double(), None if b is None else b.double(), eps, rms)
    return ref, g32


def ln_reference(c):
    """-> (ref fp64 [rows, E], gate of the fp32 output, gate of the operand-type output)."""
    kind, prec, E, rows, pad, rms, regime = c
    ref, g32 = _ln_reference(kind, kind == "ln_T" and prec == "bf16", E, rows, pad, rms, regime)
    return ref, g32, with_bf16_term(prec, g32, ref)


@functools.lru_cache(maxsize=None)
def _ln2_reference(E, rows, pad, regime):
    full, g, b, g2, b2 = norm_inputs(E, rows, pad, regime)
    y, gate1, _ = norm_ref64(full[:, :E].double(), g.double(), b.double(), LN_EPS, 0)
    z, gate2, rstd2 = norm_ref64(y, g2.double(), b2.double(), LN_EPS, 0)
    carried = gate1 * g2.double().abs() * rstd2
    return y, gate1, z, gate2 + carried


def ln2_reference(c):
    """-> (y, gate of y in fp32, gate of y in the operand type, z, gate of z in the operand type). z is the fp64 LN of the fp64 y."""
    _, prec, E, rows, pad, _, regime = c
    y, g1, z, g2 = _ln2_reference(E, rows, pad, regime)
    return y, g1, with_bf16_term(prec, g1, y), z, with_bf16_term(prec, g2, z)


def ssq_reference(x):
    """fp32 rows -> (ssq fp64 [rows], gate)."""
    E = x.shape[1]
    s = (x.double() ** 2).sum(dim=1)
    return s, 1.01 * (9 + math.ceil(E / 256)) * 2.0 ** -24 * s


# ================================================================================================================== positions
def clamp_pos(pos, n_pos, lower=True, upper=True):
    """DIVERGENCE (named in the module docstring): ids < 0 read row 0 and ids >= n_pos row n_pos - 1 where the reference project raises.
    lower / upper = False are the mutations 'clamp missing': the id wraps the way an unchecked index would leave the table."""
    if lower:
        pos = pos.clamp(min=0)
    if upper:
        pos = pos.clamp(max=n_pos - 1)
    return pos % n_pos


def _embed(tok, pos, table):
    """token + positions_embed[pos] in fp32: ONE IEEE add per element."""
    assert tok.dtype == torch.float32 and table.dtype == torch.float32
    return tok + table.index_select(0, pos.reshape(-1)).view(*pos.shape, table.shape[1])


def interleave(obs_tok, obs_mask, act_tok, L):
    """[o_1 .. o_Q, a] per step (vima_policy.py:124-144): obs_tok [T, B, Q, E], obs_mask [T, B, Q], act_tok [L_act, B, E] or None ->
    tokens [B, L, E], masks i64 [B, L] (the action slots valid)."""
    T, B, Q, E = obs_tok.shape
    n_act = 0 if act_tok is None else act_tok.shape[0]
    parts = [] if act_tok is None else [act_tok]
    act = torch.cat(parts + [torch.zeros(T - n_act, B, E)], dim=0).view(T, B, 1, E)
    tok = torch.cat([obs_tok, act], dim=2).permute(1, 0, 2, 3).reshape(B, T * (Q + 1), E)
    msk = torch.cat([obs_mask.long(), torch.ones(T, B, 1, dtype=torch.long)], dim=2).permute(1, 0, 2).reshape(B, T * (Q + 1))
    return tok[:, :L].contiguous(), msk[:, :L].contiguous()


# ------------------------------------------------------------------------------------------------------------------ dec_embed
DEC_MASKS = ("valid", "first_masked", "step_masked", "overflow")
# (prec, E, B, T, Q, L_act, mask kind); n_pos = 512 except "overflow" (n_pos = 3)
DEC_CASES = ([(p, E, B, T, Q, L_act, m) for p in PRECS for E, B in ((256, 3), (320, 1), (768, 5)) for T in (1, 2, 3) for Q in (1, 4)
              for L_act in (T - 1, T) for m in DEC_MASKS if not (m == "step_masked" and T == 1)] +
             [(p, 256, 1, 256, 1, 256, "valid") for p in PRECS])   # T Q + L_act = 512, all of pos_s[512]; 513 is refused (DEC_REFUSED)
DEC_REFUSED = (257, 1, 256)          # T, Q, L_act: 513 rows


def dec_case_id(c):
    p, E, B, T, Q, L_act, m = c
    return f"dec_embed-{p}-E{E}-B{B}-T{T}-Q{Q}-La{L_act}-{m}"


@functools.lru_cache(maxsize=None)
def dec_inputs(E, B, T, Q, L_act, mkind, seed=0):
    """obs_tok [T, B, Q, E], obs_mask u8 [T, B, Q], act_tok [max(L_act, 1), B, E], pos_table [n_pos, E], n_pos."""
    gen = _gen(21, E, B, T, Q, L_act, DEC_MASKS.index(mkind), seed)
    obs = torch.randn(T, B, Q, E, generator=gen)
    act = torch.randn(max(L_act, 1), B, E, generator=gen)
    n_pos = 3 if mkind == "overflow" else 512
    table = torch.randn(n_pos, E, generator=gen)
    mask = torch.ones(T, B, Q, dtype=torch.uint8)
    if mkind == "first_masked":
        mask[0, :, 0] = 0
        if Q > 1:
            mask[-1, 0, 1:3] = 0
    elif mkind == "step_masked":
        mask[0, :, :] = 0                         # every observation of step 0: the ids start at the first action
        mask[1, -1, :] = 0
    elif mkind == "valid" and T * Q > 8:
        mask = (torch.rand(T, B, Q, generator=gen) < 0.7).to(torch.uint8)
    return obs, mask, act, table, n_pos


def dec_embed_ref(obs, mask, act, table, n_pos, L_act, shift=0, count_masked=False, per_step=False, lower=True, upper=True):
    """-> (x fp32 [B, L, E], mask u8 [B, L], pos i64 [B, L]). The keyword arguments are mutations."""
    T, B, Q, E = obs.shape
    L = T * Q + L_act
    tok, msk = interleave(obs, mask, act[:L_act] if L_act else None, L)
    counted = torch.ones_like(msk) if count_masked else msk
    if per_step:      # cumsum restarted at every step's first token
        pad = torch.cat([counted, torch.zeros(B, T * (Q + 1) - L, dtype=torch.long)], dim=1).view(B, T, Q + 1)
        pos = (torch.cumsum(pad, dim=2) - 1).view(B, -1)[:, :L]
    else:
        pos = torch.cumsum(counted, dim=1) - 1                                   # vima_policy.py:145-146
    pos = clamp_pos(pos + shift, n_pos, lower, upper)
    return _embed(tok, pos, table), msk.to(torch.uint8), pos


def gather_pred_ref(x, T, Q, row=None):
    """tokens_out[Q - 1 :: Q + 1] (vima_policy.py:158): x [B, Lq, E] -> [T, B, E]."""
    return x[:, (Q - 1 if row is None else row)::Q + 1][:, :T].transpose(0, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ dec_embed_step
def dec_state(B, Lmax):
    return {"hist_mask": torch.full((B, Lmax), CANARY_U8, dtype=torch.uint8), "poscnt": torch.zeros(B, dtype=torch.int32),
            "fresh": torch.zeros(B, dtype=torch.uint8)}


def dec_step_ref(state, obs, mask, act, table, n_pos, L_hist, has_act):
    """One env step on the episode state (updated in place): obs [B, Q, E], mask u8 [B, Q], act [B, E] -> x fp32 [B, Q + has_act, E].
    DIVERGENCE: a fresh sample's action slot is a masked token (its act row is still embedded, at the position id of the previous token)."""
    B, Q, E = obs.shape
    fresh = state["fresh"].long()
    mk, tok = mask.long(), obs
    if has_act:
        mk = torch.cat([(1 - fresh)[:, None], mk], dim=1)
        tok = torch.cat([act[:, None], obs], dim=1)
    pos = clamp_pos(state["poscnt"].long()[:, None] + torch.cumsum(mk, dim=1) - 1, n_pos)      # xattn_gpt.py:96-103, running across steps
    Ln = Q + has_act
    state["hist_mask"][:, L_hist:L_hist + Ln] = mk.to(torch.uint8)
    state["poscnt"] += mk.sum(dim=1).to(torch.int32)
    state["fresh"].zero_()
    return _embed(tok, pos, table)


def restart_ref(state, flags):
    f = flags.bool()
    state["hist_mask"][f] = 0
    state["poscnt"][f] = 0
    state["fresh"][f] = 1


def dec_chain(E, B, Q, n_pos, steps=4, restart_at=None, seed=0):
    """The inputs of a chain of env steps: per step obs [B, Q, E], mask u8 [B, Q], act [B, E] (the action BEFORE the step; unused at step 0),
    restart flags u8 [B] applied before the step (None: no restart)."""
    gen = _gen(71, E, B, Q, n_pos, seed)
    table = torch.randn(n_pos, E, generator=gen)
    out = []
    for t in range(steps):
        mask = (torch.rand(B, Q, generator=gen) < 0.7).to(torch.uint8)
        if t == 0:
            mask[0, 0] = 0
        flags = None
        if restart_at == t:
            flags = torch.zeros(B, dtype=torch.uint8)
            flags[::2] = 1
        out.append((torch.randn(B, Q, E, generator=gen), mask, torch.randn(B, E, generator=gen), flags))
    return table, out


# ------------------------------------------------------------------------------------------------------------------ prompt_pos
# (prec, E, B samples, Lp, layout, mask kind, list or None); the slab is 64 when n_blocks ceil(Lp / 64) >= 512, else 8
PP_CASES = ([(p, E, B, Lp, lay, m, None) for p in PRECS for E, B, Lp, lay, m in (
                (256, 3, 1, "BLE", "holes"), (320, 1, 255, "LBE", "holes"), (256, 3, 256, "BLE", "holes"), (768, 5, 257, "LBE", "holes"),
                (256, 3, 600, "LBE", "empty_sample"), (256, 256, 65, "BLE", "holes"), (256, 3, 40, "BLE", "overflow"))] +
            [(p, 320, 5, 70, "LBE", "empty_sample", (4, 0, 0, 2, 4, 1, 4)) for p in PRECS] +
            [(p, 256, 3, 40, "BLE", "holes", (2, 0, 1)) for p in PRECS])


def pp_case_id(c):
    p, E, B, Lp, lay, m, lst = c
    return f"prompt_pos-{p}-E{E}-B{B}-Lp{Lp}-{lay}-{m}" + ("" if lst is None else "-list" + "".join(map(str, lst)))


def pp_slab(n_blocks, Lp):
    return 64 if n_blocks * ((Lp + 63) // 64) >= 512 else 8


@functools.lru_cache(maxsize=None)
def pp_inputs(E, B, Lp, layout, mkind, seed=0):
    """-> (storage, sb, sl, mask u8 [B, Lp], table, n_pos): storage is [B, Lp, E] ("BLE": sb = Lp E, sl = E) or [Lp, B, E] ("LBE": sb = E,
    sl = B E), the element strides of sample and position."""
    gen = _gen(31, E, B, Lp, layout == "LBE", mkind == "overflow", seed)
    store = torch.randn((B, Lp, E) if layout == "BLE" else (Lp, B, E), generator=gen)
    n_pos = 7 if mkind == "overflow" else max(Lp, 2)
    table = torch.randn(n_pos, E, generator=gen)
    mask = (torch.rand(B, Lp, generator=gen) < 0.6).to(torch.uint8)
    if Lp > 1:
        mask[0, 0] = 0                                # the lower clamp
        mask[-1, 0] = 1
    if mkind == "empty_sample":
        mask[B // 2] = 0
    if mkind == "overflow":
        mask[:] = 1
    sb, sl = (Lp * E, E) if layout == "BLE" else (E, B * E)
    return store, sb, sl, mask, table, n_pos


def pp_view(store, layout, swap=False):
    """The [B, Lp, E] view of the storage. swap (seq-first storage only) is the mutation 'sl and sb exchanged'."""
    if layout == "BLE":
        assert not swap
        return store
    Lp, B, E = store.shape
    if not swap:
        return store.transpose(0, 1)
    assert (B - 1) * B + Lp <= Lp * B
    return store.as_strided((B, Lp, E), (B * E, E, 1))


def prompt_pos_ref(view, mask, table, n_pos, lst=None, scatter=False, shift=0, count_masked=False, lower=True, upper=True):
    """prompt + xattn_positions_embed[cumsum(mask) - 1] (vima_policy.py:147, xattn_gpt.py:110-114): view [B, Lp, E] -> fp32 [n_blocks, Lp, E].
    lst: output block r comes from sample lst[r]. scatter (lst a permutation) is the mutation 'list applied to the output block'."""
    counted = torch.ones_like(mask, dtype=torch.long) if count_masked else mask.long()
    pos = clamp_pos(torch.cumsum(counted, dim=1) - 1 + shift, n_pos, lower, upper)
    out = _embed(view.contiguous(), pos, table)
    if lst is None:
        return out
    idx = torch.tensor(lst, dtype=torch.long)
    if scatter:
        assert sorted(lst) == list(range(out.shape[0]))
        return torch.zeros_like(out).index_copy_(0, idx, out)
    return out.index_select(0, idx)


# ------------------------------------------------------------------------------------------------------------------ prompt_assemble
# (prec, E, B, L)
PA_CASES = [(p, E, B, L) for p in PRECS for E, B, L in ((256, 1, 5), (320, 3, 9), (768, 5, 13))]


def pa_case_id(c):
    return "prompt_assemble-{}-E{}-B{}-L{}".format(*c)


@functools.lru_cache(maxsize=None)
def pa_inputs(E, B, L, seed=0):
    """tok_src i32 [B L]: words (>= 0, some repeated), pads (-1), object rows (<= -2, masks 0 and 1, some repeated); word_ids i64 [n_words]
    into word_table [vocab, E]; obj_tokens [n_obj, E], obj_mask u8 [n_obj]."""
    gen = _gen(41, E, B, L, seed)
    rows, n_words, n_obj, vocab = B * L, 6, 5, 11
    kind = torch.randint(0, 3, (rows,), generator=gen)
    kind[:3] = torch.tensor([0, 1, 2])[: min(3, rows)]
    src = torch.where(kind == 0, torch.randint(0, n_words, (rows,), generator=gen),
                      torch.where(kind == 1, torch.full((rows,), -1), -2 - torch.randint(0, n_obj, (rows,), generator=gen))).to(torch.int32)
    word_ids = torch.randint(0, vocab, (n_words,), generator=gen, dtype=torch.int64)
    obj_mask = torch.tensor([1, 0, 1, 0, 3], dtype=torch.uint8)     # any non-zero byte is "valid"
    return src, word_ids, torch.randn(vocab, E, generator=gen), torch.randn(n_obj, E, generator=gen), obj_mask


def prompt_assemble_ref(src, word_ids, word_table, obj_tokens, obj_mask):
    """vima_policy.py:168-233: -> (x fp32 [rows, E], mask u8 [rows]). One pool [words | a zero row | objects] and one index_select."""
    words = word_table.index_select(0, word_ids)                                   # word_embd.py:18-23
    nw, E = words.shape
    pool = torch.cat([words, torch.zeros(1, E), obj_tokens], dim=0)
    pmask = torch.cat([torch.ones(nw, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), (obj_mask != 0).to(torch.uint8)])
    s = src.long()
    idx = torch.where(s >= 0, s, torch.where(s == -1, torch.full_like(s, nw), nw - 1 - s))
    return pool.index_select(0, idx), pmask.index_select(0, idx)


# ------------------------------------------------------------------------------------------------------------------ action_l1, add_row_table
ACT_CASES = [(p, K, R, ldo, col0) for p in PRECS for K, R, ldo, col0 in ((2, 1, 256, 0), (4, 7, 1024, 256), (2, 33, 1024, 768), (4, 33, 260, 4))]


def act_case_id(c):
    return "action_l1-{}-K{}-R{}-ldo{}-col{}".format(*c)


@functools.lru_cache(maxsize=None)
def act_inputs(K, R, seed=0):
    gen = _gen(51, K, R, seed)
    idx = torch.randint(0, 100 if K == 2 else 50, (R, K), generator=gen, dtype=torch.int64)
    if K == 2:
        idx[:, 0] %= 50
    return idx, torch.randn(256, K, generator=gen), 0.5 * torch.randn(256, generator=gen)


def action_bins(K, y_bins=100.0):
    return (50.0, y_bins) if K == 2 else (50.0,) * 4           # vima_policy.py:301-322


def action_l1_ref(idx, W, b, bins):
    """relu(W (idx / bins) + b) (action_embd.py:40-56), the bbox_l1 form of tests/vit_front_reference.py -> (ref fp64 [R, 256], gate32)."""
    K = idx.shape[1]
    x = idx.double() / torch.tensor(bins, dtype=torch.float64)
    y = x @ W.double().t() + b.double()
    return torch.relu(y), (K + 4) * 2.0 ** -24 * (x.abs() @ W.double().abs().t() + b.double().abs())


def add_row_table_ref(out, table, sel, group):
    """out[r] += table[clamp(sel[r / group], 0, 1)]: the end-effector term of obs_fusion (vima_policy.py:242-259)."""
    rows = out.shape[0]
    return out + table.index_select(0, sel.clamp(0, 1)).repeat_interleave(group, dim=0)[:rows]


# ------------------------------------------------------------------------------------------------------------------ copies
def headmajor_ref(x, D, swap_ld=False):
    """rows [L, N] -> [N / D, L, D]; swap_ld: the mutation 'L and D exchanged' ([N / D, D, L])."""
    L, N = x.shape
    v = x.view(L, N // D, D)
    return (v.permute(1, 2, 0) if swap_ld else v.permute(1, 0, 2)).contiguous()


def kv_scatter_ref(x, lst, n_blocks, L, N, D, hm):
    """x [n, L, N] -> cache [n_blocks, L N] with block lst[r] = sample r (row-major, or head-major), every other block the canary."""
    n = x.shape[0]
    blk = x.view(n, L, N // D, D).permute(0, 2, 1, 3) if hm else x
    out = torch.full((n_blocks, L * N), CANARY)
    out.index_copy_(0, torch.tensor(lst, dtype=torch.long), blk.reshape(n, L * N))
    return out


def seq_kv_store_ref(x, lst, n_blocks, L, N, Lmax):
    """x [n, L, ld_in] columns [0, N) -> rows [0, L) of block lst[r] (None: r) of a cache [n_blocks, Lmax, N]; the rest stays the canary."""
    n = x.shape[0]
    out = torch.full((n_blocks, Lmax, N), CANARY)
    idx = torch.arange(n) if lst is None else torch.tensor(lst, dtype=torch.long)
    out.index_copy_(0, idx, torch.cat([x[:, :, :N], torch.full((n, Lmax - L, N), CANARY)], dim=1))
    return out


def broadcast_ref(src, rows):
    period = src.shape[0]
    return src.repeat((rows + period - 1) // period, 1)[:rows].contiguous()


# ------------------------------------------------------------------------------------------------------------------ seq_embed*
# (prec, E, B, Lp, nv kind, T, Q, L_act, n_pos): nv kind "zero" / "one" / "full" / "mixed" valid prompt tokens
SEQ_CASES = ([(p, E, B, Lp, nv, T, Q, L_act, 0) for p in PRECS for E, B, Lp, nv, T, Q, L_act in (
                (256, 3, 1, "zero", 1, 1, 0), (256, 3, 1, "full", 2, 1, 2), (320, 1, 5, "one", 2, 4, 1), (768, 5, 5, "mixed", 3, 1, 3),
                (256, 3, 70, "mixed", 2, 16, 1), (320, 5, 70, "full", 1, 4, 1), (256, 1, 5, "zero", 2, 4, 2))] +
             [(p, 256, 3, 5, "mixed", 3, 4, 2, 9) for p in PRECS])      # n_pos = 9 < L: the upper clamp


def seq_case_id(c):
    p, E, B, Lp, nv, T, Q, L_act, n_pos = c
    return f"seq_embed-{p}-E{E}-B{B}-Lp{Lp}-{nv}-T{T}-Q{Q}-La{L_act}" + (f"-npos{n_pos}" if n_pos else "")


@functools.lru_cache(maxsize=None)
def seq_inputs(E, B, Lp, nvk, T, Q, L_act, n_pos=0, seed=0):
    """prompt storage [Lp, B, E] (seq-first: sb = E, sl = B E), pmask u8 [B, Lp] (a valid prefix, as the reference project builds it), sep [E],
    obs [T, B, Q, E], act [max(L_act, 1), B, E], table [n_pos, E], n_pos (default: the sequence length + 2)."""
    gen = _gen(61, E, B, Lp, T, Q, L_act, n_pos, seed)
    L = Lp + 1 + T * Q + L_act
    n_pos = n_pos or L + 2
    nv = {"zero": torch.zeros(B), "one": torch.ones(B), "full": torch.full((B,), Lp), "mixed": torch.arange(B) * Lp // max(B - 1, 1)}[nvk].long()
    pmask = (torch.arange(Lp)[None, :] < nv[:, None]).to(torch.uint8)
    return (torch.randn(Lp, B, E, generator=gen), pmask, torch.randn(E, generator=gen), torch.randn(T, B, Q, E, generator=gen),
            torch.randn(max(L_act, 1), B, E, generator=gen), torch.randn(n_pos, E, generator=gen), n_pos)


def seq_positions(pmask, L):
    """vima_gpt_policy.py:126-184 / gpt.py:177-185: prompt token l at min(l, nv - 1), the separator at nv, then nv + 1 ... -> i64 [B, L]."""
    B, Lp = pmask.shape
    nv = pmask.long().sum(dim=1, keepdim=True)
    ar = torch.arange(L)[None, :].expand(B, L)
    return torch.cat([torch.minimum(ar[:, :Lp], nv - 1), nv + ar[:, : L - Lp]], dim=1)


def seq_embed_ref(prompt, pmask, sep, obs, act, table, n_pos, L_act, shift=0):
    """prompt [B, Lp, E] view -> (x fp32 [B, L, E], mask u8 [B, L])."""
    T, B, Q, E = obs.shape
    Lp = pmask.shape[1]
    n_tail = T * Q + L_act
    tail, _ = interleave(obs, torch.ones(T, B, Q, dtype=torch.uint8), act[:L_act] if L_act else None, n_tail)
    tok = torch.cat([prompt, sep.view(1, 1, E).expand(B, 1, E), tail], dim=1)
    L = Lp + 1 + n_tail
    pos = clamp_pos(seq_positions(pmask, L) + shift, n_pos)
    return _embed(tok.contiguous(), pos, table), torch.cat([pmask, torch.ones(B, L - Lp, dtype=torch.uint8)], dim=1)


def seq_state(B, n_pos):
    return {"cache_mask": torch.full((B, n_pos), CANARY_U8, dtype=torch.uint8), "posbase": torch.full((B,), -7, dtype=torch.int32),
            "fresh": torch.zeros(B, dtype=torch.uint8)}


def seq_prefill_ref(state, prompt, pmask, sep, table, n_pos, lst=None):
    """Rows [0, Lp] of the listed samples -> (x [n, Lp + 1, E], mask [n, Lp + 1]); their cache_mask rows [0, Lp] and posbase are written."""
    B, Lp, E = prompt.shape
    idx = torch.arange(B) if lst is None else torch.tensor(lst, dtype=torch.long)
    pm = pmask.index_select(0, idx)
    tok = torch.cat([prompt.index_select(0, idx), sep.view(1, 1, E).expand(len(idx), 1, E)], dim=1)
    pos = clamp_pos(seq_positions(pm, Lp + 1), n_pos)
    mask = torch.cat([pm, torch.ones(len(idx), 1, dtype=torch.uint8)], dim=1)
    state["cache_mask"][:, : Lp + 1] = state["cache_mask"][:, : Lp + 1].index_copy(0, idx, mask)
    state["posbase"].index_copy_(0, idx, (pm.long().sum(dim=1) + 1).to(torch.int32))
    return _embed(tok.contiguous(), pos, table), mask


def seq_step_ref(state, obs, act, table, n_pos, row0, has_act):
    """obs [B, Q, E], act [B, E] -> x [B, Q + has_act, E]. DIVERGENCE: a fresh sample's action row is a masked key that takes no position id,
    and ZEROS are embedded in place of the caller's act row."""
    B, Q, E = obs.shape
    fresh = state["fresh"].long()
    mk, tok = torch.ones(B, Q, dtype=torch.long), obs
    if has_act:
        mk = torch.cat([(1 - fresh)[:, None], mk], dim=1)
        tok = torch.cat([torch.where(fresh.bool()[:, None], torch.zeros_like(act), act)[:, None], obs], dim=1)
    pos = clamp_pos(state["posbase"].long()[:, None] + torch.cumsum(mk, dim=1) - mk, n_pos)     # the id BEFORE the row is counted
    Ln = Q + has_act
    state["cache_mask"][:, row0:row0 + Ln] = mk.to(torch.uint8)
    state["posbase"] += mk.sum(dim=1).to(torch.int32)
    state["fresh"].zero_()
    return _embed(tok.contiguous(), pos, table)


def seq_restart_ref(state, lst, lo, hi):
    idx = torch.tensor(lst, dtype=torch.long)
    cm = state["cache_mask"]
    cm[:, lo:hi] = cm[:, lo:hi].index_fill(0, idx, 0)
    state["fresh"].index_fill_(0, idx, 1)
