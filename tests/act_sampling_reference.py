"""fp64 restatement of the sampling controls of vima_action_select_ex / vima_act_ex (include/vima_hip.h), shared by
tests/test_act_sampling_build.py (budgets, self-checks) and tests/test_act_sampling_gpu.py (the kernel), with the inputs both use.

Per segment of n logits x:  z = x / T (ONE fp32 division; T clamped to [1e-4, 1e4], NaN = 1), everything after in fp64:
rank(i) = #{j : z_j > z_i} + #{j < i : z_j == z_i}; top-k keeps rank < k; top-p (after top-k, q = softmax over the survivors) keeps
the bin of rank r iff the mass of the surviving bins of rank < r is < p; pi = softmax(z) over the kept set K; the inverse CDF of
tests/act_reference.py over pi in bin order, a result outside K moved to the last bin of K at or below it.

A (row, dimension) pair is EXEMPT from a comparison iff some rank-ordered cumulative mass is within CDF_MARGIN of p, or u is within
CDF_MARGIN of a cumulative boundary of pi: there the answer is decided below fp32 resolution. A key is exempt if any of its dimensions is."""
import functools

import numpy as np
import torch

from tests import act_reference as ref

ROWS = 256
SCALES = ref.SCALES
MARGIN = ref.CDF_MARGIN
TEMPERATURES = ("0.25", "1.0", "3.0", "mix")
MIX_VALUES = (0.1, 0.5, 1.0, 2.0, 7.5)
KP = ((0, 1.0), (1, 1.0), (5, 1.0), (50, 1.0), (0, 0.9), (0, 0.5), (10, 0.77), (0, 1e-3))
INPUTS = tuple((kind, s) for kind in ("random", "quantised") for s in SCALES)
STAT_GATE = 2e-5      # the gate of tests/test_act_gpu.py, here relative to max(1, |ref|, sum over the key's dims of max |z|)
ONE_BELOW = np.nextafter(np.float32(1.0), np.float32(0.0))


@functools.lru_cache(maxsize=None)
def logits(kind, scale):
    """random: act_reference.random_logits(scale, rows=256); quantised: the same rounded to quarters (exact ties). Read-only."""
    x = ref.random_logits(scale, rows=ROWS)
    if kind == "quantised":
        x = (np.round(4.0 * x) / 4.0).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def uniforms():
    u = ref.random_uniforms(rows=ROWS)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def temperature(name, rows=ROWS):
    """float32 [rows]: a constant, or "mix" = one of MIX_VALUES per row"""
    if name == "mix":
        g = torch.Generator().manual_seed(3000)
        t = np.asarray(MIX_VALUES, dtype=np.float32)[torch.randint(0, len(MIX_VALUES), (rows,), generator=g).numpy()]
    else:
        t = np.full(rows, float(name), dtype=np.float32)
    t.setflags(write=False)
    return t


def combinations():
    """the 192 (kind, scale, temperature name, k, p)"""
    return [(kind, s, t, k, p) for kind, s in INPUTS for t in TEMPERATURES for k, p in KP]


def clamp_temperature(T):
    T = np.asarray(T, dtype=np.float32).copy()
    T[np.isnan(T)] = 1.0
    return np.clip(T, np.float32(1e-4), np.float32(1e4))


def scaled(x, T):
    """z float32 [R,700]: one correctly rounded fp32 division per element (T None: x itself)"""
    if T is None:
        return np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.asarray(x, dtype=np.float32) / clamp_temperature(T)[:, None]).astype(np.float32)


def ranks(z):
    """[R,n] -> int ranks by the definition (exact comparisons, ties to the lower index)"""
    zi, zj = z[:, :, None], z[:, None, :]
    n = z.shape[1]
    lower = np.arange(n)[None, :] < np.arange(n)[:, None]          # [i, j]: j < i
    return (zj > zi).sum(axis=2) + ((zj == zi) & lower[None]).sum(axis=2)


def kept_set(z, k, p, dtype=np.float64):
    """-> (keep bool [R,n], exempt bool [R]: a rank-ordered cumulative mass within MARGIN of p). dtype float32 emulates the kernel."""
    R, n = z.shape
    rk = ranks(z)
    keep = rk < k if 0 < k < n else np.ones((R, n), dtype=bool)
    exempt = np.zeros(R, dtype=bool)
    if p < 1.0:
        zz = z.astype(dtype)
        e = np.where(keep, np.exp(zz - zz.max(axis=1, keepdims=True)), 0).astype(dtype)
        by_rank = np.zeros((R, n), dtype=dtype)
        np.put_along_axis(by_rank, rk, e, axis=1)
        s = e.sum(axis=1, keepdims=True, dtype=dtype)
        incl = np.cumsum(by_rank, axis=1, dtype=dtype)
        below = np.concatenate([np.zeros((R, 1), dtype), incl[:, :-1]], axis=1)          # mass of the ranks below
        survives = (below / s) < dtype(p)
        exempt = (np.abs(incl.astype(np.float64) / s.astype(np.float64) - p) <= MARGIN).any(axis=1)
        keep = keep & np.take_along_axis(survives, rk, axis=1)
    return keep, exempt


def kept_set_by_sorting(z, k, p):
    """the same kept set from a stable descending sort (valid without ties; stable sort gives ties to the lower index too)"""
    R, n = z.shape
    order = np.argsort(-z.astype(np.float64), axis=1, kind="stable")
    zs = np.take_along_axis(z.astype(np.float64), order, axis=1)
    ks = np.ones((R, n), dtype=bool)
    if 0 < k < n:
        ks[:, k:] = False
    if p < 1.0:
        e = np.where(ks, np.exp(zs - zs[:, :1]), 0.0)
        q = e / e.sum(axis=1, keepdims=True)
        ks &= (np.cumsum(q, axis=1) - q) < p
    keep = np.zeros((R, n), dtype=bool)
    np.put_along_axis(keep, order, ks, axis=1)
    return keep


def _segment(z, k, p, u, given):
    R, n = z.shape
    keep, exempt = kept_set(z, k, p)
    z64 = z.astype(np.float64)
    m = np.where(keep, z64, -np.inf).max(axis=1, keepdims=True)
    e = np.where(keep, np.exp(z64 - m), 0.0)
    s = e.sum(axis=1, keepdims=True)
    pi = e / s
    with np.errstate(invalid="ignore"):
        logpi = np.where(keep, z64 - (m + np.log(s)), -np.inf)
    ent = -np.where(pi > 0, pi * np.where(keep, logpi, 0.0), 0.0).sum(axis=1)
    mode = z.argmax(axis=1)
    if given is not None:
        bins = np.clip(given, 0, n - 1)
    elif u is None:
        bins = mode
    else:
        uu = np.where(np.isnan(u), np.float32(0), np.clip(u, np.float32(0), ONE_BELOW)).astype(np.float64)[:, None]
        c = np.cumsum(pi, axis=1)
        bins = np.minimum((c <= uu).sum(axis=1), n - 1)
        exempt = exempt | (np.abs(c - uu) <= MARGIN).any(axis=1)
        at_or_below = np.where(keep & (np.arange(n)[None, :] <= bins[:, None]), np.arange(n)[None, :], -1).max(axis=1)
        bins = np.where(at_or_below >= 0, at_or_below, mode)
    lp = np.take_along_axis(logpi, bins[:, None], axis=1)[:, 0]
    return keep, pi, bins, lp, ent, exempt


def per_key(a, how=np.sum):
    return np.stack([how(a[:, f:f + w], axis=1) for f, w in zip(ref.KEY_FIRST, ref.KEY_DIMS)], axis=1)


def reference(x, u=None, T=None, k=0, p=1.0, given=None):
    """x float32 [R,700], u float32 [R,12] or None (the mode), T float32 [R] or None, given int [R,12] or None ->
    dict: keep / pi (12 arrays [R,n]), bins [R,12], log_prob / entropy [R,4] (per key), log_prob_dim / entropy_dim [R,12],
    exempt [R,12], exempt_key [R,4], zmax [R,12] (max |z| of the segment), zmax_key [R,4] (summed over the key's dimensions)."""
    z = scaled(x, T)
    out = {"keep": [], "pi": []}
    cols = {n: [] for n in ("bins", "lp", "ent", "exempt", "zmax")}
    for d, zs in enumerate(ref.segments(z)):
        keep, pi, bins, lp, ent, exempt = _segment(zs, k, p, None if u is None else u[:, d], None if given is None else given[:, d])
        out["keep"].append(keep)
        out["pi"].append(pi)
        for n, v in (("bins", bins), ("lp", lp), ("ent", ent), ("exempt", exempt), ("zmax", np.abs(zs.astype(np.float64)).max(axis=1))):
            cols[n].append(v)
    c = {n: np.stack(v, axis=1) for n, v in cols.items()}
    out.update(bins=c["bins"], log_prob_dim=c["lp"], entropy_dim=c["ent"], exempt=c["exempt"], zmax=c["zmax"],
               log_prob=per_key(c["lp"]), entropy=per_key(c["ent"]), exempt_key=per_key(c["exempt"], np.any), zmax_key=per_key(c["zmax"]))
    return out


@functools.lru_cache(maxsize=None)
def combination(kind, scale, tname, k, p):
    """the reference of one of the 192 combinations, sampled with uniforms(); computed once and shared"""
    return reference(logits(kind, scale), uniforms(), temperature(tname), k, p)


def stat_bound(want, zmax):
    return STAT_GATE * np.maximum(1.0, np.maximum(np.abs(np.where(np.isfinite(want), want, 0.0)), zmax))


def emulate32(x, T, k, p):
    """The kernel's arithmetic in fp32 numpy (exp, sums, division, log in float32; the summation ORDER differs from the wave
    reductions) -> per-dimension log pi of the mode [R,12], entropy [R,12], keep (12 arrays). It shares `ranks` and the logic of
    `kept_set` with the fp64 reference: it is independent of it in the float arithmetic only; the rank logic itself is checked
    against `kept_set_by_sorting` (on tie-free inputs) and, with ties, by the kernel's own compare loop on the GPU."""
    z = scaled(x, T)
    lps, ents, keeps = [], [], []
    for zs in ref.segments(z):
        keep, _ = kept_set(zs, k, p, dtype=np.float32)
        m = zs.max(axis=1, keepdims=True)
        e = np.where(keep, np.exp(zs - m, dtype=np.float32), np.float32(0))
        s = e.sum(axis=1, keepdims=True, dtype=np.float32)
        lse = (m + np.log(s, dtype=np.float32)).astype(np.float32)
        pr = (e / s).astype(np.float32)
        pl = np.where(keep & (pr > 0), pr * (zs - lse), np.float32(0)).astype(np.float32)
        ents.append(-pl.sum(axis=1, dtype=np.float32))
        lps.append((m - lse)[:, 0])
        keeps.append(keep)
    return np.stack(lps, axis=1), np.stack(ents, axis=1), keeps
