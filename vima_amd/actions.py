"""Action selection on the device: from the 700 raw logits of the action head to discrete bins, the continuous action the
environment takes, log-probability and entropy -- `vima_action_select` of include/vima_hip.h, one launch of `act_select_kernel`
(vima_amd/csrc/action_select.hip), no host synchronisation and no torch arithmetic.

    sel = select_actions(policy.action_logits(predicted))            # the mode of every dimension
    sel = select_actions(logits, uniforms=torch.rand(R, 12, device=dev), action_bounds=meta["action_bounds"])

`VIMAPolicy.act` is the same selection fused behind the action head, followed by the action embedding (`vima_act`).

Sampling controls (`vima_action_select_ex` / `vima_act_ex`, `act_sample_kernel` of vima_amd/csrc/action_sample.hip): a temperature,
top-k / top-p truncation, several candidates per state, and `score_actions` / `VIMAPolicy.evaluate_actions` for the
log-probability of actions the caller already has.

    sel = select_actions(logits, uniforms=torch.rand(R, 8, 12, device=dev), temperature=0.7, top_k=10, top_p=0.9, n_samples=8)
    lp = score_actions(logits, sel_single.actions, temperature=0.7).log_prob
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

ACTION_KEYS = ("pose0_position", "pose0_rotation", "pose1_position", "pose1_rotation")
KEY_DIMS = (2, 4, 2, 4)
KEY_FIRST = (0, 2, 6, 8)
N_DIMS = 12
N_LOGITS = 700


class ActionSelection(NamedTuple):
    """Result of `select_actions` / `VIMAPolicy.act`; every entry keeps the leading dims of the input.
    actions {key: int64 [..., 2|4]} discrete bins (the argument of `forward_action_token`); continuous {key: float32 [..., 2|4]}
    bin / n_bins, rescaled and clamped to the action bounds when they were given; log_prob / entropy {key: float32 [...]};
    action_token float32 [..., E] and logits float32 [..., 700] are filled by `VIMAPolicy.act` only (None otherwise)."""
    actions: dict
    continuous: dict
    log_prob: dict
    entropy: dict
    action_token: torch.Tensor | None = None
    logits: torch.Tensor | None = None


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def bounds_array(action_bounds):
    """{"low": [2], "high": [2]} (meta["action_bounds"]) or a (low, high) pair -> ctypes float[4] {low0, low1, high0, high1},
    or None."""
    if action_bounds is None:
        return None
    low, high = (action_bounds["low"], action_bounds["high"]) if isinstance(action_bounds, dict) else action_bounds
    low = np.asarray(torch.as_tensor(low).detach().cpu().numpy() if torch.is_tensor(low) else low, dtype=np.float32).reshape(-1)
    high = np.asarray(torch.as_tensor(high).detach().cpu().numpy() if torch.is_tensor(high) else high, dtype=np.float32).reshape(-1)
    if low.shape != (2,) or high.shape != (2,):
        raise ValueError(f"action bounds must have 2 values each (x, y of the position keys), got {low.shape} / {high.shape}")
    return (ctypes.c_float * 4)(float(low[0]), float(low[1]), float(high[0]), float(high[1]))


def alloc_outputs(R: int, device):
    """The output buffers of one selection over R rows: (idx: 4 int64 tensors, cont [R,12], log_prob [R,4], entropy [R,4])."""
    idx = [torch.empty(R, w, dtype=torch.int64, device=device) for w in KEY_DIMS]
    cont = torch.empty(R, N_DIMS, dtype=torch.float32, device=device)
    logp = torch.empty(R, 4, dtype=torch.float32, device=device)
    ent = torch.empty(R, 4, dtype=torch.float32, device=device)
    return idx, cont, logp, ent


def uniforms_arg(uniforms, R: int, device):
    if uniforms is None:
        return None
    u = uniforms.to(device=device, dtype=torch.float32).reshape(-1, N_DIMS)
    if u.shape[0] != R:
        raise ValueError(f"uniforms must hold 12 values per row of logits ({R} rows), got {tuple(uniforms.shape)}")
    return u.contiguous()


def package(lead, idx, cont, logp, ent, action_token=None, logits=None) -> ActionSelection:
    actions = {k: idx[i].view(*lead, KEY_DIMS[i]) for i, k in enumerate(ACTION_KEYS)}
    continuous = {k: cont[:, KEY_FIRST[i]:KEY_FIRST[i] + KEY_DIMS[i]].reshape(*lead, KEY_DIMS[i]) for i, k in enumerate(ACTION_KEYS)}
    log_prob = {k: logp[:, i].reshape(*lead) for i, k in enumerate(ACTION_KEYS)}
    entropy = {k: ent[:, i].reshape(*lead) for i, k in enumerate(ACTION_KEYS)}
    return ActionSelection(actions, continuous, log_prob, entropy, action_token, logits)


def sample_opts(temperature, top_k, top_p, n_samples, lead, device, given=False):
    """The sampling controls of `select_actions` / `VIMAPolicy.act` as (VimaSampleOpts, temperature tensor to keep alive), or
    (None, None) when every one is at its default. `temperature`: a Python float or a tensor broadcastable to the leading dims
    `lead` of the logits, materialised as a device float32 [R]."""
    if temperature is None and top_k <= 0 and top_p >= 1.0 and n_samples == 1 and not given:
        return None, None
    temp = None
    if temperature is not None:
        temp = torch.as_tensor(temperature, dtype=torch.float32, device=device)
        temp = torch.broadcast_to(temp, tuple(lead)).reshape(-1).contiguous()
    opts = _lib.VimaSampleOpts(temp.data_ptr() if temp is not None else None, int(top_k), float(top_p), int(n_samples), int(bool(given)))
    return opts, temp


def _logits_arg(logits, who):
    if not logits.is_cuda:
        raise RuntimeError(f"{who} needs logits on the GPU: the HIP library has no CPU fallback")
    if logits.shape[-1] != N_LOGITS:
        raise AssertionError(f"expected [..., {N_LOGITS}] logits, got {tuple(logits.shape)}")
    return logits.shape[:-1], logits.to(dtype=torch.float32).reshape(-1, N_LOGITS).contiguous()


def given_bins(actions, device):
    """{key: integer bins [..., 2|4]} -> (leading dims, four contiguous int64 [R, 2|4] tensors on `device`)"""
    if set(actions.keys()) != set(ACTION_KEYS):
        raise AssertionError(f"expected action keys {ACTION_KEYS}, got {sorted(actions.keys())}")
    lead = actions[ACTION_KEYS[0]].shape[:-1]
    idx = [actions[k].to(device=device, dtype=torch.int64).reshape(-1, w).contiguous() for k, w in zip(ACTION_KEYS, KEY_DIMS)]
    if any(t.shape[0] != idx[0].shape[0] for t in idx):
        raise ValueError("the four action keys must share their leading dims")
    return lead, idx


def select_actions(logits: torch.Tensor, uniforms: torch.Tensor | None = None, action_bounds=None, *, temperature=None,
                   top_k: int = 0, top_p: float = 1.0, n_samples: int = 1) -> ActionSelection:
    """logits float32 [..., 700] on the GPU -> ActionSelection. `uniforms` [..., 12] in [0, 1) selects inverse-CDF sampling
    (None: the mode, torch.argmax of every segment); `action_bounds` rescales the continuous action like the reference loop.
    Sampling controls (`vima_action_select_ex`, one launch of `act_sample_kernel`; all defaults: `vima_action_select` as before):
    `temperature` (float or tensor broadcastable to the leading dims) divides the logits, `top_k` / `top_p` truncate every
    segment (top-p after top-k) and log_prob / entropy describe the truncated distribution; `n_samples` = S > 1 draws S candidates
    per row: every output gains a sample axis after the leading dims and `uniforms` is [..., S, 12]."""
    lead, x = _logits_arg(logits, "select_actions")
    lib = _lib.load()
    R = x.shape[0]
    opts, temp = sample_opts(temperature, top_k, top_p, n_samples, lead, x.device)
    S = int(n_samples) if opts is not None else 1
    u = uniforms_arg(uniforms, R * max(S, 1), x.device)
    idx, cont, logp, ent = alloc_outputs(R * max(S, 1), x.device)
    arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in idx])
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    if opts is None:
        _lib.check(lib.vima_action_select(_ptr(x), R, _ptr(u), bounds_array(action_bounds), arr, _ptr(cont), _ptr(logp), _ptr(ent), stream))
        return package(lead, idx, cont, logp, ent)
    _lib.check(lib.vima_action_select_ex(_ptr(x), R, _ptr(u), ctypes.byref(opts), bounds_array(action_bounds), arr, _ptr(cont), _ptr(logp),
                                         _ptr(ent), stream))
    return package((*lead, S) if S > 1 else lead, idx, cont, logp, ent)


def score_actions(logits: torch.Tensor, actions, *, temperature=None, top_k: int = 0, top_p: float = 1.0,
                  action_bounds=None) -> ActionSelection:
    """Log-probability of bins the caller already has: logits float32 [..., 700] on the GPU, `actions` {key: integer bins [..., 2|4]}
    (clamped to [0, n)) -> ActionSelection whose `actions` are the given ones, with `log_prob` (-inf for a bin the filters removed),
    `entropy` and `continuous` of the distribution `select_actions` samples from under the same controls. With the defaults this is
    MultiCategorical.log_prob(actions) / .entropy() of the raw head."""
    lead, x = _logits_arg(logits, "score_actions")
    lib = _lib.load()
    R = x.shape[0]
    alead, idx = given_bins(actions, x.device)
    if idx[0].shape[0] != R:
        raise ValueError(f"actions must hold one row per row of logits ({R} rows), got leading dims {tuple(alead)}")
    opts, temp = sample_opts(temperature, top_k, top_p, 1, lead, x.device, given=True)
    _, cont, logp, ent = alloc_outputs(R, x.device)
    arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in idx])
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(lib.vima_action_select_ex(_ptr(x), R, None, ctypes.byref(opts), bounds_array(action_bounds), arr, _ptr(cont), _ptr(logp),
                                         _ptr(ent), stream))
    return package(lead, idx, cont, logp, ent)
