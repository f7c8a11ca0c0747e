"""Action selection on the device: from the 700 raw logits of the action head to discrete bins, the continuous action the
environment takes, log-probability and entropy -- `vima_action_select` of include/vima_hip.h, one launch of `act_select_kernel`
(vima_amd/csrc/action_select.hip), no host synchronisation and no torch arithmetic.

    sel = select_actions(policy.action_logits(predicted))            # the mode of every dimension
    sel = select_actions(logits, uniforms=torch.rand(R, 12, device=dev), action_bounds=meta["action_bounds"])

`VIMAPolicy.act` is the same selection fused behind the action head, followed by the action embedding (`vima_act`).
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


def select_actions(logits: torch.Tensor, uniforms: torch.Tensor | None = None, action_bounds=None) -> ActionSelection:
    """logits float32 [..., 700] on the GPU -> ActionSelection. `uniforms` [..., 12] in [0, 1) selects inverse-CDF sampling
    (None: the mode, torch.argmax of every segment); `action_bounds` rescales the continuous action like the reference loop."""
    if not logits.is_cuda:
        raise RuntimeError("select_actions needs logits on the GPU: the HIP library has no CPU fallback")
    if logits.shape[-1] != N_LOGITS:
        raise AssertionError(f"expected [..., {N_LOGITS}] logits, got {tuple(logits.shape)}")
    lib = _lib.load()
    lead = logits.shape[:-1]
    x = logits.to(dtype=torch.float32).reshape(-1, N_LOGITS).contiguous()
    R = x.shape[0]
    u = uniforms_arg(uniforms, R, x.device)
    idx, cont, logp, ent = alloc_outputs(R, x.device)
    arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in idx])
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(lib.vima_action_select(_ptr(x), R, _ptr(u), bounds_array(action_bounds), arr, _ptr(cont), _ptr(logp), _ptr(ent), stream))
    return package(lead, idx, cont, logp, ent)
