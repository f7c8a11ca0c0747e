"""Episode snapshots: a sample's decoder state saved as bytes and restored later -- into another slot, at a later step of the ring, into a policy
of another batch size, or after a trip through the host (`VIMAPolicy.snapshot_samples` / `restore_samples`, `seq_snapshot` / `seq_restore` of the
decoder-only policies; C: vima_decode_snapshot / vima_decode_restore and the vima_seq_* pair; payload format in include/vima_hip.h).

An `EpisodeSnapshot` is the payload (a uint8 tensor: the episode's K | V rows of every layer in compact time order, their key-mask bytes, the
position counter and the fresh flag, optionally the prompt K / V block) plus a few ints that describe it, plus -- for the XAttnGPT policies -- the
sample's `prompt_token` column and `prompt_token_mask` row, which the policy's `forward_step` takes from the caller on every step."""
from __future__ import annotations

import ctypes

import torch

from . import _lib

_INFO_FIELDS = tuple(n for n, _ in _lib.VimaEpisodeSnapshotInfo._fields_)


class EpisodeSnapshot:
    def __init__(self, payload: torch.Tensor, info: dict, prompt_token: torch.Tensor | None = None, prompt_token_mask: torch.Tensor | None = None):
        if payload.dtype != torch.uint8 or payload.dim() != 1 or payload.numel() != int(info["bytes"]):
            raise ValueError(f"the payload must be a uint8 tensor of {int(info['bytes'])} bytes, got {payload.dtype} {tuple(payload.shape)}")
        self.payload = payload
        self.info = {k: int(info[k]) for k in _INFO_FIELDS}
        self.prompt_token = prompt_token              # [Lp, E]: the sample's column of the caller's prompt tokens (XAttnGPT policies with the prompt)
        self.prompt_token_mask = prompt_token_mask    # [Lp]

    # ------------------------------------------------------------------ description
    @property
    def steps(self) -> int:
        """env steps the episode had taken when the snapshot was made"""
        return self.info["steps"]

    @property
    def nbytes(self) -> int:
        return self.info["bytes"]

    @property
    def has_prompt(self) -> bool:
        return bool(self.info["flags"] & _lib.SNAPSHOT_PROMPT)

    @property
    def device(self) -> torch.device:
        return self.payload.device

    def __repr__(self):
        return (f"EpisodeSnapshot(steps={self.steps}, nbytes={self.nbytes}, has_prompt={self.has_prompt}, device={self.payload.device}, "
                f"Q={self.info['Q']}, embed_dim={self.info['embed_dim']}, layers={self.info['layers']}, prompt_len={self.info['prompt_len']})")

    # ------------------------------------------------------------------ moving
    def to(self, device) -> "EpisodeSnapshot":
        if torch.device(device) == self.payload.device:
            return self
        mv = lambda t: None if t is None else t.to(device)   # noqa: E731
        return EpisodeSnapshot(self.payload.to(device), self.info, mv(self.prompt_token), mv(self.prompt_token_mask))

    def cpu(self) -> "EpisodeSnapshot":
        return self.to("cpu")

    def state_dict(self) -> dict:
        """tensors and ints only: `torch.save(snapshot.state_dict(), f)` works, `EpisodeSnapshot.from_state_dict(torch.load(f))` reads it back"""
        sd = dict(self.info)
        sd["payload"] = self.payload
        if self.prompt_token is not None:
            sd["prompt_token"], sd["prompt_token_mask"] = self.prompt_token, self.prompt_token_mask
        return sd

    @classmethod
    def from_state_dict(cls, sd: dict) -> "EpisodeSnapshot":
        missing = [k for k in _INFO_FIELDS + ("payload",) if k not in sd]
        if missing:
            raise KeyError(f"not an EpisodeSnapshot state dict: missing {missing}")
        return cls(sd["payload"], sd, sd.get("prompt_token"), sd.get("prompt_token_mask"))

    def _c_info(self) -> _lib.VimaEpisodeSnapshotInfo:
        return _lib.VimaEpisodeSnapshotInfo(*[self.info[k] for k in _INFO_FIELDS])


def _i32(xs):
    return (ctypes.c_int32 * max(len(xs), 1))(*[int(x) for x in xs])


def _index_list(xs, what):
    if isinstance(xs, torch.Tensor):
        xs = xs.reshape(-1).tolist()
    xs = [int(x) for x in ([xs] if isinstance(xs, int) else xs)]
    if not xs:
        raise AssertionError(f"{what}: at least one sample")
    return xs


def take(policy, seq: bool, samples, with_prompt: bool) -> list[EpisodeSnapshot]:
    """vima_(seq_)decode_snapshot_size, one uint8 device tensor per sample, vima_(seq_)decode_snapshot"""
    lib, name = policy._lib, "vima_seq_decode_snapshot" if seq else "vima_decode_snapshot"
    samples = _index_list(samples, name)
    n = len(samples)
    infos = (_lib.VimaEpisodeSnapshotInfo * n)()
    _lib.check(getattr(lib, name + "_size")(policy._handle, _i32(samples), n, int(bool(with_prompt)), ctypes.cast(infos, ctypes.c_void_p)))
    bufs = [torch.empty(int(i.bytes), dtype=torch.uint8, device=policy._device) for i in infos]
    ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
    caps = (ctypes.c_int64 * n)(*[b.numel() for b in bufs])
    _lib.check(getattr(lib, name)(policy._handle, _i32(samples), n, int(bool(with_prompt)), ctypes.cast(ptrs, ctypes.c_void_p),
                                  ctypes.cast(caps, ctypes.c_void_p), ctypes.cast(infos, ctypes.c_void_p), policy._stream()))
    return [EpisodeSnapshot(b, {k: getattr(i, k) for k in _INFO_FIELDS}) for b, i in zip(bufs, infos)]


def put(policy, seq: bool, slots, snapshots) -> tuple[list[int], list[EpisodeSnapshot]]:
    """vima_(seq_)decode_restore of snapshots[i] into slot slots[i]; CPU snapshots are moved to the policy's device first. -> (slots, device snapshots)"""
    name = "vima_seq_decode_restore" if seq else "vima_decode_restore"
    slots = _index_list(slots, name)
    if isinstance(snapshots, EpisodeSnapshot):
        snapshots = [snapshots]
    snapshots = list(snapshots)
    if len(snapshots) != len(slots):
        raise AssertionError(f"{name}: {len(slots)} slots but {len(snapshots)} snapshots")
    n = len(slots)
    dev = [s.to(policy._device) for s in snapshots]
    for s in dev:
        if not s.payload.is_contiguous():
            raise AssertionError(f"{name}: a snapshot's payload must be contiguous")
    ptrs = (ctypes.c_void_p * n)(*[s.payload.data_ptr() for s in dev])
    infos = (_lib.VimaEpisodeSnapshotInfo * n)(*[s._c_info() for s in dev])
    _lib.check(getattr(policy._lib, name)(policy._handle, _i32(slots), n, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(infos, ctypes.c_void_p),
                                          policy._stream()))
    return slots, dev
