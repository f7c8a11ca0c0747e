"""Host-side mirrors of the reference's BASELINE policies, backed by the same gfx950 HIP library:

    VIMAGPTPolicy        vima/policy/vima_gpt_policy.py       (decoder-only HFGPT, one token per frame pair)
    VIMAGatoPolicy       vima/policy/vima_gato_policy.py      (decoder-only HFGPT, 16 patch tokens per frame pair)
    VIMAFlamingoPolicy   vima/policy/vima_flamingo_policy.py  (Perceiver-resampled tokens + XAttnGPT)

Same constructor arguments, method surface, return shapes and state_dict keys as the reference classes; the arithmetic runs
in the HIP kernels (`vima_rgb_obs_encode`, `vima_rgb_prompt_encode`, `vima_seq_decode` / `vima_decode`, `vima_action_*`;
rollouts: `vima_seq_prefill` / `vima_seq_decode_step` for gpt / gato, `vima_decode_step` for flamingo).
No CPU fallback. Unlike VIMAPolicy these consume whole RGB frames `{"rgb": {view: u8 [..., 3, 64, 128]}}` and have no
object masks (`forward` takes no `obs_mask`)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .policy import VIMAPolicy, VIEWS, build_prompt_index, _ptr, _pair

RGB_SHAPE = (3, 64, 128)     # img_size=(64, 128) (vima_gpt_policy.py:37-45)


class _BaselinePolicy(VIMAPolicy):
    KIND = None

    def __init__(self, *, embed_dim, n_layer, n_head, xattn_n_heads=None, vocab_size=40478, n_positions=512,
                 precision="bf16", device=None):
        if precision in ("fp8w", "fp8"):
            raise ValueError(f"precision '{precision}' is validated for VIMAPolicy only; the baseline policies run in 'bf16', 'fp32' or 'bf16x3'")
        super().__init__(embed_dim=embed_dim, xf_n_layers=n_layer, sattn_n_heads=n_head,
                         xattn_n_heads=xattn_n_heads or n_head, xattn_n_positions=256, n_positions=n_positions,
                         precision=precision, device=device)
        self._cfg.policy_kind = _lib.POLICY_KIND[self.KIND]
        self._vocab_size = vocab_size
        self._obj_xf_num_queries = int(self._lib.vima_rgb_tokens_per_image(ctypes.byref(self._cfg)))
        self.cache_prompt_kv = self.KIND == "flamingo"

    # ------------------------------------------------------------------ weights
    def expected_keys(self):
        req = _lib.required_params(self._cfg)
        n = self._cfg.xf_n_layers
        ign = ["t5_prompt_encoder.t5.shared.weight", "t5_prompt_encoder.t5.encoder.embed_tokens.weight"]
        if self.KIND == "flamingo":
            ign += ["xattn_gpt.position_ids", "xattn_gpt.xattn_position_ids"]
            ign += [f"xattn_gpt.h.{i}.attn.bias" for i in range(n)]
            ign += [f"xattn_gpt.xattns.{i}.kv_position_ids" for i in range(n)]
        else:   # tokens_embed is never read: the policies feed inputs_embeds (gpt/gpt.py:69-73)
            ign += ["transformer.lm.position_ids", "transformer.lm.tokens_embed.weight"]
        return req, ign

    # ------------------------------------------------------------------ frames
    def _rgb_inputs(self, rgb, lead_dims):
        frames = [f.reshape(-1, *f.shape[lead_dims:]) for f in self._views_of(rgb, "rgb")]
        n = frames[0].shape[0]
        for f in frames:
            if tuple(f.shape) != (n, *RGB_SHAPE):
                raise ValueError(f"rgb must be [..., 3, 64, 128] for every view, got {tuple(f.shape)}")
        self._check_img(frames)
        return [f.to(device=self._device, dtype=torch.uint8).contiguous() for f in frames], n

    def obj_encoder(self, rgb):
        """obj_encoder.forward for ONE leading dim: gpt [n, 2E]; gato [n, 16, E]; flamingo [n, 4, E] (obj_encoder.py:123-240)."""
        self._ready()
        frames, n = self._rgb_inputs(rgb, 1)
        Q, E = self._obj_xf_num_queries, self.embed_dim
        Eo = 2 * E if self.KIND == "gpt" else E
        out = torch.empty(n, Q, Eo, dtype=torch.float32, device=self._device)
        _lib.check(self._lib.vima_rgb_encode(self._handle, _pair(frames[0].data_ptr(), frames[1].data_ptr()), n, _ptr(out),
                                             self._stream()))
        return out.view(n, Eo) if self.KIND == "gpt" else out

    def forward_obs_token(self, obs):
        """obs = {"rgb": {view: u8 [L_obs, B, 3, 64, 128]}, "ee": [L_obs, B] int64} -> [L_obs, B, E] (gpt) or
        [L_obs, B, Q, E] (gato / flamingo)   (vima_gpt_policy.py:249-259, vima_gato_policy.py:253-264)"""
        self._ready()
        rgb, ee = obs["rgb"], obs["ee"]
        lead = tuple(ee.shape[:2])
        frames, n = self._rgb_inputs(rgb, 2)
        assert n == lead[0] * lead[1]
        ee = ee.to(device=self._device, dtype=torch.int64).contiguous()
        Q, E = self._obj_xf_num_queries, self.embed_dim
        out = torch.empty(n, Q, E, dtype=torch.float32, device=self._device)
        _lib.check(self._lib.vima_rgb_obs_encode(self._handle, _pair(frames[0].data_ptr(), frames[1].data_ptr()), _ptr(ee), n,
                                                 _ptr(out), self._stream()))
        return out.view(*lead, E) if self.KIND == "gpt" else out.view(*lead, Q, E)

    def forward_prompt_assembly(self, prompts):
        """(raw_prompts_token_type, word_batch, {"rgb": {view: u8 [n_img, 3, 64, 128]}}) -> (prompt_tokens [L, B, E],
        prompt_masks [B, L]); every image contributes `_obj_xf_num_queries` tokens (vima_gato_policy.py:190-251)."""
        self._ready()
        raw_types, word_batch, image_batch = prompts
        n_img_total = sum(1 for p in raw_types for t in p if t == 1)
        dev = self._device
        frames, n_img = (self._rgb_inputs(image_batch["rgb"], 1) if n_img_total > 0 else (None, 0))
        Q = self._obj_xf_num_queries
        B = len(raw_types)
        src, L_max, wp, ip = build_prompt_index(raw_types, Q)
        if wp > word_batch.numel() or ip > n_img:
            raise IndexError("prompt token types reference more words / images than provided")
        word_batch = word_batch.to(device=dev, dtype=torch.int64).contiguous()
        tok_src = torch.from_numpy(src[:, :L_max].copy()).to(dev)
        out = torch.empty(B, L_max, self.embed_dim, dtype=torch.float32, device=dev)
        omask = torch.empty(B, L_max, dtype=torch.bool, device=dev)
        _lib.check(self._lib.vima_rgb_prompt_encode(
            self._handle, _ptr(word_batch), int(word_batch.numel()),
            _pair(frames[0].data_ptr(), frames[1].data_ptr()) if frames else _pair(0, 0), n_img, _ptr(tok_src), B, L_max,
            _ptr(out), _ptr(omask), self._stream()))
        return out.transpose(0, 1), omask

    # ------------------------------------------------------------------ decoder
    def forward(self, obs_token, action_token, prompt_token, prompt_token_mask):
        """-> predicted_action_tokens [L_obs, B, E] (vima_gpt_policy.py:118-187, vima_gato_policy.py:115-188,
        vima_flamingo_policy.py:121-154). Note the baseline signature: no obs_mask."""
        self._ready()
        if obs_token.dim() == 3:
            obs_token = obs_token.unsqueeze(2)
        L_obs, B, Q, E = obs_token.shape
        if Q != self._obj_xf_num_queries:
            raise AssertionError(f"obs_token must carry {self._obj_xf_num_queries} tokens per step, got {Q}")
        if obs_token.dtype != torch.float32 or prompt_token.dtype != torch.float32:
            raise AssertionError(f"obs_token / prompt_token must be float32, got {obs_token.dtype} / {prompt_token.dtype}")
        if prompt_token.dim() != 3 or prompt_token.shape[1] != B or prompt_token.shape[2] != E:
            raise AssertionError(f"prompt_token must be [Lp, {B}, {E}], got {tuple(prompt_token.shape)}")
        if tuple(prompt_token_mask.shape) != (B, prompt_token.shape[0]):
            raise AssertionError("prompt_token_mask shape does not match the prompt tokens")
        if self.KIND == "flamingo":
            ones = torch.ones(L_obs, B, Q, dtype=torch.bool, device=self._device)
            return VIMAPolicy.forward(self, obs_token, ones, action_token, prompt_token, prompt_token_mask)
        dev = self._device
        obs_token = obs_token.to(device=dev, dtype=torch.float32).contiguous()
        L_act = 0
        if action_token is not None:
            L_act = action_token.shape[0]
            action_token = action_token.to(device=dev, dtype=torch.float32).contiguous()
        if prompt_token.stride(-1) != 1:
            prompt_token = prompt_token.contiguous()
        prompt_token = prompt_token.to(device=dev, dtype=torch.float32)
        prompt_token_mask = prompt_token_mask.to(device=dev, dtype=torch.bool).contiguous()
        Lp = prompt_token.shape[0]
        # the reference builds the position ids on the host from the per-sample number of valid prompt tokens
        # (vima_gato_policy.py:156-184, one `.item()` per sample); a sample without any valid prompt token gets the id -1 there and the
        # embedding lookup raises. The C entry point is asynchronous and clamps instead, so the same refusal happens here.
        if not bool(prompt_token_mask.any(dim=1).all()):
            raise IndexError("index out of range in self (a sample has no valid prompt token: position id -1, vima_gato_policy.py:164)")
        out = torch.empty(L_obs, B, E, dtype=torch.float32, device=dev)
        _lib.check(self._lib.vima_seq_decode(
            self._handle, _ptr(obs_token), _ptr(action_token), L_obs, B, L_act, _ptr(prompt_token), prompt_token.stride(1),
            prompt_token.stride(0), _ptr(prompt_token_mask), Lp, _ptr(out), self._stream()))
        return out

    def forward_step(self, obs_token, prev_action_token, prompt_token, prompt_token_mask, step: int):
        """Incremental decoding of one env step (see VIMAPolicy.forward_step). VIMAFlamingoPolicy decodes with XAttnGPT, so the
        episode caches of `vima_decode_step` apply unchanged (every token valid). The decoder-only policies step with
        `seq_prefill` / `seq_step`: their prompt is a sequence prefix consumed once, not an operand passed every step."""
        if self.KIND != "flamingo":
            raise NotImplementedError("forward_step needs the XAttnGPT episode caches (VIMAPolicy / VIMAFlamingoPolicy); the decoder-only "
                                      "policies decode incrementally with seq_prefill / seq_step")
        if obs_token.dim() == 4:
            obs_token = obs_token[-1]
        ones = torch.ones(obs_token.shape[:2], dtype=torch.bool, device=self._device)
        return VIMAPolicy.forward_step(self, obs_token, ones, prev_action_token, prompt_token, prompt_token_mask, step)

    def forward_steps(self, obs_token, action_token, prompt_token, prompt_token_mask, step: int):
        """T env steps as one pass (see VIMAPolicy.forward_steps): obs_token [T,B,Q,E], every token valid. VIMAFlamingoPolicy only; the
        decoder-only policies fill their cache with `seq_prefill` and step with `seq_step`."""
        if self.KIND != "flamingo":
            raise NotImplementedError("forward_steps needs the XAttnGPT episode caches (VIMAPolicy / VIMAFlamingoPolicy); the decoder-only "
                                      "policies take T env steps in one pass with seq_steps (after seq_prefill)")
        ones = torch.ones(obs_token.shape[:3], dtype=torch.bool, device=self._device)
        return VIMAPolicy.forward_steps(self, obs_token, ones, action_token, prompt_token, prompt_token_mask, step)

    def restart_samples(self, restart, prompt_token, prompt_token_mask, history=None):
        """VIMAPolicy.restart_samples; `history` = (obs_token [T,n_r,Q,E], action_token [T-1,n_r,E] | None) -- every token valid -- or the
        three-tuple of VIMAPolicy with its mask. VIMAFlamingoPolicy only; the decoder-only policies restart with `seq_restart` (which takes `history=` too)."""
        if history is None:
            return VIMAPolicy.restart_samples(self, restart, prompt_token, prompt_token_mask)
        if self.KIND != "flamingo":
            raise NotImplementedError("restart_samples(history=) needs the XAttnGPT episode caches (VIMAPolicy / VIMAFlamingoPolicy); the "
                                      "decoder-only policies install a history with seq_restart(history=)")
        if len(history) == 2:
            history = (history[0], torch.ones(history[0].shape[:3], dtype=torch.bool, device=self._device), history[1])
        return VIMAPolicy.restart_samples(self, restart, prompt_token, prompt_token_mask, history)

    def fork_samples(self, source, prompt_token, prompt_token_mask):
        """VIMAPolicy.fork_samples. VIMAFlamingoPolicy only; the decoder-only policies fork with `seq_fork` (their prompt is the cache prefix)."""
        if self.KIND != "flamingo":
            raise NotImplementedError("fork_samples needs the XAttnGPT episode caches (VIMAPolicy / VIMAFlamingoPolicy); the decoder-only "
                                      "policies fork with seq_fork")
        return VIMAPolicy.fork_samples(self, source, prompt_token, prompt_token_mask)

    def snapshot_samples(self, samples, prompt_token, prompt_token_mask, with_prompt=True):
        """VIMAPolicy.snapshot_samples. VIMAFlamingoPolicy only; the decoder-only policies snapshot with `seq_snapshot` (their prompt is the cache prefix)."""
        if self.KIND != "flamingo":
            raise NotImplementedError("snapshot_samples needs the XAttnGPT episode caches (VIMAPolicy / VIMAFlamingoPolicy); the decoder-only "
                                      "policies snapshot with seq_snapshot")
        return VIMAPolicy.snapshot_samples(self, samples, prompt_token, prompt_token_mask, with_prompt)

    def restore_samples(self, slots, snapshots, prompt_token, prompt_token_mask):
        """VIMAPolicy.restore_samples. VIMAFlamingoPolicy only; the decoder-only policies restore with `seq_restore`."""
        if self.KIND != "flamingo":
            raise NotImplementedError("restore_samples needs the XAttnGPT episode caches (VIMAPolicy / VIMAFlamingoPolicy); the decoder-only "
                                      "policies restore with seq_restore")
        return VIMAPolicy.restore_samples(self, slots, snapshots, prompt_token, prompt_token_mask)

    def history_room(self) -> int:
        if self.KIND != "flamingo":
            raise NotImplementedError("history_room: VIMAPolicy / VIMAFlamingoPolicy only (the decoder-only policies have seq_history_room)")
        return VIMAPolicy.history_room(self)

    # ------------------------------------------------------------------ incremental decoding (gpt / gato)
    def _seq_only(self, what):
        if self.KIND == "flamingo":
            raise NotImplementedError(f"{what}: decoder-only policies (gpt / gato) only; VIMAFlamingoPolicy steps with forward_step")
        self._ready()

    def _seq_prompt(self, prompt_token, prompt_token_mask):
        E = self.embed_dim
        if prompt_token.dim() != 3 or prompt_token.shape[2] != E or prompt_token.dtype != torch.float32:
            raise AssertionError(f"prompt_token must be float32 [Lp, B, {E}], got {prompt_token.dtype} {tuple(prompt_token.shape)}")
        if tuple(prompt_token_mask.shape) != (prompt_token.shape[1], prompt_token.shape[0]):
            raise AssertionError("prompt_token_mask shape does not match the prompt tokens")
        if prompt_token.stride(-1) != 1:
            prompt_token = prompt_token.contiguous()
        return prompt_token.to(self._device), prompt_token_mask.to(device=self._device, dtype=torch.bool).contiguous()

    def seq_prefill(self, prompt_token, prompt_token_mask):
        """Start an episode batch of incremental decoding (no reference counterpart: its loop re-feeds the whole sequence to `forward`
        every env step): prompt_token [Lp, B, E] + the separator run through the stack ONCE and every layer's K/V stay in the native
        handle. Then call `seq_step` once per env step. A sample without any valid prompt token is refused like in `forward`.
        With `set_option("seq_ring", 1)` the cache rows behind the prompt + separator are a ring (see `seq_restart`); the prefill is then
        needed once per batch, not once per n_positions rows."""
        self._seq_only("seq_prefill")
        prompt_token, prompt_token_mask = self._seq_prompt(prompt_token, prompt_token_mask)
        if not bool(prompt_token_mask.any(dim=1).all()):
            raise IndexError("index out of range in self (a sample has no valid prompt token: position id -1, vima_gato_policy.py:164)")
        Lp, B = prompt_token.shape[0], prompt_token.shape[1]
        _lib.check(self._lib.vima_seq_prefill(self._handle, _ptr(prompt_token), prompt_token.stride(1), prompt_token.stride(0),
                                              _ptr(prompt_token_mask), B, Lp, self._stream()))
        self._seq_t, self._ep_B = 0, B

    def seq_step(self, obs_token, prev_action_token=None):
        """One env step of the episode batch started by `seq_prefill`: obs_token [B, Q, E] ([B, E] or [B, 1, E] for GPT) and, from the
        second step on, the embedded action of the previous step [B, E]. The step number is kept here. Returns the predicted action
        token [B, E] == forward(<full history>)[step]. IndexError when the sequence would exceed n_positions, like `forward`.
        With option `seq_ring` the step number is unbounded; IndexError then names the first sample whose OWN episode would exceed the
        ring (n_positions - Lp - 1 rows, skipped tail rows included), nothing changes, and the step succeeds once that sample has been
        restarted. `steps_left()` tells in advance."""
        self._seq_only("seq_step")
        Q, E = self._obj_xf_num_queries, self.embed_dim
        if obs_token.dim() == 2:
            obs_token = obs_token.unsqueeze(1)
        if obs_token.dim() != 3 or obs_token.shape[1] != Q or obs_token.shape[2] != E or obs_token.dtype != torch.float32:
            raise AssertionError(f"obs_token must be float32 [B, {Q}, {E}], got {obs_token.dtype} {tuple(obs_token.shape)}")
        B = obs_token.shape[0]
        step = getattr(self, "_seq_t", None)
        if step is None:
            raise _lib.VimaError("seq_step: no running episode (call seq_prefill first)")
        obs_token = obs_token.to(device=self._device).contiguous()
        if step > 0:
            if prev_action_token is None:
                raise AssertionError("seq_step: the previous action token is required from the second step on")
            if prev_action_token.dim() == 3:
                prev_action_token = prev_action_token[-1]
            if tuple(prev_action_token.shape) != (B, E) or prev_action_token.dtype != torch.float32:
                raise AssertionError(f"prev_action_token must be float32 [{B}, {E}], got {tuple(prev_action_token.shape)}")
            prev_action_token = prev_action_token.to(device=self._device).contiguous()
        else:
            prev_action_token = None
        out = torch.empty(B, E, dtype=torch.float32, device=self._device)
        _lib.check(self._lib.vima_seq_decode_step(self._handle, _ptr(obs_token), _ptr(prev_action_token), step, B, _ptr(out), self._stream()))
        self._seq_t = step + 1
        return out

    def seq_steps(self, obs_token, action_token=None):
        """T env steps of the episode batch as ONE pass (`vima_seq_decode_chunk`): obs_token [T, B, Q, E] ([T, B, E] for GPT); action_token
        [T, B, E] once the batch has taken a step (row 0 = the action of the step before the chunk), [T-1, B, E] before its first step (None for
        T = 1). Returns [T, B, E], row j == what `seq_step` returns for step j of the chunk (up to summation order; T = 1 IS `seq_step`, bit for
        bit). Resumes a recorded rollout, or scores a recorded prefix teacher-forced before stepping on. IndexError, nothing changed, when the
        chunk does not fit: linear cache "room for N more steps"; with `seq_ring` the chunk is one unit of the ring (never split, it skips the
        tail whole), so it can be refused -- naming the sample -- where single steps still pass."""
        self._seq_only("seq_steps")
        Q, E = self._obj_xf_num_queries, self.embed_dim
        if obs_token.dim() == 3 and Q == 1:
            obs_token = obs_token.unsqueeze(2)
        if obs_token.dim() != 4 or obs_token.shape[2] != Q or obs_token.shape[3] != E or obs_token.dtype != torch.float32:
            raise AssertionError(f"obs_token must be float32 [T, B, {Q}, {E}], got {obs_token.dtype} {tuple(obs_token.shape)}")
        T, B = obs_token.shape[0], obs_token.shape[1]
        if T < 1:
            raise AssertionError("seq_steps: at least one step")
        step = getattr(self, "_seq_t", None)
        if step is None:
            raise _lib.VimaError("seq_steps: no running episode (call seq_prefill first)")
        n_act = T if step > 0 else T - 1
        if n_act > 0:
            if action_token is None:
                raise AssertionError(f"seq_steps: action_token [{n_act}, {B}, {E}] is required (the actions in front of / between the chunk's steps)")
            if tuple(action_token.shape) != (n_act, B, E) or action_token.dtype != torch.float32:
                raise AssertionError(f"action_token must be float32 [{n_act}, {B}, {E}], got {action_token.dtype} {tuple(action_token.shape)}")
            action_token = action_token.to(device=self._device).contiguous()
        else:
            action_token = None
        obs_token = obs_token.to(device=self._device).contiguous()
        out = torch.empty(T, B, E, dtype=torch.float32, device=self._device)
        _lib.check(self._lib.vima_seq_decode_chunk(self._handle, _ptr(obs_token), _ptr(action_token), step, T, B, _ptr(out), self._stream()))
        self._seq_t = step + T
        return out

    def seq_restart(self, restart, prompt_token, prompt_token_mask, history=None):
        """Per-sample episode restart inside the stepping batch: every sample with `restart[b]` true forgets its history, takes its new
        prompt from `prompt_token[:, b]` / `prompt_token_mask[b]` (same [Lp, B, E] / [B, Lp] layout and the same Lp as `seq_prefill`;
        other samples' rows are not read) and its next `seq_step` ignores its row of `prev_action_token`. All flagged samples are
        rebuilt in one batched prefill. The batch keeps stepping with `seq_step`; a restart does not give cache rows back
        (`steps_left`): when they run out, start over with `seq_prefill` -- unless option `seq_ring` is set: the restarted samples' rows
        then return to the ring, a restart takes no rows itself, and a batch whose samples are each restarted before their
        `steps_left()` entry reaches 0 never calls `seq_prefill` again (`decode_ring` is VIMAPolicy's ring and is refused here).
        history = (obs_token [T, n_r, Q, E], action_token [T-1, n_r, E] | None), n_r = the flagged samples in increasing order: the flagged
        samples join the batch MID-episode -- T recorded env steps are installed in the cache rows of the batch's last T steps (one pass over
        [prompt | sep | history]), the teacher-forced predictions [T, n_r, E] are returned, and the next `seq_step` consumes each sample's row
        of `prev_action_token` (the action of history step T - 1). IndexError, nothing changed, when T > `seq_history_room()` or the sequence
        exceeds n_positions. Without `history`: returns None."""
        self._seq_only("seq_restart")
        prompt_token, prompt_token_mask = self._seq_prompt(prompt_token, prompt_token_mask)
        flags = torch.as_tensor(restart).to(dtype=torch.uint8, device="cpu").contiguous()
        Lp, B = prompt_token.shape[0], prompt_token.shape[1]
        if flags.numel() != B:
            raise AssertionError(f"restart must have one flag per sample ({B}), got {flags.numel()}")
        if not bool(prompt_token_mask[flags.bool().to(self._device)].any(dim=1).all()):
            raise IndexError("index out of range in self (a restarted sample has no valid prompt token: position id -1, vima_gato_policy.py:164)")
        if history is None:
            _lib.check(self._lib.vima_seq_decode_restart(self._handle, ctypes.c_void_p(flags.data_ptr()), B, _ptr(prompt_token),
                                                         prompt_token.stride(1), prompt_token.stride(0), _ptr(prompt_token_mask), Lp, self._stream()))
            return None
        Q, E = self._obj_xf_num_queries, self.embed_dim
        obs_token, action_token = history
        if obs_token.dim() == 3 and Q == 1:
            obs_token = obs_token.unsqueeze(2)
        n_r = int(flags.bool().sum())
        if obs_token.dim() != 4 or tuple(obs_token.shape[1:]) != (n_r, Q, E) or obs_token.dtype != torch.float32:
            raise AssertionError(f"history obs_token must be float32 [T, {n_r}, {Q}, {E}] (one column per flagged sample), got {obs_token.dtype} {tuple(obs_token.shape)}")
        T = obs_token.shape[0]
        if T > 1:
            if action_token is None or tuple(action_token.shape) != (T - 1, n_r, E) or action_token.dtype != torch.float32:
                raise AssertionError(f"history action_token must be float32 [{T - 1}, {n_r}, {E}]")
            action_token = action_token.to(device=self._device).contiguous()
        else:
            action_token = None
        obs_token = obs_token.to(device=self._device).contiguous()
        out = torch.empty(T, n_r, E, dtype=torch.float32, device=self._device)
        _lib.check(self._lib.vima_seq_decode_restart_history(
            self._handle, ctypes.c_void_p(flags.data_ptr()), B, _ptr(prompt_token), prompt_token.stride(1), prompt_token.stride(0),
            _ptr(prompt_token_mask), Lp, _ptr(obs_token), _ptr(action_token), T, _ptr(out), self._stream()))
        return out

    def seq_fork(self, source):
        """Branch rollouts inside the stepping batch: slot b continues the episode of slot `source[b]` (length-B ints; `source[b] == b`:
        untouched). Nothing is recomputed (vima_seq_decode_fork): the source's prefix rows [prompt | sep] and the live rows of its history
        in every layer's K/V cache, its key mask, position counter and restart flag are copied into the destination's slot, whose old
        episode is dropped. There are no prompt tensors to update: the prompt is the cache prefix. Every source must be its own source
        (`source[source[b]] == source[b]`: no chains, no swaps); ValueError otherwise, and nothing changes. The destination's next
        `seq_step` consumes or ignores its row of `prev_action_token` exactly as the source's would; fed the source's inputs it returns
        the source's output bit for bit, fed others it is a branch. `steps_left()` of a destination is its source's; a later
        `seq_restart` (with or without `history=`) of a forked slot works as on any other."""
        self._seq_only("seq_fork (VIMAFlamingoPolicy forks with fork_samples)")
        B = getattr(self, "_ep_B", 0)
        if getattr(self, "_seq_t", None) is None or B <= 0:
            raise _lib.VimaError("seq_fork: no running episode (call seq_prefill first)")
        src, src_p = self._fork_source(source, B)
        _lib.check(self._lib.vima_seq_decode_fork(self._handle, src_p, B, self._stream()))

    def seq_snapshot(self, samples):
        """Episode snapshots of the listed samples of the stepping batch -> list[EpisodeSnapshot] (vima_amd/episodes.py;
        vima_seq_decode_snapshot): the sample's prefix rows [prompt | sep] and the rows of its env steps in compact time order, in every
        layer's K/V cache, their key mask, position counter and restart flag -- wherever the ring holds the rows now. Nothing is recomputed,
        the batch is not touched, there are no prompt tensors to carry: the prompt is the cache prefix. One upload and 2 launches whatever
        the number of samples and layers. Snapshots live on the device; `.cpu()` / `.state_dict()` carry them anywhere."""
        self._seq_only("seq_snapshot (VIMAFlamingoPolicy snapshots with snapshot_samples)")
        if getattr(self, "_seq_t", None) is None:
            raise _lib.VimaError("seq_snapshot: no running episode (call seq_prefill first)")
        from . import episodes
        return episodes.take(self, True, samples, True)

    def seq_restore(self, slots, snapshots):
        """Slot `slots[i]` of the stepping batch becomes the episode of `snapshots[i]` (vima_seq_decode_restore): a restart of the slot
        followed by an install of the snapshot's rows in the cache rows the last `snapshot.steps` batch steps wrote -- at any later step, in
        any slot, on any policy of the same kind, embed_dim, layers, precision element size, Q and prompt length (another batch size,
        another ring phase). The slot's next `seq_step` consumes or ignores its row of `prev_action_token` as the snapshot's sample would
        have. `steps_left()` of the slot is that of a sample restarted `snapshot.steps` batch steps ago. One snapshot may go to several
        slots; CPU snapshots are moved to the device here. More steps than `seq_history_room()`: IndexError; a mismatched snapshot or a
        slot listed twice: ValueError; nothing changes in either case."""
        self._seq_only("seq_restore (VIMAFlamingoPolicy restores with restore_samples)")
        if getattr(self, "_seq_t", None) is None:
            raise _lib.VimaError("seq_restore: no running episode (call seq_prefill first)")
        from . import episodes
        episodes.put(self, True, slots, snapshots)

    def seq_history_room(self) -> int:
        """The largest T `seq_restart(..., history=)` accepts now: the most recent batch steps whose cache rows are all still there (without
        `seq_ring`: the steps taken since `seq_prefill`). Host bookkeeping only."""
        self._seq_only("seq_history_room")
        room = ctypes.c_int32(0)
        _lib.check(self._lib.vima_seq_history_room(self._handle, ctypes.byref(room)))
        return int(room.value)

    # steps_left() is VIMAPolicy's: on a gpt / gato handle vima_decode_steps_left reports the episode of seq_prefill / seq_step (all entries
    # equal: how many further seq_step calls fit into n_positions; with option seq_ring per sample: how many more would succeed if that sample
    # alone were never restarted)


class VIMAGPTPolicy(_BaselinePolicy):
    """vima/policy/vima_gpt_policy.py:9-116"""
    KIND = "gpt"

    def __init__(self, *, embed_dim: int, vocab_size=40478, n_positions=512, n_layer=12, n_head=12, dropout: float = 0.1,
                 precision="bf16", device=None):
        super().__init__(embed_dim=embed_dim, n_layer=n_layer, n_head=n_head, vocab_size=vocab_size, n_positions=n_positions,
                         precision=precision, device=device)


class VIMAGatoPolicy(_BaselinePolicy):
    """vima/policy/vima_gato_policy.py:10-113"""
    KIND = "gato"

    def __init__(self, *, embed_dim: int, vocab_size=40478, n_positions=512, n_layer=12, n_head=12, dropout: float = 0.1,
                 precision="bf16", device=None):
        super().__init__(embed_dim=embed_dim, n_layer=n_layer, n_head=n_head, vocab_size=vocab_size, n_positions=n_positions,
                         precision=precision, device=device)


class VIMAFlamingoPolicy(_BaselinePolicy):
    """vima/policy/vima_flamingo_policy.py:9-119"""
    KIND = "flamingo"

    def __init__(self, *, embed_dim: int, dt_n_layers: int, dt_n_heads: int, xattn_n_heads: int, precision="bf16", device=None):
        super().__init__(embed_dim=embed_dim, n_layer=dt_n_layers, n_head=dt_n_heads, xattn_n_heads=xattn_n_heads,
                         precision=precision, device=device)


BASELINES = {"gpt": VIMAGPTPolicy, "gato": VIMAGatoPolicy, "flamingo": VIMAFlamingoPolicy}


def build_baseline(cfg, precision="bf16", device=None):
    """cfg: vima_testing.synthetic.BaselineConfig"""
    kw = cfg.ctor_kwargs()
    return BASELINES[cfg.kind](**kw, precision=precision, device=device)
