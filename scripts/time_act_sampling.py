"""Wall time of the stochastic action step of VIMA-200M in bf16 with its two paths, alternated inside one process on one GPU, at batch
1, 32 and 256:

    host    forward_action_decoder -> logit warping in torch (temperature, top-k, top-p per action dimension, the usual warper
            order) -> MultiCategorical.sample / .log_prob -> forward_action_token (the only way before the sampling controls)
    device  VIMAPolicy.act(..., temperature=, top_k=, top_p=, n_samples=) / VIMAPolicy.evaluate_actions (vima_act_ex: action head,
            act_sample_kernel, action embedding in one native call)

Three workloads: `sample` = one incremental env step (examples/episode_loop.py: forward_obs_token -> forward_step -> action) with
act(sample=True, temperature=0.7, top_k=10, top_p=0.9); `candidates` = the same env step with n_samples=8 (the first candidate is
fed back); `evaluate` = evaluate_actions on a [T = 8, B] block of predicted tokens and given actions (one call, no decoder).
Per workload, path and batch: median, minimum, maximum and interquartile range of the device-synchronised wall time (host clock, a
device synchronise at both ends). Last: the device time of act_sample_kernel next to act_select_kernel on the same rows of logits
(HIP events around back-to-back launches through the C ABI on fixed buffers).

    python scripts/time_act_sampling.py [--batches 1 32 256] [--steps 8] [--repeats 11] [--warmup 2] [--out profiles/act_sampling_time.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vima_testing import synthetic as syn  # noqa: E402
from vima_amd import _lib  # noqa: E402
from vima_amd.actions import alloc_outputs  # noqa: E402
from vima_amd.dists import MultiCategorical  # noqa: E402
from vima_amd.policy import VIMAPolicy, ACTION_KEYS  # noqa: E402

PATHS = ("host", "device")
CONTROLS = dict(temperature=0.7, top_k=10, top_p=0.9)
N_CAND = 8


def warp(dist, temperature, top_k, top_p):
    """the host path's logit warping of one key's MultiCategorical -> a MultiCategorical of the truncated distribution"""
    out = []
    for x in torch.split(dist.raw_logits, list(dist._action_dims), dim=-1):
        z = x / temperature
        if 0 < top_k < z.shape[-1]:
            kth = torch.topk(z, top_k, dim=-1).values[..., -1:]
            z = z.masked_fill(z < kth, float("-inf"))
        if top_p < 1.0:
            zs, order = torch.sort(z, dim=-1, descending=True)
            q = torch.softmax(zs, dim=-1)
            drop = (torch.cumsum(q, dim=-1) - q) >= top_p
            z = z.masked_fill(drop.scatter(-1, order, drop), float("-inf"))
        out.append(z)
    return MultiCategorical(torch.cat(out, dim=-1), dist._action_dims)


def host_step(policy, predicted, n):
    """predicted [..., E] -> (actions of the first sample, its token, log-probabilities); n samples per state"""
    dists = {k: warp(d, **CONTROLS) for k, d in policy.forward_action_decoder(predicted).items()}
    if n == 1:
        actions = {k: d.sample() for k, d in dists.items()}
        logp = {k: dists[k].log_prob(actions[k]) for k in ACTION_KEYS}
        return actions, policy.forward_action_token(actions), logp
    actions = {k: d.sample((n,)).movedim(0, -2) for k, d in dists.items()}          # [..., n, 2|4]
    logp = {k: dists[k].log_prob(actions[k].movedim(-2, 0)).movedim(0, -1) for k in ACTION_KEYS}
    tokens = policy.forward_action_token(actions)
    return {k: v[..., 0, :] for k, v in actions.items()}, tokens[..., 0, :], logp


def episode(policy, path, n, observations, prompt_tokens, prompt_masks):
    prev = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t, obs in enumerate(observations):
        obs_token, obs_mask = policy.forward_obs_token(obs)
        predicted = policy.forward_step(obs_token, obs_mask, prev, prompt_tokens, prompt_masks, step=t)
        if path == "device":
            sel = policy.act(predicted.unsqueeze(0), sample=True, n_samples=n, **CONTROLS)
            prev = sel.action_token if n == 1 else sel.action_token[..., 0, :]
        else:
            _, prev, _ = host_step(policy, predicted.unsqueeze(0), n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(observations) * 1e3


def evaluate(policy, path, predicted, actions):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if path == "device":
        out = policy.evaluate_actions(predicted, actions, **CONTROLS)
        logp = out.log_prob
    else:
        dists = {k: warp(d, **CONTROLS) for k, d in policy.forward_action_decoder(predicted).items()}
        logp = {k: dists[k].log_prob(actions[k]) for k in ACTION_KEYS}
        _ = {k: dists[k].entropy() for k in ACTION_KEYS}      # evaluate_actions returns the entropy too: the host path pays for it as well
        policy.forward_action_token(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, logp


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return q[0], q[2]


def report(lines, name, times, unit):
    med = {}
    for p in PATHS:
        v = times[p]
        q1, q3 = quartiles(v)
        med[p] = statistics.median(v)
        lines.append(f"  {name:<10} {p:<6} median {med[p]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  IQR {q3 - q1:7.3f} ms ({100 * (q3 - q1) / med[p]:.2f} %)")
    diff = med["device"] - med["host"]
    lines.append(f"  {name:<10} device - host = {diff:+.3f} ms per {unit} ({100 * diff / med['host']:+.2f} %)")
    return diff


def kernel_time(fn, iters=200):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="200M")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_act_sampling.py measures on the GPU: no device found")
    dev = "cuda:0"
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_state_dict(cfg, 0, head_gain=0.5), strict=True)
    lines = [f"scripts/time_act_sampling.py: VIMA-{args.model} bf16, controls {CONTROLS}; sample / candidates: incremental env-step loop of "
             f"examples/episode_loop.py, {args.steps} env steps per episode, ms per env step; evaluate: one call on a [8, B] block, ms per call",
             f"{args.repeats} timed runs per path (alternating host, device, host, device ... in one process) after {args.warmup} warm-up runs each",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "time: host clock with a device synchronise at both ends; spread: interquartile range of the timed runs", ""]
    slower = []
    for B in args.batches:
        prompt = syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1), dev)
        prompt_tokens, prompt_masks = policy.forward_prompt_assembly(prompt)
        observations = [syn.to_device(syn.make_obs(1, B, 4, seed=100 + t), dev) for t in range(args.steps)]
        lines.append(f"batch {B}:")
        for name, n_samples in (("sample", 1), ("candidates", N_CAND)):
            times = {p: [] for p in PATHS}
            for i in range(args.warmup + args.repeats):
                for p in PATHS:                      # alternating: clock drift and neighbours hit both paths alike
                    ms = episode(policy, p, n_samples, observations, prompt_tokens, prompt_masks)
                    if i >= args.warmup:
                        times[p].append(ms)
            if report(lines, name, times, "env step") > 0:
                slower.append((B, name))
        g = torch.Generator().manual_seed(5)
        predicted = torch.randn(8, B, policy.embed_dim, generator=g).to(dev)
        given = policy.act(predicted, sample=True, **CONTROLS).actions
        times = {p: [] for p in PATHS}
        lp = {}
        for i in range(args.warmup + args.repeats):
            for p in PATHS:
                ms, lp[p] = evaluate(policy, p, predicted, given)
                if i >= args.warmup:
                    times[p].append(ms)
        if report(lines, "evaluate", times, "call") > 0:
            slower.append((B, "evaluate"))
        finite = torch.isfinite(lp["host"]["pose0_rotation"]) & torch.isfinite(lp["device"]["pose0_rotation"])
        err = (lp["host"]["pose0_rotation"] - lp["device"]["pose0_rotation"])[finite].abs().max().item()
        lines.append(f"  evaluate   max |log_prob(host) - log_prob(device)| on pose0_rotation: {err:.2e} ({int((~finite).sum())} of {finite.numel()} "
                     "not finite on either path: sort-based and rank-based nucleus differ where the mass sits on p)")
        lines.append("")
    lines.append("kernel time on R rows of logits: HIP events around 200 back-to-back launches through the C ABI on fixed buffers (no "
                 "allocation, no torch work between the launches), us per launch:")
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for R in args.batches:
        x = torch.randn(R, 700, device=dev)
        T = torch.full((R,), 0.7, device=dev)

        def launcher(opts, S=1):
            u = torch.rand(R * S, 12, device=dev)
            idx, cont, logp, ent = alloc_outputs(R * S, dev)
            arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in idx])
            keep = (u, idx, cont, logp, ent)                          # the buffers live as long as the closure
            if opts is None:
                return lambda: (keep, lib.vima_action_select(x.data_ptr(), R, u.data_ptr(), None, arr, cont.data_ptr(), logp.data_ptr(),
                                                             ent.data_ptr(), stream))
            return lambda: (keep, lib.vima_action_select_ex(x.data_ptr(), R, u.data_ptr(), ctypes.byref(opts), None, arr, cont.data_ptr(),
                                                            logp.data_ptr(), ent.data_ptr(), stream))
        t_old = kernel_time(launcher(None))
        t_plain = kernel_time(launcher(_lib.VimaSampleOpts(T.data_ptr(), 0, 1.0, 1, 0)))
        t_k = kernel_time(launcher(_lib.VimaSampleOpts(T.data_ptr(), 10, 1.0, 1, 0)))
        t_new = kernel_time(launcher(_lib.VimaSampleOpts(T.data_ptr(), 10, 0.9, 1, 0)))
        t_cand = kernel_time(launcher(_lib.VimaSampleOpts(T.data_ptr(), 10, 0.9, N_CAND, 0), N_CAND))
        lines.append(f"  rows {R:>4}: act_select_kernel {t_old:6.2f}   act_sample_kernel: temperature only {t_plain:6.2f}   + top-k 10 {t_k:6.2f}   "
                     f"+ top-p 0.9 {t_new:6.2f}   the same, {N_CAND} candidates ({R * N_CAND} output rows) {t_cand:6.2f}")
    lines.append("")
    lines.append("device path slower than the host path (median): " + (", ".join(f"batch {b} {name}" for b, name in slower) if slower else "nowhere"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
