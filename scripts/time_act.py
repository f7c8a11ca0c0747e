"""Wall time of one incremental env step (examples/episode_loop.py: forward_obs_token -> forward_step -> action) of VIMA-200M in
bf16 with the two action paths, alternated episode by episode inside one process on one GPU, at batch 1, 32 and 256:

    host   forward_action_decoder -> MultiCategorical.mode -> forward_action_token -> _de_discretize_actions
           (12 torch Categoricals, softmax + argmax per dimension, four action_l1 launches; the path before `VIMAPolicy.act` existed)
    act    VIMAPolicy.act (vima_act: action head, act_select_kernel, action embedding in one native call)

Per path and batch: the device-synchronised wall time per env step of every timed episode (host clock around the episode, a device
synchronise at both ends), its median, minimum, maximum and interquartile range (the run-to-run spread), and the LIBRARY's launches
per env step from the handle's profiler (one extra, untimed episode per path; torch's own kernels of the host path are not the
library's and are not counted there). The two paths must choose the same actions. Verdict per batch: the act median may exceed the
host median by at most the host path's interquartile range.

    python scripts/time_act.py [--batches 1 32 256] [--steps 8] [--repeats 15] [--warmup 3] [--out profiles/act_select_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vima_testing import synthetic as syn  # noqa: E402
from vima_amd.policy import VIMAPolicy, ACTION_KEYS  # noqa: E402

PATHS = ("host", "act")


def episode(policy, path, observations, prompt_tokens, prompt_masks):
    """One episode of len(observations) env steps; returns (ms per env step, discrete actions of the last step)."""
    prev = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t, obs in enumerate(observations):
        obs_token, obs_mask = policy.forward_obs_token(obs)
        predicted = policy.forward_step(obs_token, obs_mask, prev, prompt_tokens, prompt_masks, step=t)
        if path == "act":
            sel = policy.act(predicted.unsqueeze(0))
            actions, prev, continuous = sel.actions, sel.action_token, sel.continuous
        else:
            dists = policy.forward_action_decoder(predicted.unsqueeze(0))
            actions = {k: v.mode() for k, v in dists.items()}
            prev = policy.forward_action_token(actions)
            continuous = policy._de_discretize_actions(actions)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / len(observations) * 1e3
    return ms, actions, continuous


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="200M")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_act.py measures on the GPU: no device found")
    dev = "cuda:0"
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_state_dict(cfg, 0), strict=True)
    lines = [f"scripts/time_act.py: VIMA-{args.model} bf16, incremental env-step loop of examples/episode_loop.py, {args.steps} env steps per episode, "
             f"{args.repeats} timed episodes per path (alternating host, act, host, act ... in one process) after {args.warmup} warm-up episodes each",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "time: host clock around one episode with a device synchronise at both ends, divided by the env steps; ms per env step",
             "spread: interquartile range of the timed episodes; launches: the library's own, per env step, from vima_prof_read "
             "(the torch kernels of the host path's distribution step are not counted by it)", ""]
    verdicts = []
    for B in args.batches:
        prompt = syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1), dev)
        prompt_tokens, prompt_masks = policy.forward_prompt_assembly(prompt)
        observations = [syn.to_device(syn.make_obs(1, B, 4, seed=100 + t), dev) for t in range(args.steps)]
        last = {}
        for _ in range(args.warmup):
            for p in PATHS:
                _, last[p], _ = episode(policy, p, observations, prompt_tokens, prompt_masks)
        same = all(torch.equal(last["host"][k], last["act"][k]) for k in ACTION_KEYS)
        times = {p: [] for p in PATHS}
        for _ in range(args.repeats):
            for p in PATHS:                      # alternating: clock drift and neighbours hit both paths alike
                times[p].append(episode(policy, p, observations, prompt_tokens, prompt_masks)[0])
        launches = {}
        for p in PATHS:
            policy.prof_enable(True)
            policy.prof_read()
            episode(policy, p, observations, prompt_tokens, prompt_masks)
            r = policy.prof_read()
            policy.prof_enable(False)
            launches[p] = {k: r[k]["launches"] / args.steps for k in ("gemm", "attention", "other")}
        lines.append(f"batch {B}: last-step actions of the two paths identical: {same}")
        med = {}
        for p in PATHS:
            v = times[p]
            q1, q3 = quartiles(v)
            med[p] = statistics.median(v)
            n = launches[p]
            lines.append(f"  {p:<4} median {med[p]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  IQR {q3 - q1:7.3f} ms ({100 * (q3 - q1) / med[p]:.2f} %)   "
                         f"library launches per step: {sum(n.values()):7.2f} (gemm {n['gemm']:.2f}, attention {n['attention']:.2f}, other {n['other']:.2f})")
            lines.append(f"       episodes: {' '.join(f'{x:.3f}' for x in v)}")
        q1, q3 = quartiles(times["host"])
        diff = med["act"] - med["host"]
        ok = diff <= q3 - q1
        verdicts.append(ok and same)
        lines.append(f"  act - host = {diff:+.3f} ms per env step ({100 * diff / med['host']:+.2f} %); host IQR {q3 - q1:.3f} ms -> "
                     f"{'PASS' if ok else 'FAIL'}: act median {'is not' if ok else 'IS'} above the host median by more than the host path's spread")
        lines.append("")
    lines.append("all batches: " + ("PASS" if all(verdicts) else "FAIL"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
