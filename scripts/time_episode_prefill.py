"""What the episode prefill saves (`forward_steps`, `restart_samples(..., history=)`): VIMA-200M, bf16, Q = 8, 512-token prompts, batch 256 and
batch 1, one process on one GPU, the compared routes alternated window by window. The decoder alone: observation and action tokens are prepared.

    (a) forward_steps of T = 2 / 8 / 32 env steps (steps 1 .. T behind an untimed step 0) against the T forward_step calls it replaces. Expected:
        the chunk wins by more than both interquartile ranges at every T (same arithmetic, 1 / T of the launches); where it does not, the record
        says so.
    (b) an install of 1 / 8 / 32 samples with T = 8 steps of history inside a running batch of 256 (one restart_samples call) against the only
        alternative without it: replaying those episodes with forward_step (step 0 with their prompts, then 7 steps) on a separate policy of that
        batch size.
    (c) the launch counts of (a) and (b), from the profiling counters, in runs of their own.

Times: host clock around a window that starts and ends with a device synchronise; medians, interquartile ranges (the run-to-run spread), every
window listed.

    python scripts/time_episode_prefill.py [--model 200M] [--batches 256,1] [--repeats 11] [--warmup 2] [--out profiles/episode_prefill_time.txt]
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
from vima_amd.policy import VIMAPolicy  # noqa: E402

TS = (2, 8, 32)
HIST_T = 8


def summary(name, v, unit="ms"):
    q = statistics.quantiles(v, n=4, method="inclusive")
    med, iqr = statistics.median(v), q[2] - q[0]
    return med, iqr, [f"  {name:<26} median {med:9.3f} {unit}  min {min(v):9.3f}  max {max(v):9.3f}  IQR {iqr:8.3f} {unit} ({100 * iqr / med:.2f} %)",
                      f"       windows: {' '.join(f'{x:.3f}' for x in v)}"]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launches(policy, fn):
    policy.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    n = sum(v["launches"] for v in policy.prof_read().values())
    policy.prof_enable(False)
    return n


def make_policy(cfg, dev):
    policy = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_state_dict(cfg, 0), strict=True)
    return policy


def tokens(policy, B, steps, dev):
    """[steps,B,Q,E], [steps,B,Q], [steps,B,E]: 8 distinct env steps, repeated"""
    o, m = [], []
    for t in range(8):
        ot, om = policy.forward_obs_token(syn.to_device(syn.make_obs(1, B, 4, seed=100 + t), dev))
        o.append(ot.reshape(B, ot.shape[-2], ot.shape[-1]))
        m.append(om.reshape(B, om.shape[-1]))
    a = policy.forward_action_token(syn.to_device(syn.make_actions(8, B, seed=7), dev))
    idx = [t % 8 for t in range(steps)]
    return torch.stack([o[i] for i in idx]).contiguous(), torch.stack([m[i] for i in idx]).contiguous(), a[idx].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="200M")
    ap.add_argument("--batches", default="256,1")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_episode_prefill.py measures on the GPU: no device found")
    dev = "cuda:0"
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = make_policy(cfg, dev)
    lines = [f"scripts/time_episode_prefill.py: VIMA-{args.model} bf16, Q = 8, 512-token prompts, n_positions {cfg.n_positions}; {args.repeats} timed windows per "
             f"route after {args.warmup} warm-up windows, routes alternated in one process; the decoder alone (tokens prepared)",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "time: host clock around a window with a device synchronise at both ends; ms per window; spread: interquartile range", ""]
    verdicts = []
    for B in [int(x) for x in args.batches.split(",")]:
        pt, pm = policy.forward_prompt_assembly(syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1), dev))
        otok, omask, atok = tokens(policy, B, max(TS) + 1, dev)

        def step0():
            policy.forward_step(otok[0], omask[0], None, pt, pm, step=0)

        def singles(T):
            for t in range(1, T + 1):
                policy.forward_step(otok[t], omask[t], atok[t - 1], pt, pm, step=t)

        def chunk(T):
            policy.forward_steps(otok[1:T + 1], omask[1:T + 1], atok[0:T], pt, pm, step=1)

        lines.append(f"(a) batch {B}: env steps 1 .. T behind an untimed step 0, T forward_step calls against one forward_steps call")
        for T in TS:
            t = {"steps": [], "chunk": []}
            for rep in range(args.warmup + args.repeats):
                for route, fn in (("steps", singles), ("chunk", chunk)):
                    step0()
                    ms = timed(lambda: fn(T))
                    if rep >= args.warmup:
                        t[route].append(ms)
            m0, i0, txt = summary(f"T = {T:2d}, {T} forward_step", t["steps"])
            lines += txt
            m1, i1, txt = summary(f"T = {T:2d}, forward_steps", t["chunk"])
            lines += txt
            step0()
            n0 = launches(policy, lambda: singles(T))
            step0()
            n1 = launches(policy, lambda: chunk(T))
            good = m0 - m1 > max(i0, i1)
            verdicts.append((f"(a) batch {B} T {T}", good))
            lines.append(f"  steps - chunk = {m0 - m1:+.3f} ms ({m0 / m1:.2f}x); IQRs {i0:.3f} / {i1:.3f} ms -> the chunk "
                         f"{'wins by more than both spreads' if good else 'does NOT win by more than both spreads'}; (c) launches {n0} against {n1}")
        lines.append("")
        if B < 64:
            continue
        # ---- (b) install against replay, inside the running batch of B
        policy.set_option("decode_ring", 1)
        step0()
        singles(HIST_T)
        assert policy.history_room() >= HIST_T
        lines.append(f"(b) batch {B}, ring on, at batch step {HIST_T + 1}: one restart_samples(history=) call of n samples with T = {HIST_T} against replaying them "
                     f"(forward_step 0 .. {HIST_T - 1}) on a separate policy of batch n")
        small = make_policy(cfg, dev)
        for n_r in (1, 8, 32):
            flags = [b % (B // n_r) == 0 and b // (B // n_r) < n_r for b in range(B)]
            who = [b for b in range(B) if flags[b]]
            hist = (otok[:HIST_T, who].contiguous(), omask[:HIST_T, who].contiguous(), atok[:HIST_T - 1, who].contiguous())
            spt, spm = pt[:, who].contiguous(), pm[who].contiguous()

            def install():
                policy.restart_samples(flags, pt, pm, history=hist)

            def replay():
                for s in range(HIST_T):
                    small.forward_step(hist[0][s], hist[1][s], hist[2][s - 1] if s > 0 else None, spt, spm, step=s)

            t = {"install": [], "replay": []}
            for rep in range(args.warmup + args.repeats):
                for route, fn in (("replay", replay), ("install", install)):
                    ms = timed(fn)
                    if rep >= args.warmup:
                        t[route].append(ms)
            m0, i0, txt = summary(f"n = {n_r:2d}, replay", t["replay"])
            lines += txt
            m1, i1, txt = summary(f"n = {n_r:2d}, install", t["install"])
            lines += txt
            n0, n1 = launches(small, replay), launches(policy, install)
            good = m0 - m1 > max(i0, i1)
            verdicts.append((f"(b) batch {B} n {n_r}", good))
            lines.append(f"  replay - install = {m0 - m1:+.3f} ms ({m0 / m1:.2f}x); IQRs {i0:.3f} / {i1:.3f} ms -> the install "
                         f"{'wins by more than both spreads' if good else 'does NOT win by more than both spreads'}; (c) launches {n0} against {n1}")
        del small
        policy.set_option("decode_ring", 0)
        lines.append("")
    lines.append("expected wins: " + "; ".join(f"{k}: {'yes' if v else 'NO'}" for k, v in verdicts))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
