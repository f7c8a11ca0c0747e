"""What the episode prefill of the decoder-only baselines saves (`seq_steps`, `seq_restart(..., history=)`): Gato (Q = 16) and GPT (Q = 1), embed_dim
768, 11 layers, 12 heads, bf16, n_positions 512, batch 32 and batch 1, one process on one GPU, the compared routes alternated window by window. The
decoder alone: observation and action tokens are prepared.

    (a) seq_steps of T env steps (steps 1 .. T behind an untimed prefill and step 0) against the T seq_step calls it replaces. Expected: the chunk
        wins by more than both interquartile ranges at every T (same arithmetic, 1 / T of the launches); where it does not, the record says so.
    (b) an install of 1 / 4 samples with T = 8 steps of history inside a running batch of 32, ring on (one seq_restart(history=) call), against the
        only alternative without it: replaying those episodes (seq_prefill with their prompts, then 8 seq_step calls) on a separate policy of that
        batch size.
    (c) the launch counts of (a) and (b), from the profiling counters, in runs of their own.

Times: host clock around a window that starts and ends with a device synchronise; medians, interquartile ranges (the run-to-run spread), every
window listed.

    python scripts/time_seq_prefill.py [--kinds gato,gpt] [--batches 32,1] [--repeats 11] [--warmup 2] [--out profiles/seq_prefill_time.txt]
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
from vima_amd.baselines import build_baseline  # noqa: E402

TS = {"gato": (2, 8, 16), "gpt": (2, 8, 32)}
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
    policy = build_baseline(cfg, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_baseline_state_dict(cfg, 0), strict=True)
    return policy


def tokens(policy, B, steps, dev):
    """obs tokens [steps,B,Q,E] ([steps,B,E] for GPT) and action tokens [steps,B,E]: 8 distinct env steps, repeated"""
    o = [policy.forward_obs_token(syn.to_device(syn.make_rgb_obs(1, B, seed=100 + t), dev))[0] for t in range(8)]
    a = policy.forward_action_token(syn.to_device(syn.make_actions(8, B, seed=7), dev))
    idx = [t % 8 for t in range(steps)]
    return torch.stack([o[i] for i in idx]).contiguous(), a[idx].contiguous()


def verdict(lines, verdicts, tag, what, m0, i0, m1, i1, n0, n1, names):
    good = m0 - m1 > max(i0, i1)
    verdicts.append((tag, good))
    lines.append(f"  {names[0]} - {names[1]} = {m0 - m1:+.3f} ms ({m0 / m1:.2f}x); IQRs {i0:.3f} / {i1:.3f} ms -> the {what} "
                 f"{'wins by more than both spreads' if good else 'does NOT win by more than both spreads'}; (c) launches {n0} against {n1}")


def measure(kind, args, dev, lines, verdicts):
    cfg = syn.BaselineConfig(kind, 768, 11, 12)
    policy = make_policy(cfg, dev)
    Q = cfg.obs_tokens
    for B in [int(x) for x in args.batches.split(",")]:
        pt, pm = policy.forward_prompt_assembly(syn.to_device(syn.make_rgb_prompt(B, n_segments=8, words_per_segment=8, seed=1236), dev))
        pt = pt.contiguous()
        Lp = pt.shape[0]
        otok, atok = tokens(policy, B, max(TS[kind]) + 1, dev)
        lines.append(f"---- {kind}: embed_dim 768, 11 layers, 12 heads, bf16, Q = {Q}, prompt {Lp} tokens + separator, n_positions {cfg.n_positions}, batch {B}")

        def start():
            policy.seq_prefill(pt, pm)
            policy.seq_step(otok[0])

        def singles(T):
            for t in range(1, T + 1):
                policy.seq_step(otok[t], atok[t - 1])

        def chunk(T):
            policy.seq_steps(otok[1:T + 1], atok[0:T])

        lines.append("(a) env steps 1 .. T behind an untimed prefill and step 0, T seq_step calls against one seq_steps call")
        for T in TS[kind]:
            t = {"steps": [], "chunk": []}
            for rep in range(args.warmup + args.repeats):
                for route, fn in (("steps", singles), ("chunk", chunk)):
                    start()
                    ms = timed(lambda: fn(T))
                    if rep >= args.warmup:
                        t[route].append(ms)
            m0, i0, txt = summary(f"T = {T:2d}, {T} seq_step", t["steps"])
            lines += txt
            m1, i1, txt = summary(f"T = {T:2d}, seq_steps", t["chunk"])
            lines += txt
            start()
            n0 = launches(policy, lambda: singles(T))
            start()
            n1 = launches(policy, lambda: chunk(T))
            verdict(lines, verdicts, f"(a) {kind} batch {B} T {T}", "chunk", m0, i0, m1, i1, n0, n1, ("steps", "chunk"))
        lines.append("")
        if B < 8:
            continue
        # ---- (b) install against replay, inside the running batch of B
        policy.set_option("seq_ring", 1)
        start()
        singles(HIST_T)
        assert policy.seq_history_room() >= HIST_T
        lines.append(f"(b) batch {B}, ring on, at batch step {HIST_T + 1}: one seq_restart(history=) call of n samples with T = {HIST_T} against replaying them "
                     f"(seq_prefill, seq_step 0 .. {HIST_T - 1}) on a separate policy of batch n")
        small = make_policy(cfg, dev)
        for n_r in (1, 4):
            flags = [b % (B // n_r) == 0 and b // (B // n_r) < n_r for b in range(B)]
            who = [b for b in range(B) if flags[b]]
            hist = (otok[:HIST_T, who].contiguous(), atok[:HIST_T - 1, who].contiguous())
            spt, spm = pt[:, who].contiguous(), pm[who].contiguous()

            def install():
                policy.seq_restart(flags, pt, pm, history=hist)

            def replay():
                small.seq_prefill(spt, spm)
                for s in range(HIST_T):
                    small.seq_step(hist[0][s], hist[1][s - 1] if s > 0 else None)

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
            verdict(lines, verdicts, f"(b) {kind} batch {B} n {n_r}", "install", m0, i0, m1, i1, n0, n1, ("replay", "install"))
        del small
        policy.set_option("seq_ring", 0)
        lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="gato,gpt")
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seq_prefill.py measures on the GPU: no device found")
    dev = "cuda:0"
    lines = [f"scripts/time_seq_prefill.py: {args.repeats} timed windows per route after {args.warmup} warm-up windows, routes alternated in one process; the "
             f"decoder alone (tokens prepared)",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "time: host clock around a window with a device synchronise at both ends; ms per window; spread: interquartile range", ""]
    verdicts = []
    for kind in args.kinds.split(","):
        measure(kind, args, dev, lines, verdicts)
    lines.append("expected wins: " + "; ".join(f"{k}: {'yes' if v else 'NO'}" for k, v in verdicts))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
