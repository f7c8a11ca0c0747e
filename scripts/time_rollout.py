"""What continuous batched rollouts cost and save (option "decode_ring", batched `restart_samples`): VIMA-200M, bf16, batch 256, Q = 8,
512-token prompts, one process on one GPU, the compared paths alternated window by window.

    (a) env step (forward_obs_token -> forward_step -> act) in the FIRST lap, ring off against ring on: same rows, same keys read, only the
        bookkeeping and the windowed causal compare differ. Gate: the ring-on median may exceed the ring-off median by at most the ring-off
        interquartile range.
    (b) env step in steady state after the wrap, where every step reads the whole written ring (about n_positions keys): the price of never resetting.
    (c) one restart_samples call with 1, 8 and 32 flagged samples, per-sample loop (restart_batched 0) against the batched form (1). Gate: at 32 the
        batched median lies below the loop's median by more than both interquartile ranges.
    (d) a full batch reset (forward_step step 0: the prompt K/V of all 256 samples), and that time divided by the 57 steps a linear cache lasts.

Times: host clock around a window that starts and ends with a device synchronise; medians, interquartile ranges (the run-to-run spread), every
window listed.

    python scripts/time_rollout.py [--batch 256] [--window 16] [--repeats 11] [--warmup 2] [--out profiles/rollout_ring_time.txt]
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


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return q[0], q[2]


def summary(name, v, unit="ms"):
    q1, q3 = quartiles(v)
    med = statistics.median(v)
    return med, q3 - q1, [f"  {name:<22} median {med:9.3f} {unit}  min {min(v):9.3f}  max {max(v):9.3f}  IQR {q3 - q1:8.3f} {unit} ({100 * (q3 - q1) / med:.2f} %)",
                          f"       windows: {' '.join(f'{x:.3f}' for x in v)}"]


class Loop:
    """The env-step loop on one policy; `step` counts up across windows until `start` begins a new batch episode."""

    def __init__(self, policy, observations, prompt_tokens, prompt_masks):
        self.p, self.obs, self.pt, self.pm = policy, observations, prompt_tokens, prompt_masks
        self.step, self.prev = 0, None

    def start(self):
        self.step, self.prev = 0, None

    def steps(self, n):
        """n env steps; returns ms per env step (device-synchronised at both ends)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            obs_token, obs_mask = self.p.forward_obs_token(self.obs[self.step % len(self.obs)])
            predicted = self.p.forward_step(obs_token, obs_mask, self.prev, self.pt, self.pm, step=self.step)
            self.prev = self.p.act(predicted.unsqueeze(0)).action_token
            self.step += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def restart(self, flags):
        """one restart_samples call; returns ms (device-synchronised at both ends)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.p.restart_samples(flags, self.pt, self.pm)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="200M")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--window", type=int, default=16, help="env steps per timed window")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rollout.py measures on the GPU: no device found")
    dev = "cuda:0"
    B, W = args.batch, args.window
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_state_dict(cfg, 0), strict=True)
    prompt_tokens, prompt_masks = policy.forward_prompt_assembly(syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1), dev))
    observations = [syn.to_device(syn.make_obs(1, B, 4, seed=100 + t), dev) for t in range(8)]
    loop = Loop(policy, observations, prompt_tokens, prompt_masks)
    Q = 8
    n_pos = 512
    lines = [f"scripts/time_rollout.py: VIMA-{args.model} bf16, batch {B}, Q = {Q}, prompt {prompt_tokens.shape[0]} tokens, n_positions {n_pos}; "
             f"windows of {W} env steps (forward_obs_token -> forward_step -> act), {args.repeats} timed windows per path after {args.warmup} warm-up windows, "
             "paths alternated in one process",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "time: host clock around a window with a device synchronise at both ends; ms per env step (a, b), ms per call (c, d); spread: interquartile range", ""]
    ok = True

    # ---- (a) first lap, ring off / on: step 0 (untimed, builds the prompt K/V), then one window of steps 1 .. W
    times = {0: [], 1: []}
    for rep in range(args.warmup + args.repeats):
        for ring in (0, 1):
            policy.set_option("decode_ring", ring)
            loop.start()
            loop.steps(1)
            ms = loop.steps(W)
            if rep >= args.warmup:
                times[ring].append(ms)
    lines.append(f"(a) env step in the first lap (steps 1 .. {W} after step 0, the same {Q + 1} new rows and {Q} .. {Q + (Q + 1) * W} keys in both modes)")
    med0, iqr0, txt = summary("ring off", times[0])
    lines += txt
    med1, iqr1, txt = summary("ring on", times[1])
    lines += txt
    good = med1 - med0 <= iqr0
    ok &= good
    lines += [f"  ring on - ring off = {med1 - med0:+.3f} ms per env step ({100 * (med1 - med0) / med0:+.2f} %); ring-off IQR {iqr0:.3f} ms -> "
              f"{'PASS' if good else 'FAIL'}: the ring-on median {'is not' if good else 'IS'} above the ring-off median by more than the ring-off spread", ""]

    # ---- (b) steady state: ring on, run past the wrap; before every window all samples are restarted (untimed), so the window is legal and
    # every step reads the whole written ring
    policy.set_option("decode_ring", 1)
    loop.start()
    everyone = [True] * B
    steady = []
    laps = 0
    while loop.step * (Q + 1) < 2 * n_pos:      # two laps of warm-up: the high-water mark reaches the end of the ring
        loop.steps(W)
        loop.restart(everyone)
        laps += 1
    for rep in range(args.repeats):
        steady.append(loop.steps(W))
        loop.restart(everyone)
    lines.append(f"(b) env step in steady state after the wrap (ring on; every step reads the whole written ring, ~{n_pos} keys instead of {Q} .. {Q + (Q + 1) * W}; "
                 f"restarts outside the timed windows; step counter at {loop.step})")
    med_b, _, txt = summary("ring on, steady", steady)
    lines += txt
    lines += [f"  against the first lap with the ring off: {med_b - med0:+.3f} ms per env step ({100 * (med_b - med0) / med0:+.2f} %). No gate: the price of the feature.", ""]
    # ---- (c) one restart call, loop against batched (ring on, running batch; a restart is legal at any time)
    lines.append("(c) one restart_samples call (new prompt K/V of the flagged samples: gather + per layer GEMM + scatter), per-sample loop against batched")
    for n_r in (1, 8, 32):
        flags = [b % (B // n_r) == 0 and b // (B // n_r) < n_r for b in range(B)]
        assert sum(flags) == n_r
        t = {0: [], 1: []}
        for rep in range(args.warmup + args.repeats):
            for batched in (0, 1):
                policy.set_option("restart_batched", batched)      # (does not end the running episode)
                ms = loop.restart(flags)
                if rep >= args.warmup:
                    t[batched].append(ms)
        m0, i0, txt = summary(f"{n_r:2d} flagged, loop", t[0])
        lines += txt
        m1, i1, txt = summary(f"{n_r:2d} flagged, batched", t[1])
        lines += txt
        if n_r == 32:
            good = m0 - m1 > max(i0, i1)
            ok &= good
            lines.append(f"  loop - batched = {m0 - m1:+.3f} ms per call at 32 flagged; IQRs {i0:.3f} / {i1:.3f} ms -> {'PASS' if good else 'FAIL'}: the batched median "
                         f"{'lies' if good else 'does NOT lie'} below the loop's by more than both spreads")
        else:
            lines.append(f"  loop - batched = {m0 - m1:+.3f} ms per call")
    policy.set_option("restart_batched", 1)
    lines.append("")

    # ---- (d) a full batch reset: step 0 with all prompts
    reset = []
    for rep in range(args.warmup + 5):
        loop.start()
        ms = loop.steps(1)
        if rep >= args.warmup:
            reset.append(ms)
    left = (n_pos + 1) // (Q + 1)          # steps in the life of a linear cache, step 0 included
    med_d, _, txt = summary("step 0 (batch reset)", reset)
    lines.append(f"(d) a full batch reset: env step 0 with {B} prompts (prompt K/V of every sample, all layers)")
    lines += txt
    lines += [f"  a linear cache pays it every {left} steps: {med_d / left:.3f} ms per env step ({100 * med_d / left / med0:.2f} % of the first-lap step), plus every "
              "in-flight episode thrown away; the ring pays (b) - (a) instead and keeps them", ""]
    lines.append("gates (a) and (c): " + ("PASS" if ok else "FAIL"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
