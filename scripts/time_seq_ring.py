"""What continuous batched rollouts of the decoder-only baselines cost and save (option "seq_ring"): VIMAGatoPolicy and VIMAGPTPolicy at the
`bench.py --policy` shape (embed_dim 768, 11 layers, 12 heads, prompt of 8 x (8 words + 1 RGB frame pair)), bf16, batch 256, one process on one
GPU, ring off and ring on alternated window by window. No gate is fixed in advance: the numbers are reported either way.

    (a) env step (forward_obs_token -> seq_step -> act) in the FIRST lap, ring off against ring on: same rows, same keys read, the same launches;
        only the host bookkeeping differs. Expectation: equal within the interquartile range.
    (b) env step in steady state after the wrap, where every step reads the whole written image (about n_positions keys): the price of never
        starting over.
    (c) one seq_restart call with 1, 8 and 32 flagged samples (ring on, inside the running batch).
    (d) the batch-wide seq_prefill that the ring removes, and that time divided by the env steps a linear cache lasts.

Times: host clock around a window that starts and ends with a device synchronise; medians, interquartile ranges (the run-to-run spread), every
window listed. The comparison is always ring off in the same process, never a stored number.

    python scripts/time_seq_ring.py [--policies gato,gpt] [--batch 256] [--window 16] [--repeats 11] [--warmup 2] [--out profiles/seq_ring_time.txt]
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


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return q[0], q[2]


def summary(name, v, unit="ms"):
    q1, q3 = quartiles(v)
    med = statistics.median(v)
    return med, q3 - q1, [f"  {name:<22} median {med:9.3f} {unit}  min {min(v):9.3f}  max {max(v):9.3f}  IQR {q3 - q1:8.3f} {unit} ({100 * (q3 - q1) / med:.2f} %)",
                          f"       windows: {' '.join(f'{x:.3f}' for x in v)}"]


class Loop:
    """The env-step loop on one policy (the step counter lives in the policy); `start` begins a new batch episode with a prefill."""

    def __init__(self, policy, observations, prompt_tokens, prompt_masks):
        self.p, self.obs, self.pt, self.pm = policy, observations, prompt_tokens, prompt_masks
        self.step, self.prev = 0, None

    def start(self):
        """one batch-wide seq_prefill; returns ms (device-synchronised at both ends)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.p.seq_prefill(self.pt, self.pm)
        torch.cuda.synchronize()
        self.step, self.prev = 0, None
        return (time.perf_counter() - t0) * 1e3

    def steps(self, n):
        """n env steps; returns ms per env step (device-synchronised at both ends)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            obs_token = self.p.forward_obs_token(self.obs[self.step % len(self.obs)])
            predicted = self.p.seq_step(obs_token[0], self.prev)
            self.prev = self.p.act(predicted.unsqueeze(0)).action_token
            self.step += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def restart(self, flags):
        """one seq_restart call; returns ms (device-synchronised at both ends)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.p.seq_restart(flags, self.pt, self.pm)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3


def measure(kind, args, dev):
    B, W = args.batch, args.window
    cfg = syn.BaselineConfig(kind, 768, 11, 12)
    policy = build_baseline(cfg, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_baseline_state_dict(cfg, 0), strict=True)
    prompt_tokens, prompt_masks = policy.forward_prompt_assembly(syn.to_device(syn.make_rgb_prompt(B, n_segments=8, words_per_segment=8, seed=1236), dev))
    prompt_tokens = prompt_tokens.contiguous()
    observations = [syn.to_device(syn.make_rgb_obs(1, B, seed=100 + t), dev) for t in range(8)]
    loop = Loop(policy, observations, prompt_tokens, prompt_masks)
    Q, n_pos, Lp = cfg.obs_tokens, cfg.n_positions, prompt_tokens.shape[0]
    P0, R = Lp + 1, n_pos - Lp - 1
    life = 1 + (R - Q) // (Q + 1)          # env steps in the life of a linear cache, step 0 included
    W = min(W, life - 1)
    bytes_per_key = 2 * cfg.embed_dim * 2 * cfg.n_layer   # K | V, bf16, every layer
    lines = [f"---- {kind}: embed_dim 768, 11 layers, 12 heads, bf16, batch {B}, Q = {Q}, prompt {Lp} tokens + separator (P0 = {P0}), n_positions {n_pos}, ring R = {R} rows; "
             f"a linear cache lasts {life} env steps; windows of {W} env steps (forward_obs_token -> seq_step -> act), {args.repeats} timed windows per path after "
             f"{args.warmup} warm-up windows, paths alternated in one process", ""]

    # ---- (a) first lap, ring off / on: prefill and step 0 (untimed), then one window of steps 1 .. W; (d) the prefill of the same repeats
    times, prefill = {0: [], 1: []}, []
    for rep in range(args.warmup + args.repeats):
        for ring in (0, 1):
            policy.set_option("seq_ring", ring)
            ms_p = loop.start()
            loop.steps(1)
            ms = loop.steps(W)
            if rep >= args.warmup:
                times[ring].append(ms)
                prefill.append(ms_p)
    k_lo, k_hi = P0 + Q + Q + 1, P0 + Q + (Q + 1) * W
    lines.append(f"(a) env step in the first lap (steps 1 .. {W} after step 0: the same {Q + 1} new rows and {k_lo} .. {k_hi} keys in both modes)")
    med0, iqr0, txt = summary("ring off", times[0])
    lines += txt
    med1, iqr1, txt = summary("ring on", times[1])
    lines += txt
    lines += [f"  ring on - ring off = {med1 - med0:+.3f} ms per env step ({100 * (med1 - med0) / med0:+.2f} %); IQRs {iqr0:.3f} / {iqr1:.3f} ms: the medians "
              f"{'agree' if abs(med1 - med0) <= max(iqr0, iqr1) else 'DIFFER by more than'} within the run-to-run spread", ""]

    # ---- (b) steady state: ring on, run past the wrap; before every window all samples are restarted (untimed), so the window is legal and every
    # step reads the whole written image [0, hw)
    policy.set_option("seq_ring", 1)
    loop.start()
    everyone = [True] * B
    while loop.step * (Q + 1) < 2 * R + W * (Q + 1):      # two laps of warm-up: the high-water mark has stopped moving
        loop.steps(W)
        loop.restart(everyone)
    steady = []
    for rep in range(args.repeats):
        steady.append(loop.steps(W))
        loop.restart(everyone)
    lines.append(f"(b) env step in steady state after the wrap (ring on; every step reads the whole written image, ~{n_pos} keys instead of {k_lo} .. {k_hi}; "
                 f"restarts outside the timed windows; step counter at {loop.step})")
    med_b, _, txt = summary("ring on, steady", steady)
    lines += txt
    extra_keys = n_pos - (k_lo + k_hi) / 2
    lines += [f"  against the first lap with the ring off: {med_b - med0:+.3f} ms per env step ({100 * (med_b - med0) / med0:+.2f} %): about {extra_keys:.0f} more keys per "
              f"sample x {bytes_per_key} bytes of K | V per key over all layers x {B} samples = {extra_keys * bytes_per_key * B / 1e6:.0f} MB more cache traffic per step "
              "(most of those keys are masked: read, scored, weight 0)", ""]

    # ---- (c) one restart call inside the running batch (a restart is legal at any time and takes no ring rows)
    lines.append(f"(c) one seq_restart call (ring on): key-mask clear + one prefill of n_flagged x {P0} rows through the stack, scattered by sample list")
    for n_r in (1, 8, 32):
        if n_r > B:
            continue
        flags = [b % (B // n_r) == 0 and b // (B // n_r) < n_r for b in range(B)]
        assert sum(flags) == n_r
        t = []
        for rep in range(args.warmup + args.repeats):
            ms = loop.restart(flags)
            if rep >= args.warmup:
                t.append(ms)
        lines += summary(f"{n_r:2d} flagged", t)[2]
    lines.append("")

    # ---- (d) the batch-wide prefill the ring removes
    med_d, _, txt = summary("seq_prefill (batch)", prefill)
    lines.append(f"(d) the batch-wide seq_prefill of {B} prompts ({B} x {P0} rows through the stack), both modes pooled")
    lines += txt
    lines += [f"  a linear cache pays it every {life} env steps: {med_d / life:.3f} ms per env step ({100 * med_d / life / med0:.2f} % of the first-lap step), plus every "
              "in-flight episode cut; the ring pays (b) - (a) instead and keeps them", ""]
    del policy
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="gato,gpt")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--window", type=int, default=16, help="env steps per timed window (at most the life of a linear cache - 1)")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seq_ring.py measures on the GPU: no device found")
    dev = "cuda:0"
    lines = ["scripts/time_seq_ring.py: decoder-only baselines at the bench.py --policy shape, option seq_ring off against on",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "time: host clock around a window with a device synchronise at both ends; ms per env step (a, b), ms per call (c, d); spread: interquartile range", ""]
    for kind in args.policies.split(","):
        lines += measure(kind, args, dev)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
