"""Rollout of B vectorised environments with a decoder-only baseline policy (VIMAGPTPolicy / VIMAGatoPolicy) on the MI355X path.
The prompt is a sequence PREFIX: `seq_prefill` runs it through the decoder once, every env step then feeds only its own tokens
(`seq_step`) against the K/V cache in the native handle, instead of re-feeding [prompt | sep | o, a, o, a, ...] to `forward`.

    python examples/baseline_rollout_loop.py [--policy gato] [--batch 32] [--steps 60] [--ring 1]

Per env step: forward_obs_token -> seq_step -> act (action head, mode, action embedding in one native call). Episodes end at different
steps; a finished sample is restarted with a new prompt (`seq_restart`: all flagged samples in one batched prefill) while the others
keep their histories. The batch shares ONE row space of n_positions rows. With `--ring 1` (the default; option "seq_ring") the rows behind
the prompt are a ring and a restart gives the sample's rows back: the loop never calls `seq_prefill` again, and a sample whose
`steps_left()` entry reaches 0 (its own episode would outgrow the ring) is restarted like a finished one. With `--ring 0` a restart
gives no rows back: when `steps_left()` reaches 0 the whole batch starts over with `seq_prefill` and every in-flight episode is cut
(Gato at this shape: every 18 env steps). Synthetic inputs stand in for the simulator.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vima_testing import synthetic as syn                      # noqa: E402
from vima_amd.baselines import build_baseline             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", default="gato", choices=["gpt", "gato"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--prompts", type=int, default=3, help="encoded prompt batches the new episodes draw from")
    ap.add_argument("--ring", type=int, default=1, choices=[0, 1], help="option seq_ring: the cache rows behind the prompt are a ring (1, default) or linear (0)")
    args = ap.parse_args()
    dev = "cuda:0"
    B = args.batch
    cfg = syn.BaselineConfig(args.policy, 768, 11, 12)
    policy = build_baseline(cfg, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_baseline_state_dict(cfg, 0), strict=True)
    policy.set_option("seq_ring", args.ring)
    # a real loop encodes the prompt of every new episode; here they come from a small pool (same layout -> same Lp)
    pool = []
    for k in range(args.prompts):
        tok, mask = policy.forward_prompt_assembly(syn.to_device(syn.make_rgb_prompt(B, n_segments=4, words_per_segment=6, seed=1 + k), dev))
        pool.append((tok.contiguous(), mask))
    prompt_tokens, prompt_masks = pool[0][0].clone(), pool[0][1].clone()             # [Lp, B, E], [B, Lp]: the CURRENT prompt of every sample
    observations = [syn.to_device(syn.make_rgb_obs(1, B, seed=100 + t), dev) for t in range(8)]   # stands in for env.step()
    length = [5 + (7 * b) % 11 for b in range(B)]                                     # env steps until sample b's episode is "done"
    age, which = [0] * B, [0] * B
    episodes = resets = 0
    prev = None
    policy.seq_prefill(prompt_tokens, prompt_masks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        if t > 0:
            flags = [age[b] >= length[b] for b in range(B)]
            left = policy.steps_left().tolist()                                       # host bookkeeping only: no synchronisation
            if args.ring:                                                             # a sample out of ring rows ends like a finished one
                flags = [f or n == 0 for f, n in zip(flags, left)]
            for b in range(B):
                if flags[b]:
                    episodes += 1
                    age[b], which[b] = 0, (which[b] + 1) % len(pool)
                    prompt_tokens[:, b], prompt_masks[b] = pool[which[b]][0][:, b], pool[which[b]][1][b]
            if not args.ring and left[0] == 0:
                # the shared row space is used up: every sample starts over. A simulator would finish the running episodes first (or re-feed
                # their histories); the synthetic ones are simply cut here
                policy.seq_prefill(prompt_tokens, prompt_masks)
                age, prev = [0] * B, None
                resets += 1
            elif any(flags):
                policy.seq_restart(flags, prompt_tokens, prompt_masks)                # all flagged samples in one call
        obs_token = policy.forward_obs_token(observations[t % len(observations)])     # [1, B, E] (gpt) or [1, B, Q, E] (gato)
        predicted = policy.seq_step(obs_token[0], prev)                               # the step counter lives in the policy
        sel = policy.act(predicted.unsqueeze(0))
        prev = sel.action_token                                                       # ignored for the samples restarted before the next step
        age = [a + 1 for a in age]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(f"{args.policy} batch {B}, seq_ring {args.ring}: {args.steps} env steps, {ms:.2f} ms per step including restarts; {episodes} episodes restarted, "
          f"{resets} batch-wide prefills after steps_left() == 0; last action pose0_position = {sel.continuous['pose0_position'][0, 0].tolist()}")


if __name__ == "__main__":
    main()
