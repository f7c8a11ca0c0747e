"""Continuous rollout of B vectorised environments on the MI355X path: the batch never stops. Episodes end at different steps; a
finished sample is restarted with a new prompt (`restart_samples`) while the others keep their histories, and the episode caches'
shared row space is a ring (`set_option("decode_ring", 1)`), so no step count forces the whole batch back to step 0.

    python examples/rollout_loop.py [--model 200M] [--batch 32] [--steps 500] [--prompts 3] [--stochastic]

Per env step: forward_obs_token -> forward_step -> act (action head, mode, action embedding in one native call). Synthetic inputs
stand in for the simulator, as in examples/episode_loop.py. Episode lengths are staggered (6 .. 28 steps); every eighth sample's
episode "never ends" and shows the one rule of ring mode: a sample's own episode is bounded by n_positions tokens, `steps_left()`
tells how many more steps each sample can take, and a sample at 0 is restarted before the next step (here: its episode is cut).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vima_testing import synthetic as syn                      # noqa: E402
from vima_amd.policy import VIMAPolicy                    # noqa: E402


def pick_candidate(cand, best):
    """`cand`: the ActionSelection of act(..., n_samples=S), every field with a sample axis after the leading dims; `best` int64
    [...]: the candidate to keep per state -> the ActionSelection of that candidate alone, every field without the sample axis."""
    def pick(v, has_feature_axis):
        index = best[..., None, None].expand(*best.shape, 1, v.shape[-1]) if has_feature_axis else best[..., None]
        return torch.gather(v, best.dim(), index).squeeze(best.dim())
    return cand._replace(actions={k: pick(v, True) for k, v in cand.actions.items()},
                         continuous={k: pick(v, True) for k, v in cand.continuous.items()},
                         log_prob={k: pick(v, False) for k, v in cand.log_prob.items()},
                         entropy={k: pick(v, False) for k, v in cand.entropy.items()},
                         action_token=pick(cand.action_token, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="200M")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--prompts", type=int, default=3, help="encoded prompt batches the new episodes draw from")
    ap.add_argument("--stochastic", action="store_true", help="sample 4 candidate actions per state on the device (temperature 0.7, top-k 10, "
                    "top-p 0.9) and take the likeliest, instead of the mode")
    args = ap.parse_args()
    dev = "cuda:0"
    B = args.batch
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_state_dict(cfg, 0), strict=True)   # create_policy_from_ckpt(path, dev) with a real checkpoint
    policy.set_option("decode_ring", 1)
    # a real loop encodes the prompt of every new episode (forward_prompt_assembly on the restarted samples); here they come from a small pool
    pool = [policy.forward_prompt_assembly(syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1 + k), dev))
            for k in range(args.prompts)]
    prompt_tokens, prompt_masks = pool[0][0].clone(), pool[0][1].clone()             # [Lp, B, E], [B, Lp]: the CURRENT prompt of every sample
    observations = [syn.to_device(syn.make_obs(1, B, 4, seed=100 + t), dev) for t in range(16)]   # stands in for env.step()
    length = [10 ** 9 if b % 8 == 7 else 6 + (7 * b) % 23 for b in range(B)]          # env steps until sample b's episode is "done"
    age, which = [0] * B, [0] * B
    episodes = forced = 0
    prev = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        if t > 0:
            left = policy.steps_left().tolist()                                       # host bookkeeping only: no synchronisation
            flags = [age[b] >= length[b] or left[b] == 0 for b in range(B)]
            if any(flags):
                for b in range(B):
                    if flags[b]:
                        forced += age[b] < length[b]
                        episodes += 1
                        age[b], which[b] = 0, (which[b] + 1) % len(pool)
                        prompt_tokens[:, b], prompt_masks[b] = pool[which[b]][0][:, b], pool[which[b]][1][b]
                policy.restart_samples(flags, prompt_tokens, prompt_masks)             # all flagged samples in one call
        obs_token, obs_mask = policy.forward_obs_token(observations[t % len(observations)])
        predicted = policy.forward_step(obs_token, obs_mask, prev, prompt_tokens, prompt_masks, step=t)   # step just counts up
        if args.stochastic:   # 4 candidates per state from one pass of the action head; keep the one with the largest log-probability
            cand = policy.act(predicted.unsqueeze(0), sample=True, temperature=0.7, top_k=10, top_p=0.9, n_samples=4)
            sel = pick_candidate(cand, sum(cand.log_prob.values()).argmax(dim=-1))
        else:
            sel = policy.act(predicted.unsqueeze(0))
        prev = sel.action_token                                                       # ignored for the samples restarted before the next step
        age = [a + 1 for a in age]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(f"{args.model} batch {B}: {args.steps} env steps without a batch-wide reset, {ms:.2f} ms per step including restarts; "
          f"{episodes} episodes restarted ({forced} of them cut by steps_left() == 0); "
          f"last action pose0_position = {sel.continuous['pose0_position'][0, 0].tolist()}")


if __name__ == "__main__":
    main()
