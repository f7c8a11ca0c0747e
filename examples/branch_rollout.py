"""Branch rollouts on the MI355X path: best-of-S action search with a look-ahead scorer, without recomputing anything. The batch holds G groups
of S slots; one slot of a group carries the group's episode (its "main" slot). At every k-th env step

    1. `act(predicted, sample=True, n_samples=S)` draws S candidate actions for the main slot from ONE pass of the action head,
    2. `fork_samples(source, ...)` copies the main slot's episode state (history K/V, key mask, position counter, prompt K/V) into the
       group's other S - 1 slots -- one table upload and three kernel launches, whatever G and S,
    3. the next `forward_step` feeds slot s candidate s: S one-step continuations of the same episode, side by side in the batch,
    4. a toy scorer (the confidence of the branch's next prediction: the summed log-probability of its mode) picks a branch, and the slot
       that holds it simply becomes the group's main slot: survivors keep their slots, nothing is copied back.

Between branch points every slot steps with the mode of its own prediction; the slots that are not main just run along.

    python examples/branch_rollout.py [--model 200M] [--groups 8] [--samples 4] [--every 4] [--steps 200]

Synthetic inputs stand in for the simulator, as in examples/rollout_loop.py (a real loop would clone the simulator state per branch). The
episode caches run as a ring (`decode_ring`); a group whose episode is done, or whose main slot is out of rows (`steps_left() == 0`), is
restarted as a whole with its next prompt.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vima_testing import synthetic as syn                      # noqa: E402
from vima_amd.policy import VIMAPolicy                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="200M")
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--samples", type=int, default=4, help="S: candidates per branch point = slots per group")
    ap.add_argument("--every", type=int, default=4, help="k: branch at every k-th env step")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--prompts", type=int, default=3, help="encoded prompt batches the new episodes draw from")
    args = ap.parse_args()
    dev = "cuda:0"
    G, S = args.groups, args.samples
    B = G * S                                                                          # slot g * S + s
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_state_dict(cfg, 0), strict=True)   # create_policy_from_ckpt(path, dev) with a real checkpoint
    policy.set_option("decode_ring", 1)
    group_of = torch.arange(B, device=dev) // S
    # one prompt per group, the same in all of its slots
    pool = []
    for k in range(args.prompts):
        pt, pm = policy.forward_prompt_assembly(syn.to_device(syn.make_prompt(G, n_segments=32, words_per_segment=8, q_per_view=4, seed=1 + k), dev))
        pool.append((pt[:, group_of].contiguous(), pm[group_of].contiguous()))
    prompt_tokens, prompt_masks = pool[0][0].clone(), pool[0][1].clone()             # [Lp, B, E], [B, Lp]
    observations = [syn.to_device(syn.make_obs(1, B, 4, seed=100 + t), dev) for t in range(16)]   # stands in for env.step() of every branch
    length = [12 + (7 * g) % 17 for g in range(G)]                                    # env steps until group g's episode is "done"
    main_slot = [g * S for g in range(G)]
    age, which = [0] * G, [0] * G
    episodes = branches = moved = 0
    prev, pending = None, []                                                          # the groups whose branches take their step next
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.steps):
        if t > 0:
            left = policy.steps_left().tolist()                                       # host bookkeeping only
            done = [age[g] >= length[g] or left[main_slot[g]] == 0 for g in range(G)]
            if any(done):
                flags = [done[b // S] for b in range(B)]
                for g in range(G):
                    if done[g]:
                        episodes += 1
                        age[g], which[g], main_slot[g] = 0, (which[g] + 1) % len(pool), g * S
                        sl = slice(g * S, (g + 1) * S)
                        prompt_tokens[:, sl], prompt_masks[sl] = pool[which[g]][0][:, sl], pool[which[g]][1][sl]
                policy.restart_samples(flags, prompt_tokens, prompt_masks)
        obs_token, obs_mask = policy.forward_obs_token(observations[t % len(observations)])
        predicted = policy.forward_step(obs_token, obs_mask, prev, prompt_tokens, prompt_masks, step=t)   # [B, E]
        mode = policy.act(predicted.unsqueeze(0))
        if pending:   # 4. the branches have taken their step: keep, per group, the one whose next prediction is the most confident
            score = sum(mode.log_prob.values())[0].view(G, S)
            best = score.argmax(dim=1).tolist()
            for g in pending:
                if age[g] > 0:                                                        # (a group restarted in front of this step has no branches left)
                    moved += g * S + best[g] != main_slot[g]
                    main_slot[g] = g * S + best[g]
            pending = []
        prev = mode.action_token[0].clone()                                           # [B, E]
        branching = [g for g in range(G) if (age[g] + 1) % args.every == 0 and age[g] + 1 < length[g]]
        if branching:
            heads = torch.tensor([main_slot[g] for g in branching], device=dev)
            cand = policy.act(predicted[heads].unsqueeze(0), sample=True, temperature=0.7, top_k=10, top_p=0.9, n_samples=S)   # 1.
            source = list(range(B))
            for i, g in enumerate(branching):
                for s in range(S):
                    source[g * S + s] = main_slot[g]
                prev[g * S:(g + 1) * S] = cand.action_token[0, i]                     # 3. slot s of the group is fed candidate s
            prompt_tokens, prompt_masks = policy.fork_samples(source, prompt_tokens, prompt_masks)   # 2.
            branches += len(branching)
            pending = branching
        age = [a + 1 for a in age]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(f"{args.model}, {G} groups x {S} slots: {args.steps} env steps, {ms:.2f} ms per step including restarts and forks; {branches} branch points "
          f"of {S} candidates ({moved} times another slot than the main one won), {episodes} episodes restarted; "
          f"last action pose0_position of group 0 = {mode.continuous['pose0_position'][0, main_slot[0]].tolist()}")


if __name__ == "__main__":
    main()
