"""Resume an interrupted rollout: the tokens of a running batch are all that has to be saved. A new policy object refills its episode
caches from them in ONE pass (`forward_steps`, the multi-step prefill) and goes on stepping; its actions equal those of the policy that
was never interrupted. The same tokens let ONE in-flight episode join another running batch (`restart_samples(..., history=)`).

    python examples/resume_rollout.py [--model 20M] [--batch 8] [--steps 6] [--more 4]

Synthetic inputs stand in for the simulator, as in examples/episode_loop.py.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vima_testing import synthetic as syn                      # noqa: E402
from vima_amd.policy import VIMAPolicy                    # noqa: E402


def make_policy(cfg, dev):
    policy = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_state_dict(cfg, 0), strict=True)   # create_policy_from_ckpt(path, dev) with a real checkpoint
    return policy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="20M")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6, help="env steps before the interruption")
    ap.add_argument("--more", type=int, default=4, help="env steps after it")
    args = ap.parse_args()
    dev, B, K, M = "cuda:0", args.batch, args.steps, args.more
    cfg = syn.config(args.model, xattn_n_positions=512)
    observations = [syn.to_device(syn.make_obs(1, B, 4, seed=100 + t), dev) for t in range(K + M)]   # stands in for env.step()
    prompt = syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1), dev)

    # ---- the rollout that is interrupted after K steps (and, for comparison, is in fact allowed to go on)
    first = make_policy(cfg, dev)
    prompt_tokens, prompt_masks = first.forward_prompt_assembly(prompt)
    saved_obs, saved_mask, saved_act, actions = [], [], [], []
    prev = None
    for t in range(K + M):
        obs_token, obs_mask = first.forward_obs_token(observations[t])
        sel = first.act(first.forward_step(obs_token, obs_mask, prev, prompt_tokens, prompt_masks, step=t).unsqueeze(0))
        prev = sel.action_token
        actions.append(sel.actions)
        if t < K:   # what a checkpoint of the rollout holds: the tokens fed so far and the actions taken
            saved_obs.append(obs_token[-1] if obs_token.dim() == 4 else obs_token)
            saved_mask.append(obs_mask[-1] if obs_mask.dim() == 3 else obs_mask)
            saved_act.append(prev[-1] if prev.dim() == 3 else prev)

    # ---- a new policy object: K steps of history in one pass, then on with single steps
    second = make_policy(cfg, dev)
    h_obs, h_mask, h_act = torch.stack(saved_obs), torch.stack(saved_mask), torch.stack(saved_act)      # [K,B,Q,E], [K,B,Q], [K,B,E]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    predicted = second.forward_steps(h_obs, h_mask, h_act[:K - 1] if K > 1 else None, prompt_tokens, prompt_masks, step=0)   # [K,B,E]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    replayed = second.act(predicted)                                                  # the teacher-forced pass scores the prefix as well
    same = all(torch.equal(replayed.actions[k][t], actions[t][k][0]) for t in range(K) for k in replayed.actions)
    prev = h_act[K - 1]
    for t in range(K, K + M):
        obs_token, obs_mask = second.forward_obs_token(observations[t])
        sel = second.act(second.forward_step(obs_token, obs_mask, prev, prompt_tokens, prompt_masks, step=t).unsqueeze(0))
        prev = sel.action_token
        same = same and all(torch.equal(sel.actions[k], actions[t][k]) for k in sel.actions)
    print(f"{args.model} batch {B}: {K} steps of history refilled in one pass ({ms:.2f} ms, first call), {M} further steps; "
          f"actions equal to the uninterrupted rollout: {same}")

    # ---- one episode of that batch joins another running batch (sample 0 of a batch that has taken K steps of its own)
    third = make_policy(cfg, dev)
    other = syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=2), dev)
    pt, pm = third.forward_prompt_assembly(other)
    pt, pm = pt.clone(), pm.clone()
    prev3 = None
    for t in range(K):
        obs_token, obs_mask = third.forward_obs_token(observations[(t + 3) % (K + M)])
        prev3 = third.act(third.forward_step(obs_token, obs_mask, prev3, pt, pm, step=t).unsqueeze(0)).action_token
    b = B - 1                                                                          # the episode that moves: sample b of the first batch
    pt[:, 0], pm[0] = prompt_tokens[:, b], prompt_masks[b]
    flags = [True] + [False] * (B - 1)
    assert third.history_room() >= K
    third.restart_samples(flags, pt, pm, history=(h_obs[:, b:b + 1], h_mask[:, b:b + 1], h_act[:K - 1, b:b + 1] if K > 1 else None))
    prev3 = prev3[-1] if prev3.dim() == 3 else prev3
    prev3 = prev3.clone()
    prev3[0] = h_act[K - 1, b]
    obs_token, obs_mask = third.forward_obs_token(observations[(K + 3) % (K + M)])
    own_token, own_mask = first.forward_obs_token(observations[K])
    obs_token, obs_mask = obs_token.clone(), obs_mask.clone()
    obs_token[..., 0, :, :], obs_mask[..., 0, :] = own_token[..., b, :, :], own_mask[..., b, :]
    sel = third.act(third.forward_step(obs_token, obs_mask, prev3, pt, pm, step=K).unsqueeze(0))
    moved = all(torch.equal(sel.actions[k][0, 0], actions[K][k][0, b]) for k in sel.actions)
    print(f"sample {b} moved into another batch as its sample 0 with {K} steps of history; its next action equals the one it took at home: {moved}")


if __name__ == "__main__":
    main()
