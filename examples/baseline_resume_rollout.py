"""Resume an interrupted rollout of a decoder-only baseline policy (VIMAGPTPolicy / VIMAGatoPolicy): the tokens of a running batch are all that
has to be saved. A new policy object prefills the prompts (`seq_prefill`), refills its episode cache from the saved tokens in ONE pass
(`seq_steps`, the multi-step prefill) and goes on stepping; its actions equal those of the policy that was never interrupted. The same tokens
let ONE in-flight episode join another running batch (`seq_restart(..., history=)`). The decoder-only twin of examples/resume_rollout.py.

    python examples/baseline_resume_rollout.py [--policy gato] [--batch 8] [--steps 6] [--more 4]

Synthetic inputs stand in for the simulator, as in examples/baseline_rollout_loop.py.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vima_testing import synthetic as syn                      # noqa: E402
from vima_amd.baselines import build_baseline             # noqa: E402


def make_policy(cfg, dev):
    policy = build_baseline(cfg, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_baseline_state_dict(cfg, 0), strict=True)
    return policy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", default="gato", choices=["gpt", "gato"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6, help="env steps before the interruption")
    ap.add_argument("--more", type=int, default=4, help="env steps after it")
    args = ap.parse_args()
    dev, B, K, M = "cuda:0", args.batch, args.steps, args.more
    cfg = syn.BaselineConfig(args.policy, 768, 11, 12)
    observations = [syn.to_device(syn.make_rgb_obs(1, B, seed=100 + t), dev) for t in range(K + M)]   # stands in for env.step()
    prompt = syn.to_device(syn.make_rgb_prompt(B, n_segments=4, words_per_segment=6, seed=1), dev)

    # ---- the rollout that is interrupted after K steps (and, for comparison, is in fact allowed to go on)
    first = make_policy(cfg, dev)
    prompt_tokens, prompt_masks = first.forward_prompt_assembly(prompt)
    prompt_tokens = prompt_tokens.contiguous()
    first.seq_prefill(prompt_tokens, prompt_masks)
    saved_obs, saved_act, actions = [], [], []
    prev = None
    for t in range(K + M):
        obs_token = first.forward_obs_token(observations[t])[0]                        # [B, Q, E] (gato) / [B, E] (gpt)
        sel = first.act(first.seq_step(obs_token, prev).unsqueeze(0))
        prev = sel.action_token[-1] if sel.action_token.dim() == 3 else sel.action_token
        actions.append(sel.actions)
        if t < K:   # what a checkpoint of the rollout holds: the tokens fed so far and the actions taken
            saved_obs.append(obs_token)
            saved_act.append(prev)

    # ---- a new policy object: the prompts, then K steps of history in one pass, then on with single steps
    second = make_policy(cfg, dev)
    h_obs, h_act = torch.stack(saved_obs), torch.stack(saved_act)                      # [K,B,Q,E] ([K,B,E] for gpt), [K,B,E]
    second.seq_prefill(prompt_tokens, prompt_masks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    predicted = second.seq_steps(h_obs, h_act[:K - 1] if K > 1 else None)              # [K,B,E]: before the batch's first step, K - 1 actions
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    replayed = second.act(predicted)                                                   # the teacher-forced pass scores the prefix as well
    same = all(torch.equal(replayed.actions[k][t], actions[t][k][0]) for t in range(K) for k in replayed.actions)
    prev = h_act[K - 1]
    for t in range(K, K + M):
        obs_token = second.forward_obs_token(observations[t])[0]
        sel = second.act(second.seq_step(obs_token, prev).unsqueeze(0))
        prev = sel.action_token[-1] if sel.action_token.dim() == 3 else sel.action_token
        same = same and all(torch.equal(sel.actions[k], actions[t][k]) for k in sel.actions)
    print(f"{args.policy} batch {B}: {K} steps of history refilled in one pass ({ms:.2f} ms, first call), {M} further steps; "
          f"actions equal to the uninterrupted rollout: {same}")

    # ---- one episode of that batch joins another running batch (as sample 0 of a batch that has taken K steps of its own)
    third = make_policy(cfg, dev)
    other = syn.to_device(syn.make_rgb_prompt(B, n_segments=4, words_per_segment=6, seed=2), dev)     # same layout -> same Lp
    pt, pm = third.forward_prompt_assembly(other)
    pt, pm = pt.contiguous().clone(), pm.clone()
    third.seq_prefill(pt, pm)
    prev3 = None
    for t in range(K):
        obs_token = third.forward_obs_token(observations[(t + 3) % (K + M)])[0]
        a = third.act(third.seq_step(obs_token, prev3).unsqueeze(0)).action_token
        prev3 = a[-1] if a.dim() == 3 else a
    b = B - 1                                                                          # the episode that moves: sample b of the first batch
    pt[:, 0], pm[0] = prompt_tokens[:, b], prompt_masks[b]
    flags = [True] + [False] * (B - 1)
    assert third.seq_history_room() >= K
    third.seq_restart(flags, pt, pm, history=(h_obs[:, b:b + 1].contiguous(), h_act[:K - 1, b:b + 1].contiguous() if K > 1 else None))
    prev3 = prev3.clone()
    prev3[0] = h_act[K - 1, b]                                                         # the moved episode's last action; the others keep their own
    obs_token = third.forward_obs_token(observations[(K + 3) % (K + M)])[0].clone()
    obs_token[0] = first.forward_obs_token(observations[K])[0][b]
    sel = third.act(third.seq_step(obs_token, prev3).unsqueeze(0))
    moved = all(torch.equal(sel.actions[k][0, 0], actions[K][k][0, b]) for k in sel.actions)
    print(f"sample {b} moved into another batch as its sample 0 with {K} steps of history; its next action equals the one it took at home: {moved}")


if __name__ == "__main__":
    main()
