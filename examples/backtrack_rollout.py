"""Episode snapshots on the MI355X path: a small depth-first action search that holds more tree nodes than the batch has slots, and backtracks
without replaying anything. One episode runs in slot 0 of a batch of S slots. At every node

    1. `snapshot_samples([0], ..., with_prompt=False)` saves the node -- the episode's K/V rows in time order, mask, counter and flag; a few MB
       that stay valid however far the ring advances (the prompt-less form: the whole search lives inside one prompt group),
    2. `act(predicted, sample=True, n_samples=S)` draws S candidate actions from ONE pass of the action head,
    3. `restore_samples(range(S), [node] * S, ...)` puts the node into all S slots (one snapshot, S slots, three launches) and the next
       `forward_step` feeds slot s candidate s: S one-step continuations side by side,
    4. a toy scorer (the confidence of the branch's next prediction) ranks the children. The best child becomes the new node -- unless it scores
       below the best score the search has seen higher up, in which case the search BACKTRACKS (once per node): the parent's snapshot, taken
       several batch steps ago, is restored and its next-best candidate is taken instead.

At the end the episode is moved into a second policy with another batch size (`.cpu()`, `state_dict()`, `from_state_dict()`, `restore_samples`):
parking an episode, or handing it to another rank.

    python examples/backtrack_rollout.py [--model 20M] [--samples 4] [--depth 12]

Synthetic inputs stand in for the simulator, as in examples/branch_rollout.py (a real search would snapshot the simulator state per node too).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vima_testing import synthetic as syn                      # noqa: E402
from vima_amd.episodes import EpisodeSnapshot              # noqa: E402
from vima_amd.policy import VIMAPolicy                    # noqa: E402


def make(cfg, dev):
    policy = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision="bf16", device=dev)
    policy.load_state_dict(syn.make_state_dict(cfg, 0), strict=True)   # create_policy_from_ckpt(path, dev) with a real checkpoint
    policy.set_option("decode_ring", 1)
    return policy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="20M")
    ap.add_argument("--samples", type=int, default=4, help="S: candidates per node = slots of the batch")
    ap.add_argument("--depth", type=int, default=12, help="env steps of the episode the search commits to")
    args = ap.parse_args()
    dev, S = "cuda:0", args.samples
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = make(cfg, dev)
    one = syn.make_prompt(1, n_segments=32, words_per_segment=8, q_per_view=4, seed=1)
    pt, pm = policy.forward_prompt_assembly(syn.to_device(one, dev))
    pt, pm = pt.expand(-1, S, -1).contiguous(), pm.expand(S, -1).contiguous()      # one prompt group: every slot holds the same prompt
    observations = [policy.forward_obs_token(syn.to_device(syn.make_obs(1, S, 4, seed=100 + t), dev)) for t in range(16)]

    def step(t, prev):
        """one batch step; the slots' observations stand in for the simulator's answer to each candidate"""
        o, m = observations[t % len(observations)]
        predicted = policy.forward_step(o, m, prev, pt, pm, step=t)
        mode = policy.act(predicted.unsqueeze(0))
        return predicted, sum(mode.log_prob.values())[0]                               # [S, E], [S]

    t = 0
    predicted, _ = step(t, None)
    t += 1
    stack = []                        # the search path: (snapshot of the node, candidate action tokens [S, E], scores [S] or None, tried)
    depth = nodes = backtracks = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while depth < args.depth:
        (node,) = policy.snapshot_samples([0], pt, pm, with_prompt=False)               # 1.
        cand = policy.act(predicted[:1].unsqueeze(0), sample=True, temperature=0.7, top_k=10, top_p=0.9, n_samples=S).action_token[0, 0]   # 2. [S, E]
        stack.append([node, cand, None, set()])
        nodes += 1
        while True:
            node, cand, scores, tried = stack[-1]
            if policy.steps_left().min().item() == 0 or node.steps > policy.history_room():
                raise SystemExit("the ring is shorter than the search path: raise n_positions")
            policy.restore_samples(list(range(S)), [node] * S, pt, pm)                  # 3. the node in every slot
            predicted, s = step(t, cand)
            t += 1
            if scores is None:
                stack[-1][2] = scores = s.clone()
            if len(stack) == 1 and len(tried) == S:
                tried.clear()                                                           # the root has nowhere to backtrack to
            order = [i for i in scores.argsort(descending=True).tolist() if i not in tried]
            parent_best = max((float(f[2].max()) for f in stack[:-1]), default=float("-inf"))
            if order and (len(stack) == 1 or float(scores[order[0]]) >= parent_best or len(stack[-2][3]) >= 2):
                pick = order[0]
                tried.add(pick)
                break
            stack.pop()                                                                 # 4. backtrack: the parent node, another candidate
            depth -= 1
            backtracks += 1
        # the chosen child continues in slot 0: it already sits in slot `pick` with its step taken
        (child,) = policy.snapshot_samples([pick], pt, pm, with_prompt=False)
        policy.restore_samples([0], [child], pt, pm)
        predicted = predicted[pick:pick + 1].expand(S, -1).contiguous()
        depth += 1
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print(f"{args.model}: committed {depth} env steps after {t} batch steps of {S} slots; {nodes} nodes held as snapshots of up to "
          f"{max(f[0].nbytes for f in stack) / 1e6:.2f} MB, {backtracks} backtracks; {ms / t:.2f} ms per batch step including snapshots and restores")
    # ---- move the episode into a policy of another batch size, through the host
    (final,) = policy.snapshot_samples([0], pt, pm)                                     # with the prompt: it leaves its prompt group
    parcel = final.cpu().state_dict()                                                   # tensors and ints: torch.save(parcel, path) works
    other = make(cfg, dev)
    B2 = 2
    qt, qm = other.forward_prompt_assembly(syn.to_device(syn.make_prompt(B2, n_segments=32, words_per_segment=8, q_per_view=4, seed=9), dev))
    qt, qm = qt.contiguous().clone(), qm.clone()
    o2 = [other.forward_obs_token(syn.to_device(syn.make_obs(1, B2, 4, seed=300 + k), dev)) for k in range(final.steps + 1)]
    prev = None
    for k in range(final.steps):                                                        # the other batch has to be that far into its own rollout
        prev = other.act(other.forward_step(*o2[k], prev, qt, qm, step=k).unsqueeze(0)).action_token[0].clone()
    qt, qm = other.restore_samples([1], [EpisodeSnapshot.from_state_dict(parcel)], qt, qm)
    out = other.forward_step(*o2[final.steps], prev, qt, qm, step=final.steps)
    print(f"moved: a snapshot of {final.steps} steps, {final.nbytes / 1e6:.2f} MB, restored into slot 1 of a batch of {B2}; steps_left there "
          f"{other.steps_left().tolist()}, next prediction finite: {bool(torch.isfinite(out[1]).all())}")


if __name__ == "__main__":
    main()
