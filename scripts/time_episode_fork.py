"""What a fork costs (`fork_samples`, `seq_fork`) against the only other way to put an in-flight episode into another batch slot, the restart with
a recorded history: VIMA-200M, bf16, Q = 8, 512-token prompts, batch 256, ring on, and Gato at batch 32; one process on one GPU, the compared
routes alternated window by window. The decoder alone: observation and action tokens are prepared.

    (a) fork_samples of n = 1 / 8 / 32 destinations after 8 env steps against restart_samples(history=<those 8 steps>) of the same samples, in
        both splits: one source -> n, and n sources -> n. The same for Gato (seq_fork against seq_restart(history=)) at batch 32, n = 1 / 8.
    (b) group start: restart_samples of 32 samples that share 4 prompts against restarting 4 of them and forking the other 28.
    (c) the K | V copy launch alone (vima_op_episode_fork on a buffer of the episode cache's shape, device events around the call, its small
        table upload included): bytes read + written per second counted from the job table (a source is read once per job of at most 8
        destinations), next to the same traffic counted per pair (2 x), and to the 6.29 TB/s of a float4 copy on this GPU as context.

Times: host clock around a window that starts and ends with a device synchronise; medians, interquartile ranges, every window listed.

    python scripts/time_episode_fork.py [--model 200M] [--batch 256] [--repeats 11] [--warmup 2] [--out profiles/episode_fork_time.txt]
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_episode_prefill import launches, make_policy, summary, timed, tokens  # noqa: E402
from vima_amd import _lib  # noqa: E402
from vima_amd.baselines import build_baseline  # noqa: E402
from vima_testing import synthetic as syn  # noqa: E402

HIST_T = 8
MAX_DST = 8        # kForkMaxDst of vima_amd/csrc/kernels.h


def compare(lines, verdicts, tag, name0, fn0, name1, fn1, args, count=None):
    t = {0: [], 1: []}
    for rep in range(args.warmup + args.repeats):
        for k, fn in ((0, fn0), (1, fn1)):
            ms = timed(fn)
            if rep >= args.warmup:
                t[k].append(ms)
    m0, i0, txt = summary(name0, t[0])
    lines += txt
    m1, i1, txt = summary(name1, t[1])
    lines += txt
    good = m0 - m1 > i0 + i1
    verdicts.append((tag, good))
    extra = f"; launches {count[0]} against {count[1]}" if count else ""
    lines.append(f"  {name0.split(',')[-1].strip()} - {name1.split(',')[-1].strip()} = {m0 - m1:+.3f} ms ({m0 / m1:.2f}x); IQRs {i0:.3f} + {i1:.3f} ms -> the fork "
                 f"{'wins by more than the two spreads' if good else 'does NOT win by more than the two spreads'}{extra}")


def spread(B, n):
    return [b for b in range(B) if b % (B // n) == 0 and b // (B // n) < n]


def i32(xs):
    return (ctypes.c_int32 * max(len(xs), 1))(*xs)


def copy_alone(lines, policy, NL, B, L, N, args):
    cache = torch.randn(NL, B, L, N, device="cuda:0").bfloat16()
    row = N * 2
    lines.append(f"(c) the K | V copy launch alone on a bf16 buffer [{NL}][{B}][{L}][{N}] ({cache.numel() * 2 / 2 ** 30:.2f} GiB); rows of {row} B per layer")
    for name, groups in (("1 -> 1, 71 rows", [(3, [0], 71)]), ("1 -> 8, 71 rows", [(3, spread(B, 8), 71)]), ("1 -> 32, 71 rows", [(3, spread(B, 32), 71)]),
                         ("1 -> 8, 512 rows", [(3, spread(B, 8), L)]), ("1 -> 32, 512 rows", [(3, spread(B, 32), L)]),
                         ("32 -> 32, 512 rows", [(d + 1, [d], L) for d in spread(B, 32)])):
        gs, gp, ds, rp, rg, moved, pairwise = [], [0], [], [0], [], 0, 0
        for s, d, rows in groups:
            gs.append(s); ds += d; gp.append(len(ds)); rg += [0, rows]; rp.append(len(rg) // 2)
            moved += NL * rows * row * (-(-len(d) // MAX_DST) + len(d))
            pairwise += NL * rows * row * 2 * len(d)
        a = [i32(x) for x in (gs, gp, ds, rp, rg)]

        def run():
            _lib.check(policy._lib.vima_op_episode_fork(policy._handle, ctypes.c_void_p(cache.data_ptr()), 2, NL, B, L, N, *a, len(gs), policy._stream()))

        us = []
        for rep in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); run(); e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                us.append(e0.elapsed_time(e1) * 1e3)
        med, iqr, txt = summary(name, us, "us")
        lines += txt
        lines.append(f"  job table: {moved / 1e6:.1f} MB read + written -> {moved / med / 1e6:.2f} TB/s ({100 * moved / med / 1e6 / 6.29:.0f} % of the 6.29 TB/s float4 copy); "
                     f"counted per pair the same copy would move {pairwise / 1e6:.1f} MB ({pairwise / moved:.2f}x)")
    del cache
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="200M")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_episode_fork.py measures on the GPU: no device found")
    dev, B = "cuda:0", args.batch
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = make_policy(cfg, dev)
    lines = [f"scripts/time_episode_fork.py: VIMA-{args.model} bf16, Q = 8, 512-token prompts, n_positions {cfg.n_positions}, batch {B}, decode_ring 1; {args.repeats} timed "
             f"windows per route after {args.warmup} warm-up windows, routes alternated in one process; the decoder alone (tokens prepared)",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "time: host clock around a window with a device synchronise at both ends; ms per window; spread: interquartile range", ""]
    verdicts = []
    pt, pm = policy.forward_prompt_assembly(syn.to_device(syn.make_prompt(B, n_segments=32, words_per_segment=8, q_per_view=4, seed=1), dev))
    pt, pm = pt.contiguous().clone(), pm.clone()
    otok, omask, atok = tokens(policy, B, HIST_T + 1, dev)
    policy.set_option("decode_ring", 1)
    policy.forward_step(otok[0], omask[0], None, pt, pm, step=0)
    for t in range(1, HIST_T):
        policy.forward_step(otok[t], omask[t], atok[t - 1], pt, pm, step=t)
    assert policy.history_room() >= HIST_T
    E, NL = cfg.embed_dim, cfg.xf_n_layers
    per_dst = (HIST_T * 9 - 1 + pt.shape[0]) * NL * 2 * E * 2
    lines.append(f"(a) at batch step {HIST_T}: fork_samples of n destinations against restart_samples(history = the source's {HIST_T} steps) of the same samples; "
                 f"a destination is ({HIST_T * 9 - 1} + {pt.shape[0]}) rows x {NL} layers x {2 * E * 2} B = {per_dst / 1e6:.1f} MB (derived)")
    for n in (1, 8, 32):
        who = spread(B, n)
        for split, srcs in (("one source", [3] * n), ("n sources", [d + 1 for d in who])):
            source = list(range(B))
            for d, s in zip(who, srcs):
                source[d] = s
            flags = [b in who for b in range(B)]
            hist = (otok[:HIST_T, srcs].contiguous(), omask[:HIST_T, srcs].contiguous(), atok[:HIST_T - 1, srcs].contiguous())
            policy.fork_samples(source, pt, pm)       # the prompt columns of the destinations are their sources' from here on, for both routes

            def install():
                policy.restart_samples(flags, pt, pm, history=hist)

            def fork():
                policy.fork_samples(source, pt, pm)

            count = (launches(policy, install), launches(policy, fork))
            compare(lines, verdicts, f"(a) n {n} {split}", f"n = {n:2d} {split}, history", install, f"n = {n:2d} {split}, fork", fork, args, count)
    lines.append("")
    # ---- (b) group start
    who = spread(B, 32)
    heads = who[::8]
    source = list(range(B))
    for i, d in enumerate(who):
        source[d] = heads[i // 8]
        pt[:, d], pm[d] = pt[:, heads[i // 8]], pm[heads[i // 8]]
    f32, f4 = [b in who for b in range(B)], [b in heads for b in range(B)]
    lines.append("(b) group start: 32 samples that share 4 prompts -- restart_samples of the 32 against restart_samples of 4 and fork_samples of the other 28")

    def restart32():
        policy.restart_samples(f32, pt, pm)

    def restart4_fork28():
        policy.restart_samples(f4, pt, pm)
        policy.fork_samples(source, pt, pm)

    count = (launches(policy, restart32), launches(policy, restart4_fork28))
    compare(lines, verdicts, "(b) group start", "32 samples, restart 32", restart32, "32 samples, restart 4 + fork 28", restart4_fork28, args, count)
    lines.append("")
    copy_alone(lines, policy, NL, B, cfg.n_positions, 2 * E, args)
    del policy
    torch.cuda.empty_cache()
    # ---- Gato, batch 32
    Bg, Lp = 32, 64
    gcfg = syn.BaselineConfig("gato", 768, 12, 12, vocab_size=16, n_positions=512)
    gato = build_baseline(gcfg, precision="bf16", device=dev)
    gato.load_state_dict(syn.make_baseline_state_dict(gcfg, 0), strict=True)
    gato.set_option("seq_ring", 1)
    Qg = gato._obj_xf_num_queries
    g = torch.Generator().manual_seed(5)
    gp_, gm = torch.randn(Lp, Bg, 768, generator=g).to(dev), torch.ones(Bg, Lp, dtype=torch.bool, device=dev)
    go, ga = torch.randn(HIST_T, Bg, Qg, 768, generator=g).to(dev), torch.randn(HIST_T, Bg, 768, generator=g).to(dev)
    gato.seq_prefill(gp_, gm)
    for t in range(HIST_T):
        gato.seq_step(go[t], ga[t - 1] if t else None)
    lines.append(f"(a') Gato (embed 768, 12 layers), bf16, batch {Bg}, Q = {Qg}, {Lp}-token prompts, seq_ring 1, at batch step {HIST_T}: seq_fork of n destinations against "
                 f"seq_restart(history = the source's {HIST_T} steps)")
    for n in (1, 8):
        who = spread(Bg, n)
        srcs = [d + 1 for d in who]
        source = list(range(Bg))
        for d, s in zip(who, srcs):
            source[d] = s
            gp_[:, d] = gp_[:, s]
        flags = [b in who for b in range(Bg)]
        hist = (go[:, srcs].contiguous(), ga[:HIST_T - 1, srcs].contiguous())

        def ginstall():
            gato.seq_restart(flags, gp_, gm, history=hist)

        def gfork():
            gato.seq_fork(source)

        count = (launches(gato, ginstall), launches(gato, gfork))
        compare(lines, verdicts, f"(a') gato n {n}", f"n = {n:2d} n sources, history", ginstall, f"n = {n:2d} n sources, fork", gfork, args, count)
    lines.append("")
    lines.append("the fork beats the history route by more than the two spreads: " + "; ".join(f"{k}: {'yes' if v else 'NO'}" for k, v in verdicts))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
