"""What a snapshot + restore costs (`snapshot_samples` + `restore_samples`, `seq_snapshot` + `seq_restore`) against the route it replaces, the
restart with a recorded history: VIMA-200M, bf16, Q = 8, 512-token prompts, batch 256, ring on, and Gato at batch 32; one process on one GPU, the
compared routes alternated window by window. The decoder alone: observation and action tokens are prepared.

    (a) snapshot_samples + restore_samples of n = 1 / 8 / 32 samples with 8 env steps behind them (into the slots they came from) against
        restart_samples(history=<those 8 steps>) of the same samples, with and without the prompt block; restore_samples alone is listed too
        (a tree search snapshots a node once and backtracks to it many times). The same for Gato at batch 32, n = 1 / 8.
    (b) the pack and unpack launches alone (vima_op_episode_pack / _unpack on a buffer of the episode cache's shape, device events around the
        call, its small table upload included): bytes read + written per second, next to the fork kernel's 5.0 - 5.2 TB/s
        (profiles/episode_fork_time.txt) and to the 6.29 TB/s of a float4 copy on this GPU as context.

Times: host clock around a window that starts and ends with a device synchronise; medians, interquartile ranges, every window listed. Nothing is
gated: where the new route is not faster, the verdict line says so.

    python scripts/time_episode_snapshot.py [--model 200M] [--batch 256] [--repeats 11] [--warmup 2] [--out profiles/episode_snapshot_time.txt]
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
from time_episode_fork import i32, spread  # noqa: E402
from vima_amd import _lib  # noqa: E402
from vima_amd.baselines import build_baseline  # noqa: E402
from vima_testing import synthetic as syn  # noqa: E402

HIST_T = 8


def compare(lines, verdicts, tag, routes, args, counts):
    """routes: [(name, fn)], the first is the history route; alternated window by window"""
    t = [[] for _ in routes]
    for rep in range(args.warmup + args.repeats):
        for k, (_, fn) in enumerate(routes):
            ms = timed(fn)
            if rep >= args.warmup:
                t[k].append(ms)
    stats = []
    for (name, _), v in zip(routes, t):
        m, i, txt = summary(name, v)
        lines += txt
        stats.append((m, i))
    (m0, i0), (m1, i1) = stats[0], stats[1]
    good = m0 - m1 > i0 + i1
    verdicts.append((tag, good))
    lines.append(f"  history - (snapshot + restore) = {m0 - m1:+.3f} ms ({m0 / m1:.2f}x); IQRs {i0:.3f} + {i1:.3f} ms -> the new route "
                 f"{'wins by more than the two spreads' if good else 'does NOT win by more than the two spreads'}; launches per call: "
                 + ", ".join(f"{n.split(',')[-1].strip()} {c}" for (n, _), c in zip(routes, counts)))


def kernels_alone(lines, policy, NL, B, L, N, args):
    cache = torch.randn(NL, B, L, N, device="cuda:0").bfloat16()
    row = N * 2
    lines.append(f"(b) the pack / unpack launch alone on a bf16 buffer [{NL}][{B}][{L}][{N}] ({cache.numel() * 2 / 2 ** 30:.2f} GiB); rows of {row} B per layer; "
                 "a row is read once and written once")
    wrap = [(L - 40 + k) % L for k in range(71)]
    for name, rowmap, n_map, samples, D in (("1 sample, 71 mapped rows", wrap, 71, [3], 0), ("8 samples, 71 mapped rows", wrap, 71, spread(B, 8), 0),
                                             ("32 samples, 71 mapped rows", wrap, 71, spread(B, 32), 0),
                                             ("8 samples, 512 rows", None, L, spread(B, 8), 0), ("32 samples, 512 rows", None, L, spread(B, 32), 0),
                                             ("32 samples, 512 rows, head-major 64", None, L, spread(B, 32), 64)):
        pays = [torch.empty(NL, n_map, N, dtype=torch.bfloat16, device="cuda:0") for _ in samples]
        ptrs = (ctypes.c_void_p * len(pays))(*[p.data_ptr() for p in pays])
        a = (i32(rowmap) if rowmap is not None else None, n_map, i32(samples), i32([n_map] * len(samples)), ctypes.cast(ptrs, ctypes.c_void_p), len(samples))
        moved = 2 * NL * n_map * row * len(samples)
        for what in ("pack", "unpack"):
            fn = getattr(policy._lib, "vima_op_episode_" + what)

            def run():
                _lib.check(fn(policy._handle, ctypes.c_void_p(cache.data_ptr()), 2, NL, B, L, N, D, *a, policy._stream()))

            us = []
            for rep in range(args.warmup + args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(); run(); e1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    us.append(e0.elapsed_time(e1) * 1e3)
            med, iqr, txt = summary(f"{what}, {name}", us, "us")
            lines += txt
            lines.append(f"  {moved / 1e6:.1f} MB read + written -> {moved / med / 1e6:.2f} TB/s ({100 * moved / med / 1e6 / 6.29:.0f} % of the 6.29 TB/s float4 copy)")
        del pays
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
        raise SystemExit("time_episode_snapshot.py measures on the GPU: no device found")
    dev, B = "cuda:0", args.batch
    cfg = syn.config(args.model, xattn_n_positions=512)
    policy = make_policy(cfg, dev)
    lines = [f"scripts/time_episode_snapshot.py: VIMA-{args.model} bf16, Q = 8, 512-token prompts, n_positions {cfg.n_positions}, batch {B}, decode_ring 1; {args.repeats} "
             f"timed windows per route after {args.warmup} warm-up windows, routes alternated in one process; the decoder alone (tokens prepared)",
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
    lines.append(f"(a) at batch step {HIST_T}: snapshot_samples + restore_samples of n samples (into their own slots) against restart_samples(history = their "
                 f"{HIST_T} steps) of the same samples")
    for n in (1, 8, 32):
        who = spread(B, n)
        flags = [b in who for b in range(B)]
        hist = (otok[:HIST_T, who].contiguous(), omask[:HIST_T, who].contiguous(), atok[:HIST_T - 1, who].contiguous())
        for with_prompt in (True, False):
            held = policy.snapshot_samples(who, pt, pm, with_prompt=with_prompt)
            lines.append(f"  n = {n}, {'with' if with_prompt else 'without'} the prompt block: {held[0].nbytes / 1e6:.2f} MB per snapshot "
                         f"({HIST_T * 9 - 1}{' + ' + str(pt.shape[0]) if with_prompt else ''} rows x {NL} layers x {2 * E * 2} B + mask and header)")

            def install():
                policy.restart_samples(flags, pt, pm, history=hist)

            def both():
                policy.restore_samples(who, policy.snapshot_samples(who, pt, pm, with_prompt=with_prompt), pt, pm)

            def restore():
                policy.restore_samples(who, held, pt, pm)

            def snapshot():
                policy.snapshot_samples(who, pt, pm, with_prompt=with_prompt)

            tagp = "prompt" if with_prompt else "no prompt"
            counts = (launches(policy, install), f"{launches(policy, snapshot)} + {launches(policy, restore)}", launches(policy, restore))
            compare(lines, verdicts, f"(a) n {n} {tagp}",
                    [(f"n = {n:2d} {tagp}, history", install), (f"n = {n:2d} {tagp}, snapshot + restore", both), (f"n = {n:2d} {tagp}, restore alone", restore)],
                    args, counts)
            del held
    lines.append("")
    kernels_alone(lines, policy, NL, B, cfg.n_positions, 2 * E, args)
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
    lines.append(f"(a') Gato (embed 768, 12 layers), bf16, batch {Bg}, Q = {Qg}, {Lp}-token prompts, seq_ring 1, at batch step {HIST_T}: seq_snapshot + seq_restore of n "
                 f"samples against seq_restart(history = their {HIST_T} steps)")
    for n in (1, 8):
        who = spread(Bg, n)
        flags = [b in who for b in range(Bg)]
        hist = (go[:, who].contiguous(), ga[:HIST_T - 1, who].contiguous())
        held = gato.seq_snapshot(who)
        lines.append(f"  n = {n}: {held[0].nbytes / 1e6:.2f} MB per snapshot")

        def ginstall():
            gato.seq_restart(flags, gp_, gm, history=hist)

        def gboth():
            gato.seq_restore(who, gato.seq_snapshot(who))

        def grestore():
            gato.seq_restore(who, held)

        counts = (launches(gato, ginstall), f"{launches(gato, lambda: gato.seq_snapshot(who))} + {launches(gato, grestore)}", launches(gato, grestore))
        compare(lines, verdicts, f"(a') gato n {n}",
                [(f"n = {n:2d}, history", ginstall), (f"n = {n:2d}, snapshot + restore", gboth), (f"n = {n:2d}, restore alone", grestore)], args, counts)
    lines.append("")
    lines.append("snapshot + restore beats the history route by more than the two spreads: " + "; ".join(f"{k}: {'yes' if v else 'NO'}" for k, v in verdicts))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
