"""Wall time of one env step of a decoder-only baseline policy (VIMAGPTPolicy / VIMAGatoPolicy at the `bench.py --policy gpt|gato`
shape: embed_dim 768, 11 layers, 12 heads, batch 256, prompt of 8 x (8 words + 1 frame pair)) through the two decoder routes,
alternated inside one process on one GPU:

    step     seq_step (vima_seq_decode_step): only the rows of env step t against the episode K/V cache
    refeed   forward (vima_seq_decode) on [prompt | sep | o, a, ..., o_t]: the whole history, the only route before seq_step existed

Timed at env steps 0, 1, 4 and the last one that fits into n_positions. Every timed episode steps from a fresh `seq_prefill` to the last
step; at each measured step the `seq_step` call is timed (host clock, a device synchronise at both ends) and right after it the
`forward` call on the same history. The decoder inputs are random token tensors (the encoders in front are the same for both routes
and are not timed). The one-off `seq_prefill` is timed on its own. Per route and step: median, minimum, maximum and interquartile range
of the timed episodes, and the library's launches from the handle's profiler (one extra, untimed episode).

    python scripts/time_seq_step.py [--policies gpt gato] [--batch 256] [--repeats 9] [--warmup 2] [--out profiles/seq_step_time.txt]
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def episode(pol, ptok, pmask, otok, atok, marks, prof=None):
    """One episode up to the last step; returns {"prefill": ms, ("step", t): ms, ("refeed", t): ms} for t in marks and the worst
    |seq_step - forward| seen at the marks. prof: dict filled with the library's launches of every timed call instead of timing."""
    res, worst = {}, 0.0

    def run(key, fn):
        if prof is not None:
            pol.prof_enable(True)
            out = fn()
            torch.cuda.synchronize()
            prof[key] = {k: v["launches"] for k, v in pol.prof_read().items()}
            pol.prof_enable(False)
            return out
        res[key], out = timed(fn)
        return out

    run("prefill", lambda: pol.seq_prefill(ptok, pmask))
    for t in range(otok.shape[0]):
        prev = None if t == 0 else atok[t - 1]
        if t not in marks:
            pol.seq_step(otok[t], prev)
            continue
        got = run(("step", t), lambda: pol.seq_step(otok[t], prev))
        full = run(("refeed", t), lambda: pol.forward(otok[:t + 1], atok[:t] if t else None, ptok, pmask))
        worst = max(worst, (got - full[t]).abs().max().item())
    return res, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", nargs="+", default=["gpt", "gato"], choices=["gpt", "gato"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--opt", action="append", default=[], help="library option key=value (vima_set_option), repeatable")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seq_step.py measures on the GPU: no device found")
    dev = "cuda:0"
    B, E = args.batch, 768
    lines = [f"scripts/time_seq_step.py: decoder-only baselines at the bench.py --policy shape (embed_dim 768, 11 layers, 12 heads), {args.precision}, "
             f"batch {B}; {args.repeats} timed episodes after {args.warmup} warm-up episodes; in every episode the two routes alternate at each "
             "measured step (seq_step, then forward on the same history)" + (f"; options {args.opt}" if args.opt else ""),
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "time: host clock around ONE call with a device synchronise at both ends, ms; spread: interquartile range of the timed episodes",
             "rows: sequence rows per sample the call pushes through the 11 blocks; launches: the library's own (vima_prof_read), gemm / attention / other", ""]
    for kind in args.policies:
        cfg = syn.BaselineConfig(kind, E, 11, 12)
        pol = build_baseline(cfg, precision=args.precision, device=dev)
        pol.load_state_dict(syn.make_baseline_state_dict(cfg, 0), strict=True)
        for kv in args.opt:
            k, v = kv.split("=")
            pol.set_option(k, int(v))
        Q = cfg.obs_tokens
        Lp = args.segments * (args.words + Q)
        T = 1 + (cfg.n_positions - (Lp + 1 + Q)) // (Q + 1)          # env steps that fit: Lp + 1 + T (Q + 1) - 1 <= n_positions
        marks = sorted({t for t in (0, 1, 4, T - 1) if t < T})
        g = torch.Generator().manual_seed(1)
        ptok = torch.randn(Lp, B, E, generator=g).to(dev)
        pmask = torch.ones(B, Lp, dtype=torch.bool, device=dev)
        otok = torch.randn(T, B, Q, E, generator=g).to(dev)
        atok = torch.randn(T - 1, B, E, generator=g).to(dev)
        worst = 0.0
        for _ in range(args.warmup):
            worst = max(worst, episode(pol, ptok, pmask, otok, atok, marks)[1])
        runs = [episode(pol, ptok, pmask, otok, atok, marks)[0] for _ in range(args.repeats)]
        prof = {}
        episode(pol, ptok, pmask, otok, atok, marks, prof)
        assert pol.steps_left().tolist() == [0] * B
        lines.append(f"{kind}: prompt {Lp} tokens, {Q} observation token(s) per step, n_positions {cfg.n_positions} -> {T} env steps per episode; "
                     f"max |seq_step - forward| at the measured steps {worst:.3e}")

        def row(label, key, rows):
            v = [r[key] for r in runs]
            q1, q3 = quartiles(v)
            n = prof[key]
            lines.append(f"  {label:<16} rows {rows:>4}  median {statistics.median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  IQR {q3 - q1:6.3f} ms   "
                         f"launches {sum(n.values()):4d} (gemm {n['gemm']}, attention {n['attention']}, other {n['other']})")
            return statistics.median(v), q3 - q1

        row("seq_prefill", "prefill", Lp + 1)
        for t in marks:
            ms_s, iqr_s = row(f"step {t} seq_step", ("step", t), Q + (1 if t else 0))
            ms_f, iqr_f = row(f"step {t} refeed", ("refeed", t), Lp + 1 + (t + 1) * (Q + 1) - 1)
            faster = ms_s + max(iqr_s, iqr_f) < ms_f
            lines.append(f"    -> refeed / seq_step = {ms_f / ms_s:6.2f}x ({'seq_step faster beyond the spread' if faster else 'seq_step NOT faster beyond the spread'})")
        lines.append("")
        del pol
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
