"""Cold-step time of the VIMA-200M policy forward (xattn_n_positions 512, 512-token prompt, Q = 8, bench.py's seeds) in the
precisions fp32, bf16x3 and bf16, alternating step by step on one process and one GPU, at batch 64 and 256. Per precision:
median of the timed steps (device events around each step, after a warm-up, default options), the library profiler's
per-class split of one single-stream step (GEMM / attention / other) and the all-GEMM throughput, against the bf16 matrix
peak for bf16 and against that peak / 3 for bf16x3 (three bf16 MFMAs per product).

    python scripts/time_precision.py [--batches 64 256] [--steps 7] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vima_testing import synthetic as syn  # noqa: E402
from vima_amd.policy import VIMAPolicy  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0   # MI355X dense bf16 matrix peak
PRECISIONS = ("fp32", "bf16x3", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = syn.config("200M", xattn_n_positions=512)
    sd = syn.make_state_dict(cfg, 0)
    words, qv, n_seg = 8, 4, 32                     # 32 x [8 words + 1 image -> 8 object tokens] = 512 prompt tokens
    pols = {}
    for prec in PRECISIONS:
        p = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=512, precision=prec, device=dev)
        p.load_state_dict(sd, strict=True)
        pols[prec] = p
    results = []
    for B in args.batches:
        prompts = syn.to_device(syn.make_prompt(B, n_segments=n_seg, words_per_segment=words, q_per_view=qv, seed=1236), dev)
        obs = syn.to_device(syn.make_obs(1, B, qv, seed=1336), dev)

        def step(pol):
            ptok, pmask = pol.forward_prompt_assembly(prompts)
            otok, omask = pol.forward_obs_token(obs)
            return pol.action_logits(pol.forward(otok, omask, None, ptok, pmask)[-1])

        logits = {}
        for prec in PRECISIONS:
            for _ in range(args.warmup):
                logits[prec] = step(pols[prec]).float().cpu()
        torch.cuda.synchronize()
        times = {prec: [] for prec in PRECISIONS}
        for _ in range(args.steps):
            for prec in PRECISIONS:             # alternating: clock / thermal drift hits every precision alike
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(pols[prec])
                b.record()
                b.synchronize()
                times[prec].append(a.elapsed_time(b))
        for prec in PRECISIONS:
            # per-class split on ONE stream (as bench.py does): the profiler's events bracket each launch on its stream, so with the
            # two T5 / ViT streams overlapping a launch's span would also count the other stream's work
            pol = pols[prec]
            pol.set_option("dual_stream", 0)
            step(pol)
            torch.cuda.synchronize()
            pol.prof_enable(True)
            step(pol)
            torch.cuda.synchronize()
            gk = pol.prof_read_gemm_kernels()
            prof = pol.prof_read_ex()
            pol.prof_enable(False)
            pol.set_option("dual_stream", 1)   # the default, under which the steps above were timed
            gemm_ms = prof["gemm"]["ms"] + prof["gemm_residual"]["ms"]
            gemm_fl = prof["gemm"]["flops"] + prof["gemm_residual"]["flops"]
            tf = gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
            peak = {"bf16": BF16_PEAK_TFLOPS, "bf16x3": BF16_PEAK_TFLOPS / 3}.get(prec)
            rec = {"batch": B, "precision": prec, "median_ms": round(statistics.median(times[prec]), 3),
                   "steps_ms": [round(t, 3) for t in times[prec]],
                   "split_ms": {"gemm": round(gemm_ms, 3), "attention": round(prof["attention"]["ms"], 3), "other": round(prof["other"]["ms"], 3)},
                   "gemm_tflops": round(tf, 1), "gemm_frac_of_peak": round(tf / peak, 3) if peak else None,
                   "gemm_kernels": sorted(gk),
                   "max_abs_logit_diff_vs_fp32": round((logits[prec] - logits["fp32"]).abs().max().item(), 8),
                   "max_abs_logit": round(logits["fp32"].abs().max().item(), 6)}
            results.append(rec)
            print(json.dumps(rec), flush=True)
        med = {r["precision"]: r["median_ms"] for r in results if r["batch"] == B}
        print(f"batch {B}: fp32 {med['fp32']:.2f} ms, bf16x3 {med['bf16x3']:.2f} ms, bf16 {med['bf16']:.2f} ms; "
              f"fp32 / bf16x3 = {med['fp32'] / med['bf16x3']:.2f}x", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
