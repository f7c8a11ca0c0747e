#!/usr/bin/env python
"""Bit-for-bit equivalence of two builds of libvima_hip.so over the encoder stacks of the cold step (T5 layer forms, ViT block forms, the
three fp8 calibrators, the baselines' ViT): profiles/stage_fold_equivalence.txt is this script's output.

    python scripts/stage_fold_equivalence.py PARENT_LIB NEW_LIB [--only SUBSTRING] > profiles/stage_fold_equivalence.txt

Every case runs in a fresh child process per library (VIMA_HIP_LIB), one process at a time, each under its own time limit; the script stops
at the first child that fails, times out or differs. Per case the two libraries must agree on: the SHA-256 of every output tensor's bytes,
the GEMM launch log (kernel, M, N, K in launch order), the per-class launch counts / FLOPs / bytes and, in fp8 cases, the scale vectors
of the three calibrated groups. The `episodes` group (scripts/episode_entry_cases.py; --only episodes) adds host values (history_room, steps_left,
graph_stats) and, for every refused call, its return code and vima_last_error() text. The kernels are deterministic (amax is a max), so a difference is a bug, not noise."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
RAGGED = [[0, 1, 0, 0], [0, 0, 1, 0, 1, 0, 0], [0, 0, 0]]


class Rec:
    """What one child reports: output hashes, launch logs, scales and the facts that show a branch was engaged."""

    def __init__(self, pol):
        self.pol, self.out = pol, {"sha256": {}, "gemm_log": [], "classes": {}, "scales": {}, "values": {}, "refusals": [], "engaged": {}}
        pol.prof_enable(True)

    def tensor(self, name, t):
        import torch
        torch.cuda.synchronize()
        t = t.detach().contiguous().cpu()
        self.out["sha256"][name] = hashlib.sha256(t.view(torch.uint8).numpy().tobytes() if t.dtype != torch.bool else t.numpy().tobytes()).hexdigest()

    def step(self, name):
        """Close one profiled call: its GEMM launch log and per-class counts."""
        import torch
        torch.cuda.synchronize()
        log = [[g["kernel"], g["M"], g["N"], g["K"]] for g in self.pol.prof_read_gemm_launches()]
        self.out["gemm_log"].append([name, log])
        self.out["classes"][name] = {k: [v["launches"], v["flops"], v["bytes"]] for k, v in self.pol.prof_read_ex().items()}
        self.out["engaged"][name + ": fp8 GEMM launches"] = sum(1 for g in log if g[0].endswith(", true>"))
        self.out["engaged"][name + ": GEMM row counts"] = sorted({g[1] for g in log})

    def scales(self, name):
        self.out["scales"][name] = {g: (None if s is None else [float.hex(float(v)) for v in s.flatten()])
                                    for g in ("t5", "vit", "kv") for s in [self.pol.fp8_act_scales(g)]}


def vima(prec="bf16", model="2M", seed=3, npos=256, **opts):
    from tests.gpu_common import loaded_policy
    from vima_testing import synthetic as syn
    cfg = syn.config(model, xattn_n_positions=npos)
    pol = loaded_policy(cfg, syn.make_state_dict(cfg, seed, head_gain=0.5), prec, **opts)
    rec = Rec(pol)
    rec.out["engaged"]["options"] = dict(opts, precision=prec)
    return pol, rec


def t5_case(B, L, prec="bf16", **opts):
    import torch
    pol, rec = vima(prec, **opts)
    g = torch.Generator().manual_seed(B * L)
    x = torch.randn(B, L, 768, generator=g).to(DEV)
    mask = torch.rand(B, L, generator=g) > 0.1
    mask[:, 0] = True
    rec.tensor("t5_encode", pol.t5_encode(x, mask.to(DEV)))
    rec.step("t5_encode")
    return rec


def assembly_case(prec="bf16", **opts):
    from vima_testing import synthetic as syn
    pol, rec = vima(prec, **opts)
    ptok, pmask = pol.forward_prompt_assembly(syn.to_device(syn.make_prompt(3, layout=RAGGED, q_per_view=2, seed=11), DEV))
    rec.tensor("prompt_tokens", ptok)
    rec.tensor("prompt_masks", pmask)
    rec.step("forward_prompt_assembly")
    return rec


def fp8_t5_case(B, **opts):
    """Calibrating call, then fp8 call (the shape of tests/test_fp8_gpu.py::_case at B = 28)."""
    from vima_testing import synthetic as syn
    pol, rec = vima("fp8", seed=21, npos=512, **opts)
    p = syn.to_device(syn.make_prompt(B, n_segments=64, words_per_segment=4, q_per_view=2, seed=501), DEV)
    for call in ("calibrating", "fp8"):
        ptok, pmask = pol.forward_prompt_assembly(p)
        rec.tensor(call + " prompt_tokens", ptok)
        rec.step(call)
        rec.scales("after " + call)
    return rec


def vit_case(n, qv=4, prec="bf16", obs=False, **opts):
    import torch
    from vima_testing import synthetic as syn
    pol, rec = vima(prec, **opts)
    objs = syn._objects(torch.Generator().manual_seed(n), (n,), qv)
    rec.tensor("obj_encoder", pol.obj_encoder(syn.to_device(objs["cropped_img"], DEV), syn.to_device(objs["bbox"], DEV)))
    rec.step("obj_encoder (%d crops)" % (2 * n * qv))
    if obs:
        ot, om = pol.forward_obs_token(syn.to_device(syn.make_obs(2, 5, 2, seed=7), DEV))
        rec.tensor("obs_token", ot)
        rec.tensor("obs_mask", om)
        rec.step("forward_obs_token")
    return rec


def _logits(pol, ptok, pmask, obs):
    ot, om = pol.forward_obs_token(obs)
    return pol.action_logits(pol.forward(obs_token=ot, obs_mask=om, action_token=None, prompt_token=ptok, prompt_token_mask=pmask)[-1])


def fp8_vit_kv_case():
    """B = 64, Lp = 512, 16 384 prompt crops (tests/test_fp8_gpu.py::test_fp8_vit_and_kv_projection...): the ViT's calibrating and fp8 calls, and the
    prompt K/V calibrator through `forward`: an ineligible call (2 samples), the calibrating call, the fp8 call, fp8_recalibrate, two headrooms."""
    from vima_testing import synthetic as syn
    pol, rec = vima("fp8", seed=22, npos=512, dual_stream=0)
    pol.cache_prompt_kv = False
    prompts, obs = syn.make_prompt(64, n_segments=64, words_per_segment=4, q_per_view=2, seed=601), syn.make_obs(1, 64, 2, seed=602)
    p, o = syn.to_device(prompts, DEV), syn.to_device(obs, DEV)
    p2, o2 = syn.to_device(syn.cut_prompt(prompts, [0, 1]), DEV), syn.to_device(syn.cut_obs(obs, [0, 1]), DEV)

    def call(name, pp, oo):
        ptok, pmask = pol.forward_prompt_assembly(pp)
        rec.tensor(name + " prompt_tokens", ptok)
        rec.tensor(name + " logits", _logits(pol, ptok, pmask, oo))
        rec.step(name)
        rec.scales("after " + name)

    call("ineligible (B = 2)", p2, o2)
    call("calibrating", p, o)
    call("fp8", p, o)
    pol.set_option("fp8_recalibrate", 1)
    rec.scales("after fp8_recalibrate")
    call("recalibrating", p, o)
    for pct in (100, 125):
        pol.set_option("fp8_headroom_pct", pct)
        call("headroom %d calibrating" % pct, p, o)
    return rec


def precision_case(prec):
    """The small default cases in one precision: t5_encode, the direct assembly, the ViT and one whole forward."""
    import torch
    from vima_testing import synthetic as syn
    pol, rec = vima(prec)
    g = torch.Generator().manual_seed(72)
    x, mask = torch.randn(3, 24, 768, generator=g).to(DEV), torch.ones(3, 24, dtype=torch.bool)
    rec.tensor("t5_encode", pol.t5_encode(x, mask.to(DEV)))
    rec.step("t5_encode")
    ptok, pmask = pol.forward_prompt_assembly(syn.to_device(syn.make_prompt(3, layout=RAGGED, q_per_view=2, seed=11), DEV))
    rec.tensor("prompt_tokens", ptok)
    rec.step("forward_prompt_assembly")
    rec.tensor("logits", _logits(pol, ptok, pmask, syn.to_device(syn.make_obs(1, 3, 2, seed=12), DEV)))
    rec.step("forward")
    rec.scales("end")
    return rec


def baseline_case(kind, prec):
    """rgb_vit at the size of tests/test_baselines_gpu.py::test_baseline_matches_oracle_other_shapes: one forward_obs_token and one full forward."""
    from oracle.cases import run_baseline
    from vima_amd.baselines import build_baseline
    from vima_testing import synthetic as syn
    cfg = syn.BaselineConfig(kind, 384, 3, 12, xattn_n_heads=12 if kind == "flamingo" else 0, vocab_size=8)
    pol = build_baseline(cfg, precision=prec, device=DEV)
    pol.load_state_dict(syn.make_baseline_state_dict(cfg, seed=41, head_gain=0.5), strict=True)
    rec = Rec(pol)
    layout = [[0, 1, 0, 0], [0, 0, 1, 0, 1, 0, 0], [0, 0, 0], [1], [0, 1, 1, 0]]
    obs = syn.to_device(syn.make_rgb_obs(2, 5, seed=43), DEV)
    rec.tensor("obs_token", pol.forward_obs_token(obs))
    rec.step("forward_obs_token")
    out = run_baseline(pol, syn.to_device(syn.make_rgb_prompt(5, layout=layout, seed=42), DEV), obs, syn.to_device(syn.make_actions(2, 5, seed=44), DEV))
    for k in ("prompt_tokens", "obs_tokens", "predicted"):
        rec.tensor(k, out[k])
    rec.step("forward")
    return rec


CASES = {   # name -> (time limit of one child in seconds, function)
    "t5 B=3 L=24 default": (120, lambda: t5_case(3, 24)),
    "t5 B=3 L=24 dual_stream=0": (120, lambda: t5_case(3, 24, dual_stream=0)),
    "t5 B=3 L=24 stream_T=0": (120, lambda: t5_case(3, 24, stream_T=0)),
    "t5 B=3 L=24 t5_fuse_rms=0": (120, lambda: t5_case(3, 24, t5_fuse_rms=0)),
    "t5 B=3 L=1100 t5_pad=1 (half 0: 2200 -> 2304 rows)": (180, lambda: t5_case(3, 1100, t5_pad=1)),
    "t5 B=3 L=1100 t5_pad=0": (180, lambda: t5_case(3, 1100, t5_pad=0)),
    "prompt assembly ragged stream_T=1 (direct entry)": (120, lambda: assembly_case(stream_T=1)),
    "prompt assembly ragged stream_T=0": (120, lambda: assembly_case(stream_T=0)),
    "fp8 t5 B=28 L=512 dual_stream=0": (300, lambda: fp8_t5_case(28, dual_stream=0)),
    "fp8 t5 B=56 L=512 two halves": (300, lambda: fp8_t5_case(56)),
    "vit 320 crops default + forward_obs_token": (120, lambda: vit_case(40, obs=True)),
    "vit 320 crops vit_prune_last=0": (120, lambda: vit_case(40, vit_prune_last=0)),
    "vit 320 crops stream_T=0": (120, lambda: vit_case(40, stream_T=0)),
    "vit 2200 crops vit_pad=1 (-> 2304)": (180, lambda: vit_case(275, vit_pad=1)),
    "vit 2200 crops vit_pad=0": (180, lambda: vit_case(275, vit_pad=0)),
    "vit 2200 crops dual_vit_crops=512 (two streams)": (180, lambda: vit_case(275, dual_vit_crops=512)),
    "vit 2200 crops vit_chunk=600 (four chunks)": (180, lambda: vit_case(275, vit_chunk=600)),
    "fp8 vit 16384 crops + prompt K/V calibrator B=64 Lp=512": (420, fp8_vit_kv_case),
    "precision bf16": (120, lambda: precision_case("bf16")),
    "precision fp32": (120, lambda: precision_case("fp32")),
    "precision bf16x3": (120, lambda: precision_case("bf16x3")),
    "precision fp8w": (120, lambda: precision_case("fp8w")),
    "precision fp8 below the 160-tile bar (stays on the fp8w kernels)": (120, lambda: precision_case("fp8")),
}
for _kind in ("gato", "gpt", "flamingo"):
    for _prec in ("bf16", "fp32"):
        CASES["baseline %s %s" % (_kind, _prec)] = (180, lambda k=_kind, p=_prec: baseline_case(k, p))


# the `episodes` group: the episode entry points of the C ABI and their refusals (scripts/episode_entry_cases.py)
from scripts.episode_entry_cases import episode_cases  # noqa: E402
CASES.update(episode_cases(Rec, DEV))


def child(name):
    import torch
    with torch.no_grad():
        rec = CASES[name][1]()
    print("RESULT " + json.dumps(rec.out), flush=True)


def run_child(lib, name):
    env = dict(os.environ, VIMA_HIP_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CASES[name][0])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or len(lines) != 1:
        raise RuntimeError("child failed (exit %d) for %s with %s\n%s" % (r.returncode, name, lib, r.stderr[-2000:]))
    return json.loads(lines[0][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib", nargs="?")
    ap.add_argument("new_lib", nargs="?")
    ap.add_argument("--child")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    print("parent library: %s\nnew library:    %s" % (args.parent_lib, args.new_lib))
    n = 0
    for name in CASES:
        if args.only not in name:
            continue
        try:
            a, b = run_child(args.parent_lib, name), run_child(args.new_lib, name)   # one GPU process at a time
        except (RuntimeError, subprocess.TimeoutExpired) as e:
            print("\n== %s\nSTOPPED: %s" % (name, e), flush=True)
            return 1
        print("\n== %s" % name)
        for k, v in b["engaged"].items():
            print("   engaged  %s: %s" % (k, v))
        same = True
        for part in ("sha256", "gemm_log", "classes", "scales", "values", "refusals"):
            eq = a[part] == b[part]
            same = same and eq
            print("   %-8s %s" % (part, "EQUAL" if eq else "DIFFERENT"))
            if part == "sha256" or not eq:
                for k in (b[part] if isinstance(b[part], dict) else range(len(b[part]))):
                    print("      %s: parent %s | new %s" % (k, a[part][k] if not isinstance(a[part], dict) or k in a[part] else None, b[part][k]))
        for call, cls in b["classes"].items():
            print("   launches %s: %s; GEMM log of %d launches" % (call, {k: v[0] for k, v in cls.items()}, sum(len(l) for nm, l in b["gemm_log"] if nm == call)))
        for k, v in b["values"].items():
            print("   value    %s: %s" % (k, v))
        for r in b["refusals"]:
            print("   refused  %s" % r)
        for call, sc in b["scales"].items():
            print("   scales   %s: %s" % (call, {g: (None if v is None else "%d values, sha256 %s" % (len(v), hashlib.sha256(json.dumps(v).encode()).hexdigest()[:16])) for g, v in sc.items()}))
        sys.stdout.flush()
        if not same:
            print("STOPPED: the libraries differ in this case")
            return 1
        n += 1
    print("\nALL %d CASES EQUAL (output hashes, GEMM launch logs, per-class launch counts / FLOPs / bytes, fp8 scale vectors, host values, refusals)" % n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
