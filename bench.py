"""bench.py -- policy-forward steps/sec of the MI355X-native VIMA policy (BASELINE.json metric).

One step = one COLD batched policy evaluation: raw uint8 crops / bboxes / word ids ->
forward_prompt_assembly (object ViT + T5) -> forward_obs_token (ViT) -> forward (XAttnGPT) -> action head -> [B,700]
logits, on synthetic inputs already resident in HBM. Default workload = BASELINE.json configs[2]:
VIMA-200M, batch 256 per GPU, 512-token prompt (32 x [8 words + 1 image -> 8 object tokens]), 8 object tokens/obs.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (one rank per GPU, RCCL)

Multi-GPU = data parallel, weak scaling: every rank evaluates its own batch of 256 with a full weight replica and the
only collective is one all-gather of the [256,700] logits per step (vima_allgather_logits in the C ABI, RCCL over xGMI).
`python bench.py --gpus N` on its own re-launches itself with N ranks; it exits non-zero when fewer than N GPUs are visible.
Prints ONE JSON line on rank 0. `--dump-outputs DIR` also writes the logits of the last timed step to DIR/logits.npy.

A plain run does what the headline figure needs and nothing else: set-up, warm-up, the timed steps, the dump, the line. `--full` adds,
after the timed steps and outside them, everything else this file measures: the WARM / incremental / batch-1 / batch-32 steps and the other
BASELINE.json configurations (config.secondary_cold), the per-class and per-kernel profile pass with its rooflines, the HBM traffic
of the dominant kernel and the CPU baseline. `--headline-only`, `--no-side-configs`, `--live-pmc off` and `--no-cpu-baseline` leave single
parts of `--full` out; `--launch-log` needs it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL (must be set before the runtime starts)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BF16_PEAK_TFLOPS = 2500.0   # dense bf16 MFMA peak, MI355X (guides/MI355X_MICROARCH.md)
FP8_PEAK_TFLOPS = 5000.0    # dense fp8 MFMA peak (MX / f8f6f4 K = 64 instructions), same guide
FP32_PEAK_TFLOPS = 157.3


def flops_per_sample(E, N, Lp, n_prompt_obj, Q, T):
    """Algorithmic FLOPs (2 per MAC) of one sample, formulas of SURVEY.md section 8(d)."""
    vit = 2 * 4 * 768 * 768 + 4 * (2 * 5 * 768 * 2304 + 4 * 25 * 768 + 2 * 5 * 768 ** 2 + 2 * (2 * 5 * 768 * 3072)) + 2 * 768 ** 2
    obj = vit + 2 * (4 * 768 + 768 ** 2 + 768 ** 2) + 2 * 1536 * E
    obs = obj + 2 * (E + 2) * E
    pobj = obj + 2 * (E * 768 + 768 ** 2 + 768 ** 2)
    t5 = 12 * (24 * Lp * 768 ** 2 + 4 * Lp ** 2 * 768) + (2 * Lp * 768 * E if E != 768 else 0)
    Lq = T * (Q + 1) - 1
    xgpt = N * (60 * Lq * E ** 2 + 4 * Lp * E ** 2 + 4 * Lq * Lp * E + 4 * Lq ** 2 * E)
    head = 12 * 2 * (E * 512 + 512 ** 2) + 2 * 512 * 700
    prompt = n_prompt_obj * pobj + t5
    step = T * Q * obs + xgpt + head
    return prompt + step, step


_LIVE_PMC = None   # summary dict of live_pmc_traffic() once collected in this run


def pmc_traffic(kernel=None):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/): the counters need their own profiler runs
    (FETCH_SIZE and WRITE_SIZE do not fit one pass), so bench.py reports the last committed measurement of this same command
    rather than collecting it live. `kernel` = a rocprofv3 kernel name: that kernel's own bytes per launch (newer summaries
    carry a per-kernel table); without it, or for older summaries, the average over all bf16 GEMM launches. None if absent."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    if _LIVE_PMC is None and not files:
        return None
    try:
        d = _LIVE_PMC if _LIVE_PMC is not None else json.load(open(files[-1]))
        if kernel is not None:
            pk = d.get("per_kernel", {})
            key = kernel.replace(" ", "")
            for name, v in pk.items():
                if name.replace(" ", "") == key:
                    return round(float(v["bytes_per_launch"]), 1)
            return None
        return round(float(d["gemm_bf16_bytes_per_launch"]), 1)
    except Exception:
        return None


def gpu_numa_cpus(dev_index: int):
    """(numa_node, sorted cpu list) of the host CPUs local to GPU `dev_index`, from the PCI address torch reports and sysfs
    (/sys/bus/pci/devices/<dddd:bb:dd.f>/{numa_node,local_cpulist}); None when any piece is unavailable."""
    try:
        pr = torch.cuda.get_device_properties(dev_index)
        addr = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
        base = f"/sys/bus/pci/devices/{addr}"
        node = int(open(base + "/numa_node").read().strip())
        cpus = []
        for part in open(base + "/local_cpulist").read().strip().split(","):
            if not part:
                continue
            lo, _, hi = part.partition("-")
            cpus.extend(range(int(lo), int(hi or lo) + 1))
        return (node, sorted(cpus)) if cpus else None
    except Exception:   # noqa: BLE001 -- no PCI ids in this torch build, no sysfs entry, node -1 ...
        return None


def pin_to_gpu_numa(dev_index: int):
    """N > 1 ranks each issue ~500 launches per step: keep a rank's host threads on the NUMA node of ITS GPU.
    Returns what was done, for the JSON line; never fails the run."""
    info = gpu_numa_cpus(dev_index)
    if info is None or not hasattr(os, "sched_setaffinity"):
        return {"pinned": False, "reason": "GPU NUMA node / local cpulist not available"}
    node, cpus = info
    allowed = sorted(set(cpus) & set(os.sched_getaffinity(0)))
    if node < 0 or len(allowed) < 2:
        return {"pinned": False, "numa_node": node, "reason": "no NUMA locality reported or too few allowed CPUs on that node"}
    try:
        os.sched_setaffinity(0, allowed)
    except OSError as e:
        return {"pinned": False, "numa_node": node, "reason": str(e)}
    return {"pinned": True, "numa_node": node, "cpus": len(allowed)}


def live_pmc_traffic(argv_tail, timeout_s=150.0):
    """HBM bytes per launch measured NOW: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE: they do not fit one pass) over a
    subprocess running this same workload for one step with dual_stream = 0, which also writes the GEMM launch log (kernel, M, N, K
    in launch order) so that per-dispatch counter values can be attributed to GEMM SHAPES (scripts/pmc_summary.py). Returns
    (summary dict, None) or (None, reason)."""
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not found"
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import pmc_summary
    except Exception as e:   # noqa: BLE001
        return None, f"scripts/pmc_summary.py not importable: {e}"
    tmp = tempfile.mkdtemp(prefix="vima_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    log = os.path.join(tmp, "launches.json")
    t_end = time.perf_counter() + timeout_s
    dbs = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        out = os.path.join(tmp, ctr.lower())
        cmd = [exe, "--kernel-trace", "--pmc", ctr, "-d", out, "-o", "bench", "--", sys.executable, os.path.abspath(__file__),
               "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline", "--headline-only", "--live-pmc", "off", "--opt", "dual_stream=0",
               "--launch-log", log] + argv_tail
        left = t_end - time.perf_counter()
        if left < 10:
            return None, "time budget for the live PMC passes exhausted"
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=left)
        except subprocess.TimeoutExpired:
            return None, f"rocprofv3 --pmc {ctr} pass timed out"
        db = None
        for root_, _, files in os.walk(out):
            for f in files:
                if f.endswith("_results.db"):
                    db = os.path.join(root_, f)
        if r.returncode != 0 or db is None:
            return None, f"rocprofv3 --pmc {ctr} pass failed (rc {r.returncode}): {(r.stderr or r.stdout)[-300:]}"
        dbs[ctr] = db
    try:
        summ = pmc_summary.summarise(dbs["FETCH_SIZE"], dbs["WRITE_SIZE"], log if os.path.exists(log) else None)
    except Exception as e:   # noqa: BLE001
        return None, f"pmc summary failed: {type(e).__name__}: {e}"
    summ["source"] = "live: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (two passes) over this workload, 1 step, dual_stream=0, in this bench.py run"
    return summ, None


def cached_state_dict(syn, cfg, rank, world, dist):
    """Seeded random weights. One rank: built here. N ranks: rank 0 builds them and writes ONE file, the others wait at a barrier and read it
    (memory-mapped), rank 0 removes it -- instead of N concurrent host-side builds. Returns (state dict, how it was obtained)."""
    if world == 1:
        return syn.make_state_dict(cfg, 0), "built in process"
    # rank 0 creates a PRIVATE directory (mkdtemp: mode 0700, unpredictable name) and tells the others where it is; the ranks of one node share its
    # file system (bench.py is a single-node tool: --nnodes=1)
    import tempfile
    holder = [None]
    sd = None
    t0 = time.perf_counter()
    if rank == 0:
        holder[0] = os.path.join(tempfile.mkdtemp(prefix="vima_sd_"), "state_dict.pt")
        sd = syn.make_state_dict(cfg, 0)
        torch.save(sd, holder[0])
    dist.broadcast_object_list(holder, src=0, device=(torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else None))
    path = holder[0]
    if rank != 0:
        try:
            sd = torch.load(path, map_location="cpu", mmap=True, weights_only=True)
        except TypeError:       # torch without the mmap argument: still tensors only, never arbitrary pickles
            sd = torch.load(path, map_location="cpu", weights_only=True)
    dist.barrier()
    if rank == 0:
        try:
            os.remove(path)
            os.rmdir(os.path.dirname(path))
        except OSError:
            pass
    return sd, f"rank 0 built it once ({time.perf_counter() - t0:.1f} s incl. the file), ranks 1..{world - 1} read {os.path.basename(path)}"


def rccl_summary(path, max_chars=1500):
    """What RCCL logged about the communicators of this process (NCCL_DEBUG=INFO, subsystems INIT,GRAPH, into NCCL_DEBUG_FILE): version line,
    channel count, the first ring / tree lines. Best effort: None when the file is missing or empty."""
    try:
        lines = open(path, errors="replace").read().splitlines()
    except OSError:
        return None
    import re
    pick = {"version": None, "rings": [], "trees": [], "channels": None, "algo_lines": []}
    for ln in lines:
        low = ln.lower()
        if pick["version"] is None and ("rccl version" in low or "nccl version" in low):
            pick["version"] = ln.split("INFO", 1)[-1].strip()[:160]
        if re.search(r"\bring \d+ *:", low) and len(pick["rings"]) < 2:
            pick["rings"].append(ln.split("INFO", 1)[-1].strip()[:160])
        if re.search(r"\btrees? \[", low) and len(pick["trees"]) < 1:
            pick["trees"].append(ln.split("INFO", 1)[-1].strip()[:160])
        m = re.search(r"(\d+) coll channels", low)
        if m:
            pick["channels"] = ln.split("INFO", 1)[-1].strip()[:160]
    try:
        pick["torch_nccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:   # noqa: BLE001
        pass
    pick["log_lines"] = len(lines)
    out = {k: v for k, v in pick.items() if v}
    return out or None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """--dump-outputs DIR: what the timed path returned in its last step, one DIR/<name>.npy per array in float32, so that two builds can
    be compared output for output on the same seeded inputs. When the arrays exceed 64 MB together, every array keeps the same fixed,
    seeded sample of its rows, and the row indices go to DIR/<name>_rows.npy (float64)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    total = sum(a.numel() * 4 for a in arrays.values())
    budget = DUMP_LIMIT_BYTES - (1 << 20)         # headroom for the row-index files and the .npy headers
    for name, a in arrays.items():
        a = a.detach().float().cpu()
        if total > DUMP_LIMIT_BYTES:
            keep = max(1, a.shape[0] * budget // total)
            rows = torch.randperm(a.shape[0], generator=torch.Generator().manual_seed(0))[:keep].sort().values
            a = a[rows]
            np.save(os.path.join(dirname, f"{name}_rows.npy"), rows.double().numpy())
        np.save(os.path.join(dirname, f"{name}.npy"), a.contiguous().numpy())


def usable_cores() -> int:
    """Cores this process may actually use (affinity mask and cgroup CPU quota), not the host's os.cpu_count()."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    return max(1, n)


def run_cpu_baseline(cfg, sd, n_seg, qv, cpu_batch, B, budget_s=30.0, words=8):
    """The oracle (torch fp32 port of the reference CPU path) timed on the host cores on a BOUNDED sample of the same
    workload. Thread count is calibrated first (a 256-thread host with a small cgroup quota is slower at 256 threads)."""
    from oracle.vima_oracle import OraclePolicy
    from vima_testing import synthetic as syn
    # kind "reference": the UNMODIFIED reference policy (vima/policy/vima_policy.py through oracle/ref_shim.py) when /root/reference exists on this
    # machine (the build container); on the GPU box it does not, and the timed CPU path is the oracle port (kind "port")
    ref_mod = None
    try:
        from oracle import ref_shim
        if ref_shim.reference_available():
            ref_mod = ref_shim
    except Exception:   # noqa: BLE001
        ref_mod = None
    ncores = usable_cores()
    cands = sorted({max(1, ncores >> s) for s in range(0, 6)} | {min(ncores, 8)}, reverse=True)
    a = torch.randn(1024, 768)
    w = torch.randn(3072, 768)
    best_t, best_rate = cands[-1], 0.0
    for t in cands:
        torch.set_num_threads(t)
        torch.nn.functional.linear(a, w)
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < 0.25:
            torch.nn.functional.linear(a, w)
            n += 1
        rate = n / (time.perf_counter() - t0)
        if rate > best_rate * 1.05:
            best_t, best_rate = t, rate
    torch.set_num_threads(best_t)
    if ref_mod is not None:
        from oracle.cases import run_policy
        from oracle.vima_oracle import ACTION_KEYS
        ref = ref_mod.build_reference_policy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions)
        ref.load_state_dict(sd, strict=True)
        ref.eval()

        class _RefCold:   # the reference driven like scripts/example.py drives it: prompt, obs tokens, forward, action decoder
            def cold_step(self, p, o):
                _, d = run_policy(ref, p, {"objects": ref_mod.MapDict(o["objects"]), "ee": o["ee"]}, None)
                return torch.cat([d[k].raw_logits if hasattr(d[k], "raw_logits") else torch.cat([c.logits for c in d[k]._dists], dim=-1) for k in ACTION_KEYS], dim=-1)
        orc = _RefCold()
    else:
        orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    t_start = time.perf_counter()
    with torch.no_grad():
        p1 = syn.make_prompt(1, n_segments=n_seg, words_per_segment=words, q_per_view=qv, seed=1236)
        o1 = syn.make_obs(1, 1, qv, seed=1336)
        t0 = time.perf_counter()
        orc.cold_step(p1, o1)                                   # warm-up + cost probe at batch 1
        t_b1 = time.perf_counter() - t0
        cb, it, cdt = 1, 1, t_b1
        if t_b1 * (cpu_batch + 1) < budget_s:                   # affordable: time the requested sample batch
            pc = syn.make_prompt(cpu_batch, n_segments=n_seg, words_per_segment=words, q_per_view=qv, seed=1236)
            oc = syn.make_obs(1, cpu_batch, qv, seed=1336)
            it, t1 = 0, time.perf_counter()
            while it < 3 and (time.perf_counter() - t_start) + (time.perf_counter() - t1) / max(it, 1) < budget_s:
                orc.cold_step(pc, oc)
                it += 1
                if it == 1 and (time.perf_counter() - t1) * 2 + (time.perf_counter() - t_start) > budget_s:
                    break
            cb, cdt = cpu_batch, (time.perf_counter() - t1) / max(it, 1)
    samples_per_s = cb / cdt
    if ref_mod is not None:
        what = (f"the UNMODIFIED reference policy (/root/reference through oracle/ref_shim.py: prompt assembly incl. its Python loop, obs tokens, forward, "
                f"action decoder), same VIMA-200M cold workload at batch {cb}")
    else:
        what = (f"oracle (torch fp32 restatement of the reference's CPU path), same VIMA-200M cold workload at batch {cb}; NOT in the timed port: the "
                "reference's O(B*Lp) Python prompt-assembly loop (vima_policy.py:168-233; the oracle assembles with index ops) and its DataDict plumbing. "
                "/root/reference does not exist on this machine, so the shimmed reference cannot be timed here; in the build container (same workload, batch 4) "
                "the unmodified reference and this port run within a few per cent of each other (profiles/r05_cpu_reference_vs_port.json)")
    return {"value": round(samples_per_s / B, 6), "unit": "steps/s", "cores": best_t, "kind": "reference" if ref_mod is not None else "port",
            "sample": f"{what} ({it} timed pass(es), {cdt:.2f} s each = {samples_per_s:.3f} samples/s), expressed in batch-{B} steps/s",
            "usable_cores": ncores, "host_cpu_count": os.cpu_count(), "threads_tried": cands}


def side_config(syn, sd_cache, dev, rank, *, model, batch, prompt_len, qv, words, precision, T, steps):
    """One other BASELINE.json configuration on its own handle, outside the timed region: COLD step time (best of 3 x `steps`), the
    library profiler's per-class split of one step and the MFMA roofline of the algorithmic FLOPs -- the FLOPs the fp8-operand GEMM kernels
    (`gemm_pp_kernel<.., true>`) executed are priced against the 5 PF dense fp8 peak, everything else against 2.5 PF bf16."""
    from vima_amd.policy import VIMAPolicy
    Q = 2 * qv
    seg = words + Q
    assert prompt_len % seg == 0
    n_seg = prompt_len // seg
    cfg = syn.config(model, xattn_n_positions=max(256, prompt_len))
    key = (model, cfg.xattn_n_positions)
    if key not in sd_cache:
        sd_cache[key] = syn.make_state_dict(cfg, 0)
    pol = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision=precision, device=dev)
    pol.load_state_dict(sd_cache[key], strict=True)
    prompts = syn.to_device(syn.make_prompt(batch, n_segments=n_seg, words_per_segment=words, q_per_view=qv, seed=1236 + rank), dev)
    obs = syn.to_device(syn.make_obs(T, batch, qv, seed=1336 + rank), dev)
    past = syn.to_device(syn.make_actions(T - 1, batch, seed=1436 + rank), dev) if T > 1 else None

    def step():
        ptok, pmask = pol.forward_prompt_assembly(prompts)
        otok, omask = pol.forward_obs_token(obs)
        atok = pol.forward_action_token(past) if past is not None else None
        return pol.action_logits(pol.forward(otok, omask, atok, ptok, pmask)[-1])

    for _ in range(3):          # fp8: the first pass calibrates the activation scales (fp8w kernels), the next ones run fp8 activations
        out = step()
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(out).all())
    ms = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize(dev)
        ms = min(ms, (time.perf_counter() - t0) / steps * 1e3)
    pol.set_option("dual_stream", 0)
    step()
    torch.cuda.synchronize(dev)
    pol.prof_enable(True)
    step()
    torch.cuda.synchronize(dev)
    gk = pol.prof_read_gemm_kernels()
    prof = pol.prof_read_ex()
    pol.prof_enable(False)
    cold, _ = flops_per_sample(cfg.embed_dim, cfg.xf_n_layers, prompt_len, n_seg * Q, Q, T)
    f8 = sum(v["flops"] for k, v in gk.items() if k.endswith(", true>"))
    total = batch * cold
    t_roof = (min(f8, total) / (FP8_PEAK_TFLOPS * 1e12) + max(total - f8, 0.0) / (BF16_PEAK_TFLOPS * 1e12)) * 1e3
    gemm_ms = prof["gemm"]["ms"] + prof["gemm_residual"]["ms"]
    gemm_fl = prof["gemm"]["flops"] + prof["gemm_residual"]["flops"]
    dom = max(gk, key=lambda k: gk[k]["ms"]) if gk else None
    del pol
    torch.cuda.empty_cache()
    return {"workload": f"VIMA-{model} COLD policy forward, batch {batch}, {prompt_len}-token prompt ({n_seg} x [{words} words + 1 image]), "
                        f"{Q} object tokens/obs, T={T}, {precision}",
            "ms_per_step": round(ms, 3), "steps_per_s": round(1e3 / ms, 2), "samples_per_s": round(batch * 1e3 / ms, 1),
            "timing": f"best of 3 x {steps} steps", "bound": "mfma", "roofline_ms": round(t_roof, 4), "roofline_frac": round(t_roof / ms, 4),
            "algorithmic_tflop_per_step": round(total / 1e12, 3), "fp8_gemm_flop_share": round(f8 / total, 3) if total else 0.0,
            "whole_step_tflops": round(total / (ms * 1e-3) / 1e12, 1),
            "all_gemm_tflops": round(gemm_fl / (gemm_ms * 1e-3) / 1e12, 1) if gemm_ms > 0 else 0.0,
            "gemm_ms": round(gemm_ms, 3), "attention_ms": round(prof["attention"]["ms"], 3), "other_ms": round(prof["other"]["ms"], 3),
            "dominant_kernel": dom, "dominant_kernel_ms": round(gk[dom]["ms"], 3) if dom else None,
            "dominant_kernel_tflops": round(gk[dom]["flops"] / (gk[dom]["ms"] * 1e-3) / 1e12, 1) if dom and gk[dom]["ms"] > 0 else None}


def extras(args, pol, syn, cfg, prompts, obs, past, sync, dev, rank, n_seg, Q, B, sd=None):
    """WARM step, incremental env step and the batch-1 / batch-32 cold steps (reported as extras, outside the timed region)."""
    secondary = {}
    # ---- WARM step (prompt tokens reused: obs ViT + decoder + action head), timed the same way, reported as an extra
    ptok_c, pmask_c = pol.forward_prompt_assembly(prompts)

    def warm_step():
        otok, omask = pol.forward_obs_token(obs)
        atok = pol.forward_action_token(past) if past is not None else None
        pred = pol.forward(otok, omask, atok, ptok_c, pmask_c)
        return pol.action_logits(pred[-1])

    warm_step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        warm_step()
    sync()
    warm_ms = (time.perf_counter() - t0) / args.steps * 1e3

    # ---- INCREMENTAL episode: env steps 1..8 through vima_decode_step (history in the native episode
    # caches), each step = obs ViT of ONE step + decoder on the newest tokens + action head; reported as an extra
    obs1 = syn.to_device(syn.make_obs(1, B, args.qv, seed=1536 + rank), dev)
    act1 = syn.to_device(syn.make_actions(1, B, seed=1636 + rank), dev)

    def env_step(t):
        otok, omask = pol.forward_obs_token(obs1)
        atok = pol.forward_action_token(act1) if t > 0 else None
        pred = pol.forward_step(otok, omask, atok, ptok_c, pmask_c, t)
        return pol.action_logits(pred)

    for t in range(3):
        env_step(t)                                   # warm-up episode
    env_step(0)                                       # step 0 (builds the prompt K/V cache) is not timed
    sync()
    t0 = time.perf_counter()
    for t in range(1, 9):
        env_step(t)                                   # steps 1..8: 9 new tokens against 8..71 cached ones
    sync()
    inc_ms = (time.perf_counter() - t0) / 8 * 1e3

    # ---- north_star's other batch sizes, driver-visible in the same run: COLD steps at batch 1 and 32 of
    # the same model / prompt, each with the roofline that binds it (batch 1: the ~676 MB of bf16 weights over HBM;
    # batch 32: bf16 MFMA)
    WEIGHT_BYTES = {"bf16": 676e6, "fp8w": 370e6, "fp8": 370e6, "fp32": 1352e6}[args.precision]          # weights touched once per pass
    for b2 in (1, 32):
        if b2 >= B:
            continue
        p2 = syn.to_device(syn.make_prompt(b2, n_segments=n_seg, words_per_segment=args.words, q_per_view=args.qv, seed=1236 + rank), dev)
        o2 = syn.to_device(syn.make_obs(1, b2, args.qv, seed=1336 + rank), dev)

        def step2():
            ptok, pmask = pol.forward_prompt_assembly(p2)
            otok, omask = pol.forward_obs_token(o2)
            return pol.action_logits(pol.forward(otok, omask, None, ptok, pmask)[-1])

        step2()
        step2()
        sync()
        n2 = max(args.steps, 20)
        ms2 = float("inf")
        for _ in range(3):          # these steps take milliseconds and ~500 launches each: best of three repeats of n2 steps
            t0 = time.perf_counter()
            for _ in range(n2):
                step2()
            sync()
            ms2 = min(ms2, (time.perf_counter() - t0) / n2 * 1e3)
        cold2, _ = flops_per_sample(cfg.embed_dim, cfg.xf_n_layers, args.prompt_len, n_seg * Q, Q, 1)
        t_mfma = b2 * cold2 / ((FP32_PEAK_TFLOPS if args.precision == "fp32" else BF16_PEAK_TFLOPS) * 1e12) * 1e3
        t_hbm = WEIGHT_BYTES / 8e12 * 1e3
        secondary[f"batch_{b2}"] = {
            "ms_per_step": round(ms2, 3), "steps_per_s": round(1e3 / ms2, 2), "samples_per_s": round(b2 * 1e3 / ms2, 1),
            "bound": "hbm" if t_hbm > t_mfma else "mfma", "roofline_ms": round(max(t_hbm, t_mfma), 4),
            "roofline_frac": round(max(t_hbm, t_mfma) / ms2, 4), "timing": f"best of 3 x {n2} steps"}

    # ---- the other BASELINE.json configurations, driver-visible in the same record: configs[1] (VIMA-20M, batch 32,
    # 256-token prompt, 4 object tokens / obs), the single-GPU share of configs[4] (1024-token prompt, bf16 and fp8) and T = 8 (the history
    # re-fed like the reference's eval loop does). Only from the default workload (rank 0 of a 1-GPU run): they need their own handles.
    default_run = (args.model == "200M" and B == 256 and args.prompt_len == 512 and args.precision == "bf16" and not args.opt
                   and os.environ.get("WORLD_SIZE", "1") == "1")
    if default_run and not args.no_side_configs:
        sd_cache = {("200M", cfg.xattn_n_positions): sd} if sd is not None else {}
        for name, kw in (("cfg2_20M", dict(model="20M", batch=32, prompt_len=256, qv=2, words=4, precision="bf16", T=1, steps=20)),
                         ("lp1024_bf16", dict(model="200M", batch=256, prompt_len=1024, qv=4, words=8, precision="bf16", T=1, steps=3)),
                         ("lp1024_fp8", dict(model="200M", batch=256, prompt_len=1024, qv=4, words=8, precision="fp8", T=1, steps=3)),
                         ("t8", dict(model="200M", batch=256, prompt_len=512, qv=4, words=8, precision="bf16", T=8, steps=3))):
            try:
                secondary[name] = side_config(syn, sd_cache, dev, rank, **kw)
            except Exception as e:   # noqa: BLE001 -- a side configuration must never take the headline line down
                secondary[name] = {"error": f"{type(e).__name__}: {e}"}
    return warm_ms, inc_ms, secondary


def bench_baseline_policy(args):
    """`--policy gpt|gato|flamingo`: ONE measured line for a baseline policy (reference:
    vima/policy/vima_gpt_policy.py:118-187, vima_gato_policy.py:115-188, vima_flamingo_policy.py:121-227) at the VIMA-200M transformer size
    (embed_dim 768, 11 layers, 12 heads), batch `--batch`, a prompt of 8 segments of (`--words` words + 1 RGB frame pair) and T = `--steps-history`
    observation steps: the COLD step (prompt encoding + observation encoding + decoder + action head), timed like the headline, with the
    library's own per-class split (HIP events on the launch stream). Not the headline metric: `config.workload` names it."""
    from vima_testing import synthetic as syn
    from vima_amd.baselines import build_baseline
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    kind = args.policy
    cfg = syn.BaselineConfig(kind, 768, 11, 12, xattn_n_heads=12 if kind == "flamingo" else 0)
    sd = syn.make_baseline_state_dict(cfg, 0)
    pol = build_baseline(cfg, precision=args.precision, device=dev)
    pol.load_state_dict(sd, strict=True)
    for kv in args.opt:
        k, v = kv.split("=")
        pol.set_option(k, int(v))
    B, T, n_seg = args.batch, args.steps_history, 8
    prompts = syn.to_device(syn.make_rgb_prompt(B, n_segments=n_seg, words_per_segment=args.words, seed=1236), dev)
    obs = syn.to_device(syn.make_rgb_obs(T, B, seed=1336), dev)
    past = syn.to_device(syn.make_actions(T - 1, B, seed=1436), dev) if T > 1 else None

    def step():
        ptok, pmask = pol.forward_prompt_assembly(prompts)
        otok = pol.forward_obs_token(obs)
        atok = pol.forward_action_token(past) if past is not None else None
        pred = pol.forward(otok, atok, ptok, pmask)
        return pol.action_logits(pred[-1]), ptok.shape[0]

    for _ in range(max(args.warmup, 1)):
        logits, Lp = step()
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all() and tuple(logits.shape) == (B, 700)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        logits, _ = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"logits": logits})
    split = roofline = None
    if args.full:          # the per-class split and the executed FLOPs come from a profiled step of their own
        pol.prof_enable(True)
        pol.set_option("dual_stream", 0)
        step()
        torch.cuda.synchronize()
        prof = pol.prof_read_ex()
        pol.prof_enable(False)
        tot_fl = sum(prof[k]["flops"] for k in prof)
        split = {k: {"ms": round(v["ms"], 3), "launches": v["launches"], "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ms"] > 0 else 0.0}
                 for k, v in prof.items()}
        peak = BF16_PEAK_TFLOPS if args.precision != "fp32" else FP32_PEAK_TFLOPS
        roofline = {"bound": "mfma", "achieved": round(tot_fl / (ms * 1e-3) / 1e12, 1), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(tot_fl / (ms * 1e-3) / 1e12 / peak, 4),
                    "traffic": None, "note": "whole step: the launch log's executed FLOPs / wall time"}
    print(json.dumps({
        "metric": f"policy-forward steps/sec, {kind} baseline policy (VIMA-200M transformer size), batch {B}", "value": round(1e3 / ms, 4), "unit": "steps/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
        "config": {"workload": f"{kind} baseline policy: embed_dim 768, 11 layers, 12 heads; batch {B}; prompt of {n_seg} x ({args.words} words + 1 RGB frame pair) = "
                               f"{Lp} tokens; T = {T} observation steps ({cfg.obs_tokens} tokens each); COLD step (prompt + observation encoding, decoder, "
                               f"action head); random-init weights", "policy": kind, "prompt_tokens": int(Lp), "obs_tokens_per_step": cfg.obs_tokens},
        "class_split_dual_stream_off": split, "roofline": roofline}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", default="vima", choices=["vima", "gpt", "gato", "flamingo"], help="vima: the headline workload (default); gpt / gato / flamingo: "
                    "one measured line for that BASELINE policy (1 GPU, its own metric)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256, help="samples per GPU per step")
    ap.add_argument("--model", default="200M")
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--qv", type=int, default=4, help="objects per view (Q = 2*qv object tokens per observation)")
    ap.add_argument("--words", type=int, default=8, help="words per prompt segment (a segment = words + 1 image)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "fp8w", "fp8"])
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure everything else: the warm / incremental / batch-1 / "
                    "batch-32 steps, the other BASELINE.json configurations, the per-kernel profile pass and its rooflines, the HBM traffic of the "
                    "dominant kernel, the CPU baseline. Off by default: a plain run sets up, warms up, times the steps and prints its line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--headline-only", action="store_true", help="with --full: skip the warm / incremental / batch-1 / batch-32 extras (profiler runs: "
                    "every kernel launch in the trace then belongs to the headline workload)")
    ap.add_argument("--cpu-batch", type=int, default=4)
    ap.add_argument("--steps-history", type=int, default=1, help="T: observation steps in the history (T-1 past actions)")
    ap.add_argument("--opt", action="append", default=[], help="library option key=value (vima_set_option), repeatable")
    ap.add_argument("--live-pmc", default="auto", choices=["auto", "off"], help="with --full. auto: collect roofline.traffic NOW with two rocprofv3 --pmc passes "
                    "over a subprocess of this workload (1 GPU, default workload only, rocprofv3 installed); off / unavailable: the last committed "
                    "profiles/r*_pmc_traffic.json. The JSON line says which (roofline.traffic_source)")
    ap.add_argument("--launch-log", default=None, help="with --full: write the GEMM launch log of one step (kernel, M, N, K in launch order) to this JSON file "
                    "(scripts/pmc_summary.py joins it with per-dispatch counter values)")
    ap.add_argument("--dry-ranks", type=int, default=0, help="CPU self-check of the N > 1 HOST path (VERDICT r4 item 6): re-launches this script with N ranks "
                    "over gloo, a stub communicator behind LogitsComm (same call order as the RCCL one: id drawn by rank 0, broadcast, join, all-gather, "
                    "destroy), the rank-0-written state-dict cache, the agreement all-reduce, K synthetic steps with the barrier / max-over-ranks timing "
                    "and teardown. No GPU, no policy, no measurement: the line it prints is marked dry_run")
    ap.add_argument("--no-side-configs", action="store_true", help="with --full: skip the other BASELINE.json configurations (VIMA-20M batch 32, Lp = 1024 in bf16 "
                    "and fp8, T = 8) that the default run reports under config.secondary_cold")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last timed step returned "
                    "(the [global batch, 700] action logits) to DIR/logits.npy in float32; the inputs are seeded, so two builds can be compared")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.launch_log and not args.full:
        ap.error("--launch-log is written by the profile pass: it needs --full")
    if args.policy != "vima":
        if args.gpus != 1 or os.environ.get("WORLD_SIZE", "1") != "1":
            sys.exit("bench.py --policy gpt|gato|flamingo is a single-GPU line")
        return bench_baseline_policy(args)

    # ---- N ranks: `--gpus N` without a torchrun environment re-launches this script under torch.distributed.run with one
    # rank per GPU; it never silently measures fewer GPUs than asked for.
    # VIMA_BENCH_SHARED_GPU=1 (tests only): every rank uses GPU 0 and the ranks talk over gloo, so that the self-relaunch / rank
    # agreement / max-over-ranks path below can be EXECUTED on a one-GPU box; the printed line is marked and is not a measurement
    shared_gpu = os.environ.get("VIMA_BENCH_SHARED_GPU") == "1"
    dry = os.environ.get("VIMA_BENCH_DRY") == "1"
    if args.dry_ranks == 1 or args.dry_ranks < 0:
        sys.exit("bench.py: --dry-ranks needs at least 2 ranks (it rehearses the N > 1 host path)")
    if args.dry_ranks and "WORLD_SIZE" not in os.environ:
        import socket
        import subprocess
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        argv = [a for i, a in enumerate(sys.argv[1:]) if a != "--gpus" and (i == 0 or sys.argv[i] != "--gpus") and not a.startswith("--gpus=")]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.dry_ranks}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + argv + ["--gpus", str(args.dry_ranks)]
        sys.exit(subprocess.call(cmd, env=dict(os.environ, VIMA_BENCH_DRY="1", OMP_NUM_THREADS="1")))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        if not shared_gpu:           # counting devices starts the HIP runtime: in the shared-GPU test mode the launcher never opens the GPU
            visible = torch.cuda.device_count()
            if visible < args.gpus:
                sys.exit(f"bench.py: --gpus {args.gpus} requested but only {visible} GPU(s) are visible on this node; refusing to "
                         f"print a {visible}-GPU number as a {args.gpus}-GPU result")
        import socket
        import subprocess
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if shared_gpu:
        local_rank = 0
    if not dry and torch.cuda.device_count() <= local_rank:
        sys.exit(f"bench.py: rank {rank} needs GPU {local_rank} but only {torch.cuda.device_count()} are visible")
    import torch.distributed as dist
    dev = torch.device("cpu") if dry else torch.device("cuda", local_rank)
    if not dry:
        torch.cuda.set_device(dev)
    affinity0 = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None
    host_affinity = (pin_to_gpu_numa(local_rank) if world > 1 and not dry else
                     {"pinned": False, "reason": "dry run: no GPU" if dry else "single rank: not pinned"})
    comm = None
    rccl_log = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if shared_gpu or dry:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            # RCCL's own account of what it built (version, channels, ring / tree per channel) goes to a per-process FILE -- stdout carries exactly
            # one JSON line -- and rank 0's copy is summarised into config.collective_info after the first collectives
            if "NCCL_DEBUG" not in os.environ:
                os.environ["NCCL_DEBUG"] = "INFO"
                os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,GRAPH")
                os.environ.setdefault("NCCL_DEBUG_FILE", "/tmp/vima_rccl_%h_%p.log")
            rccl_log = os.environ.get("NCCL_DEBUG_FILE", "").replace("%h", __import__("socket").gethostname()).replace("%p", str(os.getpid())) or None
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        world = dist.get_world_size()                  # the LIVE RCCL world size is what gets reported as n_gpus

    from vima_amd import parallel
    from vima_testing import synthetic as syn
    from vima_amd.policy import VIMAPolicy
    collective = None
    stub = None
    if world > 1 and dry:
        stub = parallel.StubCommBackend()
        comm = parallel.LogitsComm(dev, backend=stub)        # same creation order as the RCCL communicator below: rank 0 draws the id, broadcast, join
        ok = torch.tensor([1 if comm.world == world else 0])
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)            # the agreement step of the real path
        assert int(ok.item()) == 1
        collective = "LogitsComm over a StubCommBackend (gloo): DRY RUN of the N > 1 host path, no GPU"
    elif world > 1 and shared_gpu:
        collective = "torch.distributed all_gather over gloo (VIMA_BENCH_SHARED_GPU test mode: ranks share one GPU, RCCL refuses that)"
    elif world > 1:
        # RCCL communicator behind the C ABI (vima_allgather_logits). Every rank must take the same path: agree on success
        # through the torch.distributed group; if any rank failed to create it, all fall back to torch.distributed's own
        # all-gather (also RCCL) and the line says so.
        err = ""
        try:
            comm = parallel.LogitsComm(dev)
            assert comm.world == world
        except Exception as e:   # noqa: BLE001
            comm, err = None, f"{type(e).__name__}: {e}"
        ok = torch.tensor([0 if comm is None else 1], device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            collective = "vima_allgather_logits (C ABI, RCCL)"
        else:
            if comm is not None:
                comm.close()
            comm = None
            collective = f"torch.distributed all_gather_into_tensor (RCCL); C-ABI communicator unavailable on some rank: {err or 'other rank'}"

    Q = 2 * args.qv
    seg_len = args.words + Q                         # words + 1 image (Q object tokens) per segment
    assert args.prompt_len % seg_len == 0, "prompt length must be a multiple of words + Q"
    n_seg = args.prompt_len // seg_len
    cfg = syn.config("2M" if dry else args.model, xattn_n_positions=max(256, args.prompt_len))
    # seeded random weights (no checkpoints offline). N > 1: rank 0 builds them once and the others read its file -- eight concurrent builds of the
    # 389 M-parameter dict (orthogonal inits on the host) would each take minutes on a node whose cores are split eight ways
    sd, sd_source = cached_state_dict(syn, cfg, rank, world, dist)
    B = args.batch
    T = args.steps_history
    pol = prompts = obs = past = None
    if not dry:
        pol = VIMAPolicy(**cfg.ctor_kwargs(), xattn_n_positions=cfg.xattn_n_positions, precision=args.precision, device=dev)
        pol.load_state_dict(sd, strict=True)
        for kv in args.opt:
            k, v = kv.split("=")
            pol.set_option(k, int(v))
        prompts = syn.to_device(syn.make_prompt(B, n_segments=n_seg, words_per_segment=args.words, q_per_view=args.qv, seed=1236 + rank), dev)
        obs = syn.to_device(syn.make_obs(T, B, args.qv, seed=1336 + rank), dev)
        past = syn.to_device(syn.make_actions(T - 1, B, seed=1436 + rank), dev) if T > 1 else None

    ag_events = []    # (start, end) events around the logits all-gather of every TIMED step (N > 1): a bad scaling curve must be
                      # attributable to the collective or to the ranks' own step time from the JSON line alone

    class _HostEvent:      # dry run: the all-gather bracket with the host clock (same (start, end).elapsed_time interface, milliseconds)
        def __init__(self):
            self.t = 0.0

        def record(self):
            self.t = time.perf_counter()

        def elapsed_time(self, other):
            return (other.t - self.t) * 1e3

    def local_logits():
        if dry:            # a value only THIS rank and row can produce: the gathered matrix is checked below
            return (torch.arange(B, dtype=torch.float32)[:, None] + 1000.0 * rank).expand(B, 700).contiguous()
        ptok, pmask = pol.forward_prompt_assembly(prompts)
        otok, omask = pol.forward_obs_token(obs)
        atok = pol.forward_action_token(past) if past is not None else None
        pred = pol.forward(otok, omask, atok, ptok, pmask)
        return pol.action_logits(pred[-1])

    def step(timed=False):
        logits = local_logits()
        if world == 1:
            return logits
        if not timed:
            return parallel.all_gather_logits(logits, global_batch=B * world, comm=comm)
        e0, e1 = (_HostEvent(), _HostEvent()) if dry else (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e0.record()        # torch's current stream = the stream LogitsComm enqueues vima_allgather_logits on
        out_ = parallel.all_gather_logits(logits, global_batch=B * world, comm=comm)
        e1.record()
        ag_events.append((e0, e1))
        return out_

    def sync():
        if not dry:
            torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            if not dry:
                torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        out = step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step(timed=True)
    if not dry:
        torch.cuda.synchronize(dev)
    dt_own = time.perf_counter() - t0          # this rank's own K steps, before the closing barrier
    sync()
    dt = time.perf_counter() - t0
    ranks_info = None
    if world > 1:
        ag_us = sum(a.elapsed_time(b) for a, b in ag_events) / max(len(ag_events), 1) * 1e3
        mine = torch.tensor([dt, dt_own, ag_us], dtype=torch.float64, device=dev)   # (gloo gathers host tensors in the dry run)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        allr = torch.stack(allr).cpu()
        dt = float(allr[:, 0].max())               # the contract: MAX over ranks of the barrier-bracketed time
        own_ms = (allr[:, 1] / args.steps * 1e3).tolist()
        ags = allr[:, 2].tolist()
        ranks_info = {"ms_per_step_own": [round(v, 3) for v in own_ms], "ms_per_step_own_min": round(min(own_ms), 3),
                      "ms_per_step_own_max": round(max(own_ms), 3), "slowest_rank": int(max(range(world), key=lambda r: own_ms[r])),
                      "allgather_us": [round(v, 1) for v in ags], "allgather_us_min": round(min(ags), 1), "allgather_us_max": round(max(ags), 1),
                      "note": "ms_per_step_own: each rank's K steps up to its own device synchronize (no barrier); allgather_us: HIP events around the "
                              "logits all-gather on its stream, mean over the timed steps (includes waiting for the slowest rank to arrive)"}
    assert out.shape == (B * world, 700) and bool(torch.isfinite(out).all())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"logits": out})
    ms_per_step = dt / args.steps * 1e3
    collective_info = None
    if rccl_log and rank == 0:
        collective_info = rccl_summary(rccl_log)
    if rccl_log:
        try:
            os.remove(rccl_log)          # summarised above: do not leave one log file per rank and run in /tmp
        except OSError:
            pass
    if dry:
        # every rank holds every rank's rows, in rank order
        want = (torch.arange(B, dtype=torch.float32)[None, :] + 1000.0 * torch.arange(world, dtype=torch.float32)[:, None]).reshape(-1)
        assert torch.equal(out[:, 0], want) and torch.equal(out[:, 699], want), "dry run: the gathered logits are not [rank 0 rows, rank 1 rows, ...]"
        calls = [None] * world
        dist.all_gather_object(calls, stub.calls)
        comm.close()
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0:
            assert all(c[:1] == ["create"] for c in calls[1:]) and calls[0][:2] == ["unique_id", "create"], calls
            assert all(c.count("all_gather") == args.steps + args.warmup for c in calls), calls
            print(json.dumps({"metric": "policy-forward steps/sec, VIMA-200M, 512-token prompt, batch 256", "value": None, "unit": "steps/s", "n_gpus": world,
                              "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "dry_run": True, "data": "synthetic",
                              "config": {"workload": "DRY RUN of bench.py's N > 1 host path on CPU: no GPU, no policy; NOT a measurement",
                                         "global_batch": B * world, "parallelism": f"dp{world}", "collective": collective, "state_dict": sd_source,
                                         "stub_calls_rank0": calls[0][:3] + ["..."] + calls[0][-1:], "ranks": ranks_info, "host_affinity": [host_affinity]}}))
        return

    warm_ms = inc_ms = float("nan")
    secondary = {}
    if args.full and not args.headline_only:
        warm_ms, inc_ms, secondary = extras(args, pol, syn, cfg, prompts, obs, past, sync, dev, rank, n_seg, Q, B, sd=sd)

    cold, warm = flops_per_sample(cfg.embed_dim, cfg.xf_n_layers, args.prompt_len, n_seg * Q, Q, T)
    peak = FP32_PEAK_TFLOPS if args.precision == "fp32" else BF16_PEAK_TFLOPS   # fp8w: fp8 weights are widened to bf16 in registers, the matrix op is the bf16 MFMA
    HBM_PEAK_GBS = 8000.0
    if not args.full:
        # a plain run: the whole step over its timed wall clock is all the roofline there is without runs of its own
        warm_roof = inc_roof = None
        ws_tflops = B * cold / (ms_per_step * 1e-3) / 1e12
        roofline = {"kernel": None, "bound": "mfma", "achieved": round(ws_tflops, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ws_tflops / peak, 4),
                    "traffic": None, "whole_step_tflops": round(ws_tflops, 2), "whole_step_frac": round(ws_tflops / peak, 4),
                    "note": "whole step: the algorithmic FLOPs of the cold step over the timed wall clock. The per-kernel and per-class figures, the HBM "
                            "traffic of the dominant kernel, the warm / incremental / other-batch / other-configuration steps and the CPU baseline "
                            "take runs of their own: --full"}
    else:
        # ---- per-class kernel time (HIP events on the launch stream), same workload, outside the timed region. The
        # two-stream software pipelining is switched off for this pass so that kernels do not overlap each other and the
        # event-bracketed durations are those of the kernels alone (what rocprofv3 --kernel-trace reports for the
        # committed profile, which is taken with --opt dual_stream=0 for the same reason).
        pol.set_option("dual_stream", 0)
        step()
        torch.cuda.synchronize(dev)
        pol.prof_enable(True)
        step()
        torch.cuda.synchronize(dev)
        gk = pol.prof_read_gemm_kernels()           # per KERNEL (the launcher's choice), before the class read resets the records
        if args.launch_log and rank == 0:
            json.dump([{k: e[k] for k in ("kernel", "M", "N", "K")} for e in pol.prof_read_gemm_launches()], open(args.launch_log, "w"))
        prof = pol.prof_read_ex()
        pol.prof_enable(False)

        # ---- HBM traffic of the dominant kernel: measured NOW when possible (two rocprofv3 --pmc passes over a subprocess of this same
        # workload), else the last committed summary -- the line says which
        global _LIVE_PMC
        traffic_source = "committed profiles/r*_pmc_traffic.json (not collected in this run)"
        default_workload = (world == 1 and args.model == "200M" and B == 256 and args.prompt_len == 512 and args.qv == 4 and args.words == 8
                            and T == 1 and args.precision == "bf16" and not args.opt)
        if args.live_pmc == "auto" and rank == 0 and default_workload and not args.headline_only:
            t_pmc = time.perf_counter()
            summ, why = live_pmc_traffic([])
            if summ is not None:
                _LIVE_PMC = summ
                traffic_source = f"{summ['source']} ({time.perf_counter() - t_pmc:.0f} s)"
            else:
                traffic_source = f"committed profiles/r*_pmc_traffic.json (live collection unavailable: {why})"

        g0, g3 = prof["gemm"], prof["gemm_residual"]

        def klass(d, name, peak=peak):
            if name.endswith(", true>"):
                peak = FP8_PEAK_TFLOPS           # fp8 e4m3 operands on v_mfma_scale_f32_32x32x64_f8f6f4: priced against the 5 PF dense fp8 peak
            tf = d["flops"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else 0.0
            gbs = d["bytes"] / (d["ms"] * 1e-3) / 1e9 if d["ms"] > 0 else 0.0
            inten = d["flops"] / d["bytes"] if d["bytes"] > 0 else 0.0
            hbm_bound = inten < peak * 1e12 / (HBM_PEAK_GBS * 1e9)       # below the machine balance (312 FLOP/B for bf16)
            return {"kernel": name, "bound": "hbm" if hbm_bound else "mfma",
                    "achieved": round(gbs if hbm_bound else tf, 2), "peak": HBM_PEAK_GBS if hbm_bound else peak,
                    "unit": "GB/s" if hbm_bound else "TFLOP/s",
                    "frac": round((gbs / HBM_PEAK_GBS) if hbm_bound else (tf / peak), 4),
                    "launches_per_step": d["launches"], "avg_launch_us": round(d["ms"] * 1e3 / max(d["launches"], 1), 2),
                    "ms_per_step": round(d["ms"], 3), "tflops": round(tf, 2), "algorithmic_gbs": round(gbs, 1),
                    "flop_per_byte": round(inten, 1), "algorithmic_mb_per_launch": round(d["bytes"] / max(d["launches"], 1) / 1e6, 1)}

        k_res = klass(g3, "vima::gemm_persistent_kernel<ACT_NONE, EPI 4 | EPI 3> (+ gemm_kernel fallbacks): the residual GEMMs (T5 o / wo and ViT "
                          "out_proj / c_proj with the stream in bf16: read + write 2 B per element, RMS partials; decoder: fp32 stream)")
        k_plain = klass(g0, "vima::gemm_persistent_kernel<*, EPI 1|2> / vima::gemm_kernel: all other GEMM launches (bf16-only output)")
        gemm_ms = g0["ms"] + g3["ms"]
        gemm_tflops = (g0["flops"] + g3["flops"]) / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        # the DOMINANT KERNEL (most time in the step), under the name rocprofv3 prints for it, with its own algorithmic flops /
        # bytes and its own counter traffic
        dom_name = max(gk, key=lambda k: gk[k]["ms"]) if gk else None
        roofline = klass(gk[dom_name], dom_name) if dom_name else dict(k_res if g3["ms"] >= g0["ms"] else k_plain)
        roofline.update({
            "traffic": pmc_traffic(dom_name) if dom_name else pmc_traffic(),
            "traffic_all_gemm_launches": pmc_traffic(),
            "traffic_source": traffic_source,
            "traffic_per_shape": ([{k: (round(v, 1) if isinstance(v, float) else v) for k, v in r.items()} for r in _LIVE_PMC["per_shape"][:12]]
                                  if _LIVE_PMC and _LIVE_PMC.get("per_shape") else None),
            "gemm_kernels": {k: {"ms_per_step": round(v["ms"], 3), "launches": v["launches"],
                                 "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ms"] > 0 else 0.0,
                                 "algorithmic_mb_per_launch": round(v["bytes"] / max(v["launches"], 1) / 1e6, 1)}
                             for k, v in sorted(gk.items(), key=lambda kv: -kv[1]["ms"])[:10]},
            "gemm_classes": [k_plain, k_res],
            "all_gemm": {"bound": "mfma", "achieved": round(gemm_tflops, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(gemm_tflops / peak, 4),
                         "launches_per_step": g0["launches"] + g3["launches"], "ms_per_step": round(gemm_ms, 3)},
            "gemm_ms_per_step": round(gemm_ms, 3), "attention_ms_per_step": round(prof["attention"]["ms"], 3),
            "other_ms_per_step": round(prof["other"]["ms"], 3),
            "whole_step_tflops": round(B * cold / (ms_per_step * 1e-3) / 1e12, 2),
            "whole_step_frac": round(B * cold / (ms_per_step * 1e-3) / 1e12 / peak, 4),
            "note": "per-class numbers: HIP events around every launch in a separate pass with dual_stream=0 (un-overlapped kernel "
                    "durations, what rocprofv3 --kernel-trace reports for the committed profile); achieved = ALGORITHMIC flops or bytes "
                    "(each operand / output / epilogue input once) over that time; `bound` from the kernel's flop/byte vs the 312 FLOP/B "
                    "machine balance; `kernel` = the kernel with the most time in the step; `traffic` = ITS HBM bytes per launch from the "
                    + ("rocprofv3 PMC passes collected live by this run" if _LIVE_PMC is not None else "committed rocprofv3 PMC passes (profiles/)")
                    + " (`traffic_source`; `traffic_all_gemm_launches`: average over all bf16 GEMM launches). "
                    "whole_step_*: the 49.09 TFLOP algorithmic numerator over the timed wall clock (the last ViT block is computed for the "
                    "cls token only -- executed GEMM FLOPs are ~6 % below the algorithmic count)",
        })

        # secondary rooflines: the WARM step (prompt reused: obs ViT + decoder against the cached prompt K/V +
        # action head) and the incremental env step are bound by the matrix pipe on their ~1.4 TFLOP and by HBM on the per-layer
        # K/V stream (B x Lp x 2E bf16 per decoder layer) + the weights; both bounds are reported, the larger one is the roofline
        def small_roofline(ms, flops):
            if not (ms == ms and ms > 0):
                return None
            kv_bytes = cfg.xf_n_layers * B * args.prompt_len * 2 * cfg.embed_dim * 2.0
            w_bytes = {"bf16": 676e6, "fp8w": 370e6, "fp8": 370e6, "fp32": 1352e6}[args.precision] * 0.45      # decoder + obs ViT + heads (no T5)
            t_mfma, t_hbm = flops / (peak * 1e12) * 1e3, (kv_bytes + w_bytes) / (HBM_PEAK_GBS * 1e9) * 1e3
            return {"bound": "hbm" if t_hbm > t_mfma else "mfma", "mfma_ms": round(t_mfma, 4), "hbm_ms": round(t_hbm, 4),
                    "roofline_ms": round(max(t_mfma, t_hbm), 4), "frac": round(max(t_mfma, t_hbm) / ms, 4),
                    "algorithmic_tflop": round(flops / 1e12, 3), "kv_stream_mb": round(kv_bytes / 1e6, 1)}

        # executed FLOPs of a WARM / incremental step: the per-layer prompt K/V projection (2 * Lp * 2E * E per sample and layer) is cached
        kv_proj_flops = cfg.xf_n_layers * 2.0 * args.prompt_len * 2 * cfg.embed_dim * cfg.embed_dim
        warm_roof = small_roofline(warm_ms, B * (warm - kv_proj_flops))
        inc_roof = small_roofline(inc_ms, B * (warm - kv_proj_flops))

    cpu_baseline = None
    if args.full and rank == 0 and not args.no_cpu_baseline:          # timed on rank 0's host cores, outside the timed region, for every N
        if affinity0 is not None and host_affinity.get("pinned"):
            os.sched_setaffinity(0, affinity0)          # the NUMA pin was for the GPU step; the CPU baseline gets the cores the process was given
        cpu_baseline = run_cpu_baseline(cfg, sd, n_seg, args.qv, args.cpu_batch, B, budget_s=20.0, words=args.words)
    affinities = [host_affinity]
    if world > 1:
        affinities = [None] * world
        dist.all_gather_object(affinities, host_affinity)

    if rank == 0:
        line = {
            "metric": "policy-forward steps/sec, VIMA-200M, 512-token prompt, batch 256",
            "value": round(world * args.steps / dt, 4), "unit": "steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": f"VIMA-{args.model} COLD policy forward (prompt assembly ViT+T5, obs ViT, XAttnGPT, action head) "
                                   f"batch {B}/GPU, {args.prompt_len}-token prompt ({n_seg} x [{args.words} words + 1 image]), {Q} object tokens/obs, T={T}",
                       "global_batch": B * world, "prompt_len": args.prompt_len, "parallelism": f"dp{world}", "collective": collective,
                       "collective_info": collective_info, "state_dict": sd_source,
                       "samples_per_s": round(world * B * args.steps / dt, 1),
                       "algorithmic_tflop_per_step_per_gpu": round(B * cold / 1e12, 2),
                       "warm_ms_per_step": round(warm_ms, 3) if warm_ms == warm_ms else None, "warm_steps_per_s": round(world * 1e3 / warm_ms, 2) if warm_ms == warm_ms else None,
                       "incremental_env_step_ms": round(inc_ms, 3) if inc_ms == inc_ms else None,
                       "warm_roofline": warm_roof, "incremental_roofline": inc_roof,
                       "secondary_cold": secondary,
                       "ranks": ranks_info, "host_affinity": affinities,
                       **({"shared_gpu_test": "all ranks on GPU 0 over gloo: exercises the launcher path, NOT a multi-GPU measurement"} if shared_gpu else {})},
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(line))
    if world > 1:
        if comm is not None:
            comm.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
