"""bench.py on the GPU: a plain run measures the headline and nothing else, `--full` measures everything else after the same timed steps
(tiny model, so that both runs take seconds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "2M", "--batch", "4", "--prompt-len", "64", "--qv", "2", "--words", "4"]


def _run(extra, dump_dir):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + TINY + extra + ["--dump-outputs", str(dump_dir)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), np.load(os.path.join(dump_dir, "logits.npy"))


def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    plain, lp = _run([], tmp_path / "plain")
    full, lf = _run(["--full"], tmp_path / "full")
    for d in (plain, full):          # the headline fields say the same in both
        assert d["metric"] == "policy-forward steps/sec, VIMA-200M, 512-token prompt, batch 256" and d["unit"] == "steps/s"
        assert d["higher_is_better"] is True and d["dtype"] == "bf16" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
        assert d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-2          # value = 1 / (seconds per step) on one GPU
    # plain: nothing that takes a run of its own
    assert plain["cpu_baseline"] is None and plain["config"]["secondary_cold"] == {}
    assert plain["config"]["warm_ms_per_step"] is None and plain["config"]["incremental_env_step_ms"] is None
    assert plain["roofline"]["kernel"] is None and plain["roofline"]["traffic"] is None and "gemm_kernels" not in plain["roofline"]
    assert plain["roofline"]["whole_step_tflops"] > 0
    # --full: the extras, the profile pass and the CPU baseline, as before
    assert full["cpu_baseline"] is not None and full["cpu_baseline"]["cores"] >= 1 and full["cpu_baseline"]["value"] > 0
    assert full["config"]["warm_ms_per_step"] > 0 and full["config"]["incremental_env_step_ms"] > 0
    assert full["config"]["secondary_cold"]["batch_1"]["ms_per_step"] > 0
    assert full["roofline"]["gemm_kernels"] and full["roofline"]["gemm_ms_per_step"] > 0 and full["roofline"]["whole_step_tflops"] > 0
    # the timed steps and what --dump-outputs writes are the same with and without --full
    assert lp.shape == (4, 700) and lp.dtype == np.float32 and np.isfinite(lp).all()
    assert np.array_equal(lp, lf)
