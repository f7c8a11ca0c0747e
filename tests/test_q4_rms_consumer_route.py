"""Where the fused-RMSNorm consumers go (no GPU): gemm_route() through tests/gemm_route_driver.cpp, the stand-alone host program of
tests/test_gemm_route_build.py (same compilers, same sanitizer flags).

A consumer with 24 partials per row (E = 768), a bf16 output and neither bias nor residual takes the 256x384 four-wave tile's
row-scale form (kernel_id 19000 + (act + 1) * 10 + 7) wherever the four-wave kernel takes 256-row tiles at all: from 32 768 rows on at
default knobs. Option gemm_q4_rs = 0 (the driver has no column for it: environment variable VIMA_GEMM_Q4_RS, the knob's process default)
sends them back to gemm_pp_kernel, as does everything the form does not have."""
import os
import shutil
import subprocess

import pytest

from tests import gemm_route_cases as C
from tests.episode_driver import COMPILERS, FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCU = 256
PP_NONE, PP_RELU = 1011, 1021          # gemm_pp_kernel, bf16-output epilogue
Q4RS_NONE, Q4RS_RELU = 19017, 19027    # gemm_q4_kernel<ACT, 7, 2>
Q4_NONE = 19011                        # gemm_q4_kernel<0, 1, 2>


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("q4_rms_route") / "gemm_route_driver")
    errors = []
    for cc in COMPILERS:
        if not shutil.which(cc[0]):
            continue
        r = subprocess.run(cc + FLAGS + ["-I", os.path.join(ROOT, "vima_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_route_driver.cpp"), "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(" ".join(cc) + ":\n" + r.stderr[-2000:])
    raise AssertionError("no host compiler built the driver:\n" + "\n".join(errors))


def _routes(exe, rows, knob=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VIMA_")}
    if knob is not None:
        env["VIMA_GEMM_Q4_RS"] = str(knob)
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in C.driver_lines(rows, NCU)), capture_output=True, text=True, env=env)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(rows)
    return out


def consumer(name, M, N, act=0, parts=24, K=768, opts=None, ptrs=None, **ints):
    p = {"rs_ssq": 0}
    p.update(ptrs or {})
    return C.row(name, M, N, K, opts=opts, ptrs=p, act=act, rs_parts=parts, **ints)


def test_headline_consumers_take_the_four_wave_tile_by_default(driver):
    rows = [consumer("T5 q|k|v, half batch", 65536, 2304), consumer("T5 wi, half batch", 65536, 3072, act=C.R.ACT_RELU),
            consumer("T5 q|k|v, whole batch", 131072, 2304), consumer("32 768 rows", 32768, 2304)]
    assert _routes(driver, rows) == [f"0 {Q4RS_NONE}", f"0 {Q4RS_RELU}", f"0 {Q4RS_NONE}", f"0 {Q4RS_NONE}"]
    assert _routes(driver, rows, knob=1) == _routes(driver, rows)


def test_knob_off_and_small_problems_stay_on_the_ping_pong_kernel(driver):
    rows = [consumer("T5 q|k|v, half batch", 65536, 2304), consumer("T5 wi, half batch", 65536, 3072, act=C.R.ACT_RELU)]
    assert _routes(driver, rows, knob=0) == [f"0 {PP_NONE}", f"0 {PP_RELU}"]
    small = [consumer("below 32 768 rows", 32512, 2304), consumer("batch 32", 16384, 3072, act=C.R.ACT_RELU)]
    assert _routes(driver, small) == [f"0 {PP_NONE}", f"0 {PP_RELU}"]
    # gemm_q4 = 1: the tile wherever it fits (what the GPU test uses to reach it with small problems); the knob still holds
    forced = [consumer("12 288 rows at gemm_q4 1", 12288, 2304, opts={"gemm_q4": 1})]
    assert _routes(driver, forced) == [f"0 {Q4RS_NONE}"]
    assert _routes(driver, forced, knob=0) == [f"0 {PP_NONE}"]


def test_what_the_form_does_not_have_declines(driver):
    rows = [consumer("bf16 residual stream", 65536, 2304, ptrs={"resT": 0}),
            consumer("32 partials", 65536, 3072, parts=32, K=1024),
            consumer("12 partials", 65536, 2304, parts=12),
            consumer("bias", 65536, 2304, ptrs={"bias": 0}),
            consumer("QuickGELU", 65536, 3072, act=C.R.ACT_QUICKGELU),
            consumer("head-major", 65536, 2304, hm_D=64, hm_L=512)]
    got = _routes(driver, rows)
    assert not any(g.split()[1].startswith("19") for g in got), got
    assert got[1:5] == [f"0 {PP_NONE}", f"0 {PP_NONE}", f"0 {PP_NONE}", "0 1041"], got
    # ... and the plain forms of the tile are where they were
    plain = [C.row("no row scale", 65536, 2304, 768), consumer("128x384 tile", 16384, 2304, opts={"gemm_q4": 2})]
    assert _routes(driver, plain) == [f"0 {Q4_NONE}", "0 20011"]
    assert _routes(driver, plain, knob=0) == [f"0 {Q4_NONE}", "0 20011"]
