"""launch_gemm's kernel selection on the CPU: vima_amd/csrc/gemm_route.h (HIP-free) is compiled into tests/gemm_route_driver.cpp, a stand-alone
host program, under AddressSanitizer and UndefinedBehaviorSanitizer, run as a child process, and held to tests/golden/gemm_routes.json:

  routes       every row of tests/gemm_route_cases.rows(): the return class (0 / invalid / other) and GemmArgs::kernel_id that vima_op_gemm gave
               for it on an MI355X BEFORE gemm_route.h existed (one eligibility prefix per launcher, seven hand-kept predicates);
  predicates   gemm_pair_large, gemm_pair_ok, gemm_lnfold_producer_ok, gemm_dual_ok, gemm_a8_ok, gemm_grouped_ok and gemm_headmajor_ok (at
               (hm_D, hm_L) = (64, 256), (64, 512), (64, 128), (48, 256), each with a8 = 0 and 1), tabulated from the bodies they had then over
               M in {1, 32, 33, 255, 256, 2304, 2560, 16384, 32768, 131072} x N in {64, 96, 768, 1536, 2304, 3072, 4096} x
               K in {64, 128, 192, 256, 768, 3072} x leading dimensions {K, K + 8}, at default knobs and with each routing knob moved alone to
               every value gemm_forms_reference.SWEEP uses (plus gemm_res_maxwg 8 and gemm_q4 3).

Both are data recorded from the parent, none of it is what the code under test gives. fp8 operands (GemmArgs::a8 / w8) cannot be reached through
vima_op_gemm and so have no route rows: they are held by the gemm_a8_ok / gemm_headmajor_ok(a8 = 1) columns here, by tests/test_fp8_gpu.py and
by whole-model launch logs (profiles/gemm_route_launch_logs.txt)."""
import os
import subprocess

import pytest

from tests import gemm_route_cases as C
from tests.episode_driver import ROOT, build_driver


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory, "gemm_route_driver")


@pytest.fixture(scope="module")
def golden():
    return C.golden()


def _run(exe, lines):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VIMA_")}   # the knobs' process defaults are the built-in ones
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, env=env)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])   # a sanitizer report ends the program with a non-zero status
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def test_header_is_hip_free():
    for name in ("gemm_route.h", "gemm_args.h"):
        with open(os.path.join(ROOT, "vima_amd", "csrc", name)) as f:
            src = f.read()
        assert "#include <hip" not in src and "hipStream_t" not in src, name


def test_golden_rows_are_the_listed_rows(golden):
    """The table was recorded for exactly the rows the module lists (a row edited, added or dropped needs a new recording)."""
    assert golden["rows_sha1"] == C.rows_sha1(C.rows()) and len(golden["routes"]) == len(C.rows())
    assert len(golden["predicates"]) == len(C.predicate_knobs())
    for t in golden["predicates"]:
        assert sorted(t) == sorted(C.PREDICATES) and all(len(v) == len(C.predicate_grid()) for v in t.values())


def test_every_family_has_a_row(golden):
    seen = {kid // 1000 for rc, kid in golden["routes"] if rc == 0}
    assert set(C.FAMILIES) <= seen, sorted(set(C.FAMILIES) - seen)
    assert [g for r, g in zip(C.rows(), golden["routes"]) if r["opts"].get("gemm_tile") in (13, 14)] == [(0, 0), (0, 0)]


def test_route_of_every_row(driver, golden):
    rows = C.rows()
    got = _run(driver, C.driver_lines(rows, golden["num_cu"]))
    bad = [(r["name"], r["opts"], f"{rc} {kid}", g) for r, (rc, kid), g in zip(rows, golden["routes"], got) if g != f"{rc} {kid}"]
    assert not bad, f"{len(bad)} of {len(rows)} rows route differently (name, options, recorded, now): {bad[:10]}"


def test_predicates_over_the_grid(driver, golden):
    got = _run(driver, C.predicate_lines())
    G = len(C.predicate_grid())
    bad = []
    for i, (opts, t) in enumerate(zip(C.predicate_knobs(), golden["predicates"])):
        for c, name in enumerate(C.PREDICATES):
            now = "".join(ln[c] for ln in got[i * G:(i + 1) * G])
            if now != t[name]:
                j = next(k for k in range(G) if now[k] != t[name][k])
                bad.append((name, opts, C.predicate_grid()[j], t[name][j], now[j]))
    assert not bad, f"{len(bad)} predicate columns differ (predicate, options, first (M, N, K, ld), recorded, now): {bad[:10]}"
