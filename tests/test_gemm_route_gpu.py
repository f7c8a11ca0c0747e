"""The rows of tests/gemm_route_cases.py through vima_op_gemm on the built library: the return class and GemmArgs::kernel_id of every row are
the ones recorded in tests/golden/gemm_routes.json (on an MI355X, before kernel selection moved into vima_amd/csrc/gemm_route.h). The buffers are
allocated here at the rows' sizes; their contents do not matter to routing. The two lab tiles (gemm_tile 13 / 14) report kernel_id 0 and must
keep doing so. fp8 operands are not reachable through this entry: see tests/test_gemm_route_build.py."""
import pytest

from tests import gemm_route_cases as C

pytestmark = pytest.mark.gpu


def test_recorded_route_of_every_row():
    golden, rows = C.golden(), C.rows()
    assert golden["rows_sha1"] == C.rows_sha1(rows)
    assert golden["num_cu"] == C.num_cu(), "the table was recorded on another CU count: the round-counting rules would differ"
    got = C.launch_rows(rows)
    bad = [(r["name"], r["opts"], want, g) for r, want, g in zip(rows, golden["routes"], got) if g != want]
    assert not bad, f"{len(bad)} of {len(rows)} rows route differently (name, options, recorded, now): {bad[:10]}"
    assert [g for r, g in zip(rows, got) if r["opts"].get("gemm_tile") in (13, 14)] == [(0, 0), (0, 0)]
