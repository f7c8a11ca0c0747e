"""Compile-time resources (no GPU) of the fused-RMSNorm consumer form of the 256x384 four-wave tile, gemm_q4_kernel<ACT, 7, 2>: the form
holds four row scales per lane in VGPRs through the whole K loop, next to 128 accumulator, 80 fragment and 16 address registers, and parks
48 registers of row partials across the epilogue. The budget has no slack: one register too many and hipcc spills into the loop (every
reload drains the LDS-DMA stream) or moves accumulators between the register files. Shares the one device compile of gemm.hip with
tests/test_kernel_resources.py, whose test_q4_kernel_stream_is_what_was_written audits the loop body of every instantiation, these included."""
import os
import re
import shutil

import pytest

from tests.test_kernel_resources import HIPCC, _usage

FORMS = {0: "ACT_NONE", 1: "ACT_RELU"}   # the T5 q|k|v projection and the T5 feed-forward wi


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_rms_consumer_instantiations_fit_the_register_file():
    res = _usage("gemm.hip")
    seen = {}
    for k, v in res.items():
        m = re.search(r"gemm_q4_kernelILi(\d+)ELi7ELi(\d)E", k)
        if m:
            seen[(int(m.group(1)), int(m.group(2)))] = (k, v)
    assert sorted(seen) == [(act, 2) for act in sorted(FORMS)], sorted(seen)   # the 256x384 tile only; the 128x384 tile keeps its LDS form
    for (act, _), (k, v) in seen.items():
        assert v.get("ScratchSize", 0) == 0, (FORMS[act], k, v)
        assert v.get("AGPRs", 0) == 256, (FORMS[act], k, v)
        assert v.get("VGPRs", 0) <= 256, (FORMS[act], k, v)
        assert v.get("Occupancy", 0) == 1, (FORMS[act], k, v)
