"""The live map's kernels (csrc/livemap.hip) stay out of scratch memory and within the registers / LDS their 256-thread
launch bounds are meant for, read from the compiler's own resource report (no GPU needed: hipcc cross-compiles).

Bounds, from the launch shape and not from what the compiler happened to produce:
  scratch  0 bytes, every kernel
  VGPRs    <= 128: a gfx950 SIMD holds 512 per lane, so four waves per SIMD stay resident -- four whole 256-thread blocks
           per CU, enough to hide the latency of the counter atomics
  LDS      k_live_box: one record per wave of the block (the scan's box, 4 doubles, and the largest x and y its rays
           reach, 2 doubles) = 4 waves x 6 doubles = 192 bytes; the trace and regrid kernels use none (the beams of a wave
           travel by lane shuffles)"""
import pytest

import kernel_report

LDS = {"k_live_box": 4 * 6 * 8, "k_live_trace": 0, "k_live_regrid": 0}


@pytest.mark.timeout(600)
def test_livemap_kernel_resources():
    seen = {k: v.resources for k, v in kernel_report.report("livemap.hip").items() if k[0].startswith("k_live_")}
    assert set(seen) == {(name, ()) for name in LDS}, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["NumVgprs"] <= 128, (k, v)
        assert v["LDSByteSize"] == LDS[k[0]], (k, v)
