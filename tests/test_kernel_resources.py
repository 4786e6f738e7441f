"""Register / scratch budget of the hot kernel, checked from the compiler's own report (no GPU needed: hipcc cross-compiles).

k_resp_rows keeps 66 packed accumulators live and is held to 128 VGPRs (4 waves per SIMD).  A spill to scratch memory does not
fail any parity test -- it costs ~3 % of the step and shows up as HBM write traffic (measured: 41 -> 107 MB per launch with
28 bytes of scratch per lane) -- so the budget is asserted here: every production instantiation (STATS = false, LDSB = false)
must report ScratchSize 0 and occupancy >= 4.
"""
import pytest

import kernel_report


@pytest.mark.timeout(900)
def test_hot_kernel_stays_out_of_scratch():
    seen = {k: v.resources for k, v in kernel_report.report("scan_matcher.hip").items() if k[0] == "k_resp_rows"}
    # <NXD, NYC, TILED, MFMA, STATS, LDSB>: production is STATS = false, LDSB = false
    production = {k: v for k, v in seen.items() if not k[1][4] and not k[1][5]}
    assert len(production) >= 5, seen  # <3,11,tiled>, <3,11,linear>, <4,8,tiled>, <4,8,linear>, <1,4,linear>
    for k, v in production.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 4, (k, v)
        assert v["NumVgprs"] <= 128, (k, v)
