"""The cloud kernels of PL-ICP (csrc/plicp.hip) stay out of scratch memory and inside the LDS budget of the ranges kernels
(PlShared is shared and unchanged), read from the compiler's own report in the device assembly (no GPU needed: hipcc
cross-compiles).  Resource metadata only."""
import pytest

import kernel_report

WANT = {"k_plicp_match_clouds", "k_plicp_debug_clouds", "k_plicp_odom_clouds"}
LDS_BUDGET = 2048 * 63 + 1024  # tests/test_plicp_resources.py's, per reading 63 bytes


@pytest.mark.timeout(600)
def test_plicp_cloud_kernels_use_no_scratch_and_fit_the_lds_budget():
    rep = kernel_report.report("plicp.hip")
    seen = {k: v.resources for k, v in rep.items() if k[0] in WANT}
    print(seen)
    assert set(seen) == {(name, ()) for name in WANT}, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDSByteSize"] <= LDS_BUDGET, (k, v)
    ranges = {k[0]: v.resources["LDSByteSize"] for k, v in rep.items() if k[0] in {"k_plicp_match", "k_plicp_debug", "k_plicp_odom"}}
    assert {v["LDSByteSize"] for v in seen.values()} == set(ranges.values()) == {129680}, (seen, ranges)  # PlShared did not change
