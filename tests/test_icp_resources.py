"""The ICP kernels (csrc/icp.hip) stay out of scratch memory and inside their LDS budget, read from the compiler's own report
in the device assembly (no GPU needed: hipcc cross-compiles).  Resource metadata only."""
import pytest

import kernel_report

WANT = {"k_icp_cloud", "k_icp_match", "k_icp_debug"}
# per point (2048 of them): the target x, y in fp64 16, the source x, y in float32 8, the correspondence in 16 bits 2, the
# source's takes-part byte 1 = 27 bytes; and the reduction scratch (4 waves x 8 doubles), rounded up to 1 KB
LDS_BUDGET = 2048 * 27 + 1024
assert LDS_BUDGET <= 64 * 1024   # two pairs fit a CU's 160 KB with room to spare


@pytest.mark.timeout(600)
def test_icp_kernels_use_no_scratch_and_fit_their_lds_budget():
    want = {(name, ()) for name in WANT}
    seen = {k: v.resources for k, v in kernel_report.report("icp.hip").items() if k[0] in WANT}
    print(seen)
    assert set(seen) == want, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDSByteSize"] <= LDS_BUDGET, (k, v)
    assert seen[("k_icp_cloud", ())]["LDSByteSize"] == 0
