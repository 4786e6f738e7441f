"""The PL-ICP kernels (csrc/plicp.hip) stay out of scratch memory and inside their LDS budget, read from the compiler's own
report in the device assembly (no GPU needed: hipcc cross-compiles).  Resource metadata only."""
import pytest

import kernel_report

WANT = {"k_plicp_match", "k_plicp_debug", "k_plicp_odom"}
# per reading (2048 of them): ref and sens points 4 x 8, the distance 8, the doubles' minimum / the survivors' distances 8, the
# owner / rank 4, five 16-bit index arrays 10, the flag byte 1 = 63 bytes; and the reduction scratch and counters
LDS_BUDGET = 2048 * 63 + 1024


@pytest.mark.timeout(600)
def test_plicp_kernels_use_no_scratch_and_fit_their_lds_budget():
    want = {(name, ()) for name in WANT}
    seen = {k: v.resources for k, v in kernel_report.report("plicp.hip").items() if k[0] in WANT}
    print(seen)
    assert set(seen) == want, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDSByteSize"] <= LDS_BUDGET, (k, v)
