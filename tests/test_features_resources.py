"""The corner-extraction kernel (csrc/features.hip) stays out of scratch memory and inside its LDS budget, read from the
compiler's own report in the device assembly (no GPU needed: hipcc cross-compiles).  Resource metadata only."""
import pytest

import kernel_report

KERNELS = {"features.hip": {"k_features"}}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("source", sorted(KERNELS))
def test_feature_kernels_use_no_scratch(source):
    want = {(name, ()) for name in KERNELS[source]}
    seen = {k: v.resources for k, v in kernel_report.report(source).items() if k[0] in KERNELS[source]}
    print(source, seen)
    assert set(seen) == want, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        # keys (u64, over v), c (float), map (u16), picked (u8) at max_scan_count = 1500 entries each, and the small counters
        assert v["LDSByteSize"] <= 1500 * (8 + 4 + 2 + 1) + 256, (k, v)
