"""The synchronisation kernels (csrc/motion_sync.hip) stay out of scratch memory and use little LDS, read from the compiler's
own report in the device assembly (no GPU needed: hipcc cross-compiles).  Resource metadata only."""
import pytest

import kernel_report

KERNELS = {"k_msync_walk", "k_msync_windows", "k_msync_blank"}
LDS_BYTES = 1024  # "small": the kernels keep their state in registers and HBM


@pytest.mark.timeout(600)
def test_msync_kernels_use_no_scratch_and_little_lds():
    seen = {k: v.resources for k, v in kernel_report.report("motion_sync.hip").items()}
    print(seen)
    assert set(seen) == {(name, ()) for name in KERNELS}, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDSByteSize"] <= LDS_BYTES, (k, v)
