"""The ray cast's kernels (csrc/raycast.hip: k_rc_*) stay out of scratch memory.  Read from the compiler's own report in the
device assembly (no GPU needed: hipcc cross-compiles).  Resource metadata only."""
import pytest

import kernel_report

KERNELS = {"k_rc_cells", "k_rc_rays", "k_rc_scans"}


@pytest.fixture(scope="module")
def report():
    seen = {k: v.resources for k, v in kernel_report.report("raycast.hip").items()}
    for k in sorted(seen):
        print(k, seen[k])
    return seen


@pytest.mark.timeout(600)
def test_raycast_kernels_use_no_scratch(report):
    assert set(report) == {(name, ()) for name in KERNELS}, sorted(report)
    for k, v in report.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDSByteSize"] == 0, (k, v)   # rays share nothing: the walk needs no LDS either
