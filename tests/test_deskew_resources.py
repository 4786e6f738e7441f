"""The de-skew kernels (csrc/deskew.hip) and the cloud -> container kernel (csrc/logodds_map.hip) stay out of scratch memory,
read from the compiler's own report in the device assembly (no GPU needed: hipcc cross-compiles).  Resource metadata only."""
import pytest

import kernel_report

KERNELS = {"deskew.hip": {"k_deskew", "k_deskew_batch", "k_deskew_angles"},
           "logodds_map.hip": {"k_hector_cloud_container", "k_hector_project"}}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("source", sorted(KERNELS))
def test_deskew_kernels_use_no_scratch(source):
    want = {(name, ()) for name in KERNELS[source]}
    seen = {k: v.resources for k, v in kernel_report.report(source).items() if k[0] in KERNELS[source]}
    print(source, seen)
    assert set(seen) == want, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
