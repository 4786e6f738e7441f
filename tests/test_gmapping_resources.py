"""Every kernel of the GMapping count map (csrc/gmapping_map.hip) stays out of scratch memory, read from the compiler's own
report in the device assembly (no GPU needed: hipcc cross-compiles)."""
import pytest

import kernel_report

KERNELS = {"k_gm_endpoint", "k_gm_trace", "k_gm_hist", "k_gm_scan", "k_gm_scatter", "k_gm_fold", "k_gm_reset", "k_gm_classify"}


@pytest.mark.timeout(600)
def test_gmapping_kernels_use_no_scratch():
    seen = {k: v.resources for k, v in kernel_report.report("gmapping_map.hip").items() if k[0].startswith("k_gm_")}
    assert set(seen) == {(name, ()) for name in KERNELS}, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
