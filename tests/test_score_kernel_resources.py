"""The pose-scoring kernels (csrc/logodds_map.hip: k_ms_*) stay out of scratch memory and within 128 VGPRs, read from the
compiler's own resource report (no GPU needed: hipcc cross-compiles; the file is compiled once for the module).

128 VGPRs: k_ms_score runs one wave per state, four states per block, and lives -- like k_gn_match_batch -- on four resident
waves per SIMD covering one another's round trips to L2 for the map cells; the other kernels are held to the same figure.
k_ms_score keeps nothing in LDS (no barrier: a state's result cannot depend on its neighbours in the block)."""
import pytest

import kernel_report

KERNELS = {("k_ms_score", (2,)), ("k_ms_score", (4,)), ("k_ms_score", (8,)), ("k_ms_score_ordered", ()), ("k_ms_best", ()),
           ("k_ms_cov", ())}
MAX_VGPRS = 128


@pytest.fixture(scope="module")
def report():
    seen = {k: v.resources for k, v in kernel_report.report("logodds_map.hip").items() if k[0].startswith("k_ms_")}
    for k in sorted(seen):
        print(k, seen[k])
    return seen


@pytest.mark.timeout(600)
def test_score_kernel_resources(report):
    assert set(report) == KERNELS, sorted(report)  # exactly the shipped kernels: no second partition rides along
    for k, v in report.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["NumVgprs"] <= MAX_VGPRS, (k, v)
    for waves in (2, 4, 8):
        k = ("k_ms_score", (waves,))
        assert report[k]["LDSByteSize"] == 0, (k, report[k])
