"""The gated chain's kernels (csrc/logodds_map.hip: k_hg_*) in the compiler's own report: no scratch memory, VGPRs within the
budget of their launch shape (512 / 256 / 128 at 256 / 512 / 1024 threads, as tests/test_matcher_kernel_resources.py holds the
matchers to), and the LDS of the kernels whose bodies they run -- k_hs_match_* and k_hector_cloud_container.  Resource
metadata only; no GPU needed (hipcc cross-compiles)."""
import pytest

import kernel_report

VGPR_BUDGET = {256: 512, 512: 256, 1024: 128}
TWINS = {"k_hg_match_reg": "k_hs_match_reg", "k_hg_match_fast": "k_hs_match_fast", "k_hg_cloud_container": "k_hector_cloud_container"}
INSTANCES = {"k_hg_match_reg": {(256, 5), (512, 3), (1024, 2)}, "k_hg_match_fast": {(256,), (512,), (1024,)},
             "k_hg_cloud_container": {()}}


@pytest.fixture(scope="module")
def report():
    want = set(TWINS) | set(TWINS.values())
    seen = {k: v.resources for k, v in kernel_report.report("logodds_map.hip").items() if k[0] in want or k[0].startswith("k_hg_")}
    for k in sorted(seen):
        print(k, seen[k])
    return seen


@pytest.mark.timeout(600)
def test_the_gated_kernels_are_exactly_these(report):
    for name, inst in INSTANCES.items():
        assert {k[1] for k in report if k[0] == name} == inst, (name, sorted(report))
    assert {k[0] for k in report if k[0].startswith("k_hg_")} == set(INSTANCES)


@pytest.mark.timeout(600)
def test_no_scratch_and_vgprs_within_the_launch_shape(report):
    for k, v in report.items():
        if not k[0].startswith("k_hg_"):
            continue
        assert v["ScratchSize"] == 0, (k, v)
        threads = k[1][0] if k[1] else 1024  # the container kernel is one block of 1024
        assert v["NumVgprs"] <= VGPR_BUDGET[threads], (k, v)


@pytest.mark.timeout(600)
def test_the_lds_of_the_ungated_twins(report):
    for hg, twin in TWINS.items():
        for inst in INSTANCES[hg]:
            assert report[(hg, inst)]["LDSByteSize"] == report[(twin, inst)]["LDSByteSize"], (hg, inst, report[(hg, inst)], report[(twin, inst)])
