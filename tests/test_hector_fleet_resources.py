"""The fleet's kernels (csrc/logodds_map.hip: k_hf_*) stay out of scratch memory, and taking the member from the grid and its
arguments from the fleet's tables costs the matcher no occupancy: every k_hf_match_* instantiation keeps at least the waves per
SIMD of its k_hs_match_* counterpart in the same compile.  Read from the compiler's own report in the device assembly (no GPU
needed: hipcc cross-compiles).  Resource metadata only."""
import pytest

import kernel_report

PLAIN = {"k_hf_project", "k_hf_mark", "k_hf_apply"}
MATCH = {"k_hf_match_reg": "k_hs_match_reg", "k_hf_match_fast": "k_hs_match_fast"}
INSTANCES = {"k_hf_match_reg": {(256, 5), (512, 3), (1024, 2)}, "k_hf_match_fast": {(256,), (512,), (1024,)}}


@pytest.fixture(scope="module")
def report():
    want = PLAIN | set(MATCH) | set(MATCH.values())
    seen = {k: v.resources for k, v in kernel_report.report("logodds_map.hip").items() if k[0] in want}
    for k in sorted(seen):
        print(k, seen[k])
    return seen


@pytest.mark.timeout(600)
def test_fleet_kernels_use_no_scratch(report):
    names = {k[0] for k in report}
    assert PLAIN | set(MATCH) <= names, names
    for name, inst in INSTANCES.items():
        assert {k[1] for k in report if k[0] == name} == inst, (name, sorted(report))
    for k, v in report.items():
        if k[0].startswith("k_hf_"):
            assert v["ScratchSize"] == 0, (k, v)


@pytest.mark.timeout(600)
def test_fleet_matchers_keep_the_single_matchers_occupancy(report):
    for hf, hs in MATCH.items():
        for inst in INSTANCES[hf]:
            assert report[(hf, inst)]["Occupancy"] >= report[(hs, inst)]["Occupancy"], (hf, inst, report[(hf, inst)], report[(hs, inst)])
