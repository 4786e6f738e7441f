"""The localiser's kernels (csrc/hector_loc_impl.hpp, compiled into csrc/logodds_map.hip: k_hl_container, k_hl_track_*) from the
compiler's own report in the device assembly (no GPU needed: hipcc cross-compiles): no scratch memory, and the static LDS of a
tracking kernel is that of the fleet's matcher of the same instantiation -- the waves' partial sums -- so the staged form's
dynamic 56 KiB (gn_form_of) stays what the existing form uses, plus nothing.  The VGPRs and waves per SIMD of k_hl_track_* are
printed beside those of k_hf_match_* of the same NT (pytest -s); DESIGN.md 4.26 says why the looping kernel holds more.
Resource metadata only."""
import pytest

import kernel_report

TRACK = {"k_hl_track_reg": "k_hf_match_reg", "k_hl_track_fast": "k_hf_match_fast"}
INSTANCES = {"k_hl_track_reg": {(256, 5), (512, 3), (1024, 2)}, "k_hl_track_fast": {(256,), (512,), (1024,)}}
STAGED_LDS = 56 * 1024  # gn_form_of's bound on the staged points


@pytest.fixture(scope="module")
def report():
    want = {"k_hl_container"} | set(TRACK) | set(TRACK.values())
    seen = {k: v.resources for k, v in kernel_report.report("logodds_map.hip").items() if k[0] in want}
    return seen


@pytest.mark.timeout(600)
def test_localiser_kernels_use_no_scratch_and_no_more_lds(report):
    names = {k[0] for k in report}
    assert {"k_hl_container"} | set(TRACK) <= names, names
    for name, inst in INSTANCES.items():
        assert {k[1] for k in report if k[0] == name} == inst, (name, sorted(report))
    for k, v in report.items():
        if k[0].startswith("k_hl_"):
            assert v["ScratchSize"] == 0, (k, v)
    for hl, hf in TRACK.items():
        for inst in INSTANCES[hl]:
            a, b = report[(hl, inst)], report[(hf, inst)]
            print("%s%s: %d VGPRs, %d waves per SIMD, %d B static LDS | %s: %d VGPRs, %d waves per SIMD, %d B" % (
                hl, inst, a["NumVgprs"], a["Occupancy"], a["LDSByteSize"], hf, b["NumVgprs"], b["Occupancy"], b["LDSByteSize"]))
            assert a["LDSByteSize"] == b["LDSByteSize"], (hl, inst)   # the staged form adds its dynamic 56 KiB to the same
            assert a["LDSByteSize"] + STAGED_LDS <= 64 * 1024, (hl, inst)  # within a launch's default dynamic limit
            assert a["Occupancy"] >= 1
