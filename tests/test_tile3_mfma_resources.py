"""Register / scratch budget of the MFMA forms of the fine response kernel on the 4x4 blocks (LSLAM_OPT_FINE_MFMA), from the
compiler's own report (no GPU needed: hipcc cross-compiles), and the instructions the form exists for -- and exists to avoid.

k_resp_tile3<kTile3Angles, MFMA = true> keeps one int32x4 accumulator per angle and sums it with two row swaps.  The packed
forms run at 8 waves per SIMD (54 VGPRs for three angles), and the MFMA forms must not lose that residency; they sum on the
matrix pipe, at least once per angle of the group, and nothing of the packed reduction (v_readlane_b32 after DPP adds) is left
in them.  The packed forms stay what they were: no MFMA."""
import pytest

import kernel_report

OPS = ("v_mfma_i32_16x16x64_i8", "v_readlane_b32", "v_permlane32_swap_b32", "v_permlane16_swap_b32")

@pytest.mark.timeout(900)
def test_fine_mfma_forms():
    # k_resp_tile3<kTile3Angles, MFMA>, keyed (angles, mfma)
    tile3 = {k[1]: v for k, v in kernel_report.report("scan_matcher.hip").items() if k[0] == "k_resp_tile3"}
    seen = {k: v.resources for k, v in tile3.items()}
    count = {k: {op: v.ops[op] for op in OPS} for k, v in tile3.items()}
    mfma = {k: v for k, v in seen.items() if k[1]}
    packed = {k: v for k, v in seen.items() if not k[1]}
    # one angle per wave (192 .. 1535 scans) and the grouped form, each in both forms
    assert len(mfma) == 2 and (1, True) in mfma and len(packed) == 2 and (1, False) in packed, seen
    for k, v in mfma.items():
        c = count[k]
        assert v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 8, (k, v)
        assert c["v_mfma_i32_16x16x64_i8"] >= k[0], (k, c)
        assert c["v_readlane_b32"] == 0, (k, c)
        # the epilogue: one pair of row swaps per angle at least
        assert c["v_permlane32_swap_b32"] >= k[0] and c["v_permlane16_swap_b32"] >= k[0], (k, c)
    for k, v in packed.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 8, (k, v)
        assert count[k]["v_mfma_i32_16x16x64_i8"] == 0, (k, count[k])
