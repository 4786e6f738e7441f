"""Register / scratch budget of the MFMA forms of the coarse response kernel (LSLAM_OPT_ROWS_MFMA), from the compiler's own
report (no GPU needed: hipcc cross-compiles), and the instruction the form exists for.

k_resp_rows<NXD, NYC, TILED, MFMA = true, STATS, LDSB> and k_resp_rows_mw<NXD, NYC, WAVES, MFMA = true> keep one int32x4
accumulator per lattice row; like the packed forms (test_kernel_resources.py) they are held to 4 waves per SIMD without scratch,
the instrumented twins included.  The default body, <3, 11, tiled>, must really sum on the matrix pipe."""
import pytest

import kernel_report


@pytest.mark.timeout(900)
def test_mfma_forms_stay_out_of_scratch():
    # k_resp_rows<NXD, NYC, TILED, MFMA, STATS, LDSB> and k_resp_rows_mw<NXD, NYC, WAVES, MFMA>
    seen = {k: v for k, v in kernel_report.report("scan_matcher.hip").items() if k[0] in ("k_resp_rows", "k_resp_rows_mw")}
    mfma = {k: v.ops["v_mfma_i32_16x16x64_i8"] for k, v in seen.items() if v.ops["v_mfma_i32_16x16x64_i8"]}
    rows = {k: v.resources for k, v in seen.items() if k[0] == "k_resp_rows" and k[1][3] and not k[1][5]}
    multi = {k: v.resources for k, v in seen.items() if k[0] == "k_resp_rows_mw" and k[1][3]}
    # <3,11> and <4,8>, tiled and linear, each with its instrumented twin; <3,11> and <4,8> at 2, 4 and 8 waves per block
    assert len(rows) == 8 and len(multi) == 6, sorted(seen)
    for k, v in {**rows, **multi}.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 4, (k, v)
        assert v["NumVgprs"] <= 128, (k, v)
        assert mfma.get(k, 0) >= 1, k
    # the default body: every inlined drain sums its 11 lattice rows with one MFMA each
    default = ("k_resp_rows", (3, 11, True, True, False, False))
    assert mfma[default] >= 11, (default, mfma[default])
    # and no packed form picked the instruction up
    assert not [k for k in mfma if k not in rows and k not in multi], mfma
