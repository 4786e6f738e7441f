"""The coarse reduce's 128-thread form (k_reduce_coarse_lds<128>, batches of 2048 scans and more) is built around residency:
8 waves per SIMD = 16 blocks of 2 waves per CU, so that the 4096 blocks of the headline batch are resident in one round on
256 CUs.  Each of three resources has to admit that, and each is read here from the compiler's own report (no GPU needed:
hipcc cross-compiles; the file is compiled ONCE for the module):

  VGPRs    <= 64   a gfx950 SIMD holds 512 per lane, allocated in granules of 8: 512 / 64 = 8 waves
  SGPRs    <= 80   8 waves per SIMD are admitted up to 80 (800 / (ceil(sgprs / 16) * 16 + 16) >= 8)
  scratch  0       a spill on the common path costs more than the residency buys
  LDS      static + dynamic <= 160 KiB / 16 = 10 240 B per block at the headline geometry (11 x 11 x 21, baseline_config);
           the dynamic bytes come from the library (lslam_debug_reduce_lds_bytes: the same ReduceLds the launch is sized with)

The 256- and 1024-thread forms (small batches, the lone MatchScan) share the block function; they keep their own register
regime and are held to no scratch."""
import ctypes as C

import pytest

import kernel_report

LDS_PER_CU = 160 * 1024
BLOCKS_PER_CU = 16  # 8 waves per SIMD x 4 SIMDs / 2 waves per block


@pytest.fixture(scope="module")
def report():
    """(NT,) -> {ScratchSize, NumVgprs, TotalNumSgprs, LDSByteSize, ...} of k_reduce_coarse_lds<NT>"""
    return {k[1]: v.resources for k, v in kernel_report.report("scan_matcher.hip").items() if k[0] == "k_reduce_coarse_lds"}


@pytest.mark.timeout(600)
def test_the_three_forms_are_built(report):
    assert set(report) == {(128,), (256,), (1024,)}, report


@pytest.mark.timeout(600)
def test_narrow_form_fits_eight_waves_per_simd(report):
    r = report[(128,)]
    assert r["ScratchSize"] == 0, r
    assert r["NumVgprs"] <= 64, r
    assert r["TotalNumSgprs"] <= 80, r


@pytest.mark.timeout(600)
def test_narrow_form_lds_admits_sixteen_blocks_per_cu(report):
    from lslam_amd import api

    L = api.lib()
    cfg = api.baseline_config()
    dims = (C.c_int * 3)()
    dyn = L.lslam_debug_reduce_lds_bytes(C.byref(cfg), 128, C.byref(dims))
    assert list(dims) == [11, 11, 21], list(dims)  # the headline geometry
    assert dyn > 0
    static = report[(128,)]["LDSByteSize"]
    assert static + dyn <= LDS_PER_CU // BLOCKS_PER_CU, (static, dyn)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("nt", [256, 1024])
def test_wide_forms_stay_out_of_scratch(report, nt):
    assert report[(nt,)]["ScratchSize"] == 0, report
