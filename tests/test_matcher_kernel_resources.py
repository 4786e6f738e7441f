"""The Gauss-Newton matcher's kernels and the streamed processor's (csrc/logodds_map.hip) stay out of scratch memory and within
the registers their launch shape is meant for, read from the compiler's own resource report (no GPU needed: hipcc
cross-compiles; the file is compiled ONCE for the module).

Bounds, from the launch shape and not from what the compiler happened to produce:
  scratch  0 bytes, every kernel
  VGPRs    a gfx950 SIMD holds 512 VGPRs per lane and a block of NT threads puts NT / 256 waves on each of a CU's four SIMDs,
           so a kernel launched with __launch_bounds__(NT) must fit 512 / (NT / 256) VGPRs per wave: 512 at 256 threads, 256
           at 512, 128 at 1024 (k_gn_match and k_gn_match_batch_ordered are bounded at 1024).  k_gn_match_batch (256
           threads, one wave per entry) is held to 128: four waves per SIMD stay resident -- the kernel lives on other waves
           covering a wave's L2 round trips.  The update kernels (256 threads) are held to 128, the four resident waves per
           SIMD the two-kernel update is written for.
  LDS      k_gn_match_batch (no barrier), k_hs_mark, k_hs_apply: none.  A streamed k_hs_match_*<NT> runs the matcher body of
           its single-call twin k_gn_match_*<NT> and nothing else in LDS: the same bytes, i.e. one partial-sum buffer each.
           The ordered kernels keep nine terms per point, sized at launch, and are not bound here."""
import pytest

import kernel_report

BY_THREADS = {256: 512, 512: 256, 1024: 128}
FORMS = {"reg": [(256, 5), (512, 3), (1024, 2)], "fast": [(256,), (512,), (1024,)]}  # <NT, PMAX> and <NT>, as instantiated


def forms(prefix):
    return {("%s_%s" % (prefix, f), args): BY_THREADS[args[0]] for f, each in FORMS.items() for args in each}


BATCH = {("k_gn_match_batch", ()): 128, ("k_gn_match_batch_ordered", ()): 128}
SINGLE = {("k_gn_match", ()): 128, **forms("k_gn_match")}
STREAMED = {**forms("k_hs_match"), ("k_hs_mark", ()): 128, ("k_hs_apply", ()): 128}


@pytest.fixture(scope="module")
def report():
    """(kernel, template arguments) -> {ScratchSize, NumVgprs, LDSByteSize, ...} of every k_gn_match* and k_hs_* kernel of the
    file."""
    return {k: v.resources for k, v in kernel_report.report("logodds_map.hip").items() if k[0].startswith(("k_gn_match", "k_hs_"))}


def hold(seen, budget, prefix):
    mine = {k: v for k, v in seen.items() if k[0].startswith(prefix)}
    assert set(mine) == set(budget), mine  # exactly the shipped kernels: no second partition rides along
    for k, v in mine.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["NumVgprs"] <= budget[k], (k, v)


@pytest.mark.timeout(600)
def test_gn_batch_kernel_resources(report):
    hold(report, BATCH, "k_gn_match_batch")
    assert report[("k_gn_match_batch", ())]["LDSByteSize"] == 0, report


@pytest.mark.timeout(600)
def test_streamed_processor_kernel_resources(report):
    hold(report, STREAMED, "k_hs_")
    for k in ("k_hs_mark", "k_hs_apply"):
        assert report[(k, ())]["LDSByteSize"] == 0, report


@pytest.mark.timeout(600)
def test_single_match_kernel_resources(report):
    hold({k: v for k, v in report.items() if not k[0].startswith("k_gn_match_batch")}, SINGLE, "k_gn_match")


@pytest.mark.timeout(600)
def test_streamed_match_keeps_one_partial_sum_buffer(report):
    for form, each in FORMS.items():
        for args in each:
            hs, gn = report[("k_hs_match_" + form, args)], report[("k_gn_match_" + form, args)]
            assert hs["LDSByteSize"] == gn["LDSByteSize"], (form, args, hs, gn)
