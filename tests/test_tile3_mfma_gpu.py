"""The MFMA sums of the fine response kernel on the 4x4 blocks (set_option('fine_mfma', 1): k_resp_tile3 sums each beam's 3x3
patch bytes with v_mfma_i32_16x16x64_i8 against a one-hot operand) against the packed form (fine_mfma 0) and the oracle.

Every numerator comparison is np.array_equal on ALL numerators of fine_sums_batch -- integer sums, no tolerance --: option on
against option off over the whole batch, with identical centres, and 24 seeded scans per case against the oracle's lattice
(kor_correlate_scan, want_sums) centred on the returned centres.  fine_mfma_launches shows which sums took each launch;
coarse_form_launches() names the form (fine_tile3), the same for both.  The i8 MFMA reads signed bytes: a grid with a byte
above 127 must fall back to the packed form on its own.

Two batch sizes: 192 scans (the first multiple of 8 with S * 11 >= kTileMinWaves: one angle per wave) and 1536
(kTile3ManyMinScans: the grouped form)."""
import math

import numpy as np
import pytest

from lslam_amd import api, synth

from test_matcher_gpu import make_pair
from test_rows_mfma_gpu import _asymmetric_grid
from test_rows_wave_edges_gpu import N_CHECK, S_TILE3, _batch, _drawn, _launched

pytestmark = pytest.mark.gpu

S_ONE = 192  # 192 * 11 = 2112 >= kTileMinWaves (2048); 184 * 11 = 2024 is not
SIZES = [S_ONE, S_TILE3]
COARSE_ANGLE_RES = 0.0349
FINE_RES = 0.00349  # baseline_config: 11 fine angles


def _fine(gm, ranges, poses, on, takes_mfma=None):
    """fine_sums_batch with the option set; asserts the form and which sums took its launches."""
    takes_mfma = bool(on) if takes_mfma is None else takes_mfma
    gm.set_option("fine_mfma", on)
    assert gm.get_option("fine_mfma") == on
    before, n0 = gm.coarse_form_launches(), gm.fine_mfma_launches
    fine, centers = gm.fine_sums_batch(ranges, poses)
    ran = _launched(gm, before)
    assert ran.get("fine_tile3", 0) >= 1 and "fine_rows" not in ran, ran
    assert gm.fine_mfma_launches - n0 == (ran["fine_tile3"] if takes_mfma else 0)
    return fine, centers


def _against_oracle(port, fine, centers, ranges, poses, check, fine_res=FINE_RES, need_nonzero=True):
    n_nonzero = 0
    for q in check:
        assert not np.isnan(centers[q]).any(), q
        _, _, _, st, want = port.correlate_scan(ranges[q], poses[q], centers[q], 0.05, 0.05, 0.5 * COARSE_ANGLE_RES, fine_res,
                                                True, True, want_sums=True)
        assert st == 0, q
        assert fine[q].shape == want.shape and np.array_equal(fine[q], want), q
        n_nonzero += int(want.any())
    if need_nonzero:
        assert n_nonzero >= N_CHECK // 2  # a kernel that returns zeros does not pass


def _on_off_oracle(port, gm, ranges, poses, check, fine_res=FINE_RES, skip=()):
    """fine_mfma 1 against 0 on every numerator of the batch (but the scans of `skip`: no lattice, no numerators), with
    identical centres, and the drawn scans against the oracle."""
    on, c_on = _fine(gm, ranges, poses, 1)
    off, c_off = _fine(gm, ranges, poses, 0)
    gm.set_option("fine_mfma", 1)
    assert np.array_equal(c_on, c_off, equal_nan=True)
    keep = np.setdiff1d(np.arange(len(ranges)), np.asarray(skip, dtype=int))
    assert on.shape == off.shape and on.shape[0] == len(ranges) and on[keep].any()
    assert np.array_equal(on[keep], off[keep])
    _against_oracle(port, on, c_on, ranges, poses, check, fine_res)
    return on, c_on


@pytest.fixture(scope="module")
def pair(ctx, oracle_lib, workload_spread):
    wl = workload_spread
    port, gm = make_pair(ctx, oracle_lib)
    port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
    gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
    yield port, gm, wl
    gm.close()
    port.close()


def test_default_follows_the_keep_rule(pair):
    """The measured default (profiles/r10/README.md)."""
    assert pair[1].get_option("fine_mfma") == 1


@pytest.mark.parametrize("S", SIZES)
def test_empty_scan_one_reading_and_a_lattice_outside(pair, S):
    """Scan 0 has no finite reading: zero operands in every MFMA, all numerators zero.  Scan 1 has one finite reading: one
    lane of one block of beams carries a patch.  Scan 2's lattice leaves the grid: no centre, and the others are unaffected."""
    port, gm, wl = pair
    assert gm.num_beams == 1081
    ranges, poses = _batch(wl, S, 300 + S)
    ranges[0] = np.nan
    ranges[1] = np.nan
    ranges[1, 517] = 3.0
    poses[2, 0] += 500.0
    fine, centers = _on_off_oracle(port, gm, ranges, poses, _drawn(S, 301 + S, always=(0, 1), never=(2,)), skip=(2,))
    assert fine.shape[1:] == (3, 3, 11)
    assert not fine[0].any()
    assert np.isnan(centers[2]).all() and not np.isnan(np.delete(centers, 2, axis=0)).any()


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("n_beams", [64, 65, 1081])
def test_beam_counts(ctx, oracle_lib, n_beams, S):
    """64 beams: one full block; 65: a last block of one lane; 1081: 17 blocks, the last of 57 lanes.  The trip count is the
    wave's, and the lanes beyond the last beam bring zero operands."""
    laser = synth.Laser(n_ranges=n_beams, angle_increment=math.radians(270.0) / n_beams)
    port, gm = make_pair(ctx, oracle_lib, laser)
    try:
        wl = synth.make_match_workload(n_base=12, n_query=12, seed=310 + n_beams % 7, laser=laser, query_spread=1.5)
        port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
        gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
        assert gm.num_beams == n_beams
        ranges, poses = _batch(wl, S, 311 + n_beams + S)
        ranges[3, :-1] = np.nan  # only the LAST beam of the scan readable: all that the last block brings
        if not np.isfinite(ranges[3, -1]):
            ranges[3, -1] = 4.0
        _on_off_oracle(port, gm, ranges, poses, _drawn(S, 312 + n_beams + S, always=(3,)))
    finally:
        gm.close()
        port.close()


@pytest.mark.parametrize("n_fine", [10, 11, 12, 13])
def test_fine_angle_groups(ctx, oracle_lib, workload_spread, n_fine):
    """The grouped form at its smallest batch with 10, 11, 12 and 13 fine angles: last groups of every size (three angles
    per wave: 1, 2, full, 1; four: 2, 3, full, 1).  An angle past the last one is not computed, and nothing is stored for it."""
    wl = workload_spread
    fine_res = COARSE_ANGLE_RES / (n_fine - 1)  # the fine pass spans +- half a coarse angle step
    port, plain = make_pair(ctx, oracle_lib)
    plain.close()
    gm = api.ScanMatcher(ctx, api.baseline_config(fine_search_angle_offset=fine_res), api.laser_params(synth.Laser()))
    try:
        port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
        gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
        ranges, poses = _batch(wl, S_TILE3, 320 + n_fine)
        fine, _ = _on_off_oracle(port, gm, ranges, poses, _drawn(S_TILE3, 330 + n_fine), fine_res)
        assert fine.shape[1:] == (3, 3, n_fine)
        assert fine[:, :, :, n_fine - 1].any()  # the last group's last angle
    finally:
        gm.close()
        port.close()


def _centre_batch(wl, gi, offset, S, seed):
    """The workload's scans searched from poses on the band of _asymmetric_grid."""
    ranges, poses = _batch(wl, S, seed)
    rng = np.random.default_rng(seed + 1)
    mid = offset + 0.05 * np.array([gi["roi_w"] // 2, gi["roi_h"] // 2])
    poses[:, :2] = mid + rng.uniform(-3.0, 3.0, size=(S, 2))
    ranges = np.where(np.isfinite(ranges), np.minimum(ranges, rng.uniform(0.5, 9.0, size=ranges.shape)), ranges)
    return ranges, poses


@pytest.fixture(scope="module")
def synthetic(ctx, oracle_lib, workload_spread):
    port, gm = make_pair(ctx, oracle_lib)
    gi = port.grid_info()
    assert gi["width"] == 2005
    yield port, gm, workload_spread, gi, np.array([-50.0, -50.0])
    gm.close()
    port.close()


@pytest.mark.parametrize("S", SIZES)
def test_byte_value_limits(synthetic, S):
    """A grid set through set_grid whose bytes differ between neighbours, rows and lane groups.  Maximum byte 127: the MFMA
    form, equal to the packed form and to the oracle.  A square of cells at 128, then at 255: the next launch takes the
    packed form by itself (counter unchanged, option still 1) and equals the oracle.  The first grid again: back on the MFMA
    form."""
    port, gm, wl, gi, offset = synthetic
    ranges, poses = _centre_batch(wl, gi, offset, S, 340 + S)
    check = _drawn(S, 341 + S)
    g127 = _asymmetric_grid(gi)
    g127[g127 > 0] += 27  # 1..100 -> 28..127
    assert g127.max() == 127
    cy, cx = gi["height"] // 2, gi["width"] // 2

    def run(grid, takes_mfma):
        port.set_grid(grid, offset)
        gm.set_grid(grid, offset)
        fine, centers = _fine(gm, ranges, poses, 1, takes_mfma=takes_mfma)
        _against_oracle(port, fine, centers, ranges, poses, check)
        return fine, centers

    first, c_first = run(g127, True)
    off, c_off = _fine(gm, ranges, poses, 0)
    assert np.array_equal(first, off) and np.array_equal(c_first, c_off)
    assert (first != first[:, ::-1]).any() and (first != first[:, :, ::-1]).any()  # the sums are not symmetric either
    for v in (128, 255):
        g = g127.copy()
        g[cy - 40:cy + 41, cx - 40:cx + 41] = v
        other, _ = run(g, False)
        assert (other != first).any()  # the cells are read
    again, c_again = run(g127, True)
    assert np.array_equal(again, first) and np.array_equal(c_again, c_first)


@pytest.mark.parametrize("S", SIZES)
def test_whole_match_records_identical(pair, S):
    """One match_batch per batch size: the records of option on and off are the same bytes, the scan whose lattice leaves
    the grid included (status -3)."""
    port, gm, wl = pair
    ranges, poses = _batch(wl, S, 350 + S)
    outside = S // 2 + 1
    poses[outside, 0] += 500.0
    gm.set_option("fine_mfma", 1)
    n0 = gm.fine_mfma_launches
    on = gm.match_batch(ranges, poses)
    assert gm.fine_mfma_launches == n0 + 1
    gm.set_option("fine_mfma", 0)
    off = gm.match_batch(ranges, poses)
    assert gm.fine_mfma_launches == n0 + 1
    gm.set_option("fine_mfma", 1)
    assert on.tobytes() == off.tobytes()
    assert on["status"][outside] == -3 and (np.delete(on["status"], outside) == 0).all()
    assert (on["response"] > 0).sum() >= S // 2
