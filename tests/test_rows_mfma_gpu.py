"""The MFMA accumulate of the coarse response kernel (set_option('rows_mfma', 1): phase B of resp_rows_wave sums the queued
rows' bytes with v_mfma_i32_16x16x64_i8 against a one-hot operand) against the packed form (rows_mfma 0) and the oracle.

Every numerator comparison is np.array_equal on ALL numerators of coarse_sums_batch -- integer sums, no tolerance --, option on
against option off over the whole batch and 24 seeded scans per case against the oracle's lattice (kor_correlate_scan,
want_sums).  rows_mfma_launches shows which accumulate took each launch; coarse_form_launches() names the form, which is the
same for both.  The i8 MFMA reads signed bytes: a grid with a byte above 127 must fall back to the packed form on its own."""
import math

import numpy as np
import pytest

from lslam_amd import synth

from test_matcher_gpu import _assert_result, make_pair
from test_rows_wave_edges_gpu import (COARSE, INDOOR, N_CHECK, S_HOT, _batch, _drawn, _indoor_batch, _launched,
                                      _own_scan_with_a_full_first_block)

pytestmark = pytest.mark.gpu

INDOOR_LATTICE = (0.15, 0.02, 0.349, 0.0349)


def _sums(gm, ranges, poses, mfma, form="rows_tiled", launches=1, takes_mfma=None):
    """coarse_sums_batch with the option set; asserts the form and which accumulate took the launches."""
    takes_mfma = bool(mfma) if takes_mfma is None else takes_mfma
    gm.set_option("rows_mfma", mfma)
    assert gm.get_option("rows_mfma") == mfma
    before, n0 = gm.coarse_form_launches(), gm.rows_mfma_launches
    got = gm.coarse_sums_batch(ranges, poses)
    assert _launched(gm, before) == {form: launches}
    assert gm.rows_mfma_launches - n0 == (launches if takes_mfma else 0)
    return got


def _on_off_oracle(port, gm, ranges, poses, check, lattice=COARSE, form="rows_tiled", launches=1, takes_mfma=True):
    """rows_mfma 1 against 0 on every numerator of the batch, and the drawn scans against the oracle."""
    on = _sums(gm, ranges, poses, 1, form, launches, takes_mfma)
    off = _sums(gm, ranges, poses, 0, form, launches)
    gm.set_option("rows_mfma", 1)
    assert on.shape == off.shape and on.shape[0] == len(ranges) and on.any()
    assert np.array_equal(on, off)
    for q in check:
        _, _, _, st, want = port.correlate_scan(ranges[q], poses[q], poses[q], *lattice, True, False, want_sums=True)
        assert st == 0, q
        assert on[q].shape == want.shape and np.array_equal(on[q], want), q
    return on


@pytest.fixture(scope="module")
def pair(ctx, oracle_lib, workload_spread):
    wl = workload_spread
    port, gm = make_pair(ctx, oracle_lib)
    port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
    gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
    yield port, gm, wl
    gm.close()
    port.close()


@pytest.fixture(scope="module")
def indoor(ctx, oracle_lib):
    """The 16 x 16 x 21 lattice with response expansion of test_rows_wave_edges_gpu: k_resp_rows<4,8>, two row passes."""
    laser = synth.Laser(range_max=30.0)
    port, gm = make_pair(ctx, oracle_lib, laser=laser, cfg_kw=INDOOR, range_threshold=12.0)
    world = synth.arena(size=24.0, n_axis=8, n_rot=3, seed=12)
    wl = synth.make_match_workload(n_base=12, n_query=13, seed=12, laser=laser, world=world, err_xy=0.08,
                                   err_th=math.radians(6.0), query_spread=0.5)
    port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
    gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
    yield port, gm, wl
    gm.close()
    port.close()


def _edge_batch(port, wl, seed):
    """104 scans: scan 0 queues nothing (zero C, no drain), scan 1 has one beam (a drain of one lane: the other 63 stay on
    the zero pad), scan 2 fills the queue from its first block; every other scan ends on a partial last drain."""
    ranges, poses = _batch(wl, S_HOT, seed)
    own = _own_scan_with_a_full_first_block(port, wl)
    ranges[0] = np.nan
    ranges[1] = np.nan
    ranges[1, 5], poses[1] = wl.base_ranges[own][5], wl.base_poses[own]  # a beam that ends on occupied cells
    ranges[2], poses[2] = wl.base_ranges[own], wl.base_poses[own]
    return ranges, poses


def test_default_is_on(pair):
    assert pair[1].get_option("rows_mfma") == 1


def test_smallest_tiled_batch(pair):
    port, gm, wl = pair
    assert gm.num_beams == 1081
    ranges, poses = _edge_batch(port, wl, 211)
    got = _on_off_oracle(port, gm, ranges, poses, _drawn(S_HOT, 212, always=(0, 1, 2)))
    assert not got[0].any() and got[1].any() and got[2].any()


def test_smallest_tiled_batch_two_row_passes(indoor):
    port, gm, wl = indoor
    ranges, poses = _indoor_batch(wl, S_HOT, 213)
    ranges[0] = np.nan
    ranges[1] = np.nan
    ranges[1, 517] = 3.0
    got = _on_off_oracle(port, gm, ranges, poses, _drawn(S_HOT, 214, always=(0, 1)), lattice=INDOOR_LATTICE, launches=4)
    assert got.shape[1:] == (16, 16, 21)
    assert not got[0].any() and got[:, :8].any() and got[:, 8:].any()
    assert got[:, :, 12:].any()  # candidates 12..15 of a row: the fourth realigned word


def _asymmetric_grid(gi):
    """Byte at (x, y) = (7 x + 13 y) mod 101 on a band around the grid's middle, zero elsewhere: neighbouring bytes, rows
    and 16-lane groups all differ, so no mix-up of them cancels."""
    h, w = gi["height"], gi["width"]
    y, x = np.mgrid[0:h, 0:w]
    grid = np.zeros((h, gi["stride"]), dtype=np.uint8)
    band = (np.abs(y - h // 2) < 260) & (np.abs(x - w // 2) < 260)
    grid[:, :w] = np.where(band, (7 * x + 13 * y) % 101, 0).astype(np.uint8)
    return grid


def _centre_batch(wl, gi, offset, seed):
    """The workload's scans searched from poses on the band of _asymmetric_grid."""
    ranges, poses = _batch(wl, S_HOT, seed)
    rng = np.random.default_rng(seed + 1)
    mid = offset + 0.05 * np.array([gi["roi_w"] // 2, gi["roi_h"] // 2])
    poses[:, :2] = mid + rng.uniform(-3.0, 3.0, size=(S_HOT, 2))
    ranges = np.where(np.isfinite(ranges), np.minimum(ranges, rng.uniform(0.5, 9.0, size=ranges.shape)), ranges)
    return ranges, poses


@pytest.fixture(scope="module")
def synthetic(ctx, oracle_lib, workload_spread):
    port, gm = make_pair(ctx, oracle_lib)
    gi = port.grid_info()
    assert abs(1.0 / 0.05 - 20.0) < 1e-9 and gi["width"] == 2005
    yield port, gm, workload_spread, gi, np.array([-50.0, -50.0])
    gm.close()
    port.close()


def test_asymmetric_grid(synthetic):
    port, gm, wl, gi, offset = synthetic
    grid = _asymmetric_grid(gi)
    assert grid.max() == 100
    port.set_grid(grid, offset)
    gm.set_grid(grid, offset)
    ranges, poses = _centre_batch(wl, gi, offset, 221)
    got = _on_off_oracle(port, gm, ranges, poses, _drawn(S_HOT, 222))
    assert (got != got[:, ::-1]).any() and (got != got[:, :, ::-1]).any()  # the sums are not symmetric either


def test_byte_value_limits(synthetic):
    """Maximum byte 127: the MFMA form, equal to the oracle.  One cell at 128, then at 255: the next launch takes the packed
    form by itself (counter unchanged, option still 1) and equals the oracle.  The first grid again: back on the MFMA form."""
    port, gm, wl, gi, offset = synthetic
    ranges, poses = _centre_batch(wl, gi, offset, 231)
    check = _drawn(S_HOT, 232)
    g127 = _asymmetric_grid(gi)
    g127[g127 > 0] += 27  # 1..100 -> 28..127
    assert g127.max() == 127
    cy, cx = gi["height"] // 2, gi["width"] // 2

    def run(grid, takes_mfma):
        port.set_grid(grid, offset)
        gm.set_grid(grid, offset)
        got = _sums(gm, ranges, poses, 1, takes_mfma=takes_mfma)
        for q in check:
            _, _, _, st, want = port.correlate_scan(ranges[q], poses[q], poses[q], *COARSE, True, False, want_sums=True)
            assert st == 0, q
            assert np.array_equal(got[q], want), q
        return got

    first = run(g127, True)
    for v in (128, 255):
        g = g127.copy()
        g[cy, cx] = v
        other = run(g, False)
        assert (other != first).any()  # the cell is read
    assert np.array_equal(run(g127, True), first)


@pytest.mark.parametrize("n_beams", [64, 65, 1081, 2048])
def test_beam_counts(ctx, oracle_lib, n_beams):
    """64 beams: one block; 65: a one-beam second block; 1081: 17 blocks; 2048 = 64 * kMaxBeamsPerLane: the most a wave takes
    unsliced (the int32 accumulators have no such limit; the host slices as before)."""
    laser = synth.Laser(n_ranges=n_beams, angle_increment=math.radians(270.0) / n_beams)
    port, gm = make_pair(ctx, oracle_lib, laser)
    try:
        wl = synth.make_match_workload(n_base=12, n_query=12, seed=240 + n_beams % 7, laser=laser, query_spread=1.5)
        port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
        gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
        assert gm.num_beams == n_beams
        ranges, poses = _batch(wl, S_HOT, 241 + n_beams)
        _on_off_oracle(port, gm, ranges, poses, _drawn(S_HOT, 242 + n_beams))
    finally:
        gm.close()
        port.close()


def test_multi_wave(pair):
    """rows_waves 2 with rows_mfma 1 (k_resp_rows_mw) against the default run."""
    port, gm, wl = pair
    ranges, poses = _edge_batch(port, wl, 251)
    default = _sums(gm, ranges, poses, 1)
    gm.set_option("rows_waves", 2)
    try:
        mw = _sums(gm, ranges, poses, 1, form="rows_multiwave")
    finally:
        gm.set_option("rows_waves", 1)
    assert default.any() and np.array_equal(mw, default)


def _whole_match(port, gm, ranges, poses, seed):
    gm.set_option("rows_mfma", 1)
    n0 = gm.rows_mfma_launches
    on = gm.match_batch(ranges, poses)
    assert gm.rows_mfma_launches > n0
    gm.set_option("rows_mfma", 0)
    n0 = gm.rows_mfma_launches
    off = gm.match_batch(ranges, poses)
    assert gm.rows_mfma_launches == n0
    gm.set_option("rows_mfma", 1)
    assert on.tobytes() == off.tobytes()
    for q in _drawn(len(ranges), seed)[:N_CHECK]:
        mean, cov, resp = port.match(ranges[q], poses[q])
        _assert_result(on[q], mean, cov, resp)


def test_whole_match(pair):
    port, gm, wl = pair
    ranges, poses = _batch(wl, S_HOT, 261)
    _whole_match(port, gm, ranges, poses, 262)


def test_whole_match_two_row_passes(indoor):
    port, gm, wl = indoor
    ranges, poses = _indoor_batch(wl, S_HOT, 263)
    _whole_match(port, gm, ranges, poses, 264)
