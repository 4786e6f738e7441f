"""The edges of a coarse response wave (resp_rows_wave) and the angle groups of the fine one (resp_tile3_wave), at the batch
sizes and scan shapes where they can go wrong: a scan that queues nothing, one beam, a queue filled by the first block of
beams alone; even and odd block counts with last blocks of 1 and of 57 beams (the odd last block goes into phase A alone);
the second pass over the lattice rows, which reuses the epilogue's LDS for the queue; a last fine-angle group that is not full;
and one whole match per lattice, with a scan whose lattice leaves the grid.

Every numerator comparison is bit equality of ALL numerators of a scan against the oracle's lattice
(kor_correlate_scan, want_sums) -- integer sums, no tolerance -- over 24 scans per case drawn by a fixed seed; poses lie
inside the grid, so the oracle accepts every drawn scan and none is skipped.  coarse_form_launches() shows that the intended
kernel form took the launch.  The match_batch cases use the tolerances of test_matcher_gpu.py."""
import math

import numpy as np
import pytest

from lslam_amd import api, synth

from test_matcher_gpu import _assert_result, make_pair

pytestmark = pytest.mark.gpu

S_HOT = 104      # the first multiple of 8 with S * 21 >= kTileMinWaves (2048): the smallest batch on the tiled one-wave form
S_TILE3 = 1536   # kTile3ManyMinScans: the smallest batch on the three-angles-per-wave fine form
N_CHECK = 24
COARSE = (0.5, 0.1, 0.349, 0.0349)  # search offset, lattice step, angle offset, angle step of the 11 x 11 x 21 lattice


def _launched(gm, before):
    after = gm.coarse_form_launches()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _batch(wl, S, seed, nan_frac=0.01):
    """S scans cycled from the workload's queries; the repeats get search centres of their own."""
    nq = len(wl.query_ranges)
    idx = np.arange(S) % nq
    rng = np.random.default_rng(seed)
    poses = wl.query_poses[idx].copy()
    far = np.arange(S) >= nq
    poses[far, :2] += rng.uniform(-0.4, 0.4, size=(int(far.sum()), 2))
    poses[far, 2] += rng.uniform(-0.3, 0.3, size=int(far.sum()))
    ranges = wl.query_ranges[idx].copy()
    ranges[rng.random(ranges.shape) < nan_frac] = np.nan
    return ranges, poses


def _drawn(S, seed, always=(), never=()):
    """N_CHECK distinct scans of the batch: the ones a case names, then a seeded draw."""
    rng = np.random.default_rng(seed)
    rest = [int(q) for q in rng.permutation(S) if int(q) not in always and int(q) not in never]
    picked = list(always) + rest[:N_CHECK - len(always)]
    assert len(set(picked)) == N_CHECK
    return picked


def _coarse_against_oracle(port, gm, ranges, poses, check, lattice=COARSE, form="rows_tiled", expansions=0):
    """`expansions`: response-expansion passes the configuration adds behind the coarse pass (same form, wider angles)."""
    before = gm.coarse_form_launches()
    got = gm.coarse_sums_batch(ranges, poses)
    assert _launched(gm, before) == {form: 1 + expansions}
    assert got.shape[0] == len(ranges) and got.any()
    for q in check:
        _, _, _, st, want = port.correlate_scan(ranges[q], poses[q], poses[q], *lattice, True, False, want_sums=True)
        assert st == 0, q
        assert got[q].shape == want.shape and np.array_equal(got[q], want), q
    return got


@pytest.fixture(scope="module")
def pair(ctx, oracle_lib, workload_spread):
    wl = workload_spread
    port, gm = make_pair(ctx, oracle_lib)
    port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
    gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
    yield port, gm, wl
    gm.close()
    port.close()


def _own_scan_with_a_full_first_block(port, wl):
    """A base scan that, seen from its own pose, has each of its first 64 beams end on occupied cells at the middle candidate
    angle (10 of 21: the scan's own heading): the oracle's numerators of the scan reduced to that one beam are not all zero."""
    for k in range(len(wl.base_ranges)):
        r, p = wl.base_ranges[k], wl.base_poses[k]
        if not np.isfinite(r[:64]).all():
            continue
        for b in range(64):
            one = np.full_like(r, np.nan)
            one[b] = r[b]
            _, _, _, st, sums = port.correlate_scan(one, p, p, *COARSE, True, False, want_sums=True)
            if st != 0 or not sums[:, :, 10].any():
                break
        else:
            return k
    raise AssertionError("no base scan fills the queue from its first block")


def test_hot_form_at_its_smallest_batch(pair):
    """104 scans of 1081 beams on k_resp_rows<3,11,true>.  Scan 0 has no readable beam: nothing is ever queued, the
    accumulators are zeroed instead of written by a first drain, and the epilogue still runs.  Scan 1 has one readable beam.
    Scan 2 is a base scan seen from its own pose whose first 64 beams all end on occupied cells at the middle candidate
    angle: there the queue reaches 64 entries -- the first drain -- on the first block of beams alone."""
    port, gm, wl = pair
    assert gm.num_beams == 1081
    ranges, poses = _batch(wl, S_HOT, 11)
    ranges[0] = np.nan
    ranges[1] = np.nan
    ranges[1, 517] = 3.0
    own = _own_scan_with_a_full_first_block(port, wl)
    ranges[2], poses[2] = wl.base_ranges[own], wl.base_poses[own]
    got = _coarse_against_oracle(port, gm, ranges, poses, _drawn(S_HOT, 12, always=(0, 1, 2)))
    assert not got[0].any() and got[2].any()


@pytest.mark.parametrize("n_beams", [128, 129, 961, 1024, 1025, 1081])
def test_block_parity(ctx, oracle_lib, n_beams):
    """Phase A takes blocks of 64 beams in pairs: 128 and 1024 beams are an even number of full blocks, 961 ends on a first
    block of a pair that holds one beam, 129 and 1025 on one-beam blocks with an empty partner, 1081 (17 blocks) on a
    57-beam block with an empty partner."""
    laser = synth.Laser(n_ranges=n_beams, angle_increment=math.radians(270.0) / n_beams)
    port, gm = make_pair(ctx, oracle_lib, laser)
    try:
        wl = synth.make_match_workload(n_base=12, n_query=12, seed=30 + n_beams % 7, laser=laser, query_spread=1.5)
        port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
        gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
        assert gm.num_beams == n_beams
        ranges, poses = _batch(wl, S_HOT, n_beams)
        ranges[3, :-1] = np.nan  # only the LAST beam of the scan readable: all that the odd last block brings
        if not np.isfinite(ranges[3, -1]):
            ranges[3, -1] = 4.0
        _coarse_against_oracle(port, gm, ranges, poses, _drawn(S_HOT, n_beams + 1, always=(3,)))
    finally:
        gm.close()
        port.close()


INDOOR = dict(search_size=0.3, resolution=0.01, smear_deviation=0.03, use_response_expansion=1)


@pytest.fixture(scope="module")
def indoor(ctx, oracle_lib):
    """The configuration the reference ships (test_reference_indoor_default_config): 16 x 16 x 21 coarse lattice."""
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


def _indoor_batch(wl, S, seed):
    nq = len(wl.query_ranges)
    idx = np.arange(S) % nq
    rng = np.random.default_rng(seed)
    poses = wl.query_poses[idx].copy()
    far = np.arange(S) >= nq
    poses[far, :2] += rng.uniform(-0.05, 0.05, size=(int(far.sum()), 2))
    poses[far, 2] += rng.uniform(-0.1, 0.1, size=int(far.sum()))
    return wl.query_ranges[idx].copy(), poses


def test_two_passes_over_the_lattice_rows(indoor):
    """k_resp_rows<4,8,true>: 16 lattice rows in two passes of 8 -- the epilogue runs twice and its LDS words are the
    queue's in between."""
    port, gm, wl = indoor
    ranges, poses = _indoor_batch(wl, S_HOT, 40)
    got = _coarse_against_oracle(port, gm, ranges, poses, _drawn(S_HOT, 41), lattice=(0.15, 0.02, 0.349, 0.0349), expansions=3)
    assert got.shape[1:] == (16, 16, 21)
    assert got[:, :8].any() and got[:, 8:].any()


@pytest.mark.parametrize("n_fine", [10, 11, 12, 13])
def test_fine_angle_groups(ctx, oracle_lib, workload_spread, n_fine):
    """k_resp_tile3<3> at its smallest batch with 10 (3+3+3+1), 11 (3+3+3+2), 12 (four full groups) and 13 fine angles."""
    wl = workload_spread
    fine_res = 0.0349 / (n_fine - 1)  # the fine pass spans +- half a coarse angle step
    port, plain = make_pair(ctx, oracle_lib)
    plain.close()
    gm = api.ScanMatcher(ctx, api.baseline_config(fine_search_angle_offset=fine_res), api.laser_params(synth.Laser()))
    try:
        port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
        gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
        ranges, poses = _batch(wl, S_TILE3, 50 + n_fine)
        before = gm.coarse_form_launches()
        fine, centers = gm.fine_sums_batch(ranges, poses)
        ran = _launched(gm, before)
        assert ran.get("fine_tile3", 0) >= 1 and "fine_rows" not in ran, ran
        assert fine.shape[1:] == (3, 3, n_fine)
        n_nonzero = 0
        for q in _drawn(S_TILE3, 60 + n_fine):
            assert not np.isnan(centers[q]).any(), q
            _, _, _, st, want = port.correlate_scan(ranges[q], poses[q], centers[q], 0.05, 0.05, 0.5 * 0.0349, fine_res, True,
                                                    True, want_sums=True)
            assert st == 0, q
            assert fine[q].shape == want.shape and np.array_equal(fine[q], want), q
            n_nonzero += int(want.any())
        assert n_nonzero >= N_CHECK // 2
    finally:
        gm.close()
        port.close()


def _match_against_oracle(port, gm, ranges, poses, check, outside):
    """One match_batch: the drawn scans against the oracle's records, the scan whose lattice leaves the grid by its status."""
    res = gm.match_batch(ranges, poses)
    for q in check:
        mean, cov, resp = port.match(ranges[q], poses[q])
        _assert_result(res[q], mean, cov, resp)
    assert res["status"][outside] == -3  # LSLAM_ERR_INDEX_OUT_OF_RANGE, as the lattice set-up wrote it
    with pytest.raises(RuntimeError):
        port.match(ranges[outside], poses[outside])
    assert (np.delete(res["status"], outside) == 0).all()


@pytest.mark.parametrize("S", [S_HOT, S_TILE3])
def test_match_batch_through_the_hot_form(pair, S):
    port, gm, wl = pair
    ranges, poses = _batch(wl, S, 70 + S)
    outside = S // 2 + 1
    poses[outside, 0] += 500.0
    before = gm.coarse_form_launches()
    _match_against_oracle(port, gm, ranges, poses, _drawn(S, 80 + S, never=(outside,)), outside)
    ran = _launched(gm, before)
    # 104 x 11 fine waves stay below kTileMinWaves (beam slices on the row kernel), 1536 scans take the three-angle form
    assert ran == {"rows_tiled": 1, "fine_tile3" if S == S_TILE3 else "fine_rows": 1}, ran


def test_match_batch_through_two_row_passes(indoor):
    port, gm, wl = indoor
    ranges, poses = _indoor_batch(wl, S_HOT, 90)
    outside = 57
    poses[outside, 1] -= 500.0
    before = gm.coarse_form_launches()
    _match_against_oracle(port, gm, ranges, poses, _drawn(S_HOT, 91, never=(outside,)), outside)
    ran = _launched(gm, before)
    # the coarse pass and its expansion passes on the tiled one-wave form, 104 x 11 fine waves on the row kernel
    assert ran.pop("rows_tiled") >= 1 and set(ran) <= {"fine_rows"}, ran
