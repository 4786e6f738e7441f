"""The 128-thread form of the coarse reduce (k_reduce_coarse_lds<128>: batches of 2048 scans and more) against the restated
oracle and against the 256-thread form, on the branches of the block that the register and LDS budget of that form had to
be cut around: the tie average over several mask words, the maximum-variance covariance of a zero response, and the
block's own generic fallback for a lattice that is not uniform.

The batch is 2048 scans = 32 distinct synthetic scans with distinct start poses, tiled 64 times; the same 32 as one batch
take the 256-thread form.  Both run with and without the penalties: with them a best response > 0 is almost never shared
(two candidates tie only with equal distance AND angle penalty), without them a scan of one reading ties on every candidate
that puts its end point on a fully occupied cell.  The oracle is run once per variant for the module."""
import math

import numpy as np
import pytest

from lslam_amd import api, synth

POSE_TOL = 1e-9  # as tests/test_matcher_gpu.py
COV_TOL = 1e-9
THR = 12.0
N_DISTINCT, N_TILES = 32, 64  # 2048 scans: the smallest batch that runs the 128-thread form
RES, SCALE = 0.05, 1.0 / 0.05
I_BOUNDARY = range(0, 12)     # start poses half a cell off the raster: where the lattice coordinates then round unevenly
N_UNEVEN_MIN = 4              # (rounding noise decides, as in tests/test_stress_gpu.py) the block's generic fallback runs
I_ONE_BEAM = (12, 13, 14)     # one reading: a best response > 0 shared by many candidates (without the penalties)
I_ALL_NAN, I_ALL_FAR = 15, 16  # no reading / every end point off the grid: response 0 everywhere, maximum variance
K_MAX_VARIANCE = 500.0        # Mapper.cpp: MAX_VARIANCE
K_TOL = 1e-6                  # KT_TOLERANCE: responses within it tie


def _kround(v):
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


def _coarse_cells(pose, off, ax):
    nx = int(_kround(0.5 * 2.0 / (2 * RES)) + 1)
    return [_kround(((pose[ax] + (-0.5 + i * (2 * RES))) - off[ax]) * SCALE) for i in range(nx)]


class Cases:
    def __init__(self, oracle_lib):
        laser = synth.Laser()
        self.laser = laser
        wl = synth.make_match_workload(n_base=20, n_query=N_DISTINCT, seed=11, laser=laser)
        self.wl = wl
        self.port = oracle_lib.PortKarto(oracle_lib.default_cfg(), oracle_lib.laser_struct(laser, THR))
        self.port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
        off = self.port.grid_info()["offset"]
        self.off = off
        ranges, poses = wl.query_ranges.copy(), wl.query_poses.copy()
        n = ranges.shape[1]
        for q in I_BOUNDARY:  # x (even q) or y (odd q) of the centre half a cell off the grid raster (tests/test_stress_gpu.py)
            ax = q & 1
            poses[q, ax] = off[ax] + (_kround((poses[q, ax] - off[ax]) * SCALE) + 0.5) * RES
        for q in I_ONE_BEAM:  # the shortest reading alone: its end point is on the mapped walls, well inside the grid
            b = int(np.argmin(np.where(np.isfinite(ranges[q]), ranges[q], np.inf)))
            keep = ranges[q, b]
            ranges[q] = np.nan
            ranges[q, b] = keep
        ranges[I_ALL_NAN] = np.nan
        ranges[I_ALL_FAR] = 59.9
        self.ranges, self.poses, self.n = ranges, poses, n
        self._exp = {}

    def expected(self, penalize):
        if penalize not in self._exp:
            self._exp[penalize] = [self.port.match(self.ranges[q], self.poses[q], penalize, True) for q in range(N_DISTINCT)]
        return self._exp[penalize]

    def coarse(self, q, penalize):
        """the oracle's coarse pass alone: response, covariance, integer numerators [ny][nx][na]"""
        p = self.poses[q]
        resp, _, cov, st, sums = self.port.correlate_scan(self.ranges[q], p, p, 0.5, 2 * RES, 0.349, 0.0349, penalize, False,
                                                          want_sums=True)
        assert st == 0
        return resp, cov, sums


@pytest.fixture(scope="module")
def cases(oracle_lib):
    return Cases(oracle_lib)


def test_inputs_reach_the_branches(cases):
    """On the CPU, with the oracle: the chosen inputs really are a non-uniform lattice, a shared best response over more than
    one 32-candidate mask word, and a zero response with the maximum variance."""
    n_uneven = 0
    for q in I_BOUNDARY:
        cells = _coarse_cells(cases.poses[q], cases.off, q & 1)
        n_uneven += {b - a for a, b in zip(cells, cells[1:])} != {2}
    assert n_uneven >= N_UNEVEN_MIN, n_uneven
    for q in I_ONE_BEAM:
        resp, cov, sums = cases.coarse(q, False)
        assert resp > 0.0
        v = sums.astype(np.float64) / (cases.n * 100.0)
        flat = np.flatnonzero(np.abs(v - v.max()).ravel() <= K_TOL)  # candidate k = cell * nA + angle: sums' own layout ...
        flat_t = np.flatnonzero(np.abs(v - v.max()).transpose(1, 0, 2).ravel() <= K_TOL)  # ... whichever axis is x
        assert len(flat) >= 3 and len(set(flat >> 5)) > 1 and len(set(flat_t >> 5)) > 1, (q, flat)
    for q in (I_ALL_NAN, I_ALL_FAR):
        for pen in (True, False):
            resp, cov, sums = cases.coarse(q, pen)
            assert resp == 0.0 and not sums.any()  # every candidate ties with the best response: all 80 mask words
            assert cov[0, 0] == K_MAX_VARIANCE and cov[1, 1] == K_MAX_VARIANCE, cov


@pytest.fixture(scope="module")
def matcher(ctx, cases):
    gm = api.ScanMatcher(ctx, api.baseline_config(range_threshold=THR), api.laser_params(cases.laser, THR))
    gm.AddScans(cases.wl.base_ranges, cases.wl.base_poses, cases.wl.center_pose)
    return gm


@pytest.fixture(scope="module")
def records(ctx, cases, matcher):
    """penalize -> (the 2048-scan batch, the 32-scan batch), each matched once"""
    out = {}

    def get(penalize):
        if penalize not in out:
            ctx.profile(True)
            ctx.profile_reset()
            big = matcher.match_batch(np.tile(cases.ranges, (N_TILES, 1)), np.tile(cases.poses, (N_TILES, 1)), doPenalize=penalize)
            prof = ctx.profile_read()
            ctx.profile(False)
            assert "reduce_coarse" in prof, prof  # the five-kernel step: the reduce is a launch of its own
            out[penalize] = (big, matcher.match_batch(cases.ranges, cases.poses, doPenalize=penalize))
        return out[penalize]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("penalize", [True, False])
def test_narrow_form_against_the_oracle(cases, records, penalize):
    """(a) 2048 scans, the 128-thread form: every record equals the oracle's record of its distinct scan."""
    big, _ = records(penalize)
    assert len(big) == N_DISTINCT * N_TILES >= 2048
    exp = cases.expected(penalize)
    for i in range(len(big)):
        mean, cov, resp = exp[i % N_DISTINCT]
        res = big[i]
        assert res["status"] == 0, i
        assert np.abs(res["pose"][:2] - mean[:2]).max() <= POSE_TOL, i
        assert abs(math.remainder(res["pose"][2] - mean[2], 2 * math.pi)) <= POSE_TOL, i
        assert np.abs(res["covariance"] - cov).max() <= COV_TOL * max(1.0, np.abs(cov).max()), i
        assert abs(res["response"] - resp) <= 1e-12, i
    assert big["response"][I_ALL_NAN] == 0.0 and big["response"][I_ALL_FAR] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("penalize", [True, False])
def test_narrow_form_equals_the_wide_form(records, penalize):
    """(b) the same scans as a batch of 32 (256-thread blocks): byte-identical records."""
    big, small = records(penalize)
    assert big.tobytes() == np.tile(small, N_TILES).tobytes()
