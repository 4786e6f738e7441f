"""The log-odds update kernels (k_logodds_pipe_ml, k_logodds_mark, k_logodds_apply, k_lo_batch_hits / _hits_lds / _rays /
_resolve / _apply) on the directed scenarios of tests/logodds_cases.py, through every route the library offers for feeding
them: the log-odds planes of every level against the plain-C oracle bit for bit, the published occupancy too.
tests/test_logodds_cases_oracle.py holds every scenario to its claim on the CPU and the oracle to the reference's own
headers.  No tolerances: the path is bit-exact by contract (same float operations per cell in the same order)."""
import numpy as np
import pytest
import torch

import logodds_cases as E
from lslam_amd import api

pytestmark = pytest.mark.gpu

# where the host measures the scans' reach at a 1 MB budget (64 whole-map windows exceed it) AND the windows of one call do
# not fit it together: these must take two rounds or more in some call (tests/test_logodds_cases_oracle.py::
# test_window_coverage has the planner's side of it).  The windows of sweep_rim's 20-cell rays are a few KB each, the maps of
# pairs, triples and beam_counts are smaller than the budget 64 times over, the other scenarios have a dozen scans.
TWO_ROUNDS = ("sweep", "long_thin_x32768", "long_thin_y32768", "non_finite_batched")


def make_map(ctx, m, monkeypatch, two_kernels=False):
    if two_kernels:
        monkeypatch.setenv("LSLAM_MAP_TWO_KERNELS", "1")  # read at map creation
    g = api.OccGridMap(ctx, m.sx, m.sy, m.cell, m.offset, levels=m.levels)
    if two_kernels:
        monkeypatch.delenv("LSLAM_MAP_TWO_KERNELS")
    return g


def compare(g, m, want, route, first, last):
    """planes and occupancy of every level against the oracle's after scans [first, last)"""
    planes, occ = want
    for lv in range(m.levels):
        got = g.logodds(lv)
        assert got.shape == planes[lv].shape and got.dtype == planes[lv].dtype
        if got.tobytes() != planes[lv].tobytes():
            differ = got.view(np.uint32) != planes[lv].view(np.uint32)
            y, x = (int(v) for v in np.argwhere(differ)[0])
            raise AssertionError(f"{route}: level {lv} after scans {first}..{last - 1}: {int(differ.sum())} cells differ, the first "
                                 f"is ({x}, {y}): device {float(got[y, x])!r}, oracle {float(planes[lv][y, x])!r}")
        assert np.array_equal(g.occupancy_i8(lv), occ[lv]), (route, lv, first, last)


def run_single(g, sc, route, exp):
    m, first = sc.map, 0
    for k, (pts, origo, pose) in enumerate(sc.scans):
        if m.levels > 1:  # matchData caches the container the levels above 0 are fed from (its pose is not used)
            g.matchData(pose, pts, origo)
        g.updateByScan(pts, origo, pose)
        # the pipelined route reads at the end only: every apply but the last runs inside a k_logodds_pipe_ml launch
        if k + 1 in exp and (route == "single_two_kernels" or k + 1 == len(sc.scans)):
            compare(g, m, exp[k + 1], route, first, k + 1)
            first = k + 1


def run_batched(g, sc, route, exp):
    """-> (rounds run at least, most rounds of one group)"""
    m = sc.map
    counts = np.array([len(p) for p, _, _ in sc.scans], np.int32)
    start = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    origos = np.stack([o for _, o, _ in sc.scans])
    poses = np.stack([q for _, _, q in sc.scans])
    on_device = route in ("batch_dev_hint", "batch_dev_whole")
    if on_device:
        packed = np.ascontiguousarray(np.concatenate([p for p, _, _ in sc.scans]), dtype=np.float32)
        d_pts = torch.from_numpy(packed).to("cuda:0")
        torch.cuda.synchronize()
    if route == "batch_windows":
        g.set_option("batch_scratch_mb", 1)  # the host measures each scan's reach and plans windows and rounds
    cuts = E.call_cuts(sc)
    rounds_run = most = first = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        if on_device:
            if route == "batch_dev_hint":
                g.set_option("batch_radius_cells", int(sc.reach[a:b].max()))
            g.updateByScans_dev(d_pts.data_ptr() + 8 * int(start[a]), counts[a:b], origos[a:b], poses[a:b])
        else:
            g.updateByScans([p for p, _, _ in sc.scans[a:b]], origos[a:b], poses[a:b])
        groups = -(-(b - a) // 64)
        if route in ("batch_windows", "batch_dev_hint"):
            st = g.batch_stats()
            assert st["window_misses"] == 0, (route, a, b, st)
            rounds_run += groups - 1 + st["rounds"]  # (the statistics carry the rounds of the call's last group of 64)
            most = max(most, st["rounds"])
        else:
            rounds_run += groups
        if b in exp:
            compare(g, m, exp[b], route, first, b)
            first = b
    assert g.batch_stats()["window_misses"] == 0
    return rounds_run, most


@pytest.mark.parametrize("name,route", E.ROUTE_CASES, ids=[f"{n}-{r}" for n, r in E.ROUTE_CASES])
def test_route_equals_the_oracle(ctx, oracle_lib, monkeypatch, name, route):
    sc = E.scenario(name)
    assert route in sc.routes
    exp = E.expected(oracle_lib, name)
    g = make_map(ctx, sc.map, monkeypatch, two_kernels=route == "single_two_kernels")
    try:
        if route in E.SINGLE:
            run_single(g, sc, route, exp)
        else:
            rounds_run, most = run_batched(g, sc, route, exp)
            if name == "sweep":  # the 6-bit epoch of the pool and flag bytes wraps every 63 rounds: several times here
                assert rounds_run > 126, rounds_run
            if route == "batch_windows" and name in TWO_ROUNDS:
                assert most >= 2, most
    finally:
        g.close()
    if name == "long_steep" and route == sc.routes[-1]:
        E._EXPECTED.pop(name, None)  # 140 MB of plane


def few_scans(n=3):
    """scans of 255, 255 and 256 points"""
    sc = E.scenario("beam_counts")
    return [sc.scans[k] for k in sc.notes["big"][22:22 + n]]


@pytest.mark.parametrize("route", E.ROUTES)
def test_more_than_65536_points_are_refused(ctx, oracle_lib, monkeypatch, route):
    """the per-cell key keeps 16 bits for the beam: every route refuses a scan of 65537 points, alone or between two others,
    and leaves the map as it was"""
    m = E.FAN_MAP
    g = make_map(ctx, m, monkeypatch, two_kernels=route == "single_two_kernels")
    o = E.make_oracle(oracle_lib, m)
    for pts, origo, pose in few_scans():
        g.updateByScan(pts, origo, pose)
        o.updateByScan(pts, origo, pose)
    want = E.oracle_planes(o, m)
    compare(g, m, want, route, 0, 3)
    rng = np.random.default_rng(7)
    long_scan = rng.uniform(-60.0, 60.0, (E.MAX_POINTS + 1, 2)).astype(np.float32)
    (p0, origo, pose) = few_scans(1)[0]
    with pytest.raises(api.LslamError):
        if route in E.SINGLE:
            g.updateByScan(long_scan, origo, pose)
        elif route in ("batch_plane", "batch_windows"):
            if route == "batch_windows":
                g.set_option("batch_scratch_mb", 1)
            g.updateByScans([p0, long_scan, p0], origo, np.stack([pose] * 3))
        else:
            if route == "batch_dev_hint":
                g.set_option("batch_radius_cells", 90)
            d_pts = torch.from_numpy(np.concatenate([p0, long_scan, p0])).to("cuda:0")
            torch.cuda.synchronize()
            g.updateByScans_dev(d_pts.data_ptr(), [len(p0), len(long_scan), len(p0)], origo, np.stack([pose] * 3))
    compare(g, m, want, route, 0, 3)
    if route in E.BATCHED:  # the long scan in the SECOND group of 64: the first group must not have been applied
        many = [p0] * 65 + [long_scan]
        with pytest.raises(api.LslamError):
            if route in ("batch_plane", "batch_windows"):
                g.updateByScans(many, origo, np.stack([pose] * 66))
            else:
                d_pts = torch.from_numpy(np.concatenate(many)).to("cuda:0")
                torch.cuda.synchronize()
                g.updateByScans_dev(d_pts.data_ptr(), [len(q) for q in many], origo, np.stack([pose] * 66))
        compare(g, m, want, route, 0, 3)
    # ... and goes on working
    g.updateByScan(p0, origo, pose)
    o.updateByScan(p0, origo, pose)
    compare(g, m, E.oracle_planes(o, m), route, 0, 4)
    g.close()


@pytest.mark.parametrize("route", E.BATCHED)
def test_sides_above_32768_are_refused_by_the_batched_routes(ctx, oracle_lib, monkeypatch, route):
    """k_lo_batch_rays keeps abs_da / 2 + c * abs_db in 32 bits: update_batch_impl refuses a level with a side above 32768
    cells (the single-scan kernels divide in 64 bits and take such a map: long_thin_x70001)"""
    sc = E.scenario("long_thin_x70001")
    m = sc.map
    g = make_map(ctx, m, monkeypatch)
    o = E.make_oracle(oracle_lib, m)
    pts, origo, pose = sc.scans[0]
    g.updateByScan(pts, origo, pose)
    o.updateByScan(pts, origo, pose)
    want = E.oracle_planes(o, m)
    with pytest.raises(api.LslamError):
        if route in ("batch_plane", "batch_windows"):
            if route == "batch_windows":
                g.set_option("batch_scratch_mb", 1)
            g.updateByScans([pts, pts], origo, np.stack([pose] * 2))
        else:
            if route == "batch_dev_hint":
                g.set_option("batch_radius_cells", int(sc.reach[0]))
            d_pts = torch.from_numpy(np.concatenate([pts, pts])).to("cuda:0")
            torch.cuda.synchronize()
            g.updateByScans_dev(d_pts.data_ptr(), [len(pts), len(pts)], origo, np.stack([pose] * 2))
    compare(g, m, want, route, 0, 1)
    g.close()


def test_just_once_rounding(ctx, oracle_lib):
    """updateByScanJustOnce with begin and metres per cell passed explicitly: round(p / 0.05) in double, half away from zero,
    on points at and next to every tie of a 41 x 37 map; NaN, +-Inf and 3e9 are dropped"""
    m = E.JUST_ONCE
    g = api.OccGridMap(ctx, m.sx, m.sy, m.cell, m.offset)
    o = oracle_lib.PortHector(m.sx, m.sy, m.cell, m.offset)
    for k, pts in enumerate(E.just_once_points()):
        origo = (0.0, 0.0) if k != 2 else (0.26, -0.26)  # an origo that moves the begin cell by its own rounding
        g.updateByScanJustOnce(pts, origo, E.JUST_ONCE_BEGIN, 0.05)
        o.updateByScanJustOnce(pts, origo, E.JUST_ONCE_BEGIN, 0.05)
        compare(g, m, E.oracle_planes(o, m), "just_once", 0, k + 1)
    assert np.count_nonzero(o.logodds()) > 100
    g.close()


def test_the_named_launches_ran(ctx, oracle_lib, monkeypatch):
    """a short run of the two single routes and the plain batched one under the launch profile: the pipelined route is
    k_logodds_pipe_ml launches and one flushed apply, the two-kernel route a mark and an apply per scan, the batched route
    one launch of each of its four kernels per group and round"""
    sc = E.scenario("knife_edge_l0")
    n = len(sc.scans)
    pipe = make_map(ctx, sc.map, monkeypatch)
    two = make_map(ctx, sc.map, monkeypatch, two_kernels=True)
    batch = make_map(ctx, sc.map, monkeypatch)
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_reset()
    for pts, origo, pose in sc.scans:
        pipe.updateByScan(pts, origo, pose)
        two.updateByScan(pts, origo, pose)
    batch.updateByScans([p for p, _, _ in sc.scans], np.stack([o for _, o, _ in sc.scans]), np.stack([q for _, _, q in sc.scans]))
    ctx.synchronize()  # flushes the pending apply of `pipe`
    ctx.profile(False)
    prof = ctx.profile_read()
    assert {"logodds_pipe", "logodds_mark", "logodds_apply", "lo_batch_hits", "lo_batch_rays", "lo_batch_resolve",
            "lo_batch_apply"} <= set(prof), prof
    assert prof["logodds_pipe"][0] == n and prof["logodds_mark"][0] == n and prof["logodds_apply"][0] == n + 1, prof
    assert [prof[k][0] for k in ("lo_batch_hits", "lo_batch_rays", "lo_batch_resolve", "lo_batch_apply")] == [1] * 4, prof
    want = E.expected(oracle_lib, sc.name)[n]
    for g, route in ((pipe, "single_pipe"), (two, "single_two_kernels"), (batch, "batch_plane")):
        compare(g, sc.map, want, route, 0, n)
        g.close()
