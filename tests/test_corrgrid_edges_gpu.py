"""The correlation-grid build on the device (rebuild_grid_dev: k_find_valid, k_smear_gather<HK>, k_mark_centres +
k_smear_list, k_add_scans_serial, k_anchor_chain / anchor_spec_block) against the CPU oracle on the directed scenarios of
tests/corrgrid_cases.py, through every route that builds a grid: the valid mask, AddScans (+ the parity planes, through the
coarse numerators of one scan), the scan cache's MatchScan and the streaming front-end's anchor rows -- and one matcher
rebuilt past the wrap of its 8-bit mark epoch.  Everything is compared bit for bit: tests/test_corrgrid_cases_oracle.py
asserts that no scenario rests on the last bit of a sine."""
import os

import numpy as np
import pytest

import corrgrid_cases as cc
from lslam_amd import api

pytestmark = pytest.mark.gpu

SCENARIOS = cc.all_scenarios()
IDS = [s.name for s in SCENARIOS]
COARSE_ANGLES = (0.349, 0.0349)


def make_port(oracle_lib, cfg, laser):
    ocfg = oracle_lib.default_cfg(search_size=cfg.search, resolution=cfg.resolution, smear_deviation=cfg.smear)
    return oracle_lib.PortKarto(ocfg, oracle_lib.laser_struct(laser, cfg.threshold))


def make_matcher(ctx, cfg, laser):
    gcfg = api.baseline_config(search_size=cfg.search, resolution=cfg.resolution, smear_deviation=cfg.smear,
                               range_threshold=cfg.threshold)
    return api.ScanMatcher(ctx, gcfg, api.laser_params(laser, cfg.threshold))


def diff_text(got, want):
    """the first differing grid bytes as (row, column, device, oracle)"""
    ys, xs = np.nonzero(got != want)
    return "%d bytes differ: %s" % (len(ys), [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in list(zip(ys, xs))[:12]])


def assert_grid(gm, port):
    got, want = gm.GetCorrelationGrid(), port.grid()
    assert got.shape == want.shape
    assert np.array_equal(got, want), diff_text(got, want)  # border and pad columns included
    assert np.array_equal(gm.grid_info()["offset"], port.grid_info()["offset"])


def query_of(sc):
    """the scan of the window whose sensor is nearest the grid centre, at its own pose -- its points fall on the cells it
    occupied -- where every reading stays inside the ROI from every node of the coarse lattice (the reference throws on
    a cell outside the grid); at the grid centre's pose otherwise"""
    b = int(np.argmin(np.hypot(*(sc.poses[:, :2] - sc.center[:2]).T)))
    r = sc.ranges[b]
    reach = np.abs(r[np.isfinite(r)]).max(initial=0.0) + cc.coarse_lattice(sc.cfg)[0] + 2 * sc.cfg.resolution
    half = 0.5 * (cc.geometry(sc.cfg)["roi"] - 1) * sc.cfg.resolution
    if np.abs(sc.poses[b, :2] - sc.center[:2]).max() + reach < half:
        return r, sc.poses[b]
    return r, sc.center


def assert_sums(gm, port, cfg, ranges, pose):
    off, res = cc.coarse_lattice(cfg)
    _, _, _, st, want = port.correlate_scan(ranges, pose, pose, off, res, *COARSE_ANGLES, True, False, want_sums=True)
    assert st == 0
    assert np.array_equal(gm.coarse_sums(ranges, pose), want)


ROUTE_PROFILE = {  # launch names a rebuild must / must not show (lslam_profile_read)
    "gather": ({"find_valid", "smear"}, {"grid_clear", "mark_centres", "add_scans_serial"}),  # clear-free: marks + gather
    "listed": ({"grid_clear", "find_valid", "mark_centres", "smear"}, {"add_scans_serial"}),
    "serial": ({"grid_clear", "find_valid", "add_scans_serial"}, {"mark_centres", "smear"}),
}


@pytest.mark.parametrize("sc", SCENARIOS, ids=IDS)
def test_valid_mask(ctx, oracle_lib, sc):
    port, gm = make_port(oracle_lib, sc.cfg, sc.laser), make_matcher(ctx, sc.cfg, sc.laser)
    try:
        assert gm.num_beams == port.num_beams == sc.laser.n_ranges
        for b in range(len(sc.poses)):
            pts = port.point_readings(sc.ranges[b], sc.poses[b])
            want = cc.find_valid_walk(pts, sc.center[:2])["valid"]
            mask = gm.valid_mask(sc.ranges[b], sc.poses[b], sc.center[:2])
            assert np.flatnonzero(mask).tolist() == want, b
            # the reference keeps an order-preserving subset, NaN points included: compare as point lists
            assert pts[mask.astype(bool)].tobytes() == port.find_valid_points(pts, sc.center[:2]).tobytes(), b
    finally:
        gm.close()


@pytest.mark.parametrize("sc", SCENARIOS, ids=IDS)
def test_add_scans_grid_and_sums(ctx, oracle_lib, sc):
    port, gm = make_port(oracle_lib, sc.cfg, sc.laser), make_matcher(ctx, sc.cfg, sc.laser)
    try:
        assert gm.grid_info()["kernel_size"] == sc.cfg.kernel
        port.set_base_scans(sc.ranges, sc.poses, sc.center)
        ctx.profile(True)
        ctx.profile_reset()
        gm.AddScans(sc.ranges, sc.poses, sc.center)
        prof = ctx.profile_read()
        ctx.profile(False)
        must, must_not = ROUTE_PROFILE[sc.route]
        assert must <= set(prof) and not (must_not & set(prof)), (sc.route, sorted(prof))
        assert_grid(gm, port)
        assert_sums(gm, port, sc.cfg, *query_of(sc))  # the planes the gather wrote / the rebuild left to be derived
        # again on the same matcher: the window reversed (only the serial kernel may care) and, where it has more than one
        # scan, without its first -- that scan's cells still carry the last epoch's tag and must not be centres any more
        keep = slice(None, 0, -1) if len(sc.poses) > 1 else slice(None)
        port.set_base_scans(sc.ranges[keep], sc.poses[keep], sc.center)
        gm.AddScans(sc.ranges[keep], sc.poses[keep], sc.center)
        assert_grid(gm, port)
    finally:
        gm.close()


def _record(t):
    resp, pose, cov = t
    return np.concatenate([[resp], pose, cov.ravel()]).tobytes()


@pytest.mark.parametrize("sc", SCENARIOS, ids=IDS)
def test_scan_cache_match_scan(ctx, oracle_lib, sc):
    """ScanCache.put + MatchScan on a second matcher: the window named by ids (slot list in the clear-free form; gathered
    into a contiguous workspace for 37 x 37, 41 x 41 and 2048 beams) builds the oracle's grid, and the record is
    ScanMatcher.MatchScan's byte for byte."""
    port = make_port(oracle_lib, sc.cfg, sc.laser)
    plain, cached = make_matcher(ctx, sc.cfg, sc.laser), make_matcher(ctx, sc.cfg, sc.laser)
    cache = api.ScanCache(ctx, api.laser_params(sc.laser, sc.cfg.threshold))
    try:
        B = len(sc.poses)
        if sc.claims.get("same_scan"):  # one scan named B times
            ids = np.zeros(B, dtype=np.int64)
            cache.put(0, sc.ranges[0])
        else:
            ids = np.arange(B)
            for b in range(B):
                cache.put(b, sc.ranges[b])
        q = sc.ranges[0]
        a = plain.MatchScan(q, sc.center, sc.ranges, sc.poses)
        ctx.profile(True)
        ctx.profile_reset()
        b = cache.MatchScan(cached, ids, sc.poses, sc.center, query_id=-1, query_ranges=q)
        prof = ctx.profile_read()
        ctx.profile(False)
        must, must_not = ROUTE_PROFILE[sc.route]
        assert must <= set(prof) and not (must_not & set(prof)), (sc.route, sorted(prof))
        assert _record(a) == _record(b)
        port.set_base_scans(sc.ranges, sc.poses, sc.center)
        assert_grid(cached, port)
        assert_grid(plain, port)
    finally:
        cache.close()
        cached.close()
        plain.close()


def _frontend_groups():
    """the scans of the walk families, grouped by laser: each group is one short drive of a front-end"""
    groups = {}
    for sc in SCENARIOS:
        # (not the scan that is exact at its own pose only: the front-end poses every scan itself)
        if sc.family in ("non_finite", "chains", "successors") and sc.cfg.name == "hk1_176" and not sc.exact:
            groups.setdefault(sc.laser, []).append(sc)
    return sorted(groups.items(), key=lambda kv: kv[0].n_ranges)


FE_GROUPS = _frontend_groups()


@pytest.mark.parametrize("laser,group", FE_GROUPS, ids=["n%d" % l.n_ranges for l, _ in FE_GROUPS])
def test_frontend_anchor_rows(ctx, oracle_lib, laser, group):
    """FrontEnd.Process over the walk scenarios' scans, speculative anchor chains on and off: the row the ring keeps for
    every processed scan is the Python walk's anchors on the scan's points at the pose the front-end gave it."""
    cfg = cc.CONFIGS["hk1_176"]
    port = make_port(oracle_lib, cfg, laser)
    handed = {}
    for spec in (1, 0):
        os.environ["LSLAM_FE_SPEC_CHAIN"] = str(spec)
        try:
            gm = make_matcher(ctx, cfg, laser)
            fe = api.FrontEnd(gm, scan_buffer_size=8, min_travel_distance=0.2)
        finally:
            del os.environ["LSLAM_FE_SPEC_CHAIN"]
        try:
            taken = []
            for k, sc in enumerate(group + group[:3]):
                ok, _, _, _ = fe.Process(sc.ranges[0], np.array([0.3 + 0.25 * k, -0.2, 0.5]))
                if ok:
                    taken.append(sc)
            # the odometry moves 0.25 m per scan, more than the minimum travel distance: every scan is processed
            assert [sc.name for sc in taken] == [sc.name for sc in group + group[:3]] and fe.num_scans() == len(taken)
            for i, sc in enumerate(taken):
                sensor = port.sensor_pose_from_robot(fe.scan_pose(i))
                walk = cc.find_valid_walk(port.point_readings(sc.ranges[0], sensor), sensor[:2])
                d2 = walk["d2"][np.isfinite(walk["d2"])]
                assert np.abs(d2 - 0.1 * 0.1).min(initial=1.0) > cc.D2_MARGIN, (sc.name, "the pose put a distance on the threshold")
                assert fe.anchor_row(i).tolist() == walk["anchors"], (spec, i, sc.name)
            handed[spec] = fe.spec_chain_stats()["handed"]
        finally:
            fe.close()
            gm.close()
    assert handed[1] > 0 and handed[0] == 0


def test_epochs_wrap(ctx, oracle_lib):
    """One matcher at 3 x 3 (176 x 175 bytes) rebuilt 258 times (corrgrid_cases.epoch_sequence): the mark plane is never
    cleared, only tagged with an 8-bit epoch, and reset when the epoch wraps.  Windows A and B alternate and re-tag their
    own cells every time; the sectors C1 and C2 are built once, at rebuilds 1 and 2, so their marks still hold the epochs 1
    and 2 when the epoch wraps at rebuild 257 -- without the reset C1's cells would be centres again at rebuild 257 and
    C2's at 258 (tests/test_corrgrid_cases_oracle.py runs the sequence on a model of the plane, with and without the
    reset).  Rebuild 100 is an empty window (the clearing path); before rebuild 200 the grid is overwritten with 255s
    behind the rebuild's back."""
    laser, cfg, windows, center = cc.epoch_windows()
    port, gm = make_port(oracle_lib, cfg, laser), make_matcher(ctx, cfg, laser)
    try:
        want = {}
        for key, (r, p) in windows.items():
            port.set_base_scans(r, p, center)
            want[key] = port.grid()
        assert want["A"].any() and want["B"].any() and not want["empty"].any()
        assert not ((want["A"] > 0) & (want["B"] > 0)).any()  # disjoint
        for once, again in (("A+C1", "A"), ("B+C2", "B")):  # the once-only sectors reach nothing of A or B
            own = (want[once] > 0) & ~(want[again] > 0)
            assert own.any() and not (own & ((want["A"] > 0) | (want["B"] > 0))).any()
        assert gm.grid_info()["stride"] == 176 and gm.grid_info()["height"] == 175
        q, qp = windows["A+C1"][0][1], windows["A+C1"][1][1]  # sector C1 at its own pose: on stale C1 marks it would score
        for i, key in cc.epoch_sequence():
            r, p = windows[key]
            if i == 200:
                gm.set_grid(np.full_like(want["A"], 255), port.grid_info()["offset"])
            gm.AddScans(r, p, center)
            if i in cc.EPOCH_CHECKS:
                got = gm.GetCorrelationGrid()
                assert np.array_equal(got, want[key]), (i, key, diff_text(got, want[key]))
            if i in (1, 255, 256, 257):
                port.set_base_scans(r, p, center)
                assert_sums(gm, port, cfg, q, qp)
    finally:
        gm.close()
