"""The Hector localiser (lslam_hector_loc_*, api.HectorLocaliser; csrc/hector_loc_impl.hpp: k_hl_container, k_hl_track_*) on the
scenarios of tests/hector_loc_cases.py.  The yardstick everywhere but in the last test is BIT EQUALITY with a lslam_hector
processor on the same map whose update thresholds are both +inf (its gate never fires), run alone over the tracker's taken
entries in calls of the same form -- the path tests/test_hector_stream_gpu.py holds to the reference's own processor -- so no
tolerance appears there.  The maps are built once per module and then only read: every test ends by comparing every plane of
the maps it used with the bytes taken when they were built."""
import os

import numpy as np
import pytest

from lslam_amd import api

import deskew_stream_cases as D
import hector_fleet_cases as F
import hector_loc_cases as L
import hector_stream_cases as S
import hector_sync_cases as H

pytestmark = pytest.mark.gpu
f32 = np.float32
STRIDE = api.MSYNC_RECORD.itemsize // 4


def planes(m):
    return [m.logodds(lv).tobytes() for lv in range(m.levels)]


def solo_on(m):
    """The yardstick: a streamed processor whose gate never fires (x > +inf is false for every float)."""
    h = api.HectorProcessor(m)
    h.set_update_thresholds(L.INF, L.INF)
    return h


class Built:
    def __init__(self, m):
        self.m = m
        self.planes = planes(m)
        assert np.frombuffer(self.planes[0], f32).any()

    def unchanged(self):
        assert planes(self.m) == self.planes


@pytest.fixture(scope="module")
def edge_maps(ctx):
    """edges(3) and edges(1) mapped by the streamed processor from their own readings (256^2)."""
    out = {}
    for levels in (3, 1):
        sc = S.edges(levels)
        m = S.device_map(api, ctx, sc)
        h = api.HectorProcessor(m)
        h.set_update_thresholds(sc.min_dist, sc.min_angle)
        rec = h.process_many(sc.ranges, api.hector_scan(sc.laser))
        assert (rec["updated"] != 0).sum() >= 2
        h.close()
        out[levels] = Built(m)
    yield out
    for b in out.values():
        b.m.close()


@pytest.fixture(scope="module")
def chain_maps(ctx):
    """chain60 (1024^2 x 3 levels, 1081 beams) mapped under LSLAM_GN_THREADS 256 and 512 (read at map creation)."""
    sc = S.chain60()
    out, old = {}, os.environ.get("LSLAM_GN_THREADS")
    try:
        for threads in (256, 512):
            os.environ["LSLAM_GN_THREADS"] = str(threads)
            m = S.device_map(api, ctx, sc)
            h = api.HectorProcessor(m)
            h.process_many_points(sc.containers)
            h.close()
            out[threads] = Built(m)
    finally:
        if old is None:
            os.environ.pop("LSLAM_GN_THREADS", None)
        else:
            os.environ["LSLAM_GN_THREADS"] = old
    yield out
    for b in out.values():
        b.m.close()


def stack(fleet, lo, hi, what):
    return np.stack([[getattr(mb, what)[k] for mb in fleet.members] for k in range(lo, hi)])


def loc_call(fleet, loc, lo, hi, form, hints=None):
    act = None if fleet.active[lo:hi].all() else fleet.active[lo:hi]
    if form == "points":
        return loc.process_many_points([[mb.containers[k] for mb in fleet.members] for k in range(lo, hi)], hints, act)
    return loc.process_many(stack(fleet, lo, hi, "ranges"), api.hector_scan(fleet.members[0].sc.laser), hints, act)


def solo_call(fleet, r, h, lo, hi, form, hints=None):
    """Tracker r's taken entries of steps [lo, hi) through the solo processor -> records (None: it has none)."""
    mb = fleet.members[r]
    idx = [k for k in range(lo, hi) if fleet.active[k, r]]
    if not idx:
        return None
    hh = None if hints is None else np.asarray(hints)[[k - lo for k in idx], r]
    if form == "points":
        return h.process_many_points([mb.containers[k] for k in idx], hh)
    return h.process_many(mb.ranges[idx], api.hector_scan(mb.sc.laser), hh)


def hold_to_solo(fleet, loc, rec, m, form, calls, hints=None):
    """Every tracker's taken records and its state against the solo run made in the same calls; the others are blank."""
    assert rec.shape == fleet.active.shape and (rec["updated"] == 0).all()
    for r in range(len(fleet.members)):
        h = solo_on(m)
        got = [solo_call(fleet, r, h, lo, hi, form, None if hints is None else hints[lo:hi]) for lo, hi in calls]
        got = [g for g in got if g is not None]
        mine = rec[:, r]
        if got:
            assert np.ascontiguousarray(mine[fleet.active[:, r]]).tobytes() == np.concatenate(got).tobytes(), r
        pose, cov, _ = h.state()
        lp, lc = loc.state(r)
        assert lp.tobytes() == pose.tobytes() and lc.tobytes() == cov.tobytes(), r
        idle = mine[~fleet.active[:, r]]
        assert all(H.not_taken(x) for x in idle)
        h.close()


# ---- 1. solo equivalence, ranges form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False], ids=["calls_1_2_7_2", "one_call"])
@pytest.mark.parametrize("R", [1, 3, 5])
@pytest.mark.parametrize("levels", [3, 1])
def test_solo_equivalence_ranges(ctx, edge_maps, levels, R, split):
    """1. R trackers streaming edges' scans rolled by r, in calls of 1, 2, 7 and 2 steps and in one call: records and state
    bit for bit.  Every block sees the long container, then the empty one, then the one-point one in consecutive steps."""
    b = edge_maps[levels]
    fleet = L.logs(levels, R)
    calls = fleet.calls if split else [(0, fleet.n_steps)]
    loc = api.HectorLocaliser(b.m, R)
    assert loc.size == R
    rec = np.concatenate([loc_call(fleet, loc, lo, hi, "ranges") for lo, hi in calls])
    st = loc.stats()
    print("localiser stats", st)
    assert (st["steps"], st["scans"], st["calls"]) == (12, 12 * R, len(calls))
    assert st["launches"] == 2 * len(calls) and st["track_launches"] == len(calls)
    assert st["host_syncs"] == len(calls) + 1  # one per call, and the first call's cos/sin table
    for r in range(R):
        k = L.log_order(r).index(L.LONG_EMPTY_SHORT[0])
        n = rec["n_points"][k:k + 3, r]
        assert n[0] > 64 and n[1] == 0 and n[2] == 1, n
        assert rec["pose"][k + 1, r].tobytes() == rec["pose"][k, r].tobytes()          # the empty scan returns its start pose
        assert rec["cov"][k + 1, r].tobytes() == rec["cov"][k, r].tobytes()            # and leaves the covariance
    assert sorted(set(rec["n_points"][:, 0].tolist()) & {1, 63, 64, 65}) == [1, 63, 64, 65]
    hold_to_solo(fleet, loc, rec, b.m, "ranges", calls)
    loc.close()
    b.unchanged()


# ---- 2. forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(L.FORMS))
def test_forms(ctx, chain_maps, name):
    """2. the register form at 256 and 512 threads on the 1081-beam map; a call staged in LDS (1800 points at 512 threads) and
    one read from memory (7400 points), each against the solo processor in a call of the same capacity."""
    threads, pad, form = L.FORMS[name]
    b = chain_maps[threads]
    fleet = L.form_logs(name)
    (lo, hi), = fleet.calls
    assert F.form_of(threads, fleet.capacity(lo, hi)) == form
    assert all(F.form_of(threads, fleet.solo_capacity(r, lo, hi)) == form for r in range(L.FORM_R))
    loc = api.HectorLocaliser(b.m, L.FORM_R)
    rec = loc_call(fleet, loc, lo, hi, "points")
    assert loc.stats()["launches"] == 1  # the container form: the tracking kernel alone
    assert rec["n_points"].max() == (pad or rec["n_points"].max()) and rec["n_points"].min() > 300
    d = np.abs(rec["pose"][:, 0] - fleet.members[0].sc.truth[:hi]).max()
    print("%s: worst |pose - truth| of tracker 0 = %.3g" % (name, d))
    assert d < 0.1  # (it does localise: the scans are the map's own, 0.04 m apart)
    hold_to_solo(fleet, loc, rec, b.m, "points", fleet.calls)
    loc.close()
    b.unchanged()


# ---- 3. ragged -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["ranges", "points"])
def test_ragged(ctx, edge_maps, form):
    """3. R = 5 under RAGGED_MASK in its two calls: a step nobody takes, a tracker idle for a whole call, different rates."""
    b = edge_maps[3]
    fleet = F.ragged()
    loc = api.HectorLocaliser(b.m, 5)
    (lo0, hi0), (lo1, hi1) = fleet.calls
    first = loc_call(fleet, loc, lo0, hi0, form)
    idle, _ = F.RAGGED_IDLE
    before = [a.tobytes() for a in loc.state(idle)]
    assert any(np.frombuffer(x, f32).any() for x in before)
    second = loc_call(fleet, loc, lo1, hi1, form)
    assert [a.tobytes() for a in loc.state(idle)] == before
    rec = np.concatenate([first, second])
    assert all(H.not_taken(x) for x in rec[F.RAGGED_EMPTY_STEP])
    assert loc.stats()["scans"] == int(fleet.active.sum())
    hold_to_solo(fleet, loc, rec, b.m, form, fleet.calls)
    loc.close()
    b.unchanged()


def test_refusals(ctx, edge_maps):
    """What a call refuses before anything is enqueued: an inactive entry with points, first / count out of range, more than
    65536 readings, more than 65535 trackers, an ordered-sums map, more than 8 levels; n_steps == 0 does nothing."""
    b = edge_maps[3]
    sc = S.edges(3)
    scan = api.hector_scan(sc.laser)
    L_ = api.lib()
    loc = api.HectorLocaliser(b.m, 2)

    def refused(code, fn):
        with pytest.raises(api.LslamError) as e:
            fn()
        assert e.value.code == code, e.value

    refused(-1, lambda: loc.process_many_points([[sc.containers[0], sc.containers[1]]], None, [[1, 0]]))
    refused(-1, lambda: loc.set_poses(np.zeros((2, 3), f32), first=1))
    refused(-1, lambda: loc.set_poses(np.zeros((1, 3), f32), first=2 + 1))
    refused(-1, lambda: loc.state(2))
    refused(-8, lambda: loc.process_many(np.ones((1, 2, 65537), f32), scan))
    refused(-8, lambda: api.HectorLocaliser(b.m, 65536))
    out = np.zeros(2, api.HECTOR_RECORD)
    assert L_.lslam_hector_loc_process_many_points(loc.h, 0, None, None, None, None, out.ctypes.data) == 0
    st = loc.stats()
    assert (st["calls"], st["launches"], st["host_syncs"]) == (0, 0, 0)
    assert loc.process_many(sc.ranges[:1].repeat(2, axis=0)[None], scan)["n_points"].min() > 60  # (and still works)
    loc.close()
    ordered = api.OccGridMap(ctx, 64, 64, S.CELL, S.offset(64), levels=2)
    ordered.set_option("ordered_sums", 1)
    refused(-8, lambda: api.HectorLocaliser(ordered, 1))
    ordered.close()
    deep = api.OccGridMap(ctx, 1024, 1024, S.CELL, S.offset(1024), levels=9)
    assert deep.levels == 9
    refused(-8, lambda: api.HectorLocaliser(deep, 1))
    deep.close()
    b.unchanged()


# ---- 4. hints ------------------------------------------------------------------------------------------------------------------
def test_hints(ctx, edge_maps):
    """4. per-entry pose_hints, some of them far outside the map: every point is out of bounds there, no sum moves, and the
    pose comes back as the arithmetic gives it -- the solo run's."""
    b = edge_maps[3]
    R = 3
    fleet = L.logs(3, R)
    sc = fleet.members[0].sc
    rng = np.random.default_rng(3)
    hints = np.stack([[sc.truth[L.log_order(r)[k]] for r in range(R)] for k in range(fleet.n_steps)]).astype(f32)
    hints += rng.uniform(-0.01, 0.01, hints.shape).astype(f32)
    far = [(2, 0), (2, 1), (7, 2), (11, 0)]
    for k, r in far:
        hints[k, r] = L.hint_far(sc)
    loc = api.HectorLocaliser(b.m, R)
    rec = loc_call(fleet, loc, 0, fleet.n_steps, "ranges", hints)
    for k, r in far:
        assert rec["n_points"][k, r] > 0
        # no step was taken: the hint, through the levels' map <-> world transforms (a few float32 roundings)
        assert np.allclose(rec["pose"][k, r, :2], L.hint_far(sc)[:2], rtol=1e-5, atol=0.0)
    near = np.ones((fleet.n_steps, R), bool)
    near[tuple(zip(*far))] = False
    near &= rec["n_points"] > 70  # (the scans masked down to a few beams constrain little)
    d = np.abs(rec["pose"] - hints)[near].max()
    print("worst |pose - hint| over the full scans hinted near their truth: %.3g" % d)
    assert d < 0.1
    hold_to_solo(fleet, loc, rec, b.m, "ranges", [(0, fleet.n_steps)], hints)
    loc.close()
    b.unchanged()


# ---- 5. clouds -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=L.TAKE_LOGS)
def synced_log(ctx, request):
    """A log of hector_sync_cases: its map, built by process_synced, and -- from a fresh node's scans_dev -- its clouds, valid
    bytes and lslam_msync_records in HBM, with their host copies."""
    name = request.param
    c = H.case(name)
    scan = H.hector_scan(c)
    r, t, ti, iseen, oseen = H.scan_args(c)
    m = D.device_map(ctx, H.LEVELS[name])
    h, ms = D.processor(m), api.MotionSync(ctx, c["use_imu"], c["use_odom"])
    H.push_all(ms, c)
    built, _ = h.process_synced(ms, c["laser"], r, scan, t, ti, iseen, oseen)
    assert (built["updated"] != 0).any()
    h.close()
    ms.close()
    n, nr = r.shape
    ms = api.MotionSync(ctx, c["use_imu"], c["use_odom"])
    H.push_all(ms, c)
    ptrs = d_r, d_xyz, d_valid, d_rec = ctx.alloc(r.nbytes), ctx.alloc(n * nr * 12), ctx.alloc(n * nr), ctx.alloc(n * api.MSYNC_RECORD.itemsize)
    ctx.upload(d_r, np.ascontiguousarray(r, f32))
    ms.scans_dev(c["laser"], nr, d_r, nr, t, ti, d_xyz, d_valid, d_rec, iseen, oseen)
    ctx.synchronize()
    xyz, valid, srec = np.zeros((n, nr, 3), f32), np.zeros((n, nr), np.uint8), np.zeros(n, api.MSYNC_RECORD)
    for p, a in ((d_xyz, xyz), (d_valid, valid), (d_rec, srec)):
        ctx.download(p, a)
    assert srec["status"].tolist() == H.STATUSES[name]  # the take pattern the cases module claims
    yield {"name": name, "scan": scan, "built": Built(m), "n": n, "nr": nr, "d_xyz": d_xyz, "d_valid": d_valid, "d_rec": d_rec,
           "xyz": xyz, "valid": valid, "take": srec["status"] > 0}
    ms.close()
    for p in ptrs:
        ctx.free(p)
    m.close()


def test_clouds(ctx, synced_log):
    """5. the _dev form on MotionSync.scans_dev's output, its take words the records' status at stride 22, equals the solo
    process_many_clouds_dev over the same block, and the host form with the flags as bytes; two trackers with different take
    patterns in one call each equal their own solo run."""
    s = synced_log
    b, scan, n, nr, take = s["built"], s["scan"], s["n"], s["nr"], s["take"]
    loc = api.HectorLocaliser(b.m, 1)
    dev = loc.process_many_clouds_dev(n, nr, s["d_xyz"], s["d_valid"], s["d_rec"], STRIDE, scan)
    assert loc.stats()["launches"] == 2 and loc.stats()["host_syncs"] == 1 and loc.stats()["scans"] == int(take.sum())
    h = solo_on(b.m)
    want = h.process_many_clouds_dev(n, nr, s["d_xyz"], s["d_valid"], s["d_rec"], STRIDE, scan)
    assert dev[:, 0].tobytes() == want.tobytes()
    assert [H.not_taken(x) for x in want] == (~take).tolist() and want["n_points"].max() > 32
    assert b"".join(a.tobytes() for a in loc.state(0)) == b"".join(a.tobytes() for a in h.state()[:2])
    h.close()
    loc.close()
    loc = api.HectorLocaliser(b.m, 1)
    host = loc.process_many_clouds(s["xyz"][:, None], scan, s["valid"][:, None], take[:, None])
    assert host.tobytes() == dev.tobytes()
    loc.close()
    # two trackers on the same clouds: the log's own pattern, and a pattern of bytes -- with valid = None as well
    other = np.resize(np.array(H.TAKE_PATTERNS["mixed"], bool), n)
    both = np.stack([take, other], axis=1)
    loc = api.HectorLocaliser(b.m, 2)
    two = loc.process_many_clouds(np.repeat(s["xyz"][:, None], 2, axis=1), scan, np.repeat(s["valid"][:, None], 2, axis=1), both)
    assert two[:, 0].tobytes() == want.tobytes()
    h = solo_on(b.m)
    assert two[:, 1].tobytes() == h.process_many_clouds(s["xyz"], scan, s["valid"], other).tobytes()
    h.close()
    loc.close()
    loc, h = api.HectorLocaliser(b.m, 1), solo_on(b.m)
    a = loc.process_many_clouds(s["xyz"][:, None], scan, None, other[:, None])
    assert a[:, 0].tobytes() == h.process_many_clouds(s["xyz"], scan, None, other).tobytes()
    h.close()
    loc.close()
    b.unchanged()


# ---- 6. chunking ---------------------------------------------------------------------------------------------------------------
def test_chunking_changes_no_bit(ctx, edge_maps):
    """6a. LSLAM_HECTOR_LOC_OPT_MAX_STEPS_PER_LAUNCH = 1, 2, 3 against the default: the same bytes; launches = 2 x chunks."""
    b = edge_maps[3]
    R = 3
    fleet = L.logs(3, R)
    runs = {}
    for steps in (0, 1, 2, 3):
        loc = api.HectorLocaliser(b.m, R)
        loc.set_option("max_steps_per_launch", steps)
        rec = loc_call(fleet, loc, 0, fleet.n_steps, "ranges")
        st = loc.stats()
        chunks = 1 if steps == 0 else -(-fleet.n_steps // steps)
        assert (st["launches"], st["track_launches"], st["calls"]) == (2 * chunks, chunks, 1), (steps, st)
        runs[steps] = rec.tobytes() + b"".join(a.tobytes() for r in range(R) for a in loc.state(r))
        pts = loc_call(fleet, loc, 0, fleet.n_steps, "points")  # the container form, chained on: one launch per chunk
        assert loc.stats()["launches"] - st["launches"] == chunks
        runs[steps] += pts.tobytes()
        loc.close()
    assert runs[1] == runs[0] and runs[2] == runs[0] and runs[3] == runs[0]
    b.unchanged()


def test_launches_per_chunk_do_not_depend_on_R_or_steps(ctx, edge_maps):
    """6b. 2 launches and one wait per call for R = 1 and R = 300 (more blocks than CUs), for 2 and for 16 steps; 300 trackers
    fed one log give 300 times the records of one."""
    b = edge_maps[3]
    sc = S.edges(3)
    scan = api.hector_scan(sc.laser)
    log = sc.ranges[[k % 12 for k in range(16)]]
    seen = {}
    for R in (1, 300):
        loc = api.HectorLocaliser(b.m, R)
        loc.process_many(np.repeat(log[:1, None], R, axis=1), scan)  # (the cos/sin table's wait is this call's)
        for steps in (2, 16):
            before = loc.stats()
            rec = loc.process_many(np.repeat(log[:steps, None], R, axis=1), scan)
            st = loc.stats()
            assert (st["launches"] - before["launches"], st["track_launches"] - before["track_launches"],
                    st["host_syncs"] - before["host_syncs"], st["scans"] - before["scans"]) == (2, 1, 1, steps * R), (R, steps, st)
            seen[(R, steps)] = rec
        loc.close()
    for steps in (2, 16):
        one, many = seen[(1, steps)], seen[(300, steps)]
        assert all(np.ascontiguousarray(many[:, r]).tobytes() == one[:, 0].tobytes() for r in range(300)), steps
    b.unchanged()


# ---- 7. the map moves between calls --------------------------------------------------------------------------------------------
def test_map_changes_between_calls(ctx, edge_maps):
    """7. call, lslam_map_update_by_scan of one scan, call: the second call sees the map as it then is -- equal to the solo run
    made the same way on a copy -- and neither call disturbs the map's cached container, its count or the resident container."""
    b = edge_maps[3]
    sc = S.edges(3)
    scan = api.hector_scan(sc.laser)
    R = 2
    fleet = L.logs(3, R)
    moved = (sc.containers[2], (0.0, 0.0), np.array([0.05, -0.02, 0.3], f32))

    def copy():
        m = S.device_map(api, ctx, sc)
        for lv in range(m.levels):
            m.write_logodds_dev(lv, b.m.cells_dev_ptr(lv))
        m.setScan(sc.ranges[1], scan)                        # a resident container
        m.matchData((0.0, 0.0, 0.0), sc.containers[4])       # and a cached one
        return m

    m = copy()
    loc = api.HectorLocaliser(m, R)
    before = (m.cached_points(), m.container()[0].tobytes(), m.container()[1].tobytes())
    first = loc_call(fleet, loc, 0, 6, "ranges")
    assert (m.cached_points(), m.container()[0].tobytes(), m.container()[1].tobytes()) == before
    m.updateByScan(*moved)  # levels above 0 are fed from the cached container: the planes tell whether it was disturbed
    second = loc_call(fleet, loc, 6, 12, "ranges")
    after = planes(m)
    assert after != b.planes
    for r in range(R):
        ms = copy()
        h = solo_on(ms)
        a = solo_call(fleet, r, h, 0, 6, "ranges")
        ms.matchData((0.0, 0.0, 0.0), sc.containers[4])      # (the solo processor does cache its containers: put the copy's back)
        ms.updateByScan(*moved)
        assert planes(ms) == after, r
        c = solo_call(fleet, r, h, 6, 12, "ranges")
        assert first[:, r].tobytes() == a.tobytes() and second[:, r].tobytes() == c.tobytes(), r
        ms.close()
    quiet = copy()  # the same update on a copy no localiser ran on
    quiet.updateByScan(*moved)
    assert planes(quiet) == after
    quiet.close()
    m.close()
    b.unchanged()


# ---- 8. against the reference itself -------------------------------------------------------------------------------------------
def test_against_the_reference(ctx, oracle_lib):
    """8. The reference's own HectorSlamProcessor maps chain60, then -- its thresholds at +inf -- localises the first 12 scans
    again, chained from (0, 0, 0); the device localiser does the same on the reference's planes, written into a device map
    level by level.  Held to the bounds tests/test_hector_stream_gpu.py applies (hector_stream_cases.hold_to_reference)."""
    po = oracle_lib
    if not po.have_ref_hector():
        pytest.skip("oracle/_ref not built (needs the reference's sources at build time)")
    sc = S.chain60()
    proc = po.RefHectorProcessor(S.CELL, sc.n, sc.n, (0.5, 0.5), sc.levels, p_free=0.4, p_occ=0.9)
    est = np.zeros(3, f32)
    for pts in sc.containers:
        proc.update(pts, est)
        est, _ = proc.last_pose()
    ref_planes = [proc.logodds(lv) for lv in range(sc.levels)]
    proc.L.href_proc_set_update_thresholds(proc.h, L.INF, L.INF)
    est, poses, covs, upd = np.zeros(3, f32), [], [], []
    for pts in sc.containers[:12]:
        upd.append(proc.update(pts, est))
        est, cov = proc.last_pose()
        poses.append(est.copy())
        covs.append(cov.copy())
    assert [p.tobytes() for p in ref_planes] == [proc.logodds(lv).tobytes() for lv in range(sc.levels)] and not any(upd)
    proc.close()
    ref = S.RefRun(np.array(upd), np.array(poses), np.array(covs), np.zeros((12, 3), f32), ref_planes)
    m = S.device_map(api, ctx, sc)
    for lv, p in enumerate(ref_planes):
        m.write_logodds(lv, p)
    loc = api.HectorLocaliser(m, 1)
    rec = loc.process_many_points([[c] for c in sc.containers[:12]])
    S.hold_to_reference("localiser on the reference's planes", ref, rec[:, 0], [m.logodds(lv) for lv in range(sc.levels)])
    m.close()
