"""The gated streamed processor on the device: api.HectorProcessor.process_many_clouds[_dev] (clouds that are de-skewed
already, with a per-scan take word) and process_synced (lesson5's node in front of update(), the take word being the status
its walk wrote), on the logs of tests/hector_sync_cases.py and the 12-scan sequence of tests/deskew_stream_cases.py, 512^2
maps of 2 and 3 levels.

Everything is compared bit for bit -- records, every level's plane, state(), container() and cached_points() -- because the
gated kernels run the device bodies of the ungated chain on the same inputs; only test 7 (the host-driven loop, another
matcher call sequence) is held to hector_stream_cases.POSE_TOL.  Every test prints what it measured (pytest -s)."""
import numpy as np
import pytest

from lslam_amd import api

import deskew_stream_cases as D
import hector_stream_cases as S
import hector_sync_cases as H

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, UNSUPPORTED = -1, -8
# test 6's chain run and test 7: setMapUpdateMinDistDiff lowered from the node's 0.4 m to deskew_stream_cases' 0.1 m.  The logs'
# room is seen from a point that drifts about 0.06 m a scan, so a scan right behind an update stays below the gate and the one
# behind it passes it: some taken scans update the map and some do not, each some centimetres from the gate
CHAIN_MIN_DIST = {"steady": D.MIN_DIST, "imu_gap": D.MIN_DIST}


@pytest.fixture(scope="module")
def po(oracle_lib):
    if not (oracle_lib.have_ref_lesson5() and oracle_lib.have_ref_hector()):
        pytest.skip("oracle/_ref not built (needs the reference's sources at build time)")
    return oracle_lib


def fresh(ctx, levels, min_dist=None):
    m = D.device_map(ctx, levels)
    h = D.processor(m)
    if min_dist is not None:
        h.set_update_thresholds(min_dist, S.MIN_ANGLE)
    return m, h


def node(ctx, c):
    ms = api.MotionSync(ctx, c["use_imu"], c["use_odom"])
    H.push_all(ms, c)
    return ms


def synced(h, ms, c, lo=0, hi=None, hints=None, flags=None):
    r, t, ti, iseen, oseen = H.scan_args(c, lo, hi)
    return h.process_synced(ms, c["laser"], r, H.hector_scan(c), t, ti, iseen, oseen,
                            pose_hints=None if hints is None else hints[lo:hi],
                            map_without_matching=None if flags is None else flags[lo:hi])


def two_step(h, ms, c, lo=0, hi=None, hints=None, flags=None):
    """MotionSync.scans in its host form, then process_many_clouds on what it corrected."""
    r, t, ti, iseen, oseen = H.scan_args(c, lo, hi)
    xyz, valid, srec = ms.scans(c["laser"], r, t, ti, iseen, oseen)
    rec = h.process_many_clouds(xyz, H.hector_scan(c), valid, take=srec["status"] == api.MSYNC_CORRECTED,
                                pose_hints=None if hints is None else hints[lo:hi],
                                map_without_matching=None if flags is None else flags[lo:hi])
    return rec, srec


def run(ctx, name, route, chunks=None, upto=None, hints=None, flags=None, min_dist=None):
    """A log through one route on fresh handles -> (records, msync records, snapshot, hector stats, msync stats)."""
    c = H.case(name)
    n = len(c["scan_t"]) if upto is None else upto
    m, h = fresh(ctx, H.LEVELS[name], min_dist)
    ms = node(ctx, c)
    recs, srecs, k, first = [], [], 0, None
    for size in (chunks or [n]):
        a, b = route(h, ms, c, k, k + size, hints, flags)
        recs.append(a)
        srecs.append(b)
        k += size
        if first is None:
            first = (H.snapshot(m, h), h.stats())
    assert k == n
    out = (np.concatenate(recs), np.concatenate(srecs), H.snapshot(m, h), h.stats(), ms.stats(), first)
    ms.close()
    m.close()
    return out


_RUNS = {}


def whole(ctx, name, route):
    key = (name, route.__name__)
    if key not in _RUNS:
        _RUNS[key] = run(ctx, name, route)
    return _RUNS[key]


def same(a, b, what=""):
    """two snapshots, field by field"""
    for k in a:
        assert a[k] == b[k], (what, k)


# ---- 1, 2: clouds ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clouds(po, ctx):
    """sequence12, its clouds from Deskewer.batch on the host and -- Deskewer.batch_dev -- in HBM."""
    laser, seq = D.sequence12(po)
    scan = D.hector_scan(laser)
    r, params, times, rots = D.batch_inputs(seq)
    dk = api.Deskewer(ctx)
    xyz, valid = dk.batch(r, params, times, rots)
    n, nr = r.shape
    d_r, d_xyz, d_valid = ctx.alloc(r.nbytes), ctx.alloc(xyz.nbytes), ctx.alloc(n * nr)
    ctx.upload(d_r, np.ascontiguousarray(r, f32))
    dk.batch_dev(nr, d_r, nr, params, times, rots, d_xyz, d_valid)
    ctx.synchronize()
    back, vback = np.zeros_like(xyz), np.zeros((n, nr), np.uint8)
    ctx.download(d_xyz, back)
    ctx.download(d_valid, vback)
    assert back.tobytes() == xyz.tobytes() and np.array_equal(vback != 0, valid)
    xyz.setflags(write=False)
    valid.setflags(write=False)
    yield {"seq": seq, "scan": scan, "inputs": (r, params, times, rots), "xyz": xyz, "valid": valid, "d_xyz": d_xyz, "d_valid": d_valid}
    for p in (d_r, d_xyz, d_valid):
        ctx.free(p)
    dk.close()


@pytest.mark.parametrize("levels", [2, 3], ids=["2_levels", "3_levels"])
def test_cloud_form_equals_the_deskewed_form(ctx, clouds, levels):
    """1. process_many_clouds on Deskewer.batch's clouds (no take) == process_deskewed on the raw inputs; the _dev form on
    Deskewer.batch_dev's output equals both; valid=None on a block whose valid is all ones gives the bytes of passing it."""
    r, params, times, rots = clouds["inputs"]
    scan, xyz, valid = clouds["scan"], clouds["xyz"], clouds["valid"]
    m0, h0 = fresh(ctx, levels)
    want = h0.process_deskewed(r, scan, params, times, rots)
    snap = H.snapshot(m0, h0)
    assert want["n_points"].min() > 300 and 2 <= int((want["updated"] != 0).sum()) < len(want)
    assert xyz.shape[1] == 1081 and valid[:, :1024].any(1).all() and valid[:, 1024:].any(1).all()  # both compaction rounds
    m1, h1 = fresh(ctx, levels)
    got = h1.process_many_clouds(xyz, scan, valid)
    assert got.tobytes() == want.tobytes()
    same(H.snapshot(m1, h1), snap, "host form")
    m2, h2 = fresh(ctx, levels)
    dev = h2.process_many_clouds_dev(len(xyz), xyz.shape[1], clouds["d_xyz"], clouds["d_valid"], None, 1, scan)
    assert dev.tobytes() == want.tobytes()
    same(H.snapshot(m2, h2), snap, "_dev form")
    for h in (h1, h2):
        st = h.stats()
        assert (st["scans"], st["calls"], st["host_syncs"]) == (12, 1, 1), st
    ones = np.ones(valid.shape, bool)
    m3, h3 = fresh(ctx, levels)
    m4, h4 = fresh(ctx, levels)
    a = h3.process_many_clouds(xyz, scan, ones)
    b = h4.process_many_clouds(xyz, scan, None)
    assert a.tobytes() == b.tobytes() and a["n_points"].min() > 300
    same(H.snapshot(m3, h3), H.snapshot(m4, h4), "valid=None")
    print("%d levels: points per scan %s, updates %s" % (levels, want["n_points"].tolist(), want["updated"].tolist()))
    for m in (m0, m1, m2, m3, m4):
        m.close()


@pytest.mark.parametrize("pattern", sorted(H.TAKE_PATTERNS))
def test_take_equals_the_compressed_subset(ctx, clouds, pattern):
    """2. a call over 12 clouds with a take pattern == one call over only the taken clouds; the other records are zero with
    n_points = -1; `scans` advances by the taken count, calls and host_syncs by 1; the _dev form at stride 1, and at stride 22
    on the status field of an uploaded MSYNC_RECORD array, equals the host form."""
    scan, xyz, valid = clouds["scan"], clouds["xyz"], clouds["valid"]
    take = np.array(H.TAKE_PATTERNS[pattern], bool)
    idx = np.flatnonzero(take)
    levels = 3
    mc_, hc = fresh(ctx, levels)
    want = hc.process_many_clouds(xyz[idx], scan, valid[idx])
    snap = H.snapshot(mc_, hc)
    m1, h1 = fresh(ctx, levels)
    before = H.snapshot(m1, h1)
    got = h1.process_many_clouds(xyz, scan, valid, take=take)
    assert got[idx].tobytes() == want.tobytes()
    assert all(H.not_taken(got[k]) for k in np.flatnonzero(~take))
    after = H.snapshot(m1, h1)
    same(after, snap, "take")
    if not take.any():
        same(after, before, "none taken")
    st = h1.stats()
    assert (st["scans"], st["calls"], st["host_syncs"]) == (len(idx), 1, 1), st
    assert st["map_updates"] == int((want["updated"] != 0).sum())
    # the same flags as device words: stride 1 (with words that are > 1, 0 and negative), and inside lslam_msync_records
    words = np.where(take, np.arange(12) % 3 + 1, -(np.arange(12) % 3)).astype(np.int32)
    records = np.zeros(12, api.MSYNC_RECORD)
    records["status"] = np.where(take, api.MSYNC_CORRECTED, [api.MSYNC_QUEUED, api.MSYNC_WAIT_IMU, api.MSYNC_WAIT_ODOM] * 4)
    records["n_imu"] = np.where(take, -5, 7)  # the word next to the status says the opposite
    records["imu_front"] = 1
    for stride, host in ((1, words), (api.MSYNC_RECORD.itemsize // 4, records)):
        d_take = ctx.alloc(host.nbytes)
        ctx.upload(d_take, host)
        m2, h2 = fresh(ctx, levels)
        dev = h2.process_many_clouds_dev(12, xyz.shape[1], clouds["d_xyz"], clouds["d_valid"], d_take, stride, scan)
        assert dev.tobytes() == got.tobytes(), stride
        same(H.snapshot(m2, h2), after, "stride %d" % stride)
        assert h2.stats() == st
        ctx.free(d_take)
        m2.close()
    print(pattern, "taken", idx.tolist(), "updates", got["updated"].tolist())
    mc_.close()
    m1.close()


def test_none_taken_after_a_run_changes_nothing(ctx, clouds):
    """2, with state to lose: after all 12 clouds, a call that takes none leaves planes, state and containers as they were."""
    scan, xyz, valid = clouds["scan"], clouds["xyz"], clouds["valid"]
    m, h = fresh(ctx, 3)
    h.process_many_clouds(xyz, scan, valid)
    before, st0 = H.snapshot(m, h), h.stats()
    rec = h.process_many_clouds(xyz[:5], scan, valid[:5], take=np.zeros(5, bool), pose_hints=np.full((5, 3), 0.7, f32),
                                map_without_matching=np.ones(5, bool))
    assert all(H.not_taken(r) for r in rec)
    same(H.snapshot(m, h), before)
    st = h.stats()
    assert (st["scans"], st["map_updates"], st["calls"], st["host_syncs"]) == \
        (st0["scans"], st0["map_updates"], st0["calls"] + 1, st0["host_syncs"] + 1)
    assert before["cached_points"] > 300 and len(before["container"]) > 8 * 300
    m.close()


# ---- 3 .. 6: the node in front ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(H.STATUSES))
def test_synced_form_equals_msync_then_clouds(ctx, name):
    """3. process_synced == MotionSync.scans (host form) + process_many_clouds with take = status == 1, on fresh handles."""
    rec, srec, snap, st, mst, _ = whole(ctx, name, synced)
    rec2, srec2, snap2, st2, mst2, _ = whole(ctx, name, two_step)
    status = srec["status"].tolist()
    print(name, "status", status, "points", rec["n_points"].tolist(), "updates", rec["updated"].tolist())
    assert status == H.STATUSES[name]
    assert rec.tobytes() == rec2.tobytes() and srec.tobytes() == srec2.tobytes()
    same(snap, snap2)
    assert [mst[k] for k in ("callbacks", "corrected", "refused")] == [mst2[k] for k in ("callbacks", "corrected", "refused")]
    taken = np.array(status) == 1
    assert mst["corrected"] == int(taken.sum()) and mst["refused"] == int((np.array(status) < 0).sum())
    assert all(H.not_taken(rec[k]) for k in np.flatnonzero(~taken)) and (rec["n_points"][taken] > 40).all()
    assert (st["scans"], st["calls"], st["host_syncs"]) == (int(taken.sum()), 1, 1), st
    assert st2["scans"] == st["scans"] and rec["updated"][1] == 1  # the first taken scan always updates the map
    if name == "imu_gap":  # the refused callback 2, right behind the first taken scan: the planes are those of callback 1 alone
        assert H.not_taken(rec[2])
        upto2, upto3 = run(ctx, name, synced, upto=2), run(ctx, name, synced, upto=3)
        assert upto3[0][:2].tobytes() == upto2[0].tobytes() and H.not_taken(upto3[0][2])
        same(upto3[2], upto2[2], "after the refused callback")
        assert any(np.frombuffer(p, f32).any() for p in upto2[2]["planes"])
    if name == "window_sizes":  # the last callback is refused: the containers are callback 6's
        upto7 = run(ctx, name, synced, upto=7)
        assert upto7[0].tobytes() == rec[:7].tobytes()
        same(upto7[2], snap, "after the refused last callback")
        assert snap["cached_points"] == rec["n_points"][6] > 40 and len(snap["container"]) == 8 * rec["n_points"][6]
    if name == "wide":
        assert (rec["n_points"][taken] > 1024).all()


@pytest.mark.parametrize("chunks", [[1] * 14, H.CHUNKS], ids=["14x1", "1+4+1+3+5"])
def test_chunking_changes_nothing(ctx, chunks):
    """4. non_monotone in one call, in 14 calls of 1 and split inside its runs of refusals: identical; one wait per call; a
    first call that only queues takes nothing and leaves the map untouched."""
    rec, srec, snap, st, mst, _ = whole(ctx, "non_monotone", synced)
    rec2, srec2, snap2, st2, mst2, (first_snap, first_st) = run(ctx, "non_monotone", synced, chunks=chunks)
    assert rec2.tobytes() == rec.tobytes() and srec2.tobytes() == srec.tobytes()
    same(snap2, snap)
    assert st2["calls"] == st2["host_syncs"] == len(chunks) and st["calls"] == st["host_syncs"] == 1
    assert st2["scans"] == st["scans"] == H.STATUSES["non_monotone"].count(1) and st2["map_updates"] == st["map_updates"]
    assert [mst2[k] for k in ("callbacks", "corrected", "refused")] == [mst[k] for k in ("callbacks", "corrected", "refused")]
    # the first call is the queued callback alone
    assert chunks[0] == 1 and H.not_taken(rec2[0]) and first_st["scans"] == 0 and first_st["calls"] == 1
    m, h = fresh(ctx, H.LEVELS["non_monotone"])
    same(first_snap, H.snapshot(m, h), "a call that only queues")
    m.close()


def test_continuation_after_a_synced_call(ctx):
    """5. after a synced call on steady's first 8 callbacks, the rest through process_synced and through MotionSync.scans +
    process_many_clouds give equal bytes: the queued scan and the node's queues were left as the host form leaves them."""
    c = H.case("steady")
    out = []
    for rest in (synced, two_step):
        m, h = fresh(ctx, H.LEVELS["steady"])
        ms = node(ctx, c)
        a, sa = synced(h, ms, c, 0, 8)
        b, sb = rest(h, ms, c, 8, None, None, None)
        out.append((np.concatenate([a, b]).tobytes(), np.concatenate([sa, sb]).tobytes(), H.snapshot(m, h), ms.stats()))
        assert sb["status"].tolist() == [1] * 6 and sb["imu_front"][0] >= sa["imu_front"][-1] > 0
        ms.close()
        m.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    same(out[0][2], out[1][2])
    assert out[0][3]["corrected"] == out[1][3]["corrected"] == 13
    one = whole(ctx, "steady", synced)
    assert out[0][0] == one[0].tobytes() and out[0][1] == one[1].tobytes()
    same(out[0][2], one[2])


def test_with_and_without_matching(ctx):
    """6. imu_gap with explicit hints and map_without_matching on every other callback (updates are certain, the rotation is
    the host's), and in chain mode under a low gate: both routes equal."""
    name = "imu_gap"
    n = len(H.STATUSES[name])
    taken = np.array(H.STATUSES[name]) == 1
    k = np.arange(n, dtype=f32)
    hints = np.stack([0.02 * k, -0.015 * k, 0.01 * k], 1).astype(f32)
    flags = (np.arange(n) % 2 == 1)
    a = run(ctx, name, synced, hints=hints, flags=flags)
    b = run(ctx, name, two_step, hints=hints, flags=flags)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    same(a[2], b[2])
    rec = a[0]
    assert (taken & flags).sum() >= 3 and (taken & ~flags).sum() >= 3
    for i in np.flatnonzero(taken & flags):  # taken without matching: the hint is the pose, and the map is updated
        assert rec["pose"][i].tobytes() == hints[i].tobytes() and rec["updated"][i] == 1
    assert all(H.not_taken(rec[i]) for i in np.flatnonzero(~taken))
    c = run(ctx, name, synced, min_dist=CHAIN_MIN_DIST[name])
    d = run(ctx, name, two_step, min_dist=CHAIN_MIN_DIST[name])
    assert c[0].tobytes() == d[0].tobytes()
    same(c[2], d[2])
    ups = int((c[0]["updated"] != 0).sum())
    print("hints: updates %s; chain at min_dist %g: updates %s" % (rec["updated"].tolist(), CHAIN_MIN_DIST[name], c[0]["updated"].tolist()))
    assert 2 <= ups < int(taken.sum()), c[0]["updated"].tolist()
    assert c[3]["map_updates"] == ups


# ---- 7: the reference's rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steady", "imu_gap"])
def test_against_the_host_driven_loop(po, ctx, name):
    """7. every cloud MotionSync.scans corrected through setCloud -> matchContainer -> the reference's own gate on the host ->
    updateByContainer: the decisions of process_synced, poses within POSE_TOL; no decision within GATE_MARGIN of the gate."""
    c = H.case(name)
    scan = H.hector_scan(c)
    min_dist = CHAIN_MIN_DIST[name]
    rec, srec, *_ = run(ctx, name, synced, min_dist=min_dist)
    ms = node(ctx, c)
    xyz, valid, srec2 = ms.scans(c["laser"], *H.scan_args(c))
    ms.close()
    assert srec2.tobytes() == srec.tobytes()
    m = D.device_map(ctx, H.LEVELS[name])
    est, last = np.zeros(3, f32), np.full(3, S.FLT_MAX, f32)
    worst, closest, decisions = 0.0, np.inf, []
    for k in np.flatnonzero(srec["status"] == api.MSYNC_CORRECTED):
        if m.setCloud(xyz[k], valid[k], scan) > 0:
            est, _ = m.matchContainer(est)
        did = po.href_pose_difference_larger_than(est, last, min_dist, S.MIN_ANGLE)
        # how far the decision is from flipping: the distance from min_dist, and the heading difference from the +-1 rad at
        # which the reference's abs(int) stops truncating it to 0
        if last[0] != S.FLT_MAX:
            closest = min(closest, abs(float(S.pose_distance(est, last)) - min_dist), 1.0 - abs(float(est[2] - last[2])))
        if did:
            m.updateByContainer(est)
            last = est.copy()
        decisions.append(did)
        worst = max(worst, float(np.abs(est - rec["pose"][k]).max()))
        assert bool(rec["updated"][k]) == bool(did), (k, est, rec[k])
    m.close()
    print("%s at min_dist %g: decisions %s, worst |pose difference| %.3g, closest decision to the gate %.3g"
          % (name, min_dist, [int(d) for d in decisions], worst, closest))
    assert closest > S.GATE_MARGIN
    assert worst <= S.POSE_TOL
    assert 2 <= sum(decisions) < len(decisions)


# ---- 8: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_change_neither_handle(ctx):
    """8. each refused call gives its documented status, and the valid calls around them give the bytes of fresh handles."""
    name = "non_monotone"
    c = H.case(name)
    scan = H.hector_scan(c)
    want = whole(ctx, name, synced)
    m, h = fresh(ctx, H.LEVELS[name])
    ms = node(ctx, c)
    a, sa = synced(h, ms, c, 0, 4)
    r, t, ti, iseen, oseen = H.scan_args(c, 4, None)

    def refused(code, fn):
        st, mst, snap = h.stats(), ms.stats(), H.snapshot(m, h)
        with pytest.raises(api.LslamError) as e:
            fn()
        assert e.value.code == code, e.value
        assert h.stats() == st and ms.stats() == mst
        same(H.snapshot(m, h), snap)

    other = api.Context(0)
    ms_other = node(other, c)
    refused(INVALID, lambda: h.process_synced(ms_other, c["laser"], r, scan, t, ti, iseen, oseen))
    ms_other.close()
    other.close()
    refused(INVALID, lambda: h.process_synced(ms, c["laser"], r[:, :63], scan, t, ti, iseen, oseen))  # the first scan had 64
    down = iseen.copy()
    down[3] = down[2] - 1
    refused(INVALID, lambda: h.process_synced(ms, c["laser"], r, scan, t, ti, down, oseen))
    too_many = np.full(len(t), len(c["imu_t"]) + 1, np.int64)
    refused(INVALID, lambda: h.process_synced(ms, c["laser"], r, scan, t, ti, too_many, oseen))
    mo = D.device_map(ctx, 2)
    mo.set_option("ordered_sums", 1)
    ho = D.processor(mo)
    for call in (lambda: ho.process_synced(ms, c["laser"], r, scan, t, ti, iseen, oseen),
                 lambda: ho.process_many_clouds(np.zeros((2, 64, 3), f32), scan)):
        refused(UNSUPPORTED, call)
    mo.close()
    big = np.zeros((1, 65537, 3), f32)
    refused(UNSUPPORTED, lambda: h.process_many_clouds(big, scan))
    d_big = ctx.alloc(big.nbytes)
    refused(UNSUPPORTED, lambda: h.process_many_clouds_dev(1, 65537, d_big, None, None, 1, scan))
    refused(INVALID, lambda: h.process_many_clouds_dev(1, 64, d_big, None, d_big, 0, scan))  # a take word needs a stride
    ctx.free(d_big)
    b, sb = synced(h, ms, c, 4, None)
    assert np.concatenate([a, b]).tobytes() == want[0].tobytes() and np.concatenate([sa, sb]).tobytes() == want[1].tobytes()
    same(H.snapshot(m, h), want[2])
    assert [ms.stats()[k] for k in ("callbacks", "corrected", "refused")] == [want[4][k] for k in ("callbacks", "corrected", "refused")]
    ms.close()
    m.close()
