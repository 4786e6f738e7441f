"""The lesson5 de-skew on the device (csrc/deskew.hip: k_deskew, k_deskew_batch, k_deskew_angles, the lslam_deskew handle)
and its consumer k_hector_cloud_container (csrc/logodds_map.hip) on the directed scenarios of tests/deskew_edge_cases.py,
whose claims tests/test_deskew_edges_oracle.py holds without a GPU.  The tolerances are the project's: bit for bit between
the forms of this library, 2e-6 m against the numpy restatement (tests/deskew_restatement.py), bit for bit against the
restatement of rosPointCloudToDataContainer (deskew_stream_cases.cloud_container).

  IMU samples read from HBM (more than 256), mixed with staged ones in one launch   test_staging_*
  the first valid beam at tile edges and beyond tile 1, the range window's ends,
  a ROS time base, mixed use_imu / use_odom in one batch                            test_scenario_*, test_mixed_flags_*
  the cached angle table: shorter scan, other increment, growth, back again         test_angle_table_on_one_handle
  the pinned ring of four slots wrapping twice, growth in mid-ring                  test_pinned_ring_wraps_and_grows_in_flight
  imu_first[0] > 0                                                                  test_imu_first_need_not_start_at_zero
  the container's filter boundaries, non-finite points, compaction rounds           test_cloud_container_*
  a scan of 330 samples through the streamed processor                              test_hbm_scan_through_the_stream

Every test prints what it measured (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from lslam_amd import api

import deskew_edge_cases as E
import deskew_stream_cases as D

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL = 2e-6


@pytest.fixture(scope="module")
def deskewer(ctx):
    d = api.Deskewer(ctx)
    yield d
    d.close()


@pytest.fixture(scope="module")
def runs(ctx, deskewer):
    """Every scenario once: each of its calls through Deskewer.batch, each scan alone through deskew_scan.
    -> {name: [(xyz, valid, xyz_single, valid_single)] per scan}"""
    out = {}
    for name in E.BUILDERS:
        scn = E.scenario(name)
        ranges, ps, times, rots, facts = scn
        per = [None] * len(ps)
        for idx in facts["calls"]:
            xyz, valid = deskewer.batch(*E.call_inputs(scn, idx))
            for j, i in enumerate(idx):
                one, v1 = D.single(ctx, ranges[i], ps[i], times[i], rots[i])
                per[i] = (xyz[j], valid[j], one, v1)
        out[name] = per
    return out


def check_scenario(name, runs):
    """Each scan: batch == single bit for bit, valid == the restatement's, <= 2e-6 m from it, exactly zero where invalid."""
    facts = E.scenario(name)[4]
    worst = []
    for k, ((xyz, valid, one, v1), (w, wv)) in enumerate(zip(runs[name], E.restated(name))):
        assert np.array_equal(valid, v1) and xyz.tobytes() == one.tobytes(), (name, k, np.abs(xyz - one).max())
        assert np.array_equal(valid, wv), (name, k, np.flatnonzero(valid != wv))
        assert np.all(xyz[~wv] == 0) and not np.signbit(xyz[~wv]).any()
        worst.append(float(np.abs(xyz - w).max()))
    print("%s: worst |device - restatement| per scan = %s m" % (name, dict(zip(facts["names"], ["%.3g" % w for w in worst]))))
    assert max(worst) <= TOL, worst
    return worst


def test_staging_lds_and_hbm_in_one_launch(runs):
    """1. 256, 257, 330, 12 and 300 samples in one batch: blocks that stage their samples in LDS next to blocks that read them
    from HBM.  lds256 and hbm257 are the same scan but for one sample no beam reaches: the two forms agree bit for bit."""
    check_scenario("imu_staging", runs)
    per = runs["imu_staging"]
    assert per[0][1].sum() > 500
    assert per[0][0].tobytes() == per[1][0].tobytes() and np.array_equal(per[0][1], per[1][1])
    assert per[0][2].tobytes() == per[1][2].tobytes()  # and so do the single form's


def test_staging_permuting_the_scans_permutes_the_outputs(deskewer, runs):
    scn = E.scenario("imu_staging")
    perm = [2, 0, 4, 1, 3]
    xyz, valid = deskewer.batch(*E.call_inputs(scn, perm))
    for j, i in enumerate(perm):
        assert xyz[j].tobytes() == runs["imu_staging"][i][0].tobytes() and np.array_equal(valid[j], runs["imu_staging"][i][1])


@pytest.mark.parametrize("name", ["anchors", "window", "epoch", "mixed_flags"])
def test_scenario_equals_single_and_restatement(runs, name):
    """2. each scenario as one batch per geometry."""
    check_scenario(name, runs)
    per, facts = runs[name], E.scenario(name)[4]
    if name == "anchors":
        firsts = [int(np.flatnonzero(v)[0]) if v.any() else None for _, v, _, _ in per]
        assert firsts == facts["first_valid"]
        assert not per[6][0].any()
        # the anchor's own point: transStartInverse * its own transform, the identity up to rounding
        ranges, ps = E.scenario(name)[:2]
        for k in (5, 7):
            i = firsts[k]
            a = float(f32(f32(ps[k].angle_min) + f32(i) * f32(ps[k].angle_increment)))
            r = float(ranges[k][i])
            assert np.abs(per[k][0][i] - [r * np.cos(a), r * np.sin(a), 1.0]).max() < 1e-5
    if name == "window":
        for k in range(3):
            assert np.array_equal(per[k][1], facts["valid"][k])
    if name == "epoch":
        assert per[1][1][facts["exact_beam"]]


def test_mixed_flags_plain_projection_inside_a_mixed_batch(runs):
    """2. the (0,0) scan between scans that use the IMU: ((float)(r cos a), (float)(r sin a), 1.0f) exactly -- the five
    samples it owns are ignored."""
    ranges, ps, times, rots, facts = E.scenario("mixed_flags")
    k = facts["flags"].index((0, 0))
    assert facts["counts"][k] == 5 and facts["counts"][facts["flags"].index((0, 1))] == 0
    xyz, valid = runs["mixed_flags"][k][:2]
    a = (f32(ps[k].angle_min) + np.arange(E.N, dtype=f32) * f32(ps[k].angle_increment)).astype(np.float64)
    r = ranges[k].astype(np.float64)
    with np.errstate(invalid="ignore"):
        want = np.stack([(r * np.cos(a)).astype(f32), (r * np.sin(a)).astype(f32), np.ones(E.N, f32)], axis=1)
    want[~valid] = 0
    assert valid.sum() > 500 and np.array_equal(xyz, want), np.abs(xyz - want).max()


def _geometry_call(inc_n, n_beams, k):
    """Two scans of n_beams beams on the angles of E.laser(inc_n)."""
    times = E.khz(E.T0 - 0.003, 12, 0.01)
    ranges = np.stack([E.room_ranges(k + j, max(n_beams, inc_n))[:n_beams] for j in range(2)])
    ps = [E.params(E.T0, 0.1 / inc_n, inc_n, odom=(0.05 + 0.01 * j, 0.012, 0.004)) for j in range(2)]
    return ranges, ps, [times] * 2, [E.integrate(times)] * 2


def test_angle_table_on_one_handle(ctx):
    """3. the cached table serves a shorter scan of the same angles, is rebuilt for another increment, grows, and is rebuilt
    when the first geometry comes back: launches counted, every result bit-equal to the single form."""
    d = api.Deskewer(ctx)
    steps = [(600, 600, 2, "600 beams, geometry A"), (600, 300, 1, "300 beams, geometry A: the table of 600 serves"),
             (700, 300, 2, "300 beams, another angle_increment"), (700, 700, 2, "700 beams of that geometry: the table grows"),
             (600, 600, 2, "600 beams, geometry A again")]
    seen = []
    for s, (inc_n, n_beams, launches, what) in enumerate(steps):
        ranges, ps, times, rots = _geometry_call(inc_n, n_beams, s)
        before = d.stats()
        xyz, valid = d.batch(ranges, ps, times, rots)
        after = d.stats()
        seen.append(after["launches"] - before["launches"])
        assert seen[-1] == launches, (what, seen)
        if s == 3:
            assert after["growths"] > before["growths"]
        assert xyz.shape == (2, n_beams, 3) and valid.sum() > 2 * n_beams * 0.9
        for j in range(2):
            one, v1 = D.single(ctx, ranges[j], ps[j], times[j], rots[j])
            assert np.array_equal(valid[j], v1) and xyz[j].tobytes() == one.tobytes(), (what, j, np.abs(xyz[j] - one).max())
    print("launches per call:", seen)
    d.close()


def _ring_call(c):
    """Call c of nine: its own ranges, params and samples.  Call 5 (the sixth) is the imu_staging batch: 1155 samples, where
    the calls before it carry at most 36."""
    if c == 5:
        return E.call_inputs(E.scenario("imu_staging"), list(range(5)))
    n = 3 - c % 3  # (the first call is the largest of the small ones: no slot grows before the sixth)
    t0 = E.T0 + 0.5 * c
    times = E.khz(t0 - 0.003, 12 - c % 2, 0.01)
    ranges = np.stack([np.roll(E.room_ranges((c + j) % 7), 10 * c + j) for j in range(n)])
    ps = [E.params(t0, 0.1 / E.N, odom=(0.05 + 0.01 * j, 0.012 - 0.002 * c, 0.004)) for j in range(n)]
    return ranges, ps, [times] * n, [E.integrate(times, (0.001 * c, 0.0, -0.002 * c))] * n


def test_pinned_ring_wraps_and_grows_in_flight(ctx):
    """4. nine _dev calls with no synchronisation between them: the ring of four pinned slots wraps twice, and the sixth
    call's records do not fit the slots the first five sized -- every slot grows while others are in flight (a long launch
    of a second handle is put on the stream first, so that they are).  After one synchronisation every output is the host
    form's for the same inputs."""
    host = api.Deskewer(ctx)
    calls = [_ring_call(c) for c in range(9)]
    want = [host.batch(*c) for c in calls]
    host.close()
    d, busy = api.Deskewer(ctx), api.Deskewer(ctx)
    bufs = []
    try:
        for ranges, ps, _, _ in calls:
            n = len(ps)
            d_r, d_xyz, d_v = ctx.alloc(n * E.N * 4), ctx.alloc(n * E.N * 12), ctx.alloc(n * E.N)
            bufs.append((d_r, d_xyz, d_v))
            ctx.upload(d_r, np.ascontiguousarray(ranges))
        # keep the stream busy for some milliseconds, so that the nine calls find their slots' copies still in flight: one
        # scan of 2^20 beams without a valid one -- each of its 4096 blocks walks the whole scan looking for the anchor
        big = 1 << 20
        b_r, b_xyz, b_v = ctx.alloc(big * 4), ctx.alloc(big * 12), ctx.alloc(big)
        bufs.append((b_r, b_xyz, b_v))
        ctx.upload(b_r, np.full(big, np.inf, f32))
        ctx.synchronize()
        waits, growths = [d.stats()["host_waits"]], [d.stats()["growths"]]
        for c, ((ranges, ps, times, rots), (d_r, d_xyz, d_v)) in enumerate(zip(calls, bufs)):
            if c < 2:  # before the first call, and again behind it: the fifth call waits for the first one's slot only
                busy.batch_dev(big, b_r, big, [E.params(E.T0, 1e-7, use_imu=0)], None, None, b_xyz, b_v)
            d.batch_dev(E.N, d_r, E.N, ps, times, rots, d_xyz, d_v)
            waits.append(d.stats()["host_waits"])
            growths.append(d.stats()["growths"])
        ctx.synchronize()
        got_v = np.ones(big, np.uint8)
        ctx.download(b_v, got_v)
        assert not got_v.any()
        print("host waits after each call:", waits, "growths:", growths)
        assert all(b >= a for a, b in zip(waits, waits[1:]))
        assert growths[6] > growths[5] and growths[9] == growths[6]  # the sixth call grew the slots, none after it
        for c, ((ranges, ps, _, _), (d_r, d_xyz, d_v)) in enumerate(zip(calls, bufs)):
            n = len(ps)
            got, got_v = np.zeros((n, E.N, 3), f32), np.zeros((n, E.N), np.uint8)
            ctx.download(d_xyz, got)
            ctx.download(d_v, got_v)
            assert np.array_equal(got_v.astype(bool), want[c][1]), c
            assert got.tobytes() == want[c][0].tobytes(), (c, np.abs(got - want[c][0]).max())
    finally:
        ctx.synchronize()
        for b in bufs:
            for p in b:
                ctx.free(p)
        d.close()
        busy.close()


def test_imu_first_need_not_start_at_zero(ctx, deskewer, runs):
    """5. lslam_deskew_batch with seven leading NaN samples in each IMU array and imu_first starting at 7: the same bits as
    the wrapper's call (which always starts at 0) -- on the mixed batch, whose sample counts include 0."""
    scn = E.scenario("mixed_flags")
    ranges, ps, times, rots = E.call_inputs(scn, list(range(6)))
    arr, first, it, ir = api._deskew_inputs(ps, times, rots)
    lead = np.full(7, np.nan)
    first7 = (first + 7).astype(np.int32)
    it7 = np.ascontiguousarray(np.concatenate([lead, it]))
    ir7 = [np.ascontiguousarray(np.concatenate([lead, ir[a]])) for a in range(3)]
    r = np.ascontiguousarray(ranges, dtype=f32)
    xyz, valid = np.zeros((6, E.N, 3), f32), np.zeros((6, E.N), np.uint8)
    ctx.check(ctx.L.lslam_deskew_batch(deskewer.h, 6, E.N, r.ctypes.data, E.N, C.addressof(arr), first7.ctypes.data,
                                       it7.ctypes.data, ir7[0].ctypes.data, ir7[1].ctypes.data, ir7[2].ctypes.data,
                                       xyz.ctypes.data, valid.ctypes.data))
    assert first7[0] == 7 and first7[-1] == 57
    for k in range(6):
        assert np.array_equal(valid[k].astype(bool), runs["mixed_flags"][k][1]), k
        assert xyz[k].tobytes() == runs["mixed_flags"][k][0].tobytes(), (k, np.abs(xyz[k] - runs["mixed_flags"][k][0]).max())


def _set_and_compare(m, xyz, valid, scan, scale, what):
    n = m.setCloud(xyz, valid, scan)
    got, origo = m.container()
    with np.errstate(invalid="ignore"):
        want, want_origo = D.cloud_container(xyz, valid, scan, scale)
    assert n == len(want) == len(got), (what, n, len(want), len(got))
    assert got.tobytes() == want.tobytes(), what
    assert origo.tobytes() == want_origo.tobytes(), what
    return n


@pytest.mark.parametrize("pose", list(E.LASER_POSES))
def test_cloud_container_filter_boundaries(ctx, pose):
    """6. a point on, one ulp below and one ulp above every filter boundary, non-finite coordinates with valid = 1, a passing
    point with valid = 0: count, order, points and origo bit-equal to the restatement."""
    m = D.device_map(ctx, 2)
    scale = m.getScaleToMap()
    for cfg in E.CLOUD_CFGS:
        xyz, valid, names, fails = E.named_cloud(cfg)
        scan = E.cloud_scan(cfg, pose)
        n = _set_and_compare(m, xyz, valid, scan, scale, (cfg, pose))
        print("%s, %s laser: %d of %d named points kept" % (cfg, pose, n, len(names)))
        if pose == "identity":
            assert n == sum(f is None for f in fails)
            kept = xyz[[f is None for f in fails]]
            assert np.array_equal(m.container()[0], kept[:, :2] * f32(scale))
    m.close()


@pytest.mark.parametrize("pose", list(E.LASER_POSES))
def test_cloud_container_compaction_rounds_and_stale_points(ctx, pose):
    """6. clouds of 1 .. 3000 points (rounds of 1024) with kept points everywhere, nowhere, only at the very end, only at the
    start of the second round, alternating and at random; one after another on one map, shorter after longer and sparse
    after full: the count and the container read back after each are that cloud's alone."""
    m = D.device_map(ctx, 2)
    scale = m.getScaleToMap()
    scan = E.cloud_scan("issue", pose)
    counts = {}
    for name, xyz, valid, keep in E.compaction_clouds():
        counts[name] = _set_and_compare(m, xyz, valid, scan, scale, (name, pose))
        assert counts[name] == int(keep.sum()), name
    print("%s laser, points kept per cloud: %s" % (pose, counts))
    assert counts["3000_all"] == 3000 and counts["3000_none"] == 0 and counts["2049_first_of_round_2"] == 1
    m.close()


def test_hbm_scan_through_the_stream(ctx, runs):
    """7. process_deskewed over three scans whose middle one owns 330 samples == process_many_points fed the containers that
    deskew_scan + setCloud make of the same scans: records, planes and state bit-identical."""
    scn = E.scenario("imu_staging")
    idx = [0, 2, 3]  # lds256, hbm330, short12
    ranges, ps, times, rots = E.call_inputs(scn, idx)
    assert [len(t) for t in times] == [256, 330, 12]
    scan = D.hector_scan(E.laser())
    m0 = D.device_map(ctx, 2)
    conts = []
    for i in idx:
        xyz, valid = runs["imu_staging"][i][2:]
        n = m0.setCloud(xyz, valid, scan)
        conts.append(m0.container()[0])
        assert n == len(conts[-1]) > 300
    m0.close()
    m1, m2 = D.device_map(ctx, 2), D.device_map(ctx, 2)
    h1, h2 = D.processor(m1), D.processor(m2)
    rec = h1.process_deskewed(ranges, scan, ps, times, rots)
    rec2 = h2.process_many_points(conts)
    print("points per scan %s, updates %s" % (rec["n_points"].tolist(), rec["updated"].tolist()))
    assert rec["n_points"].tolist() == [len(c) for c in conts]
    assert rec.tobytes() == rec2.tobytes() and rec["updated"][0] != 0
    for lv in range(2):
        a, b = m1.logodds(lv), m2.logodds(lv)
        assert a.tobytes() == b.tobytes() and np.count_nonzero(a) > 100
    for a, b in zip(h1.state(), h2.state()):
        assert a.tobytes() == b.tobytes()
    assert m1.container()[0].tobytes() == conts[-1].tobytes()
    m1.close()
    m2.close()
