"""Live occupancy map over the front-end's resident scans (lslam_livemap_*, csrc/livemap.hip): after every update it must
equal OccupancyGrid::CreateFromScans over all processed scans at their current poses bit for bit -- dimensions, offset, both
counter planes, the classified cells -- whichever of its three paths (append / grow / rebuild) the update took."""
import math

import numpy as np
import pytest

from lslam_amd import api, synth

pytestmark = pytest.mark.gpu

RES, THR = 0.05, 20.0
OFFSET = (0.18, -0.05, 0.04)
FE_KW = dict(scan_buffer_size=20, scan_buffer_maximum_scan_distance=5.0, do_loop_closing=1, link_scan_maximum_distance=1.5,
             loop_search_maximum_distance=3.0, loop_match_minimum_chain_size=6, use_scan_barycenter=1)


def _frontend(ctx, offset=(0.0, 0.0, 0.0)):
    lp = api.laser_params(synth.Laser(), THR, offset)
    gm = api.ScanMatcher(ctx, api.baseline_config(range_threshold=THR), lp)
    return lp, gm, api.FrontEnd(gm, config=api.frontend_config(**FE_KW))


def _arena_scans(n, offset=(0.0, 0.0, 0.0)):
    """The arena loop of test_graph_frontend_variants_against_reference_live: ranges [n, 1081], odometry [n, 3]."""
    laser = synth.Laser()
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=5)
    path = synth.loop_trajectory(150, w=6.0, h=4.0, step=0.2, origin=(-3.0, -2.0))[:n]
    odom = synth.drifting_odometry(synth.loop_trajectory(150, w=6.0, h=4.0, step=0.2, origin=(-3.0, -2.0)), scale=1.02, seed=11)[:n]
    ranges = []
    for i, t in enumerate(path):
        c, s = math.cos(t[2]), math.sin(t[2])  # the scan is cast from where the LASER is
        lpose = (t[0] + c * offset[0] - s * offset[1], t[1] + s * offset[0] + c * offset[1], t[2] + offset[2])
        ranges.append(synth.ranges_to_f64(synth.cast_scan(world, lpose, laser, 0.01, 0.01, np.random.default_rng([47, i]))))
    return np.stack(ranges), np.asarray(odom)


@pytest.fixture(scope="module")
def loop_scans():
    return _arena_scans(150)


@pytest.fixture(scope="module")
def offset_scans():
    return _arena_scans(60, OFFSET)


def _check_against_reference(oracle_lib, gm, fe, grid, ranges, offset=(0.0, 0.0, 0.0)):
    """grid == CreateFromScans(the processed scans at fe.scan_pose): the reference's own where oracle/_ref is built, the
    restatement otherwise; the counter planes against the restatement's on the same box, always."""
    laser = synth.Laser()
    robot = np.stack([fe.scan_pose(i) for i in range(fe.num_scans())])
    sensor = np.stack([gm.sensor_pose_from_robot(p) for p in robot])
    assert len(ranges) == len(robot)
    port = oracle_lib.PortKarto(oracle_lib.default_cfg(), oracle_lib.laser_struct(laser, THR, offset))
    if oracle_lib.have_ref():
        ref = oracle_lib.RefKarto(oracle_lib.default_cfg(), oracle_lib.laser_struct(laser, THR, offset))
        exp, off = ref.occgrid_from_scans(ranges, robot, RES)
    else:
        exp, off = port.occgrid_from_scans(ranges, sensor, RES)
    w, h, goff, gres = grid.info()
    assert (h, w) == exp.shape and gres == RES
    assert np.array_equal(goff, off), (goff, off)
    assert np.array_equal(grid.data(), exp)
    ros = np.where(exp == 0, -1, np.where(exp == 100, 100, 0)).astype(np.int8)  # karto_slam.cc:546-569
    assert np.array_equal(grid.ros_data(), ros)
    box = port.occgrid_bounds(ranges, sensor)
    d, cnt = port.occgrid_partial(ranges, sensor, RES, box)
    assert (int(d[0]), int(d[1])) == (w, h) and int(d[2]) == (w + 7) & ~7
    assert np.array_equal(grid.export_counters(), cnt)
    assert (exp == 100).sum() > 50 and (exp == 255).sum() > 1000


def test_every_path_against_the_reference(ctx, oracle_lib, loop_scans):
    """update() after every processed scan of a loop that revisits: appends, grows and rebuilds all happen, a loop closes
    (the closing scan is re-posed inside its own Process call, before the map sees it), and the map is the reference's."""
    ranges, odom = loop_scans
    lp, gm, fe = _frontend(ctx)
    lm = api.LiveMap(fe, RES)
    kept, seen_kinds, checks = [], set(), 0
    prev = lm.stats()
    for i, (r, o) in enumerate(zip(ranges, odom)):
        ok = fe.Process(r, o)[0]
        if not ok:
            continue
        kept.append(r)
        lm.update()
        st = lm.stats()
        kind = [k for k in ("appends", "grows", "rebuilds") if st[k] == prev[k] + 1]
        assert len(kind) == 1 and st["updates"] == prev["updates"] + 1 and st["scans"] == len(kept), (i, prev, st)
        rise = st["scans_traced"] - prev["scans_traced"]
        if kind[0] == "appends":  # nothing was retraced
            assert rise == 1, (i, prev, st)
        elif kind[0] == "grows":  # the new scan, and the old ones whose rays the old bounds clipped (margin cells only)
            assert 1 <= rise <= len(kept), (i, prev, st)
        else:
            assert rise == len(kept), (i, prev, st)
        prev = st
        if len(kept) % 10 == 0 or i == len(ranges) - 1 or kind[0] not in seen_kinds:
            _check_against_reference(oracle_lib, gm, fe, lm.grid(), np.stack(kept))
            checks += 1
        seen_kinds.add(kind[0])
    st = lm.stats()
    print("live map paths over", len(kept), "scans:", st, "checks", checks, "front-end", fe.stats())
    assert st["appends"] >= 1 and st["grows"] >= 1 and st["rebuilds"] >= 1, st
    assert fe.stats()["loops_closed"] > 0
    lm.update()  # nothing new: no path taken, nothing traced
    assert lm.stats()["scans_traced"] == st["scans_traced"] and lm.stats()["updates"] == st["updates"] + 1
    lm.close()
    fe.close()
    gm.close()


def _feed_in_chunks(ctx, oracle_lib, ranges, odom, check):
    lp, gm, fe = _frontend(ctx, OFFSET)
    lm = api.LiveMap(fe, RES)
    kept = []
    for a in range(0, len(ranges), 20):
        ok = fe.ProcessMany(ranges[a:a + 20], odom[a:a + 20])[0]
        kept.extend(ranges[a:a + 20][ok])
        before = lm.stats()["scans_traced"]
        lm.update()
        st = lm.stats()
        assert st["scans"] == len(kept) == fe.num_scans()
        assert int(ok.sum()) <= st["scans_traced"] - before <= len(kept)  # the new scans ... (a rebuild) all of them
        if check:
            _check_against_reference(oracle_lib, gm, fe, lm.grid(), np.stack(kept), OFFSET)
    return lp, gm, fe, lm, np.stack(kept)


def test_chunks_laser_offset_and_lookahead(ctx, oracle_lib, offset_scans):
    """Several scans per update, fed through ProcessMany (the path on which a look-ahead match may be in flight when the
    map is asked for), the laser mounted off the base centre: the map reads the sensor poses the reference's scans report."""
    ranges, odom = offset_scans
    lp, gm, fe, lm, kept = _feed_in_chunks(ctx, oracle_lib, ranges, odom, check=True)
    assert lm.stats()["updates"] == 3
    lm.close()
    fe.close()
    gm.close()


def test_equal_to_the_one_shot_device_build(ctx, oracle_lib, offset_scans):
    ranges, odom = offset_scans
    lp, gm, fe, lm, kept = _feed_in_chunks(ctx, oracle_lib, ranges, odom, check=False)
    sensor = np.stack([gm.sensor_pose_from_robot(fe.scan_pose(i)) for i in range(fe.num_scans())])
    whole = api.OccupancyGrid.CreateFromScans(ctx, lp, kept, sensor, RES)
    live = fe.OccupancyGrid(RES)  # the convenience form: its own live map, built in one rebuild
    for g in (lm.grid(), live):
        wi, gi = whole.info(), g.info()
        assert wi[:2] == gi[:2] and np.array_equal(wi[2], gi[2]) and wi[3] == gi[3]
        assert g.counter_words() == whole.counter_words()
        assert np.array_equal(g.export_counters(), whole.export_counters())
        assert np.array_equal(g.data(), whole.data())
    whole.close()
    lm.close()
    fe.close()
    gm.close()


def test_reset_and_errors(ctx, oracle_lib, loop_scans):
    ranges, odom = loop_scans
    lp, gm, fe = _frontend(ctx)
    with pytest.raises(api.LslamError) as e:
        api.LiveMap(fe, 0.0)
    assert e.value.code == -1
    lm = api.LiveMap(fe, RES)
    assert lm.grid() is None
    with pytest.raises(api.LslamError) as e:  # no processed scan: the reference returns NULL
        lm.update()
    assert e.value.code == -1
    ok = fe.ProcessMany(ranges[:12], odom[:12])[0]
    lm.update()  # the handle is still usable
    assert lm.stats()["scans"] == int(ok.sum()) >= 6
    rebuilds = lm.stats()["rebuilds"]
    fe.reset()
    ok = fe.ProcessMany(ranges[40:45], odom[40:45])[0]
    lm.update()
    st = lm.stats()
    assert st["scans"] == int(ok.sum()) >= 3 and st["rebuilds"] == rebuilds + 1
    _check_against_reference(oracle_lib, gm, fe, lm.grid(), ranges[40:45][ok])
    fe.reset()
    with pytest.raises(api.LslamError) as e:  # reset, nothing processed since
        lm.update()
    assert e.value.code == -1
    lm.close()
    fe.close()
    gm.close()
