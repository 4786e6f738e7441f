"""lesson3's keyframe odometry on clouds, gated (csrc/plicp.hip's k_plicp_odom_clouds, api.PlicpOdometry.process_many_clouds[_dev])
against the SE(2) restatement over sm_icp on cloud_to_ldp (tests/plicp_cloud_odometry_restatement.py): flags and `valid` one for
one, poses within the project's contract of 1e-4 m / 1e-4 rad (measured 3.4e-15 on the logs, 6.6e-15 under a take pattern; printed), the truth within twice the error the
restatement itself makes on these float32 clouds on the CPU (tests/test_plicp_cloud_odom_oracle.py: 1.5e-7, so 3e-7); forms,
call splits, tracks and take gates byte for byte; and lesson5's MotionSync chained in front, on the device against on the host."""
import math

import numpy as np
import pytest

import hector_sync_cases as H
import plicp_cases as K
import plicp_cloud_odometry_restatement as CO
import plicp_odometry_restatement as O
from lslam_amd import api
from plicp_cloud_odometry_restatement import PATTERNS, WORST_TRUTH_ERROR, truth_error

pytestmark = pytest.mark.gpu
WHICH = ("keyframe", "offset", "invalid")


def _odo(ctx, lg, n_tracks=1):
    return api.PlicpOdometry(ctx, n_tracks, base_to_laser=lg.base_to_laser)   # no laser: a cloud needs none


@pytest.fixture(scope="module")
def device(ctx):
    """Every log in one call at R = 1: which -> (records [n], state [1], stats)."""
    out = {}
    for which in WHICH:
        lg = CO.log(which)
        o = _odo(ctx, lg)
        try:
            rec = o.process_many_clouds(lg.xyz, lg.stamps, lg.valid)[:, 0]
            out[which] = (rec, o.state(), o.stats())
        finally:
            o.close()
    return out


def _same_as_restatement(rec, steps):
    worst = 0.0
    for k, s in enumerate(steps):
        if s is None:
            continue
        assert (int(rec[k]["flags"]), int(rec[k]["valid"])) == (s.flags, s.valid), k
        assert (int(rec[k]["iterations"]), int(rec[k]["nvalid"])) == (s.iterations, s.nvalid), k
        d = np.abs(rec[k]["base_in_odom"] - np.array(s.base_in_odom))
        d[2] = abs(math.remainder(rec[k]["base_in_odom"][2] - s.base_in_odom[2], 2 * math.pi))
        worst = max(worst, d.max())
    return worst


def _not_taken(rec):
    z = rec.copy()
    assert np.all(z["iterations"] == -1)
    z["iterations"] = 0
    return z.tobytes() == bytes(z.nbytes)                                   # zero except iterations = -1


@pytest.mark.parametrize("which", WHICH)
def test_flags_valid_and_poses_are_the_restatements(device, which):
    worst = _same_as_restatement(device[which][0], CO.run(which)[1])
    print(which, "max |pose - restatement|", worst)
    assert worst <= 1e-4


@pytest.mark.parametrize("which", ["keyframe", "offset"])
def test_the_truth_is_tracked(device, which):
    lg = CO.log(which)
    worst = truth_error(lg, [tuple(r["base_in_odom"]) for r in device[which][0]])
    print(which, "worst pose error against the truth", worst, "allowed", 2 * WORST_TRUTH_ERROR)
    assert worst <= 2 * WORST_TRUTH_ERROR


def test_an_invalid_match_leaves_the_pose(device):
    rec = device["invalid"][0]
    assert rec[6]["valid"] == 0 and rec[6]["base_in_odom"].tobytes() == rec[5]["base_in_odom"].tobytes()


def test_one_launch_and_one_host_wait_per_call(device):
    for which, (rec, state, stats) in device.items():
        # process_many_clouds waits once; state() is a second, separate wait
        assert stats["launches"] == 1 and stats["host_waits"] == 2 and stats["scans"] == len(rec), (which, stats)
        assert state["initialized"][0] == 1


def _upload(ctx, arrays):
    ptrs = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        p = ctx.alloc(max(a.nbytes, 4))
        ctx.upload(p, a)
        ptrs.append(p)
    return ptrs


def test_host_form_equals_dev_form(ctx, device):
    lg = CO.log("keyframe")
    whole, state, _ = device["keyframe"]
    ptrs = _upload(ctx, (lg.xyz, lg.valid))
    o = _odo(ctx, lg)
    try:
        dev = o.process_many_clouds_dev(len(lg.xyz), 360, [ptrs[0]], [ptrs[1]], None, 1, lg.stamps)[:, 0]
        st = o.stats()
        assert dev.tobytes() == whole.tobytes() and o.state().tobytes() == state.tobytes()
        assert st["launches"] == 1 and st["host_waits"] == 1 and st["scans"] == 40
        o.reset()
        assert o.process_many_clouds_dev(len(lg.xyz), 360, [ptrs[0]], None, [None], 22, lg.stamps)[:, 0].tobytes() == \
            o2_bytes(ctx, lg)                                                 # NULL valid = every point (host form with valid=None)
    finally:
        o.close()
        for p in ptrs:
            ctx.free(p)


def o2_bytes(ctx, lg):
    o = _odo(ctx, lg)
    try:
        return o.process_many_clouds(lg.xyz, lg.stamps)[:, 0].tobytes()
    finally:
        o.close()


@pytest.mark.parametrize("split", [1, 7])
def test_calls_of_any_length_give_the_same_records_and_state(ctx, device, split):
    lg = CO.log("keyframe")
    whole, state, _ = device["keyframe"]
    o = _odo(ctx, lg)
    try:
        parts = [o.process_many_clouds(lg.xyz[a:a + split], lg.stamps[a:a + split], lg.valid[a:a + split])[:, 0]
                 for a in range(0, len(lg.xyz), split)]
        assert np.concatenate(parts).tobytes() == whole.tobytes()
        assert o.state().tobytes() == state.tobytes()
        o.reset()                                                         # and again after a reset
        assert o.process_many_clouds(lg.xyz, lg.stamps, lg.valid)[:, 0].tobytes() == whole.tobytes()
    finally:
        o.close()


def test_three_ragged_tracks_are_each_the_track_alone(ctx, device):
    logs = [CO.log(w) for w in WHICH]
    alone = [device[w][0] for w in WHICH]
    # no base_to_laser per track: the tracks share the handle's, so the offset log runs here under the zero transform
    o1 = api.PlicpOdometry(ctx, 1)
    try:
        alone[1] = o1.process_many_clouds(logs[1].xyz, logs[1].stamps, logs[1].valid)[:, 0]
    finally:
        o1.close()
    n_steps = 64
    xyz = np.full((n_steps, 3, 360, 3), np.nan, np.float32)               # what is not taken is not read
    valid = np.ones((n_steps, 3, 360), np.uint8)
    stamps = np.full((n_steps, 3), np.nan)
    active = np.zeros((n_steps, 3), np.uint8)
    where = [[], [], []]
    for t in range(3):
        k = 0
        for step in range(n_steps):
            if (step + t) % 3 != 0 and k < len(logs[t].xyz):
                xyz[step, t], valid[step, t], stamps[step, t], active[step, t] = logs[t].xyz[k], logs[t].valid[k], logs[t].stamps[k], 1
                where[t].append(step)
                k += 1
        assert k == len(logs[t].xyz)
    o = api.PlicpOdometry(ctx, 3)
    try:
        rec = o.process_many_clouds(xyz, stamps, valid, active=active)
        st = o.stats()
    finally:
        o.close()
    assert st["launches"] == 1 and st["host_waits"] == 1 and st["scans"] == int(active.sum())
    for t in range(3):
        assert rec[where[t], t].tobytes() == alone[t].tobytes(), t
        assert _not_taken(rec[active[:, t] == 0, t])


@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_take_pattern_is_one_call_over_the_taken_clouds(ctx, pattern):
    lg, take, steps = CO.run_taken("keyframe", pattern)
    kept = np.flatnonzero(take)
    o = _odo(ctx, lg)
    ptrs = _upload(ctx, (lg.xyz, lg.valid))
    words = np.where(take != 0, 1, np.where(np.arange(40) % 2 == 0, 0, -3)).astype(np.int32)   # refused: 0 and negative words
    records = np.zeros(40, api.MSYNC_RECORD)
    records["status"] = words
    assert api.MSYNC_RECORD.itemsize // 4 == 22 and api.MSYNC_RECORD.fields["status"][1] == 0
    ptrs += _upload(ctx, (words, records))
    try:
        only = o.process_many_clouds(lg.xyz[kept], lg.stamps[kept], lg.valid[kept])[:, 0]
        want_state = o.state()
        worst = _same_as_restatement(only, [steps[k] for k in kept])
        print(pattern, "max |pose - restatement|", worst)
        assert worst <= 1e-4
        stamps = np.where(take != 0, lg.stamps, np.nan)                    # the stamp of a refused callback is not read
        poison = lg.xyz.copy()
        poison[take == 0] = np.nan                                          # nor its cloud
        runs = {
            "active": lambda: o.process_many_clouds(poison, stamps, lg.valid, active=take),
            "take bytes": lambda: o.process_many_clouds(poison, stamps, lg.valid, take=take),
            "active and take": lambda: o.process_many_clouds(poison, stamps, lg.valid, take=take | (np.arange(40) % 3 == 0),
                                                             active=take | (np.arange(40) % 3 != 0)),
            "words, stride 1": lambda: o.process_many_clouds_dev(40, 360, [ptrs[0]], [ptrs[1]], [ptrs[2]], 1, stamps),
            "words, stride 22": lambda: o.process_many_clouds_dev(40, 360, [ptrs[0]], [ptrs[1]], [ptrs[3]], 22, stamps),
        }
        for how, go in runs.items():
            o.reset()
            before = o.stats()
            rec = go()[:, 0]
            after = o.stats()
            assert rec[kept].tobytes() == only.tobytes(), how
            assert _not_taken(rec[take == 0]), how
            assert o.state().tobytes() == want_state.tobytes(), how
            assert after["launches"] == before["launches"] + 1 and after["host_waits"] == before["host_waits"] + 1, how
            assert after["scans"] == before["scans"] + len(kept), how
    finally:
        o.close()
        for p in ptrs:
            ctx.free(p)


def test_refusals_change_nothing(ctx, device):
    lg = CO.log("invalid")
    ranges = O.invalid_log().ranges
    o = _odo(ctx, lg)
    try:
        first = o.process_many_clouds(lg.xyz[:4], lg.stamps[:4], lg.valid[:4])
        state, stats = o.state(), o.stats()
        o.set_laser(K.LASER360.angle_min, K.LASER360.angle_increment, 0.1, 30.0)
        for code, go in ((-1, lambda: o.process_many(ranges[4:6], lg.stamps[4:6])),                         # a range call after a cloud call
                         (-1, lambda: o.process_many_clouds(lg.xyz[4:6, :300], lg.stamps[4:6], lg.valid[4:6, :300])),   # another n_points
                         (-8, lambda: o.process_many_clouds(np.ones((1, 1, 2049, 3), np.float32), [0.0]))):  # 2049 points
            with pytest.raises(api.LslamError) as e:
                go()
            assert e.value.code == code
            assert o.state().tobytes() == state.tobytes()
            now = o.stats()
            assert (now["launches"], now["scans"], now["growths"]) == (stats["launches"], stats["scans"], stats["growths"])
        rest = o.process_many_clouds(lg.xyz[4:], lg.stamps[4:], lg.valid[4:])                                # and the track goes on
        assert np.concatenate([first, rest])[:, 0].tobytes() == device["invalid"][0].tobytes()
        o.reset()                                                                                            # reset frees the choice
        o.process_many(ranges[:3], lg.stamps[:3])
        with pytest.raises(api.LslamError) as e:
            o.process_many_clouds(lg.xyz[3:5], lg.stamps[3:5], lg.valid[3:5])                                # a cloud call after a range call
        assert e.value.code == -1
        before = o.stats()
        assert o.process_many_clouds(np.zeros((0, 1, 360, 3), np.float32), np.zeros((0, 1))).shape == (0, 1) and o.stats() == before
    finally:
        o.close()


# ---- lesson5 in front: MotionSync.scans[_dev] -> process_many_clouds[_dev] ---------------------------------------------------

@pytest.mark.parametrize("R", [1, 2])
def test_the_chain_on_the_device_is_the_chain_on_the_host(ctx, R):
    """imu_gap: isolated refusals, the first right behind the first taken scan.  Device route: R MotionSync nodes write xyz, valid
    and records in HBM, the odometry reads them there with &records[0].status as the take words; nothing comes down in between.
    Host route: MotionSync.scans, then process_many_clouds with take = status > 0.  At R = 2 track 1 also skips step 3."""
    c = H.case("imu_gap")
    n_msgs, n = c["ranges"].shape
    assert H.STATUSES["imu_gap"] == [0, 1, -1, 1, -1, 1, 1, -1, 1, 1, 1, 1]
    active = np.ones((n_msgs, R), np.uint8)
    if R == 2:
        active[3, 1] = 0
    # the host route
    host_xyz, host_valid, host_take = [], [], []
    for m in range(R):
        ms = api.MotionSync(ctx)
        try:
            H.push_all(ms, c)
            xyz, valid, rec = ms.scans(c["laser"], *H.scan_args(c))
        finally:
            ms.close()
        assert rec["status"].tolist() == H.STATUSES["imu_gap"]
        host_xyz.append(xyz), host_valid.append(valid), host_take.append(rec["status"] > 0)
    stamps = np.repeat(np.asarray(c["scan_t"], np.float64)[:, None], R, axis=1)
    o = api.PlicpOdometry(ctx, R)
    try:
        want = o.process_many_clouds(np.stack(host_xyz, axis=1), stamps, np.stack(host_valid, axis=1), take=np.stack(host_take, axis=1),
                                     active=active)
        want_state = o.state()
    finally:
        o.close()
    taken = np.stack(host_take, axis=1) & (active != 0)
    assert want["flags"][1, 0] == 3 and int((want["iterations"] >= 0).sum()) == int(taken.sum())
    assert np.all(want["iterations"][~taken] == -1)
    # the device route
    d_r = ctx.alloc(c["ranges"].nbytes)
    blocks = [(ctx.alloc(n_msgs * n * 12), ctx.alloc(n_msgs * n), ctx.alloc(n_msgs * api.MSYNC_RECORD.itemsize)) for _ in range(R)]
    nodes = [api.MotionSync(ctx) for _ in range(R)]
    o = api.PlicpOdometry(ctx, R)
    try:
        ctx.upload(d_r, np.ascontiguousarray(c["ranges"], np.float32))
        for ms, (d_x, d_v, d_rec) in zip(nodes, blocks):
            H.push_all(ms, c)
            ms.scans_dev(c["laser"], n, d_r, n, c["scan_t"], c["scan_tinc"], d_x, d_v, d_rec, c["imu_seen"], c["odom_seen"])
        before = o.stats()
        got = o.process_many_clouds_dev(n_msgs, n, [b[0] for b in blocks], [b[1] for b in blocks], [b[2] for b in blocks],
                                        api.MSYNC_RECORD.itemsize // 4, stamps, active=active)
        after = o.stats()
        assert got.tobytes() == want.tobytes() and o.state().tobytes() == want_state.tobytes()
        assert after["launches"] == before["launches"] + 1 and after["host_waits"] == before["host_waits"] + 1
    finally:
        o.close()
        for ms in nodes:
            ms.close()
        ctx.free(d_r)
        for b in blocks:
            for p in b:
                ctx.free(p)
