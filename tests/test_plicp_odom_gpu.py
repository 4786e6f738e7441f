"""lesson3's keyframe odometry on the device (csrc/plicp.hip's k_plicp_odom, api.PlicpOdometry) against the SE(2) restatement
over tools/plicp_cpu.py's sm_icp (tests/plicp_odometry_restatement.py): flags and `valid` one for one, poses within the
project's contract of 1e-4 m / 1e-4 rad (measured: see DESIGN.md 4.20), the truth within n_scans x 1e-6, tracks and call
splits byte for byte."""
import math

import numpy as np
import pytest

import plicp_cases as K
import plicp_odometry_restatement as O
from lslam_amd import api

pytestmark = pytest.mark.gpu


def _odo(ctx, log, n_tracks=1):
    return api.PlicpOdometry(ctx, n_tracks, base_to_laser=log.base_to_laser, laser=K.LASER360)


@pytest.fixture(scope="module")
def device(ctx):
    """Every log in one call at R = 1: which -> (records [n], state [1])."""
    out = {}
    for which in ("keyframe", "offset", "invalid"):
        log, _ = O.run(which)
        o = _odo(ctx, log)
        try:
            rec = o.process_many(log.ranges, log.stamps)[:, 0]
            out[which] = (rec, o.state(), o.stats())
        finally:
            o.close()
    return out


@pytest.mark.parametrize("which", ["keyframe", "offset", "invalid"])
def test_flags_valid_and_poses_are_the_restatements(device, which):
    log, steps = O.run(which)
    rec = device[which][0]
    worst = 0.0
    for k, s in enumerate(steps):
        assert (int(rec[k]["flags"]), int(rec[k]["valid"])) == (s.flags, s.valid), k
        assert (int(rec[k]["iterations"]), int(rec[k]["nvalid"])) == (s.iterations, s.nvalid), k
        d = np.abs(rec[k]["base_in_odom"] - np.array(s.base_in_odom))
        d[2] = abs(math.remainder(rec[k]["base_in_odom"][2] - s.base_in_odom[2], 2 * math.pi))
        worst = max(worst, d.max())
    print(which, "max |pose - restatement|", worst)
    assert worst <= 1e-4


@pytest.mark.parametrize("which", ["keyframe", "offset"])
def test_the_truth_is_tracked(device, which):
    log, _ = O.run(which)
    rec = device[which][0]
    worst = 0.0
    for k in range(len(rec)):
        want = O.mul(O.inv(tuple(log.poses[0])), tuple(log.poses[k]))
        e = rec[k]["base_in_odom"] - np.array(want)
        worst = max(worst, math.hypot(e[0], e[1]), abs(math.remainder(e[2], 2 * math.pi)))
    print(which, "worst pose error against the truth", worst)
    assert worst <= len(rec) * 1e-6


def test_an_invalid_match_leaves_the_pose(device):
    rec = device["invalid"][0]
    assert rec[6]["valid"] == 0 and rec[6]["base_in_odom"].tobytes() == rec[5]["base_in_odom"].tobytes()


def test_one_host_wait_per_call(device):
    for which, (rec, state, stats) in device.items():
        # process_many waits once; state() is a second, separate wait
        assert stats["launches"] == 1 and stats["host_waits"] == 2 and stats["scans"] == len(rec), (which, stats)
        assert state["initialized"][0] == 1


@pytest.mark.parametrize("split", [1, 7])
def test_calls_of_any_length_give_the_same_records_and_state(ctx, device, split):
    log, _ = O.run("keyframe")
    whole, state, _ = device["keyframe"]
    o = _odo(ctx, log)
    try:
        parts = [o.process_many(log.ranges[a:a + split], log.stamps[a:a + split])[:, 0] for a in range(0, len(log.ranges), split)]
        assert np.concatenate(parts).tobytes() == whole.tobytes()
        assert o.state().tobytes() == state.tobytes()
        o.reset()                                                         # and again after a reset
        assert o.process_many(log.ranges, log.stamps)[:, 0].tobytes() == whole.tobytes()
    finally:
        o.close()


def test_three_ragged_tracks_are_each_the_track_alone(ctx, device):
    logs = [O.run(w)[0] for w in ("keyframe", "offset", "invalid")]
    alone = [device[w][0] for w in ("keyframe", "offset", "invalid")]
    # no base_to_laser per track: the tracks share the handle's, so the offset log runs here under the zero transform
    o1 = api.PlicpOdometry(ctx, 1, laser=K.LASER360)
    try:
        alone[1] = o1.process_many(logs[1].ranges, logs[1].stamps)[:, 0]
    finally:
        o1.close()
    # track t's scans sit at steps where (step + t) % 3 != 0 until they run out
    n_steps = 64
    ranges = np.full((n_steps, 3, 360), np.nan, np.float32)
    stamps = np.zeros((n_steps, 3))
    active = np.zeros((n_steps, 3), np.uint8)
    where = [[], [], []]
    for t in range(3):
        k = 0
        for step in range(n_steps):
            if (step + t) % 3 != 0 and k < len(logs[t].ranges):
                ranges[step, t], stamps[step, t], active[step, t] = logs[t].ranges[k], logs[t].stamps[k], 1
                where[t].append(step)
                k += 1
        assert k == len(logs[t].ranges)
    o = api.PlicpOdometry(ctx, 3, laser=K.LASER360)
    try:
        rec = o.process_many(ranges, stamps, active)
        st = o.stats()
    finally:
        o.close()
    assert st["launches"] == 1 and st["host_waits"] == 1 and st["scans"] == int(active.sum())
    for t in range(3):
        assert rec[where[t], t].tobytes() == alone[t].tobytes(), t
        idle = rec[active[:, t] == 0, t]
        assert np.all(idle["iterations"] == -1)
        z = idle.copy()
        z["iterations"] = 0
        assert z.tobytes() == bytes(z.nbytes)                            # zero except iterations = -1


def test_refusals(ctx):
    log, _ = O.run("invalid")
    o = api.PlicpOdometry(ctx, 1)                                         # no laser set
    try:
        with pytest.raises(api.LslamError) as e:
            o.process_many(log.ranges, log.stamps)
        assert e.value.code == -1
        o.set_laser(K.LASER360.angle_min, K.LASER360.angle_increment, 0.1, 30.0)
        with pytest.raises(api.LslamError) as e:
            o.process_many(np.ones((1, 1, 2049), np.float32), [0.0])
        assert e.value.code == -8
        before = o.stats()
        assert o.process_many(np.zeros((0, 1, 360), np.float32), np.zeros((0, 1))).shape == (0, 1) and o.stats() == before
    finally:
        o.close()
