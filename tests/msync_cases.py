"""Scenarios for lesson5's synchronisation (tests/test_msync_cases_oracle.py on the CPU, tests/test_msync_gpu.py on the device):
raw IMU, odometry and LaserScan message logs of 64 to 360 beams, at most 40 scan messages, each built to reach one edge of
PruneImuDeque / PruneOdomDeque (lesson5/src/lidar_undistortion.cc:177-336).  CASES[name]() -> a dict:

    imu_t [I], imu_w [I, 3], odom_t [O], odom_pos [O, 3], odom_quat [O, 4] (xyzw), scan_t [S], scan_tinc [S] float32,
    ranges [S, n] float32, imu_seen [S], odom_seen [S] int64 (messages arrived when scan callback k ran), laser
    (angle_min, angle_increment, range_min, range_max), use_imu, use_odom,
    ref_callbacks: how many scan callbacks the reference's own node may be given (the callback that integrates 2001 samples
    would write past the node's arrays).

Odometry positions stay below 16 m, the range in which the de-skew's contract of 4e-6 m was pinned."""
import functools
import math

import numpy as np

f32 = np.float32


def _ranges(n_scans, n, seed):
    """A 6 m square room seen from a point that drifts a little, with a few beams the node skips."""
    rng = np.random.default_rng(seed)
    a = -math.pi + np.arange(n) * (2.0 * math.pi / n)
    out = np.zeros((n_scans, n), np.float32)
    for k in range(n_scans):
        r = (3.0 + 0.05 * k) / np.maximum(np.abs(np.cos(a)), np.abs(np.sin(a))) + rng.normal(0, 0.01, n)
        r[rng.integers(0, n, 3)] = np.inf
        r[rng.integers(0, n, 2)] = 0.0
        if k % 5 == 4:
            r[:3] = np.nan  # the first valid beam is not beam 0
        out[k] = r
    return out


def _odom(stamps, t0):
    """A pose that moves on an arc (below 16 m) and turns, with a little roll and pitch."""
    s = np.asarray(stamps, np.float64) - t0
    pos = np.stack([1.5 + 1.2 * s, -2.0 + 0.8 * np.sin(0.7 * s), 0.05 * s], 1)
    yaw, pitch, roll = 0.4 * s + 0.3, 0.02 * np.sin(s), 0.015 * np.cos(1.3 * s)
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    quat = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy], 1)
    return pos, quat


def _gyro(stamps, t0):
    s = np.asarray(stamps, np.float64) - t0
    return np.stack([0.05 * np.sin(3.0 * s), 0.04 * np.cos(2.0 * s), 0.4 + 0.1 * np.sin(1.7 * s)], 1)


def _seen(msg_t, when):
    """Messages that had arrived at each callback time (arrival = stamp order of the log, so a count), non-decreasing."""
    arrival = np.maximum.accumulate(np.asarray(msg_t, np.float64))
    return np.maximum.accumulate(np.searchsorted(arrival, when, side="right")).astype(np.int64)


def _case(n=64, n_scans=12, t0=10.0, period=0.1, dur=0.08, imu_hz=200.0, odom_hz=20.0, lag=0.02, imu_lag=None, odom_lag=None,
          seed=1, scan_t=None, imu_t=None, odom_t=None, use_imu=True, use_odom=True, jitter=True):
    rng = np.random.default_rng(seed)
    if scan_t is None:
        scan_t = t0 + period * np.arange(n_scans)
    scan_t = np.asarray(scan_t, np.float64)
    n_scans = len(scan_t)
    tinc = np.full(n_scans, dur / (n - 1), np.float32)
    tinc[1::3] *= f32(0.9)  # per-scan durations
    t_end = scan_t.max() + dur + 0.6
    if imu_t is None:
        imu_t = np.arange(t0 - 0.3, t_end, 1.0 / imu_hz)
        if jitter:
            imu_t = imu_t + rng.uniform(-0.2, 0.2, len(imu_t)) / imu_hz
    if odom_t is None:
        odom_t = np.arange(t0 - 0.3, t_end, 1.0 / odom_hz)
        if jitter:
            odom_t = odom_t + rng.uniform(-0.2, 0.2, len(odom_t)) / odom_hz
    imu_t, odom_t = np.asarray(imu_t, np.float64), np.asarray(odom_t, np.float64)
    lag = np.resize(np.asarray(lag, np.float64), n_scans)
    when = scan_t + dur + lag  # a scan's message arrives once the scan is over
    pos, quat = _odom(odom_t, t0)
    return {"imu_t": imu_t, "imu_w": _gyro(imu_t, t0), "odom_t": odom_t, "odom_pos": pos, "odom_quat": quat, "scan_t": scan_t,
            "scan_tinc": tinc, "ranges": _ranges(n_scans, n, seed),
            "imu_seen": _seen(imu_t, when if imu_lag is None else scan_t + dur + np.resize(np.asarray(imu_lag, np.float64), n_scans)),
            "odom_seen": _seen(odom_t, when if odom_lag is None else scan_t + dur + np.resize(np.asarray(odom_lag, np.float64), n_scans)),
            "laser": (f32(-math.pi), f32(2.0 * math.pi / n), f32(0.1), f32(30.0)), "use_imu": use_imu, "use_odom": use_odom,
            "ref_callbacks": n_scans}


def steady():
    return _case(n=360, n_scans=14, imu_hz=200.0, odom_hz=20.0, seed=2)


def interleaved():
    """Callback lags of 0.02 / 0.15 / 0.3 s: the queues hold another number of messages at every callback."""
    return _case(n=128, n_scans=16, imu_hz=400.0, odom_hz=50.0, lag=[0.02, 0.15, 0.3], seed=3)


def imu_gap():
    """No IMU message between 10.35 and 10.62 s.  The IMU messages reach callbacks 1 and 2 late (a refusal: the queue's back is older
    than the scan's end); the scan that starts at 10.5 has no sample from start - 0.1 to its end and is corrected with zero
    rotation (edge 1); the next one finds the front later than its start (a refusal)."""
    c = _case(n=96, n_scans=12, imu_hz=100.0, lag=0.05, imu_lag=[0.05, -0.12, -0.12] + [0.05] * 9, seed=4)
    keep = (c["imu_t"] < 10.35) | (c["imu_t"] > 10.62)
    return _case(n=96, n_scans=12, imu_hz=100.0, lag=0.05, imu_lag=[0.05, -0.12, -0.12] + [0.05] * 9, seed=4, imu_t=c["imu_t"][keep])


def no_lead():
    """No IMU message from 10.38 to 10.5005 s: for the scan that starts at 10.5 every sample older than the start is popped
    (older than start - 0.1 too), and the window has samples (edge 2)."""
    c = _case(n=64, n_scans=10, imu_hz=200.0, lag=0.05, seed=5, jitter=False)
    t = c["imu_t"]
    keep = (t < 10.38) | (t > 10.5005)
    return _case(n=64, n_scans=10, imu_hz=200.0, lag=0.05, seed=5, jitter=False, imu_t=t[keep])


def sparse_odom():
    """Odometry at 8 Hz against 0.08 s scans every 0.1 s: scans with no message inside them (the end message is the previous
    scan's) and scans with none between start - 0.1 and start (so is the start message)."""
    return _case(n=64, n_scans=24, imu_hz=100.0, odom_hz=8.0, lag=0.15, seed=6)


def default_start():
    """The first odometry stamp equals the first scan's start exactly: no message is before the start, so the start message is
    the default-constructed one.  Another stamp equals scan 3's end exactly (the <= of :290 takes it as the end message)."""
    t0 = 10.0
    odom_t = t0 + 0.05 * np.arange(40)
    c = _case(n=64, n_scans=8, t0=t0, imu_hz=200.0, lag=0.05, seed=7, odom_t=odom_t)
    end3 = c["scan_t"][3] + float(c["scan_tinc"][3]) * 63.0
    odom_t[int(np.searchsorted(odom_t, end3))] = end3
    return _case(n=64, n_scans=8, t0=t0, imu_hz=200.0, lag=0.05, seed=7, odom_t=odom_t)


FRONT_STRIDES = (1, 63, 64, 65, 200, 0, 40, 40, 0, 1)


def front_strides():
    """IMU at 400 Hz on an exact grid, scan starts half-way between grid points: scan k pops exactly FRONT_STRIDES[k - 1]
    messages more than scan k - 1 did (0: two scans with one stamp)."""
    grid = 9.0 + 0.0025 * np.arange(1200)
    scan_t = 10.00125 + 0.0025 * np.concatenate([[0], np.cumsum(FRONT_STRIDES)])
    scan_t = np.concatenate([scan_t, [scan_t[-1] + 0.1]])  # one more callback, for the last scan
    return _case(n=64, scan_t=scan_t, dur=0.05, lag=0.05, seed=8, imu_t=grid, odom_hz=50.0, jitter=False)


WINDOW_SIZES = (1, 2, 64, 65, 257, 2000, 2001)


def window_sizes():
    """Scan k integrates exactly WINDOW_SIZES[k] samples: one before its start and WINDOW_SIZES[k] - 1 inside it.  2001 is one
    more than the node's arrays hold (IMU_OVERFLOW); the reference is not given that callback."""
    dur = 0.08
    scan_t = 10.0 + 0.5 * np.arange(len(WINDOW_SIZES) + 1)
    imu_t = [np.array([9.5])]
    for s, m in zip(scan_t, WINDOW_SIZES):
        imu_t.append(np.array([s - 0.05]))
        if m > 1:
            imu_t.append(np.linspace(s + 0.001, s + 0.07, m - 1))
    imu_t.append(np.array([scan_t[-1] - 0.05, scan_t[-1] + 1.0]))
    c = _case(n=64, scan_t=scan_t, dur=dur, lag=0.05, seed=9, imu_t=np.concatenate(imu_t), odom_hz=20.0, jitter=False)
    c["ref_callbacks"] = len(WINDOW_SIZES)  # callback k corrects scan k - 1: the last callback is the 2001-sample one
    return c


def non_monotone():
    """One IMU and one odometry stamp 0.3 s ahead of their place: the literal pop stops at them while older messages follow."""
    c = _case(n=64, n_scans=14, imu_hz=100.0, odom_hz=20.0, lag=0.05, seed=10)
    imu_t, odom_t = c["imu_t"].copy(), c["odom_t"].copy()
    imu_t[int(np.searchsorted(imu_t, 10.33))] += 0.3
    odom_t[int(np.searchsorted(odom_t, 10.71))] += 0.3
    return _case(n=64, n_scans=14, imu_hz=100.0, odom_hz=20.0, lag=0.05, seed=10, imu_t=imu_t, odom_t=odom_t)


def epoch():
    """Stamps near 1.7e9 s: start - 0.1 and the time differences lose twenty bits."""
    return _case(n=64, n_scans=10, t0=1.7e9 + 0.25, imu_hz=200.0, odom_hz=20.0, lag=0.05, seed=11)


def flags():
    """Run under the four use_imu / use_odom combinations (FLAG_COMBINATIONS); the odometry arrives late for two callbacks."""
    return _case(n=64, n_scans=10, imu_hz=200.0, odom_hz=20.0, lag=0.05, odom_lag=[0.05] * 4 + [-0.25, -0.25] + [0.05] * 4, seed=12)


FLAG_COMBINATIONS = ((True, True), (True, False), (False, True), (False, False))


def odom_wait():
    """The odometry messages reach callbacks 3 and 4 late: PruneOdomDeque refuses after PruneImuDeque has popped."""
    return _case(n=64, n_scans=10, imu_hz=200.0, odom_hz=20.0, lag=0.05, odom_lag=[0.05] * 3 + [-0.25, -0.25] + [0.05] * 5, seed=13)


CASES = {f.__name__: functools.lru_cache(maxsize=None)(f) for f in
         (steady, interleaved, imu_gap, no_lead, sparse_odom, default_start, front_strides, window_sizes, non_monotone, epoch, flags,
          odom_wait)}


def run_reference(po, case, use_imu=None, use_odom=None):
    """The reference's own node (po.RefLesson5) over a scenario: before scan callback k it is given the IMU and odometry
    messages that had arrived by then.  -> per callback None (queued or refused) or RefLesson5.scan's dict."""
    node = po.RefLesson5(case["use_imu"] if use_imu is None else use_imu, case["use_odom"] if use_odom is None else use_odom)
    out, ni, no = [], 0, 0
    for k in range(case["ref_callbacks"]):
        for ni in range(ni, int(case["imu_seen"][k])):
            node.add_imu(case["imu_t"][ni], case["imu_w"][ni])
        ni = int(case["imu_seen"][k])
        for no in range(no, int(case["odom_seen"][k])):
            node.add_odom(case["odom_t"][no], case["odom_pos"][no], case["odom_quat"][no])
        no = int(case["odom_seen"][k])
        out.append(node.scan(case["scan_t"][k], case["laser"][0], case["laser"][1], case["scan_tinc"][k], case["laser"][2],
                             case["laser"][3], case["ranges"][k]))
    node.close()
    return out
