"""lesson5's synchronisation in plain Python: ImuCallback / OdomCallback (the two queues), CacheLaserScan's one-scan lag,
PruneImuDeque and PruneOdomDeque (lesson5/src/lidar_undistortion.cc:82-93, :127-159, :177-249, :252-336) over (stamps,
*_seen) inputs -- pinned against the reference's own node by tests/test_msync_cases_oracle.py, and the second checker of the
device path (tests/test_msync_gpu.py).  `mistakes` turns on ONE wrong reading each (MISTAKES), which the CPU test shows to
give another answer on at least one scenario.

Defined where the reference is not, as csrc/motion_sync.hip defines it: a sample inside the scan with none before the scan's
start (:237 reads imu_time_[-1]) is IMU_NO_LEAD_SAMPLE, more than 2000 integrated samples is IMU_OVERFLOW; both refuse the scan
at the IMU step (the IMU pops stay made, the odometry step does not run)."""
import ctypes
import ctypes.util
import math

import numpy as np

import deskew_restatement as dr

f32 = np.float32
QUEUED, CORRECTED, WAIT_IMU, WAIT_ODOM, IMU_NO_LEAD_SAMPLE, IMU_OVERFLOW = 0, 1, -1, -2, -3, -4
QUEUE_LENGTH = 2000
MISTAKES = ("lower_bound_pop", "retry_refused", "reset_sticky", "strict_end", "keep_every_pre_start", "end_with_scan_count")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "sinf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]

# the ulp bound OpenCL's full profile gives each libm function the odometry increment goes through
ULP_BOUND = {"sin": 4, "cos": 4, "asin": 4, "atan2": 6}


class _Libm:
    """The host libm, every result numbered in call order; `bump` = (call number, +1 / -1) moves that one result by one ulp of
    its own precision (what the device-libm allowance is derived from)."""

    def __init__(self, bump=None):
        self.calls, self.bump = [], bump

    def _out(self, name, v, single):
        k = len(self.calls)
        self.calls.append(name)
        if self.bump is not None and self.bump[0] == k:
            way = math.inf if self.bump[1] > 0 else -math.inf
            v = np.nextafter(f32(v), f32(way)) if single else math.nextafter(v, way)
        return v

    def cos(self, x): return self._out("cos", math.cos(x), False)
    def asin(self, x): return self._out("asin", math.asin(x), False)
    def atan2(self, y, x): return self._out("atan2", math.atan2(y, x), False)
    def cosf(self, x): return self._out("cos", f32(_libm.cosf(float(f32(x)))), True)
    def sinf(self, x): return self._out("sin", f32(_libm.sinf(float(f32(x)))), True)


def _rpy(q, lm):
    """tf::Matrix3x3(q).getRPY: setRotation + getEulerYPR, solution 1 (LinearMath/Matrix3x3.h), double."""
    x, y, z, w = (float(v) for v in q)
    d = x * x + y * y + z * z + w * w
    s = 2.0 / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    m00, m10, m20, m21, m22 = 1.0 - (yy + zz), xy + wz, xz - wy, yz + wx, 1.0 - (xx + yy)
    if abs(m20) >= 1.0:
        return lm.atan2(m21, m22), (math.pi / 2.0 if m20 < 0 else -math.pi / 2.0), 0.0
    pitch = -lm.asin(m20)
    roll = lm.atan2(m21 / lm.cos(pitch), m22 / lm.cos(pitch))
    yaw = lm.atan2(m10 / lm.cos(pitch), m00 / lm.cos(pitch))
    return roll, pitch, yaw


def _transform(pos, quat, lm):
    """pcl::getTransformation (float) of an odometry pose (:307-325)."""
    roll, pitch, yaw = (f32(v) for v in _rpy(quat, lm))
    A, B, Cc, D, E, F = lm.cosf(yaw), lm.sinf(yaw), lm.cosf(pitch), lm.sinf(pitch), lm.cosf(roll), lm.sinf(roll)
    DE, DF = D * E, D * F
    L = np.array([[A * Cc, A * DF - B * E, B * F + A * DE], [B * Cc, A * E + B * DF, B * DE - A * F], [-D, Cc * F, Cc * E]],
                 dtype=np.float32)
    return L, np.array([f32(pos[0]), f32(pos[1]), f32(pos[2])], dtype=np.float32)


DEFAULT_POSE = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))  # a default-constructed nav_msgs/Odometry as oracle/shim states it


def odom_increment(start_pose, end_pose, bump=None, calls_out=None):
    """:304-334: transBegin.inverse() * transEnd, its translation (float32 [3])."""
    lm = _Libm(bump)
    with np.errstate(all="ignore"):
        begin = _transform(start_pose[0], start_pose[1], lm)
        end = _transform(end_pose[0], end_pose[1], lm)
        _, t = dr.mul(dr.inverse(*begin), end)
    if calls_out is not None:
        calls_out[:] = lm.calls
    return t.astype(np.float32)


def odom_increment_allowance(start_pose, end_pose):
    """What another libm may change in odom_incre [3]: the sum, over every libm result in getRPY and getTransformation, of the
    change one ulp in that result makes, times the function's ulp bound (ULP_BOUND)."""
    calls = []
    base = odom_increment(start_pose, end_pose, calls_out=calls).astype(np.float64)
    allow = np.zeros(3)
    for k, name in enumerate(calls):
        change = np.zeros(3)
        for way in (1, -1):
            moved = odom_increment(start_pose, end_pose, bump=(k, way)).astype(np.float64)
            change = np.maximum(change, np.abs(moved - base))
        allow += change * ULP_BOUND[name]
    return allow


class Node:
    """The node's state between callbacks.  Message indices are global (counted since construction)."""

    def __init__(self, n_readings, use_imu=True, use_odom=True, mistakes=()):
        unknown = set(mistakes) - set(MISTAKES)
        assert not unknown, unknown
        self.mistakes = frozenset(mistakes)
        self.use_imu, self.use_odom = bool(use_imu), bool(use_odom)
        self.scan_count = int(n_readings)
        self.imu_t, self.imu_w = [], []
        self.odom_t, self.odom_pose = [], []
        self.imu_front = self.odom_front = 0
        self.start_odom = self.end_odom = -1
        self.queued = []  # laser_queue_: (stamp, time_increment as float32)

    def push_imu(self, stamps, gyro):
        self.imu_t += [float(t) for t in stamps]
        self.imu_w += [tuple(float(v) for v in w) for w in gyro]

    def push_odom(self, stamps, pos, quat):
        self.odom_t += [float(t) for t in stamps]
        self.odom_pose += [(tuple(float(v) for v in p), tuple(float(v) for v in q)) for p, q in zip(pos, quat)]

    def _pop(self, stamps, front, seen, start):
        if "lower_bound_pop" in self.mistakes:  # a binary search: right only where the stamps are sorted
            return self._lower_bound(stamps, front, seen, start - 0.1)
        while front < seen and stamps[front] < start - 0.1:  # :191-197, literally
            front += 1
        return front

    @staticmethod
    def _lower_bound(stamps, front, seen, lim):
        lo, hi = front, seen
        while lo < hi:
            mid = (lo + hi) // 2
            if stamps[mid] < lim:
                lo = mid + 1
            else:
                hi = mid
        return lo

    def scan(self, stamp, time_increment, imu_seen=None, odom_seen=None):
        """One ScanCallback -> the record of lslam_msync_record, plus imu_time / imu_rot of a corrected scan."""
        imu_seen = len(self.imu_t) if imu_seen is None else int(imu_seen)
        odom_seen = len(self.odom_t) if odom_seen is None else int(odom_seen)
        rec = {"status": QUEUED, "n_imu": 0, "scan_time_start": 0.0, "time_increment": 0.0, "start_odom_time": 0.0,
               "end_odom_time": 0.0, "odom_incre": np.zeros(3, np.float32), "imu_time": np.zeros(0), "imu_rot": np.zeros((0, 3)),
               "start_pose": None, "end_pose": None}
        self.queued.append((float(stamp), f32(time_increment)))
        if len(self.queued) >= 2:  # :145-156
            start, tinc = self.queued[0]
            tinc = float(tinc)
            beams = self.scan_count if "end_with_scan_count" in self.mistakes else self.scan_count - 1
            end = start + tinc * float(beams)
            rec["scan_time_start"], rec["time_increment"] = start, tinc
            status = CORRECTED
            if self.use_imu:
                status = self._prune_imu(rec, start, end, imu_seen)
            if self.use_odom and status == CORRECTED:
                status = self._prune_odom(rec, start, end, odom_seen)
            rec["status"] = status
            if status == CORRECTED or "retry_refused" not in self.mistakes:
                self.queued.pop(0)  # a refused scan has left laser_queue_ (:149-150): dropped, not retried
            if status != CORRECTED:
                rec["n_imu"], rec["imu_time"], rec["imu_rot"] = 0, np.zeros(0), np.zeros((0, 3))
        rec.update(imu_front=self.imu_front, odom_front=self.odom_front, start_odom_index=self.start_odom,
                   end_odom_index=self.end_odom)
        return rec

    def _prune_imu(self, rec, start, end, seen):
        t, f = self.imu_t, self.imu_front
        if f >= seen or t[f] > start or t[seen - 1] < end:  # :182-188
            return WAIT_IMU
        f = self.imu_front = self._pop(t, f, seen, start)
        if f >= seen:
            return WAIT_IMU
        times, rots = [], []
        for i in range(f, seen):  # :207-243
            if t[i] < start:
                if not times:  # :215-222: the first one is sample 0, rotation 0; later ones are skipped
                    times.append(t[i])
                    rots.append((0.0, 0.0, 0.0))
                elif "keep_every_pre_start" in self.mistakes:
                    dt = t[i] - times[-1]
                    rots.append(tuple(rots[-1][a] + self.imu_w[i][a] * dt for a in range(3)))
                    times.append(t[i])
                continue
            if t[i] > end:
                break
            if not times:
                return IMU_NO_LEAD_SAMPLE  # :237 would read imu_time_[-1]
            if len(times) >= QUEUE_LENGTH:
                return IMU_OVERFLOW  # :238-241 would write imu_rot_*[2000]
            dt = t[i] - times[-1]
            rots.append(tuple(rots[-1][a] + self.imu_w[i][a] * dt for a in range(3)))
            times.append(t[i])
        rec["n_imu"] = len(times)
        rec["imu_time"] = np.array(times, np.float64)
        rec["imu_rot"] = np.array(rots, np.float64).reshape(len(times), 3)
        return CORRECTED

    def _prune_odom(self, rec, start, end, seen):
        t, f = self.odom_t, self.odom_front
        if f >= seen or t[f] > start or t[seen - 1] < end:  # :257-263
            return WAIT_ODOM
        f = self.odom_front = self._pop(t, f, seen, start)
        if f >= seen:
            return WAIT_ODOM
        if "reset_sticky" in self.mistakes:
            self.start_odom = self.end_odom = -1
        for i in range(f, seen):  # :280-296
            if t[i] < start:
                self.start_odom = i
                continue
            if (t[i] < end) if "strict_end" in self.mistakes else (t[i] <= end):
                self.end_odom = i
            else:
                break
        rec["start_odom_time"] = t[self.start_odom] if self.start_odom >= 0 else 0.0
        rec["end_odom_time"] = t[self.end_odom] if self.end_odom >= 0 else 0.0
        rec["start_pose"] = self.odom_pose[self.start_odom] if self.start_odom >= 0 else DEFAULT_POSE
        rec["end_pose"] = self.odom_pose[self.end_odom] if self.end_odom >= 0 else DEFAULT_POSE
        rec["odom_incre"] = odom_increment(rec["start_pose"], rec["end_pose"])
        return CORRECTED


def run(case, mistakes=(), use_imu=None, use_odom=None):
    """Every scan callback of a scenario (tests/msync_cases.py), all messages pushed first and seen as `*_seen` say."""
    node = Node(case["ranges"].shape[1], case["use_imu"] if use_imu is None else use_imu,
                case["use_odom"] if use_odom is None else use_odom, mistakes)
    node.push_imu(case["imu_t"], case["imu_w"])
    node.push_odom(case["odom_t"], case["odom_pos"], case["odom_quat"])
    return [node.scan(case["scan_t"][k], case["scan_tinc"][k], case["imu_seen"][k], case["odom_seen"][k])
            for k in range(len(case["scan_t"]))]
