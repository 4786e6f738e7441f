"""lesson3's keyframe odometry node (lesson3/src/plicp_odometry.cc: ScanCallback :191-232, ScanMatchWithPLICP :327-436,
GetPrediction :442-456, NewKeyframeNeeded :498-517) restated in SE(2) over tools/plicp_cpu.py's sm_icp, with the three
rules of include/lslam_gpu.h: an invalid match leaves corr_ch at the identity and the state untouched, the prediction is the
reference's literally (linear.x only; nothing for a speed below 1e-6, a negative one included).

Also the 40-scan log that drives every keyframe rule, and a log with an invalid match."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

import plicp_cases as K
from lslam_amd import synth
from tools import plicp_cpu as P


def yaw(th):
    return math.atan2(math.sin(th), math.cos(th))  # tf2::getYaw of the rotation


def mul(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    return (a[0] + (c * b[0] - s * b[1]), a[1] + (s * b[0] + c * b[1]), yaw(a[2] + b[2]))


def inv(a):
    c, s = math.cos(a[2]), math.sin(a[2])
    return (-(c * a[0] + s * a[1]), -(-s * a[0] + c * a[1]), yaw(-a[2]))


@dataclasses.dataclass
class Step:
    flags: int
    valid: int
    iterations: int
    nvalid: int
    x: np.ndarray
    base_in_odom: tuple
    margins: list  # (name, value, threshold) of every threshold comparison made for this scan


class Odometry:
    def __init__(self, laser, params=None, kf_dist_linear=0.1, kf_dist_angular=5.0 * (math.pi / 180.0), kf_scan_count=10,
                 base_to_laser=(0.0, 0.0, 0.0)):
        self.laser, self.params = laser, params or P.PlicpParams()
        self.kf_lin_sq, self.kf_ang, self.kf_count = kf_dist_linear * kf_dist_linear, kf_dist_angular, kf_scan_count
        self.b2l = tuple(float(v) for v in base_to_laser)
        self.l2b = inv(self.b2l)
        self.base = (0.0, 0.0, 0.0)
        self.kf = (0.0, 0.0, 0.0)
        self.v_lin = self.v_ang = 0.0
        self.last = 0.0
        self.count = 0
        self.initialized = False
        self.ref = None

    def _ldp(self, ranges):
        L = self.laser
        return P.laser_scan_to_ldp(ranges, L.angle_min, L.angle_increment, L.range_min, L.range_max)

    def process(self, ranges, stamp) -> Step:
        if not self.initialized:
            self.initialized, self.ref, self.last = True, self._ldp(ranges), stamp
            return Step(3, 0, 0, 0, np.zeros(3), self.base, [])
        margins = []
        dt = stamp - self.last
        margins.append(("speed", self.v_lin, 1e-6))
        pred = (0.0 if self.v_lin < 1e-6 else dt * self.v_lin, 0.0, 0.0)
        pc = mul(pred, mul(self.base, inv(self.kf)))
        pcl = mul(mul(mul(mul(self.l2b, inv(self.base)), pc), self.base), self.b2l)
        cur = self._ldp(ranges)
        out = P.sm_icp(self.params, self.ref, cur, (pcl[0], pcl[1], yaw(pcl[2])))
        corr = (0.0, 0.0, 0.0)
        if out["valid"]:
            corr = mul(mul(self.b2l, tuple(out["x"])), self.l2b)
            self.base = mul(self.kf, corr)
            self.v_lin = corr[0] / dt
            self.v_ang = yaw(corr[2]) / dt
        self.count += 1
        margins.append(("angle", abs(yaw(corr[2])), self.kf_ang))
        if abs(yaw(corr[2])) > self.kf_ang:
            fresh = True
        elif self.count == self.kf_count:
            self.count = 0
            fresh = True
        else:
            margins.append(("distance", corr[0] * corr[0] + corr[1] * corr[1], self.kf_lin_sq))
            fresh = corr[0] * corr[0] + corr[1] * corr[1] > self.kf_lin_sq
        if fresh:
            self.ref, self.kf = cur, self.base
        self.last = stamp
        return Step(2 if fresh else 0, out["valid"], out["iterations"], out["nvalid"], np.array(out["x"]), self.base, margins)


@dataclasses.dataclass
class Log:
    ranges: np.ndarray   # [n, 360] float32
    stamps: np.ndarray   # [n] seconds
    poses: np.ndarray    # [n, 3] the true base poses in the world
    base_to_laser: tuple


def _free_start(rng, reach=0.9):
    """A start pose whose whole neighbourhood (the log moves less than `reach` from it) keeps 0.6 m from every wall."""
    for _ in range(10000):
        a = np.array([rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-math.pi, math.pi)])
        if all(synth.point_is_free(K.world(), a[0] + dx, a[1] + dy) for dx in (-reach, 0, reach) for dy in (-reach, 0, reach)):
            return a
    raise RuntimeError("no free start pose in the arena")


@functools.lru_cache(maxsize=None)
def keyframe_log(base_to_laser=(0.0, 0.0, 0.0)) -> Log:
    """40 noise-free 360-beam scans: 14 steps of 0.03-0.06 m forward (keyframes by distance), a turn on the spot in 13 steps of
    0.025 rad (keyframes by angle; scan 20 is none of them, or scan_count would pass 10 unseen and the count rule never fire
    again), 12 scans standing still (a keyframe by count)."""
    rng = np.random.default_rng(31)
    pose = _free_start(rng)
    steps = [(rng.uniform(0.03, 0.06), 0.0, 0.0) for _ in range(14)] + [(0.0, 0.0, 0.025)] * 13 + [(0.0, 0.0, 0.0)] * 12
    poses = [pose]
    for d in steps:
        poses.append(K.compose(poses[-1], d))
    poses = np.array(poses)
    assert len(poses) == 40
    ranges = np.stack([synth.cast_scan(K.world(), K.compose(p, base_to_laser), K.LASER360) for p in poses])
    return Log(ranges, 0.1 * np.arange(40), poses, tuple(base_to_laser))


@functools.lru_cache(maxsize=None)
def invalid_log() -> Log:
    """12 scans; between scans 5 and 6 the robot jumps 1.5 m: the match against the keyframe is beyond max_linear_correction
    (or finds no answer), so it is invalid and the pose stays."""
    rng = np.random.default_rng(32)
    pose = _free_start(rng, 1.6)
    steps = [(0.04, 0.0, 0.0)] * 5 + [(1.1, 0.3, 0.0)] + [(0.04, 0.0, 0.0)] * 5
    poses = [pose]
    for d in steps:
        poses.append(K.compose(poses[-1], d))
    poses = np.array(poses)
    ranges = np.stack([synth.cast_scan(K.world(), p, K.LASER360) for p in poses])
    return Log(ranges, 0.1 * np.arange(len(poses)), poses, (0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def run(which: str):
    """The restatement over a log -> (Log, [Step])."""
    log = {"keyframe": keyframe_log, "offset": lambda: keyframe_log((0.2, -0.1, 0.3)), "invalid": invalid_log}[which]()
    odo = Odometry(K.LASER360, base_to_laser=log.base_to_laser)
    return log, [odo.process(r, t) for r, t in zip(log.ranges, log.stamps)]
