"""ctypes host binding of liblslam_gpu.so (include/lslam_gpu.h).

Python is only the harness language of this repo (tests, bench); the classes mirror the
reference's operator interface for the hot path so the parity tests read like calls into the
reference:

* ``ScanMatcher``  <-> karto::ScanMatcher      (Mapper.h:1127-1279): Create / MatchScan /
  CorrelateScan-level batched search / GetCorrelationGrid
* ``OccGridMap``   <-> hectorslam::OccGridMapBase + MapRepMultiMap (H/map/OccGridMapBase.h,
  H/slam_main/MapRepMultiMap.h): updateByScan / updateByScanJustOnce / getGridMap

There is NO CPU fallback here: if the shared library or a GPU is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import math
import weakref

import numpy as np

from . import build as _build

LSLAM_OK = 0
ERRORS = {
    -1: "LSLAM_ERR_INVALID_ARGUMENT",
    -2: "LSLAM_ERR_NO_DEVICE",
    -3: "LSLAM_ERR_INDEX_OUT_OF_RANGE",
    -4: "LSLAM_ERR_PROBABILITY_SEARCH",
    -5: "LSLAM_ERR_NO_BEST_POSE",
    -6: "LSLAM_ERR_HIP",
    -7: "LSLAM_ERR_SMEAR_DEVIATION",
    -8: "LSLAM_ERR_UNSUPPORTED",
}


class LslamError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class MatcherConfig(C.Structure):
    """lslam_matcher_config (ScanMatcher::Create args + the Mapper parameters the matcher reads)."""

    _fields_ = [
        ("search_size", C.c_double),
        ("resolution", C.c_double),
        ("smear_deviation", C.c_double),
        ("range_threshold", C.c_double),
        ("coarse_search_angle_offset", C.c_double),
        ("coarse_angle_resolution", C.c_double),
        ("fine_search_angle_offset", C.c_double),
        ("distance_variance_penalty", C.c_double),
        ("angle_variance_penalty", C.c_double),
        ("minimum_distance_penalty", C.c_double),
        ("minimum_angle_penalty", C.c_double),
        ("use_response_expansion", C.c_int32),
        ("reserved", C.c_int32),
    ]


class LaserParams(C.Structure):
    """lslam_laser (karto::LaserRangeFinder parameters)."""

    _fields_ = [
        ("minimum_angle", C.c_double),
        ("maximum_angle", C.c_double),
        ("angular_resolution", C.c_double),
        ("minimum_range", C.c_double),
        ("maximum_range", C.c_double),
        ("range_threshold", C.c_double),
        ("offset_x", C.c_double),
        ("offset_y", C.c_double),
        ("offset_heading", C.c_double),
    ]


class MatchResult(C.Structure):
    _fields_ = [
        ("pose", C.c_double * 3),
        ("response", C.c_double),
        ("covariance", C.c_double * 9),
        ("status", C.c_int32),
        ("flags", C.c_int32),
    ]


RESULT_DTYPE = np.dtype(
    [("pose", "f8", 3), ("response", "f8"), ("covariance", "f8", (3, 3)), ("status", "i4"), ("flags", "i4")]
)
assert RESULT_DTYPE.itemsize == 112 == C.sizeof(MatchResult)


class FrontEndConfig(C.Structure):
    """lslam_frontend_config: the Mapper parameters Mapper::Process / MapperGraph read (Mapper.cpp:1457-1604)."""

    _fields_ = [
        ("scan_buffer_size", C.c_int32),
        ("use_scan_barycenter", C.c_int32),
        ("do_loop_closing", C.c_int32),
        ("loop_match_minimum_chain_size", C.c_int32),
        ("scan_buffer_maximum_scan_distance", C.c_double),
        ("minimum_travel_distance", C.c_double),
        ("minimum_travel_heading", C.c_double),
        ("minimum_time_interval", C.c_double),
        ("link_match_minimum_response_fine", C.c_double),
        ("link_scan_maximum_distance", C.c_double),
        ("loop_search_maximum_distance", C.c_double),
        ("loop_match_maximum_variance_coarse", C.c_double),
        ("loop_match_minimum_response_coarse", C.c_double),
        ("loop_match_minimum_response_fine", C.c_double),
        ("loop_search_space_dimension", C.c_double),
        ("loop_search_space_resolution", C.c_double),
        ("loop_search_space_smear_deviation", C.c_double),
    ]


def frontend_config(**kw) -> FrontEndConfig:
    """Library defaults (lslam_frontend_config_defaults) with keyword overrides."""
    c = FrontEndConfig()
    lib().lslam_frontend_config_defaults(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


class HectorScan(C.Structure):
    """lslam_hector_scan: LaserScan header + the node's filters + the base_link -> laser transform."""

    _fields_ = [(k, C.c_float) for k in (
        "angle_min", "angle_increment", "range_min", "range_max", "range_cutoff", "sqr_laser_min_dist",
        "sqr_laser_max_dist", "use_max_scan_range", "laser_z_min", "laser_z_max", "laser_x", "laser_y", "laser_z",
        "laser_yaw")]


def hector_scan(laser, min_dist=0.4, max_dist=30.0, use_max=20.0, cutoff=30.0, z_min=-1.0, z_max=1.0,
                laser_pose=(0.0, 0.0, 0.0, 0.0)) -> HectorScan:
    """The hector_slam node's parameters (hector_slam.cc:40-75, 193) for a synth.Laser."""
    return HectorScan(laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max, cutoff,
                      min_dist * min_dist, max_dist * max_dist, use_max, z_min, z_max, *laser_pose)


class DeskewParams(C.Structure):
    _fields_ = [("angle_min", C.c_float), ("angle_increment", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float),
                ("scan_time_start", C.c_double), ("time_increment", C.c_double), ("use_imu", C.c_int32),
                ("use_odom", C.c_int32), ("start_odom_time", C.c_double), ("end_odom_time", C.c_double),
                ("odom_incre_x", C.c_float), ("odom_incre_y", C.c_float), ("odom_incre_z", C.c_float), ("pad", C.c_float)]


def deskew_scan(ctx, ranges_f32, params: DeskewParams, imu_time=None, imu_rot=None):
    """lesson5 CorrectLaserScan on the device -> (xyz [n,3] float32, valid [n] bool).  imu_rot: [n_imu, 3]."""
    r = np.ascontiguousarray(ranges_f32, dtype=np.float32)
    n_imu = 0 if imu_time is None else len(imu_time)
    it = np.ascontiguousarray(imu_time if n_imu else [0.0], dtype=np.float64)
    ir = np.ascontiguousarray(np.asarray(imu_rot if n_imu else [[0.0, 0.0, 0.0]], dtype=np.float64).T)
    xyz = np.zeros((len(r), 3), np.float32)
    valid = np.zeros(len(r), np.uint8)
    ctx.check(ctx.L.lslam_deskew_scan(ctx.h, r.ctypes.data, len(r), C.byref(params), it.ctypes.data, ir[0].ctypes.data,
                                      ir[1].ctypes.data, ir[2].ctypes.data, max(n_imu, 1) if params.use_imu else 0,
                                      xyz.ctypes.data, valid.ctypes.data))
    return xyz, valid.astype(bool)


def _deskew_inputs(params, imu_times, imu_rots):
    """Per-scan params and IMU samples -> (DeskewParams array, imu_first [n+1] int32, time [T], rot [3, T] float64).
    imu_times[k]: scan k's sample times (None or empty: no sample), imu_rots[k]: [n_k, 3]."""
    n = len(params)
    arr = (DeskewParams * max(n, 1))(*params)
    counts = [0 if (imu_times is None or imu_times[k] is None) else len(imu_times[k]) for k in range(n)]
    first = np.zeros(n + 1, np.int32)
    first[1:] = np.cumsum(counts)
    total = int(first[-1])
    it = np.zeros(max(total, 1), np.float64)
    ir = np.zeros((3, max(total, 1)), np.float64)
    for k in range(n):
        if counts[k]:
            it[first[k]:first[k + 1]] = np.asarray(imu_times[k], np.float64)
            ir[:, first[k]:first[k + 1]] = np.asarray(imu_rots[k], np.float64).reshape(counts[k], 3).T
    return arr, first, it, ir


class Deskewer:
    """lslam_deskew: lesson5's CorrectLaserScan for many scans of one geometry per launch.  Owns its device and pinned
    buffers and the cached angle table; every scan's output is bit for bit deskew_scan's."""

    def __init__(self, ctx: "Context"):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        ctx.check(self.L.lslam_deskew_create(ctx.h, C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_deskew_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def batch(self, ranges, params, imu_times=None, imu_rots=None, n_readings=None):
        """ranges: [n_scans, stride] float32 (n_readings <= stride beams of each row are the scan), params: a DeskewParams per
        scan -> (xyz [n_scans, n_readings, 3] float32, valid [n_scans, n_readings] bool)."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        r = r.reshape(len(params), -1) if len(params) else r.reshape(0, r.shape[-1] if r.ndim > 1 else 0)
        n, stride = r.shape
        nr = stride if n_readings is None else int(n_readings)
        arr, first, it, ir = _deskew_inputs(params, imu_times, imu_rots)
        xyz = np.zeros((n, nr, 3), np.float32)
        valid = np.zeros((n, nr), np.uint8)
        self.ctx.check(self.L.lslam_deskew_batch(self.h, n, nr, r.ctypes.data, stride, C.addressof(arr), first.ctypes.data,
                                                 it.ctypes.data, ir[0].ctypes.data, ir[1].ctypes.data, ir[2].ctypes.data,
                                                 xyz.ctypes.data, valid.ctypes.data))
        return xyz, valid.astype(bool)

    def batch_dev(self, n_readings: int, ranges_ptr: int, ranges_stride: int, params, imu_times, imu_rots, xyz_ptr: int,
                  valid_ptr: int):
        """The same with ranges, xyz (float32) and valid (uint8) in HBM: asynchronous on the context's stream, no host wait."""
        arr, first, it, ir = _deskew_inputs(params, imu_times, imu_rots)
        self.ctx.check(self.L.lslam_deskew_batch_dev(self.h, len(params), n_readings, ranges_ptr, ranges_stride, C.addressof(arr),
                                                     first.ctypes.data, it.ctypes.data, ir[0].ctypes.data, ir[1].ctypes.data,
                                                     ir[2].ctypes.data, xyz_ptr, valid_ptr))

    def stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self.ctx.check(self.L.lslam_deskew_stats(self.h, out))
        return dict(zip(("scans", "launches", "growths", "host_waits"), (int(v) for v in out)))


MSYNC_QUEUED, MSYNC_CORRECTED, MSYNC_WAIT_IMU, MSYNC_WAIT_ODOM, MSYNC_IMU_NO_LEAD_SAMPLE, MSYNC_IMU_OVERFLOW = 0, 1, -1, -2, -3, -4
MSYNC_QUEUE_LENGTH = 2000  # LSLAM_MSYNC_QUEUE_LENGTH
MSYNC_RECORD = np.dtype([("status", np.int32), ("n_imu", np.int32), ("scan_time_start", np.float64), ("time_increment", np.float64),
                         ("start_odom_time", np.float64), ("end_odom_time", np.float64), ("odom_incre", np.float32, (3,)),
                         ("pad", np.float32), ("imu_front", np.int64), ("odom_front", np.int64), ("start_odom_index", np.int64),
                         ("end_odom_index", np.int64)])  # lslam_msync_record


class MsyncLaser(C.Structure):
    _fields_ = [("angle_min", C.c_float), ("angle_increment", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float)]


class MotionSync:
    """lslam_msync: lesson5's node from its callbacks on -- IMU, odometry and LaserScan messages in, de-skewed clouds out.  The
    queues, their fronts, the sticky start / end odometry messages and the one queued scan live on the device; `deskewer` (a
    Deskewer of the same context, made here when None) runs the back half."""

    def __init__(self, ctx: "Context", use_imu: bool = True, use_odom: bool = True, deskewer: "Deskewer | None" = None):
        self.ctx, self.L = ctx, ctx.L
        self.deskewer = deskewer if deskewer is not None else Deskewer(ctx)
        h = C.c_void_p()
        ctx.check(self.L.lslam_msync_create(ctx.h, int(use_imu), int(use_odom), C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_msync_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx.check(self.L.lslam_msync_reset(self.h))

    def push_imu(self, stamps, gyro_xyz):
        """n ImuCallbacks: stamps [n], gyro_xyz [n, 3] (angular_velocity)."""
        t = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        w = np.ascontiguousarray(gyro_xyz, np.float64).reshape(len(t), 3)
        self.ctx.check(self.L.lslam_msync_push_imu(self.h, len(t), t.ctypes.data, w.ctypes.data))

    def push_odom(self, stamps, pos_xyz, quat_xyzw):
        """n OdomCallbacks: stamps [n], pos_xyz [n, 3], quat_xyzw [n, 4]."""
        t = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        p = np.ascontiguousarray(pos_xyz, np.float64).reshape(len(t), 3)
        q = np.ascontiguousarray(quat_xyzw, np.float64).reshape(len(t), 4)
        self.ctx.check(self.L.lslam_msync_push_odom(self.h, len(t), t.ctypes.data, p.ctypes.data, q.ctypes.data))

    @staticmethod
    def _small(laser, stamps, time_increments, imu_seen, odom_seen):
        hdr = laser if isinstance(laser, MsyncLaser) else MsyncLaser(*[float(v) for v in laser])
        t = np.ascontiguousarray(stamps, np.float64).reshape(-1)
        ti = np.ascontiguousarray(time_increments, np.float32).reshape(-1)
        if len(ti) != len(t):
            raise ValueError("one time_increment per scan message")
        seen = [None if a is None else np.ascontiguousarray(a, np.int64).reshape(len(t)) for a in (imu_seen, odom_seen)]
        return hdr, t, ti, seen

    def scans(self, laser, ranges, stamps, time_increments, imu_seen=None, odom_seen=None, n_readings=None):
        """n ScanCallbacks.  laser: (angle_min, angle_increment, range_min, range_max); ranges [n, stride] float32 ->
        (xyz [n, n_readings, 3] float32, valid [n, n_readings] bool, records [n] MSYNC_RECORD).  Row k is the cloud of message
        k - 1 (row 0: the scan the previous call left queued); rows of queued or refused callbacks are zeros."""
        hdr, t, ti, seen = self._small(laser, stamps, time_increments, imu_seen, odom_seen)
        n = len(t)
        r = np.ascontiguousarray(ranges, dtype=np.float32).reshape(n, -1) if n else np.zeros((0, 0), np.float32)
        stride = r.shape[1]
        nr = stride if n_readings is None else int(n_readings)
        xyz = np.zeros((n, nr, 3), np.float32)
        valid = np.zeros((n, nr), np.uint8)
        rec = np.zeros(n, MSYNC_RECORD)
        self.ctx.check(self.L.lslam_msync_scans(self.h, self.deskewer.h, C.byref(hdr), n, nr, r.ctypes.data, stride, t.ctypes.data,
                                                ti.ctypes.data, None if seen[0] is None else seen[0].ctypes.data,
                                                None if seen[1] is None else seen[1].ctypes.data, xyz.ctypes.data,
                                                valid.ctypes.data, rec.ctypes.data))
        return xyz, valid.astype(bool), rec

    def scans_dev(self, laser, n_readings: int, ranges_ptr: int, ranges_stride: int, stamps, time_increments, xyz_ptr: int,
                  valid_ptr: int, records_ptr=None, imu_seen=None, odom_seen=None):
        """The same with ranges, xyz (float32), valid (uint8) and records (MSYNC_RECORD, may be None) in HBM: asynchronous on
        the context's stream, no host wait."""
        hdr, t, ti, seen = self._small(laser, stamps, time_increments, imu_seen, odom_seen)
        self.ctx.check(self.L.lslam_msync_scans_dev(self.h, self.deskewer.h, C.byref(hdr), len(t), n_readings, ranges_ptr,
                                                    ranges_stride, t.ctypes.data, ti.ctypes.data,
                                                    None if seen[0] is None else seen[0].ctypes.data,
                                                    None if seen[1] is None else seen[1].ctypes.data, xyz_ptr, valid_ptr,
                                                    records_ptr))

    def read_windows(self, n_msgs: int):
        """The last call's integrated IMU samples -> (imu_first [n_msgs + 1], imu_time [T], imu_rot [T, 3]).  Waits."""
        first = np.zeros(n_msgs + 1, np.int32)
        self.ctx.check(self.L.lslam_msync_read_windows(self.h, first.ctypes.data, None, None, 0))
        total = int(first[-1])
        t, rot = np.zeros(max(total, 1), np.float64), np.zeros((max(total, 1), 3), np.float64)
        if total:
            self.ctx.check(self.L.lslam_msync_read_windows(self.h, first.ctypes.data, t.ctypes.data, rot.ctypes.data, total))
        return first, t[:total], rot[:total]

    def stats(self) -> dict:
        out = (C.c_int64 * 6)()
        self.ctx.check(self.L.lslam_msync_stats(self.h, out))
        return dict(zip(("callbacks", "corrected", "refused", "launches", "growths", "host_waits"), (int(v) for v in out)))


FEATURE_SECTORS, FEATURE_PICKS, FEATURE_MAX_READINGS = 6, 20, 1500  # LSLAM_FEATURE_*
FEATURE_RECORD = np.dtype([("n_valid", np.int32), ("n_corners", np.int32), ("per_sector", np.int32, (6,))])  # lslam_feature_record


class FeatureExtractor:
    """lslam_features: lesson1's LaserScan::ScanCallback (curvature corners: the 20 sharpest points of each sixth of a scan)
    for many scans per launch.  Among equal curvatures the higher compacted index ranks first."""

    def __init__(self, ctx: "Context", edge_threshold: float = 1.0):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        ctx.check(self.L.lslam_features_create(ctx.h, C.byref(h)))
        self.h = h
        ctx._adopt(self)
        self.set_threshold(edge_threshold)

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_features_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def set_threshold(self, edge_threshold: float):
        self.ctx.check(self.L.lslam_features_set_threshold(self.h, float(edge_threshold)))

    def extract(self, ranges, n_readings=None, want_image=True, want_curvature=True):
        """ranges: [n_scans, stride] float32 (the first n_readings <= stride beams of each row are the scan) ->
        (image [n_scans, n_readings] float32, index [n_scans, 6, 20] int32 of ORIGINAL beam indices (-1 = unused),
        records FEATURE_RECORD[n_scans], curvature [n_scans, n_readings] float32); image / curvature are None when not
        wanted."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        if r.ndim != 2:
            raise ValueError("ranges must be [n_scans, stride]")
        n, stride = r.shape
        nr = stride if n_readings is None else int(n_readings)
        image = np.zeros((n, max(nr, 0)), np.float32) if want_image else None
        curv = np.zeros((n, max(nr, 0)), np.float32) if want_curvature else None
        index = np.full((n, FEATURE_SECTORS, FEATURE_PICKS), -1, np.int32)
        rec = np.zeros(n, FEATURE_RECORD)
        self.ctx.check(self.L.lslam_features_batch(self.h, n, nr, r.ctypes.data, stride,
                                                   image.ctypes.data if want_image else None, index.ctypes.data,
                                                   rec.ctypes.data, curv.ctypes.data if want_curvature else None))
        return image, index, rec, curv

    def extract_dev(self, n_scans: int, n_readings: int, ranges_ptr: int, ranges_stride: int, image_ptr, index_ptr: int,
                    records_ptr: int, curvature_ptr):
        """The same with ranges and every output in HBM (image_ptr / curvature_ptr may be None): asynchronous on the
        context's stream, no host wait."""
        self.ctx.check(self.L.lslam_features_batch_dev(self.h, n_scans, n_readings, ranges_ptr, ranges_stride, image_ptr,
                                                       index_ptr, records_ptr, curvature_ptr))

    def stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self.ctx.check(self.L.lslam_features_stats(self.h, out))
        return dict(zip(("scans", "launches", "growths", "host_waits"), (int(v) for v in out)))


PLICP_MAX_READINGS = 2048  # LSLAM_PLICP_MAX_READINGS
PLICP_RECORD = np.dtype([("x", "f8", 3), ("error", "f8"), ("valid", "i4"), ("iterations", "i4"), ("nvalid", "i4"),
                         ("reserved", "i4")])  # lslam_plicp_record
PLICP_ODOM_RECORD = np.dtype([("x", "f8", 3), ("error", "f8"), ("valid", "i4"), ("iterations", "i4"), ("nvalid", "i4"),
                              ("flags", "i4"), ("base_in_odom", "f8", 3), ("reserved", "f8")])  # lslam_plicp_odom_record
PLICP_ODOM_TRACK = np.dtype([("base_in_odom", "f8", 3), ("keyframe", "f8", 3), ("velocity", "f8", 2), ("last_icp_time", "f8"),
                             ("scan_count", "i4"), ("initialized", "i4")])  # lslam_plicp_odom_track
assert (PLICP_RECORD.itemsize, PLICP_ODOM_RECORD.itemsize, PLICP_ODOM_TRACK.itemsize) == (48, 80, 80)


class PlicpParams(C.Structure):
    """lslam_plicp_params: the sm_params sm_icp reads (scan_match_plicp.cc:43-156)."""

    _fields_ = [(k, C.c_double) for k in (
        "max_angular_correction_deg", "max_linear_correction", "epsilon_xy", "epsilon_theta", "max_correspondence_dist",
        "outliers_maxPerc", "outliers_adaptive_order", "outliers_adaptive_mult")] + [(k, C.c_int32) for k in (
            "max_iterations", "use_point_to_line_distance", "outliers_remove_doubles", "reserved")]


def plicp_params(**kw) -> PlicpParams:
    """Library defaults (lslam_plicp_params_defaults) with keyword overrides."""
    p = PlicpParams()
    lib().lslam_plicp_params_defaults(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class PlicpMatcher:
    """lslam_plicp: lesson3's ScanMatchWithPLICP for many scan pairs per launch.  Parity with the reference is unpinned (its
    arithmetic is the un-vendored csm): the results are defined by tools/plicp_cpu.py's sm_icp.  Equal distances rank by sens
    order."""

    def __init__(self, ctx: "Context", params: PlicpParams | None = None, laser=None):
        self.ctx, self.L = ctx, ctx.L
        self.params = params if params is not None else plicp_params()
        h = C.c_void_p()
        ctx.check(self.L.lslam_plicp_create(ctx.h, C.byref(self.params), C.byref(h)))
        self.h = h
        ctx._adopt(self)
        if laser is not None:
            self.set_laser(laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max)

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_plicp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def set_laser(self, angle_min: float, angle_increment: float, range_min: float, range_max: float):
        self.ctx.check(self.L.lslam_plicp_set_laser(self.h, float(angle_min), float(angle_increment), float(range_min),
                                                    float(range_max)))

    def match_batch(self, ranges, pair_ref, pair_sens, first_guess=None, n_readings=None, out=None):
        """ranges: [n_scans, stride] float32; pair b matches scan pair_sens[b] against scan pair_ref[b]; first_guess:
        [n_pairs, 3] float64 or None (zeros) -> PLICP_RECORD[n_pairs]."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        if r.ndim != 2:
            raise ValueError("ranges must be [n_scans, stride]")
        n, stride = r.shape
        nr = stride if n_readings is None else int(n_readings)
        pr = np.ascontiguousarray(pair_ref, dtype=np.int32)
        ps = np.ascontiguousarray(pair_sens, dtype=np.int32)
        if pr.shape != ps.shape or pr.ndim != 1:
            raise ValueError("pair_ref and pair_sens must be two [n_pairs] arrays")
        g = None if first_guess is None else _f64(first_guess).reshape(len(pr), 3)
        rec = np.zeros(len(pr), PLICP_RECORD) if out is None else out
        self.ctx.check(self.L.lslam_plicp_match_batch(self.h, n, nr, r.ctypes.data, stride, len(pr), pr.ctypes.data, ps.ctypes.data,
                                                      None if g is None else g.ctypes.data, rec.ctypes.data))
        return rec

    def match_consecutive(self, ranges, n_readings=None):
        """Every scan against the one before it: PLICP_RECORD[n_scans - 1], record k = scan k + 1 in scan k's frame."""
        n = len(ranges)
        idx = np.arange(max(n - 1, 0), dtype=np.int32)
        return self.match_batch(ranges, idx, idx + 1, None, n_readings)

    def match_batch_dev(self, n_scans: int, n_readings: int, ranges_ptr: int, ranges_stride: int, pair_ref, pair_sens,
                        first_guess_ptr, records_ptr: int):
        """The same with ranges, first guesses (may be None) and records in HBM: asynchronous on the context's stream, no host
        wait.  The pair indices are host arrays."""
        pr = np.ascontiguousarray(pair_ref, dtype=np.int32)
        ps = np.ascontiguousarray(pair_sens, dtype=np.int32)
        self.ctx.check(self.L.lslam_plicp_match_batch_dev(self.h, n_scans, n_readings, ranges_ptr, ranges_stride, len(pr),
                                                          pr.ctypes.data, ps.ctypes.data, first_guess_ptr, records_ptr))

    def debug_iteration(self, ranges_ref, ranges_sens, x_in=(0.0, 0.0, 0.0)):
        """One iteration from x_in -> (j1, j2 int32 [n] reading indices or -1, flags uint8 [n], x_out [3], NaN at an early
        exit).  Flags: 1 valid reading, 2 accepted before outlier rejection, 4 kept after it."""
        a = np.ascontiguousarray(ranges_ref, dtype=np.float32)
        b = np.ascontiguousarray(ranges_sens, dtype=np.float32)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError("two scans of one length")
        n = len(a)
        j1, j2 = np.full(n, -2, np.int32), np.full(n, -2, np.int32)
        flags = np.zeros(n, np.uint8)
        x = _f64(x_in)
        x_out = np.zeros(3)
        self.ctx.check(self.L.lslam_plicp_debug_iteration(self.h, a.ctypes.data, b.ctypes.data, n, x.ctypes.data, j1.ctypes.data,
                                                          j2.ctypes.data, flags.ctypes.data, x_out.ctypes.data))
        return j1, j2, flags, x_out

    def match_clouds(self, xyz, pair_ref, pair_sens, valid=None, first_guess=None, out=None):
        """xyz: [n_clouds, n, 3] float32 clouds in the de-skew's layout (Deskewer.batch, MotionSync.scans, IcpMatcher.convert),
        valid: [n_clouds, n] uint8 or None (every point) -> PLICP_RECORD[n_pairs].  No laser is needed: a point takes part iff
        its valid byte is set and x, y are finite; its reading index is its position in the cloud."""
        c = np.ascontiguousarray(xyz, dtype=np.float32)
        if c.ndim != 3 or c.shape[2] != 3:
            raise ValueError("xyz must be [n_clouds, n, 3]")
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8).reshape(c.shape[0], c.shape[1])
        pr = np.ascontiguousarray(pair_ref, dtype=np.int32)
        ps = np.ascontiguousarray(pair_sens, dtype=np.int32)
        if pr.shape != ps.shape or pr.ndim != 1:
            raise ValueError("pair_ref and pair_sens must be two [n_pairs] arrays")
        g = None if first_guess is None else _f64(first_guess).reshape(len(pr), 3)
        rec = np.zeros(len(pr), PLICP_RECORD) if out is None else out
        self.ctx.check(self.L.lslam_plicp_match_clouds(self.h, c.shape[0], c.shape[1], c.ctypes.data,
                                                       None if v is None else v.ctypes.data, len(pr), pr.ctypes.data, ps.ctypes.data,
                                                       None if g is None else g.ctypes.data, rec.ctypes.data))
        return rec

    def match_clouds_dev(self, n_clouds: int, n_points: int, xyz_ptr: int, valid_ptr, pair_ref, pair_sens, first_guess_ptr,
                         records_ptr: int):
        """The same with clouds, valid bytes (may be None), first guesses (may be None) and records in HBM: asynchronous on the
        context's stream, no host wait.  The pair indices are host arrays."""
        pr = np.ascontiguousarray(pair_ref, dtype=np.int32)
        ps = np.ascontiguousarray(pair_sens, dtype=np.int32)
        self.ctx.check(self.L.lslam_plicp_match_clouds_dev(self.h, n_clouds, n_points, xyz_ptr, valid_ptr, len(pr), pr.ctypes.data,
                                                           ps.ctypes.data, first_guess_ptr, records_ptr))

    def debug_iteration_clouds(self, ref_xyz, sens_xyz, x_in=(0.0, 0.0, 0.0), ref_valid=None, sens_valid=None):
        """debug_iteration on two [n, 3] clouds (valid bytes or None): j1, j2, flags per point of the sens cloud."""
        a = np.ascontiguousarray(ref_xyz, dtype=np.float32)
        b = np.ascontiguousarray(sens_xyz, dtype=np.float32)
        if a.shape != b.shape or a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("two [n, 3] clouds of one length")
        n = len(a)
        rv = None if ref_valid is None else np.ascontiguousarray(ref_valid, dtype=np.uint8).reshape(n)
        sv = None if sens_valid is None else np.ascontiguousarray(sens_valid, dtype=np.uint8).reshape(n)
        j1, j2 = np.full(n, -2, np.int32), np.full(n, -2, np.int32)
        flags = np.zeros(n, np.uint8)
        x = _f64(x_in)
        x_out = np.zeros(3)
        self.ctx.check(self.L.lslam_plicp_debug_iteration_clouds(
            self.h, a.ctypes.data, b.ctypes.data, None if rv is None else rv.ctypes.data, None if sv is None else sv.ctypes.data, n,
            x.ctypes.data, j1.ctypes.data, j2.ctypes.data, flags.ctypes.data, x_out.ctypes.data))
        return j1, j2, flags, x_out

    def stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self.ctx.check(self.L.lslam_plicp_stats(self.h, out))
        return dict(zip(("pairs", "launches", "growths", "host_waits"), (int(v) for v in out)))


ICP_MAX_POINTS = 2048  # LSLAM_ICP_MAX_POINTS
ICP_RECORD = np.dtype([("x", "f8", 3), ("fitness", "f8"), ("mse", "f8"), ("converged", "i4"), ("iterations", "i4"),
                       ("ncorr", "i4"), ("state", "i4"), ("reserved", "f8")])  # lslam_icp_record
assert ICP_RECORD.itemsize == 64


class IcpParams(C.Structure):
    """lslam_icp_params: what a default-configured pcl::IterativeClosestPoint reads (scan_match_icp.cc:135-164)."""

    _fields_ = [(k, C.c_double) for k in (
        "max_correspondence_distance", "transformation_epsilon", "euclidean_fitness_epsilon", "absolute_mse")] + [
            (k, C.c_int32) for k in ("max_iterations", "skip_invalid", "invalid_as_nan", "reserved")]


def icp_params(**kw) -> IcpParams:
    """Library defaults (lslam_icp_params_defaults) with keyword overrides."""
    p = IcpParams()
    lib().lslam_icp_params_defaults(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class IcpMatcher:
    """lslam_icp: lesson2's ConvertScan2PointCloud and ScanMatchWithICP for many scan pairs per launch.  Parity with the
    reference is unpinned (its arithmetic is PCL's): the results are defined by tools/icp_cpu.py's icp.  Among equal distances
    the lowest target index wins."""

    def __init__(self, ctx: "Context", params: IcpParams | None = None, laser=None):
        self.ctx, self.L = ctx, ctx.L
        self.params = params if params is not None else icp_params()
        h = C.c_void_p()
        ctx.check(self.L.lslam_icp_create(ctx.h, C.byref(self.params), C.byref(h)))
        self.h = h
        ctx._adopt(self)
        if laser is not None:
            self.set_laser(laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max)

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_icp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def set_laser(self, angle_min: float, angle_increment: float, range_min: float, range_max: float):
        self.ctx.check(self.L.lslam_icp_set_laser(self.h, float(angle_min), float(angle_increment), float(range_min),
                                                  float(range_max)))

    @staticmethod
    def _ranges(ranges, n_readings):
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        if r.ndim != 2:
            raise ValueError("ranges must be [n_scans, stride]")
        return r, r.shape[0], r.shape[1], (r.shape[1] if n_readings is None else int(n_readings))

    @staticmethod
    def _pairs(pair_source, pair_target, first_guess):
        ps = np.ascontiguousarray(pair_source, dtype=np.int32)
        pt = np.ascontiguousarray(pair_target, dtype=np.int32)
        if ps.shape != pt.shape or ps.ndim != 1:
            raise ValueError("pair_source and pair_target must be two [n_pairs] arrays")
        g = None if first_guess is None else _f64(first_guess).reshape(len(ps), 3)
        return ps, pt, g

    def convert(self, ranges, n_readings=None):
        """ranges: [n_scans, stride] float32 -> (xyz float32 [n_scans, n, 3], valid uint8 [n_scans, n])."""
        r, n, stride, nr = self._ranges(ranges, n_readings)
        xyz, valid = np.zeros((n, nr, 3), np.float32), np.zeros((n, nr), np.uint8)
        self.ctx.check(self.L.lslam_icp_convert_batch(self.h, n, nr, r.ctypes.data, stride, xyz.ctypes.data, valid.ctypes.data))
        return xyz, valid

    def convert_dev(self, n_scans: int, n_readings: int, ranges_ptr: int, ranges_stride: int, xyz_ptr: int, valid_ptr: int):
        self.ctx.check(self.L.lslam_icp_convert_batch_dev(self.h, n_scans, n_readings, ranges_ptr, ranges_stride, xyz_ptr, valid_ptr))

    def match_batch(self, ranges, pair_source, pair_target, first_guess=None, n_readings=None, out=None):
        """ranges: [n_scans, stride] float32; pair b aligns scan pair_source[b]'s cloud to scan pair_target[b]'s; first_guess:
        [n_pairs, 3] float64 (x, y, yaw) or None (zeros) -> ICP_RECORD[n_pairs]."""
        r, n, stride, nr = self._ranges(ranges, n_readings)
        ps, pt, g = self._pairs(pair_source, pair_target, first_guess)
        rec = np.zeros(len(ps), ICP_RECORD) if out is None else out
        self.ctx.check(self.L.lslam_icp_match_batch(self.h, n, nr, r.ctypes.data, stride, len(ps), ps.ctypes.data, pt.ctypes.data,
                                                    None if g is None else g.ctypes.data, rec.ctypes.data))
        return rec

    def match_batch_dev(self, n_scans: int, n_readings: int, ranges_ptr: int, ranges_stride: int, pair_source, pair_target,
                        first_guess_ptr, records_ptr: int):
        """The same with ranges, first guesses (may be None) and records in HBM: asynchronous on the context's stream, no host
        wait.  The pair indices are host arrays."""
        ps, pt, _ = self._pairs(pair_source, pair_target, None)
        self.ctx.check(self.L.lslam_icp_match_batch_dev(self.h, n_scans, n_readings, ranges_ptr, ranges_stride, len(ps),
                                                        ps.ctypes.data, pt.ctypes.data, first_guess_ptr, records_ptr))

    def match_clouds(self, xyz, pair_source, pair_target, valid=None, first_guess=None, out=None):
        """xyz: [n_clouds, n, 3] float32, valid: [n_clouds, n] uint8 or None (read only with skip_invalid) -> ICP_RECORD[n_pairs]."""
        c = np.ascontiguousarray(xyz, dtype=np.float32)
        if c.ndim != 3 or c.shape[2] != 3:
            raise ValueError("xyz must be [n_clouds, n, 3]")
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8).reshape(c.shape[0], c.shape[1])
        ps, pt, g = self._pairs(pair_source, pair_target, first_guess)
        rec = np.zeros(len(ps), ICP_RECORD) if out is None else out
        self.ctx.check(self.L.lslam_icp_match_clouds(self.h, c.shape[0], c.shape[1], c.ctypes.data, None if v is None else v.ctypes.data,
                                                     len(ps), ps.ctypes.data, pt.ctypes.data, None if g is None else g.ctypes.data,
                                                     rec.ctypes.data))
        return rec

    def match_clouds_dev(self, n_clouds: int, n_points: int, xyz_ptr: int, valid_ptr, pair_source, pair_target, first_guess_ptr,
                         records_ptr: int):
        ps, pt, _ = self._pairs(pair_source, pair_target, None)
        self.ctx.check(self.L.lslam_icp_match_clouds_dev(self.h, n_clouds, n_points, xyz_ptr, valid_ptr, len(ps), ps.ctypes.data,
                                                         pt.ctypes.data, first_guess_ptr, records_ptr))

    def debug_iteration(self, src_xyz, tgt_xyz, x_in=(0.0, 0.0, 0.0), src_valid=None, tgt_valid=None):
        """One iteration from x_in -> (corr int32 [n] (-1: rejected or masked), d2 float64 [n], inc [3] = (tx, ty, theta), NaN
        where fewer than 3 were accepted, mse, ncorr)."""
        a = np.ascontiguousarray(src_xyz, dtype=np.float32)
        b = np.ascontiguousarray(tgt_xyz, dtype=np.float32)
        if a.shape != b.shape or a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("two [n, 3] clouds of one length")
        n = len(a)
        sv = None if src_valid is None else np.ascontiguousarray(src_valid, dtype=np.uint8).reshape(n)
        tv = None if tgt_valid is None else np.ascontiguousarray(tgt_valid, dtype=np.uint8).reshape(n)
        corr, d2, inc = np.full(n, -2, np.int32), np.zeros(n), np.zeros(3)
        x, mse, ncorr = _f64(x_in), C.c_double(0.0), C.c_int32(0)
        self.ctx.check(self.L.lslam_icp_debug_iteration(self.h, a.ctypes.data, b.ctypes.data, None if sv is None else sv.ctypes.data,
                                                        None if tv is None else tv.ctypes.data, n, x.ctypes.data, corr.ctypes.data,
                                                        d2.ctypes.data, inc.ctypes.data, C.byref(mse), C.byref(ncorr)))
        return corr, d2, inc, mse.value, ncorr.value

    def stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self.ctx.check(self.L.lslam_icp_stats(self.h, out))
        return dict(zip(("pairs", "launches", "growths", "host_waits"), (int(v) for v in out)))


class PlicpOdometry:
    """lslam_plicp_odom: plicp_odometry.cc's node (keyframe scan matching, constant-velocity first guess) for n_tracks
    independent tracks, one launch and one host wait per call.  An invalid match leaves the pose untouched (corr_ch = identity);
    the prediction is the reference's, literally: linear.x only, nothing for a negative speed."""

    def __init__(self, ctx: "Context", n_tracks: int = 1, params: PlicpParams | None = None, kf_dist_linear: float = 0.1,
                 kf_dist_angular: float = 5.0 * (math.pi / 180.0), kf_scan_count: int = 10, base_to_laser=(0.0, 0.0, 0.0),
                 laser=None):
        self.ctx, self.L = ctx, ctx.L
        self.params = params if params is not None else plicp_params()
        self.n_tracks = int(n_tracks)
        b2l = _f64(base_to_laser)
        h = C.c_void_p()
        ctx.check(self.L.lslam_plicp_odom_create(ctx.h, C.byref(self.params), self.n_tracks, float(kf_dist_linear),
                                                 float(kf_dist_angular), int(kf_scan_count), b2l.ctypes.data, C.byref(h)))
        self.h = h
        ctx._adopt(self)
        if laser is not None:
            self.set_laser(laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max)

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_plicp_odom_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def set_laser(self, angle_min: float, angle_increment: float, range_min: float, range_max: float):
        self.ctx.check(self.L.lslam_plicp_odom_set_laser(self.h, float(angle_min), float(angle_increment), float(range_min),
                                                         float(range_max)))

    def reset(self):
        self.ctx.check(self.L.lslam_plicp_odom_reset(self.h))

    def process_many(self, ranges, stamps, active=None, n_readings=None):
        """ranges: [n_steps, n_tracks, stride] float32, stamps: [n_steps, n_tracks] seconds, active: [n_steps, n_tracks] or None
        -> PLICP_ODOM_RECORD[n_steps, n_tracks]."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        if r.ndim == 2 and self.n_tracks == 1:
            r = r[:, None, :]
        if r.ndim != 3 or r.shape[1] != self.n_tracks:
            raise ValueError("ranges must be [n_steps, n_tracks, stride]")
        steps, _, stride = r.shape
        nr = stride if n_readings is None else int(n_readings)
        st = _f64(stamps).reshape(steps, self.n_tracks)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8).reshape(steps, self.n_tracks)
        rec = np.zeros((steps, self.n_tracks), PLICP_ODOM_RECORD)
        self.ctx.check(self.L.lslam_plicp_odom_process_many(self.h, steps, nr, r.ctypes.data, stride, st.ctypes.data,
                                                            None if act is None else act.ctypes.data, rec.ctypes.data))
        return rec

    def process_many_clouds(self, xyz, stamps, valid=None, take=None, active=None):
        """xyz: [n_steps, n_tracks, n_points, 3] float32 clouds in the de-skew's layout, stamps [n_steps, n_tracks] seconds, valid
        [n_steps, n_tracks, n_points] or None = every point, take / active [n_steps, n_tracks] or None = every scan ->
        PLICP_ODOM_RECORD[n_steps, n_tracks].  An entry is taken iff it is active and its take flag is set; one that is not
        changes nothing of its track (record: zero with iterations = -1).  No laser is needed.  Between resets a handle runs
        either range calls or cloud calls, with one n_points."""
        R = self.n_tracks
        x = np.ascontiguousarray(xyz, dtype=np.float32)
        if x.ndim == 3 and R == 1:
            x = x[:, None]
        if x.ndim != 4 or x.shape[1] != R or x.shape[3] != 3:
            raise ValueError("xyz must be [n_steps, n_tracks, n_points, 3]")
        steps, npts = x.shape[0], x.shape[2]
        st = _f64(stamps).reshape(steps, R)
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid).astype(bool).astype(np.uint8)).reshape(steps, R, npts)
        t = None if take is None else np.ascontiguousarray(np.asarray(take).astype(bool).astype(np.uint8)).reshape(steps, R)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8).reshape(steps, R)
        rec = np.zeros((steps, R), PLICP_ODOM_RECORD)
        self.ctx.check(self.L.lslam_plicp_odom_process_many_clouds(
            self.h, steps, npts, x.ctypes.data, None if v is None else v.ctypes.data, None if t is None else t.ctypes.data,
            st.ctypes.data, None if act is None else act.ctypes.data, rec.ctypes.data))
        return rec

    def process_many_clouds_dev(self, n_steps: int, n_points: int, xyz_ptrs, valid_ptrs, take_ptrs, take_stride: int, stamps,
                                active=None):
        """The same on clouds in HBM.  xyz_ptrs / valid_ptrs / take_ptrs: n_tracks device addresses each, one block per track (R
        MotionSync.scans_dev outputs, or slices of one block); track m's row of step k is k rows into its block.  valid_ptrs,
        take_ptrs or single entries of them may be None (every point valid / every scan taken).  take words are int32, taken
        iff > 0, take_stride words apart: the `status` field of an MSYNC_RECORD array with MSYNC_RECORD.itemsize // 4.  stamps
        and active are host arrays; only they go up."""
        R = self.n_tracks

        def table(ptrs):
            if ptrs is None:
                return None
            assert len(ptrs) == R, "one device pointer per track"
            return (C.c_void_p * R)(*[p or None for p in ptrs])

        x, v, t = table(xyz_ptrs), table(valid_ptrs), table(take_ptrs)
        st = _f64(stamps).reshape(int(n_steps), R)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8).reshape(int(n_steps), R)
        rec = np.zeros((int(n_steps), R), PLICP_ODOM_RECORD)
        self.ctx.check(self.L.lslam_plicp_odom_process_many_clouds_dev(
            self.h, int(n_steps), int(n_points), x, v, t, int(take_stride), st.ctypes.data,
            None if act is None else act.ctypes.data, rec.ctypes.data))
        return rec

    def state(self) -> np.ndarray:
        out = np.zeros(self.n_tracks, PLICP_ODOM_TRACK)
        self.ctx.check(self.L.lslam_plicp_odom_state(self.h, out.ctypes.data))
        return out

    def stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self.ctx.check(self.L.lslam_plicp_odom_stats(self.h, out))
        return dict(zip(("scans", "launches", "growths", "host_waits"), (int(v) for v in out)))


class GMapGeometry(C.Structure):
    _fields_ = [("map_size_x", C.c_int32), ("map_size_y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("size_x2", C.c_int32), ("size_y2", C.c_int32), ("patches_x", C.c_int32), ("patches_y", C.c_int32),
                ("center_x", C.c_double), ("center_y", C.c_double), ("delta", C.c_double)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int64), ("total_ms", C.c_double)]


def baseline_config(**kw) -> MatcherConfig:
    """BASELINE.json cfg 3/4: 0.05 m cells, +-0.5 m / +-20 deg window, 2005x2005 grid."""
    d = dict(
        search_size=1.0,
        resolution=0.05,
        smear_deviation=0.03,
        range_threshold=49.5,
        coarse_search_angle_offset=0.349,
        coarse_angle_resolution=0.0349,
        fine_search_angle_offset=0.00349,
        distance_variance_penalty=0.3 * 0.3,
        angle_variance_penalty=math.radians(20.0) ** 2,
        minimum_distance_penalty=0.5,
        minimum_angle_penalty=0.9,
        use_response_expansion=0,
        reserved=0,
    )
    d.update(kw)
    return MatcherConfig(**d)


def laser_params(laser, range_threshold: float = 49.5, offset=(0.0, 0.0, 0.0)) -> LaserParams:
    """From a synth.Laser (LaserScan header fields, karto_slam.cc:384-395)."""
    return LaserParams(laser.angle_min, laser.angle_max, laser.angle_increment, laser.range_min,
                       laser.range_max, range_threshold, *offset)


_LIB = None


def lib() -> C.CDLL:
    """Load (building if needed) liblslam_gpu.so and declare the prototypes."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # LSLAM_GPU_LIB: developer override naming a prebuilt variant of the library (kernel A/B runs,
    # tools/ab_variants.py); it is still the HIP library -- there is no CPU fallback behind it
    path = os.environ.get("LSLAM_GPU_LIB") or _build.build_library()
    L = C.CDLL(str(path))
    vp, i32, dbl = C.c_void_p, C.c_int, C.c_double
    L.lslam_abi_version.restype = i32
    L.lslam_create.argtypes = [i32, C.POINTER(vp)]
    L.lslam_destroy.argtypes = [vp]
    L.lslam_last_error.restype = C.c_char_p
    L.lslam_last_error.argtypes = [vp]
    L.lslam_synchronize.argtypes = [vp]
    L.lslam_stream.restype = vp
    L.lslam_stream.argtypes = [vp]
    L.lslam_dev_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.lslam_dev_free.argtypes = [vp, vp]
    L.lslam_dev_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.lslam_dev_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.lslam_profile_enable.argtypes = [vp, i32]
    L.lslam_profile_only.argtypes = [vp, C.c_char_p]
    L.lslam_profile_reset.argtypes = [vp]
    L.lslam_profile_read.argtypes = [vp, vp, i32]
    L.lslam_matcher_config_defaults.argtypes = [C.POINTER(MatcherConfig)]
    L.lslam_matcher_config_defaults.restype = None
    L.lslam_matcher_create.argtypes = [vp, C.POINTER(MatcherConfig), C.POINTER(LaserParams), C.POINTER(vp)]
    L.lslam_debug_reduce_lds_bytes.argtypes = [C.POINTER(MatcherConfig), i32, C.POINTER(i32 * 3)]
    L.lslam_debug_reduce_lds_bytes.restype = i32
    L.lslam_matcher_destroy.argtypes = [vp]
    L.lslam_matcher_destroy.restype = None
    L.lslam_matcher_num_beams.argtypes = [vp]
    L.lslam_matcher_grid_info.argtypes = [vp, vp, vp]
    L.lslam_matcher_get_grid_u8.argtypes = [vp, vp]
    L.lslam_matcher_get_kernel_u8.argtypes = [vp, vp]
    L.lslam_matcher_set_grid_u8.argtypes = [vp, vp, vp]
    L.lslam_matcher_set_grid_u8_dev.argtypes = [vp, vp, vp]
    L.lslam_matcher_grid_dev_ptr.restype = vp
    L.lslam_matcher_grid_dev_ptr.argtypes = [vp]
    L.lslam_sensor_pose_from_robot.argtypes = [C.POINTER(LaserParams), vp, vp]
    L.lslam_sensor_pose_from_robot.restype = None
    L.lslam_robot_pose_from_sensor.argtypes = [C.POINTER(LaserParams), vp, vp]
    L.lslam_robot_pose_from_sensor.restype = None
    L.lslam_matcher_set_base_scans.argtypes = [vp, i32, vp, i32, vp, vp]
    L.lslam_matcher_match_scan.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, i32, vp]
    L.lslam_matcher_match_batch.argtypes = [vp, i32, vp, i32, vp, i32, i32, vp]
    L.lslam_matcher_match_batch_dev_f32.argtypes = [vp, i32, vp, i32, vp, i32, i32, vp]
    L.lslam_matcher_match_batch_dev_f64.argtypes = [vp, i32, vp, i32, vp, i32, i32, vp]
    L.lslam_matcher_debug_lookup_table.argtypes = [vp, vp, vp, dbl, dbl, dbl, vp, C.POINTER(i32)]
    L.lslam_matcher_debug_coarse_sums.argtypes = [vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32),
                                                  C.POINTER(i32), i32]
    L.lslam_matcher_debug_coarse_sums_batch.argtypes = [vp, i32, vp, i32, vp, vp]
    L.lslam_matcher_debug_fine_sums_batch.argtypes = [vp, i32, vp, i32, vp, vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.lslam_matcher_debug_valid_mask.argtypes = [vp, vp, vp, vp, vp]
    L.lslam_frontend_create.argtypes = [vp, i32, dbl, dbl, dbl, C.POINTER(vp)]
    L.lslam_frontend_destroy.argtypes = [vp]
    L.lslam_frontend_destroy.restype = None
    L.lslam_frontend_reset.argtypes = [vp]
    L.lslam_frontend_process.argtypes = [vp, vp, i32, vp, C.POINTER(i32), vp, vp, C.POINTER(dbl)]
    L.lslam_frontend_running_scans.argtypes = [vp]
    L.lslam_frontend_config_defaults.argtypes = [C.POINTER(FrontEndConfig)]
    L.lslam_frontend_config_defaults.restype = None
    L.lslam_frontend_create_ex.argtypes = [vp, C.POINTER(FrontEndConfig), C.POINTER(vp)]
    L.lslam_frontend_process_stamped.argtypes = [vp, vp, i32, vp, dbl, C.POINTER(i32), vp, vp, C.POINTER(dbl)]
    L.lslam_frontend_num_scans.argtypes = [vp]
    L.lslam_frontend_scan_pose.argtypes = [vp, i32, vp]
    L.lslam_frontend_stats.argtypes = [vp, vp]
    L.lslam_frontend_process_many.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.lslam_frontend_lookahead_stats.argtypes = [vp, vp]
    L.lslam_frontend_spec_chain_stats.argtypes = [vp, vp]
    L.lslam_debug_frontend_anchor_row.argtypes = [vp, C.c_int, vp]
    L.lslam_occgrid_create_from_scans.argtypes = [vp, C.POINTER(LaserParams), i32, vp, i32, vp, dbl, C.POINTER(vp)]
    L.lslam_occgrid_destroy.argtypes = [vp]
    L.lslam_occgrid_destroy.restype = None
    L.lslam_occgrid_info.argtypes = [vp, vp, vp, C.POINTER(dbl)]
    L.lslam_occgrid_read_u8.argtypes = [vp, vp]
    L.lslam_occgrid_read_ros_i8.argtypes = [vp, vp]
    L.lslam_occgrid_scan_bounds.argtypes = [vp, C.POINTER(LaserParams), i32, vp, i32, vp, vp]
    L.lslam_occgrid_create_partial.argtypes = [vp, C.POINTER(LaserParams), i32, vp, i32, vp, dbl, vp, C.POINTER(vp)]
    L.lslam_occgrid_counter_words.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.lslam_occgrid_export_counters.argtypes = [vp, vp, i32]
    L.lslam_occgrid_import_counters.argtypes = [vp, vp, i32, i32]
    L.lslam_occgrid_counters_dev_ptr.restype = vp
    L.lslam_occgrid_counters_dev_ptr.argtypes = [vp]
    L.lslam_occgrid_ray_cast.argtypes = [vp, i32, vp, vp, dbl, vp]
    L.lslam_occgrid_ray_cast_dev.argtypes = [vp, i32, vp, vp, dbl, vp]
    L.lslam_occgrid_ray_cast_scans.argtypes = [vp, C.POINTER(LaserParams), i32, vp, dbl, vp, i32]
    L.lslam_occgrid_ray_cast_scans_dev.argtypes = [vp, C.POINTER(LaserParams), i32, vp, dbl, vp, i32]
    L.lslam_occgrid_ray_cast_stats.argtypes = [vp, vp]
    L.lslam_occgrid_create_sharded.argtypes = [vp, C.POINTER(LaserParams), i32, vp, i32, vp, dbl, vp, C.POINTER(vp)]
    L.lslam_pool_occgrid_from_scans.argtypes = [vp, C.POINTER(LaserParams), i32, vp, i32, vp, dbl, C.POINTER(vp)]
    L.lslam_frontend_livemap_create.argtypes = [vp, dbl, C.POINTER(vp)]
    L.lslam_livemap_destroy.argtypes = [vp]
    L.lslam_livemap_destroy.restype = None
    L.lslam_livemap_update.argtypes = [vp]
    L.lslam_livemap_grid.restype = vp
    L.lslam_livemap_grid.argtypes = [vp]
    L.lslam_livemap_stats.argtypes = [vp, vp]
    L.lslam_map_create.argtypes = [vp, i32, i32, C.c_float, C.c_float, C.c_float, i32, C.POINTER(vp)]
    L.lslam_map_destroy.argtypes = [vp]
    L.lslam_map_destroy.restype = None
    L.lslam_map_reset.argtypes = [vp]
    L.lslam_map_set_update_factor_free.argtypes = [vp, C.c_float]
    L.lslam_map_set_update_factor_occupied.argtypes = [vp, C.c_float]
    L.lslam_map_levels.argtypes = [vp]
    L.lslam_map_size.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.lslam_map_scale_to_map.restype = C.c_float
    L.lslam_map_scale_to_map.argtypes = [vp, i32]
    L.lslam_map_update_by_scan.argtypes = [vp, vp, i32, vp, vp]
    L.lslam_map_update_by_scan_dev.argtypes = [vp, vp, i32, vp, vp]
    L.lslam_map_update_just_once.argtypes = [vp, vp, i32, vp, C.c_float, C.c_float, dbl]
    L.lslam_map_match_data.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.lslam_map_match_batch.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.lslam_map_match_batch_dev.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    for f in ("lslam_map_score_batch", "lslam_map_score_batch_dev"):
        getattr(L, f).argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp]
    for f in ("lslam_map_pose_covariance_batch", "lslam_map_pose_covariance_batch_dev"):
        getattr(L, f).argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp]
    for f in ("lslam_map_score_lattice", "lslam_map_score_lattice_dev"):
        getattr(L, f).argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp]
    L.lslam_map_cached_points.argtypes = [vp]
    L.lslam_map_set_option.argtypes = [vp, i32, i32]
    L.lslam_map_batch_stats.argtypes = [vp, vp]
    L.lslam_map_read_logodds.argtypes = [vp, i32, vp]
    L.lslam_map_read_occupancy_i8.argtypes = [vp, i32, vp]
    L.lslam_map_flush.argtypes = [vp]
    L.lslam_map_cells_dev_ptr.restype = vp
    L.lslam_map_cells_dev_ptr.argtypes = [vp, i32]
    L.lslam_map_set_scan.argtypes = [vp, vp, i32, C.POINTER(HectorScan), C.POINTER(i32)]
    L.lslam_map_read_container.argtypes = [vp, vp, i32, vp]
    L.lslam_map_match_container.argtypes = [vp, vp, vp, vp]
    L.lslam_map_update_by_container.argtypes = [vp, vp]
    L.lslam_map_update_batch.argtypes = [vp, i32, vp, vp, vp, vp]
    L.lslam_map_update_batch_dev.argtypes = [vp, i32, vp, vp, vp, vp]
    L.lslam_hector_create.argtypes = [vp, C.POINTER(vp)]
    L.lslam_hector_destroy.argtypes = [vp]
    L.lslam_hector_destroy.restype = None
    L.lslam_hector_reset.argtypes = [vp]
    L.lslam_hector_set_update_thresholds.argtypes = [vp, C.c_float, C.c_float]
    L.lslam_hector_set_option.argtypes = [vp, i32, i32]
    L.lslam_hector_process_many.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, i32, vp, vp, vp]
    L.lslam_hector_process_many_points.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.lslam_hector_state.argtypes = [vp, vp, vp, vp]
    L.lslam_hector_stats.argtypes = [vp, vp]
    L.lslam_hector_fleet_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.lslam_hector_fleet_destroy.argtypes = [vp]
    L.lslam_hector_fleet_destroy.restype = None
    L.lslam_hector_fleet_size.argtypes = [vp]
    L.lslam_hector_fleet_process_many.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, i32, vp, vp, vp, vp]
    L.lslam_hector_fleet_process_many_points.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.lslam_hector_fleet_stats.argtypes = [vp, vp]
    L.lslam_hector_fleet_process_many_clouds.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.lslam_hector_fleet_process_many_clouds_dev.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.lslam_hector_fleet_process_many_synced.argtypes = [vp, vp, C.POINTER(HectorScan), C.POINTER(MsyncLaser), i32, i32, vp, i32,
                                                         vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lslam_hector_fleet_sync_stats.argtypes = [vp, vp]
    L.lslam_map_write_logodds.argtypes = [vp, i32, vp]
    L.lslam_map_write_logodds_dev.argtypes = [vp, i32, vp]
    L.lslam_hector_loc_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.lslam_hector_loc_destroy.argtypes = [vp]
    L.lslam_hector_loc_destroy.restype = None
    L.lslam_hector_loc_size.argtypes = [vp]
    L.lslam_hector_loc_set_poses.argtypes = [vp, i32, i32, vp]
    L.lslam_hector_loc_state.argtypes = [vp, i32, vp, vp]
    L.lslam_hector_loc_set_option.argtypes = [vp, i32, i32]
    L.lslam_hector_loc_process_many.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, i32, vp, vp, vp]
    L.lslam_hector_loc_process_many_points.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.lslam_hector_loc_process_many_clouds.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, vp, vp, vp, vp, vp]
    L.lslam_hector_loc_process_many_clouds_dev.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, vp, vp, i32, vp, vp, vp]
    L.lslam_hector_loc_stats.argtypes = [vp, vp]
    L.lslam_pool_create.argtypes = [i32, C.POINTER(MatcherConfig), C.POINTER(LaserParams), C.POINTER(vp)]
    L.lslam_pool_create_on.argtypes = [vp, i32, C.POINTER(MatcherConfig), C.POINTER(LaserParams), C.POINTER(vp)]
    L.lslam_pool_destroy.argtypes = [vp]
    L.lslam_pool_destroy.restype = None
    L.lslam_pool_devices.argtypes = [vp]
    L.lslam_pool_last_error.argtypes = [vp]
    L.lslam_pool_last_error.restype = C.c_char_p
    L.lslam_pool_set_base_scans.argtypes = [vp, i32, vp, i32, vp, vp, i32]
    L.lslam_pool_match_batch.argtypes = [vp, i32, vp, i32, vp, i32, i32, vp]
    L.lslam_deskew_scan.argtypes = [vp, vp, i32, C.POINTER(DeskewParams), vp, vp, vp, vp, i32, vp, vp]
    L.lslam_deskew_create.argtypes = [vp, C.POINTER(vp)]
    L.lslam_deskew_destroy.argtypes = [vp]
    L.lslam_deskew_destroy.restype = None
    L.lslam_deskew_stats.argtypes = [vp, vp]
    L.lslam_deskew_batch.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lslam_deskew_batch_dev.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lslam_msync_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    L.lslam_msync_destroy.argtypes = [vp]
    L.lslam_msync_destroy.restype = None
    L.lslam_msync_reset.argtypes = [vp]
    L.lslam_msync_push_imu.argtypes = [vp, i32, vp, vp]
    L.lslam_msync_push_odom.argtypes = [vp, i32, vp, vp, vp]
    L.lslam_msync_scans.argtypes = [vp, vp, C.POINTER(MsyncLaser), i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.lslam_msync_scans_dev.argtypes = [vp, vp, C.POINTER(MsyncLaser), i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.lslam_msync_read_windows.argtypes = [vp, vp, vp, vp, i32]
    L.lslam_msync_stats.argtypes = [vp, vp]
    L.lslam_features_create.argtypes = [vp, C.POINTER(vp)]
    L.lslam_features_destroy.argtypes = [vp]
    L.lslam_features_destroy.restype = None
    L.lslam_features_set_threshold.argtypes = [vp, C.c_float]
    L.lslam_features_stats.argtypes = [vp, vp]
    L.lslam_features_batch.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp]
    L.lslam_features_batch_dev.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp]
    L.lslam_plicp_params_defaults.argtypes = [C.POINTER(PlicpParams)]
    L.lslam_plicp_params_defaults.restype = None
    L.lslam_plicp_create.argtypes = [vp, C.POINTER(PlicpParams), C.POINTER(vp)]
    L.lslam_plicp_destroy.argtypes = [vp]
    L.lslam_plicp_destroy.restype = None
    L.lslam_plicp_set_laser.argtypes = [vp, dbl, dbl, dbl, dbl]
    L.lslam_plicp_match_batch.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp]
    L.lslam_plicp_match_batch_dev.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp]
    L.lslam_plicp_debug_iteration.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.lslam_plicp_stats.argtypes = [vp, vp]
    L.lslam_plicp_odom_create.argtypes = [vp, C.POINTER(PlicpParams), i32, dbl, dbl, i32, vp, C.POINTER(vp)]
    L.lslam_plicp_odom_destroy.argtypes = [vp]
    L.lslam_plicp_odom_destroy.restype = None
    L.lslam_plicp_odom_set_laser.argtypes = [vp, dbl, dbl, dbl, dbl]
    L.lslam_plicp_odom_reset.argtypes = [vp]
    L.lslam_plicp_odom_state.argtypes = [vp, vp]
    L.lslam_plicp_odom_process_many.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp]
    L.lslam_plicp_odom_stats.argtypes = [vp, vp]
    L.lslam_plicp_match_clouds.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    L.lslam_plicp_match_clouds_dev.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    L.lslam_plicp_debug_iteration_clouds.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.lslam_plicp_odom_process_many_clouds.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.lslam_plicp_odom_process_many_clouds_dev.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp]
    L.lslam_icp_params_defaults.argtypes = [C.POINTER(IcpParams)]
    L.lslam_icp_params_defaults.restype = None
    L.lslam_icp_create.argtypes = [vp, C.POINTER(IcpParams), C.POINTER(vp)]
    L.lslam_icp_destroy.argtypes = [vp]
    L.lslam_icp_destroy.restype = None
    L.lslam_icp_set_laser.argtypes = [vp, dbl, dbl, dbl, dbl]
    L.lslam_icp_convert_batch.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    L.lslam_icp_convert_batch_dev.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    L.lslam_icp_match_batch.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp]
    L.lslam_icp_match_batch_dev.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp]
    L.lslam_icp_match_clouds.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    L.lslam_icp_match_clouds_dev.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    L.lslam_icp_debug_iteration.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.lslam_icp_stats.argtypes = [vp, vp]
    L.lslam_map_set_cloud.argtypes = [vp, vp, vp, i32, C.POINTER(HectorScan), C.POINTER(i32)]
    L.lslam_hector_process_many_deskewed.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                                                     vp, vp]
    L.lslam_hector_process_many_clouds.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, vp, vp, vp, vp, vp]
    L.lslam_hector_process_many_clouds_dev.argtypes = [vp, C.POINTER(HectorScan), i32, i32, vp, vp, vp, i32, vp, vp, vp]
    L.lslam_hector_process_many_synced.argtypes = [vp, vp, C.POINTER(HectorScan), C.POINTER(MsyncLaser), i32, i32, vp, i32, vp, vp,
                                                   vp, vp, vp, vp, vp, vp]
    L.lslam_clock_sample.argtypes = [vp, vp]
    L.lslam_matcher_get_option.argtypes = [vp, i32]
    L.lslam_matcher_set_option.argtypes = [vp, i32, i32]
    L.lslam_matcher_flush.argtypes = [vp]
    L.lslam_matcher_pipelined_steps.argtypes = [vp]
    L.lslam_matcher_pipelined_steps.restype = C.c_int64
    L.lslam_matcher_step_kernel_launches.argtypes = [vp]
    L.lslam_matcher_step_kernel_launches.restype = C.c_int64
    L.lslam_matcher_lone_kernel_launches.argtypes = [vp]
    L.lslam_matcher_lone_kernel_launches.restype = C.c_int64
    L.lslam_matcher_rows_mfma_launches.argtypes = [vp]
    L.lslam_matcher_rows_mfma_launches.restype = C.c_int64
    L.lslam_matcher_fine_mfma_launches.argtypes = [vp]
    L.lslam_matcher_fine_mfma_launches.restype = C.c_int64
    L.lslam_matcher_coarse_form_launches.argtypes = [vp, vp]
    i64 = C.c_int64
    L.lslam_scan_cache_create.argtypes = [vp, C.POINTER(LaserParams), C.POINTER(vp)]
    L.lslam_scan_cache_destroy.argtypes = [vp]
    L.lslam_scan_cache_destroy.restype = None
    L.lslam_scan_cache_put.argtypes = [vp, i64, vp]
    L.lslam_scan_cache_contains.argtypes = [vp, i64]
    L.lslam_scan_cache_prepare.argtypes = [vp, i64, vp]
    L.lslam_scan_cache_forget.argtypes = [vp, i64]
    L.lslam_scan_cache_size.argtypes = [vp]
    L.lslam_scan_cache_counters.argtypes = [vp, vp]
    L.lslam_matcher_match_scan_cached.argtypes = [vp, vp, i32, vp, vp, i64, vp, vp, i32, vp]
    L.lslam_matcher_read_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.lslam_matcher_read_beam_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.lslam_gmap_create.argtypes = [vp, dbl, dbl, dbl, dbl, dbl, C.POINTER(vp)]
    L.lslam_gmap_destroy.argtypes = [vp]
    L.lslam_gmap_destroy.restype = None
    L.lslam_gmap_info.argtypes = [vp, C.POINTER(GMapGeometry)]
    L.lslam_gmap_set_laser.argtypes = [vp, i32, C.c_float, C.c_float, dbl, dbl]
    L.lslam_gmap_angle_cache.argtypes = [vp, vp, vp]
    L.lslam_gmap_reset.argtypes = [vp]
    L.lslam_gmap_integrate.argtypes = [vp, i32, vp, vp]
    L.lslam_gmap_compute_map.argtypes = [vp, vp, dbl, vp]
    L.lslam_gmap_read_ros_i8.argtypes = [vp, dbl, vp]
    L.lslam_gmap_read_counters.argtypes = [vp, vp, vp, vp]
    L.lslam_gmap_read_patch_mask.argtypes = [vp, vp]
    L.lslam_gmap_stats.argtypes = [vp, vp]
    _LIB = L
    return L


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a: np.ndarray) -> int:
    """Address of a contiguous array's first byte.  `a.ctypes.data` builds a helper object per access (~1 us, four of them per
    per-scan call were a twentieth of a streamed scan); the buffer protocol gives the same address in a third of the time."""
    try:
        return C.addressof(C.c_char.from_buffer(a))
    except (TypeError, ValueError, BufferError):  # read-only or empty arrays
        return a.ctypes.data


class Context:
    """lslam_context: one GPU, one HIP stream."""

    def __init__(self, device: int = 0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.lslam_create(device, C.byref(h))
        if rc != LSLAM_OK:
            raise LslamError(rc, self.L.lslam_last_error(None).decode())
        self.h = h
        self.device = device
        self._children = weakref.WeakSet()  # handles that must be released before the context

    def _adopt(self, child):
        self._children.add(child)

    def check(self, rc: int):
        if rc != LSLAM_OK:
            raise LslamError(rc, self.L.lslam_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            for child in list(self._children):  # matcher / map / grid handles hold a pointer to the context
                child.close()
            self.L.lslam_destroy(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the order of finalisers is arbitrary (a context may already be gone under a handle
        # that points into it) and the process is exiting anyway: release explicitly, or not at all
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:  # incl. module globals already torn down (sys is None) late in shutdown
            pass

    def synchronize(self):
        self.check(self.L.lslam_synchronize(self.h))

    def clock_sample(self) -> np.ndarray:
        """[256][3] uint64: {CU id + 1, shader-clock ticks, 100 MHz ticks} from 256 single-wave blocks (lslam_clock_sample)."""
        out = np.zeros(768, dtype=np.uint64)
        self.check(self.L.lslam_clock_sample(self.h, out.ctypes.data))
        return out.reshape(256, 3)

    @staticmethod
    def clock_ghz(before: np.ndarray, after: np.ndarray):
        """Average shader clock [GHz] between two clock_sample() results: per CU that reported in both, (t1 - t0) / ((r1 - r0) /
        100 MHz); the median over those CUs (None when no CU is in both samples)."""
        b = {int(k): (int(t), int(r)) for k, t, r in before if k}
        ratios = []
        for k, t, r in after:
            if int(k) in b:
                t0, r0 = b[int(k)]
                if int(r) > r0 and int(t) > t0:
                    ratios.append((int(t) - t0) / ((int(r) - r0) / 1e8))
        return float(np.median(ratios)) / 1e9 if ratios else None

    @property
    def stream(self) -> int:
        return self.L.lslam_stream(self.h)

    # raw HBM helpers (bench/tests); torch tensors' data_ptr() work just as well
    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self.check(self.L.lslam_dev_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr: int):
        self.check(self.L.lslam_dev_free(self.h, ptr))

    def upload(self, ptr: int, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        self.check(self.L.lslam_dev_upload(self.h, ptr, a.ctypes.data, a.nbytes))

    def download(self, ptr: int, arr: np.ndarray):
        assert arr.flags["C_CONTIGUOUS"]
        self.check(self.L.lslam_dev_download(self.h, arr.ctypes.data, ptr, arr.nbytes))

    def profile(self, on: bool):
        self.check(self.L.lslam_profile_enable(self.h, int(on)))

    def profile_only(self, kernel_name: str | None):
        """Time only the kernels launched under this name (None = all): fewer events in the stream."""
        self.check(self.L.lslam_profile_only(self.h, kernel_name.encode() if kernel_name else None))

    def profile_reset(self):
        self.check(self.L.lslam_profile_reset(self.h))

    def profile_read(self) -> dict:
        buf = (KernelTime * 64)()
        n = self.L.lslam_profile_read(self.h, buf, 64)
        return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(n)}


MATCHER_OPTIONS = {"row_occupancy": 1, "collect_stats": 2, "lds_staged": 3, "pipeline_depth": 4, "step_kernel": 5,
                   "step_min_scans": 6, "rows_waves": 7, "check_output_reuse": 8, "lone_kernel": 9,
                   "rows_mfma": 10, "fine_mfma": 11}  # LSLAM_OPT_*
# LSLAM_FORM_* in the header's order
COARSE_FORMS = ("generic", "rows_linear", "rows_tiled", "rows_multiwave", "rows_lds_staged", "rows_stats_linear",
                "rows_stats_tiled", "rows_stats_lds_staged", "big", "fine_rows", "fine_tile3")


class ScanMatcher:
    """karto::ScanMatcher on the GPU.  Poses are SENSOR poses (x, y, heading)."""

    def __init__(self, ctx: Context, cfg: MatcherConfig, laser: LaserParams):
        self.ctx, self.L, self.cfg, self.laser = ctx, ctx.L, cfg, laser
        h = C.c_void_p()
        ctx.check(self.L.lslam_matcher_create(ctx.h, C.byref(cfg), C.byref(laser), C.byref(h)))
        self.h = h
        self._frontends = weakref.WeakSet()
        ctx._adopt(self)

    # reference spelling
    @classmethod
    def Create(cls, ctx, cfg, laser):
        """ScanMatcher::Create: returns None where the reference returns NULL."""
        try:
            return cls(ctx, cfg, laser)
        except LslamError as e:
            if e.code == -1:
                return None
            raise

    def close(self):
        if getattr(self, "h", None):
            for fe in list(self._frontends):  # a front-end borrows its matcher
                fe.close()
            self.L.lslam_matcher_destroy(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the order of finalisers is arbitrary (a context may already be gone under a handle
        # that points into it) and the process is exiting anyway: release explicitly, or not at all
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:  # incl. module globals already torn down (sys is None) late in shutdown
            pass

    @property
    def num_beams(self) -> int:
        return self.L.lslam_matcher_num_beams(self.h)

    def grid_info(self) -> dict:
        i = np.zeros(8, dtype=np.int32)
        off = np.zeros(2)
        self.ctx.check(self.L.lslam_matcher_grid_info(self.h, i.ctypes.data, off.ctypes.data))
        keys = ("width", "height", "stride", "roi_x", "roi_y", "roi_w", "roi_h", "kernel_size")
        d = {k: int(v) for k, v in zip(keys, i)}
        d["offset"] = off
        return d

    def GetCorrelationGrid(self) -> np.ndarray:
        gi = self.grid_info()
        out = np.zeros((gi["height"], gi["stride"]), dtype=np.uint8)
        self.ctx.check(self.L.lslam_matcher_get_grid_u8(self.h, out.ctypes.data))
        return out

    def kernel(self) -> np.ndarray:
        k = self.grid_info()["kernel_size"]
        out = np.zeros((k, k), dtype=np.uint8)
        self.ctx.check(self.L.lslam_matcher_get_kernel_u8(self.h, out.ctypes.data))
        return out

    def set_grid(self, grid: np.ndarray, offset):
        g = np.ascontiguousarray(grid, dtype=np.uint8)
        gi = self.grid_info()
        assert g.size == gi["height"] * gi["stride"]
        o = _f64(offset)
        self.ctx.check(self.L.lslam_matcher_set_grid_u8(self.h, g.ctypes.data, o.ctypes.data))

    def set_grid_dev(self, ptr: int, offset):
        o = _f64(offset)
        self.ctx.check(self.L.lslam_matcher_set_grid_u8_dev(self.h, ptr, o.ctypes.data))

    def set_option(self, name: str, value: int):
        self.ctx.check(self.L.lslam_matcher_set_option(self.h, MATCHER_OPTIONS[name], int(value)))

    @property
    def step_kernel_launches(self) -> int:
        """Batched matches that went out as ONE launch (set_option('step_kernel', 3 or 4)) so far."""
        return int(self.L.lslam_matcher_step_kernel_launches(self.h))

    @property
    def lone_kernel_launches(self) -> int:
        """Single-scan matches that went out as ONE launch (set_option('lone_kernel', 4 / 8 / 16)) so far."""
        return int(self.L.lslam_matcher_lone_kernel_launches(self.h))

    @property
    def rows_mfma_launches(self) -> int:
        """Row-kernel launches that summed their rows with the i8 MFMA (set_option('rows_mfma', 1) and a grid whose bytes
        are all <= 127) so far; they are counted in coarse_form_launches() under the same form names as the packed form."""
        return int(self.L.lslam_matcher_rows_mfma_launches(self.h))

    @property
    def fine_mfma_launches(self) -> int:
        """k_resp_tile3 launches that summed their patches with the i8 MFMA (set_option('fine_mfma', 1) and a grid whose
        bytes are all <= 127) so far; coarse_form_launches() counts them under fine_tile3 like the packed form's."""
        return int(self.L.lslam_matcher_fine_mfma_launches(self.h))

    def coarse_form_launches(self) -> dict:
        """Response-kernel launches so far, per form (lslam_matcher_coarse_form_launches): every coarse form goes out
        under the one profile name 'resp_rows_coarse', so this is how a caller that selected a form with set_option sees
        that it -- and not a fallback -- ran."""
        out = (C.c_int64 * len(COARSE_FORMS))()
        self.ctx.check(self.L.lslam_matcher_coarse_form_launches(self.h, out))
        return {name: int(out[i]) for i, name in enumerate(COARSE_FORMS)}

    def get_option(self, name: str) -> int:
        v = int(self.L.lslam_matcher_get_option(self.h, MATCHER_OPTIONS[name]))
        if v < 0:
            raise LslamError(v, "lslam_matcher_get_option(%s)" % name)
        return v

    def flush(self):
        """Order the context stream behind every pipelined step in flight (set_option('pipeline_depth', D > 1))."""
        self.ctx.check(self.L.lslam_matcher_flush(self.h))

    @property
    def pipelined_steps(self) -> int:
        return int(self.L.lslam_matcher_pipelined_steps(self.h))

    def read_stats(self) -> dict:
        out = (C.c_uint64 * 4)()
        self.ctx.check(self.L.lslam_matcher_read_stats(self.h, out))
        b = (C.c_uint64 * 4)()
        self.ctx.check(self.L.lslam_matcher_read_beam_stats(self.h, b))
        return {"rows_in_range": int(out[0]), "rows_live": int(out[1]), "beam_angles": int(out[2]),
                "beam_angles_queued": int(out[3]), "beams_readable": int(b[0]), "beams_live_in_some_angle": int(b[1]),
                "lds_drains_staged": int(b[2]), "lds_drains_global": int(b[3])}

    @property
    def grid_dev_ptr(self) -> int:
        """Device address of the raw grid bytes.  After WRITING through it call set_grid_dev(ptr, offset) with the same
        pointer: the parity planes, row-occupancy bitmaps and tiled copies derived from the grid are refreshed only
        when the matcher is told that the grid changed."""
        return self.L.lslam_matcher_grid_dev_ptr(self.h)

    def sensor_pose_from_robot(self, robot):
        r, out = _f64(robot), np.zeros(3)
        self.L.lslam_sensor_pose_from_robot(C.byref(self.laser), r.ctypes.data, out.ctypes.data)
        return out

    def robot_pose_from_sensor(self, sensor):
        s, out = _f64(sensor), np.zeros(3)
        self.L.lslam_robot_pose_from_sensor(C.byref(self.laser), s.ctypes.data, out.ctypes.data)
        return out

    def AddScans(self, base_ranges, base_sensor_poses, center_pose):
        """MatchScan steps 1-4 + AddScans: rebuild the grid around center_pose."""
        r, p, c = _f64(base_ranges), _f64(base_sensor_poses), _f64(center_pose)
        r = r.reshape(-1, r.shape[-1]) if r.size else r.reshape(0, max(self.num_beams, 1))
        self.ctx.check(self.L.lslam_matcher_set_base_scans(self.h, r.shape[0], r.ctypes.data, r.shape[1],
                                                           p.ctypes.data, c.ctypes.data))

    def MatchScan(self, query_ranges, query_sensor_pose, base_ranges, base_sensor_poses,
                  doPenalize: bool = True, doRefineMatch: bool = True):
        """ScanMatcher::MatchScan -> (response, mean pose, covariance 3x3)."""
        q, qp = _f64(query_ranges), _f64(query_sensor_pose)
        r, p = _f64(base_ranges), _f64(base_sensor_poses)
        r = r.reshape(-1, r.shape[-1]) if r.size else r.reshape(0, max(self.num_beams, 1))
        res = np.zeros(1, dtype=RESULT_DTYPE)
        self.ctx.check(self.L.lslam_matcher_match_scan(self.h, r.shape[0], _ptr(r), r.shape[1], _ptr(p),
                                                       _ptr(q), _ptr(qp), int(doPenalize),
                                                       int(doRefineMatch), _ptr(res)))
        if res["status"][0] != 0:
            raise LslamError(int(res["status"][0]), "the reference would have thrown here")
        return float(res["response"][0]), res["pose"][0].copy(), res["covariance"][0].copy()

    def match_batch(self, ranges, sensor_poses, doPenalize: bool = True, doRefineMatch: bool = True) -> np.ndarray:
        """Coarse+fine search of S independent scans against the CURRENT grid (host arrays)."""
        r, p = _f64(ranges), _f64(sensor_poses)
        r = r.reshape(-1, r.shape[-1])
        res = np.zeros(r.shape[0], dtype=RESULT_DTYPE)
        self.ctx.check(self.L.lslam_matcher_match_batch(self.h, r.shape[0], r.ctypes.data, r.shape[1], p.ctypes.data,
                                                        int(doPenalize), int(doRefineMatch), res.ctypes.data))
        return res

    def match_batch_dev(self, n_scans: int, ranges_ptr: int, stride: int, poses_ptr: int, out_ptr: int,
                        dtype="f32", doPenalize: bool = True, doRefineMatch: bool = True):
        """Same with float32/float64 ranges, poses and results resident in HBM; asynchronous.  With
        set_option('pipeline_depth', D > 1) consecutive calls are pipelined steps: up to D in flight at once, so give D
        consecutive calls their own result buffers and read them after ctx.synchronize()."""
        fn = self.L.lslam_matcher_match_batch_dev_f32 if dtype == "f32" else self.L.lslam_matcher_match_batch_dev_f64
        self.ctx.check(fn(self.h, n_scans, ranges_ptr, stride, poses_ptr, int(doPenalize), int(doRefineMatch), out_ptr))

    # inspection hooks (parity tests)
    def lookup_table(self, ranges, sensor_pose, angle_center, angle_offset, angle_resolution) -> np.ndarray:
        r, p = _f64(ranges), _f64(sensor_pose)
        na = C.c_int()
        self.ctx.check(self.L.lslam_matcher_debug_lookup_table(self.h, r.ctypes.data, p.ctypes.data, angle_center,
                                                               angle_offset, angle_resolution, None, C.byref(na)))
        out = np.zeros((na.value, self.num_beams), dtype=np.int32)
        self.ctx.check(self.L.lslam_matcher_debug_lookup_table(self.h, r.ctypes.data, p.ctypes.data, angle_center,
                                                               angle_offset, angle_resolution, out.ctypes.data,
                                                               C.byref(na)))
        return out

    def coarse_sums(self, ranges, sensor_pose, force_generic: bool = False) -> np.ndarray:
        r, p = _f64(ranges), _f64(sensor_pose)
        nx, ny, na = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.L.lslam_matcher_debug_coarse_sums(self.h, r.ctypes.data, p.ctypes.data, None,
                                                              C.byref(nx), C.byref(ny), C.byref(na), 0))
        out = np.zeros((ny.value, nx.value, na.value), dtype=np.int32)
        self.ctx.check(self.L.lslam_matcher_debug_coarse_sums(self.h, r.ctypes.data, p.ctypes.data, out.ctypes.data,
                                                              C.byref(nx), C.byref(ny), C.byref(na),
                                                              int(force_generic)))
        return out

    def coarse_sums_batch(self, ranges, sensor_poses) -> np.ndarray:
        """Coarse-pass response numerators of EVERY scan of a batch, [n_scans, ny, nx, na] int32, through the launches a
        coarse-only match of that batch takes (lslam_matcher_debug_coarse_sums_batch)."""
        r, p = _f64(ranges), _f64(sensor_poses)
        n = r.shape[0]
        nx, ny, na = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.L.lslam_matcher_debug_coarse_sums(self.h, r.ctypes.data, p.ctypes.data, None,
                                                              C.byref(nx), C.byref(ny), C.byref(na), 0))
        out = np.zeros((n, ny.value, nx.value, na.value), dtype=np.int32)
        self.ctx.check(self.L.lslam_matcher_debug_coarse_sums_batch(self.h, n, r.ctypes.data, r.shape[1], p.ctypes.data,
                                                                    out.ctypes.data))
        return out

    def fine_sums_batch(self, ranges, sensor_poses):
        """Fine-pass numerators of every scan of a batch and the centre each fine pass was searched around:
        ([n_scans, ny, nx, na] int32, [n_scans, 3]) (lslam_matcher_debug_fine_sums_batch)."""
        r, p = _f64(ranges), _f64(sensor_poses)
        n = r.shape[0]
        nx, ny, na = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.L.lslam_matcher_debug_fine_sums_batch(self.h, n, r.ctypes.data, r.shape[1], p.ctypes.data, None, None,
                                                                  C.byref(nx), C.byref(ny), C.byref(na)))
        out = np.zeros((n, ny.value, nx.value, na.value), dtype=np.int32)
        centers = np.zeros((n, 3))
        self.ctx.check(self.L.lslam_matcher_debug_fine_sums_batch(self.h, n, r.ctypes.data, r.shape[1], p.ctypes.data,
                                                                  centers.ctypes.data, out.ctypes.data, C.byref(nx), C.byref(ny),
                                                                  C.byref(na)))
        return out, centers

    def valid_mask(self, ranges, sensor_pose, viewpoint) -> np.ndarray:
        r, p, v = _f64(ranges), _f64(sensor_pose), _f64(viewpoint)
        out = np.zeros(self.num_beams, dtype=np.uint8)
        self.ctx.check(self.L.lslam_matcher_debug_valid_mask(self.h, r.ctypes.data, p.ctypes.data, v.ctypes.data,
                                                             out.ctypes.data))
        return out


class ScanCache:
    """lslam_scan_cache: the device-side scan cache behind seam B1 (readings, world points and FindValidPoints anchors of
    every scan the caller has named, resident in HBM); MatchScan then names its base scans by id."""

    PENALIZE, REFINE, QUERY_TAKES_RESULT_POSE = 1, 2, 4

    def __init__(self, ctx: Context, laser: LaserParams):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        ctx.check(self.L.lslam_scan_cache_create(ctx.h, C.byref(laser), C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_scan_cache_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def put(self, scan_id: int, ranges):
        r = _f64(ranges)
        self.ctx.check(self.L.lslam_scan_cache_put(self.h, int(scan_id), r.ctypes.data))

    def prepare(self, scan_id: int, sensor_pose):
        """World points + anchors of a cached scan at this pose, enqueued (asynchronous)."""
        p = _f64(sensor_pose)
        self.ctx.check(self.L.lslam_scan_cache_prepare(self.h, int(scan_id), p.ctypes.data))

    def __contains__(self, scan_id: int) -> bool:
        return bool(self.L.lslam_scan_cache_contains(self.h, int(scan_id)))

    def forget(self, scan_id: int = -1):
        self.ctx.check(self.L.lslam_scan_cache_forget(self.h, int(scan_id)))

    def __len__(self) -> int:
        return int(self.L.lslam_scan_cache_size(self.h))

    def counters(self) -> dict:
        out = np.zeros(5, dtype=np.int64)
        self.ctx.check(self.L.lslam_scan_cache_counters(self.h, out.ctypes.data))
        return dict(zip(("matches", "uploads", "refreshed", "speculated", "resident_bytes"), (int(v) for v in out)))

    def MatchScan(self, matcher: "ScanMatcher", base_ids, base_sensor_poses, query_sensor_pose, query_id: int = -1,
                  query_ranges=None, doPenalize: bool = True, doRefineMatch: bool = True, takes_result_pose: bool = False):
        """ScanMatcher::MatchScan with the base scans named by id -> (response, mean pose, covariance 3x3)."""
        ids = np.ascontiguousarray(base_ids, dtype=np.int64)
        p, qp = _f64(base_sensor_poses), _f64(query_sensor_pose)
        q = _f64(query_ranges) if query_ranges is not None else None
        flags = (1 if doPenalize else 0) | (2 if doRefineMatch else 0) | (4 if takes_result_pose else 0)
        res = np.zeros(1, dtype=RESULT_DTYPE)
        self.ctx.check(self.L.lslam_matcher_match_scan_cached(matcher.h, self.h, len(ids), _ptr(ids), _ptr(p),
                                                              int(query_id), _ptr(q) if q is not None else None,
                                                              _ptr(qp), flags, _ptr(res)))
        if res["status"][0] != 0:
            raise LslamError(int(res["status"][0]), "the reference would have thrown here")
        return float(res["response"][0]), res["pose"][0].copy(), res["covariance"][0].copy()


class MatcherPool:
    """lslam_pool: the batched many-scan mode over several GPUs of one node from ONE process -- one matcher per device,
    the shared grid copied device-to-device, scans [r*B/W, (r+1)*B/W) on device r, results in scan order."""

    def __init__(self, cfg: MatcherConfig, laser: LaserParams, devices=0):
        self.L = lib()
        h = C.c_void_p()
        if isinstance(devices, int):
            rc = self.L.lslam_pool_create(devices, C.byref(cfg), C.byref(laser), C.byref(h))
        else:
            ids = np.ascontiguousarray(devices, dtype=np.int32)
            rc = self.L.lslam_pool_create_on(ids.ctypes.data, len(ids), C.byref(cfg), C.byref(laser), C.byref(h))
        if rc != LSLAM_OK:
            raise LslamError(rc, self.L.lslam_pool_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the order of finalisers is arbitrary (a context may already be gone under a handle
        # that points into it) and the process is exiting anyway: release explicitly, or not at all
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:  # incl. module globals already torn down (sys is None) late in shutdown
            pass

    def _check(self, rc):
        if rc != LSLAM_OK:
            raise LslamError(rc, self.L.lslam_pool_last_error(self.h).decode())

    @property
    def devices(self) -> int:
        return self.L.lslam_pool_devices(self.h)

    def AddScans(self, base_ranges, base_sensor_poses, center_pose, rebuild_everywhere: bool = False):
        r, p, c = _f64(base_ranges), _f64(base_sensor_poses), _f64(center_pose)
        r = r.reshape(-1, r.shape[-1])
        self._check(self.L.lslam_pool_set_base_scans(self.h, r.shape[0], r.ctypes.data, r.shape[1], p.ctypes.data,
                                                     c.ctypes.data, int(rebuild_everywhere)))

    def CreateOccupancyGrid(self, laser: LaserParams, ranges, sensor_poses, resolution: float):
        """OccupancyGrid::CreateFromScans sharded over the pool's devices in this one process: RCCL (ncclCommInitAll +
        all-reduce) when the devices are distinct, counter addition on the first device otherwise.  Returns
        (cells [h, w] uint8, offset_xy)."""
        r, p = _f64(ranges), _f64(sensor_poses)
        r = r.reshape(-1, r.shape[-1])
        h = C.c_void_p()
        self._check(self.L.lslam_pool_occgrid_from_scans(self.h, C.byref(laser), r.shape[0], r.ctypes.data, r.shape[1],
                                                         p.ctypes.data, float(resolution), C.byref(h)))
        dims, off, res = np.zeros(2, np.int32), np.zeros(2), C.c_double()
        self.L.lslam_occgrid_info(h, dims.ctypes.data, off.ctypes.data, C.byref(res))
        out = np.zeros((int(dims[1]), int(dims[0])), dtype=np.uint8)
        rc = self.L.lslam_occgrid_read_u8(h, out.ctypes.data)
        self.L.lslam_occgrid_destroy(h)
        self._check(rc)
        return out, off

    def match_batch(self, ranges, sensor_poses, doPenalize: bool = True, doRefineMatch: bool = True) -> np.ndarray:
        r, p = _f64(ranges), _f64(sensor_poses)
        r = r.reshape(-1, r.shape[-1])
        out = np.zeros(r.shape[0], dtype=RESULT_DTYPE)
        self._check(self.L.lslam_pool_match_batch(self.h, r.shape[0], r.ctypes.data, r.shape[1], p.ctypes.data,
                                                  int(doPenalize), int(doRefineMatch), out.ctypes.data))
        return out


class FrontEnd:
    """karto::Mapper::Process with every processed scan resident in HBM: running-window match, AddEdges with
    LinkNearChains, TryCloseLoop (config=frontend_config(...)); without `config` the round-1 four-parameter form
    (library defaults for the graph side, loop closing off)."""

    def __init__(self, matcher: ScanMatcher, scan_buffer_size=70, scan_buffer_max_distance=20.0,
                 min_travel_distance=0.2, min_travel_heading=math.radians(10.0), config: FrontEndConfig | None = None):
        self.m, self.ctx, self.L = matcher, matcher.ctx, matcher.L
        h = C.c_void_p()
        if config is not None:
            self.ctx.check(self.L.lslam_frontend_create_ex(matcher.h, C.byref(config), C.byref(h)))
        else:
            self.ctx.check(self.L.lslam_frontend_create(matcher.h, scan_buffer_size, scan_buffer_max_distance,
                                                        min_travel_distance, min_travel_heading, C.byref(h)))
        self.h = h
        self._livemaps = weakref.WeakSet()  # live maps read this front-end: released before it
        self._grids = {}                    # OccupancyGrid(resolution)'s live maps, by resolution
        matcher._frontends.add(self)

    def close(self):
        if getattr(self, "h", None):
            for lm in list(self._livemaps):
                lm.close()
            self._grids.clear()
            self.L.lslam_frontend_destroy(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the order of finalisers is arbitrary (a context may already be gone under a handle
        # that points into it) and the process is exiting anyway: release explicitly, or not at all
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:  # incl. module globals already torn down (sys is None) late in shutdown
            pass

    def Process(self, ranges, odom_pose, time_s: float = 0.0):
        """-> (processed, corrected robot pose, covariance 3x3, response)"""
        r, o = _f64(ranges), _f64(odom_pose)
        ok, resp = C.c_int(), C.c_double()
        pose, cov = np.zeros(3), np.zeros(9)
        self.ctx.check(self.L.lslam_frontend_process_stamped(self.h, _ptr(r), r.shape[0], _ptr(o), time_s,
                                                             C.byref(ok), _ptr(pose), _ptr(cov), C.byref(resp)))
        return bool(ok.value), pose, cov.reshape(3, 3), resp.value

    def ProcessMany(self, ranges, odom_poses, times_s=None):
        """Mapper::Process over scans already at hand, with one scan of look-ahead (the loop search of scan t and the
        running-window match of scan t + 1 share the device).  -> (processed [n] bool, corrected robot poses [n, 3],
        covariances [n, 3, 3], responses [n]); identical to n Process calls."""
        r = _f64(ranges)
        r = r.reshape(-1, r.shape[-1])
        o = _f64(odom_poses).reshape(-1, 3)
        n = r.shape[0]
        assert o.shape[0] == n
        t = None if times_s is None else _f64(times_s)
        ok = np.zeros(n, dtype=np.int32)
        pose, cov, resp = np.zeros((n, 3)), np.zeros((n, 9)), np.zeros(n)
        self.ctx.check(self.L.lslam_frontend_process_many(self.h, n, r.ctypes.data, r.shape[1], o.ctypes.data,
                                                          None if t is None else t.ctypes.data, ok.ctypes.data, pose.ctypes.data,
                                                          cov.ctypes.data, resp.ctypes.data))
        return ok.astype(bool), pose, cov.reshape(n, 3, 3), resp

    def anchor_row(self, scan_id: int) -> np.ndarray:
        """FindValidPoints' anchors of a resident scan at its current pose (beam indices in order)."""
        out = np.zeros(self.m.num_beams + 1, dtype=np.int32)
        self.ctx.check(self.L.lslam_debug_frontend_anchor_row(self.h, int(scan_id), out.ctypes.data))
        return out[1:1 + out[0]].copy()

    def spec_chain_stats(self) -> dict:
        """Speculative anchor chains: world-point refreshes handed one / of those, the ones that recomputed the chain."""
        out = np.zeros(2, dtype=np.int64)
        self.ctx.check(self.L.lslam_frontend_spec_chain_stats(self.h, out.ctypes.data))
        return {"handed": int(out[0]), "recomputed": int(out[1])}

    def lookahead_stats(self) -> dict:
        out = np.zeros(3, dtype=np.int64)
        self.ctx.check(self.L.lslam_frontend_lookahead_stats(self.h, out.ctypes.data))
        return {"started": int(out[0]), "accepted": int(out[1]), "discarded": int(out[2])}

    def num_scans(self) -> int:
        return self.L.lslam_frontend_num_scans(self.h)

    def scan_pose(self, scan_id: int) -> np.ndarray:
        out = np.zeros(3)
        self.ctx.check(self.L.lslam_frontend_scan_pose(self.h, scan_id, out.ctypes.data))
        return out

    def stats(self) -> dict:
        out = np.zeros(6, dtype=np.int64)
        self.ctx.check(self.L.lslam_frontend_stats(self.h, out.ctypes.data))
        return dict(zip(("scans", "edges", "chain_matches", "loop_coarse_matches", "loop_fine_matches", "loops_closed"),
                        (int(v) for v in out)))

    def running_scans(self) -> int:
        return self.L.lslam_frontend_running_scans(self.h)

    def reset(self):
        self.ctx.check(self.L.lslam_frontend_reset(self.h))

    def OccupancyGrid(self, resolution: float):
        """SlamKarto::updateMap's OccupancyGrid::CreateFromScans(GetAllProcessedScans(), resolution): the front-end's live
        map at this resolution, brought up to date.  The grid is a view, valid until the next call."""
        lm = self._grids.get(float(resolution))
        if lm is None or lm.h is None:
            lm = self._grids[float(resolution)] = LiveMap(self, resolution)
        lm.update()
        return lm.grid()


class OccupancyGrid:
    """karto::OccupancyGrid (hit/pass counters) built on the GPU from scans at sensor poses."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.L, self.h = ctx, ctx.L, h
        ctx._adopt(self)

    @classmethod
    def CreateFromScans(cls, ctx: Context, laser: LaserParams, ranges, sensor_poses, resolution: float):
        """OccupancyGrid::CreateFromScans; None where the reference returns NULL (no scans)."""
        r, p = _f64(ranges), _f64(sensor_poses)
        r = r.reshape(-1, r.shape[-1]) if r.size else r.reshape(0, 1)
        if r.shape[0] == 0:
            return None
        h = C.c_void_p()
        ctx.check(ctx.L.lslam_occgrid_create_from_scans(ctx.h, C.byref(laser), r.shape[0], r.ctypes.data, r.shape[1],
                                                        p.ctypes.data, resolution, C.byref(h)))
        return cls(ctx, h)

    # ---- sharded build: boxes merge by min/max, counters by integer addition, both exact ----
    @staticmethod
    def scan_bounds(ctx: Context, laser: LaserParams, ranges, sensor_poses) -> np.ndarray:
        """Box (minx, miny, maxx, maxy) ComputeDimensions derives from THESE scans; no scans -> the identity box."""
        r, p = _f64(ranges), _f64(sensor_poses)
        r = r.reshape(-1, r.shape[-1]) if r.size else r.reshape(0, 1)
        box = np.zeros(4)
        ctx.check(ctx.L.lslam_occgrid_scan_bounds(ctx.h, C.byref(laser), r.shape[0], r.ctypes.data, r.shape[1], p.ctypes.data,
                                                  box.ctypes.data))
        return box

    @classmethod
    def CreatePartial(cls, ctx: Context, laser: LaserParams, ranges, sensor_poses, resolution: float, box):
        """Counters of these scans (possibly none) on the grid of `box`, the merged box of all shards."""
        r, p, b = _f64(ranges), _f64(sensor_poses), _f64(box)
        r = r.reshape(-1, r.shape[-1]) if r.size else r.reshape(0, 1)
        h = C.c_void_p()
        ctx.check(ctx.L.lslam_occgrid_create_partial(ctx.h, C.byref(laser), r.shape[0], r.ctypes.data, r.shape[1],
                                                     p.ctypes.data, resolution, b.ctypes.data, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def CreateSharded(cls, ctx: Context, laser: LaserParams, ranges, sensor_poses, resolution: float, nccl_comm: int):
        """This rank's scans in, the grid of ALL ranks' scans out: box all-reduce + ONE counter all-reduce, RCCL called by
        the library itself on the context stream (lslam_occgrid_create_sharded).  nccl_comm: an ncclComm_t handle."""
        r, p = _f64(ranges), _f64(sensor_poses)
        r = r.reshape(-1, r.shape[-1]) if r.size else r.reshape(0, 1)
        h = C.c_void_p()
        ctx.check(ctx.L.lslam_occgrid_create_sharded(ctx.h, C.byref(laser), r.shape[0], r.ctypes.data, r.shape[1], p.ctypes.data,
                                                     float(resolution), C.c_void_p(nccl_comm), C.byref(h)))
        return cls(ctx, h)

    def counter_words(self) -> int:
        n = C.c_size_t()
        self.ctx.check(self.L.lslam_occgrid_counter_words(self.h, C.byref(n)))
        return int(n.value)

    def export_counters(self) -> np.ndarray:
        """uint32 [2, stride*height]: pass plane, hit plane."""
        out = np.zeros(self.counter_words(), dtype=np.uint32)
        self.ctx.check(self.L.lslam_occgrid_export_counters(self.h, out.ctypes.data, 0))
        return out.reshape(2, -1)

    def import_counters(self, counters, accumulate: bool = False):
        c = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1)
        if c.size != self.counter_words():
            raise ValueError(f"expected {self.counter_words()} counter words, got {c.size}")
        self.ctx.check(self.L.lslam_occgrid_import_counters(self.h, c.ctypes.data, 0, int(accumulate)))

    def export_counters_dev(self, dev_ptr: int):
        self.ctx.check(self.L.lslam_occgrid_export_counters(self.h, C.c_void_p(dev_ptr), 1))

    def import_counters_dev(self, dev_ptr: int, accumulate: bool = False):
        self.ctx.check(self.L.lslam_occgrid_import_counters(self.h, C.c_void_p(dev_ptr), 1, int(accumulate)))

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_occgrid_destroy(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the order of finalisers is arbitrary (a context may already be gone under a handle
        # that points into it) and the process is exiting anyway: release explicitly, or not at all
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:  # incl. module globals already torn down (sys is None) late in shutdown
            pass

    def info(self):
        d, off, res = np.zeros(2, dtype=np.int32), np.zeros(2), C.c_double()
        self.ctx.check(self.L.lslam_occgrid_info(self.h, d.ctypes.data, off.ctypes.data, C.byref(res)))
        return int(d[0]), int(d[1]), off, res.value

    def data(self) -> np.ndarray:
        w, h, _, _ = self.info()
        out = np.zeros((h, w), dtype=np.uint8)
        self.ctx.check(self.L.lslam_occgrid_read_u8(self.h, out.ctypes.data))
        return out

    def ros_data(self) -> np.ndarray:
        w, h, _, _ = self.info()
        out = np.zeros((h, w), dtype=np.int8)
        self.ctx.check(self.L.lslam_occgrid_read_ros_i8(self.h, out.ctypes.data))
        return out

    # ---- OccupancyGrid::RayCast (Karto.h:5717-5755), batched ----
    @staticmethod
    def laser_beams(laser: LaserParams) -> int:
        """The beam count the library derives from a laser: (kt_int32u)Round((max - min) / resolution)."""
        v = (laser.maximum_angle - laser.minimum_angle) / laser.angular_resolution
        return int(math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5))

    def ray_cast(self, poses, max_range) -> np.ndarray:
        """Distance from every pose (x, y, heading) along its heading to the first cell that is not free, at most
        max_range (a scalar for all rays, or one value per ray).  -> float64 [n]"""
        p = _f64(poses).reshape(-1, 3)
        out = np.zeros(p.shape[0])
        if np.ndim(max_range) == 0:
            mr, common = None, float(max_range)
        else:
            mr, common = _f64(max_range).reshape(-1), 0.0
            if mr.size != p.shape[0]:
                raise ValueError(f"expected {p.shape[0]} max ranges, got {mr.size}")
        self.ctx.check(self.L.lslam_occgrid_ray_cast(self.h, p.shape[0], p.ctypes.data, None if mr is None else mr.ctypes.data,
                                                     common, out.ctypes.data))
        return out

    def ray_cast_scans(self, laser: LaserParams, sensor_poses, max_range: float, out_stride: int | None = None) -> np.ndarray:
        """The range image `laser` would see from every sensor pose: beam i looks along heading + minimum_angle +
        i * angular_resolution.  -> float64 [n_poses, out_stride] (out_stride defaults to the beam count; columns past it
        are left zero), the layout match_batch and the front-end take as ranges."""
        p = _f64(sensor_poses).reshape(-1, 3)
        stride = self.laser_beams(laser) if out_stride is None else int(out_stride)
        out = np.zeros((p.shape[0], max(stride, 0)))
        self.ctx.check(self.L.lslam_occgrid_ray_cast_scans(self.h, C.byref(laser), p.shape[0], p.ctypes.data, float(max_range),
                                                           out.ctypes.data, stride))
        return out

    def ray_cast_dev(self, n_rays: int, poses_ptr: int, max_ranges_ptr: int | None, max_range: float, out_ptr: int):
        """ray_cast on device pointers: enqueued on the context stream, no host wait (results after ctx.synchronize())."""
        self.ctx.check(self.L.lslam_occgrid_ray_cast_dev(self.h, int(n_rays), C.c_void_p(poses_ptr),
                                                         C.c_void_p(max_ranges_ptr) if max_ranges_ptr else None,
                                                         float(max_range), C.c_void_p(out_ptr)))

    def ray_cast_scans_dev(self, laser: LaserParams, n_poses: int, poses_ptr: int, max_range: float, out_ptr: int,
                           out_stride: int):
        self.ctx.check(self.L.lslam_occgrid_ray_cast_scans_dev(self.h, C.byref(laser), int(n_poses), C.c_void_p(poses_ptr),
                                                               float(max_range), C.c_void_p(out_ptr), int(out_stride)))

    def ray_cast_stats(self) -> dict:
        out = np.zeros(4, dtype=np.int64)
        self.ctx.check(self.L.lslam_occgrid_ray_cast_stats(self.h, out.ctypes.data))
        return dict(zip(("calls", "rays", "refreshes", "samples"), (int(v) for v in out)))


class _OccupancyGridView(OccupancyGrid):
    """An lslam_occgrid somebody else owns (a live map's): everything OccupancyGrid reads, nothing it releases."""

    def __init__(self, ctx: Context, h, owner):
        self.ctx, self.L, self.h, self._owner = ctx, ctx.L, h, owner

    def close(self):
        self.h = None


class LiveMap:
    """The occupancy grid of ALL the front-end's processed scans, kept up to date on the device: update() traces only the
    scans processed since the last one unless the grid has to move (see lslam_livemap_update); after it the map equals
    OccupancyGrid::CreateFromScans over every processed scan at its current pose."""

    def __init__(self, frontend: FrontEnd, resolution: float):
        self.fe, self.ctx, self.L = frontend, frontend.ctx, frontend.L
        h = C.c_void_p()
        self.ctx.check(self.L.lslam_frontend_livemap_create(frontend.h, float(resolution), C.byref(h)))
        self.h = h
        self._view = None
        frontend._livemaps.add(self)

    def close(self):
        if getattr(self, "h", None):
            if self._view is not None:
                self._view.close()
            self.L.lslam_livemap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:  # incl. module globals already torn down (sys is None) late in shutdown
            pass

    def update(self):
        if self._view is not None:  # the borrowed grid is valid until the next update
            self._view.close()
            self._view = None
        self.ctx.check(self.L.lslam_livemap_update(self.h))

    def grid(self):
        """The map as an OccupancyGrid (info / data / ros_data / export_counters ...) that does not own the handle; None
        before the first update."""
        g = self.L.lslam_livemap_grid(self.h)
        if not g:
            return None
        if self._view is None or self._view.h is None:
            self._view = _OccupancyGridView(self.ctx, C.c_void_p(g), self)
        return self._view

    def stats(self) -> dict:
        out = np.zeros(6, dtype=np.int64)
        self.ctx.check(self.L.lslam_livemap_stats(self.h, out.ctypes.data))
        return dict(zip(("updates", "appends", "grows", "rebuilds", "scans_traced", "scans"), (int(v) for v in out)))


class OccGridMap:
    """hectorslam log-odds occupancy grid pyramid on the GPU (OccGridMapBase / MapRepMultiMap)."""

    def __init__(self, ctx: Context, size_x: int, size_y: int, cell_length: float, offset=(0.0, 0.0),
                 levels: int = 1):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        ctx.check(self.L.lslam_map_create(ctx.h, size_x, size_y, cell_length, offset[0], offset[1], levels, C.byref(h)))
        self.h = h
        # what save() records and load() compares: the arguments as the library took them (floats are C floats there)
        self.geometry = np.array([size_x, size_y, np.float32(cell_length), np.float32(offset[0]), np.float32(offset[1])], np.float64)
        ctx._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            for proc in list(getattr(self, "_processors", ())):  # a HectorProcessor borrows its map
                proc.close()
            self.L.lslam_map_destroy(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the order of finalisers is arbitrary (a context may already be gone under a handle
        # that points into it) and the process is exiting anyway: release explicitly, or not at all
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:  # incl. module globals already torn down (sys is None) late in shutdown
            pass

    def reset(self):
        self.ctx.check(self.L.lslam_map_reset(self.h))

    def setUpdateFreeFactor(self, p: float):
        self.ctx.check(self.L.lslam_map_set_update_factor_free(self.h, p))

    def setUpdateOccupiedFactor(self, p: float):
        self.ctx.check(self.L.lslam_map_set_update_factor_occupied(self.h, p))

    @property
    def levels(self) -> int:
        return self.L.lslam_map_levels(self.h)

    def size(self, level: int = 0):
        sx, sy = C.c_int(), C.c_int()
        self.ctx.check(self.L.lslam_map_size(self.h, level, C.byref(sx), C.byref(sy)))
        return sx.value, sy.value

    def getScaleToMap(self, level: int = 0) -> float:
        return self.L.lslam_map_scale_to_map(self.h, level)

    def updateByScan(self, points_xy, origo_xy, robot_pose_world):
        """MapRepMultiMap::updateByScan.  Level 0 takes this container; the levels above 0 take the container cached
        by the LAST matchData call (the reference's dataContainers: empty before the first matchData, stale if a
        different scan was matched).  At most 65536 points (LslamError beyond; the reference has no limit); NaN / Inf
        / out-of-int-range points are dropped like on the reference's x86 build.  Asynchronous: enqueued when this
        returns, readers are ordered after it."""
        p = np.ascontiguousarray(points_xy, dtype=np.float32).reshape(-1, 2)
        o = np.ascontiguousarray(origo_xy, dtype=np.float32)
        w = np.ascontiguousarray(robot_pose_world, dtype=np.float32)
        self.ctx.check(self.L.lslam_map_update_by_scan(self.h, _ptr(p), p.shape[0], _ptr(o), _ptr(w)))

    def updateByScan_dev(self, points_ptr: int, n: int, origo_xy, robot_pose_world):
        o = np.ascontiguousarray(origo_xy, dtype=np.float32)
        w = np.ascontiguousarray(robot_pose_world, dtype=np.float32)
        self.ctx.check(self.L.lslam_map_update_by_scan_dev(self.h, points_ptr, n, o.ctypes.data, w.ctypes.data))

    def setScan(self, ranges_f32, scan: HectorScan) -> int:
        """LaserScan -> DataContainer on the device (hector_slam.cc:193, 320-362); returns the container size."""
        r = np.ascontiguousarray(ranges_f32, dtype=np.float32)
        n = C.c_int32()
        self.ctx.check(self.L.lslam_map_set_scan(self.h, r.ctypes.data, r.shape[0], C.byref(scan), C.byref(n)))
        return n.value

    def setCloud(self, xyz, valid, scan: HectorScan) -> int:
        """A de-skewed cloud (deskew_scan / Deskewer.batch: xyz [n,3], valid [n]) -> DataContainer on the device
        (hector_slam.cc:320-362); returns the container size.  lesson5's cloud has z ~ 1: the z window must contain 1."""
        p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        v = np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)
        assert len(v) == len(p)
        n = C.c_int32()
        self.ctx.check(self.L.lslam_map_set_cloud(self.h, p.ctypes.data, v.ctypes.data, len(p), C.byref(scan), C.byref(n)))
        return n.value

    def container(self):
        """-> (points [n,2] float32, origo [2]) of the resident container."""
        origo = np.zeros(2, np.float32)
        n = self.L.lslam_map_read_container(self.h, None, 0, origo.ctypes.data)
        pts = np.zeros((max(n, 0), 2), np.float32)
        if n > 0:
            self.L.lslam_map_read_container(self.h, pts.ctypes.data, n, origo.ctypes.data)
        return pts, origo

    def matchContainer(self, begin_estimate_world):
        b = np.ascontiguousarray(begin_estimate_world, dtype=np.float32)
        pose, cov = np.zeros(3, dtype=np.float32), np.zeros(9, dtype=np.float32)
        self.ctx.check(self.L.lslam_map_match_container(self.h, b.ctypes.data, pose.ctypes.data, cov.ctypes.data))
        return pose, cov.reshape(3, 3)

    def updateByContainer(self, robot_pose_world):
        w = np.ascontiguousarray(robot_pose_world, dtype=np.float32)
        self.ctx.check(self.L.lslam_map_update_by_container(self.h, w.ctypes.data))

    def updateByScans(self, points_list, origos_xy, robot_poses_world):
        """Batched update: exactly len(points_list) successive updateByScan calls (every level fed the same scan),
        marked in parallel and applied in one pass over the map."""
        counts = np.array([len(p) for p in points_list], dtype=np.int32)
        pts = (np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in points_list])
               if len(points_list) else np.zeros((0, 2), np.float32))
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(origos_xy, dtype=np.float32), (len(counts), 2)))
        w = np.ascontiguousarray(robot_poses_world, dtype=np.float32).reshape(len(counts), 3)
        self.ctx.check(self.L.lslam_map_update_batch(self.h, len(counts), pts.ctypes.data, counts.ctypes.data,
                                                     o.ctypes.data, w.ctypes.data))

    def updateByScans_dev(self, points_ptr: int, counts, origos_xy, robot_poses_world):
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(origos_xy, dtype=np.float32), (len(counts), 2)))
        w = np.ascontiguousarray(robot_poses_world, dtype=np.float32).reshape(len(counts), 3)
        self.ctx.check(self.L.lslam_map_update_batch_dev(self.h, len(counts), points_ptr, counts.ctypes.data,
                                                         o.ctypes.data, w.ctypes.data))

    def updateByScanJustOnce(self, points_xy_m, origo_xy=(0.0, 0.0), begin=(800.0, 800.0), metres_per_cell=0.05):
        p = np.ascontiguousarray(points_xy_m, dtype=np.float32).reshape(-1, 2)
        o = np.ascontiguousarray(origo_xy, dtype=np.float32)
        self.ctx.check(self.L.lslam_map_update_just_once(self.h, p.ctypes.data, p.shape[0], o.ctypes.data,
                                                         begin[0], begin[1], metres_per_cell))

    def matchData(self, begin_estimate_world, points_xy, origo_xy=(0.0, 0.0)):
        """MapRepMultiMap::matchData -> (pose[3] float32, covMatrix 3x3 float32).  Like the reference
        (MapRepMultiMap.h:161) the container is cached: the NEXT updateByScan feeds the levels above 0
        from it, whatever container that call is handed."""
        p = np.ascontiguousarray(points_xy, dtype=np.float32).reshape(-1, 2)
        o = np.ascontiguousarray(origo_xy, dtype=np.float32)
        b = np.ascontiguousarray(begin_estimate_world, dtype=np.float32)
        pose, cov = np.zeros(3, dtype=np.float32), np.zeros(9, dtype=np.float32)
        self.ctx.check(self.L.lslam_map_match_data(self.h, p.ctypes.data, p.shape[0], o.ctypes.data, b.ctypes.data,
                                                   pose.ctypes.data, cov.ctypes.data))
        return pose, cov.reshape(3, 3)

    def matchBatch(self, begin_world, containers, entry_container=None, counts=None):
        """Many matchData calls against the map as it is, in one launch -> (poses[B,3], covs[B,3,3]).  `containers`: a
        list of (n,2) float32 arrays, or -- with `counts` -- one packed (sum(counts),2) array; `entry_container[B]` names
        each entry's container (None: entry i uses container i).  A pure query: unlike matchData it caches no container."""
        if counts is None:
            counts = np.array([len(p) for p in containers], dtype=np.int32)
            pts = (np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in containers])
                   if len(containers) else np.zeros((0, 2), np.float32))
        else:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            pts = np.asarray(containers, dtype=np.float32).reshape(-1, 2)
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        b = np.ascontiguousarray(begin_world, dtype=np.float32).reshape(-1, 3)
        ec = None if entry_container is None else np.ascontiguousarray(entry_container, dtype=np.int32)
        poses, covs = np.zeros((len(b), 3), np.float32), np.zeros((len(b), 9), np.float32)
        self.ctx.check(self.L.lslam_map_match_batch(self.h, len(b), len(counts), pts.ctypes.data, counts.ctypes.data,
                                                    None if ec is None else ec.ctypes.data, b.ctypes.data,
                                                    poses.ctypes.data, covs.ctypes.data))
        return poses, covs.reshape(-1, 3, 3)

    def matchBatch_dev(self, n_entries: int, points_ptr: int, counts, entry_container, begin_ptr: int, poses_ptr: int,
                       covs_ptr: int = 0):
        """matchBatch on device pointers (points, start poses, results in HBM); asynchronous on the context stream."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        ec = None if entry_container is None else np.ascontiguousarray(entry_container, dtype=np.int32)
        self.ctx.check(self.L.lslam_map_match_batch_dev(self.h, n_entries, len(counts), points_ptr, counts.ctypes.data,
                                                        None if ec is None else ec.ctypes.data, begin_ptr, poses_ptr,
                                                        covs_ptr or None))

    @staticmethod
    def _pack(containers, counts):
        """-> (packed points [sum, 2] float32, counts int32) of a list of containers, or of one packed array with `counts`."""
        if counts is None:
            counts = np.array([len(p) for p in containers], dtype=np.int32)
            pts = (np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in containers])
                   if len(containers) else np.zeros((0, 2), np.float32))
        else:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            pts = np.asarray(containers, dtype=np.float32).reshape(-1, 2)
        return np.ascontiguousarray(pts, dtype=np.float32), counts

    def scoreBatch(self, poses_world, containers, entry_container=None, counts=None, level: int = 0):
        """getResidualForState / getLikelihoodForState (OccGridMapUtil.h:342-374) of many (container, world pose) pairs on
        one level of the map as it is -> (residual[B], likelihood[B]).  Containers as for matchBatch.  A pure query."""
        pts, counts = self._pack(containers, counts)
        w = np.ascontiguousarray(poses_world, dtype=np.float32).reshape(-1, 3)
        ec = None if entry_container is None else np.ascontiguousarray(entry_container, dtype=np.int32)
        res, lik = np.zeros(len(w), np.float32), np.zeros(len(w), np.float32)
        self.ctx.check(self.L.lslam_map_score_batch(self.h, len(w), len(counts), pts.ctypes.data, counts.ctypes.data,
                                                    None if ec is None else ec.ctypes.data, w.ctypes.data, int(level),
                                                    res.ctypes.data, lik.ctypes.data))
        return res, lik

    def scoreBatch_dev(self, n_entries: int, points_ptr: int, counts, entry_container, poses_ptr: int, level: int,
                       residual_ptr: int, likelihood_ptr: int):
        """scoreBatch on device pointers (residual_ptr may be 0); asynchronous on the context stream."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        ec = None if entry_container is None else np.ascontiguousarray(entry_container, dtype=np.int32)
        self.ctx.check(self.L.lslam_map_score_batch_dev(self.h, n_entries, len(counts), points_ptr, counts.ctypes.data,
                                                        None if ec is None else ec.ctypes.data, poses_ptr, int(level),
                                                        residual_ptr or None, likelihood_ptr or None))

    def poseCovarianceBatch(self, poses_world, containers, entry_container=None, counts=None, level: int = 0):
        """getCovarianceForPose + getCovMatrixWorldCoords (OccGridMapUtil.h:249-339) per (container, world pose) ->
        (likelihoods[B,7] of the sigma points, cov_map[B,3,3] in level cells / rad, cov_world[B,3,3] in m / rad)."""
        pts, counts = self._pack(containers, counts)
        w = np.ascontiguousarray(poses_world, dtype=np.float32).reshape(-1, 3)
        ec = None if entry_container is None else np.ascontiguousarray(entry_container, dtype=np.int32)
        lik = np.zeros((len(w), 7), np.float32)
        cm, cw = np.zeros((len(w), 9), np.float32), np.zeros((len(w), 9), np.float32)
        self.ctx.check(self.L.lslam_map_pose_covariance_batch(self.h, len(w), len(counts), pts.ctypes.data, counts.ctypes.data,
                                                              None if ec is None else ec.ctypes.data, w.ctypes.data,
                                                              int(level), lik.ctypes.data, cm.ctypes.data, cw.ctypes.data))
        return lik, cm.reshape(-1, 3, 3), cw.reshape(-1, 3, 3)

    def poseCovarianceBatch_dev(self, n_entries: int, points_ptr: int, counts, entry_container, poses_ptr: int, level: int,
                                likelihoods_ptr: int, cov_map_ptr: int = 0, cov_world_ptr: int = 0):
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        ec = None if entry_container is None else np.ascontiguousarray(entry_container, dtype=np.int32)
        self.ctx.check(self.L.lslam_map_pose_covariance_batch_dev(
            self.h, n_entries, len(counts), points_ptr, counts.ctypes.data, None if ec is None else ec.ctypes.data, poses_ptr,
            int(level), likelihoods_ptr or None, cov_map_ptr or None, cov_world_ptr or None))

    @staticmethod
    def lattice_poses(centre_world, counts, steps) -> np.ndarray:
        """The world poses scoreLattice evaluates, [nt * ny * nx, 3] float32 in the volume's order, by its own expression."""
        c = np.asarray(centre_world, np.float32)
        d = np.asarray(steps, np.float32)
        nx, ny, nt = (int(v) for v in counts)
        ax = [c[a] + (np.arange(n, dtype=np.int64) - n // 2).astype(np.float32) * d[a] for a, n in enumerate((nx, ny, nt))]
        out = np.zeros((nt, ny, nx, 3), np.float32)
        out[..., 0] = ax[0][None, None, :]
        out[..., 1] = ax[1][None, :, None]
        out[..., 2] = ax[2][:, None, None]
        return out.reshape(-1, 3)

    def scoreLattice(self, points_xy, centre_world, counts, steps, level: int = 0):
        """Likelihoods of one container over a lattice of world poses around centre_world (counts = (nx, ny, nt), steps =
        (dx, dy, dtheta)) -> (volume[nt, ny, nx], best linear index or -1, best likelihood)."""
        p = np.ascontiguousarray(points_xy, dtype=np.float32).reshape(-1, 2)
        c = np.ascontiguousarray(centre_world, dtype=np.float32)
        n3 = np.ascontiguousarray(counts, dtype=np.int32)
        d = np.ascontiguousarray(steps, dtype=np.float32)
        assert c.shape == (3,) and n3.shape == (3,) and d.shape == (3,)
        vol = np.zeros(max(int(n3[0]), 0) * max(int(n3[1]), 0) * max(int(n3[2]), 0), np.float32)
        bi, bl = C.c_int32(0), C.c_float(0.0)
        self.ctx.check(self.L.lslam_map_score_lattice(self.h, p.ctypes.data, p.shape[0], c.ctypes.data, n3.ctypes.data,
                                                      d.ctypes.data, int(level), vol.ctypes.data, C.addressof(bi), C.addressof(bl)))
        return vol.reshape(int(n3[2]), int(n3[1]), int(n3[0])), bi.value, np.float32(bl.value)

    def scoreLattice_dev(self, points_ptr: int, n: int, centre_world, counts, steps, level: int, volume_ptr: int,
                         best_index_ptr: int = 0, best_likelihood_ptr: int = 0):
        c = np.ascontiguousarray(centre_world, dtype=np.float32)
        n3 = np.ascontiguousarray(counts, dtype=np.int32)
        d = np.ascontiguousarray(steps, dtype=np.float32)
        self.ctx.check(self.L.lslam_map_score_lattice_dev(self.h, points_ptr, n, c.ctypes.data, n3.ctypes.data, d.ctypes.data,
                                                          int(level), volume_ptr or None, best_index_ptr or None,
                                                          best_likelihood_ptr or None))

    def relocalise(self, container, centre_world, counts, steps, level: int, k: int):
        """Global-then-local: score the lattice on `level`, start matchBatch from its k best states, score the k matched
        poses on level 0 -> (poses[k,3], likelihoods[k], covs[k,3,3]) sorted by likelihood, best first."""
        p = np.ascontiguousarray(container, dtype=np.float32).reshape(-1, 2)
        vol, _, _ = self.scoreLattice(p, centre_world, counts, steps, level)
        flat = vol.reshape(-1)
        order = np.argsort(-np.where(np.isnan(flat), -np.inf, flat), kind="stable")[:max(int(k), 0)]
        starts = self.lattice_poses(centre_world, counts, steps)[order]
        if not len(starts):
            return np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros((0, 3, 3), np.float32)
        poses, covs = self.matchBatch(starts, [p], entry_container=np.zeros(len(starts), np.int32))
        _, lik = self.scoreBatch(poses, [p], entry_container=np.zeros(len(starts), np.int32), level=0)
        best = np.argsort(-np.where(np.isnan(lik), -np.inf, lik), kind="stable")
        return poses[best], lik[best], covs[best]

    def set_option(self, name: str, value: int):
        """'ordered_sums': matchData adds its sums in point order (bit-equal to the CPU restatement) instead of in parallel."""
        self.ctx.check(self.L.lslam_map_set_option(self.h, {"ordered_sums": 1, "batch_scratch_mb": 2, "batch_radius_cells": 3}[name],
                                                   int(value)))

    def batch_stats(self) -> dict:
        """Scratch of the batched update: bytes held, rounds of the last batch, cells outside their window (must be 0), budget."""
        out = (C.c_int64 * 4)()
        self.ctx.check(self.L.lslam_map_batch_stats(self.h, out))
        return {"scratch_bytes": int(out[0]), "rounds": int(out[1]), "window_misses": int(out[2]), "budget_bytes": int(out[3])}

    def cached_points(self) -> int:
        return self.L.lslam_map_cached_points(self.h)

    def logodds(self, level: int = 0) -> np.ndarray:
        sx, sy = self.size(level)
        out = np.zeros((sy, sx), dtype=np.float32)
        self.ctx.check(self.L.lslam_map_read_logodds(self.h, level, out.ctypes.data))
        return out

    def occupancy_i8(self, level: int = 0) -> np.ndarray:
        sx, sy = self.size(level)
        out = np.zeros((sy, sx), dtype=np.int8)
        self.ctx.check(self.L.lslam_map_read_occupancy_i8(self.h, level, out.ctypes.data))
        return out

    def cells_dev_ptr(self, level: int = 0) -> int:
        return self.L.lslam_map_cells_dev_ptr(self.h, level)

    def write_logodds(self, level: int, plane):
        """The inverse of logodds(): `plane` [size_y, size_x] float32 becomes the level's log-odds plane, bit for bit (NaN,
        +-inf and -0.0 included).  Containers, update factors and counters stay; the next update treats every cell as not yet
        touched by its scan."""
        sx, sy = self.size(level)
        p = np.ascontiguousarray(plane, dtype=np.float32)
        if p.size != sx * sy:
            raise ValueError(f"level {level} takes {sy} x {sx} cells, got {p.shape}")
        self.ctx.check(self.L.lslam_map_write_logodds(self.h, level, p.ctypes.data))

    def write_logodds_dev(self, level: int, ptr: int):
        """The same from a float32 plane in HBM (asynchronous on the context's stream); another map's cells_dev_ptr(level) of
        the same context and level size makes this the device-to-device snapshot."""
        self.ctx.check(self.L.lslam_map_write_logodds_dev(self.h, level, ptr))

    def save(self, path):
        """The pyramid as a numpy .npz: geometry (size_x, size_y, cell_length, offset_x, offset_y), levels, level_0 .. level_{n-1}."""
        planes = {f"level_{i}": self.logodds(i) for i in range(self.levels)}
        with open(path, "wb") as f:  # (np.savez would append .npz to a bare name)
            np.savez(f, geometry=self.geometry, levels=np.int32(self.levels), **planes)

    def load(self, path):
        """Planes saved by save() into this map.  Refuses a file whose geometry or number of levels differs from the map's."""
        with np.load(path) as z:
            if not np.array_equal(z["geometry"], self.geometry) or int(z["levels"]) != self.levels:
                raise ValueError(f"{path}: geometry {z['geometry'].tolist()} x {int(z['levels'])} levels is not this map's "
                                 f"{self.geometry.tolist()} x {self.levels}")
            planes = [z[f"level_{i}"] for i in range(self.levels)]
        for i, p in enumerate(planes):
            if p.shape != self.size(i)[::-1]:
                raise ValueError(f"{path}: level {i} is {p.shape}")
        for i, p in enumerate(planes):
            self.write_logodds(i, p)


HECTOR_RECORD = np.dtype([("pose", np.float32, 3), ("cov", np.float32, (3, 3)), ("updated", np.int32), ("n_points", np.int32),
                          ("pad", np.int32, 2)])
assert HECTOR_RECORD.itemsize == 64


class HectorProcessor:
    """hectorslam::HectorSlamProcessor (H/slam_main/HectorSlamProcessor.h:57-117) streamed on the device: many scans per
    call, the pose chain, the map-update decision and the update geometry never leave the GPU; one host synchronisation
    per call.  Borrows `map` (an OccGridMap), which stays usable through its own methods between calls."""

    def __init__(self, map: "OccGridMap"):
        self.map, self.ctx, self.L = map, map.ctx, map.L
        h = C.c_void_p()
        self.ctx.check(self.L.lslam_hector_create(map.h, C.byref(h)))
        self.h = h
        if not hasattr(map, "_processors"):
            map._processors = []
        map._processors.append(self)

    def close(self):
        if getattr(self, "h", None):
            for fleet in list(getattr(self, "_fleets", ())):  # a HectorFleet borrows its processors
                fleet.close()
            self.L.lslam_hector_destroy(self.h)
            self.h = None
            if self in getattr(self.map, "_processors", ()):
                self.map._processors.remove(self)

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx.check(self.L.lslam_hector_reset(self.h))

    def set_update_thresholds(self, min_dist: float, min_angle: float):
        self.ctx.check(self.L.lslam_hector_set_update_thresholds(self.h, min_dist, min_angle))

    def set_option(self, name: str, value: int):
        """'fabs_angle_gate': compare fabsf of the wrapped heading difference instead of the reference toolchain's abs(int)."""
        self.ctx.check(self.L.lslam_hector_set_option(self.h, {"fabs_angle_gate": 1}[name], int(value)))

    @staticmethod
    def _hints_flags(n, pose_hints, map_without_matching):
        hints = None if pose_hints is None else np.ascontiguousarray(pose_hints, dtype=np.float32).reshape(n, 3)
        if map_without_matching is None:
            flags = None
        else:
            flags = np.ascontiguousarray(np.broadcast_to(np.asarray(map_without_matching, dtype=np.uint8), (n,)))
        return hints, flags

    def process_many(self, ranges, scan: HectorScan, pose_hints=None, map_without_matching=None) -> np.ndarray:
        """ranges: [n_scans, n_readings] float32 LaserScans -> HECTOR_RECORD[n_scans].  pose_hints None: chained."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        r = r.reshape(-1, r.shape[-1]) if r.ndim != 2 else r
        n = r.shape[0]
        hints, flags = self._hints_flags(n, pose_hints, map_without_matching)
        out = np.zeros(n, HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_process_many(
            self.h, C.byref(scan), n, r.shape[1], r.ctypes.data, r.shape[1], None if hints is None else hints.ctypes.data,
            None if flags is None else flags.ctypes.data, out.ctypes.data))
        return out

    def process_deskewed(self, ranges, scan: HectorScan, params, imu_times=None, imu_rots=None, pose_hints=None,
                         map_without_matching=None) -> np.ndarray:
        """ranges: [n_scans, n_readings] RAW LaserScans + what Deskewer.batch takes -> HECTOR_RECORD[n_scans]: one batched
        de-skew launch, then cloud -> container, match, mark and apply per scan; one host synchronisation."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        r = r.reshape(len(params), -1) if len(params) else r.reshape(0, r.shape[-1] if r.ndim > 1 else 0)
        n = r.shape[0]
        hints, flags = self._hints_flags(n, pose_hints, map_without_matching)
        arr, first, it, ir = _deskew_inputs(params, imu_times, imu_rots)
        out = np.zeros(n, HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_process_many_deskewed(
            self.h, C.byref(scan), n, r.shape[1], r.ctypes.data, r.shape[1], C.addressof(arr), first.ctypes.data, it.ctypes.data,
            ir[0].ctypes.data, ir[1].ctypes.data, ir[2].ctypes.data, None if hints is None else hints.ctypes.data,
            None if flags is None else flags.ctypes.data, out.ctypes.data))
        return out

    def process_many_clouds(self, xyz, scan: HectorScan, valid=None, take=None, pose_hints=None, map_without_matching=None) -> np.ndarray:
        """xyz: [n_scans, n_points, 3] float32 clouds in the de-skew's layout (Deskewer.batch, MotionSync.scans), valid
        [n_scans, n_points] or None = every point, take [n_scans] or None = every scan -> HECTOR_RECORD[n_scans].  A scan with
        take == 0 changes nothing of the processor; its record is zero with n_points = -1."""
        x = np.ascontiguousarray(xyz, dtype=np.float32)
        if x.ndim != 3 or x.shape[2] != 3:
            raise ValueError("xyz must be [n_scans, n_points, 3]")
        n, npts = x.shape[0], x.shape[1]
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid).astype(bool).astype(np.uint8)).reshape(n, npts)
        t = None if take is None else np.ascontiguousarray(np.asarray(take).astype(bool).astype(np.uint8)).reshape(n)
        hints, flags = self._hints_flags(n, pose_hints, map_without_matching)
        out = np.zeros(n, HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_process_many_clouds(
            self.h, C.byref(scan), n, npts, x.ctypes.data, None if v is None else v.ctypes.data,
            None if t is None else t.ctypes.data, None if hints is None else hints.ctypes.data,
            None if flags is None else flags.ctypes.data, out.ctypes.data))
        return out

    def process_many_clouds_dev(self, n_scans: int, n_points: int, xyz_ptr: int, valid_ptr, take_ptr, take_stride: int,
                                scan: HectorScan, pose_hints=None, map_without_matching=None) -> np.ndarray:
        """The same on clouds in HBM (xyz float32, valid uint8 or None).  take_ptr: int32 words in HBM, scan k is taken iff
        word k * take_stride is > 0 (None: every scan) -- the `status` field of an MSYNC_RECORD array with take_stride =
        MSYNC_RECORD.itemsize // 4 serves as it stands."""
        hints, flags = self._hints_flags(n_scans, pose_hints, map_without_matching)
        out = np.zeros(n_scans, HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_process_many_clouds_dev(
            self.h, C.byref(scan), n_scans, n_points, xyz_ptr, valid_ptr, take_ptr, int(take_stride),
            None if hints is None else hints.ctypes.data, None if flags is None else flags.ctypes.data, out.ctypes.data))
        return out

    def process_synced(self, sync: "MotionSync", laser, ranges, scan: HectorScan, stamps, time_increments, imu_seen=None,
                       odom_seen=None, pose_hints=None, map_without_matching=None, n_readings=None):
        """n ScanCallbacks of lesson5's node (what MotionSync.scans takes; the IMU and odometry messages pushed into `sync`
        before) chained into update(): -> (HECTOR_RECORD[n], MSYNC_RECORD[n]), record k of both for callback k.  A callback
        whose status is not MSYNC_CORRECTED changes nothing of the processor.  One host synchronisation."""
        hdr, t, ti, seen = MotionSync._small(laser, stamps, time_increments, imu_seen, odom_seen)
        n = len(t)
        r = np.ascontiguousarray(ranges, dtype=np.float32).reshape(n, -1) if n else np.zeros((0, 0), np.float32)
        stride = r.shape[1]
        nr = stride if n_readings is None else int(n_readings)
        hints, flags = self._hints_flags(n, pose_hints, map_without_matching)
        out, rec = np.zeros(n, HECTOR_RECORD), np.zeros(n, MSYNC_RECORD)
        self.ctx.check(self.L.lslam_hector_process_many_synced(
            self.h, sync.h, C.byref(scan), C.byref(hdr), n, nr, r.ctypes.data, stride, t.ctypes.data, ti.ctypes.data,
            None if seen[0] is None else seen[0].ctypes.data, None if seen[1] is None else seen[1].ctypes.data,
            None if hints is None else hints.ctypes.data, None if flags is None else flags.ctypes.data, out.ctypes.data,
            rec.ctypes.data))
        return out, rec

    def process_many_points(self, containers, pose_hints=None, map_without_matching=None, origos_xy=None, counts=None) -> np.ndarray:
        """containers: a list of (n, 2) float32 arrays in level-0 cell units, or -- with `counts` -- one packed array."""
        if counts is None:
            counts = np.array([len(p) for p in containers], dtype=np.int32)
            pts = (np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in containers])
                   if len(containers) else np.zeros((0, 2), np.float32))
        else:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            pts = np.asarray(containers, dtype=np.float32).reshape(-1, 2)
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        n = len(counts)
        hints, flags = self._hints_flags(n, pose_hints, map_without_matching)
        o = None if origos_xy is None else np.ascontiguousarray(np.broadcast_to(np.asarray(origos_xy, dtype=np.float32), (n, 2)))
        out = np.zeros(n, HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_process_many_points(
            self.h, n, pts.ctypes.data, counts.ctypes.data, None if o is None else o.ctypes.data,
            None if hints is None else hints.ctypes.data, None if flags is None else flags.ctypes.data, out.ctypes.data))
        return out

    def process(self, points_xy, pose_hint=None, map_without_matching=False, origo_xy=(0.0, 0.0)):
        """HectorSlamProcessor::update for one container (a call of one) -> its record."""
        rec = self.process_many_points([points_xy], None if pose_hint is None else [pose_hint], [map_without_matching],
                                       [origo_xy])
        return rec[0]

    def state(self):
        """-> (lastScanMatchPose[3], lastScanMatchCov[3,3], lastMapUpdatePose[3])"""
        pose, cov, upd = np.zeros(3, np.float32), np.zeros(9, np.float32), np.zeros(3, np.float32)
        self.ctx.check(self.L.lslam_hector_state(self.h, pose.ctypes.data, cov.ctypes.data, upd.ctypes.data))
        return pose, cov.reshape(3, 3), upd

    def stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self.ctx.check(self.L.lslam_hector_stats(self.h, out))
        return dict(zip(("scans", "map_updates", "calls", "host_syncs"), (int(v) for v in out)))


class HectorFleet:
    """R HectorProcessors, each on its own map, advanced one scan each per step with the launches of ONE processor's chain
    (lslam_hector_fleet_*).  Borrows the processors: each keeps its state, thresholds, options and map, and stays usable on
    its own between fleet calls.  Per-scan arrays are [n_steps, R, ...]; `active` [n_steps, R] marks the scans that exist (a
    scan that does not changes nothing of its member and comes back as a zero record with n_points = -1)."""

    def __init__(self, processors):
        self.processors = list(processors)
        if not self.processors:
            raise LslamError(-1, "a fleet needs at least one processor")
        self.ctx, self.L = self.processors[0].ctx, self.processors[0].L
        arr = (C.c_void_p * len(self.processors))(*[p.h for p in self.processors])
        h = C.c_void_p()
        self.ctx.check(self.L.lslam_hector_fleet_create(arr, len(self.processors), C.byref(h)))
        self.h = h
        for p in self.processors:
            p.__dict__.setdefault("_fleets", []).append(self)

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_hector_fleet_destroy(self.h)
            self.h = None
            for p in self.processors:
                if self in getattr(p, "_fleets", ()):
                    p._fleets.remove(self)

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    @property
    def size(self) -> int:
        return int(self.L.lslam_hector_fleet_size(self.h))

    def _per_scan(self, n_steps, pose_hints, map_without_matching, active):
        n = n_steps * len(self.processors)
        hints = None if pose_hints is None else np.ascontiguousarray(pose_hints, dtype=np.float32).reshape(n, 3)
        flags, act = (None if a is None else
                      np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.uint8), (n_steps, len(self.processors)))).reshape(n)
                      for a in (map_without_matching, active))
        return hints, flags, act

    def process_many(self, ranges, scan: HectorScan, pose_hints=None, map_without_matching=None, active=None) -> np.ndarray:
        """ranges: [n_steps, R, n_readings] float32 LaserScans of one geometry -> HECTOR_RECORD[n_steps, R]."""
        R = len(self.processors)
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        r = r.reshape(-1, R, r.shape[-1])
        n_steps = r.shape[0]
        hints, flags, act = self._per_scan(n_steps, pose_hints, map_without_matching, active)
        out = np.zeros((n_steps, R), HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_fleet_process_many(
            self.h, C.byref(scan), n_steps, r.shape[2], r.ctypes.data, r.shape[2], None if hints is None else hints.ctypes.data,
            None if flags is None else flags.ctypes.data, None if act is None else act.ctypes.data, out.ctypes.data))
        return out

    def process_many_points(self, containers, pose_hints=None, map_without_matching=None, active=None, origos_xy=None,
                            counts=None) -> np.ndarray:
        """containers[step][member]: (n, 2) float32 arrays in the member's level-0 cell units (None or empty where the scan
        is not active), or -- with `counts` [n_steps, R] -- one packed array in step-major order."""
        R = len(self.processors)
        if counts is None:
            flat = [np.zeros((0, 2), np.float32) if p is None else np.asarray(p, dtype=np.float32).reshape(-1, 2)
                    for row in containers for p in row]
            assert len(flat) % R == 0, "every step needs one container per member"
            counts = np.array([len(p) for p in flat], dtype=np.int32)
            pts = np.concatenate(flat) if flat else np.zeros((0, 2), np.float32)
        else:
            counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
            pts = np.asarray(containers, dtype=np.float32).reshape(-1, 2)
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        n_steps = len(counts) // R
        n = n_steps * R
        hints, flags, act = self._per_scan(n_steps, pose_hints, map_without_matching, active)
        o = None if origos_xy is None else np.ascontiguousarray(np.broadcast_to(np.asarray(origos_xy, dtype=np.float32), (n_steps, R, 2)))
        out = np.zeros((n_steps, R), HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_fleet_process_many_points(
            self.h, n_steps, pts.ctypes.data, counts.ctypes.data, None if o is None else o.ctypes.data,
            None if hints is None else hints.ctypes.data, None if flags is None else flags.ctypes.data,
            None if act is None else act.ctypes.data, out.ctypes.data))
        return out

    def process_many_clouds(self, xyz, scan: HectorScan, valid=None, take=None, pose_hints=None, map_without_matching=None,
                            active=None) -> np.ndarray:
        """xyz: [n_steps, R, n_points, 3] float32 clouds in the de-skew's layout, valid [n_steps, R, n_points] or None = every
        point, take [n_steps, R] or None = every scan -> HECTOR_RECORD[n_steps, R].  An entry is taken iff it is active and its
        take flag is set; one that is not changes nothing of its member (record: zero with n_points = -1)."""
        R = len(self.processors)
        x = np.ascontiguousarray(xyz, dtype=np.float32)
        if x.ndim != 4 or x.shape[1] != R or x.shape[3] != 3:
            raise ValueError("xyz must be [n_steps, R, n_points, 3]")
        n_steps, npts = x.shape[0], x.shape[2]
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid).astype(bool).astype(np.uint8)).reshape(n_steps, R, npts)
        t = None if take is None else np.ascontiguousarray(np.asarray(take).astype(bool).astype(np.uint8)).reshape(n_steps, R)
        hints, flags, act = self._per_scan(n_steps, pose_hints, map_without_matching, active)
        out = np.zeros((n_steps, R), HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_fleet_process_many_clouds(
            self.h, C.byref(scan), n_steps, npts, x.ctypes.data, None if v is None else v.ctypes.data,
            None if t is None else t.ctypes.data, None if hints is None else hints.ctypes.data,
            None if flags is None else flags.ctypes.data, None if act is None else act.ctypes.data, out.ctypes.data))
        return out

    def process_many_clouds_dev(self, n_steps: int, n_points: int, xyz_ptrs, valid_ptrs, take_ptrs, take_stride: int,
                                scan: HectorScan, pose_hints=None, map_without_matching=None, active=None) -> np.ndarray:
        """The same on clouds in HBM.  xyz_ptrs / valid_ptrs / take_ptrs: R device addresses each, one block per member (R
        MotionSync.scans_dev outputs, or slices of one block); member m's row of step k is k rows into its block.  valid_ptrs,
        take_ptrs or single entries of them may be None (every point valid / every scan taken).  take words are int32, taken
        iff > 0, take_stride words apart: the `status` field of an MSYNC_RECORD array with MSYNC_RECORD.itemsize // 4."""
        R = len(self.processors)

        def table(ptrs):
            if ptrs is None:
                return None
            assert len(ptrs) == R, "one device pointer per member"
            return (C.c_void_p * R)(*[p or None for p in ptrs])

        x, v, t = table(xyz_ptrs), table(valid_ptrs), table(take_ptrs)
        hints, flags, act = self._per_scan(n_steps, pose_hints, map_without_matching, active)
        out = np.zeros((n_steps, R), HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_fleet_process_many_clouds_dev(
            self.h, C.byref(scan), int(n_steps), int(n_points), x, v, t, int(take_stride),
            None if hints is None else hints.ctypes.data, None if flags is None else flags.ctypes.data,
            None if act is None else act.ctypes.data, out.ctypes.data))
        return out

    def process_synced(self, syncs, laser, ranges, scan: HectorScan, stamps, time_increments, imu_seen=None, odom_seen=None,
                       pose_hints=None, map_without_matching=None, active=None, n_readings=None):
        """Raw messages in for R robots: syncs[R] are the members' MotionSync nodes (their IMU and odometry pushed before);
        ranges [n_steps, R, stride], stamps / time_increments / imu_seen / odom_seen [n_steps, R] -- member m's ScanCallbacks of
        the call are its steps with active != 0, in step order -> (HECTOR_RECORD[n_steps, R], MSYNC_RECORD[n_steps, R]).  The
        synchronisation and the de-skew of all members run in 5 launches per call; one host synchronisation."""
        R = len(self.processors)
        syncs = list(syncs)
        assert len(syncs) == R, "one MotionSync per member"
        hdr = laser if isinstance(laser, MsyncLaser) else MsyncLaser(*[float(v) for v in laser])
        t = np.ascontiguousarray(stamps, np.float64).reshape(-1, R)
        n_steps = t.shape[0]
        ti = np.ascontiguousarray(time_increments, np.float32).reshape(n_steps, R)
        seen = [None if a is None else np.ascontiguousarray(a, np.int64).reshape(n_steps, R) for a in (imu_seen, odom_seen)]
        r = np.ascontiguousarray(ranges, dtype=np.float32).reshape(n_steps, R, -1)
        stride = r.shape[2]
        nr = stride if n_readings is None else int(n_readings)
        hints, flags, act = self._per_scan(n_steps, pose_hints, map_without_matching, active)
        arr = (C.c_void_p * R)(*[s.h for s in syncs])
        out, rec = np.zeros((n_steps, R), HECTOR_RECORD), np.zeros((n_steps, R), MSYNC_RECORD)
        self.ctx.check(self.L.lslam_hector_fleet_process_many_synced(
            self.h, arr, C.byref(scan), C.byref(hdr), n_steps, nr, r.ctypes.data, stride, t.ctypes.data, ti.ctypes.data,
            None if seen[0] is None else seen[0].ctypes.data, None if seen[1] is None else seen[1].ctypes.data,
            None if hints is None else hints.ctypes.data, None if flags is None else flags.ctypes.data,
            None if act is None else act.ctypes.data, out.ctypes.data, rec.ctypes.data))
        return out, rec

    def sync_stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self.ctx.check(self.L.lslam_hector_fleet_sync_stats(self.h, out))
        return dict(zip(("calls", "launches", "growths", "host_waits"), (int(v) for v in out)))

    def stats(self) -> dict:
        out = (C.c_int64 * 6)()
        self.ctx.check(self.L.lslam_hector_fleet_stats(self.h, out))
        return dict(zip(("steps", "scans", "map_updates", "calls", "host_syncs", "launches"), (int(v) for v in out)))


class HectorLocaliser:
    """R trackers localising on ONE finished map (lslam_hector_loc_*): each entry is HectorSlamProcessor::update with the gate
    never firing -- matchData from the hint or the tracker's own last pose, no map update.  Borrows `map` (an OccGridMap),
    which it only reads and which stays usable, and changeable, through its own methods between calls.  Per-entry arrays are
    [n_steps, R, ...] as in HectorFleet; an entry that is not taken leaves its tracker alone (record: zero, n_points = -1)."""

    def __init__(self, map: "OccGridMap", n_trackers: int):
        self.map, self.ctx, self.L = map, map.ctx, map.L
        h = C.c_void_p()
        self.ctx.check(self.L.lslam_hector_loc_create(map.h, int(n_trackers), C.byref(h)))
        self.h = h
        self.n_trackers = int(n_trackers)
        if not hasattr(map, "_processors"):
            map._processors = []
        map._processors.append(self)  # closed with the map, before it

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_hector_loc_destroy(self.h)
            self.h = None
            if self in getattr(self.map, "_processors", ()):
                self.map._processors.remove(self)

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    @property
    def size(self) -> int:
        return int(self.L.lslam_hector_loc_size(self.h))

    def set_poses(self, poses_xyh, first: int = 0):
        """lastScanMatchPose of trackers first .. first + len(poses) - 1."""
        p = np.ascontiguousarray(poses_xyh, dtype=np.float32).reshape(-1, 3)
        self.ctx.check(self.L.lslam_hector_loc_set_poses(self.h, int(first), p.shape[0], p.ctypes.data))

    def state(self, tracker: int):
        """-> (lastScanMatchPose[3], lastScanMatchCov[3,3]) of one tracker"""
        pose, cov = np.zeros(3, np.float32), np.zeros(9, np.float32)
        self.ctx.check(self.L.lslam_hector_loc_state(self.h, int(tracker), pose.ctypes.data, cov.ctypes.data))
        return pose, cov.reshape(3, 3)

    def set_option(self, name: str, value: int):
        """'max_steps_per_launch': steps per chunk of a call (0: the default, from the 64 MiB container budget)."""
        self.ctx.check(self.L.lslam_hector_loc_set_option(self.h, {"max_steps_per_launch": 1}[name], int(value)))

    def stats(self) -> dict:
        out = (C.c_int64 * 6)()
        self.ctx.check(self.L.lslam_hector_loc_stats(self.h, out))
        return dict(zip(("steps", "scans", "calls", "host_syncs", "launches", "track_launches"), (int(v) for v in out)))

    def _per_entry(self, n_steps, pose_hints, active):
        R = self.n_trackers
        hints = None if pose_hints is None else np.ascontiguousarray(pose_hints, dtype=np.float32).reshape(n_steps * R, 3)
        act = None if active is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(active, dtype=np.uint8), (n_steps, R))).reshape(n_steps * R)
        return hints, act

    def process_many(self, ranges, scan: HectorScan, pose_hints=None, active=None) -> np.ndarray:
        """ranges: [n_steps, R, n_readings] float32 LaserScans of one geometry -> HECTOR_RECORD[n_steps, R]."""
        R = self.n_trackers
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        r = r.reshape(-1, R, r.shape[-1])
        n_steps = r.shape[0]
        hints, act = self._per_entry(n_steps, pose_hints, active)
        out = np.zeros((n_steps, R), HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_loc_process_many(
            self.h, C.byref(scan), n_steps, r.shape[2], r.ctypes.data, r.shape[2], None if hints is None else hints.ctypes.data,
            None if act is None else act.ctypes.data, out.ctypes.data))
        return out

    def process_many_points(self, containers, pose_hints=None, active=None, counts=None) -> np.ndarray:
        """containers[step][tracker]: (n, 2) float32 arrays in level-0 cell units (None or empty where the entry is not
        active), or -- with `counts` [n_steps, R] -- one packed array in step-major order."""
        R = self.n_trackers
        if counts is None:
            flat = [np.zeros((0, 2), np.float32) if p is None else np.asarray(p, dtype=np.float32).reshape(-1, 2)
                    for row in containers for p in row]
            assert len(flat) % R == 0, "every step needs one container per tracker"
            counts = np.array([len(p) for p in flat], dtype=np.int32)
            pts = np.concatenate(flat) if flat else np.zeros((0, 2), np.float32)
        else:
            counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
            pts = np.asarray(containers, dtype=np.float32).reshape(-1, 2)
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        n_steps = len(counts) // R
        hints, act = self._per_entry(n_steps, pose_hints, active)
        out = np.zeros((n_steps, R), HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_loc_process_many_points(
            self.h, n_steps, pts.ctypes.data, counts.ctypes.data, None if hints is None else hints.ctypes.data,
            None if act is None else act.ctypes.data, out.ctypes.data))
        return out

    def process_many_clouds(self, xyz, scan: HectorScan, valid=None, take=None, pose_hints=None, active=None) -> np.ndarray:
        """xyz: [n_steps, R, n_points, 3] float32 clouds in the de-skew's layout, valid [n_steps, R, n_points] or None = every
        point, take [n_steps, R] or None = every entry -> HECTOR_RECORD[n_steps, R]."""
        R = self.n_trackers
        x = np.ascontiguousarray(xyz, dtype=np.float32)
        if x.ndim != 4 or x.shape[1] != R or x.shape[3] != 3:
            raise ValueError("xyz must be [n_steps, R, n_points, 3]")
        n_steps, npts = x.shape[0], x.shape[2]
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid).astype(bool).astype(np.uint8)).reshape(n_steps, R, npts)
        t = None if take is None else np.ascontiguousarray(np.asarray(take).astype(bool).astype(np.uint8)).reshape(n_steps, R)
        hints, act = self._per_entry(n_steps, pose_hints, active)
        out = np.zeros((n_steps, R), HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_loc_process_many_clouds(
            self.h, C.byref(scan), n_steps, npts, x.ctypes.data, None if v is None else v.ctypes.data,
            None if t is None else t.ctypes.data, None if hints is None else hints.ctypes.data,
            None if act is None else act.ctypes.data, out.ctypes.data))
        return out

    def process_many_clouds_dev(self, n_steps: int, n_points: int, xyz_ptr: int, valid_ptr, take_ptr, take_stride: int,
                                scan: HectorScan, pose_hints=None, active=None) -> np.ndarray:
        """The same on clouds in HBM: xyz [n_steps * R, n_points, 3] float32, valid uint8 or None, take_ptr int32 words
        take_stride apart or None; entry i is taken iff it is active and word i * take_stride is > 0 -- the `status` field of
        an MSYNC_RECORD array with take_stride = MSYNC_RECORD.itemsize // 4 serves as it stands."""
        hints, act = self._per_entry(int(n_steps), pose_hints, active)
        out = np.zeros((int(n_steps), self.n_trackers), HECTOR_RECORD)
        self.ctx.check(self.L.lslam_hector_loc_process_many_clouds_dev(
            self.h, C.byref(scan), int(n_steps), int(n_points), xyz_ptr, valid_ptr, take_ptr, int(take_stride),
            None if hints is None else hints.ctypes.data, None if act is None else act.ctypes.data, out.ctypes.data))
        return out


class GMappingMap:
    """lesson4's GMapping ScanMatcherMap (hit / visit counts + float hit-position sums per cell) on the GPU, with the
    lesson4_gmapping_node callback (gmapping.cc:127-242) as compute_map.  Ranges are float32; poses (x, y, theta)."""

    NODE = dict(xmin=-40.0, ymin=-40.0, xmax=40.0, ymax=40.0, delta=0.05, max_range=30 - 0.01, max_use_range=25.0,
                occ_thresh=0.25)  # GMapping::InitParams (gmapping.cc:44-62)

    def __init__(self, ctx: Context, xmin=-40.0, ymin=-40.0, xmax=40.0, ymax=40.0, delta=0.05):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        ctx.check(ctx.L.lslam_gmap_create(ctx.h, float(xmin), float(ymin), float(xmax), float(ymax), float(delta), C.byref(h)))
        self.h = h
        ctx._adopt(self)
        g = GMapGeometry()
        ctx.check(ctx.L.lslam_gmap_info(self.h, C.byref(g)))
        self.info = {k: getattr(g, k) for k, _ in GMapGeometry._fields_}
        self.n_beams = 0

    @property
    def storage_shape(self):
        return self.info["map_size_y"], self.info["map_size_x"]

    def set_laser(self, n_beams: int, angle_min: float, angle_increment: float, max_range=30 - 0.01, max_use_range=25.0):
        """CreateCache: the message's float32 angle fields."""
        self.ctx.check(self.L.lslam_gmap_set_laser(self.h, int(n_beams), float(angle_min), float(angle_increment),
                                                   float(max_range), float(max_use_range)))
        self.n_beams = int(n_beams)

    def angle_cache(self):
        c, s = np.zeros(self.n_beams), np.zeros(self.n_beams)
        self.ctx.check(self.L.lslam_gmap_angle_cache(self.h, c.ctypes.data, s.ctypes.data))
        return c, s

    def reset(self):
        self.ctx.check(self.L.lslam_gmap_reset(self.h))

    def _ranges(self, ranges):
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        if r.ndim == 1:
            r = r.reshape(1, -1)
        if r.ndim != 2 or (r.shape[0] > 0 and r.shape[1] != self.n_beams):
            raise ValueError(f"ranges must be [n_scans, {self.n_beams}] float32")
        return r

    def integrate(self, ranges, poses=None):
        """n_scans x n_beams readings at poses (n_scans x 3; None = all at the origin), applied in order."""
        r = self._ranges(ranges)
        p = None
        if poses is not None:
            p = _f64(poses).reshape(-1, 3)
            if p.shape[0] != r.shape[0]:
                raise ValueError("one pose per scan")
        self.ctx.check(self.L.lslam_gmap_integrate(self.h, r.shape[0], r.ctypes.data, None if p is None else p.ctypes.data))

    def compute_map(self, ranges, occ_thresh: float = 0.25) -> np.ndarray:
        """The node's callback: reset, one scan at the origin, the published int8 grid [height, width]."""
        r = self._ranges(ranges)
        if r.shape[0] != 1:
            raise ValueError("compute_map takes one scan")
        out = np.empty((self.info["height"], self.info["width"]), np.int8)
        self.ctx.check(self.L.lslam_gmap_compute_map(self.h, r.ctypes.data, float(occ_thresh), out.ctypes.data))
        return out

    def ros_i8(self, occ_thresh: float = 0.25) -> np.ndarray:
        out = np.empty((self.info["height"], self.info["width"]), np.int8)
        self.ctx.check(self.L.lslam_gmap_read_ros_i8(self.h, float(occ_thresh), out.ctypes.data))
        return out

    def counters(self):
        """-> visits, n (int32), acc_x, acc_y (float32), each [map_size_y, map_size_x]"""
        shape = self.storage_shape
        v, n = np.empty(shape, np.int32), np.empty(shape, np.int32)
        acc = np.empty((2,) + shape, np.float32)
        self.ctx.check(self.L.lslam_gmap_read_counters(self.h, v.ctypes.data, n.ctypes.data, acc.ctypes.data))
        return v, n, acc[0], acc[1]

    def patch_mask(self) -> np.ndarray:
        out = np.empty((self.info["patches_y"], self.info["patches_x"]), np.uint8)
        self.ctx.check(self.L.lslam_gmap_read_patch_mask(self.h, out.ctypes.data))
        return out

    def stats(self) -> dict:
        out = np.zeros(4, np.int64)
        self.ctx.check(self.L.lslam_gmap_stats(self.h, out.ctypes.data))
        return dict(scans=int(out[0]), beams=int(out[1]), hits=int(out[2]), dropped=int(out[3]))

    def close(self):
        if getattr(self, "h", None):
            self.L.lslam_gmap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass
