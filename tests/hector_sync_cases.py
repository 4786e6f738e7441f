"""Scenarios for the gated streamed processor (lslam_hector_process_many_clouds[_dev], lslam_hector_process_many_synced;
api.HectorProcessor.process_many_clouds[_dev] / process_synced): lesson5's message logs of tests/msync_cases.py chained into
lesson4's HectorSlamProcessor on the maps of tests/deskew_stream_cases.py.

STATUSES[name] is the status of every scan callback of a log as tests/msync_restatement.py gives it (0 queued, 1 corrected,
negative refused); tests/test_hector_sync_cases_oracle.py holds the restatement to these rows on the CPU, so the GPU tests may
rest their coverage claims on them:

  steady        no refusal
  imu_gap       isolated refusals, the first right behind the first taken scan (which always updates the map)
  non_monotone  runs of two and of three refusals, of both kinds
  no_lead       one refusal in mid-stream (a sample inside the scan, none before its start)
  window_sizes  the LAST callback refused
  wide          1081 beams: both 1024-beam compaction rounds of the container kernel; no refusal

Pure numpy; the device API is handed in by the caller."""
import functools

import numpy as np

import deskew_stream_cases as D
import hector_stream_cases as S
import msync_cases as mc

f32 = np.float32
STATUSES = {
    "steady": [0] + [1] * 13,
    "imu_gap": [0, 1, -1, 1, -1, 1, 1, -1, 1, 1, 1, 1],
    "non_monotone": [0, 1, 1, 1, -1, -1, 1, -1, -2, -2, 1, -2, 1, 1],
    "no_lead": [0, 1, 1, 1, 1, 1, -3, 1, 1, 1],
    "window_sizes": [0, 1, 1, 1, 1, 1, 1, -4],
    "wide": [0] + [1] * 5,
}
CHUNKS = [1, 4, 1, 3, 5]  # of non_monotone: ends behind the queued callback, inside the first run of refusals, just past it, and
#                           inside the second run
TAKE_PATTERNS = {
    "all": [1] * 12,
    "none": [0] * 12,
    "first_not": [0] + [1] * 11,
    "last_not": [1] * 11 + [0],
    "mixed": [1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 1, 0],
}
LEVELS = {"steady": 3, "imu_gap": 2, "non_monotone": 3, "no_lead": 2, "window_sizes": 3, "wide": 2}  # 2 and 3 levels, both used


@functools.lru_cache(maxsize=None)
def wide():
    return mc._case(n=1081, n_scans=6, imu_hz=200.0, odom_hz=20.0, lag=0.05, seed=14)


def case(name):
    return wide() if name == "wide" else mc.CASES[name]()


class Laser:
    """What deskew_stream_cases.hector_scan reads of a laser, from a log's LaserScan header."""

    def __init__(self, c):
        self.angle_min, self.angle_increment, self.range_min, self.range_max = (float(v) for v in c["laser"])
        self.n_ranges = c["ranges"].shape[1]


def hector_scan(c):
    return D.hector_scan(Laser(c))


def push_all(ms, c):
    ms.push_imu(c["imu_t"], c["imu_w"])
    ms.push_odom(c["odom_t"], c["odom_pos"], c["odom_quat"])


def scan_args(c, lo=0, hi=None):
    """(ranges, stamps, time_increments, imu_seen, odom_seen) of callbacks [lo, hi) -- what MotionSync.scans and
    HectorProcessor.process_synced take behind the laser header."""
    return c["ranges"][lo:hi], c["scan_t"][lo:hi], c["scan_tinc"][lo:hi], c["imu_seen"][lo:hi], c["odom_seen"][lo:hi]


def snapshot(m, h):
    """Everything of a processor and its map a scan may change, as bytes."""
    pts, origo = m.container()
    return {"planes": [m.logodds(lv).tobytes() for lv in range(m.levels)], "state": [a.tobytes() for a in h.state()],
            "container": pts.tobytes(), "origo": origo.tobytes(), "cached_points": m.cached_points()}


def not_taken(rec):
    """A record the gated chain wrote for a scan it did not take: all zero except n_points = -1."""
    z = np.zeros(1, rec.dtype)
    z["n_points"] = -1
    return rec.tobytes() == z[0].tobytes()
