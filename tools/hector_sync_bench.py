#!/usr/bin/env python3
"""Raw IMU, odometry and LaserScan messages in, Hector poses and a map out: tools/msync_bench.py's message rates
(1081 beams, 400 Hz IMU, 50 Hz odometry) on tools/hector_stream_bench.py's pyramid (1024^2, 3 levels), 300 scan callbacks, in
calls of 16 and in one call of 300, through

  (a) HectorProcessor.process_synced: the node's callbacks, the de-skew and the gated chain in one call, one wait,
  (b) MotionSync.scans in its host form (clouds down) + HectorProcessor.process_many_clouds with take = status == 1 (clouds up
      again), two waits per call, and
  (c) MotionSync.scans + the host-driven loop per corrected cloud (setCloud -> matchContainer -> updateByContainer, three
      blocking round trips per scan) -- the only route before the gated chain existed.

Every route and call size is warmed up first; the routes then alternate REPEATS times in one process, timed with a host clock
around calls that end in the library's own wait, the pushes of the messages included.  The JSON line carries median, min and
max per route in microseconds per scan callback, whether (a) and (b) gave the same bytes, and -- from the library's launch
profile of one call of 16 -- the launches per call.  No threshold: the figures are reported.
Usage: python tools/hector_sync_bench.py [--scans 300] [--repeats 7]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))  # msync_bench imports the restatement
sys.path.insert(0, str(ROOT / "tools"))
import lslam  # noqa: E402,F401
from lslam_amd import api  # noqa: E402
import msync_bench  # noqa: E402


class Laser:
    def __init__(self, hdr):
        self.angle_min, self.angle_increment, self.range_min, self.range_max = (float(v) for v in hdr)


def spread_us(times, scans):
    return {k: round(1e6 * v / scans, 2) for k, v in msync_bench.spread(times).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    log = msync_bench.make_log(a.scans)
    n, cell, levels = 1024, 0.05, 3
    off = (n * cell * 0.5, n * cell * 0.5)
    scan = api.hector_scan(Laser(log["laser"]), z_min=-1.0, z_max=2.0)  # lesson5's cloud has z ~ 1
    ctx = api.Context(0)  # raises without a GPU: nothing here is measured on a CPU
    gmap = api.OccGridMap(ctx, n, n, cell, off, levels=levels)
    gmap.setUpdateOccupiedFactor(0.9)
    proc = api.HectorProcessor(gmap)
    proc.set_update_thresholds(-1.0, -1.0)  # every taken scan updates the map
    ms = api.MotionSync(ctx)

    def args(lo, hi):
        return log["ranges"][lo:hi], log["scan_t"][lo:hi], log["scan_tinc"][lo:hi], log["imu_seen"][lo:hi], log["odom_seen"][lo:hi]

    def start():
        ms.reset()
        proc.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        ms.push_imu(log["imu_t"], log["imu_w"])
        ms.push_odom(log["odom_t"], log["odom_pos"], log["odom_quat"])
        return t0

    def route_a(chunk):
        t0, out = start(), []
        for k in range(0, a.scans, chunk):
            r, t, ti, iseen, oseen = args(k, k + chunk)
            out.append(proc.process_synced(ms, log["laser"], r, scan, t, ti, iseen, oseen)[0])
        return time.perf_counter() - t0, np.concatenate(out)

    def route_b(chunk):
        t0, out = start(), []
        for k in range(0, a.scans, chunk):
            xyz, valid, rec = ms.scans(log["laser"], *args(k, k + chunk))
            out.append(proc.process_many_clouds(xyz, scan, valid, take=rec["status"] == api.MSYNC_CORRECTED))
        return time.perf_counter() - t0, np.concatenate(out)

    def route_c(chunk):
        t0, poses = start(), []
        est = np.zeros(3, np.float32)
        for k in range(0, a.scans, chunk):
            xyz, valid, rec = ms.scans(log["laser"], *args(k, k + chunk))
            for j in np.flatnonzero(rec["status"] == api.MSYNC_CORRECTED):
                if gmap.setCloud(xyz[j], valid[j], scan) > 0:
                    est, _ = gmap.matchContainer(est)
                gmap.updateByContainer(est)
                poses.append(est.copy())
        ctx.synchronize()
        return time.perf_counter() - t0, np.array(poses)

    res = {"config": "lesson5 node -> lesson4 HectorSlamProcessor: 1081 beams, 400 Hz IMU, 50 Hz odometry, 1024^2 x 3 levels",
           "scans": a.scans, "repeats": a.repeats, "unit": "us per scan callback"}
    for chunk in (16, a.scans):
        routes = (("a_process_synced", route_a), ("b_msync_then_clouds", route_b), ("c_msync_then_host_loop", route_c))
        warm = {name: fn(chunk)[1] for name, fn in routes}
        times = {name: [] for name, _ in routes}
        for _ in range(a.repeats):  # alternating
            for name, fn in routes:
                times[name].append(fn(chunk)[0])
        taken = warm["a_process_synced"]["n_points"] >= 0
        leg = {name: spread_us(ts, a.scans) for name, ts in times.items()}
        leg["a_equals_b_bytes"] = bool(warm["a_process_synced"].tobytes() == warm["b_msync_then_clouds"].tobytes())
        leg["taken"] = int(taken.sum())
        leg["worst_pose_difference_a_vs_host_loop"] = float(np.abs(warm["a_process_synced"]["pose"][taken] -
                                                                   warm["c_msync_then_host_loop"]).max())
        res["calls_of_%d" % chunk] = leg
    # launches and waits of ONE call of 16 on warm handles
    start()
    r, t, ti, iseen, oseen = args(0, 16)
    proc.process_synced(ms, log["laser"], r, scan, t, ti, iseen, oseen)
    h0, m0 = proc.stats(), ms.stats()
    ctx.profile(True)
    ctx.profile_reset()
    r, t, ti, iseen, oseen = args(16, 32)
    proc.process_synced(ms, log["laser"], r, scan, t, ti, iseen, oseen)
    ctx.profile(False)
    h1, m1 = proc.stats(), ms.stats()
    res["one_call_of_16"] = {"launches": {k: int(v[0]) for k, v in ctx.profile_read().items()},
                             "kernel_us_per_launch": {k: round(1e3 * v[1] / max(v[0], 1), 2) for k, v in ctx.profile_read().items()},
                             "msync_launches": m1["launches"] - m0["launches"], "msync_host_waits": m1["host_waits"] - m0["host_waits"],
                             "hector_host_syncs": h1["host_syncs"] - h0["host_syncs"], "hector_calls": h1["calls"] - h0["calls"],
                             "hector_scans_taken": h1["scans"] - h0["scans"]}
    print(json.dumps(res))
    ms.close()
    gmap.close()
    ctx.close()


if __name__ == "__main__":
    main()
