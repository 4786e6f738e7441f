#!/usr/bin/env python3
"""R robots, raw IMU, odometry and LaserScan messages in, Hector poses and R maps out: the workload of
tools/hector_sync_bench.py (1081 beams, 400 Hz IMU, 50 Hz odometry, 1024^2 x 3 levels, 300 scan callbacks per member) on R
nodes and R processors, calls of 16 steps.  Member r gets the log with its scans rolled by r (the stamps and the IMU and
odometry messages are the log's: they decide what the node takes, the scans what the matcher sees).  Three legs in one process:

  (A) solo          the members one after another through their own HectorProcessor.process_synced -- R walks, R de-skew
                    launches and R chains per step; the baseline, existing code
  (B) fleet         api.HectorFleet.process_synced -- one walk, one windows, one de-skew launch per call, one chain per step
  (C) nodes + fleet every member's own MotionSync.scans_dev into HBM, then HectorFleet.process_many_clouds_dev on the
                    records' status words -- what the fleet-wide synchronisation buys over R per-handle ones.  Its ranges are
                    in HBM before the clock starts (scans_dev takes device rows); (A) and (B) carry theirs up inside the clock.

Every pass resets nodes and processors and pushes every node's messages inside the clock.  A warm-up pass of each leg, then
--repeats passes with the legs alternating; per leg the median and the spread (max - min) of the aggregate callbacks/s, and
microseconds per step.  The records of the three legs are compared bit for bit in every pass.  --profile adds one pass of (A)
and of (B) with HIP-event times per launch.  Prints one JSON line.
Usage: python tools/hector_fleet_sync_bench.py --members 16 [--scans 300] [--chunk 16] [--repeats 5] [--profile]"""
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
from hector_sync_bench import Laser  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    R, S = a.members, a.scans
    log = msync_bench.make_log(S)
    beams = log["ranges"].shape[1]
    n, cell, levels = 1024, 0.05, 3
    off = (n * cell * 0.5, n * cell * 0.5)
    scan = api.hector_scan(Laser(log["laser"]), z_min=-1.0, z_max=2.0)  # lesson5's cloud has z ~ 1
    ctx = api.Context(0)  # raises without a GPU: nothing here is measured on a CPU
    maps, procs, nodes = [], [], []
    for r in range(R):
        m = api.OccGridMap(ctx, n, n, cell, off, levels=levels)
        m.setUpdateOccupiedFactor(0.9)
        h = api.HectorProcessor(m)
        h.set_update_thresholds(-1.0, -1.0)  # every taken scan updates the map
        maps.append(m)
        procs.append(h)
        nodes.append(api.MotionSync(ctx))
    fleet = api.HectorFleet(procs)
    ranges = np.stack([np.roll(log["ranges"], -r, axis=0) for r in range(R)], axis=1)  # [S, R, beams]
    rec_words = api.MSYNC_RECORD.itemsize // 4
    # leg (C): every member's rolled ranges in HBM, and its clouds, valid flags and records of one call
    d_ranges = [ctx.alloc(S * beams * 4) for _ in range(R)]
    for r in range(R):
        ctx.upload(d_ranges[r], np.ascontiguousarray(ranges[:, r]))
    d_xyz = [ctx.alloc(a.chunk * beams * 12) for _ in range(R)]
    d_valid = [ctx.alloc(a.chunk * beams) for _ in range(R)]
    d_rec = [ctx.alloc(a.chunk * api.MSYNC_RECORD.itemsize) for _ in range(R)]
    calls = [(lo, min(lo + a.chunk, S)) for lo in range(0, S, a.chunk)]

    def small(lo, hi):
        return log["scan_t"][lo:hi], log["scan_tinc"][lo:hi], log["imu_seen"][lo:hi], log["odom_seen"][lo:hi]

    def start():
        for ms, h in zip(nodes, procs):
            ms.reset()
            h.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        for ms in nodes:
            ms.push_imu(log["imu_t"], log["imu_w"])
            ms.push_odom(log["odom_t"], log["odom_pos"], log["odom_quat"])
        return t0

    def leg_solo():
        t0, out = start(), []
        for lo, hi in calls:
            t, ti, iseen, oseen = small(lo, hi)
            out.append(np.stack([procs[r].process_synced(nodes[r], log["laser"], ranges[lo:hi, r], scan, t, ti, iseen, oseen)[0]
                                 for r in range(R)], axis=1))
        return time.perf_counter() - t0, np.concatenate(out)

    def leg_fleet():
        t0, out = start(), []
        for lo, hi in calls:
            t, ti, iseen, oseen = (np.repeat(v[:, None], R, axis=1) for v in small(lo, hi))
            out.append(fleet.process_synced(nodes, log["laser"], ranges[lo:hi], scan, t, ti, iseen, oseen)[0])
        return time.perf_counter() - t0, np.concatenate(out)

    def leg_nodes_then_fleet():
        t0, out = start(), []
        for lo, hi in calls:
            t, ti, iseen, oseen = small(lo, hi)
            for r in range(R):
                nodes[r].scans_dev(log["laser"], beams, d_ranges[r] + lo * beams * 4, beams, t, ti, d_xyz[r], d_valid[r], d_rec[r],
                                   iseen, oseen)
            out.append(fleet.process_many_clouds_dev(hi - lo, beams, d_xyz, d_valid, d_rec, rec_words, scan))
        return time.perf_counter() - t0, np.concatenate(out)

    legs = {"A_solo": leg_solo, "B_fleet": leg_fleet, "C_nodes_then_fleet": leg_nodes_then_fleet}
    for fn in legs.values():  # warm-up: allocations, code objects
        fn()
    times = {k: [] for k in legs}
    equal, taken = True, 0
    for _ in range(a.repeats):
        recs = {}
        for name, fn in legs.items():
            dt, recs[name] = fn()
            times[name].append(dt)
        equal = equal and all(recs[k].tobytes() == recs["A_solo"].tobytes() for k in recs)
        taken = int((recs["A_solo"]["n_points"] >= 0).sum())
    res = {"config": "hector fleet, raw messages in: 1081 beams, 400 Hz IMU, 50 Hz odometry, 1024^2 x 3 levels, calls of %d steps" % a.chunk,
           "members": R, "scans": S, "repeats": a.repeats, "records_bit_equal": bool(equal), "taken": taken}
    for name, v in times.items():
        rate = [R * S / t for t in v]
        res[name] = {"callbacks_per_s_median": round(statistics.median(rate), 1), "callbacks_per_s_spread": round(max(rate) - min(rate), 1),
                     "us_per_step_median": round(1e6 * statistics.median(v) / S, 2),
                     "us_per_step_spread": round(1e6 * (max(v) - min(v)) / S, 2)}
    res["B_over_A"] = round(res["B_fleet"]["callbacks_per_s_median"] / res["A_solo"]["callbacks_per_s_median"], 3)
    res["B_over_C"] = round(res["B_fleet"]["callbacks_per_s_median"] / res["C_nodes_then_fleet"]["callbacks_per_s_median"], 3)
    if a.profile:
        for name in ("A_solo", "B_fleet"):
            ctx.profile(True)
            ctx.profile_reset()
            legs[name]()
            ctx.synchronize()
            ctx.profile(False)
            res[name]["kernel_us_per_launch"] = {k: round(1e3 * ms / max(launches, 1), 2)
                                                 for k, (launches, ms) in ctx.profile_read().items()}
            res[name]["launches"] = {k: int(launches) for k, (launches, ms) in ctx.profile_read().items()}
    st, ss = fleet.stats(), fleet.sync_stats()
    res["fleet_launches_per_step"] = st["launches"] / max(st["steps"], 1)
    res["fleet_sync_launches_per_call"] = ss["launches"] / max(ss["calls"], 1)
    res["fleet_host_syncs_per_call"] = st["host_syncs"] / max(st["calls"], 1)
    print(json.dumps(res))
    for ms in nodes:
        ms.close()
    for m in maps:
        m.close()


if __name__ == "__main__":
    main()
