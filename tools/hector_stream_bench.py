#!/usr/bin/env python3
"""lesson4's front-end loop, host-driven and streamed, on the workload of tools/bench_extra.py::hector_front_end (1024^2, 3
levels, 300 scans by default), in one process and one run:

  host_points      matchData(points) + updateByScan(points) per scan, as that function does it (the yardstick)
  host_container   setScan(ranges) + matchContainer + updateByContainer per scan (the resident-container loop)
  stream_N         HectorProcessor.process_many over the same ranges in calls of N scans (1, 16, all)

Every leg matches every scan from the same hints and updates the map with every scan (the streamed processor's thresholds
are set below zero so that its gate always passes: the same work).  A warm-up pass first, then --repeats timed passes on a
reset map; min and median scans/s.  --profile adds a pass with HIP-event kernel times (lslam_profile_*).
Prints one JSON line."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import lslam  # noqa: E402,F401
from lslam_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    laser = synth.Laser()
    n, cell, levels = 1024, 0.05, 3
    off = (n * cell * 0.5, n * cell * 0.5)
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=3)
    path = synth.trajectory(world, a.scans, step=0.05, seed=3, bounds=6.0)
    rng = np.random.default_rng(1)
    ranges = np.stack([synth.cast_scan(world, t, laser, 0.01, 0.0, rng) for t in path]).astype(np.float32)
    pts_all = [synth.hector_points(r, laser, 1.0 / cell, use_max=20.0) for r in ranges]
    hints = np.array([(t + np.array([0.05, -0.04, 0.02])) for t in path], np.float32)
    hints[0] = path[0]
    scan = api.hector_scan(laser)
    ctx = api.Context(0)
    gmap = api.OccGridMap(ctx, n, n, cell, off, levels=levels)
    gmap.setUpdateOccupiedFactor(0.9)
    proc = api.HectorProcessor(gmap)
    proc.set_update_thresholds(-1.0, -1.0)

    def host_points():
        poses = []
        for pts, hint in zip(pts_all, hints):
            pose = gmap.matchData(hint, pts)[0]
            gmap.updateByScan(pts, (0.0, 0.0), pose)
            poses.append(pose)
        ctx.synchronize()
        return np.array(poses)

    def host_container():
        poses = []
        for r, hint in zip(ranges, hints):
            gmap.setScan(r, scan)
            pose = gmap.matchContainer(hint)[0]
            gmap.updateByContainer(pose)
            poses.append(pose)
        ctx.synchronize()
        return np.array(poses)

    def stream(chunk):
        def run():
            out = [proc.process_many(ranges[k:k + chunk], scan, hints[k:k + chunk]) for k in range(0, a.scans, chunk)]
            return np.concatenate(out)["pose"]
        return run

    legs = [("host_points", host_points), ("host_container", host_container), ("stream_1", stream(1)),
            ("stream_16", stream(16)), ("stream_%d" % a.scans, stream(a.scans))]
    res = {"config": "lesson4 front-end loop, host-driven and streamed: 1024^2 x 3 levels, 1081 beams", "scans": a.scans,
           "repeats": a.repeats}
    poses = {}
    for name, fn in legs:
        proc.reset()
        fn()  # warm-up: allocations, the cos / sin table, code objects
        times = []
        for _ in range(a.repeats):
            proc.reset()
            ctx.synchronize()
            t0 = time.perf_counter()
            poses[name] = fn()
            times.append(time.perf_counter() - t0)
        res[name] = {"scans_per_s_best": round(a.scans / min(times), 1), "scans_per_s_median": round(a.scans / statistics.median(times), 1)}
        if a.profile:
            proc.reset()
            ctx.profile(True); ctx.profile_reset()
            fn()
            ctx.synchronize()
            ctx.profile(False)
            res[name]["kernel_us_per_launch"] = {k: round(1e3 * ms / max(launches, 1), 2) for k, (launches, ms) in ctx.profile_read().items()}
    before = proc.stats()
    proc.reset()
    stream(16)()
    after = proc.stats()
    res["host_syncs_per_call"] = (after["host_syncs"] - before["host_syncs"]) / max(after["calls"] - before["calls"], 1)
    res["max_pose_diff_stream_vs_host_container"] = float(np.abs(poses["stream_16"] - poses["host_container"]).max())
    res["max_pose_err_vs_truth_xy"] = float(np.hypot(*(poses["stream_%d" % a.scans][:, :2] - path[:, :2]).T).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
