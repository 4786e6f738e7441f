"""Live occupancy map over the front-end's resident scans against the route without it: one JSON line per N.

A front-end is filled with N synthetic 1081-beam scans (laps of one loop, through ProcessMany), then four things are timed,
each as wall clock around the (host-synchronous) call and as the HIP-event sum of its kernels (the library's own per-launch
events, lslam_profile_*; the host-to-device copies of (a) show up in its wall clock only):
  (a) no live map: N lslam_frontend_scan_pose calls, robot -> sensor poses, lslam_occgrid_create_from_scans from host arrays
      (uploads every reading again, retraces every ray)
  (b) live rebuild: the first update of a fresh live map (every resident scan traced, nothing uploaded but ids and poses)
  (c) live append: update after 16 more scans were processed (median of --reps)
  (d) lslam_occgrid_read_ros_i8 of the live map (classification + read back: what the node publishes)

    python tools/livemap_bench.py [--n 500 4000] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import lslam  # noqa: E402,F401
from lslam_amd import api, synth  # noqa: E402

RES, THR, LAP = 0.05, 20.0, 125


class Timed:
    """wall ms of one call; kernels(): the HIP-event time of every kernel it launched, by name"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __call__(self, fn):
        self.ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return out, {"wall_ms": round((time.perf_counter() - t0) * 1e3, 3)}

    def kernels(self, fn):
        self.ctx.profile_reset()
        self.ctx.profile(True)
        out = fn()
        self.ctx.profile(False)
        per = self.ctx.profile_read()
        return out, {k: round(v[1], 4) for k, v in sorted(per.items())}


def run(ctx, n_scans: int, reps: int, lap_ranges, lap_path):
    lp = api.laser_params(synth.Laser(), THR)
    gm = api.ScanMatcher(ctx, api.baseline_config(range_threshold=THR), lp)
    fe = api.FrontEnd(gm, scan_buffer_size=20, scan_buffer_max_distance=5.0)
    timed = Timed(ctx)
    idx = np.arange(n_scans + 16 * (2 * reps + 2)) % LAP
    kept = []

    def feed(a, b):
        ok = fe.ProcessMany(lap_ranges[idx[a:b]], lap_path[idx[a:b]])[0]
        kept.extend(idx[a:b][ok])

    t0 = time.perf_counter()
    feed(0, n_scans)
    fill_s = time.perf_counter() - t0
    n = fe.num_scans()

    def parent_route():
        robot = np.stack([fe.scan_pose(i) for i in range(fe.num_scans())])
        sensor = np.stack([gm.sensor_pose_from_robot(p) for p in robot])
        t1 = time.perf_counter()
        g = api.OccupancyGrid.CreateFromScans(ctx, lp, lap_ranges[np.asarray(kept)], sensor, RES)
        dt = (time.perf_counter() - t1) * 1e3
        info = g.info()
        g.close()
        return info, dt

    parent_route()  # warm-up (first-use allocations, code objects)
    (info_a, create_ms), a = timed(parent_route)
    a["create_from_scans_wall_ms"] = round(create_ms, 3)
    a["upload_MB"] = round(n * 1081 * 8 / 1e6, 2)
    _, a["kernels_ms"] = timed.kernels(parent_route)

    api.LiveMap(fe, RES).update()  # warm-up
    best = None
    for _ in range(reps):
        lm = api.LiveMap(fe, RES)
        _, b = timed(lm.update)
        assert lm.stats()["rebuilds"] == 1
        if best is None or b["wall_ms"] < best["wall_ms"]:
            best = b
        lm.close()
    lm = api.LiveMap(fe, RES)
    _, best["kernels_ms"] = timed.kernels(lm.update)
    assert lm.grid().info()[:2] == info_a[:2]

    appends, kinds, pos = [], [], n_scans
    for r in range(2 * reps):
        feed(pos, pos + 16)
        pos += 16
        before = lm.stats()
        if r < reps:
            _, c = timed(lm.update)
            appends.append(c)
        else:
            _, c = timed.kernels(lm.update)
            appends_k = c
        after = lm.stats()
        kinds.append([k for k in ("appends", "grows", "rebuilds") if after[k] != before[k]][0])
    c = {"wall_ms": float(np.median([x["wall_ms"] for x in appends])),
         "kernels_ms": appends_k, "paths": kinds, "scans_per_update": int((lm.stats()["scans"] - n) / (2 * reps))}

    g = lm.grid()
    g.ros_data()
    reads = [timed(g.ros_data)[1] for _ in range(reps)]
    d = {"wall_ms": float(np.median([x["wall_ms"] for x in reads]))}
    _, d["kernels_ms"] = timed.kernels(g.ros_data)
    w, h = g.info()[:2]
    out = {"metric": "livemap", "n_scans": n, "grid": [w, h], "fill_s": round(fill_s, 2), "a_parent_route": a, "b_live_rebuild": best,
           "c_live_append_16": c, "d_read_ros_i8": d, "stats": lm.stats()}
    print(json.dumps(out), flush=True)
    lm.close()
    fe.close()
    gm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[500, 4000])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = api.Context(0)
    laser = synth.Laser()
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=5)
    path = synth.loop_trajectory(LAP, w=8.0, h=4.5, step=0.2, origin=(-4.0, -2.25))
    ranges = np.stack([synth.ranges_to_f64(synth.cast_scan(world, t, laser, 0.01, 0.01, np.random.default_rng([3, i])))
                       for i, t in enumerate(path)])
    for n in a.n:
        run(ctx, n, a.reps, ranges, np.asarray(path))
    ctx.close()


if __name__ == "__main__":
    main()
