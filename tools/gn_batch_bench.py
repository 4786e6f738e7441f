#!/usr/bin/env python3
"""Throughput of the batched Gauss-Newton match (lslam_map_match_batch_dev) on one synthetic map: B entries of 1081
points, B in {1, 64, 512, 4096}, in three legs:
  (a) distinct   B containers, one start pose each
  (b) shared     ONE container, B start poses (re-localisation from K hypotheses)
  (c) single     B successive lslam_map_match_data calls on the inputs of (a): the only route without the batch call
Legs (a) and (b) keep points, start poses and results in HBM and are timed from the call to the end of
lslam_synchronize; leg (c) is the host call, which returns with the result.  Warm-up first, then --reps timed repetitions
per point; medians.  Prints one JSON line (matches per second, and the batch's ratio over (c))."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import lslam  # noqa: E402,F401
from lslam_amd import api, synth  # noqa: E402

N, CELL, LEVELS, POINTS = 1024, 0.05, 3, 1081


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,512,4096")
    ap.add_argument("--reps", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--single-cap", type=int, default=512, help="leg (c) times at most this many calls per repetition")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    ctx = api.Context(0)
    laser = synth.Laser()
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=3)
    off = (N * CELL * 0.5, N * CELL * 0.5)
    gmap = api.OccGridMap(ctx, N, N, CELL, off, levels=LEVELS)
    gmap.setUpdateOccupiedFactor(0.9)
    path = synth.trajectory(world, 64, step=0.1, seed=3, bounds=6.0)
    rng = np.random.default_rng(1)
    conts = []
    for t in path:
        r = synth.cast_scan(world, t, laser, 0.01, 0.0, rng)
        p = synth.hector_points(r, laser, 1.0 / CELL, use_max=20.0)
        reps = -(-POINTS // len(p))  # every container holds exactly 1081 points: the scan, replicated with 0.05-cell noise
        conts.append(np.concatenate([p] + [p + rng.normal(0.0, 0.05, p.shape).astype(np.float32) for _ in range(reps - 1)])[:POINTS]
                     .astype(np.float32))
    for k in range(0, 64, 8):
        gmap.matchData(path[k].astype(np.float32), conts[k])
        gmap.updateByScan(conts[k], (0.0, 0.0), path[k].astype(np.float32))
    ctx.synchronize()

    bmax = max(sizes)
    pts = np.ascontiguousarray(np.concatenate(conts), np.float32)  # 64 distinct containers, entries cycle through them
    off_rng = np.random.default_rng(2)
    ec_all = (np.arange(bmax) % 64).astype(np.int32)
    begin_all = (np.stack([path[k] for k in ec_all]) +
                 np.concatenate([off_rng.uniform(-0.1, 0.1, (bmax, 2)), off_rng.uniform(-0.04, 0.04, (bmax, 1))], axis=1)).astype(np.float32)
    # leg (a) wants B DISTINCT containers in memory (B x 8.6 KB of points): the 64 scans tiled to B
    pts_a = np.ascontiguousarray(np.tile(pts.reshape(64, POINTS, 2), (-(-bmax // 64), 1, 1))[:bmax].reshape(-1, 2))
    d_pts_a, d_begin = ctx.alloc(pts_a.nbytes), ctx.alloc(begin_all.nbytes)
    d_pose, d_cov = ctx.alloc(bmax * 12), ctx.alloc(bmax * 36)
    ctx.upload(d_pts_a, pts_a)
    ctx.upload(d_begin, begin_all)
    counts_a = np.full(bmax, POINTS, np.int32)
    one = np.array([POINTS], np.int32)

    def timed(fn, reps):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    out = {"tool": "gn_batch_bench", "points": POINTS, "map": N, "levels": LEVELS, "reps": args.reps, "sizes": {}}
    for b in sizes:
        def leg_a():
            gmap.matchBatch_dev(b, d_pts_a, counts_a[:b], None, d_begin, d_pose, d_cov)
            ctx.synchronize()

        def leg_b():
            gmap.matchBatch_dev(b, d_pts_a, one, np.zeros(b, np.int32), d_begin, d_pose, d_cov)
            ctx.synchronize()

        nb = min(b, args.single_cap)

        def leg_c():
            for k in range(nb):
                gmap.matchData(begin_all[k], conts[ec_all[k]])

        ta, tb = timed(leg_a, args.reps), timed(leg_b, args.reps)
        tc = timed(leg_c, max(5, args.reps // max(1, nb // 8))) / nb * b
        out["sizes"][str(b)] = {
            "distinct_matches_per_s": b / ta, "shared_matches_per_s": b / tb, "single_calls_matches_per_s": b / tc,
            "distinct_us": ta * 1e6, "shared_us": tb * 1e6, "single_calls_us": tc * 1e6,
            "distinct_over_single": tc / ta, "shared_over_single": tc / tb,
        }
    for p in (d_pts_a, d_begin, d_pose, d_cov):
        ctx.free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
