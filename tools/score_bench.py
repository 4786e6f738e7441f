#!/usr/bin/env python3
"""Throughput of pose scoring (lslam_map_score_batch_dev / lslam_map_pose_covariance_batch_dev / lslam_map_score_lattice_dev) on
the 1024^2, 3-level synthetic map with 1081-point containers:
  scoreBatch            B in {64, 512, 4096, 32768} states on level 0, with B distinct containers and with ONE shared container
  poseCovarianceBatch   4096 entries (28672 states + the covariance epilogue)
  scoreLattice          41 x 41 x 21 = 35301 states on level 2 and on level 0 (+ the best-state reduction)
each in the default mode and with LSLAM_MAP_OPT_ORDERED_SUMS, and -- the partition A/B -- the default mode with 2, 4 and 8
points per lane in flight (LSLAM_SCORE_CHUNK, read when a map is created; results do not depend on it).
Points, poses and results stay in HBM; a call is timed from its start to the end of lslam_synchronize.  Warm-up first, then
--reps timed repetitions per point; medians.  Prints one JSON line; the reference's CPU time per state, recorded with the golden
file on its host, rides along as a host figure."""
import argparse
import json
import os
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import lslam  # noqa: E402,F401
from lslam_amd import api, synth  # noqa: E402

N, CELL, LEVELS, POINTS = 1024, 0.05, 3, 1081
LATTICE = (41, 41, 21)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,512,4096,32768")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", default="batch,covariance,lattice", help="prefixes of the legs to run (a counter pass wants one)")
    ap.add_argument("--modes", default="2,4,8,ordered", help="default-mode chunk sizes and / or 'ordered'")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    legs_on = tuple(args.legs.split(","))
    modes = args.modes.split(",")
    chunks = [int(c) for c in modes if c != "ordered"] or [4]
    ctx = api.Context(0)
    laser = synth.Laser()
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=3)
    off = (N * CELL * 0.5, N * CELL * 0.5)
    path = synth.trajectory(world, 64, step=0.1, seed=3, bounds=6.0)
    rng = np.random.default_rng(1)
    conts = []
    for t in path:
        r = synth.cast_scan(world, t, laser, 0.01, 0.0, rng)
        p = synth.hector_points(r, laser, 1.0 / CELL, use_max=20.0)
        reps = -(-POINTS // len(p))  # every container holds exactly 1081 points: the scan, replicated with 0.05-cell noise
        conts.append(np.concatenate([p] + [p + rng.normal(0.0, 0.05, p.shape).astype(np.float32) for _ in range(reps - 1)])[:POINTS]
                     .astype(np.float32))

    def make_map(chunk):
        os.environ["LSLAM_SCORE_CHUNK"] = str(chunk)
        try:
            m = api.OccGridMap(ctx, N, N, CELL, off, levels=LEVELS)
        finally:
            del os.environ["LSLAM_SCORE_CHUNK"]
        m.setUpdateOccupiedFactor(0.9)
        for k in range(0, 64, 8):
            m.matchData(path[k].astype(np.float32), conts[k])
            m.updateByScan(conts[k], (0.0, 0.0), path[k].astype(np.float32))
        return m

    maps = {c: make_map(c) for c in chunks}
    ctx.synchronize()

    bmax = max(sizes + [4096])
    off_rng = np.random.default_rng(2)
    ec_all = (np.arange(bmax) % 64).astype(np.int32)
    poses_all = (np.stack([path[k] for k in ec_all]) +
                 np.concatenate([off_rng.uniform(-0.1, 0.1, (bmax, 2)), off_rng.uniform(-0.04, 0.04, (bmax, 1))], axis=1)).astype(np.float32)
    pts64 = np.ascontiguousarray(np.concatenate(conts), np.float32).reshape(64, POINTS, 2)
    pts_a = np.ascontiguousarray(np.tile(pts64, (-(-bmax // 64), 1, 1))[:bmax].reshape(-1, 2))  # B DISTINCT containers in memory
    d_pts, d_poses = ctx.alloc(pts_a.nbytes), ctx.alloc(poses_all.nbytes)
    d_res, d_lik = ctx.alloc(bmax * 4), ctx.alloc(max(bmax * 4, 4096 * 28, int(np.prod(LATTICE)) * 4))
    d_cm, d_cw, d_best = ctx.alloc(4096 * 36), ctx.alloc(4096 * 36), ctx.alloc(16)
    ctx.upload(d_pts, pts_a)
    ctx.upload(d_poses, poses_all)
    counts_a = np.full(bmax, POINTS, np.int32)
    one = np.array([POINTS], np.int32)
    centre = path[0].astype(np.float32)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    def legs(m):
        """name -> (states, seconds) of every leg on one map in its current mode."""
        out = {}
        names = (["batch_distinct_%d" % b for b in sizes] + ["batch_shared_%d" % b for b in sizes] +
                 ["covariance_4096", "lattice_41x41x21_L2", "lattice_41x41x21_L0"])
        want = {n for n in names if n.startswith(legs_on)}
        for b in sizes:
            def distinct():
                m.scoreBatch_dev(b, d_pts, counts_a[:b], None, d_poses, 0, d_res, d_lik)
                ctx.synchronize()

            def shared():
                m.scoreBatch_dev(b, d_pts, one, np.zeros(b, np.int32), d_poses, 0, d_res, d_lik)
                ctx.synchronize()

            if "batch_distinct_%d" % b in want:
                out["batch_distinct_%d" % b] = (b, timed(distinct))
            if "batch_shared_%d" % b in want:
                out["batch_shared_%d" % b] = (b, timed(shared))

        def cov():
            m.poseCovarianceBatch_dev(4096, d_pts, counts_a[:4096], None, d_poses, 0, d_lik, d_cm, d_cw)
            ctx.synchronize()

        if "covariance_4096" in want:
            out["covariance_4096"] = (7 * 4096, timed(cov))
        for level, step in ((2, 0.2), (0, 0.05)):
            def lattice():
                m.scoreLattice_dev(d_pts, POINTS, centre, LATTICE, (step, step, 0.02), level, d_lik, d_best, d_best + 4)
                ctx.synchronize()

            if "lattice_41x41x21_L%d" % level in want:
                out["lattice_41x41x21_L%d" % level] = (int(np.prod(LATTICE)), timed(lattice))
        return {k: {"states": n, "us": t * 1e6, "ns_per_state": t * 1e9 / n, "states_per_s": n / t} for k, (n, t) in out.items()}

    res = {"tool": "score_bench", "points": POINTS, "map": N, "levels": LEVELS, "reps": args.reps, "warmup": args.warmup}
    for chunk, m in maps.items():
        if str(chunk) in modes:
            res["default_chunk%d" % chunk] = legs(m)
    if "ordered" in modes:
        m = maps[chunks[0]]
        m.set_option("ordered_sums", 1)
        res["ordered"] = legs(m)
        m.set_option("ordered_sums", 0)
    golden = ROOT / "tests" / "golden" / "score_golden.npz"
    if golden.exists():
        res["reference_cpu_us_per_state_on_its_recording_host"] = float(np.load(golden)["ref_cpu_state_s"]) * 1e6
    for p in (d_pts, d_poses, d_res, d_lik, d_cm, d_cw, d_best):
        ctx.free(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
