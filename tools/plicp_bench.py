#!/usr/bin/env python3
"""Measurements for lesson3's batched PL-ICP, in one run.  Scans: a robot creeping through the bench arena
(synth.arena(size=24, n_axis=6, n_rot=3, seed=4)), 0.03-0.06 m and up to 0.02 rad between scans, sigma = 0.002 m noise;
B CONSECUTIVE pairs of 360-beam and 1081-beam scans (64 distinct scans; larger batches tile them) through

  host form   lslam_plicp_match_batch: pinned staging up and down, one launch, one wait (host clock around the call)
  dev form    lslam_plicp_match_batch_dev with every buffer resident: host clock over CALLS calls and one synchronise
  kernel      HIP events around each launch of the kernel alone
  odometry    lslam_plicp_odom_process_many: R tracks x STEPS scans in one launch (host clock around the call)
  cpu         tools/plicp_cpu.py's sm_icp on the first pairs, one core: a HOST figure

After a warm-up of every shape each figure is taken REPEATS times and reported as median (min, max).  The host and dev forms'
records are compared byte for byte at the sizes timed.  Usage: python tools/plicp_bench.py [--repeats N] [--sizes 1,64,512,4096]
[--tracks 1,16,256] [--cpu-pairs N]"""
import argparse
import json
import math
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import lslam  # noqa: E402,F401
from lslam_amd import api, synth  # noqa: E402
from tools import plicp_cpu  # noqa: E402

UNIQUE = 64
LASERS = {360: synth.Laser(n_ranges=360, angle_min=-math.pi, angle_increment=math.radians(1.0), range_min=0.1, range_max=30.0),
          1081: synth.Laser(n_ranges=1081, angle_min=math.radians(-135.0), angle_increment=math.radians(0.25), range_min=0.1,
                            range_max=30.0)}


def make_log(laser, n=UNIQUE + 1, seed=7):
    """n scans along a slow arc that stays clear of the walls."""
    world = synth.arena(size=24.0, n_axis=6, n_rot=3, seed=4)
    rng = np.random.default_rng(seed)
    while True:
        pose = np.array([rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-3, 3)])
        poses = [pose]
        for _ in range(n - 1):
            d, th = rng.uniform(0.03, 0.06), rng.uniform(-0.02, 0.02)
            p = poses[-1]
            poses.append(np.array([p[0] + d * math.cos(p[2]), p[1] + d * math.sin(p[2]), p[2] + th]))
        if all(synth.point_is_free(world, p[0], p[1], 0.6) for p in poses):
            break
    return np.stack([synth.cast_scan(world, p, laser, 0.002, 0.0, rng) for p in poses]).astype(np.float32)


def spread(xs, scale=1.0):
    return {"median": scale * statistics.median(xs), "min": scale * min(xs), "max": scale * max(xs)}


def bench_pairs(ctx, beams, B, repeats, calls):
    laser = LASERS[beams]
    scans = make_log(laser)
    ref = (np.arange(B) % UNIQUE).astype(np.int32)
    sens = ref + 1
    m = api.PlicpMatcher(ctx, laser=laser)
    host = m.match_batch(scans, ref, sens)  # warm-up
    m.match_batch(scans, ref, sens)
    growths = m.stats()["growths"]
    t_host = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        m.match_batch(scans, ref, sens)
        t_host.append(time.perf_counter() - t0)
    grew = m.stats()["growths"] - growths
    p_r, p_o = ctx.alloc(scans.nbytes), ctx.alloc(B * 48)
    ctx.upload(p_r, scans)

    def dev():
        m.match_batch_dev(len(scans), beams, p_r, beams, ref, sens, None, p_o)

    dev()
    ctx.synchronize()
    got = np.zeros(B, api.PLICP_RECORD)
    ctx.download(p_o, got)
    identical = got.tobytes() == host.tobytes()
    t_dev = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            dev()
        ctx.synchronize()
        t_dev.append((time.perf_counter() - t0) / calls)
    t_kernel = []
    ctx.profile(True)
    ctx.profile_only("plicp_match")
    for _ in range(repeats):
        ctx.profile_reset()
        for _ in range(calls):
            dev()
        ctx.synchronize()
        launches, ms = ctx.profile_read().get("plicp_match", (0, 0.0))
        t_kernel.append(1e-3 * ms / max(launches, 1))
    ctx.profile(False)
    ctx.profile_only(None)
    ctx.free(p_r)
    ctx.free(p_o)
    m.close()
    return {"beams": beams, "B": B, "host_equals_dev": bool(identical), "valid": int(host["valid"].sum()),
            "iterations_per_pair": float(host["iterations"].mean()), "iterations_min_max": [int(host["iterations"].min()),
                                                                                           int(host["iterations"].max())],
            "nvalid_mean": float(host["nvalid"].mean()), "host_form_ms": spread(t_host, 1e3), "dev_form_ms": spread(t_dev, 1e3),
            "kernel_ms": spread(t_kernel, 1e3), "kernel_us_per_pair": spread(t_kernel, 1e6 / B),
            "host_form_us_per_pair": spread(t_host, 1e6 / B), "growths_after_warmup": grew}


def bench_odom(ctx, beams, R, steps, repeats):
    laser = LASERS[beams]
    scans = make_log(laser, steps)
    ranges = np.ascontiguousarray(np.repeat(scans[:, None, :], R, axis=1))
    stamps = np.repeat(0.1 * np.arange(steps)[:, None], R, axis=1)
    o = api.PlicpOdometry(ctx, R, laser=laser)
    rec = o.process_many(ranges, stamps)  # warm-up
    t = []
    for _ in range(repeats):
        o.reset()
        t0 = time.perf_counter()
        o.process_many(ranges, stamps)
        t.append(time.perf_counter() - t0)
    o.close()
    return {"beams": beams, "tracks": R, "steps": steps, "valid": int(rec["valid"].sum()), "keyframes": int((rec["flags"] & 2 > 0).sum()),
            "call_ms": spread(t, 1e3), "us_per_scan": spread(t, 1e6 / (R * steps)), "us_per_step": spread(t, 1e6 / steps)}


def bench_cpu(beams, n_pairs):
    laser = LASERS[beams]
    scans = make_log(laser)
    ldp = [plicp_cpu.laser_scan_to_ldp(s, laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max)
           for s in scans[:n_pairs + 1]]
    params = plicp_cpu.PlicpParams()
    t, its = [], []
    for k in range(n_pairs):
        t0 = time.perf_counter()
        out = plicp_cpu.sm_icp(params, ldp[k], ldp[k + 1])
        t.append(time.perf_counter() - t0)
        its.append(out["iterations"])
    return {"beams": beams, "pairs": n_pairs, "ms_per_pair": spread(t, 1e3), "iterations_per_pair": float(np.mean(its))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1,64,512,4096")
    ap.add_argument("--tracks", default="1,16,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cpu-pairs", type=int, default=6)
    a = ap.parse_args()
    ctx = api.Context(0)  # raises without a GPU: nothing of the device path is measured on a CPU
    out = {"pairs": [], "odometry": [], "cpu_helper_one_core_host_figure": []}
    for beams in (360, 1081):
        for B in (int(v) for v in a.sizes.split(",")):
            out["pairs"].append(bench_pairs(ctx, beams, B, a.repeats, 20 if B <= 64 else 3))
            print(json.dumps(out["pairs"][-1]), flush=True)
        for R in (int(v) for v in a.tracks.split(",")):
            out["odometry"].append(bench_odom(ctx, beams, R, a.steps, a.repeats))
            print(json.dumps(out["odometry"][-1]), flush=True)
        out["cpu_helper_one_core_host_figure"].append(bench_cpu(beams, a.cpu_pairs))
        print(json.dumps(out["cpu_helper_one_core_host_figure"][-1]), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
