#!/usr/bin/env python3
"""Measurements for lesson2's batched point-to-point ICP, in one run.  Scans: tools/plicp_bench.py's log (a robot
creeping through the bench arena, 0.03-0.06 m and up to 0.02 rad between scans, sigma = 0.002 m noise); B CONSECUTIVE pairs of
360-beam and 1081-beam scans (64 distinct scans; larger batches tile them) through

  host form   lslam_icp_match_batch: pinned staging up and down, a conversion and a match launch, one wait (host clock)
  dev form    lslam_icp_match_batch_dev with every buffer resident: host clock over CALLS calls and one synchronise
  kernel      HIP events around each launch of k_icp_match alone (and of k_icp_cloud alone)
  cpu         tools/icp_cpu.py's icp on the first pairs, one core: a HOST figure

After a warm-up of every shape each figure is taken REPEATS times and reported as median (min, max).  The host and dev forms'
records are compared byte for byte at the sizes timed.  Usage: python tools/icp_bench.py [--repeats N] [--sizes 1,64,512,4096]
[--cpu-pairs N]"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import lslam  # noqa: E402,F401
from lslam_amd import api  # noqa: E402
from tools import icp_cpu  # noqa: E402
from tools.plicp_bench import LASERS, UNIQUE, make_log, spread  # noqa: E402


def kernel_time(ctx, name, run, repeats, calls):
    t = []
    ctx.profile(True)
    ctx.profile_only(name)
    for _ in range(repeats):
        ctx.profile_reset()
        for _ in range(calls):
            run()
        ctx.synchronize()
        launches, ms = ctx.profile_read().get(name, (0, 0.0))
        t.append(1e-3 * ms / max(launches, 1))
    ctx.profile(False)
    ctx.profile_only(None)
    return t


def bench_pairs(ctx, beams, B, repeats, calls):
    laser = LASERS[beams]
    scans = make_log(laser)
    src = (np.arange(B) % UNIQUE).astype(np.int32)
    tgt = src + 1
    m = api.IcpMatcher(ctx, laser=laser)
    host = m.match_batch(scans, src, tgt)  # warm-up
    m.match_batch(scans, src, tgt)
    growths = m.stats()["growths"]
    t_host = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        m.match_batch(scans, src, tgt)
        t_host.append(time.perf_counter() - t0)
    grew = m.stats()["growths"] - growths
    p_r, p_o = ctx.alloc(scans.nbytes), ctx.alloc(B * 64)
    ctx.upload(p_r, scans)

    def dev():
        m.match_batch_dev(len(scans), beams, p_r, beams, src, tgt, None, p_o)

    dev()
    ctx.synchronize()
    got = np.zeros(B, api.ICP_RECORD)
    ctx.download(p_o, got)
    identical = got.tobytes() == host.tobytes()
    t_dev = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            dev()
        ctx.synchronize()
        t_dev.append((time.perf_counter() - t0) / calls)
    t_kernel = kernel_time(ctx, "icp_match", dev, repeats, calls)
    t_cloud = kernel_time(ctx, "icp_cloud", dev, repeats, calls)
    ctx.free(p_r)
    ctx.free(p_o)
    m.close()
    searches = float((host["iterations"] + 1).sum())  # one search per iteration and one for the fitness score
    evals = searches * beams * beams
    return {"beams": beams, "B": B, "host_equals_dev": bool(identical), "converged": int(host["converged"].sum()),
            "iterations_per_pair": float(host["iterations"].mean()), "iterations_min_max": [int(host["iterations"].min()),
                                                                                           int(host["iterations"].max())],
            "states": {str(s): int((host["state"] == s).sum()) for s in np.unique(host["state"])},
            "host_form_ms": spread(t_host, 1e3), "dev_form_ms": spread(t_dev, 1e3), "kernel_ms": spread(t_kernel, 1e3),
            "cloud_kernel_us": spread(t_cloud, 1e6), "kernel_us_per_pair": spread(t_kernel, 1e6 / B),
            "host_form_us_per_pair": spread(t_host, 1e6 / B), "distance_evaluations": evals,
            "kernel_gevals_per_s": spread([evals / t / 1e9 for t in t_kernel]), "growths_after_warmup": grew}


def bench_cpu(beams, n_pairs):
    laser = LASERS[beams]
    scans = make_log(laser)
    clouds = [icp_cpu.scan_to_cloud(s, laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max)[0]
              for s in scans[:n_pairs + 1]]
    t, its = [], []
    for k in range(n_pairs):
        t0 = time.perf_counter()
        out = icp_cpu.icp(clouds[k], clouds[k + 1], trace=False)
        t.append(time.perf_counter() - t0)
        its.append(out["iterations"])
    return {"beams": beams, "pairs": n_pairs, "ms_per_pair": spread(t, 1e3), "iterations_per_pair": float(np.mean(its))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1,64,512,4096")
    ap.add_argument("--cpu-pairs", type=int, default=6)
    a = ap.parse_args()
    ctx = api.Context(0)  # raises without a GPU: nothing of the device path is measured on a CPU
    out = {"pairs": [], "cpu_helper_one_core_host_figure": []}
    for beams in (360, 1081):
        for B in (int(v) for v in a.sizes.split(",")):
            out["pairs"].append(bench_pairs(ctx, beams, B, a.repeats, 20 if B <= 64 else 3))
            print(json.dumps(out["pairs"][-1]), flush=True)
        out["cpu_helper_one_core_host_figure"].append(bench_cpu(beams, a.cpu_pairs))
        print(json.dumps(out["cpu_helper_one_core_host_figure"][-1]), flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
