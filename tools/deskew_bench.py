#!/usr/bin/env python3
"""Measurements for the batched lesson5 de-skew and the streamed processor's de-skewed form, in one run:

  (a) B = 64 and 256 scans of 1081 beams through lslam_deskew_batch (host form: pinned staging up and down, one wait)
      against B successive lslam_deskew_scan calls; the batched kernel's own time from HIP events around it (_dev form,
      buffers resident).  The outputs of the two paths are compared bit for bit at the sizes timed.
  (b) HectorProcessor.process_deskewed in calls of 16 against the host-driven loop (deskew_scan -> setCloud -> matchContainer
      -> gate on the host -> updateByContainer) over 300 scans; decisions and poses of the two are compared.

The two sides of each comparison alternate inside one process, REPEATS times after a warm-up of every shape; the JSON line
carries the median and the spread (min, max) of each.  Usage: python tools/deskew_bench.py [--repeats N] [--scans N]"""
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
sys.path.insert(0, str(ROOT / "tests"))  # the numpy restatement of the update gate (hector_stream_cases.gate)
import lslam  # noqa: E402,F401
from lslam_amd import api, synth  # noqa: E402
import hector_stream_cases as S  # noqa: E402

f32 = np.float32
PERIOD, DUR = 0.12, 0.1


def truth(t, w=0.3, v=0.5):
    yaw = w * t
    return np.array([v / w * math.sin(yaw), v / w * (1.0 - math.cos(yaw)), yaw])


def make_scans(n_scans, seed=7):
    """Scans along an arc with the state lesson5's Prune* steps would leave: 11 integrated 100 Hz yaw-rate samples and the
    odometry increment over the sweep."""
    laser = synth.Laser()
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=5)
    rng = np.random.default_rng(seed)
    base = [synth.cast_scan(world, truth(PERIOD * k), laser, 0.01, 0.02, rng).astype(f32) for k in range(min(n_scans, 300))]
    ranges = np.stack([base[k % len(base)] for k in range(n_scans)])
    params, times, rots = [], [], []
    for k in range(n_scans):
        t0 = 1000.0 + PERIOD * k
        a, b = truth(PERIOD * k), truth(PERIOD * k + DUR)
        c, s = math.cos(a[2]), math.sin(a[2])
        dx, dy = b[0] - a[0], b[1] - a[1]
        params.append(api.DeskewParams(laser.angle_min, laser.angle_increment, laser.range_min, 30.0, t0, DUR / ranges.shape[1], 1, 1,
                                       t0 - 0.004, t0 + DUR - 0.004, c * dx + s * dy, -s * dx + c * dy, 0.0, 0.0))
        t = [t0 - 0.003 + 0.01 * j for j in range(11)]
        times.append(t)
        rots.append([[0.0, 0.0, 0.3 * (tj - t[0])] for tj in t])
    return laser, ranges, params, times, rots


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def bench_batch(ctx, B, repeats):
    laser, ranges, params, times, rots = make_scans(B)
    d = api.Deskewer(ctx)

    def singles():
        return [api.deskew_scan(ctx, ranges[k], params[k], times[k], rots[k]) for k in range(B)]

    xyz, valid = d.batch(ranges, params, times, rots)  # warm-up of both, and the comparison
    one = singles()
    same = all(xyz[k].tobytes() == one[k][0].tobytes() and np.array_equal(valid[k], one[k][1]) for k in range(B))
    growths = d.stats()["growths"]
    t_batch, t_loop = [], []
    for _ in range(repeats):  # alternating
        t0 = time.perf_counter()
        d.batch(ranges, params, times, rots)
        t_batch.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        singles()
        t_loop.append(time.perf_counter() - t0)
    # the kernel alone: buffers resident, HIP events around every launch of it
    n = ranges.shape[1]
    d_r, d_xyz, d_v = ctx.alloc(ranges.nbytes), ctx.alloc(B * n * 12), ctx.alloc(B * n)
    ctx.upload(d_r, ranges)
    d.batch_dev(n, d_r, n, params, times, rots, d_xyz, d_v)
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_only("deskew_batch")
    ctx.profile_reset()
    for _ in range(20):
        d.batch_dev(n, d_r, n, params, times, rots, d_xyz, d_v)
    ctx.synchronize()
    ctx.profile(False)
    ctx.profile_only(None)
    prof = ctx.profile_read().get("deskew_batch", {})
    t0 = time.perf_counter()
    for _ in range(20):
        d.batch_dev(n, d_r, n, params, times, rots, d_xyz, d_v)
    ctx.synchronize()
    dev_call = (time.perf_counter() - t0) / 20
    for p in (d_r, d_xyz, d_v):
        ctx.free(p)
    st = d.stats()
    d.close()
    mb, ml = statistics.median(t_batch), statistics.median(t_loop)
    return {"B": B, "beams": n, "bit_identical": bool(same), "batch_s": spread(t_batch), "single_loop_s": spread(t_loop),
            "speedup_median": ml / mb, "batch_us_per_scan": 1e6 * mb / B, "single_us_per_scan": 1e6 * ml / B,
            "kernel": prof, "dev_form_call_s": dev_call, "growths_after_warmup": st["growths"] - growths,
            "host_waits": st["host_waits"]}


def bench_stream(ctx, n_scans, call, repeats):
    laser, ranges, params, times, rots = make_scans(n_scans, seed=9)
    scan = api.hector_scan(laser, z_min=-1.0, z_max=2.0)
    n_map = 1024

    def fresh():
        m = api.OccGridMap(ctx, n_map, n_map, S.CELL, S.offset(n_map), levels=3)
        m.setUpdateFreeFactor(0.4)
        m.setUpdateOccupiedFactor(0.9)
        return m

    def streamed():
        m = fresh()
        h = api.HectorProcessor(m)
        ctx.synchronize()
        t0 = time.perf_counter()
        recs = [h.process_deskewed(ranges[k:k + call], scan, params[k:k + call], times[k:k + call], rots[k:k + call])
                for k in range(0, n_scans, call)]
        dt = time.perf_counter() - t0
        st = h.stats()
        m.close()
        return dt, np.concatenate(recs), st

    def host_loop():
        m = fresh()
        est, last = np.zeros(3, f32), np.full(3, S.FLT_MAX, f32)
        poses, upd = [], []
        ctx.synchronize()
        t0 = time.perf_counter()
        for k in range(n_scans):
            x, v = api.deskew_scan(ctx, ranges[k], params[k], times[k], rots[k])
            if m.setCloud(x, v, scan) > 0:
                est, _ = m.matchContainer(est)
            did = S.gate(est, last)
            if did:
                m.updateByContainer(est)
                last = est.copy()
            poses.append(est.copy())
            upd.append(did)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        m.close()
        return dt, np.array(poses), np.array(upd)

    _, rec, st = streamed()  # warm-up of both, and the comparison
    _, poses, upd = host_loop()
    t_s, t_h = [], []
    for _ in range(repeats):
        t_s.append(streamed()[0])
        t_h.append(host_loop()[0])
    ms, mh = statistics.median(t_s), statistics.median(t_h)
    return {"scans": n_scans, "scans_per_call": call, "streamed_s": spread(t_s), "host_loop_s": spread(t_h),
            "speedup_median": mh / ms, "streamed_us_per_scan": 1e6 * ms / n_scans, "host_loop_us_per_scan": 1e6 * mh / n_scans,
            "same_decisions": bool(np.array_equal(upd, rec["updated"] != 0)),
            "worst_pose_difference": float(np.abs(poses - rec["pose"]).max()), "map_updates": int((rec["updated"] != 0).sum()),
            "min_points": int(rec["n_points"].min()), "calls": st["calls"], "host_syncs": st["host_syncs"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scans", type=int, default=300)
    a = ap.parse_args()
    ctx = api.Context(0)  # raises without a GPU: nothing here is measured on a CPU
    out = {"deskew_batch": [bench_batch(ctx, B, a.repeats) for B in (64, 256)],
           "stream": bench_stream(ctx, a.scans, 16, max(3, a.repeats // 2))}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
