#!/usr/bin/env python3
"""Measurements for the cloud forms of lesson3's PL-ICP, in one run, at 360 and 1081 points.  Scans: tools/plicp_bench.py's
log (a robot creeping through the bench arena, sigma = 0.002 m), converted on the host to float32 clouds as a converter does
(x = float32(r cos theta), y = float32(r sin theta), the valid byte by the node's range window).

  (a) pairs     lslam_plicp_match_clouds against lslam_plicp_match_batch on the same scans, B consecutive pairs: the host forms (host
                clock around the call, which ends in its wait) and the _dev forms with every buffer resident (host clock over CALLS
                calls and one synchronise).  The two kernels differ in their loader alone.
  (b) odometry  STEPS steps of R tracks through lslam_plicp_odom_process_many_clouds_dev (clouds resident: stamps up, records down)
                against lslam_plicp_odom_process_many (ranges from host memory), host clock around the call.
  (c) chain     raw messages in, poses out: lslam_msync_scans_dev (400 Hz IMU, 50 Hz odometry) and then
                lslam_plicp_odom_process_many_clouds_dev with &records[0].status as the take words, R nodes and R tracks; timed
                from the first push to the odometry's return, and the odometry call alone.

Every shape is warmed up on both routes first; the routes then ALTERNATE REPEATS times in one process, and each figure is reported
as median (min, max).  The forms' records are compared at the sizes timed: host against _dev byte for byte, clouds against ranges
by `valid` and the largest |x| difference (float32 points: not the same numbers).  No threshold: the figures are reported.
Usage: python tools/plicp_cloud_bench.py [--repeats N] [--sizes 1,64,512,4096] [--tracks 1,16,256] [--steps 20]"""
import argparse
import json
import math
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import lslam  # noqa: E402,F401
from lslam_amd import api  # noqa: E402
from plicp_bench import LASERS, UNIQUE, make_log, spread  # noqa: E402


def to_clouds(ranges, laser):
    r = np.asarray(ranges, np.float64)
    th = laser.angle_min + np.arange(r.shape[-1], dtype=np.float64) * laser.angle_increment
    with np.errstate(invalid="ignore"):
        ok = (r > laser.range_min) & (r < laser.range_max)
    rr = np.where(ok, r, 0.0)
    xyz = np.zeros(r.shape + (3,), np.float32)
    xyz[..., 0], xyz[..., 1] = (rr * np.cos(th)).astype(np.float32), (rr * np.sin(th)).astype(np.float32)
    return xyz, ok.astype(np.uint8)


def alternate(routes, repeats):
    """routes: name -> callable returning seconds.  Every route once per round, REPEATS rounds."""
    t = {k: [] for k in routes}
    for _ in range(repeats):
        for k, go in routes.items():
            t[k].append(go())
    return t


def bench_pairs(ctx, beams, B, repeats, calls):
    laser = LASERS[beams]
    scans = make_log(laser)
    xyz, valid = to_clouds(scans, laser)
    ref = (np.arange(B) % UNIQUE).astype(np.int32)
    sens = ref + 1
    m = api.PlicpMatcher(ctx, laser=laser)
    p_r, p_x, p_v, p_o = ctx.alloc(scans.nbytes), ctx.alloc(xyz.nbytes), ctx.alloc(valid.nbytes), ctx.alloc(B * 48)
    ctx.upload(p_r, scans), ctx.upload(p_x, xyz), ctx.upload(p_v, valid)

    def timed(fn, n=1, sync=False):
        def go():
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            if sync:
                ctx.synchronize()
            return (time.perf_counter() - t0) / n
        return go

    routes = {
        "ranges_host": timed(lambda: m.match_batch(scans, ref, sens)),
        "clouds_host": timed(lambda: m.match_clouds(xyz, ref, sens, valid)),
        "ranges_dev": timed(lambda: m.match_batch_dev(len(scans), beams, p_r, beams, ref, sens, None, p_o), calls, True),
        "clouds_dev": timed(lambda: m.match_clouds_dev(len(xyz), beams, p_x, p_v, ref, sens, None, p_o), calls, True),
    }
    got = np.zeros(B, api.PLICP_RECORD)
    host_r, host_c = m.match_batch(scans, ref, sens), m.match_clouds(xyz, ref, sens, valid)   # warm-up, and the comparison
    routes["clouds_dev"]()
    ctx.download(p_o, got)
    same = got.tobytes() == host_c.tobytes()
    for go in routes.values():
        go()
    growths = m.stats()["growths"]
    t = alternate(routes, repeats)
    grew = m.stats()["growths"] - growths
    for p in (p_r, p_x, p_v, p_o):
        ctx.free(p)
    m.close()
    dx = np.abs(host_c["x"] - host_r["x"])
    out = {"what": "pairs", "points": beams, "B": B, "clouds_host_equals_dev": bool(same),
           "valid_ranges_clouds": [int(host_r["valid"].sum()), int(host_c["valid"].sum())],
           "iterations_ranges_clouds": [float(host_r["iterations"].mean()), float(host_c["iterations"].mean())],
           "max_abs_x_clouds_minus_ranges": float(dx.max()), "growths_after_warmup": grew}
    for k, v in t.items():
        out[k + "_ms"] = spread(v, 1e3)
    out["clouds_over_ranges_dev"] = float(np.median(t["clouds_dev"]) / np.median(t["ranges_dev"]))
    out["clouds_over_ranges_host"] = float(np.median(t["clouds_host"]) / np.median(t["ranges_host"]))
    return out


def bench_odom(ctx, beams, R, steps, repeats):
    laser = LASERS[beams]
    scans = make_log(laser, steps)
    xyz1, valid1 = to_clouds(scans, laser)
    ranges = np.ascontiguousarray(np.repeat(scans[:, None, :], R, axis=1))
    stamps = np.repeat(0.1 * np.arange(steps)[:, None], R, axis=1)
    p_x, p_v = ctx.alloc(xyz1.nbytes), ctx.alloc(valid1.nbytes)          # one resident block; every track reads it
    ctx.upload(p_x, xyz1), ctx.upload(p_v, valid1)
    o_r, o_c = api.PlicpOdometry(ctx, R, laser=laser), api.PlicpOdometry(ctx, R)

    def ranges_host():
        o_r.reset()
        t0 = time.perf_counter()
        o_r.process_many(ranges, stamps)
        return time.perf_counter() - t0

    def clouds_dev():
        o_c.reset()
        t0 = time.perf_counter()
        o_c.process_many_clouds_dev(steps, beams, [p_x] * R, [p_v] * R, None, 1, stamps)
        return time.perf_counter() - t0

    rec_r = o_r.process_many(ranges, stamps)
    o_c.reset()
    rec_c = o_c.process_many_clouds_dev(steps, beams, [p_x] * R, [p_v] * R, None, 1, stamps)
    ranges_host(), clouds_dev()
    t = alternate({"ranges_host": ranges_host, "clouds_dev": clouds_dev}, repeats)
    o_r.close(), o_c.close()
    ctx.free(p_x), ctx.free(p_v)
    d = np.abs(rec_c["base_in_odom"] - rec_r["base_in_odom"])
    return {"what": "odometry", "points": beams, "tracks": R, "steps": steps,
            "valid_ranges_clouds": [int(rec_r["valid"].sum()), int(rec_c["valid"].sum())],
            "keyframes_ranges_clouds": [int((rec_r["flags"] & 2 > 0).sum()), int((rec_c["flags"] & 2 > 0).sum())],
            "max_abs_pose_clouds_minus_ranges": float(d.max()),
            "ranges_host_ms": spread(t["ranges_host"], 1e3), "clouds_dev_ms": spread(t["clouds_dev"], 1e3),
            "clouds_dev_us_per_scan": spread(t["clouds_dev"], 1e6 / (R * steps)),
            "clouds_over_ranges": float(np.median(t["clouds_dev"]) / np.median(t["ranges_host"]))}


def make_messages(n_scans, beams, seed=3):
    """400 Hz IMU and 50 Hz odometry around n_scans scans at 10 Hz (80 ms each), as tools/msync_bench.py makes them."""
    rng = np.random.default_rng(seed)
    t0, period, dur = 100.0, 0.1, 0.08
    scan_t = t0 + period * np.arange(n_scans)
    t_end = scan_t[-1] + dur + 0.5
    imu_t = np.arange(t0 - 0.3, t_end, 1.0 / 400.0)
    imu_t += rng.uniform(-0.2, 0.2, len(imu_t)) / 400.0
    odom_t = np.arange(t0 - 0.3, t_end, 1.0 / 50.0)
    odom_t += rng.uniform(-0.2, 0.2, len(odom_t)) / 50.0
    s = imu_t - t0
    imu_w = np.stack([0.0 * s, 0.0 * s, 0.05 + 0.02 * np.sin(0.5 * s)], 1)
    s = odom_t - t0
    yaw = 0.05 * s
    pos = np.stack([0.4 * s, 0.0 * s, 0.0 * s], 1)
    quat = np.stack([0 * s, 0 * s, np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    when = scan_t + dur + 0.02
    return {"scan_t": scan_t, "scan_tinc": np.full(n_scans, dur / (beams - 1), np.float32), "imu_t": imu_t, "imu_w": imu_w,
            "odom_t": odom_t, "odom_pos": pos, "odom_quat": quat,
            "imu_seen": np.searchsorted(imu_t, when, side="right").astype(np.int64),
            "odom_seen": np.searchsorted(odom_t, when, side="right").astype(np.int64)}


def bench_chain(ctx, beams, R, steps, repeats):
    laser = LASERS[beams]
    scans = make_log(laser, steps)
    msg = make_messages(steps, beams)
    hdr = (np.float32(laser.angle_min), np.float32(laser.angle_increment), np.float32(laser.range_min), np.float32(laser.range_max))
    stamps = np.repeat(msg["scan_t"][:, None], R, axis=1)
    words = api.MSYNC_RECORD.itemsize // 4
    d_r = ctx.alloc(scans.nbytes)
    ctx.upload(d_r, scans)
    blocks = [(ctx.alloc(steps * beams * 12), ctx.alloc(steps * beams), ctx.alloc(steps * api.MSYNC_RECORD.itemsize)) for _ in range(R)]
    nodes = [api.MotionSync(ctx) for _ in range(R)]
    o = api.PlicpOdometry(ctx, R)
    last = {}

    def chain():
        o.reset()
        for ms in nodes:
            ms.reset()
        t0 = time.perf_counter()
        for ms, (d_x, d_v, d_rec) in zip(nodes, blocks):
            ms.push_imu(msg["imu_t"], msg["imu_w"])
            ms.push_odom(msg["odom_t"], msg["odom_pos"], msg["odom_quat"])
            ms.scans_dev(hdr, beams, d_r, beams, msg["scan_t"], msg["scan_tinc"], d_x, d_v, d_rec, msg["imu_seen"], msg["odom_seen"])
        t1 = time.perf_counter()
        last["rec"] = o.process_many_clouds_dev(steps, beams, [b[0] for b in blocks], [b[1] for b in blocks], [b[2] for b in blocks],
                                                words, stamps)
        t2 = time.perf_counter()
        last["odom"] = t2 - t1
        return t2 - t0

    chain()
    chain()
    t, t_odo = [], []
    for _ in range(repeats):
        t.append(chain())
        t_odo.append(last["odom"])
    rec = last["rec"]
    status = np.zeros(steps, api.MSYNC_RECORD)
    ctx.download(blocks[0][2], status)
    o.close()
    for ms in nodes:
        ms.close()
    ctx.free(d_r)
    for b in blocks:
        for p in b:
            ctx.free(p)
    return {"what": "chain", "points": beams, "tracks": R, "steps": steps, "corrected_per_node": int((status["status"] > 0).sum()),
            "taken": int((rec["iterations"] >= 0).sum()), "valid": int(rec["valid"].sum()),
            "chain_ms": spread(t, 1e3), "odometry_enqueue_to_return_ms": spread(t_odo, 1e3),
            "chain_us_per_scan": spread(t, 1e6 / (R * steps))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1,64,512,4096")
    ap.add_argument("--tracks", default="1,16,256")
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    ctx = api.Context(0)  # raises without a GPU: nothing of the device path is measured on a CPU
    out = []
    for beams in (360, 1081):
        for B in (int(v) for v in a.sizes.split(",")):
            out.append(bench_pairs(ctx, beams, B, a.repeats, 20 if B <= 64 else 3))
            print(json.dumps(out[-1]), flush=True)
        for R in (int(v) for v in a.tracks.split(",")):
            out.append(bench_odom(ctx, beams, R, a.steps, a.repeats))
            print(json.dumps(out[-1]), flush=True)
        for R in (int(v) for v in a.tracks.split(",")):
            out.append(bench_chain(ctx, beams, R, a.steps, a.repeats))
            print(json.dumps(out[-1]), flush=True)
    print(json.dumps({"plicp_cloud_bench": out}))
    ctx.close()


if __name__ == "__main__":
    main()
