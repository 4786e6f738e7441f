#!/usr/bin/env python3
"""Timing of lesson5's synchronisation on the device: a log of 64 / 512 / 4096 scans of 1081 beams at 10 Hz with
400 Hz IMU and 50 Hz odometry, raw messages in and de-skewed clouds out, through

  (a) lslam_msync_scans (host form: messages and ranges from host memory, one wait),
  (b) lslam_msync_scans_dev (ranges and outputs resident in HBM; timed to the end of the stream), and
  (c) the same log synchronised on the host by the plain-Python restatement of the node (tests/msync_restatement.py) and
      handed to lslam_deskew_batch -- what a caller had to do before; its two parts are timed separately.

Every size is warmed up on every route first; the routes then alternate REPEATS times in one process and the JSON line
carries median, min and max of each.  The routes' records are compared (equal but for odom_incre, which the device libm
computes on route a / b) and their clouds (within the de-skew's 4e-6 m).  No threshold: the figures are reported.
Usage: python tools/msync_bench.py [--repeats N] [--sizes 64,512,4096]"""
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
sys.path.insert(0, str(ROOT / "tests"))  # the restatement
import lslam  # noqa: E402,F401
from lslam_amd import api  # noqa: E402
import msync_restatement as mr  # noqa: E402

f32 = np.float32
N, PERIOD, DUR, T0 = 1081, 0.1, 0.08, 100.0


def make_log(n_scans, seed=3):
    rng = np.random.default_rng(seed)
    a = -0.75 * math.pi + np.arange(N) * (1.5 * math.pi / (N - 1))
    base = np.stack([(4.0 + 0.02 * k) / np.maximum(np.abs(np.cos(a)), np.abs(np.sin(a))) + rng.normal(0, 0.01, N) for k in range(64)])
    ranges = np.ascontiguousarray(base[np.arange(n_scans) % 64], dtype=np.float32)
    scan_t = T0 + PERIOD * np.arange(n_scans)
    t_end = scan_t[-1] + DUR + 0.5
    imu_t = np.arange(T0 - 0.3, t_end, 1.0 / 400.0)
    imu_t += rng.uniform(-0.2, 0.2, len(imu_t)) / 400.0
    odom_t = np.arange(T0 - 0.3, t_end, 1.0 / 50.0)
    odom_t += rng.uniform(-0.2, 0.2, len(odom_t)) / 50.0
    s = imu_t - T0
    imu_w = np.stack([0.02 * np.sin(3 * s), 0.02 * np.cos(2 * s), 0.3 + 0.1 * np.sin(0.5 * s)], 1)
    s = odom_t - T0
    yaw = 0.3 * s
    pos = np.stack([6.0 * np.sin(0.05 * s), 6.0 * np.cos(0.04 * s), 0.0 * s], 1)  # below 16 m
    quat = np.stack([0 * s, 0 * s, np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    when = scan_t + DUR + 0.02
    return {"ranges": ranges, "scan_t": scan_t, "scan_tinc": np.full(n_scans, DUR / (N - 1), np.float32), "imu_t": imu_t, "imu_w": imu_w,
            "odom_t": odom_t, "odom_pos": pos, "odom_quat": quat,
            "imu_seen": np.searchsorted(imu_t, when, side="right").astype(np.int64),
            "odom_seen": np.searchsorted(odom_t, when, side="right").astype(np.int64),
            "laser": (f32(a[0]), f32(1.5 * math.pi / (N - 1)), f32(0.1), f32(30.0))}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def bench(ctx, n_scans, repeats):
    log = make_log(n_scans)
    ms, dk = api.MotionSync(ctx), api.Deskewer(ctx)
    d_r, d_x, d_v = ctx.alloc(log["ranges"].nbytes), ctx.alloc(n_scans * N * 12), ctx.alloc(n_scans * N)
    d_rec = ctx.alloc(n_scans * api.MSYNC_RECORD.itemsize)
    ctx.upload(d_r, log["ranges"])

    def push():
        ms.push_imu(log["imu_t"], log["imu_w"])
        ms.push_odom(log["odom_t"], log["odom_pos"], log["odom_quat"])

    def host_form():
        ms.reset()
        t0 = time.perf_counter()
        push()
        out = ms.scans(log["laser"], log["ranges"], log["scan_t"], log["scan_tinc"], log["imu_seen"], log["odom_seen"])
        return time.perf_counter() - t0, out

    def dev_form():
        ms.reset()
        t0 = time.perf_counter()
        push()
        ms.scans_dev(log["laser"], N, d_r, N, log["scan_t"], log["scan_tinc"], d_x, d_v, d_rec, log["imu_seen"], log["odom_seen"])
        ctx.synchronize()
        return time.perf_counter() - t0

    def host_sync():
        t0 = time.perf_counter()
        node = mr.Node(N)
        node.push_imu(log["imu_t"], log["imu_w"])
        node.push_odom(log["odom_t"], log["odom_pos"], log["odom_quat"])
        recs = [node.scan(log["scan_t"][k], log["scan_tinc"][k], log["imu_seen"][k], log["odom_seen"][k]) for k in range(n_scans)]
        ks = [k for k, r in enumerate(recs) if r["status"] == mr.CORRECTED]
        params = [api.DeskewParams(*log["laser"], r["scan_time_start"], r["time_increment"], 1, 1, r["start_odom_time"],
                                   r["end_odom_time"], *[float(v) for v in r["odom_incre"]], 0.0) for r in (recs[k] for k in ks)]
        times = [recs[k]["imu_time"] if recs[k]["n_imu"] else np.zeros(1) for k in ks]
        rots = [recs[k]["imu_rot"] if recs[k]["n_imu"] else np.zeros((1, 3)) for k in ks]
        t1 = time.perf_counter()
        xyz, valid = dk.batch(log["ranges"][[k - 1 for k in ks]], params, times, rots)
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, recs, ks, xyz, valid

    # warm-up of every route, and the comparison
    _, (xyz, valid, rec) = host_form()
    dev_form()
    x2, v2, r2 = np.zeros_like(xyz), np.zeros(valid.shape, np.uint8), np.zeros_like(rec)
    ctx.download(d_x, x2), ctx.download(d_v, v2), ctx.download(d_rec, r2)
    dev_is_host = x2.tobytes() == xyz.tobytes() and np.array_equal(v2.astype(bool), valid) and r2.tobytes() == rec.tobytes()
    _, _, recs, ks, hx, hv = host_sync()
    same_records = all(
        (d["status"], d["n_imu"], d["scan_time_start"], d["time_increment"], d["start_odom_time"], d["end_odom_time"], d["imu_front"],
         d["odom_front"], d["start_odom_index"], d["end_odom_index"]) ==
        (r["status"], r["n_imu"], r["scan_time_start"], r["time_increment"], r["start_odom_time"], r["end_odom_time"], r["imu_front"],
         r["odom_front"], r["start_odom_index"], r["end_odom_index"]) for d, r in zip(rec, recs))
    incre = max(float(np.abs(rec["odom_incre"][k].astype(np.float64) - recs[k]["odom_incre"]).max()) for k in ks)
    cloud = float(np.nanmax(np.abs(xyz[ks].astype(np.float64) - hx.astype(np.float64))))
    same_valid = bool(np.array_equal(valid[ks], hv) and np.array_equal(np.isnan(xyz[ks]), np.isnan(hx)))
    growths = ms.stats()["growths"] + dk.stats()["growths"]
    t_host, t_dev, t_sync, t_dsk = [], [], [], []
    for _ in range(repeats):  # alternating
        t_host.append(host_form()[0])
        t_dev.append(dev_form())
        a, b = host_sync()[:2]
        t_sync.append(a)
        t_dsk.append(b)
    st = ms.stats()
    grown = st["growths"] + dk.stats()["growths"] - growths
    for p in (d_r, d_x, d_v, d_rec):
        ctx.free(p)
    ms.close()
    dk.close()
    before = [a + b for a, b in zip(t_sync, t_dsk)]
    return {"scans": n_scans, "beams": N, "imu_messages": len(log["imu_t"]), "odom_messages": len(log["odom_t"]),
            "corrected": len(ks), "msync_host_form_s": spread(t_host), "msync_dev_form_s": spread(t_dev),
            "host_restatement_s": spread(t_sync), "deskew_batch_s": spread(t_dsk), "host_route_s": spread(before),
            "host_form_us_per_scan": 1e6 * statistics.median(t_host) / n_scans,
            "dev_form_us_per_scan": 1e6 * statistics.median(t_dev) / n_scans,
            "host_route_us_per_scan": 1e6 * statistics.median(before) / n_scans,
            "records_equal": bool(same_records), "dev_form_equals_host_form": bool(dev_is_host), "valid_equal": same_valid,
            "worst_odom_incre_difference_m": incre, "worst_cloud_difference_m": cloud, "growths_after_warmup": grown}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="64,512,4096")
    a = ap.parse_args()
    ctx = api.Context(0)  # raises without a GPU: nothing here is measured on a CPU
    out = {"msync": [bench(ctx, int(s), a.repeats if int(s) <= 512 else max(3, a.repeats // 2)) for s in a.sizes.split(",")]}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
