"""GMapping count map on the GPU: one JSON line.

  node callback   lslam_gmap_compute_map on a 1081-beam synth scan, default node box (1600^2): device time (HIP-event sums of
                  its kernels) and end-to-end wall time per call including the 2.56 MB int8 read back
  accumulate      --scans x 1081-beam synth scans along a synth trajectory into one 1600^2 map: device time and scans/s

The reference's CPU time per callback is in tests/golden/gmapping_golden.npz (ref_cpu_callback_s, measured on the host that
generated the fixture; printed here as recorded, not re-measured).

    python tools/gmapping_bench.py [--scans 4096] [--reps 50]
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


def device_ms(ctx) -> float:
    return sum(ms for _, ms in ctx.profile_read().values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    ctx = api.Context(0)
    laser = synth.Laser()
    world = synth.arena(size=50.0, n_axis=10, n_rot=4, seed=3)
    scan = synth.cast_scan(world, (0.0, 0.0, 0.0), laser).astype(np.float32)
    m = api.GMappingMap(ctx)
    m.set_laser(laser.n_ranges, np.float32(laser.angle_min), np.float32(laser.angle_increment))
    for _ in range(a.warmup):
        m.compute_map(scan)
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(a.reps):
        m.compute_map(scan)
    ctx.profile(False)
    node_dev = device_ms(ctx) / a.reps
    t0 = time.perf_counter()
    for _ in range(a.reps):
        m.compute_map(scan)
    node_e2e = (time.perf_counter() - t0) * 1e3 / a.reps

    poses = synth.trajectory(world, a.scans, seed=4)
    ranges = np.stack([synth.cast_scan(world, tuple(p), laser) for p in poses]).astype(np.float32)
    m.reset()
    m.integrate(ranges, poses)  # warm-up: grows the scratch buffers
    m.reset()
    ctx.profile_reset()
    ctx.profile(True)
    t0 = time.perf_counter()
    m.integrate(ranges, poses)
    wall = time.perf_counter() - t0
    ctx.profile(False)
    per_kernel = ctx.profile_read()
    acc_dev = sum(ms for _, ms in per_kernel.values())
    st = m.stats()

    gold = np.load(ROOT / "tests" / "golden" / "gmapping_golden.npz")
    ref = gold["ref_cpu_callback_s"]
    print(json.dumps({
        "metric": "gmapping_map",
        "node_callback_device_ms": round(node_dev, 4),
        "node_callback_e2e_ms": round(node_e2e, 4),
        "accumulate_scans": a.scans,
        "accumulate_device_ms": round(acc_dev, 3),
        "accumulate_scans_per_s_device": round(a.scans / (acc_dev * 1e-3), 1),
        "accumulate_wall_ms": round(wall * 1e3, 3),
        "accumulate_kernels_ms": {k: round(v[1], 3) for k, v in sorted(per_kernel.items())},
        "accumulate_stats": st,
        "reference_cpu_callback_ms_fixture_host": [round(ref[0] * 1e3, 3), round(ref[1] * 1e3, 3)],
    }))
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
