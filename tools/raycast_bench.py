"""Batched OccupancyGrid::RayCast on the device (lslam_occgrid_ray_cast*, csrc/raycast.hip): one JSON line per world.

A 0.05 m occupancy grid is built from synthetic 1081-beam scans of a world (the bench world: bench.py's 80 m arena; the dense
world: its 140 obstacles on 60 m x 60 m), then --poses sensor poses x 1081 beams are cast on it, everything resident in HBM
(the _dev entry points), at max_range 12 and 49.5.  The poses are drawn per world, same count and seed, from that world's free
space (a pose inside an obstacle or outside the map ends every ray at its first sample and measures nothing):
  scans     lslam_occgrid_ray_cast_scans_dev: wall clock around enqueue + synchronise and the HIP-event time of the kernel
            (the library's own per-launch events), best of --reps; scans/s, rays/s and samples/s from the kernel time, the
            samples being what the reference's loop would have tested (lslam_occgrid_ray_cast_stats)
  rays      the same rays through lslam_occgrid_ray_cast_dev with the headings computed on the host
  refresh   the cell plane derived from the counters (k_rc_cells), once per change of the map
  single    --single single-ray host calls (lslam_occgrid_ray_cast with n = 1), per call: what a caller pays who does not batch
  ref_cpu_ns_per_ray   the reference's own compiled RayCast per ray at max_range 12 on a 0.05 m grid, recorded by
            tests/golden/make_raycast_golden.py ON THE HOST THAT RAN IT (one CPU core) -- not measured here, not a GPU figure

The GPU work runs in a child process under its own time limit (--limit seconds).

    python tools/raycast_bench.py [--poses 4096] [--reps 5] [--single 256] [--label TEXT]
"""
from __future__ import annotations

import argparse
import json
import math
import pathlib
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

RES, THR = 0.05, 49.5
MAX_RANGES = (12.0, 49.5)


def free_poses(synth, world, n, half, seed, margin=0.5):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x, y = rng.uniform(-half, half, 2)
        if synth.point_is_free(world, x, y, margin):
            out.append((x, y, rng.uniform(-math.pi, math.pi)))
    return np.asarray(out)


def kernel_ms(ctx, fn, name):
    ctx.profile_reset()
    ctx.profile(True)
    fn()
    ctx.synchronize()
    ctx.profile(False)
    return ctx.profile_read()[name][1]


def run_world(ctx, api, synth, name, world, half, n_map, n_poses, reps, n_single):
    laser = synth.Laser()
    lp = api.laser_params(laser, THR)
    beams = api.OccupancyGrid.laser_beams(lp)
    map_poses = free_poses(synth, world, n_map, half, seed=31)
    ranges = np.stack([synth.ranges_to_f64(synth.cast_scan(world, p, laser)) for p in map_poses])
    og = api.OccupancyGrid.CreateFromScans(ctx, lp, ranges, map_poses, RES)
    w, h, _, _ = og.info()
    cells = og.data()
    poses = free_poses(synth, world, n_poses, half, seed=32)
    d_poses, d_out = ctx.alloc(poses.nbytes), ctx.alloc(n_poses * beams * 8)
    ctx.upload(d_poses, poses)
    headings = poses[:, 2:3] + lp.minimum_angle + np.arange(beams)[None, :] * lp.angular_resolution
    rays = np.stack([np.repeat(poses[:, 0], beams), np.repeat(poses[:, 1], beams), headings.reshape(-1)], axis=1)
    d_rays = ctx.alloc(rays.nbytes)
    ctx.upload(d_rays, rays)
    out = {"metric": "raycast", "world": name, "grid": [w, h], "free_share": round(float((cells == 255).mean()), 3),
           "map_scans": n_map, "poses": n_poses, "beams": beams}
    # the cell plane: derived by the first cast after the counters changed
    out["refresh_kernel_ms"] = round(kernel_ms(ctx, lambda: og.ray_cast_scans_dev(lp, 1, d_poses, 12.0, d_out, beams), "rc_cells"), 4)
    for mr in MAX_RANGES:
        def scans():
            og.ray_cast_scans_dev(lp, n_poses, d_poses, mr, d_out, beams)

        def as_rays():
            og.ray_cast_dev(n_poses * beams, d_rays, None, mr, d_out)

        scans()
        ctx.synchronize()
        s0 = og.ray_cast_stats()["samples"]
        scans()
        samples = og.ray_cast_stats()["samples"] - s0
        walls = []
        for _ in range(reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            scans()
            ctx.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        k_scans = min(kernel_ms(ctx, scans, "rc_scans") for _ in range(reps))
        k_rays = min(kernel_ms(ctx, as_rays, "rc_rays") for _ in range(reps))
        got = np.zeros(n_poses * beams)
        ctx.download(d_out, got)
        n_rays = n_poses * beams
        out[f"max_range_{mr:g}"] = {
            "scans_kernel_ms": round(k_scans, 4), "scans_wall_ms": round(min(walls), 4), "rays_kernel_ms": round(k_rays, 4),
            "scans_per_s": round(n_poses / (k_scans * 1e-3)), "rays_per_s": round(n_rays / (k_scans * 1e-3)),
            "samples": int(samples), "samples_per_ray": round(samples / n_rays, 1),
            "samples_per_s": round(samples / (k_scans * 1e-3)), "ns_per_ray": round(k_scans * 1e6 / n_rays, 3),
            "mean_range_m": round(float(got.mean()), 3), "stopped_share": round(float((got < mr).mean()), 3)}
    one = np.zeros((1, 3))
    t0 = time.perf_counter()
    for i in range(n_single):
        one[0] = rays[(i * 977) % len(rays)]
        og.ray_cast(one, 12.0)
    out["single_ray_call_us"] = round((time.perf_counter() - t0) / max(n_single, 1) * 1e6, 2)
    out["stats"] = og.ray_cast_stats()
    for p in (d_poses, d_out, d_rays):
        ctx.free(p)
    og.close()
    return out


def child(a):
    import lslam  # noqa: F401
    from lslam_amd import api, synth

    ref_ns = None
    golden = ROOT / "tests" / "golden" / "raycast_golden.npz"
    if golden.exists():
        with np.load(golden) as z:
            ref_ns = round(float(z["ref_cpu_ray_s"]) * 1e9, 1)
    ctx = api.Context(0)
    worlds = (("bench", synth.arena(), 36.0, 96), ("dense", synth.arena(size=60.0, n_axis=100, n_rot=40, seed=21), 27.0, 96))
    for name, world, half, n_map in worlds:
        out = run_world(ctx, api, synth, name, world, half, n_map, a.poses, a.reps, a.single)
        out["ref_cpu_ns_per_ray"] = ref_ns
        out["ref_cpu_note"] = "reference RayCast, one CPU core of the host that recorded the golden; max_range 12, 0.05 m cells"
        if a.label:
            out["label"] = a.label
        print(json.dumps(out), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single", type=int, default=256)
    ap.add_argument("--label", default="")
    ap.add_argument("--limit", type=int, default=300, help="seconds the GPU child may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, __file__, "--child", "--poses", str(a.poses), "--reps", str(a.reps), "--single", str(a.single),
           "--label", a.label]
    try:
        p = subprocess.run(cmd, timeout=a.limit)
    except subprocess.TimeoutExpired:
        print(json.dumps({"metric": "raycast", "error": f"the GPU child did not finish within {a.limit} s"}), flush=True)
        return 124
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
