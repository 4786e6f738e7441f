#!/usr/bin/env python3
"""Measurements for lesson1's batched corner extraction, in one run: B = 64, 512 and 4096 scans of 1081 beams
from the bench world (synth.arena(), sigma = 0.01 noise, 1 % dropouts) through

  host form    lslam_features_batch: pinned staging up and down, one launch, one wait (host clock around the call)
  single loop  the same scans as B successive one-scan calls of the same entry point
  dev form     lslam_features_batch_dev with every buffer resident: host clock over 20 calls and one synchronise
  kernel       HIP events around each of 20 launches of the kernel alone

The host form and the single loop alternate inside one process, REPEATS times after a warm-up of every shape, and their outputs
are compared bit for bit at the sizes timed; every figure is a median with its (min, max).  The reference's CPU time per scan
printed beside them is the one recorded in tests/golden/features_golden.npz: a HOST figure from the machine that wrote the
golden, not measured here.  Usage: python tools/features_bench.py [--repeats N] [--sizes 64,512,4096]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import lslam  # noqa: E402,F401
from lslam_amd import api, synth  # noqa: E402

UNIQUE = 256  # distinct ray-cast scans; larger batches tile them


def make_scans(n_scans, seed=7):
    world = synth.arena()
    laser = synth.Laser()
    rng = np.random.default_rng(seed)
    base = []
    while len(base) < min(n_scans, UNIQUE):
        x, y = rng.uniform(-35, 35, 2)
        if synth.point_is_free(world, x, y, 0.8):
            base.append(synth.cast_scan(world, (x, y, rng.uniform(-3, 3)), laser, 0.01, 0.01, rng))
    return np.stack([base[k % len(base)] for k in range(n_scans)]).astype(np.float32)


def spread(xs, scale=1.0):
    return {"median": scale * statistics.median(xs), "min": scale * min(xs), "max": scale * max(xs)}


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def bench(ctx, B, repeats):
    ranges = make_scans(B)
    n = ranges.shape[1]
    f = api.FeatureExtractor(ctx)

    def singles():
        return [f.extract(ranges[k:k + 1]) for k in range(B)]

    batch = f.extract(ranges)  # warm-up of both, and the comparison
    one = singles()
    identical = all(same([a[k:k + 1] for a in batch], one[k]) for k in range(B))
    growths = f.stats()["growths"]
    t_batch, t_loop = [], []
    for _ in range(repeats):  # alternating
        t0 = time.perf_counter()
        f.extract(ranges)
        t_batch.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        singles()
        t_loop.append(time.perf_counter() - t0)
    grew = f.stats()["growths"] - growths
    # the _dev form and the kernel alone: buffers resident
    p = [ctx.alloc(ranges.nbytes), ctx.alloc(B * n * 4), ctx.alloc(B * 120 * 4), ctx.alloc(B * 32), ctx.alloc(B * n * 4)]
    ctx.upload(p[0], ranges)

    def dev():
        f.extract_dev(B, n, p[0], n, p[1], p[2], p[3], p[4])

    dev()
    ctx.synchronize()
    image = np.zeros((B, n), np.float32)
    ctx.download(p[1], image)
    identical = identical and image.tobytes() == batch[0].tobytes()
    waits = f.stats()["host_waits"]
    t_dev = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(20):
            dev()
        ctx.synchronize()
        t_dev.append((time.perf_counter() - t0) / 20)
    dev_waits = f.stats()["host_waits"] - waits
    t_kernel = []
    ctx.profile(True)
    ctx.profile_only("features")
    for _ in range(repeats):
        ctx.profile_reset()
        for _ in range(20):
            dev()
        ctx.synchronize()
        launches, ms = ctx.profile_read().get("features", (0, 0.0))
        t_kernel.append(1e-3 * ms / max(launches, 1))
    ctx.profile(False)
    ctx.profile_only(None)
    for q in p:
        ctx.free(q)
    f.close()
    mb, ml = statistics.median(t_batch), statistics.median(t_loop)
    return {"B": B, "beams": n, "bit_identical": bool(identical), "corners_per_scan": float(batch[2]["n_corners"].mean()),
            "host_form_s": spread(t_batch), "single_loop_s": spread(t_loop), "speedup_median": ml / mb,
            "host_form_us_per_scan": spread(t_batch, 1e6 / B), "single_us_per_scan": spread(t_loop, 1e6 / B),
            "dev_form_call_us": spread(t_dev, 1e6), "dev_form_us_per_scan": spread(t_dev, 1e6 / B),
            "kernel_us": spread(t_kernel, 1e6), "kernel_us_per_scan": spread(t_kernel, 1e6 / B),
            "growths_after_warmup": grew, "dev_form_host_waits": dev_waits}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sizes", default="64,512,4096")
    a = ap.parse_args()
    ctx = api.Context(0)  # raises without a GPU: nothing here is measured on a CPU
    golden = ROOT / "tests" / "golden" / "features_golden.npz"
    ref = float(np.load(golden)["ref_cpu_scan_s"]) if golden.exists() else None
    out = {"features_batch": [bench(ctx, int(B), a.repeats) for B in a.sizes.split(",")],
           "reference_cpu_us_per_scan_recorded_in_golden": None if ref is None else 1e6 * ref}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
