#!/usr/bin/env python3
"""R streamed HectorProcessors, each on its own map, over the workload of tools/hector_stream_bench.py (1024^2 x 3 levels, 300
scans of 1081 beams, every scan matched from its hint and mapped, calls of 16 steps; member r streams the log rolled by r
scans), in one process:

  (A) solo    the members one after another through their own process_many_points -- R chains per step
  (B) fleet   api.HectorFleet.process_many_points -- one chain per step

Both legs take the containers packed per call (built before the clock starts) and run on maps reset before every pass.  A
warm-up pass of each, then --repeats passes with the legs alternating; per leg the median and the spread (max - min) of the
aggregate member-scans/s.  --profile adds one fleet pass with HIP-event times per hf_* launch.  The last pass's records of
the two legs are compared bit for bit.  Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    R, S = a.members, a.scans
    laser = synth.Laser()
    n, cell, levels = 1024, 0.05, 3
    off = (n * cell * 0.5, n * cell * 0.5)
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=3)
    path = synth.trajectory(world, S, step=0.05, seed=3, bounds=6.0)
    rng = np.random.default_rng(1)
    ranges = np.stack([synth.cast_scan(world, t, laser, 0.01, 0.0, rng) for t in path]).astype(np.float32)
    pts_all = [np.ascontiguousarray(synth.hector_points(r, laser, 1.0 / cell, use_max=20.0), dtype=np.float32) for r in ranges]
    hints_all = np.array([(t + np.array([0.05, -0.04, 0.02])) for t in path], np.float32)
    hints_all[0] = path[0]
    counts_all = np.array([len(p) for p in pts_all], np.int32)

    ctx = api.Context(0)
    maps, procs = [], []
    for r in range(R):
        m = api.OccGridMap(ctx, n, n, cell, off, levels=levels)
        m.setUpdateOccupiedFactor(0.9)
        h = api.HectorProcessor(m)
        h.set_update_thresholds(-1.0, -1.0)  # the gate always passes: every scan is mapped
        maps.append(m)
        procs.append(h)
    fleet = api.HectorFleet(procs)

    # per call: the fleet's packed arrays [step][member], and each member's own
    calls = []
    for lo in range(0, S, a.chunk):
        steps = range(lo, min(lo + a.chunk, S))
        idx = np.array([[(k + r) % S for r in range(R)] for k in steps])  # [steps, R]
        fl = (np.concatenate([pts_all[i] for i in idx.ravel()]), counts_all[idx.ravel()].copy(), hints_all[idx].copy())
        solo = [(np.concatenate([pts_all[i] for i in idx[:, r]]), counts_all[idx[:, r]].copy(), hints_all[idx[:, r]].copy())
                for r in range(R)]
        calls.append((fl, solo))

    def reset():
        for h in procs:
            h.reset()
        ctx.synchronize()

    def leg_solo():
        out = []
        for _, solo in calls:
            out.append(np.stack([procs[r].process_many_points(p, h, counts=c) for r, (p, c, h) in enumerate(solo)], axis=1))
        return np.concatenate(out)

    def leg_fleet():
        return np.concatenate([fleet.process_many_points(p, h, counts=c) for (p, c, h), _ in calls])

    legs = {"solo": leg_solo, "fleet": leg_fleet}
    for fn in legs.values():  # warm-up: allocations, code objects
        reset()
        fn()
    rates = {k: [] for k in legs}
    recs = {}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            reset()
            t0 = time.perf_counter()
            recs[name] = fn()
            rates[name].append(R * S / (time.perf_counter() - t0))
    res = {"config": "hector fleet: 1024^2 x 3 levels, 1081 beams, calls of %d steps" % a.chunk, "members": R, "scans": S,
           "repeats": a.repeats}
    for name, v in rates.items():
        res[name] = {"scans_per_s_median": round(statistics.median(v), 1), "scans_per_s_spread": round(max(v) - min(v), 1),
                     "scans_per_s_min": round(min(v), 1), "scans_per_s_max": round(max(v), 1)}
    res["fleet_over_solo"] = round(res["fleet"]["scans_per_s_median"] / res["solo"]["scans_per_s_median"], 3)
    res["records_bit_equal"] = bool(recs["solo"].tobytes() == recs["fleet"].tobytes())
    if a.profile:
        for name, fn in legs.items():
            reset()
            ctx.profile(True)
            ctx.profile_reset()
            fn()
            ctx.synchronize()
            ctx.profile(False)
            res[name]["kernel_us_per_launch"] = {k: round(1e3 * ms / max(launches, 1), 2)
                                                 for k, (launches, ms) in ctx.profile_read().items()}
    st = fleet.stats()
    res["fleet_launches_per_step"] = st["launches"] / max(st["steps"], 1)
    res["fleet_host_syncs_per_call"] = st["host_syncs"] / max(st["calls"], 1)
    print(json.dumps(res))
    for m in maps:
        m.close()


if __name__ == "__main__":
    main()
