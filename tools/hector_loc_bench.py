#!/usr/bin/env python3
"""R trackers localising on one finished map, on the workload of tools/hector_stream_bench.py (1024^2 x 3 levels, a 300-scan log
of 1081 beams, calls of 16 steps).  The map is built once from the log and then only read.  Tracker r streams the log there
and back starting r scans in, so consecutive scans of a tracker are always 0.05 m apart and no chain is ever lost.

  (A) localiser   api.HectorLocaliser.process_many: R trackers, 2 launches per chunk of a call
  (B) solo        the same trackers as +inf-threshold HectorProcessors, one after another through process_many
  (C) host loop   OccGridMap.setScan + matchContainer per scan, chained on the host

(B) and (C) run their trackers one after another, so their aggregate rate does not depend on how many there are: they are
measured over the first min(R, --baseline-trackers) trackers.  Inputs are built before the clock starts.  A warm-up pass of
each leg, then --repeats timed windows with the legs alternating, a window being as many whole passes as fill --window
seconds (every pass ends in the call's own wait for the stream); printed as median (min-max) scans/s.  One more localiser pass per R
under HIP-event timing gives the tracking and container kernels' time per launch (lslam_profile_read).  Last:
write_logodds / write_logodds_dev of the 1024^2 level 0, in ms (the _dev form with the wait for the stream).  Prints a table
and one JSON line."""
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


def spread(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def show(s):
    return "%.0f (%.0f-%.0f)" % (s["median"], s["min"], s["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trackers", type=int, nargs="*", default=[1, 4, 16, 64, 256, 1024])
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--baseline-trackers", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.25, help="seconds a timed window lasts at least (whole passes)")
    a = ap.parse_args()
    S = a.scans
    laser = synth.Laser()
    scan = api.hector_scan(laser)
    n, cell, levels = 1024, 0.05, 3
    off = (n * cell * 0.5, n * cell * 0.5)
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=3)
    path = synth.trajectory(world, S, step=0.05, seed=3, bounds=6.0)
    rng = np.random.default_rng(1)
    ranges = np.stack([synth.cast_scan(world, t, laser, 0.01, 0.0, rng) for t in path]).astype(np.float32)

    ctx = api.Context(0)
    m = api.OccGridMap(ctx, n, n, cell, off, levels=levels)
    m.setUpdateOccupiedFactor(0.9)
    builder = api.HectorProcessor(m)
    builder.set_update_thresholds(-1.0, -1.0)  # the gate always passes: every scan of the log is mapped
    hints = np.array(path, np.float32)
    builder.process_many(ranges, scan, hints, [1] * S)
    builder.close()
    plane0 = m.logodds(0)

    there_and_back = np.concatenate([np.arange(S), np.arange(S - 2, 0, -1)])

    def log_of(r):  # [S] scan indices of tracker r
        return there_and_back[(np.arange(S) + r) % len(there_and_back)]

    res = {"config": "hector localiser: 1024^2 x 3 levels, 1081 beams, %d scans per tracker, calls of %d steps" % (S, a.chunk),
           "repeats": a.repeats, "baseline_trackers": a.baseline_trackers, "by_trackers": {}}
    print("%6s  %-28s %-28s %-28s %s" % ("R", "localiser scans/s", "solo scans/s", "host loop scans/s", "hl_track us/launch (per step)"))
    for R in a.trackers:
        B = min(R, a.baseline_trackers)
        idx = np.stack([log_of(r) for r in range(R)], axis=1)  # [S, R]
        start = np.array(path, np.float32)[idx[0]]
        calls = [np.ascontiguousarray(ranges[idx[lo:lo + a.chunk]]) for lo in range(0, S, a.chunk)]
        loc = api.HectorLocaliser(m, R)
        solos = []
        for _ in range(B):
            h = api.HectorProcessor(m)
            h.set_update_thresholds(float("inf"), float("inf"))
            solos.append(h)

        def leg_loc():
            loc.set_poses(start)
            return np.concatenate([loc.process_many(c, scan) for c in calls])

        def leg_solo():
            out = []
            for r, h in enumerate(solos):
                first = h.process_many(ranges[idx[:1, r]], scan, start[r:r + 1])  # (its chain starts where the tracker's does)
                out.append(np.concatenate([first] + [h.process_many(ranges[idx[max(lo, 1):lo + a.chunk, r]], scan)
                                                     for lo in range(0, S, a.chunk)]))
            return np.stack(out, axis=1)

        def leg_host():
            out = np.zeros((S, B, 3), np.float32)
            for r in range(B):
                pose = start[r]
                for k in range(S):
                    m.setScan(ranges[idx[k, r]], scan)
                    pose, _ = m.matchContainer(pose)
                    out[k, r] = pose
            return out

        legs = {"localiser": (leg_loc, R), "solo": (leg_solo, B), "host_loop": (leg_host, B)}
        got = {}
        for name, (fn, _) in legs.items():
            got[name] = fn()
        rates = {k: [] for k in legs}
        for _ in range(a.repeats):
            for name, (fn, trackers) in legs.items():
                ctx.synchronize()
                passes, t0 = 0, time.perf_counter()
                while passes == 0 or time.perf_counter() - t0 < a.window:  # whole passes until the window is filled
                    got[name] = fn()
                    passes += 1
                rates[name].append(passes * trackers * S / (time.perf_counter() - t0))
        row = {name: spread(v) for name, v in rates.items()}
        row["records_bit_equal_to_solo"] = bool(np.ascontiguousarray(got["localiser"][:, :B]).tobytes() == got["solo"].tobytes())
        before = loc.stats()
        ctx.profile(True)
        ctx.profile_reset()
        leg_loc()
        ctx.synchronize()
        ctx.profile(False)
        prof = ctx.profile_read()
        st = loc.stats()
        row["kernel_us_per_launch"] = {k: round(1e3 * ms / max(launches, 1), 2) for k, (launches, ms) in prof.items()
                                       if k.startswith("hl_")}
        launches = st["track_launches"] - before["track_launches"]
        row["hl_track_us_per_step"] = round(1e3 * prof["hl_track"][1] / S, 2)
        row["launches_per_call"] = (st["launches"] - before["launches"]) / (st["calls"] - before["calls"])
        row["chunks_per_call"] = launches / (st["calls"] - before["calls"])
        row["host_syncs_per_call"] = (st["host_syncs"] - before["host_syncs"]) / (st["calls"] - before["calls"])
        res["by_trackers"][R] = row
        print("%6d  %-28s %-28s %-28s %.1f (%.1f)" % (R, show(row["localiser"]), show(row["solo"]), show(row["host_loop"]),
                                                    row["kernel_us_per_launch"]["hl_track"], row["hl_track_us_per_step"]), flush=True)
        loc.close()
        for h in solos:
            h.close()

    other = api.OccGridMap(ctx, n, n, cell, off, levels=levels)
    host_ms, dev_ms = [], []
    for _ in range(a.repeats + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        other.write_logodds(0, plane0)
        host_ms.append(1e3 * (time.perf_counter() - t0))
        src = m.cells_dev_ptr(0)
        ctx.synchronize()
        t0 = time.perf_counter()
        other.write_logodds_dev(0, src)
        ctx.synchronize()
        dev_ms.append(1e3 * (time.perf_counter() - t0))
    assert other.logodds(0).tobytes() == plane0.tobytes()
    res["write_logodds_ms"], res["write_logodds_dev_ms"] = spread(host_ms[1:], 4), spread(dev_ms[1:], 4)
    print("1024^2 level 0, ms: write_logodds %(median).4f (%(min).4f-%(max).4f)" % res["write_logodds_ms"],
          "  write_logodds_dev %(median).4f (%(min).4f-%(max).4f)" % res["write_logodds_dev_ms"])
    print(json.dumps(res))
    other.close()
    m.close()


if __name__ == "__main__":
    main()
