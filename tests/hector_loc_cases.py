"""Scenarios for the Hector localiser (lslam_hector_loc_*, api.HectorLocaliser): R trackers on ONE finished map, each entry a
matchData from the tracker's own last pose (or a hint) and no map update.  The yardstick is always a lslam_hector processor on
the same map with both update thresholds +inf (x > +inf is false for every float, NaN included: the gate never fires), run
alone over the tracker's taken entries -- a path tests/test_hector_stream_gpu.py holds to the reference's own processor.

  (a) logs(levels, R)   tracker r streams edges(levels)' scans in LOG_ORDER rolled by r.  LOG_ORDER moves the one-point scan
                        behind the empty one, so that consecutive steps of a block see a LONG container (scan 4), the EMPTY one
                        (scan 5) and a SHORT one (scan 10, one point): what a block that loops could carry over in LDS or in
                        registers.  Streamed in calls of 1, 2, 7 and 2 steps (CALLS) and in one call of all 12.
  (b) FORMS             the first 12 scans of chain60 (1081 beams, 1024^2 x 3 levels) under LSLAM_GN_THREADS 256 and 512 -- the
                        register form -- and container-form calls padded to 1800 points (beyond 512 x 3: staged in LDS) and to
                        7400 (beyond the 7168 that fit 56 KiB: read from memory)
  (c) ragged            hector_fleet_cases.ragged(): R = 5 under RAGGED_MASK in its two calls
  (d) TAKE              per-tracker take patterns of the cloud form on a log of hector_sync_cases

Pure numpy; tests/test_hector_loc_cases.py checks these claims without a GPU, tests/test_hector_loc_gpu.py runs them."""
import functools

import numpy as np

import hector_fleet_cases as F
import hector_stream_cases as S
import hector_sync_cases as H

f32 = np.float32
INF = float("inf")

LOG_ORDER = [0, 1, 2, 3, 4, S.EDGE_EMPTY, 10, 7, 8, 9, 6, 11]
LONG_EMPTY_SHORT = (4, S.EDGE_EMPTY, 10)
CALLS = [(0, 1), (1, 3), (3, 10), (10, 12)]  # 1, 2, 7 and 2 steps
MAX_R = 5                                     # rolls that keep LONG_EMPTY_SHORT consecutive (none wraps it around the end)


def log_order(r):
    n = len(LOG_ORDER)
    return [LOG_ORDER[(k + r) % n] for k in range(n)]


@functools.lru_cache(maxsize=None)
def logs(levels, R):
    sc = S.edges(levels)
    members = []
    for r in range(R):
        order = log_order(r)
        members.append(F.Member(sc, [sc.containers[k] for k in order], sc.ranges[order], None, False))
    return F.Fleet(members, np.ones((len(LOG_ORDER), R), bool), list(CALLS))


# ---- (b) name -> (LSLAM_GN_THREADS, points every container is padded to or None, the form both sides must select)
FORMS = {"reg256": (256, None, "reg256"), "reg512": (512, None, "reg512"), "lds512": (512, 1800, "fast-lds"),
         "mem512": (512, 7400, "fast-mem")}
FORM_STEPS = 12
FORM_R = 3


def padded(points, n):
    """A container repeated up to n points (a point that appears twice is a point like any other to the matcher)."""
    p = np.asarray(points, f32).reshape(-1, 2)
    return np.ascontiguousarray(np.tile(p, (-(-n // len(p)), 1))[:n])


@functools.lru_cache(maxsize=None)
def form_logs(name):
    """Tracker r streams chain60's first FORM_STEPS scans rolled by r; padded: every container but tracker r's step r is cut to
    half the padding, so that a tracker's own longest container is the call's and the lengths still differ."""
    _, pad, _ = FORMS[name]
    sc = S.chain60()
    members = []
    for r in range(FORM_R):
        conts = [sc.containers[(k + r) % FORM_STEPS] for k in range(FORM_STEPS)]
        if pad is not None:
            conts = [padded(c, pad if k % FORM_R == r else pad // 2) for k, c in enumerate(conts)]
        members.append(F.Member(sc, conts, None, None, False))
    return F.Fleet(members, np.ones((FORM_STEPS, FORM_R), bool), [(0, FORM_STEPS)])


# ---- (d)
TAKE_LOGS = ("imu_gap", "non_monotone")  # isolated refusals; runs of two and three refusals


def status_take(name):
    return np.array(H.STATUSES[name]) > 0


def hint_far(sc):
    """A start pose so far outside the map that every point of every container is out of bounds on every level."""
    return np.array([1.0e4 * S.CELL * sc.n, -1.0e4 * S.CELL * sc.n, 0.5], f32)
