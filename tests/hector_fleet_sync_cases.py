"""Fleets for the Hector fleet's gated forms (lslam_hector_fleet_process_many_clouds[_dev], lslam_hector_fleet_process_many_synced;
api.HectorFleet.process_many_clouds[_dev] / process_synced): the message logs of tests/hector_sync_cases.py, one per member,
laid over a common sequence of steps.  Member m's callback j is step FIRST + j; outside its steps the member is not active.

  ragged64  R = 3 on the three 64-beam logs whose LaserScan header is identical, 14 steps: non_monotone on steps 0-13 (3
            levels), no_lead on steps 2-11 (2 levels), window_sizes on steps 1-8 (3 levels, a smaller map).  By the rows of
            hector_sync_cases.STATUSES step 8 holds three refusals of three kinds (-2, -3, -4): nobody is taken; step 0 holds
            only a queued scan; member 2's last callback is refused; members join and leave in mid-call.
  wide2     R = 2, both members on the 1081-beam log (both 1024-beam compaction rounds of the container kernel), maps of 2 and
            of 3 levels.
  solo      R = 1 on imu_gap, 96 beams.
  wide1     R = 1 on the 1081-beam log: what a node that was reset after shorter scans continues with.

tests/test_hector_fleet_sync_cases_oracle.py holds these claims to STATUSES on the CPU.  Pure numpy; the device API is handed
in by the caller."""
import collections

import numpy as np

import hector_sync_cases as H

f32 = np.float32
Member = collections.namedtuple("Member", "log first levels map_n")
FLEETS = {
    "ragged64": (14, [Member("non_monotone", 0, 3, 512), Member("no_lead", 2, 2, 512), Member("window_sizes", 1, 3, 384)]),
    "wide2": (6, [Member("wide", 0, 2, 512), Member("wide", 0, 3, 512)]),
    "solo": (12, [Member("imu_gap", 0, 2, 512)]),
    "wide1": (6, [Member("wide", 0, 2, 512)]),
}
CHUNKS = H.CHUNKS          # of ragged64: member 0 is non_monotone, whose runs of refusals these ends fall into
CONTINUE_AT = 7            # tests 5: the fleet for steps [0, 7), the members alone for the rest, and the other way round
INACTIVE = -9              # statuses(): the member has no callback in this step


def steps(name):
    return FLEETS[name][0]


def members(name):
    return FLEETS[name][1]


def callbacks(mb):
    return len(H.STATUSES[mb.log])


def active(name):
    """[steps, R] bool: member m has a callback in step k"""
    n, mbs = FLEETS[name]
    a = np.zeros((n, len(mbs)), bool)
    for m, mb in enumerate(mbs):
        a[mb.first:mb.first + callbacks(mb), m] = True
    return a


def statuses(name):
    """[steps, R]: the status STATUSES gives each (step, member); INACTIVE where the member has no callback"""
    n, mbs = FLEETS[name]
    s = np.full((n, len(mbs)), INACTIVE, np.int64)
    for m, mb in enumerate(mbs):
        s[mb.first:mb.first + callbacks(mb), m] = H.STATUSES[mb.log]
    return s


def span(mb, lo, hi):
    """The callbacks [a, b) of a member that fall into steps [lo, hi)."""
    return min(max(lo - mb.first, 0), callbacks(mb)), min(max(hi - mb.first, 0), callbacks(mb))


def step_arrays(name, lo=0, hi=None):
    """(ranges [n, R, beams], stamps, time_increments, imu_seen, odom_seen [n, R], active [n, R]) of steps [lo, hi): what
    HectorFleet.process_synced takes.  Rows of entries that are not active are zero (they are not read)."""
    n_steps, mbs = FLEETS[name]
    hi = n_steps if hi is None else hi
    R, n = len(mbs), hi - lo
    beams = H.case(mbs[0].log)["ranges"].shape[1]
    r = np.zeros((n, R, beams), f32)
    t, ti = np.zeros((n, R), np.float64), np.zeros((n, R), f32)
    iseen, oseen = np.zeros((n, R), np.int64), np.zeros((n, R), np.int64)
    for m, mb in enumerate(mbs):
        c = H.case(mb.log)
        a, b = span(mb, lo, hi)
        at = slice(mb.first + a - lo, mb.first + b - lo)
        r[at, m], t[at, m], ti[at, m], iseen[at, m], oseen[at, m] = H.scan_args(c, a, b)
    return r, t, ti, iseen, oseen, active(name)[lo:hi]


def spread(name, per_member, lo=0, hi=None, fill=0):
    """per_member[m]: an array with one row per callback of member m -> [n, R, ...] with the rows at their steps."""
    n_steps, mbs = FLEETS[name]
    hi = n_steps if hi is None else hi
    first = np.asarray(per_member[0])
    out = np.full((hi - lo, len(mbs)) + first.shape[1:], fill, first.dtype)
    for m, mb in enumerate(mbs):
        a, b = span(mb, lo, hi)
        out[mb.first + a - lo:mb.first + b - lo, m] = np.asarray(per_member[m])[a:b]
    return out
