"""Fleets for lslam_hector_fleet_* (api.HectorFleet): R streamed processors, each on its own map, stepped in lockstep.  Every
fleet is made of the scenarios of tests/hector_stream_cases.py, and the yardstick is always the member run ALONE through
lslam_hector_process_many[_points] over its own active scans -- a path tests/test_hector_stream_gpu.py holds to the
reference's processor.

  (a) hetero     R = 3, container form: edges(3) (256^2, 3 levels, <= 90 points, the empty scan and the 63 / 64 / 65 / 1-point
                 scans), edges(1) (one level) and the first 12 scans of chain60 (1024^2, 3 levels, a 1081-beam laser); 12 steps
  (b) rolled     R members on edges(3), ranges form: member r streams the scenario's scans rolled by r, so the members differ
  (c) mapping    R = 3 on mapping25, hints + map_without_matching (the host-trig path), member r starting r scans in
  (d) ragged     R = 5 on edges(3) in two calls of 6 steps under RAGGED_MASK: a step nobody takes, a member that sits a whole
                 call out, members with different scan rates

Pure numpy; tests/test_hector_fleet_cases.py checks each fleet's preconditions without a GPU and
tests/test_hector_fleet_gpu.py runs them."""
import functools
from typing import NamedTuple

import numpy as np

import hector_stream_cases as S

f32 = np.float32

# the matcher's form follows LSLAM_GN_THREADS (at map creation) and the capacity of the CALL: the register form holds up to
# 5 / 3 / 2 points per thread at 256 / 512 / 1024 threads, the staged form beyond (csrc/logodds_map.hip: gn_form_of)
REG_LIMIT = {256: 1280, 512: 1536, 1024: 2048}
LDS_LIMIT = 7168  # points whose coordinates fit the staged form's 56 KiB of LDS


def form_of(threads, capacity):
    if capacity <= REG_LIMIT[threads]:
        return "reg%d" % threads
    return "fast-lds" if capacity <= LDS_LIMIT else "fast-mem"


class Member(NamedTuple):
    sc: S.Scenario        # map geometry, laser and thresholds
    containers: list      # [n_steps] of (n, 2) float32, None where the member sits the step out
    ranges: object        # [n_steps, n_readings] float32, or None
    hints: object         # [n_steps, 3] float32, or None: chained
    no_match: bool


class Fleet(NamedTuple):
    members: list         # [R] of Member
    active: np.ndarray    # [n_steps, R] bool
    calls: list           # [(first step, one past the last step)] the scenario is streamed in

    @property
    def n_steps(self):
        return len(self.active)

    def capacity(self, lo, hi):
        """Points per scan a container-form fleet call over steps [lo, hi) is sized for: its longest container."""
        return max(len(m.containers[k]) for m in self.members for k in range(lo, hi) if m.containers[k] is not None)

    def solo_capacity(self, r, lo, hi):
        """... and the member's own call over its active scans of those steps (None: it has none)."""
        n = [len(self.members[r].containers[k]) for k in range(lo, hi) if self.active[k, r]]
        return max(n) if n else None


def _all_active(n_steps, R):
    return np.ones((n_steps, R), bool)


@functools.lru_cache(maxsize=None)
def hetero():
    e3, e1, c = S.edges(3), S.edges(1), S.chain60()
    members = [Member(e3, list(e3.containers), None, None, False), Member(e1, list(e1.containers), None, None, False),
               Member(c, list(c.containers[:12]), None, None, False)]
    return Fleet(members, _all_active(12, 3), [(0, 12)])


@functools.lru_cache(maxsize=None)
def rolled(R):
    e3 = S.edges(3)
    n = len(e3.containers)
    members = []
    for r in range(R):
        order = [(k + r) % n for k in range(n)]
        members.append(Member(e3, [e3.containers[k] for k in order], e3.ranges[order], None, False))
    return Fleet(members, _all_active(n, R), [(0, n)])


@functools.lru_cache(maxsize=None)
def mapping():
    sc = S.mapping25()
    R = 3
    n = len(sc.containers) - (R - 1)
    members = [Member(sc, list(sc.containers[r:r + n]), None, sc.hints[r:r + n], True) for r in range(R)]
    return Fleet(members, _all_active(n, R), [(0, n)])


# [step, member]; step 3 is taken by nobody; member 3 sits the whole second call out; member 1 scans at half rate; member 4
# joins late; member 2 leaves early
RAGGED_MASK = np.array([
    [1, 1, 1, 1, 0],
    [1, 0, 1, 1, 0],
    [1, 1, 1, 0, 1],
    [0, 0, 0, 0, 0],
    [1, 1, 1, 1, 1],
    [1, 0, 1, 1, 1],
    [1, 1, 1, 0, 1],
    [1, 0, 1, 0, 1],
    [1, 1, 0, 0, 1],
    [1, 0, 0, 0, 1],
    [1, 1, 0, 0, 1],
    [1, 0, 0, 0, 1],
], bool)
RAGGED_CALLS = [(0, 6), (6, 12)]
RAGGED_EMPTY_STEP = 3
RAGGED_IDLE = (3, 1)  # (member, index of the call it sits out)


@functools.lru_cache(maxsize=None)
def ragged():
    """Member r takes the scans of edges(3) rolled by r, one per ACTIVE step: a member's log has no holes, the steps have."""
    e3 = S.edges(3)
    n = len(e3.containers)
    members = []
    for r in range(RAGGED_MASK.shape[1]):
        conts, ranges, j = [], np.full((len(RAGGED_MASK), e3.ranges.shape[1]), np.nan, f32), 0
        for k in range(len(RAGGED_MASK)):
            if RAGGED_MASK[k, r]:
                conts.append(e3.containers[(j + r) % n])
                ranges[k] = e3.ranges[(j + r) % n]
                j += 1
            else:
                conts.append(None)
        members.append(Member(e3, conts, ranges, None, False))
    return Fleet(members, RAGGED_MASK.copy(), list(RAGGED_CALLS))
