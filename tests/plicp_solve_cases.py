"""Cases that hold PL-ICP's closed-form solve to the minimum of its own cost (tests/plicp_minimum.py): scan pairs whose
iterations solve with LARGE residuals, where the Lagrange multiplier is far from zero.  A polynomial that agrees with the
Lagrange condition only at lambda = 0 passes every noise-free known-motion test; it does not pass these.

A SolveCase is a plicp_cases.Case plus the poses `x_ins` from which one iteration is taken (the first guess, and for some the
restatement's x after its iterations 1, 2 and 3).  The existing scenarios are taken from plicp_cases by name and keep their
claims there; a NEW case's claim is a predicate over `old_miss`, the distance from the reference's pose of a solve whose
polynomial agrees with the Lagrange condition only at lambda = 0 (tests/test_plicp_solve_oracle.py builds that polynomial and
asserts the claim): the case is worth having because such a solve misses by more than 1e-7 on it.

Every (case, x_in) must keep these conditions, asserted by tests/test_plicp_solve_oracle.py on the CPU alone; the seeds below
were chosen so that they hold:
  * the iteration keeps >= 8 correspondences, whose normals span >= 3 directions more than 10 degrees apart,
  * the reduced 2x2 problem is far from rank-deficient: e0 / e1 >= 1e-6,
  * the minimum is unique: runner_up_gap >= 1e-6,
  * no case-level decision of the iteration is undecided, and at most 2 readings are."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

import plicp_cases as K
import plicp_minimum as M
import plicp_restatement as R

OLD_MISS = 1e-7
MIN_KEPT, MIN_DIRECTIONS, DIRECTION_DEG, MIN_GAP, MAX_UNDECIDED = 8, 3, 10.0, 1e-6, 2
MIN_CONDITIONING = 1e-6   # e0 / e1 of S: ten orders above what rounding leaves of an exactly rank-deficient scene

EXISTING = ([f"noisy_360_s0.01_{k}" for k in range(3)] + [f"noisy_360_s0.002_{k}" for k in range(3)] +
            ["identity_360", "modes_max_iterations_1", "modes_point_to_point"])
LATER_ITERATIONS = [f"noisy_360_s0.01_{k}" for k in range(3)]   # also from the restatement's x after iterations 1, 2, 3


@dataclasses.dataclass
class SolveCase:
    case: K.Case
    x_ins: tuple            # of 3-tuples
    new: bool               # built here: case.claim is a predicate over old_miss

    @property
    def name(self):
        return self.case.name


def _misses(old_miss):
    return old_miss > OLD_MISS


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []
    for name in EXISTING:
        c = K.by_name()[name]
        x_ins = [tuple(c.guess)]
        if name in LATER_ITERATIONS:
            its = K.expected(name)[2]
            x_ins += [tuple(its[k].sol) for k in range(3)]
        out.append(SolveCase(c, tuple(x_ins), False))

    def add(name, laser, ref, sens, truth, guess=(0.0, 0.0, 0.0)):
        c = K.Case(name, "solve", laser, np.asarray(ref, np.float32), np.asarray(sens, np.float32), {}, guess=tuple(guess),
                   truth=truth, claim=_misses)
        out.append(SolveCase(c, (tuple(guess),), True))

    # ---- 64 beams: few correspondences, so one noisy reading weighs much
    for sigma, seed in ((0.002, 30), (0.01, 31), (0.05, 32)):
        ref, sens, d = K.pair(K.LASER64, np.random.default_rng(seed), noise=sigma)
        add(f"solve_64_s{sigma}", K.LASER64, ref, sens, d)
    # ---- a moved object: 30 adjacent sens readings 0.3 m short, residuals that survive the adaptive cut
    ref, sens, d = K.pair(K.LASER360, np.random.default_rng(33))
    sens = sens.copy()
    sens[100:130] -= 0.3
    add("solve_moved_object", K.LASER360, ref, sens, d)
    # ---- a first guess 0.15 m / 0.08 rad off the truth: lambda is far from 0 in iteration 1
    ref, sens, d = K.pair(K.LASER360, np.random.default_rng(34))
    add("solve_far_guess", K.LASER360, ref, sens, d, guess=d + np.array([0.12, -0.09, 0.08]))
    # ---- 1081 beams, noisy
    ref, sens, d = K.pair(K.LASER1081, np.random.default_rng(35), noise=0.01)
    add("solve_1081_s0.01", K.LASER1081, ref, sens, d)
    return tuple(out)


def by_name() -> dict:
    return {c.name: c for c in cases()}


IDS = [(c.name, k) for c in cases() for k in range(len(c.x_ins))]   # every (case, index into x_ins)
NEW = [c.name for c in cases() if c.new]


def directions(nrm) -> int:
    """How many of the normals' directions lie more than DIRECTION_DEG apart from each other: the normals are unit vectors,
    their directions angles on the full circle, picked greedily in ascending angle (n and -n count as two: a wall seen from
    either side.  What this condition is there to keep away, a scene of exactly two LINES, is what `conditioning` measures)."""
    picked = []
    for t in np.sort(np.arctan2(nrm[:, 1], nrm[:, 0])):
        if all(min(abs(t - s), 2 * math.pi - abs(t - s)) > math.radians(DIRECTION_DEG) for s in picked):
            picked.append(t)
    return len(picked)


def conditioning(p, q, nrm) -> float:
    """e0 / e1 of the reduced 2x2 matrix S (the cost with t eliminated is u^T S u + h^T u).  Exactly two walls make e0 = 0 and
    the solve has no unique answer; rounding leaves e0 / e1 of the order 1e-16 x the count there."""
    e = np.linalg.eigvalsh(np.asarray(M._reduced(M._ld(p), M._ld(q), M._ld(nrm))[3], dtype=np.float64))
    return float(e[0] / e[1])


@dataclasses.dataclass
class Problem:
    it: R.Iteration
    p: np.ndarray           # the kept correspondences, in reading order: sens points (sens frame),
    q: np.ndarray           # their ref points
    nrm: np.ndarray         # and their segments' unit normals
    x: np.ndarray           # plicp_minimum's pose,
    cost: float             # its cost
    gap: float              # and its runner_up_gap


@functools.lru_cache(maxsize=None)
def problem(name: str, k: int) -> Problem:
    """The restatement's iteration of case `name` from its x_ins[k], the kept correspondences and their minimum; computed
    once and left unchanged."""
    sc = by_name()[name]
    c = sc.case
    ref, sens = c.ldp(c.ref), c.ldp(c.sens)
    it = R.iteration(c.params(), ref, sens, sc.x_ins[k])
    kept = np.flatnonzero(it.flags & 4)
    q_all, p_all = ref.points(), sens.points()
    seg = q_all[it.j2[kept]] - q_all[it.j1[kept]]
    nrm = np.stack([-seg[:, 1], seg[:, 0]], axis=1) / np.linalg.norm(seg, axis=1)[:, None]
    p, q = p_all[kept], q_all[it.j1[kept]]
    if len(kept) < 3:
        return Problem(it, p, q, nrm, np.full(3, np.nan), float("nan"), 0.0)
    x, cost, gap = M.minimum(p, q, nrm)
    return Problem(it, p, q, nrm, x, cost, gap)
