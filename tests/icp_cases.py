"""Scenarios for lesson2's point-to-point ICP (csrc/icp.hip against tools/icp_cpu.py's icp).  The world is plicp_cases.py's
24 m arena and the scan pairs are built the way plicp_cases.pair builds them.  Every case is a pair of CLOUDS (n x 3 float32,
with their valid bytes): a ranges case keeps its scans and laser too, and its clouds are the helper's conversion of them, so
that the match is compared on identical inputs and the conversion on its own.  Every case carries a `claim`: a predicate over
the helper's result saying what the case is there for, asserted by tests/test_icp_cases_oracle.py on the helper alone."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

import plicp_cases as PK
from lslam_amd import synth
from tools import icp_cpu as I

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1081, 2048)   # 2049 is refused
UNDECIDED_REL = 1e-9     # a target point with other coordinates within 1e-9 (1 + d2) of the best
NEAR_ABS = 1e-15         # | |mse - prev| - absolute_mse | below this: the iteration count is near
RIGID_TRUTH = (0.003, -0.002, 0.002)


def laser_of(n: int) -> synth.Laser:
    if n == 360:
        return PK.LASER360
    if n == 1081:
        return PK.LASER1081
    return synth.Laser(n_ranges=n, angle_min=-math.pi, angle_increment=2.0 * math.pi / n, range_min=0.1, range_max=40.0)


@dataclasses.dataclass
class Case:
    name: str
    scenario: str
    src: np.ndarray                  # float32 [n, 3]
    tgt: np.ndarray
    src_valid: np.ndarray | None     # uint8 [n]
    tgt_valid: np.ndarray | None
    overrides: dict                  # IcpParams fields that differ from the defaults
    guess: tuple = (0.0, 0.0, 0.0)
    truth: np.ndarray | None = None  # source -> target, where the scenario knows it
    claim: object = None             # (result dict, Case) -> bool
    laser: synth.Laser | None = None  # ranges cases: the scans the clouds were converted from
    src_ranges: np.ndarray | None = None
    tgt_ranges: np.ndarray | None = None

    def params(self) -> I.IcpParams:
        return I.IcpParams(**self.overrides)

    @property
    def n(self) -> int:
        return len(self.src)


def cloud(laser, ranges, invalid_as_nan=0):
    return I.scan_to_cloud(ranges, laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max, invalid_as_nan)


def inverse(d):
    """The pose of the first scan in the second one's frame: what aligns the first cloud (source) to the second (target)."""
    c, s = math.cos(d[2]), math.sin(d[2])
    return np.array([-(c * d[0] + s * d[1]), -(-s * d[0] + c * d[1]), -d[2]])


def _near(tol_xy, tol_th):
    def claim(res, c):
        e = res["x"] - c.truth
        return res["converged"] == 1 and math.hypot(e[0], e[1]) < tol_xy and abs(math.remainder(e[2], 2 * math.pi)) < tol_th
    return claim


def _drop(r, rng, rate):
    return np.where(rng.random(r.shape) < rate, np.float32(np.inf), r).astype(np.float32)


def window_scan(laser) -> np.ndarray:
    """Readings on, and one float32 ulp either side of, range_min and range_max; +-inf, NaN and negative readings."""
    lo, hi = np.float32(laser.range_min), np.float32(laser.range_max)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    special = [lo, np.nextafter(lo, down), np.nextafter(lo, up), hi, np.nextafter(hi, down), np.nextafter(hi, up), np.inf, -np.inf,
               np.nan, -1.0, -0.0, 0.0, np.float32(-5.0)]
    r = np.full(laser.n_ranges, 5.0, np.float32)
    r[3:3 + len(special)] = np.array(special, np.float32)
    return r


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []

    def add_clouds(name, scenario, src, tgt, sv=None, tv=None, overrides=None, **kw):
        src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
        out.append(Case(name, scenario, src, tgt, sv, tv, overrides or {}, **kw))

    def add_ranges(name, scenario, laser, a, b, overrides=None, **kw):
        (sx, sv), (tx, tv) = cloud(laser, a), cloud(laser, b)
        out.append(Case(name, scenario, sx, tx, sv, tv, overrides or {}, laser=laser, src_ranges=np.asarray(a, np.float32),
                        tgt_ranges=np.asarray(b, np.float32), **kw))

    # ---- sizes: the wave and block strides, the tile widths of the search (1, 2 and 4 points a lane) and the limit
    rng = np.random.default_rng(30)
    for n in SIZES:
        a, b, d = PK.pair(laser_of(n), rng, motion=(0.02, -0.015, 0.004))
        few = n < 3
        add_ranges(f"size_{n}", "sizes", laser_of(n), a, b, truth=inverse(d),
                   claim=(lambda f: lambda res, c: (res["state"] == I.STATE_FEW and res["iterations"] == 0) if f
                          else res["converged"] == 1 and res["ncorr"] == c.n)(few))
    # ---- scan pairs at 64 / 360 / 1081 beams: no origin points, origin points in one cloud, in both in different numbers
    rng = np.random.default_rng(31)
    for n in (64, 360, 1081):
        a, b, d = PK.pair(laser_of(n), rng)
        for tag, ra, rb in (("clean", 0.0, 0.0), ("drop_target", 0.0, 0.05), ("drop_both", 0.03, 0.08)):
            sa, sb = _drop(a, rng, ra), _drop(b, rng, rb)
            want = (bool(ra), bool(rb))
            add_ranges(f"pair_{n}_{tag}", "pairs", laser_of(n), sa, sb, truth=inverse(d),
                       claim=(lambda w: lambda res, c: res["converged"] == 1 and res["ncorr"] == c.n and
                              (bool((c.src_valid == 0).any()), bool((c.tgt_valid == 0).any())) == w and
                              (w == (False, False) or int((c.src_valid == 0).sum()) != int((c.tgt_valid == 0).sum())))(want))
    # ---- identical / all_invalid: 1 iteration, state 2, x exactly zero (all_invalid: through exact ties on every distance)
    rng = np.random.default_rng(32)
    a, _, _ = PK.pair(PK.LASER360, rng)
    a = _drop(a, rng, 0.02)
    exact_zero = lambda res, c: (res["iterations"], res["state"], res["converged"]) == (1, I.STATE_TRANSFORM, 1) and \
        np.all(res["x"] == 0.0) and res["mse"] == 0.0 and res["fitness"] == 0.0
    add_ranges("identical", "identical", PK.LASER360, a, a, truth=np.zeros(3), claim=exact_zero)
    blank = np.full(360, np.inf, np.float32)
    add_ranges("all_invalid", "all_invalid", PK.LASER360, blank, blank, truth=np.zeros(3), claim=exact_zero)
    # ---- rigid_copy: a cloud and its float32-rounded rigid image
    a, _, _ = PK.pair(PK.LASER360, rng)
    p, _ = cloud(PK.LASER360, a)
    c0, s0 = math.cos(RIGID_TRUTH[2]), math.sin(RIGID_TRUTH[2])
    q = p.copy()
    q[:, 0] = (c0 * p[:, 0].astype(np.float64) - s0 * p[:, 1].astype(np.float64) + RIGID_TRUTH[0]).astype(np.float32)
    q[:, 1] = (s0 * p[:, 0].astype(np.float64) + c0 * p[:, 1].astype(np.float64) + RIGID_TRUTH[1]).astype(np.float32)
    add_clouds("rigid_copy", "rigid_copy", p, q, truth=np.array(RIGID_TRUTH), claim=_near(1e-6, 1e-6))
    # ---- duplicates: exact duplicate target points that are not the origin; the lowest index of each group is the one taken
    a, b, d = PK.pair(PK.LASER360, rng)
    (p, _), (q, _) = cloud(PK.LASER360, a), cloud(PK.LASER360, b)
    q = q.copy()
    q[11] = q[12] = q[10]
    q[201] = q[200]
    def lowest_of_group(res, c):
        first = res["trace"][0].corr
        return res["converged"] == 1 and (np.any(first == 10) or np.any(first == 200)) and not np.any(np.isin(first, (11, 12, 201)))
    add_clouds("duplicates", "duplicates", p, q, truth=inverse(d), claim=lowest_of_group)
    # ---- few: a max_correspondence_distance that leaves 2, and exactly 3, correspondences in the first search
    a, b, d = PK.pair(PK.LASER360, rng, motion=(0.2, 0.1, 0.05))
    (p, _), (q, _) = cloud(PK.LASER360, a), cloud(PK.LASER360, b)
    first = np.sort(np.sqrt(I.one_iteration(p, q).d2))
    add_clouds("few_2", "few", p, q, overrides={"max_correspondence_distance": float(0.5 * (first[1] + first[2]))}, truth=inverse(d),
               claim=lambda res, c: (res["converged"], res["iterations"], res["ncorr"], res["state"]) == (0, 0, 2, I.STATE_FEW)
               and np.all(res["x"] == 0.0))
    add_clouds("few_3", "few", p, q, overrides={"max_correspondence_distance": float(0.5 * (first[2] + first[3]))}, truth=inverse(d),
               claim=lambda res, c: res["trace"][0].ncorr == 3 and res["iterations"] >= 1)
    # ---- gate / tie: exactly representable geometry.  An L of 128 target points a unit apart; the source is the target moved
    #      by (0.25, 0): every best d2 is exactly 0.0625 = 0.25^2, so the gate decides at equality.  In `tie_midway` one source
    #      point lies exactly midway between two target points: the lower index takes it.
    k = np.arange(64, dtype=np.float32)
    L = np.zeros((128, 3), np.float32)
    L[:64, 0] = k + 1.0
    L[64:, 1] = k + 1.0
    moved = L.copy()
    moved[:, 0] += np.float32(0.25)
    add_clouds("gate_exact", "gate", moved, L, overrides={"max_correspondence_distance": 0.25}, truth=np.array([-0.25, 0.0, 0.0]),
               claim=lambda res, c: res["trace"][0].ncorr == 128 and np.all(res["trace"][0].d2 == 0.0625))
    mid = moved.copy()
    mid[5, 0] = np.float32(6.5)      # between target 5 (x = 6) and target 6 (x = 7)
    add_clouds("tie_midway", "gate", mid, L, truth=np.array([-0.25, 0.0, 0.0]),
               claim=lambda res, c: res["trace"][0].corr[5] == 5 and res["trace"][0].d2[5] == 0.25 and res["trace"][0].d2_other[5] == 0.25)
    # ---- first_guess
    a, b, d = PK.pair(PK.LASER360, rng)
    add_ranges("first_guess", "first_guess", PK.LASER360, a, b, guess=tuple(inverse(d) + np.array((0.03, -0.02, 0.01))),
               truth=inverse(d), claim=lambda res, c: res["converged"] == 1 and res["trace"][0].mse < 0.01)
    # ---- skip_invalid: 0 against 1 on one pair with dropouts, the valid mask through the clouds form
    a, b, d = PK.pair(PK.LASER360, rng)
    a, b = _drop(a, rng, 0.05), _drop(b, rng, 0.08)
    (p, pv), (q, qv) = cloud(PK.LASER360, a), cloud(PK.LASER360, b)
    add_clouds("skip_invalid_0", "skip_invalid", p, q, pv, qv, truth=inverse(d),
               claim=lambda res, c: res["trace"][0].ncorr == c.n)
    add_clouds("skip_invalid_1", "skip_invalid", p, q, pv, qv, overrides={"skip_invalid": 1}, truth=inverse(d),
               claim=lambda res, c: res["trace"][0].ncorr == int(c.src_valid.sum()) < c.n and
               np.all(res["trace"][0].corr[c.src_valid == 0] == -1) and not np.any(np.isin(res["trace"][0].corr, np.flatnonzero(c.tgt_valid == 0))))
    # ---- the stop rules, each reached by its parameter
    a, b, d = PK.pair(PK.LASER360, rng)
    state_is = lambda s: (lambda res, c: res["state"] == s and res["converged"] == 1 and 1 < res["iterations"] < 10)
    add_ranges("stop_transform", "stop_rules", PK.LASER360, a, b, {"transformation_epsilon": 1e-5}, truth=inverse(d),
               claim=state_is(I.STATE_TRANSFORM))
    add_ranges("stop_abs_mse", "stop_rules", PK.LASER360, a, b, {"absolute_mse": 1e-4}, truth=inverse(d), claim=state_is(I.STATE_ABS_MSE))
    add_ranges("stop_rel_mse", "stop_rules", PK.LASER360, a, b, {"absolute_mse": 0.0, "euclidean_fitness_epsilon": 0.2},
               truth=inverse(d), claim=state_is(I.STATE_REL_MSE))
    add_ranges("stop_iterations", "stop_rules", PK.LASER360, a, b, {"max_iterations": 2}, truth=inverse(d),
               claim=lambda res, c: (res["state"], res["iterations"], res["converged"]) == (I.STATE_ITERATIONS, 2, 1))
    # ---- window: the ends of (range_min, range_max) and the readings that are no ranges, against an ordinary scan
    w = window_scan(PK.LASER64)
    a, _, _ = PK.pair(PK.LASER64, rng)
    def window(res, c):
        v = c.src_valid
        return list(v[3:16]) == [0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0] and v.sum() == 64 - 11 and np.all(c.src[v == 0] == 0.0)
    add_ranges("window", "window", PK.LASER64, w, a, claim=window)
    return tuple(out)


def by_name() -> dict:
    return {c.name: c for c in cases()}


NAMES = [c.name for c in cases()]
SCENARIOS = sorted({c.scenario for c in cases()})
RANGES_NAMES = [c.name for c in cases() if c.laser is not None]


@functools.lru_cache(maxsize=None)
def expected(name: str, mistake: str | None = None):
    """The helper's result (with its trace) of a case, computed once and left unchanged."""
    c = by_name()[name]
    src, tgt, sv, tv = c.src, c.tgt, c.src_valid, c.tgt_valid
    if mistake == "window_inclusive" and c.laser is not None:
        L = c.laser
        (src, sv), (tgt, tv) = (I.scan_to_cloud(r, L.angle_min, L.angle_increment, L.range_min, L.range_max, 0, mistake)
                                for r in (c.src_ranges, c.tgt_ranges))
    return I.icp(src, tgt, c.params(), c.guess, sv, tv, mistake=mistake)


@functools.lru_cache(maxsize=None)
def margins(name: str):
    """(undecided: bool [iterations, n], near: bool) of a case's expected trace."""
    res = expected(name)
    c = by_name()[name]
    und = np.zeros((len(res["trace"]), c.n), bool)
    near = False
    for k, it in enumerate(res["trace"]):
        with np.errstate(invalid="ignore"):
            und[k] = np.isfinite(it.d2) & (it.d2_other - it.d2 <= UNDECIDED_REL * (1.0 + it.d2))
        near = near or it.mse_gap <= NEAR_ABS
    return und, near


def decided(name: str) -> bool:
    und, near = margins(name)
    return not und.any() and not near
