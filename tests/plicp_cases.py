"""Scenarios for lesson3's PL-ICP (csrc/plicp.hip against tools/plicp_cpu.py's sm_icp).  The world is test_plicp.py's 24 m
arena; the lasers are its 360-beam (1 deg) one and a 1081-beam (0.25 deg, -135 deg) one; relative motions stay within
+-0.25 m / +-0.12 rad.  Every scenario carries a `claim`: a predicate over (result, first iteration) saying what the scenario
is there for, asserted by tests/test_plicp_cases_oracle.py on the CPU restatement alone."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from lslam_amd import synth
from tools import plicp_cpu as P

LASER360 = synth.Laser(n_ranges=360, angle_min=-math.pi, angle_increment=math.radians(1.0), range_min=0.1, range_max=30.0)
LASER1081 = synth.Laser(n_ranges=1081, angle_min=math.radians(-135.0), angle_increment=math.radians(0.25), range_min=0.1,
                        range_max=30.0)
LASER2048 = synth.Laser(n_ranges=2048, angle_min=-math.pi, angle_increment=2.0 * math.pi / 2048, range_min=0.1, range_max=40.0)
LASER64 = synth.Laser(n_ranges=64, angle_min=-math.pi, angle_increment=2.0 * math.pi / 64, range_min=0.1, range_max=40.0)


@dataclasses.dataclass
class Case:
    name: str
    scenario: str
    laser: synth.Laser
    ref: np.ndarray                 # float32 [n]
    sens: np.ndarray                # float32 [n]
    overrides: dict                 # PlicpParams fields that differ from the defaults
    guess: tuple = (0.0, 0.0, 0.0)
    truth: np.ndarray | None = None  # the relative motion, where the scenario knows it
    claim: object = None            # (result dict, first Iteration, Case) -> bool

    def params(self) -> P.PlicpParams:
        return P.PlicpParams(**self.overrides)

    def ldp(self, ranges) -> P.Ldp:
        L = self.laser
        return P.laser_scan_to_ldp(ranges, L.angle_min, L.angle_increment, L.range_min, L.range_max)


@functools.lru_cache(maxsize=None)
def world():
    return synth.arena(size=24.0, n_axis=6, n_rot=3, seed=4)


def compose(a, d):
    ca, sa = math.cos(a[2]), math.sin(a[2])
    return np.array([a[0] + ca * d[0] - sa * d[1], a[1] + sa * d[0] + ca * d[1], a[2] + d[2]])


def pair(laser, rng, noise=0.0, dropout=0.0, motion=None, free=True):
    """Two scans of the arena a known motion apart (test_plicp.py's construction; free: both poses keep 0.6 m from every
    wall) -> (ref, sens, motion)."""
    while True:
        a = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-math.pi, math.pi)])
        d = np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(-0.12, 0.12)])
        if motion is not None:
            d = np.asarray(motion, dtype=np.float64)
        b = compose(a, d)
        if not free or (synth.point_is_free(world(), a[0], a[1]) and synth.point_is_free(world(), b[0], b[1])):
            break
    kw = dict(noise_sigma=noise, dropout=dropout, rng=rng) if (noise or dropout) else {}
    return synth.cast_scan(world(), a, laser, **kw), synth.cast_scan(world(), compose(a, d), laser, **kw), d


def _recovered(tol_xy, tol_th):
    def claim(res, it1, c):
        e = res["x"] - c.truth
        return res["valid"] == 1 and math.hypot(e[0], e[1]) < tol_xy and abs(math.remainder(e[2], 2 * math.pi)) < tol_th
    return claim


def _exit(why, iteration=1):
    return lambda res, it1, c: res["valid"] == 0 and res["iterations"] == 0 and it1.exit == why


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []

    def add(name, scenario, laser, ref, sens, overrides=None, **kw):
        out.append(Case(name, scenario, laser, np.asarray(ref, np.float32), np.asarray(sens, np.float32), overrides or {}, **kw))

    # ---- known_motion: 8 noise-free pairs per laser (the 360-beam ones are test_plicp.py's)
    for tag, laser, seed in (("360", LASER360, 0), ("1081", LASER1081, 1)):
        rng = np.random.default_rng(seed)
        for k in range(8):
            ref, sens, d = pair(laser, rng, free=(tag != "360"))
            add(f"known_motion_{tag}_{k}", "known_motion", laser, ref, sens, truth=d, claim=_recovered(1e-6, 1e-6))
    # ---- noisy: range noise and 1 % dropouts; some of them use all 10 iterations
    rng = np.random.default_rng(10)
    for tag, laser, count in (("360", LASER360, 3), ("1081", LASER1081, 1)):
        for sigma in (0.01, 0.002):
            for k in range(count):
                ref, sens, d = pair(laser, rng, noise=sigma, dropout=0.01)
                add(f"noisy_{tag}_s{sigma}_{k}", "noisy", laser, ref, sens, truth=d,
                    claim=lambda res, it1, c: res["valid"] == 1 and res["nvalid"] > 150)  # (not all of them converge in 10)
    # ---- identity: no motion, two independent noisy scans from one place (exact duplicates tie every distance at zero, which
    #      the rank rule decides and numpy's sort does not: tests/test_plicp_gpu.py takes them by their properties)
    rng = np.random.default_rng(11)
    ref, sens, d = pair(LASER360, rng, noise=0.002, motion=(0.0, 0.0, 0.0))
    add("identity_360", "identity", LASER360, ref, sens, truth=d, claim=_recovered(0.01, 0.01))
    # ---- guessed: a first guess near the truth, and one on the other side of it
    rng = np.random.default_rng(12)
    for k, off in enumerate(((0.03, -0.02, 0.01), (-0.05, 0.04, -0.02))):
        ref, sens, d = pair(LASER360, rng)
        add(f"guessed_{k}", "guessed", LASER360, ref, sens, guess=tuple(d + np.array(off)), truth=d, claim=_recovered(1e-6, 1e-6))
    # ---- beam_counts: V valid readings of 2048, the same ones on both sides (the wave and block strides, and the limit)
    rng = np.random.default_rng(13)
    ref, sens, d = pair(LASER2048, rng, motion=(0.02, -0.015, 0.004))  # (less than the spacing of the points on a wall)
    for v in (2, 3, 4, 63, 64, 65, 255, 256, 257, 2048):
        mask = np.ones(2048, bool)
        if v < 2048:
            mask[:] = False                   # two blocks a quarter turn apart: walls of two directions, a well-posed solve
            mask[900:900 + (v + 1) // 2] = True
            mask[1412:1412 + v // 2] = True
        claim = (lambda vv: lambda res, it1, c: int((it1.flags & 1).sum()) == vv and (it1.exit == "few_valid") == (vv < 3))(v)
        add(f"beam_counts_{v}", "beam_counts", LASER2048, np.where(mask, ref, np.inf), np.where(mask, sens, np.inf), claim=claim)
    # ---- holes: the ref scan loses readings so that j2 must take the other side, or has no side to take; j1 at both ends
    rng = np.random.default_rng(14)
    ref, sens, d = pair(LASER360, rng)
    third = ref.copy()
    third[2::3] = np.inf                      # valid, valid, lost: every valid reading has exactly one valid neighbour
    def one_sided(res, it1, c):
        v = (it1.flags & 1) == 1
        up, down = it1.j2[v] == it1.j1[v] + 1, it1.j2[v] == it1.j1[v] - 1
        return res["valid"] == 1 and up.sum() > 20 and down.sum() > 20 and np.all(up | down | (it1.j2[v] == -1))
    add("holes_one_side", "holes", LASER360, third, sens, truth=d, claim=one_sided)
    lone = ref.copy()
    lone[100:200:2] = np.inf                  # every other reading of a stretch lost: no valid neighbour on either side
    def no_side(res, it1, c):
        v = (it1.flags & 1) == 1
        return res["valid"] == 1 and ((it1.j2[v] == -1) & (it1.j1[v] >= 0)).sum() > 10 and not np.any(it1.flags[it1.j2 == -1] & 2)
    add("holes_no_side", "holes", LASER360, lone, sens, truth=d, claim=no_side)
    def both_ends(res, it1, c):
        return res["valid"] == 1 and np.any(it1.j1 == 0) and np.any(it1.j1 == c.laser.n_ranges - 1)
    add("holes_ends", "holes", LASER360, ref, sens, truth=d, claim=both_ends)
    # ---- far: part of the correspondences lie beyond max_correspondence_dist and are not accepted
    rng = np.random.default_rng(15)
    ref, sens, d = pair(LASER360, rng, motion=(0.2, 0.1, 0.05))
    def some_far(res, it1, c):
        v = (it1.flags & 1) == 1
        refused = v & ((it1.flags & 2) == 0) & (it1.j2 >= 0)
        return res["iterations"] >= 1 and refused.sum() > 20 and (it1.flags & 2).astype(bool).sum() > 20
    add("far", "far", LASER360, ref, sens, {"max_correspondence_dist": 0.15}, truth=d, claim=some_far)
    # ---- rejected: the solution lies beyond the allowed correction: valid = 0, x still reported
    def refused_with_x(res, it1, c):
        e = res["x"] - c.truth
        return res["valid"] == 0 and res["iterations"] >= 1 and res["nvalid"] >= 3 and math.hypot(e[0], e[1]) < 1e-6
    ref, sens, d = pair(LASER360, rng, motion=(0.2, 0.1, 0.02))
    add("rejected_linear", "rejected", LASER360, ref, sens, {"max_linear_correction": 0.1}, truth=d, claim=refused_with_x)
    ref, sens, d = pair(LASER360, rng, motion=(0.02, 0.01, 0.1))
    add("rejected_angular", "rejected", LASER360, ref, sens, {"max_angular_correction_deg": 2.0}, truth=d, claim=refused_with_x)
    # ---- too_few: fewer than 3 survivors at each of the three exits
    ref, sens, d = pair(LASER360, rng, motion=(0.2, 0.1, 0.05))
    add("too_few_corr", "too_few", LASER360, ref, sens, {"max_correspondence_dist": 1e-4}, claim=_exit("few_corr"))
    add("too_few_kept", "too_few", LASER360, ref, sens, {"outliers_adaptive_order": 0.0, "outliers_adaptive_mult": 0.0},
        claim=_exit("few_kept"))
    # a singular solve: with doubles kept, four sens readings all land on ONE ref segment (two adjacent ref readings; the
    # third valid one stands alone and can take no segment): one normal up to its sign, so |det| is rounding noise
    k = 40
    ref3 = np.full(360, np.inf, np.float32)
    ref3[[k, k + 1, k + 180]] = ref[[k, k + 1, k + 180]]
    sens4 = np.full(360, np.inf, np.float32)
    sens4[k - 1:k + 3] = ref[k - 1:k + 3]
    add("too_few_singular", "too_few", LASER360, ref3, sens4, {"outliers_remove_doubles": 0}, claim=_exit("singular"))
    # ---- modes
    rng = np.random.default_rng(16)
    ref, sens, d = pair(LASER360, rng)
    add("modes_point_to_point", "modes", LASER360, ref, sens, {"use_point_to_line_distance": 0}, truth=d,
        claim=lambda res, it1, c: res["valid"] == 1)
    add("modes_keep_doubles", "modes", LASER360, ref, sens, {"outliers_remove_doubles": 0}, truth=d, claim=_recovered(1e-6, 1e-6))
    for m in (1, 3):
        add(f"modes_max_iterations_{m}", "modes", LASER360, ref, sens, {"max_iterations": m}, truth=d,
            claim=(lambda mm: lambda res, it1, c: res["iterations"] == mm)(m))
    # ---- empty: nothing valid on one side or the other
    for tag, fill in (("inf", np.inf), ("nan", np.nan)):
        blank = np.full(360, fill, np.float32)
        add(f"empty_ref_{tag}", "empty", LASER360, blank, sens, claim=_exit("few_valid"))
        add(f"empty_sens_{tag}", "empty", LASER360, ref, blank, claim=_exit("few_valid"))
    return tuple(out)


def by_name() -> dict:
    return {c.name: c for c in cases()}


NAMES = [c.name for c in cases()]
SCENARIOS = sorted({c.scenario for c in cases()})


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(sm_icp's result, the restatement's result, its iterations, near_epsilon) of a case, computed once."""
    import plicp_restatement as R

    c = by_name()[name]
    ref, sens = c.ldp(c.ref), c.ldp(c.sens)
    direct = P.sm_icp(c.params(), ref, sens, c.guess)
    res, its, near = R.iterate(c.params(), ref, sens, c.guess)
    return direct, res, its, near
