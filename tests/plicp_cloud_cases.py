"""Scenarios for the cloud forms of lesson3's PL-ICP (csrc/plicp.hip's k_plicp_match_clouds / k_plicp_debug_clouds against
tools/plicp_cpu.py's sm_icp on cloud_to_ldp).  Every scenario of tests/plicp_cases.py is carried over to a cloud pair -- x =
float32(r cos theta), y = float32(r sin theta) computed in float64 and then rounded, the valid byte by the node's rule, an
invalid reading written as (0, 0, 0) -- and scenarios that only a cloud can pose are added.  Every scenario carries a `claim`
over (result, first iteration, case), asserted by tests/test_plicp_cloud_cases_oracle.py on the CPU restatement alone.

RECOVERY_BOUND.  float32 points cost accuracy (half an ulp of a 10 m coordinate is 4.8e-7 m), so the 1e-6 m / 1e-6 rad to which
the ranges form recovers a known motion need not hold.  Measured on the CPU (sm_icp on the carried-over clouds that know their
motion and claim to recover it: known_motion, guessed, rejected, modes_keep_doubles), the worst error is
WORST_MEASURED = 6.5e-8 (6.48e-8, on r_known_motion_1081_5; m or rad, whichever is larger;
tests/test_plicp_cloud_cases_oracle.py prints it and holds it); allowed is 2 x that, 1.3e-7 -- the 1e-6 still holds."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

import plicp_cases as K
from tools import plicp_cpu as P

WORST_MEASURED = 6.5e-8
RECOVERY_BOUND = 2 * WORST_MEASURED


def ranges_to_cloud(ranges, laser):
    """-> (xyz float32 [n, 3], valid uint8 [n]) of one scan, or of a stack of scans."""
    r = np.asarray(ranges, dtype=np.float64)
    theta = laser.angle_min + np.arange(r.shape[-1], dtype=np.float64) * laser.angle_increment
    with np.errstate(invalid="ignore"):
        ok = (r > laser.range_min) & (r < laser.range_max)
    rr = np.where(ok, r, 0.0)
    xyz = np.zeros(r.shape + (3,), np.float32)
    xyz[..., 0] = (rr * np.cos(theta)).astype(np.float32)
    xyz[..., 1] = (rr * np.sin(theta)).astype(np.float32)
    return xyz, ok.astype(np.uint8)


@dataclasses.dataclass
class CloudCase:
    name: str
    scenario: str
    ref_xyz: np.ndarray                 # float32 [n, 3]
    sens_xyz: np.ndarray
    ref_valid: np.ndarray | None        # uint8 [n] or None = every point
    sens_valid: np.ndarray | None
    overrides: dict
    guess: tuple = (0.0, 0.0, 0.0)
    truth: np.ndarray | None = None
    claim: object = None                # (result dict, first Iteration, CloudCase) -> bool
    laser: object = None                # the carried-over case's laser (its claims read n_ranges)
    same_as: str | None = None          # the case whose result this one's must equal exactly

    def params(self) -> P.PlicpParams:
        return P.PlicpParams(**self.overrides)

    def ldps(self):
        return P.cloud_to_ldp(self.ref_xyz, self.ref_valid), P.cloud_to_ldp(self.sens_xyz, self.sens_valid)


def _recovered(tol):
    def claim(res, it1, c):
        e = res["x"] - c.truth
        return res["valid"] == 1 and math.hypot(e[0], e[1]) < tol and abs(math.remainder(e[2], 2 * math.pi)) < tol
    return claim


def _refused_with_x(res, it1, c):
    e = res["x"] - c.truth
    return res["valid"] == 0 and res["iterations"] >= 1 and res["nvalid"] >= 3 and math.hypot(e[0], e[1]) < RECOVERY_BOUND


# the carried-over claims that hold a known motion to the ranges form's 1e-6: here to the bound measured on clouds
RECOVERING = ("known_motion", "guessed", "rejected")


def recovering(name: str) -> bool:
    return name.startswith("r_") and (K.by_name()[name[2:]].scenario in RECOVERING or name == "r_modes_keep_doubles")


def _participants(res, it1, c):
    return int((it1.flags & 1).sum())


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []

    def add(name, scenario, ref, sens, rv, sv, overrides=None, **kw):
        out.append(CloudCase(name, scenario, np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(sens, np.float32),
                             None if rv is None else np.ascontiguousarray(rv, np.uint8),
                             None if sv is None else np.ascontiguousarray(sv, np.uint8), overrides or {}, **kw))

    # ---- every ranges scenario as a cloud pair
    for c in K.cases():
        (rx, rv), (sx, sv) = ranges_to_cloud(c.ref, c.laser), ranges_to_cloud(c.sens, c.laser)
        claim = c.claim
        if c.scenario in ("known_motion", "guessed") or c.name == "modes_keep_doubles":
            claim = _recovered(RECOVERY_BOUND)
        elif c.scenario == "rejected":
            claim = _refused_with_x
        add("r_" + c.name, c.scenario, rx, sx, rv, sv, dict(c.overrides), guess=c.guess, truth=c.truth, claim=claim, laser=c.laser)

    base = K.by_name()["known_motion_360_1"]
    (bx, bv), (sx, sv) = ranges_to_cloud(base.ref, base.laser), ranges_to_cloud(base.sens, base.laser)
    assert bv.all() and sv.all()
    d = base.truth
    # ---- valid NULL against all-ones bytes
    add("valid_ones", "valid_null", bx, sx, bv, sv, truth=d, claim=_recovered(RECOVERY_BOUND))
    add("valid_null", "valid_null", bx, sx, None, None, truth=d, claim=_recovered(RECOVERY_BOUND), same_as="valid_ones")
    add("valid_null_ref_only", "valid_null", bx, sx, None, sv, truth=d, claim=_recovered(RECOVERY_BOUND), same_as="valid_ones")
    # ---- not finite under valid = 1: excluded, exactly as if the byte said so
    bad = {7: (np.nan, 1.0), 100: (1.0, np.nan), 255: (np.inf, 1.0), 256: (1.0, -np.inf), 359: (np.nan, np.nan)}
    nfx, nfs, cut = bx.copy(), sx.copy(), bv.copy()
    for i, (x, y) in bad.items():
        nfx[i, :2] = (x, y)
        nfs[i, :2] = (y, x)
        cut[i] = 0
    where = np.array(sorted(bad))
    add("nonfinite_masked", "nonfinite", bx, sx, cut, cut, truth=d, claim=lambda res, it1, c: res["valid"] == 1)
    add("nonfinite", "nonfinite", nfx, nfs, bv, sv, truth=d, same_as="nonfinite_masked",
        claim=lambda res, it1, c: res["valid"] == 1 and not np.any(it1.flags[where] & 1) and _participants(res, it1, c) == 355)
    add("nonfinite_no_bytes", "nonfinite", nfx, nfs, None, None, truth=d, same_as="nonfinite_masked",
        claim=lambda res, it1, c: not np.any(it1.flags[where] & 1))
    # ---- NaN z is never read
    zx, zs = bx.copy(), sx.copy()
    zx[::3, 2] = np.nan
    zs[1::2, 2] = np.nan
    zs[5, 2] = np.inf
    add("nan_z", "nan_z", zx, zs, bv, sv, truth=d, same_as="valid_ones", claim=lambda res, it1, c: _participants(res, it1, c) == 360)
    # ---- a point at the origin with valid = 1 takes part (no range window)
    ox, os_ = bx.copy(), sx.copy()
    ox[50] = 0.0
    os_[50] = 0.0
    add("origin_point", "origin", ox, os_, bv, sv, truth=d,
        claim=lambda res, it1, c: bool(it1.flags[50] & 1) and it1.j1[50] == 50 and res["valid"] == 1)
    # ---- 0, 1, 2 and 3 participating points on either side: the `< 3` exit is taken with 0, 1, 2 and passed with 3.  With three
    #      sens points an iteration would go on to solve from three correspondences, which has no unique answer (lslam_gpu.h, rule
    #      4 of the PL-ICP section: all roots cost zero), so nothing could be held to it; the 3-point cases therefore run with a
    #      correspondence limit of 0.1 mm and stop at the NEXT exit, "few_corr", which is as decided as the first.
    for side in ("ref", "sens"):
        for v in (0, 1, 2, 3):
            m = np.zeros(360, np.uint8)
            m[[40, 41, 220][:v]] = 1
            rv_, sv_ = (m, sv) if side == "ref" else (bv, m)
            claim = (lambda vv, ss: lambda res, it1, c: it1.exit == ("few_valid" if vv < 3 else "few_corr") and
                     (ss != "sens" or _participants(res, it1, c) == vv))(v, side)
            add(f"few_{side}_{v}", "few_points", bx, sx, rv_, sv_, {"max_correspondence_dist": 1e-4} if v == 3 else None, claim=claim)
    # ---- 255 / 256 / 257 / 2048 points with holes across the 256-thread tiles
    big = K.by_name()["beam_counts_2048"]
    (gx, gv), (hx, hv) = ranges_to_cloud(big.ref, big.laser), ranges_to_cloud(big.sens, big.laser)
    for n in (255, 256, 257, 2048):
        # a quarter turn of a scan is one wall: spread the n points over the whole turn so that the solve is well posed
        pick = (np.arange(n) * 2048) // n
        rv_, sv_ = gv[pick].copy(), hv[pick].copy()
        for lo, hi in ((60, 67), (126, 130), (190, 194), (250, 262), (509, 516), (1020, 1030), (1790, 1800), (2040, 2047)):
            rv_[lo:hi] = 0                      # (slices past n are empty)
            sv_[lo + 1:hi + 2] = 0
        want = int(sv_.sum())
        add(f"tiles_{n}", "tiles", gx[pick], hx[pick], rv_, sv_,
            claim=(lambda w: lambda res, it1, c: _participants(res, it1, c) == w and res["valid"] == 1)(want))
    # ---- two identical neighbouring ref points: a segment of length 0, the correspondence is rejected
    tx = bx.copy()
    tx[121] = tx[120]
    def zero_segment(res, it1, c):
        on = np.flatnonzero(((it1.j1 == 120) & (it1.j2 == 121)) | ((it1.j1 == 121) & (it1.j2 == 120)))
        return res["valid"] == 1 and len(on) >= 1 and not np.any(it1.flags[on] & 2)
    add("twin_points", "twin", tx, sx, bv, sv, truth=d, claim=zero_segment)
    # ---- three neighbouring pairs swapped in index order on both sides: bearings no longer monotone, neighbours by index
    wx, ws = bx.copy(), sx.copy()
    for i in (30, 170, 301):
        wx[[i, i + 1]] = wx[[i + 1, i]]
        ws[[i, i + 1]] = ws[[i + 1, i]]
    def swapped(res, it1, c):
        ref, _ = c.ldps()
        turn = np.diff(np.unwrap(ref.theta))
        e = res["x"] - c.truth
        return res["valid"] == 1 and int((turn < 0).sum()) == 3 and math.hypot(e[0], e[1]) < 0.01 and abs(e[2]) < 0.01
    add("swapped_pairs", "swapped", wx, ws, bv, sv, truth=d, claim=swapped)
    return tuple(out)


def by_name() -> dict:
    return {c.name: c for c in cases()}


NAMES = [c.name for c in cases()]
SCENARIOS = sorted({c.scenario for c in cases()})
CLOUD_ONLY = sorted(["valid_null", "nonfinite", "nan_z", "origin", "few_points", "tiles", "twin", "swapped"])


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(sm_icp's result, the restatement's result, its iterations, near_epsilon) of a case on cloud_to_ldp, computed once."""
    import plicp_restatement as R

    c = by_name()[name]
    ref, sens = c.ldps()
    direct = P.sm_icp(c.params(), ref, sens, c.guess)
    res, its, near = R.iterate(c.params(), ref, sens, c.guess)
    return direct, res, its, near
