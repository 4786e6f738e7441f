"""One iteration of tools/plicp_cpu.py's sm_icp, with the discrete decisions it takes on the way and how far each was from
going the other way.  The expressions are sm_icp's own, in its order, so that iterating `iteration` reproduces sm_icp's x,
iterations, nvalid and valid exactly (tests/test_plicp_cases_oracle.py asserts it); the solve IS plicp_cpu's.

Per READING of the sens scan (what lslam_plicp_debug_iteration reports):
  j1, j2   ref reading indices of the segment, -1 where none (an invalid reading; j2: no valid index neighbour of j1)
  flags    bit 0 valid reading, bit 1 correspondence accepted before outlier rejection, bit 2 kept after it
  undecided  True where one of this reading's decisions is within REL of flipping
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from tools import plicp_cpu as P

REL = 1e-9  # a decision closer than this (relative) to flipping is "undecided"


@dataclasses.dataclass
class Iteration:
    j1: np.ndarray
    j2: np.ndarray
    flags: np.ndarray
    sol: np.ndarray | None      # the solved pose, None at an early exit
    exit: str | None            # None, "few_valid", "few_corr", "few_kept", "singular"
    nvalid: int
    error: float
    undecided: np.ndarray       # bool per sens reading
    case_undecided: list        # names of case-level decisions within REL of flipping


def _close(a, b):
    """|a - b| within REL of the larger magnitude (both finite)."""
    return np.abs(a - b) <= REL * np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


def iteration(params: P.PlicpParams, ref: P.Ldp, sens: P.Ldp, x, margins: bool = True) -> Iteration:
    n = len(sens.valid)
    ref_ok = np.flatnonzero(ref.valid)
    sens_ok = np.flatnonzero(sens.valid)
    j1_r = np.full(n, -1, np.int32)
    j2_r = np.full(n, -1, np.int32)
    flags = np.zeros(n, np.uint8)
    flags[sens_ok] = 1
    und = np.zeros(n, bool)
    case_und = []
    if len(ref_ok) < 3 or len(sens_ok) < 3:
        return Iteration(j1_r, j2_r, flags, None, "few_valid", 0, float("inf"), und, case_und)
    q_all = ref.points()
    p_all = sens.points()
    x = np.array(x, dtype=np.float64)
    max_d2 = params.max_correspondence_dist ** 2
    c, s = math.cos(x[2]), math.sin(x[2])
    pw = p_all[sens_ok] @ np.array([[c, s], [-s, c]]) + x[:2]
    d2 = ((pw[:, None, :] - q_all[ref_ok][None, :, :]) ** 2).sum(axis=2)
    j1k = d2.argmin(axis=1)
    j1 = ref_ok[j1k]
    dmin = d2[np.arange(len(sens_ok)), j1k]
    nref = len(ref.valid)
    lo, hi = np.clip(j1 - 1, 0, nref - 1), np.clip(j1 + 1, 0, nref - 1)
    d_lo = np.where((ref.valid[lo] == 1) & (lo != j1), ((pw - q_all[lo]) ** 2).sum(axis=1), np.inf)
    d_hi = np.where((ref.valid[hi] == 1) & (hi != j1), ((pw - q_all[hi]) ** 2).sum(axis=1), np.inf)
    j2 = np.where(d_lo <= d_hi, lo, hi)
    has2 = np.isfinite(np.minimum(d_lo, d_hi))
    ok = (dmin <= max_d2) & has2
    seg = q_all[j2] - q_all[j1]
    seg_len = np.linalg.norm(seg, axis=1)
    ok &= seg_len > 1e-12
    nrm = np.zeros_like(seg)
    nrm[ok] = np.stack([-seg[ok, 1], seg[ok, 0]], axis=1) / seg_len[ok, None]
    dist = np.abs(((pw - q_all[j1]) * nrm).sum(axis=1)) if params.use_point_to_line_distance else np.sqrt(dmin)
    j1_r[sens_ok] = j1
    j2_r[sens_ok] = np.where(has2, j2, -1)
    flags[sens_ok] |= (ok.astype(np.uint8) << 1)
    u = np.zeros(len(sens_ok), bool)  # undecided, by sens order
    if margins:
        if d2.shape[1] > 1:
            part = np.partition(d2, 1, axis=1)
            u |= _close(part[:, 0], part[:, 1])                      # best against second-best d^2
        both = np.isfinite(d_lo) & np.isfinite(d_hi)
        u |= both & _close(np.where(both, d_lo, 0.0), np.where(both, d_hi, 1.0))  # d_lo against d_hi
        u |= has2 & _close(dmin, max_d2)                             # the correspondence distance against its limit
        u |= has2 & (dmin <= max_d2) & _close(seg_len, 1e-12)        # the segment length against its guard
    pre = ok.copy()
    if params.outliers_remove_doubles:
        order = np.lexsort((dist, j1))
        first = np.ones(len(order), dtype=bool)
        first[1:] = j1[order][1:] != j1[order][:-1]
        keep = np.zeros(len(order), dtype=bool)
        keep[order[first]] = True
        ok &= keep
        if margins:  # the doubles' winner against the runner-up, on ref points where it matters to an accepted point
            so, jo, do = order, j1[order], dist[order]
            for a in np.flatnonzero(first):
                b = a + 1
                if b < len(so) and jo[b] == jo[a] and (pre[so[a]] or pre[so[b]]) and _close(do[a], do[b]) and do[a] != do[b]:
                    u[so[a]] = u[so[b]] = True
    idx = np.flatnonzero(ok)

    def done(sol, why, nvalid=0, err=float("inf")):
        und[sens_ok] = u
        return Iteration(j1_r, j2_r, flags, sol, why, nvalid, err, und, case_und)

    if len(idx) < 3:
        return done(None, "few_corr")
    srt = idx[np.argsort(dist[idx])]
    ncut = max(3, int(math.floor(params.outliers_maxPerc * len(srt))))
    full = srt
    srt = srt[:ncut]
    ridx = min(len(srt) - 1, int(math.floor(params.outliers_adaptive_order * len(srt))))
    ref_err = dist[srt[ridx]]
    thr = params.outliers_adaptive_mult * ref_err + 1e-12
    if margins:
        if len(full) > len(srt):  # the trimmed cut: the last one in against the first one out
            a, b = dist[full[len(srt) - 1]], dist[full[len(srt)]]
            if a == b or _close(a, b):  # (equal distances: numpy's sort order among them is not the library's tie rule)
                u[full[(dist[full] == a) | (dist[full] == b)]] = True
        # the adaptive threshold: which distance sits at rank ridx, and every distance against the threshold
        for nb in (ridx - 1, ridx + 1):
            if 0 <= nb < len(srt) and dist[srt[nb]] != ref_err and _close(dist[srt[nb]], ref_err):
                case_und.append("adaptive_rank")
        u[srt] |= _close(dist[srt], thr)
    srt = srt[dist[srt] <= thr]
    flags[sens_ok[srt]] |= 4
    if len(srt) < 3:
        return done(None, "few_kept")
    sol = P._solve_point_to_line(p_all[sens_ok][srt], q_all[j1[srt]], nrm[srt])
    if margins:
        a = np.stack([nrm[srt, 0], nrm[srt, 1]], axis=1)
        det = abs(np.linalg.det(a.T @ a))
        if abs(det - 1e-12) <= 1e-3 * 1e-12:  # |det| against its guard (sums of ~n terms: a wide band)
            case_und.append("det")
    if sol is None:
        return done(None, "singular")
    cs, sn = math.cos(sol[2]), math.sin(sol[2])
    res = ((p_all[sens_ok][srt] @ np.array([[cs, sn], [-sn, cs]]) + sol[:2] - q_all[j1[srt]]) * nrm[srt]).sum(axis=1)
    return done(sol, None, len(srt), float((res ** 2).sum()))


def iterate(params: P.PlicpParams, ref: P.Ldp, sens: P.Ldp, first_guess=(0.0, 0.0, 0.0)):
    """sm_icp through `iteration` -> (result dict as sm_icp's, the list of Iteration, near_epsilon).  near_epsilon: a step
    landed within REL of epsilon_xy / epsilon_theta, so the iteration COUNT is undecided."""
    out = {"valid": 0, "x": np.zeros(3), "iterations": 0, "nvalid": 0, "error": float("inf")}
    x = np.array(first_guess, dtype=np.float64)
    its, near = [], False
    nvalid, err, it = 0, float("inf"), 0
    for it in range(1, params.max_iterations + 1):
        r = iteration(params, ref, sens, x, margins=(it == 1))
        its.append(r)
        if r.sol is None:
            return out, its, near
        nvalid, err = r.nvalid, r.error
        delta = r.sol - x
        delta[2] = math.remainder(delta[2], 2.0 * math.pi)
        x = r.sol
        dxy, dth = math.hypot(delta[0], delta[1]), abs(delta[2])
        near |= abs(dxy - params.epsilon_xy) <= REL or abs(dth - params.epsilon_theta) <= REL
        if dxy < params.epsilon_xy and abs(delta[2]) < params.epsilon_theta:
            break
    out.update(iterations=it, nvalid=int(nvalid), error=err, x=x)
    lin = math.hypot(x[0] - first_guess[0], x[1] - first_guess[1])
    ang = abs(math.remainder(x[2] - first_guess[2], 2.0 * math.pi))
    within = lin <= params.max_linear_correction and ang <= math.radians(params.max_angular_correction_deg)
    out["valid"] = int(within and nvalid >= 3)
    out["valid_undecided"] = bool(_close(lin, params.max_linear_correction) or
                                  _close(ang, math.radians(params.max_angular_correction_deg)))
    return out, its, near
