"""lesson2 point-to-point ICP pair match -- a CPU HELPER under tools/, NOT part of the accelerator package (which holds only
the GPU path and has no CPU fallback).  numpy only.

Follows the two nodes of lesson2:
  * `scan_to_cloud` -- ConvertScan2PointCloud (lesson2/src/scan_match_icp.cc:89-130) and, with invalid_as_nan = 1,
                       ScanToPointCloud2Converter::ScanCallback (scan_to_pointclod2_converter.cc:44-92),
  * `icp`           -- ScanMatchWithICP (scan_match_icp.cc:135-164): a default-configured
                       pcl::IterativeClosestPoint<PointXYZ, PointXYZ>, source = last cloud, target = current cloud.

PARITY UNPINNED: the arithmetic of the reference lives in PCL (with FLANN and Eigen under it), which is neither vendored nor
pinned.  `icp` below RESTATES PCL 1.8's IterativeClosestPoint::computeTransformation with DefaultConvergenceCriteria; it is
this restatement, not PCL, that defines what csrc/icp.hip computes.  Five deliberate rules:
  1. LOWEST INDEX: among equal distances the lowest target index wins (FLANN's order among equals is unspecified).
  2. FP64 ON THE ORIGINAL POINTS: every iteration transforms the ORIGINAL float32 source points by the accumulated
     transform in fp64, where PCL re-transforms a float cloud in place.
  3. 2-D CLOSED FORM: theta = atan2(Sxy - Syx, Sxx + Syy), t = qbar - R(theta) pbar on x, y (z is ignored), where PCL runs a
     3-D SVD.
  4. LITERAL ORIGIN POINTS: an invalid reading stays in the cloud as the point (0, 0, 0), as the node leaves it (it even sets
     is_dense = true), and is matched like any other point.
  5. skip_invalid = 1 is the opt-in that removes the invalid readings from both clouds.  A point whose x or y is not finite
     (the converter's NaN point) never takes part, in either mode.
And one fact about the definition: the ORDER OF THE SUMS is part of it (`block_sum`: 256 strided partials, a binary tree per
64, the four groups in order -- the order the kernel sums in).  With the default transformation_epsilon = 0, rule (b) fires
only on an increment that is exactly the identity, which at a fixed point is a matter of the sums' last bit.

The iteration, in this order: transform; nearest target per source point; accept iff d2 <= max_correspondence_distance^2;
fewer than 3 accepted -> converged = 0, state 5, x keeps the accumulated pose; fit in two passes (means, centred sums);
T <- increment o T; iterations += 1; mse = mean accepted d2 of THIS iteration's search; stop rules (a) iterations >=
max_iterations -> state 1, (b) cos(theta) >= 1 - transformation_epsilon and |t|^2 <= transformation_epsilon -> state 2,
(c) |mse - prev| < absolute_mse -> state 3, (d) |mse - prev| / prev < euclidean_fitness_epsilon -> state 4; else prev = mse.
"""
from __future__ import annotations

import dataclasses
import math
import sys

import numpy as np

DBL_MAX = sys.float_info.max
STATE_NOT_CONVERGED, STATE_ITERATIONS, STATE_TRANSFORM, STATE_ABS_MSE, STATE_REL_MSE, STATE_FEW = 0, 1, 2, 3, 4, 5
MISTAKES = ("tie_high", "no_centre", "theta_sign", "compose_order", "swap", "mse_after", "gate_strict", "window_inclusive")


@dataclasses.dataclass
class IcpParams:
    """What lesson2 leaves in place: PCL's defaults."""

    max_iterations: int = 10
    max_correspondence_distance: float = math.sqrt(DBL_MAX)
    transformation_epsilon: float = 0.0
    euclidean_fitness_epsilon: float = -DBL_MAX
    absolute_mse: float = 1e-12
    skip_invalid: int = 0
    invalid_as_nan: int = 0


@dataclasses.dataclass
class Iteration:
    """What one iteration decided."""

    corr: np.ndarray      # int32 [n]: the target index per source point, -1 = rejected or masked
    d2: np.ndarray        # float64 [n]: the best squared distance (inf where the point is masked or has no target)
    d2_other: np.ndarray  # float64 [n]: the best among the target points whose COORDINATES differ from the winner's
    ncorr: int
    inc: np.ndarray | None  # (tx, ty, theta), None where fewer than 3 were accepted
    mse: float
    state: int            # the stop rule that fired, 0 = none, 5 = fewer than 3 correspondences
    mse_gap: float        # | |mse - prev| - absolute_mse |, inf where rule (c) was not reached


def scan_to_cloud(ranges, angle_min, angle_increment, range_min, range_max, invalid_as_nan=0, mistake=None):
    """ranges float32 [n] -> (xyz float32 [n, 3], valid uint8 [n])."""
    r = np.asarray(ranges, dtype=np.float32)
    n = len(r)
    lo, hi = np.float32(range_min), np.float32(range_max)
    with np.errstate(invalid="ignore"):
        if mistake == "window_inclusive":
            valid = np.isfinite(r) & (r >= lo) & (r <= hi)
        else:
            valid = np.isfinite(r) & (r > lo) & (r < hi)
    angle = np.float32(angle_min) + np.arange(n, dtype=np.float32) * np.float32(angle_increment)  # float32 throughout
    assert angle.dtype == np.float32
    a = angle.astype(np.float64)
    rv = np.where(valid, r, np.float32(0)).astype(np.float64)
    fill = np.float32(np.nan) if invalid_as_nan else np.float32(0)
    xyz = np.full((n, 3), fill, np.float32)
    xyz[valid, 0] = (rv * np.cos(a)).astype(np.float32)[valid]
    xyz[valid, 1] = (rv * np.sin(a)).astype(np.float32)[valid]
    xyz[valid, 2] = np.float32(0)
    return xyz, valid.astype(np.uint8)


def _usable(xyz, valid, skip):
    ok = np.isfinite(xyz[:, 0]) & np.isfinite(xyz[:, 1])
    if skip and valid is not None:
        ok &= np.asarray(valid).astype(bool)
    return ok


def _search(px, py, src_ok, qx, qy, tgt_ok, tie_high=False, want_other=False):
    """Nearest usable target per usable source point -> (j int64 [n] (-1: none), d2 [n], d2_other [n])."""
    n, m = len(px), len(qx)
    j = np.full(n, -1, np.int64)
    d2 = np.full(n, np.inf)
    other = np.full(n, np.inf)
    if n == 0 or m == 0 or not tgt_ok.any() or not src_ok.any():
        return j, d2, other
    dx = px[:, None] - qx[None, :]
    dy = py[:, None] - qy[None, :]
    d = dx * dx + dy * dy
    d[:, ~tgt_ok] = np.inf
    if tie_high:
        jj = m - 1 - np.argmin(d[:, ::-1], axis=1)
    else:
        jj = np.argmin(d, axis=1)  # the first of equals
    best = d[np.arange(n), jj]
    hit = src_ok & np.isfinite(best)
    j[hit] = jj[hit]
    d2[hit] = best[hit]
    if want_other:
        same = (qx[None, :] == qx[jj][:, None]) & (qy[None, :] == qy[jj][:, None])
        d[same] = np.inf
        other[hit] = d.min(axis=1)[hit]
    return j, d2, other


def block_sum(values, take) -> float:
    """The sum of values[take] in the DEFINED order: 256 partial sums, partial l over the points l, l + 256, ... in ascending
    index; a binary tree over each group of 64 partials (l += l + 32, then + 16, ... + 1); the four groups in order.  With
    transformation_epsilon = 0 rule (b) asks whether an increment is exactly the identity, which at a fixed point is decided by
    the last bit of these sums: the order is part of the definition, and csrc/icp.hip sums in it."""
    v = np.where(take, values, 0.0)
    tiles = max(1, -(-len(v) // 256))
    padded = np.zeros(tiles * 256)
    padded[:len(v)] = v
    part = np.zeros(256)
    for row in padded.reshape(tiles, 256):
        part = part + row
    w = part.reshape(4, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
    total = 0.0
    for g in range(4):
        total = total + float(w[g, 0])
    return total


def icp(src_xyz, tgt_xyz, params: IcpParams | None = None, first_guess=(0.0, 0.0, 0.0), src_valid=None, tgt_valid=None,
        mistake=None, trace=True) -> dict:
    """-> {x[3], fitness, mse, converged, iterations, ncorr, state, trace: [Iteration]}."""
    P = params if params is not None else IcpParams()
    src = np.asarray(src_xyz, dtype=np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt_xyz, dtype=np.float32).reshape(-1, 3)
    if mistake == "swap":
        src, tgt, src_valid, tgt_valid = tgt, src, tgt_valid, src_valid
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    qx, qy = tgt[:, 0].astype(np.float64), tgt[:, 1].astype(np.float64)
    src_ok, tgt_ok = _usable(src, src_valid, P.skip_invalid), _usable(tgt, tgt_valid, P.skip_invalid)
    max_d2 = P.max_correspondence_distance * P.max_correspondence_distance
    c, s = math.cos(first_guess[2]), math.sin(first_guess[2])
    tx, ty = float(first_guess[0]), float(first_guess[1])
    prev = DBL_MAX
    out = {"converged": 0, "iterations": 0, "ncorr": 0, "state": STATE_NOT_CONVERGED, "mse": 0.0, "trace": []}
    while True:
        px = (c * sx - s * sy) + tx
        py = (s * sx + c * sy) + ty
        j, d2, other = _search(px, py, src_ok, qx, qy, tgt_ok, mistake == "tie_high", trace)
        with np.errstate(invalid="ignore"):
            acc = (j >= 0) & ((d2 < max_d2) if mistake == "gate_strict" else (d2 <= max_d2))
        ncorr = int(acc.sum())
        out["ncorr"] = ncorr
        corr = np.where(acc, j, -1).astype(np.int32)
        if ncorr < 3:
            out["state"] = STATE_FEW
            out["trace"].append(Iteration(corr, d2, other, ncorr, None, out["mse"], STATE_FEW, math.inf))
            break
        jj = np.where(acc, j, 0)
        ax, ay, bx, by = px, py, qx[jj], qy[jj]          # per source point; only the accepted ones are summed
        pbx, pby = block_sum(ax, acc) / ncorr, block_sum(ay, acc) / ncorr
        qbx, qby = block_sum(bx, acc) / ncorr, block_sum(by, acc) / ncorr
        if mistake == "no_centre":
            ux, uy, vx, vy = ax, ay, bx, by
        else:
            ux, uy, vx, vy = ax - pbx, ay - pby, bx - qbx, by - qby
        with np.errstate(invalid="ignore"):
            sxx, sxy = block_sum(ux * vx, acc), block_sum(ux * vy, acc)
            syx, syy = block_sum(uy * vx, acc), block_sum(uy * vy, acc)
        th = math.atan2(sxy - syx, sxx + syy)
        if mistake == "theta_sign":
            th = -th
        ct, st = math.cos(th), math.sin(th)
        ix, iy = qbx - (ct * pbx - st * pby), qby - (st * pbx + ct * pby)
        if mistake == "compose_order":   # T o increment
            c, s, tx, ty = c * ct - s * st, s * ct + c * st, (c * ix - s * iy) + tx, (s * ix + c * iy) + ty
        else:                            # increment o T
            c, s, tx, ty = ct * c - st * s, st * c + ct * s, (ct * tx - st * ty) + ix, (st * tx + ct * ty) + iy
        out["iterations"] += 1
        if mistake == "mse_after":
            ex, ey = ((ct * ax - st * ay) + ix) - bx, ((st * ax + ct * ay) + iy) - by
            mse = block_sum(ex * ex + ey * ey, acc) / ncorr
        else:
            mse = block_sum(d2, acc) / ncorr
        out["mse"] = mse
        state, gap = STATE_NOT_CONVERGED, math.inf
        if out["iterations"] >= P.max_iterations:
            state = STATE_ITERATIONS
        elif ct >= 1.0 - P.transformation_epsilon and ix * ix + iy * iy <= P.transformation_epsilon:
            state = STATE_TRANSFORM
        else:
            gap = abs(abs(mse - prev) - P.absolute_mse)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.float64(abs(mse - prev)) / np.float64(prev)
            if abs(mse - prev) < P.absolute_mse:
                state = STATE_ABS_MSE
            elif rel < P.euclidean_fitness_epsilon:
                state = STATE_REL_MSE
        out["trace"].append(Iteration(corr, d2, other, ncorr, np.array([ix, iy, th]), mse, state, gap))
        if state:
            out["converged"], out["state"] = 1, state
            break
        prev = mse
    px = (c * sx - s * sy) + tx
    py = (s * sx + c * sy) + ty
    j, d2, _ = _search(px, py, src_ok, qx, qy, tgt_ok, mistake == "tie_high")
    hit = j >= 0
    out["fitness"] = block_sum(d2, hit) / int(hit.sum()) if hit.any() else DBL_MAX
    out["x"] = np.array([tx, ty, math.atan2(s, c)])
    return out


def one_iteration(src_xyz, tgt_xyz, params: IcpParams | None = None, x_in=(0.0, 0.0, 0.0), src_valid=None, tgt_valid=None):
    """The first iteration from x_in, as k_icp_debug reports it."""
    P = dataclasses.replace(params if params is not None else IcpParams(), max_iterations=1)
    return icp(src_xyz, tgt_xyz, P, x_in, src_valid, tgt_valid)["trace"][0]
