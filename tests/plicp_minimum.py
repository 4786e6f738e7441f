"""The minimum of the point-to-line cost that PL-ICP's solve claims to minimise, by a route that shares nothing with
tools/plicp_cpu.py's _solve_point_to_line and does not go through the Lagrange quartic.

    cost(t, theta) = sum_k (n_k . (R(theta) p_k + t - q_k))^2

Eliminating t (the cost is quadratic in it) leaves C(theta) = u^T S u + h^T u + c0 with u = (cos theta, sin theta).  dC/dtheta
is a trigonometric polynomial of degree 2 -- at most four zeros on the circle -- so its sign changes on a 4096-step lattice
find every stationary angle unless two of them lie within 1.5e-3 rad; each is bisected down to neighbouring doubles, and the
lowest C wins.  All sums and every evaluation are in np.longdouble (64-bit mantissa on x86)."""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
LATTICE = 4096


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def cost(x, p, q, nrm) -> float:
    """The sum of squared point-to-line residuals at the pose x = (tx, ty, theta), straight from its definition."""
    p, q, nrm = _ld(p), _ld(q), _ld(nrm)
    th = LD(x[2])
    c, s = np.cos(th), np.sin(th)
    rx = (c * p[:, 0] - s * p[:, 1]) + LD(x[0]) - q[:, 0]
    ry = (s * p[:, 0] + c * p[:, 1]) + LD(x[1]) - q[:, 1]
    res = nrm[:, 0] * rx + nrm[:, 1] * ry
    return float((res * res).sum())


def _reduced(p, q, nrm):
    """(ainv, B, g, S, h): the 2x2 blocks of the normal equations with t eliminated."""
    nx, ny = nrm[:, 0], nrm[:, 1]
    cols = [nx, ny, nx * p[:, 0] + ny * p[:, 1], ny * p[:, 0] - nx * p[:, 1]]   # d residual / d (tx, ty, cos, sin)
    b = nx * q[:, 0] + ny * q[:, 1]
    m = np.array([[(ci * cj).sum() for cj in cols] for ci in cols], dtype=LD)
    g = np.array([-2 * (ci * b).sum() for ci in cols], dtype=LD)
    a00, a01, a11 = m[0, 0], m[0, 1], m[1, 1]
    det = a00 * a11 - a01 * a01
    ainv = np.array([[a11, -a01], [-a01, a00]], dtype=LD) / det
    B = m[:2, 2:]
    S = m[2:, 2:] - B.T @ ainv @ B
    h = g[2:] - B.T @ ainv @ g[:2]
    return ainv, B, g, S, h


def minimum(p, q, nrm):
    """-> (x[3] float64, cost, runner_up_gap).  cost is the full sum of squared residuals at x; runner_up_gap is
    (C2 - C1) / C2 between the lowest stationary cost C1 and the next local minimum's C2 (inf where there is no other)."""
    p, q, nrm = _ld(p), _ld(q), _ld(nrm)
    ainv, B, g, S, h = _reduced(p, q, nrm)

    def slope(th):  # dC/dtheta, of a scalar or an array of angles
        th = np.asarray(th, dtype=np.float64).astype(LD)
        c, s = np.cos(th), np.sin(th)
        return 2 * (-s * (S[0, 0] * c + S[0, 1] * s) + c * (S[1, 0] * c + S[1, 1] * s)) + (h[1] * c - h[0] * s)

    def pose(th):
        u = np.array([np.cos(LD(th)), np.sin(LD(th))])
        t = -(ainv @ (B @ u + g[:2] / 2))
        return np.array([float(t[0]), float(t[1]), math.atan2(math.sin(th), math.cos(th))])

    grid = [2.0 * math.pi * i / LATTICE for i in range(LATTICE + 1)]
    d = slope(grid)
    found = []  # (cost, pose, is a minimum)
    for i in range(LATTICE):
        if d[i] == 0 or (d[i] < 0) != (d[i + 1] < 0):
            lo, hi, lo_neg = grid[i], grid[i + 1], d[i] < 0
            if d[i] == 0:
                hi, lo_neg = lo, d[i - 1] < 0
            while True:
                mid = 0.5 * (lo + hi)
                if not (lo < mid < hi):
                    break
                if (slope(mid) < 0) == lo_neg:
                    lo = mid
                else:
                    hi = mid
            x = min((pose(lo), pose(hi)), key=lambda xx: cost(xx, p, q, nrm))
            found.append((cost(x, p, q, nrm), x, lo_neg))
    assert found, "a continuous function on the circle has a minimum"
    found.sort(key=lambda f: f[0])
    best = found[0]
    others = [f[0] for f in found[1:] if f[2]]
    gap = (others[0] - best[0]) / others[0] if others and others[0] > 0 else float("inf")
    return best[1], best[0], gap
