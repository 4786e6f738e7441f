"""OccGridMapUtil's pose scoring restated in numpy: getResidualForState / getLikelihoodForState (H/map/OccGridMapUtil.h:342-374)
with interpMapValue (:379-434), the seven sigma points and the weighted covariance of getCovarianceForPose (:249-306) and
getCovMatrixWorldCoords (:314-339) -- once in float32, operation by operation in the order the recorded reference evaluates
them (tests/test_score_oracle.py holds it to the golden file bit for bit), and once in float64 from the same planes, which is
what the device's parallel sums are measured against.

Rounding that is not numpy's: exp is the C library's double exp rounded to float (getGridProbability, GridMapLogOdds.h:123-127),
sin / cos of a heading the double functions rounded to float, as the ordered device kernels evaluate them."""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64


class Level:
    """One level of a map as the scoring reads it: the plane's cell probabilities, its size, world -> raster constants."""

    def __init__(self, plane, cell, off, level):
        self.sy, self.sx = plane.shape
        self.cell = f32(cell)
        self.scale = f32(1.0) / self.cell                       # GridMapBase.h:276
        self.tx, self.ty = self.scale * f32(off[0]), self.scale * f32(off[1])
        self.factor = f32(1.0 / 2.0 ** level)                   # MapRepMultiMap.h:161
        lo = np.asarray(plane, f32).reshape(-1)
        odds = np.array([math.exp(float(v)) for v in lo], f64).astype(f32)
        self.prob = odds / (odds + f32(1.0))                    # float32 [sy * sx]
        odds64 = np.exp(lo.astype(f64))
        self.prob64 = odds64 / (odds64 + 1.0)

    def map_pose(self, world):
        """getMapCoordsPose (GridMapBase.h:238-242) of world poses [S,3] float32 -> [S,3] float32."""
        w = np.asarray(world, f32).reshape(-1, 3)
        e0 = (self.scale * w[:, 0] + f32(0.0) * w[:, 1]) + self.tx
        e1 = (f32(0.0) * w[:, 0] + self.scale * w[:, 1]) + self.ty
        return np.stack([e0, e1, w[:, 2]], 1)

    def map_pose64(self, world):
        w = np.asarray(world, f32).reshape(-1, 3).astype(f64)
        return np.stack([f64(self.scale) * w[:, 0] + f64(self.tx), f64(self.scale) * w[:, 1] + f64(self.ty), w[:, 2]], 1)


def _sincos32(a):
    return (np.array([math.sin(float(v)) for v in a], f64).astype(f32), np.array([math.cos(float(v)) for v in a], f64).astype(f32))


def terms(lv: Level, pts, states):
    """1 - interpMapValue(T(state) * p * factor) per (state, point) in float32 -> [S, n]; states on the level's raster."""
    st = np.asarray(states, f32).reshape(-1, 3)
    q = np.asarray(pts, f32).reshape(-1, 2) * lv.factor
    s, c = _sincos32(st[:, 2])
    px, py = q[None, :, 0], q[None, :, 1]
    cx = (c[:, None] * px + (-s)[:, None] * py) + st[:, 0:1]
    cy = (s[:, None] * px + c[:, None] * py) + st[:, 1:2]
    out = (cx < 0) | (cx > f32(lv.sx - 2)) | (cy < 0) | (cy > f32(lv.sy - 2))  # pointOutOfMapBounds (:60-63)
    with np.errstate(invalid="ignore"):
        ix, iy = np.where(out, 0, cx).astype(np.int32), np.where(out, 0, cy).astype(np.int32)
    fx, fy = cx - ix.astype(f32), cy - iy.astype(f32)
    idx = iy * lv.sx + ix
    i0, i1, i2, i3 = lv.prob[idx], lv.prob[idx + 1], lv.prob[idx + lv.sx], lv.prob[idx + lv.sx + 1]
    xi, yi = f32(1.0) - fx, f32(1.0) - fy
    v = ((i0 * xi + i1 * fx) * yi) + ((i2 * xi + i3 * fx) * fy)
    return f32(1.0) - np.where(out, f32(0.0), v), out


def score(lv: Level, pts, states, chunk=512):
    """-> (residual[S], likelihood[S]) float32: the terms added in container order like the reference's loop (:366-371)."""
    st = np.asarray(states, f32).reshape(-1, 3)
    n = len(np.asarray(pts).reshape(-1, 2))
    res = np.zeros(len(st), f32)
    if n:
        step = max(1, chunk * 1081 // max(n, 1))
        for a in range(0, len(st), step):
            t, _ = terms(lv, pts, st[a:a + step])
            res[a:a + step] = np.cumsum(t, axis=1, dtype=f32)[:, -1]  # (an accumulate is sequential)
    with np.errstate(invalid="ignore", divide="ignore"):
        return res, f32(1.0) - (res / f32(n))


def score_world(lv: Level, pts, world):
    return score(lv, pts, lv.map_pose(world))


def score64(lv: Level, pts, world, chunk=512, states=None):
    """The same quantities in float64 from the same plane, container and float32 world poses -> (residual[S], likelihood[S]).
    `states`: float32 states on the level's raster instead (the sigma points), taken as they are."""
    st = lv.map_pose64(world) if states is None else np.asarray(states, f32).reshape(-1, 3).astype(f64)
    q = np.asarray(pts, f32).reshape(-1, 2).astype(f64) * f64(lv.factor)
    n = len(q)
    res = np.zeros(len(st), f64)
    step = max(1, chunk * 1081 // max(n, 1))
    for a in range(0, len(st), step if n else len(st) or 1):
        e = st[a:a + step]
        s, c = np.sin(e[:, 2])[:, None], np.cos(e[:, 2])[:, None]
        cx = c * q[None, :, 0] - s * q[None, :, 1] + e[:, 0:1]
        cy = s * q[None, :, 0] + c * q[None, :, 1] + e[:, 1:2]
        out = (cx < 0) | (cx > lv.sx - 2) | (cy < 0) | (cy > lv.sy - 2)
        ix, iy = np.where(out, 0, cx).astype(np.int64), np.where(out, 0, cy).astype(np.int64)
        fx, fy = cx - ix, cy - iy
        idx = iy * lv.sx + ix
        p = lv.prob64
        v = (p[idx] * (1 - fx) + p[idx + 1] * fx) * (1 - fy) + (p[idx + lv.sx] * (1 - fx) + p[idx + lv.sx + 1] * fx) * fy
        res[a:a + step] = (1.0 - np.where(out, 0.0, v)).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return res, 1.0 - res / f64(n)


def sigma_points(map_pose):
    """The seven states of getCovarianceForPose (:252-268) around one pose on the level's raster -> [7,3] float32."""
    x, y, a = (f32(v) for v in map_pose)
    dT, dA = f32(1.5), f32(0.05)
    return np.array([[x + dT, y, a], [x - dT, y, a], [x, y + dT, a], [x, y - dT, a], [x, y, a + dA], [x, y, a - dA], [x, y, a]], f32)


def covariance(sp, lik, cell):
    """Weighted mean and covariance of the sigma points (:280-302) and the world scaling (:314-339) in float32, in Eigen's
    orders (oracle/shim/Eigen/Core: the 7-term sum() in halves, += coefficient-wise, the outer product before its scalar)
    -> (cov_map[3,3], cov_world[3,3])."""
    sp, l = np.asarray(sp, f32), np.asarray(lik, f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inv = f32(1.0) / ((l[0] + (l[1] + l[2])) + ((l[3] + l[4]) + (l[5] + l[6])))
        mean = np.zeros(3, f32)
        for i in range(7):
            mean = mean + sp[i] * l[i]
        mean = mean * inv
        m = np.zeros((3, 3), f32)
        for i in range(7):
            d = sp[i] - mean
            m = m + (l[i] * inv) * np.outer(d, d).astype(f32)
        sc = f32(cell)
        sq = sc * sc
        w = np.zeros((3, 3), f32)
        w[0, 0], w[1, 1] = m[0, 0] * sq, m[1, 1] * sq
        w[1, 0] = m[1, 0] * sq
        w[0, 1] = w[1, 0]
        w[2, 0] = m[2, 0] * sc
        w[0, 2] = w[2, 0]
        w[2, 1] = m[2, 1] * sc
        w[1, 2] = w[2, 1]
        w[2, 2] = m[2, 2]
    return m, w


def pose_covariance(lv: Level, pts, world):
    """-> (likelihoods[7], cov_map, cov_world) float32 of one (container, world pose)."""
    sp = sigma_points(lv.map_pose(world)[0])
    _, lik = score(lv, pts, sp)
    return (lik,) + covariance(sp, lik, lv.cell)


def best_state(volume):
    """Highest likelihood, lowest linear index among equals, NaN never; (-1, NaN) when every value is NaN."""
    v = np.asarray(volume, f32).reshape(-1)
    if not len(v) or np.isnan(v).all():
        return -1, f32(np.nan)
    i = int(np.argmax(np.where(np.isnan(v), -np.inf, v)))
    return i, v[i]


# ---- the golden file's maps as Levels, and E_ref --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def levels():
    """(map name, level) -> Level, from the golden file's planes."""
    import score_cases as S

    g = S.golden()
    return {(name, L): Level(g.planes[name, L], cell, m.off, L)
            for name, m in g.maps.items() for L, (_, _, cell) in enumerate(S.level_list(m))}


@functools.lru_cache(maxsize=None)
def float64_all():
    """(residual[Q], likelihood[Q]) in float64 of every recorded query, in score_cases.all_queries() order."""
    import score_cases as S

    g, lv = S.golden(), levels()
    qs = S.all_queries()
    res, lik = np.zeros(len(qs)), np.zeros(len(qs))
    groups = {}
    for i, q in enumerate(qs):
        groups.setdefault((q.map, q.container, q.level), []).append(i)
    for (m, c, L), idx in groups.items():
        r, l = score64(lv[m, L], g.containers[c], np.array([qs[i].pose for i in idx], f32))
        res[idx], lik[idx] = r, l
    return res, lik


@functools.lru_cache(maxsize=None)
def e_ref():
    """E_ref: the worst |reference - float64| likelihood over all recorded queries (NaN against NaN is no difference)."""
    import score_cases as S

    g = S.golden()
    _, lik = float64_all()
    d = np.abs(g.likelihood.astype(f64) - lik)
    assert (np.isnan(g.likelihood) == np.isnan(lik)).all()
    return float(np.nanmax(d))


# The floor of the default mode's bound: gn_prob_f evaluates exp and the reciprocal on the hardware units at
# ~1e-7 relative each, so a cell probability (<= 1) is off by <= 2e-7; interpMapValue is a weighted mean of four of them --
# bounded here without using that the weights sum to one, 4 * 2e-7 --, and the likelihood ends in one division, 1e-7 of a
# value <= 1.  Sums of n such terms are divided by n again, so the bound does not grow with the container.
FLOOR = 4 * 2e-7 + 1e-7


def bound():
    return max(4.0 * e_ref(), FLOOR)
