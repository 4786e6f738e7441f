"""A numpy restatement of the GMapping hit/visit count map contract (include/lslam_gpu.h lslam_gmap_*),
in our own words: lesson4_gmapping_node's callback (CreateCache, ComputeMap, PublishMap over a ScanMatcherMap) plus the
library's generalisation to many scans at poses with cells outside the storage skipped and counted.

Everything fp64 is evaluated element by element in the contract's order (numpy ufuncs round each operation and never
fuse a multiply-add).  cos / sin come from the host libm's sincos(), like the library's host code: the node's CreateCache
loop takes cos and sin of one angle, which g++ -O2 merges into one sincos call, and glibc's sincos can differ from its cos
in the last bit (beam 927 of the 1081-beam fixture scan).
"""
from __future__ import annotations

import ctypes
import ctypes.util
import math
from dataclasses import dataclass, field

import numpy as np

PATCH_MAG = 5
NODE_DEFAULTS = dict(max_range=30 - 0.01, max_use_range=25.0, xmin=-40.0, ymin=-40.0, xmax=40.0, ymax=40.0, delta=0.05,
                     occ_thresh=0.25)


_LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_LIBM.sincos.restype = None
_LIBM.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]


def sincos(a: float):
    """(sin a, cos a) from the host libm's sincos()"""
    s, c = ctypes.c_double(), ctypes.c_double()
    _LIBM.sincos(float(a), ctypes.byref(s), ctypes.byref(c))
    return s.value, c.value


def c_round(v: np.ndarray) -> np.ndarray:
    """C round(): half away from zero (x - trunc(x) is exact in binary floating point)."""
    v = np.asarray(v, dtype=np.float64)
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


@dataclass
class Geometry:
    xmin: float
    ymin: float
    xmax: float
    ymax: float
    delta: float

    def __post_init__(self):
        wx, wy = (self.xmax - self.xmin) / self.delta, (self.ymax - self.ymin) / self.delta
        self.patches_x, self.patches_y = int(math.ceil(wx)) >> PATCH_MAG, int(math.ceil(wy)) >> PATCH_MAG
        self.size_x, self.size_y = self.patches_x << PATCH_MAG, self.patches_y << PATCH_MAG
        self.cx, self.cy = (self.xmin + self.xmax) / 2.0, (self.ymin + self.ymax) / 2.0
        self.size_x2 = int(c_round((self.cx - self.xmin) / self.delta))
        self.size_y2 = int(c_round((self.cy - self.ymin) / self.delta))
        self.width, self.height = int(wx), int(wy)  # (uint32) truncation of the double quotient

    def world2map(self, x, y):
        return (c_round((np.asarray(x) - self.cx) / self.delta).astype(np.int64) + self.size_x2,
                c_round((np.asarray(y) - self.cy) / self.delta).astype(np.int64) + self.size_y2)


def angle_cache(n_beams: int, angle_min: float, angle_increment: float):
    """angle_i = angle_min + i * angle_increment in float32, then double cos / sin (one sincos) -> (cos_i, sin_i)."""
    a = np.float32(angle_min) + np.arange(n_beams, dtype=np.float32) * np.float32(angle_increment)
    sc = np.array([sincos(float(v)) for v in a]).reshape(-1, 2)
    return sc[:, 1].copy(), sc[:, 0].copy()


def grid_line(p0, p1):
    """GridLineTraversal::gridLine, stepped: Bresenham from the endpoint with the smaller major coordinate (p0 on a tie),
    the list reversed when that was p1.  Returns the points from p0 to p1."""
    (x0, y0), (x1, y1) = p0, p1
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    pts = []
    if dy <= dx:
        if x0 > x1:
            x, y, ydir, xend = x1, y1, -1, x0
        else:
            x, y, ydir, xend = x0, y0, 1, x1
        up = (y1 - y0) * ydir > 0
        d, i1, i2 = 2 * dy - dx, 2 * dy, 2 * (dy - dx)
        pts.append((x, y))
        while x < xend:
            x += 1
            if d < 0:
                d += i1
            else:
                y += 1 if up else -1
                d += i2
            pts.append((x, y))
    else:
        if y0 > y1:
            x, y, xdir, yend = x1, y1, -1, y0
        else:
            x, y, xdir, yend = x0, y0, 1, y1
        right = (x1 - x0) * xdir > 0
        d, i1, i2 = 2 * dx - dy, 2 * dx, 2 * (dx - dy)
        pts.append((x, y))
        while y < yend:
            y += 1
            if d < 0:
                d += i1
            else:
                x += 1 if right else -1
                d += i2
            pts.append((x, y))
    if pts[0] != (x0, y0):
        pts.reverse()
    return pts


def line_cells_closed(p0x, p0y, p1x, p1y):
    """The same lines in closed form, vectorised over many: the minor offset after k major steps from the walk's start is
    floor((2 dmin k + dmaj) / (2 dmaj)).  Returns (line index, x, y, is_last) with the points of each line from p0 to p1."""
    p0x, p0y, p1x, p1y = (np.asarray(a, dtype=np.int64) for a in (p0x, p0y, p1x, p1y))
    dx, dy = np.abs(p1x - p0x), np.abs(p1y - p0y)
    xmaj = dy <= dx
    dmaj, dmin = np.where(xmaj, dx, dy), np.where(xmaj, dy, dx)
    from_p1 = np.where(xmaj, p0x > p1x, p0y > p1y)
    sx, sy = np.where(from_p1, p1x, p0x), np.where(from_p1, p1y, p0y)
    ex, ey = np.where(from_p1, p0x, p1x), np.where(from_p1, p0y, p1y)
    smin = np.where(xmaj, np.where(ey >= sy, 1, -1), np.where(ex >= sx, 1, -1))
    L = dmaj + 1
    line = np.repeat(np.arange(len(p0x)), L)
    start = np.cumsum(L) - L
    k = np.arange(int(L.sum())) - np.repeat(start, L)
    dm, dn = dmaj[line], dmin[line]
    m = np.where(dm > 0, (2 * dn * k + dm) // np.maximum(2 * dm, 1), 0)
    xm = xmaj[line]
    x = np.where(xm, sx[line] + k, sx[line] + smin[line] * m)
    y = np.where(xm, sy[line] + smin[line] * m, sy[line] + k)
    fp = from_p1[line]
    is_last = np.where(fp, k == 0, k == dm)  # p1
    # order each line's points from p0 to p1 (reversed walks)
    order_k = np.where(fp, dm - k, k)
    order = np.lexsort((order_k, line))
    return line[order], x[order], y[order], is_last[order]


@dataclass
class MapState:
    geo: Geometry
    visits: np.ndarray = field(init=False)
    n: np.ndarray = field(init=False)
    acc_x: np.ndarray = field(init=False)
    acc_y: np.ndarray = field(init=False)
    mask: np.ndarray = field(init=False)
    stats: list = field(init=False)

    def __post_init__(self):
        g = self.geo
        self.visits = np.zeros((g.size_y, g.size_x), np.int64)
        self.n = np.zeros((g.size_y, g.size_x), np.int64)
        self.acc_x = np.zeros((g.size_y, g.size_x), np.float32)
        self.acc_y = np.zeros((g.size_y, g.size_x), np.float32)
        self.mask = np.zeros((g.patches_y, g.patches_x), np.uint8)
        self.stats = [0, 0, 0, 0]  # scans, beams used, hits applied, cell updates dropped outside

    def _inside(self, x, y):
        return (x >= 0) & (y >= 0) & (x < self.geo.size_x) & (y < self.geo.size_y)

    def integrate(self, ranges, poses, cos_i, sin_i, max_range, max_use_range):
        """Scans in order; each scan's free updates, then its hits in beam order."""
        ranges = np.atleast_2d(np.asarray(ranges, dtype=np.float32))
        for s in range(ranges.shape[0]):
            pose = (0.0, 0.0, 0.0) if poses is None else tuple(float(v) for v in poses[s])
            self._scan(ranges[s], pose, cos_i, sin_i, max_range, max_use_range)

    def _scan(self, r, pose, cos_i, sin_i, max_range, max_use_range):
        g = self.geo
        x, y, th = pose
        s, c = sincos(th)
        d = r.astype(np.float64)
        with np.errstate(invalid="ignore"):
            used = ~((d > max_range) | (d == 0.0) | ~np.isfinite(d))
        idx = np.nonzero(used)[0]
        d = np.minimum(d[idx], max_use_range)
        ca, sa = cos_i[idx], sin_i[idx]
        phx = x + d * (c * ca - s * sa)
        phy = y + d * (s * ca + c * sa)
        p0x, p0y = g.world2map(x, y)
        p1x, p1y = g.world2map(phx, phy)
        self.stats[0] += 1
        self.stats[1] += len(idx)
        if len(idx):
            _, lx, ly, last = line_cells_closed(np.full(len(idx), p0x), np.full(len(idx), p0y), p1x, p1y)
            lx, ly = lx[~last], ly[~last]
            ins = self._inside(lx, ly)
            self.stats[3] += int((~ins).sum())
            np.add.at(self.visits, (ly[ins], lx[ins]), 1)
            self.mask[ly[ins] >> PATCH_MAG, lx[ins] >> PATCH_MAG] = 1
        hit = d < max_use_range
        hx, hy = p1x[hit], p1y[hit]
        fx, fy = phx[hit].astype(np.float32), phy[hit].astype(np.float32)
        ins = self._inside(hx, hy)
        self.stats[3] += int((~ins).sum())
        self.stats[2] += int(ins.sum())
        for cx_, cy_, ax_, ay_ in zip(hx[ins], hy[ins], fx[ins], fy[ins]):  # float32 sums in beam order
            self.acc_x[cy_, cx_] = np.float32(self.acc_x[cy_, cx_] + ax_)
            self.acc_y[cy_, cx_] = np.float32(self.acc_y[cy_, cx_] + ay_)
            self.n[cy_, cx_] += 1
            self.visits[cy_, cx_] += 1
            self.mask[cy_ >> PATCH_MAG, cx_ >> PATCH_MAG] = 1

    def publish(self, occ_thresh: float) -> np.ndarray:
        """height x width int8: -1 unvisited, 100 when n / visits > occ_thresh, else 0; 0 beyond the storage."""
        g = self.geo
        out = np.zeros((g.height, g.width), np.int8)
        v = self.visits
        with np.errstate(invalid="ignore", divide="ignore"):
            occ = self.n.astype(np.float64) / v.astype(np.float64)
        out[:g.size_y, :g.size_x] = np.where(v == 0, -1, np.where(occ > occ_thresh, 100, 0))
        return out


def node_callback(ranges, angle_min, angle_increment, cfg=None):
    """One callback of lesson4_gmapping_node on a fresh map -> (MapState, published int8)."""
    c = dict(NODE_DEFAULTS, **(cfg or {}))
    st = MapState(Geometry(c["xmin"], c["ymin"], c["xmax"], c["ymax"], c["delta"]))
    cos_i, sin_i = angle_cache(len(ranges), angle_min, angle_increment)
    st.integrate(ranges, None, cos_i, sin_i, c["max_range"], c["max_use_range"])
    return st, st.publish(c["occ_thresh"])


def pack_counters(prefix: str, visits, n, acc_x, acc_y) -> dict:
    """Counter planes as small fixture arrays: a bitmap of visited cells, their visits (uint16), and the hit cells
    (n > 0) with n and the raw float32 bits of acc."""
    v = np.asarray(visits).reshape(-1)
    assert v.max(initial=0) < 65536
    hit = np.flatnonzero(np.asarray(n).reshape(-1))
    return {prefix + "visited": np.packbits(v > 0), prefix + "visits": v[v > 0].astype(np.uint16),
            prefix + "hit_cells": hit.astype(np.int32), prefix + "n": np.asarray(n).reshape(-1)[hit].astype(np.int32),
            prefix + "acc_x_bits": np.asarray(acc_x, np.float32).reshape(-1)[hit].view(np.uint32),
            prefix + "acc_y_bits": np.asarray(acc_y, np.float32).reshape(-1)[hit].view(np.uint32)}


def unpack_counters(d, prefix: str, shape):
    """-> visits, n (int32), acc_x, acc_y (float32), each of `shape`."""
    cells = int(np.prod(shape))
    visited = np.unpackbits(d[prefix + "visited"])[:cells].astype(bool)
    visits = np.zeros(cells, np.int32)
    visits[visited] = d[prefix + "visits"]
    n = np.zeros(cells, np.int32)
    ax = np.zeros(cells, np.uint32)
    ay = np.zeros(cells, np.uint32)
    h = d[prefix + "hit_cells"]
    n[h] = d[prefix + "n"]
    ax[h] = d[prefix + "acc_x_bits"]
    ay[h] = d[prefix + "acc_y_bits"]
    return (visits.reshape(shape), n.reshape(shape), ax.view(np.float32).reshape(shape), ay.view(np.float32).reshape(shape))
