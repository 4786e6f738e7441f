"""Directed scenarios for the Hector log-odds map update (csrc/logodds_map.hip: k_logodds_pipe_ml, k_logodds_mark,
k_logodds_apply and the four k_lo_batch_* kernels behind updateByScans): one-beam sweeps over every octant on a non-square
map whose sides are no multiple of the 8 x 8-cell tile, rays from the rim, every ordered pair and triple of short beams,
beam counts around every switch of kernel form, maps 32768 and 70001 cells long, rays long and steep enough for
k_lo_batch_rays' float quotient to be wrong, end points an ulp from a cell border, the demo variant's rounding ties, an odd
pyramid and non-finite points in batches.

Pure numpy; the oracle (oracle.pyoracle) and the device API are handed in by the caller: tests/test_logodds_cases_oracle.py
checks on the CPU that every scenario is what it claims, tests/test_logodds_edges_gpu.py runs the same scenarios through
every route of the device path.  Everything is seeded.

A scenario is a list of scans (points [n, 2] float32 in level-0 cells, origo, world pose) on one map.  ROUTES are the ways
the library can be fed such a list; stepped_cells() is a third statement of the traversal next to the oracle's C and the
kernels' closed form: the reference's loop (H/map/OccGridMapBase.h:240-299) written down cell by cell."""
import ctypes
import ctypes.util
import functools
import math
from typing import NamedTuple, Optional

import numpy as np

F32 = np.float32
MB = 1 << 20
ROUTES = ("single_pipe", "single_two_kernels", "batch_plane", "batch_windows", "batch_dev_hint", "batch_dev_whole")
SINGLE, BATCHED = ROUTES[:2], ROUTES[2:]
CALL_SIZES = (64, 1, 63, 65, 130)   # scans per batched call, cycled: ragged, below / at / above the 64-scan group
CHECKPOINT = 2000                   # scans between two comparisons on the routes that may read in between
MAX_POINTS = 65536                  # kMaxBeams
TILE = 8


class MapSpec(NamedTuple):
    sx: int
    sy: int
    cell: float
    offset: tuple
    levels: int = 1


class Scenario(NamedTuple):
    name: str
    map: MapSpec
    scans: list                     # [(points [n, 2] float32, origo (2,) float32, pose (3,) float32)]
    reach: np.ndarray               # [S] cells: no finite point of scan k lies farther from its origo
    routes: tuple
    calls: Optional[tuple] = None   # scans per batched call; None: CALL_SIZES cycled
    notes: Optional[dict] = None    # what the CPU test needs to hold the scenario to its claim


def rep_offset(sx, sy, cell):
    """MapRepMultiMap's mid offset in its own float32 arithmetic (H/slam_main/MapRepMultiMap.h:62-66)"""
    return float(F32(cell) * F32(sx) * F32(0.5)), float(F32(cell) * F32(sy) * F32(0.5))


def level_dims(m):
    return [(m.sx >> i, m.sy >> i) for i in range(m.levels)]


def plane_bytes(sx, sy):
    """one scan's whole-map window: 64 bytes per 8 x 8-cell tile"""
    return ((sx + TILE - 1) // TILE) * ((sy + TILE - 1) // TILE) * 64


def host_measures_reach(m, budget=MB):
    """lslam_map_update_batch measures the scans' reach -- and so plans windows and rounds -- only where 64 whole-map
    windows exceed the budget; on a smaller map every window is the map and a group of 64 scans is one round."""
    return plane_bytes(m.sx, m.sy) * 64 > budget


def host_reach(pts, origo):
    """the reach lslam_map_update_batch measures for a scan, in its float32 arithmetic; non-finite: unbounded"""
    if len(pts) == 0:
        return 1.0
    d = pts.astype(F32) - np.asarray(origo, F32)
    with np.errstate(all="ignore"):
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if not (np.isfinite(d2).all() and (d2 < F32(1e18)).all()):
        return 2e9
    return float(np.sqrt(d2.max(), dtype=F32) * F32(1.0001) + F32(1.0))


def stated_reach(pts, origo):
    fin = pts[np.isfinite(pts).all(axis=1) & (np.abs(pts) < 1e6).all(axis=1)].astype(np.float64)
    if len(fin) == 0:
        return 1
    return int(math.ceil(np.hypot(fin[:, 0] - float(origo[0]), fin[:, 1] - float(origo[1])).max())) + 1


def call_cuts(sc):
    """-> boundaries [0, ..., S] of the batched calls"""
    S, cuts, k = len(sc.scans), [0], 0
    sizes = sc.calls if sc.calls is not None else CALL_SIZES
    while cuts[-1] < S:
        cuts.append(min(S, cuts[-1] + sizes[k % len(sizes)]))
        k += 1
    return cuts


def checkpoints(sc):
    """-> scan counts at which a route may compare: the first call boundary at or after every CHECKPOINT scans, and the end"""
    out, want = [], CHECKPOINT
    for c in call_cuts(sc)[1:]:
        if c >= want:
            out.append(c)
            want = c + CHECKPOINT
    if not out or out[-1] != len(sc.scans):
        out.append(len(sc.scans))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the third statement
# ---------------------------------------------------------------------------------------------------------------------------
def stepped_cells(x0, y0, x1, y1):
    """Cells bresenham2D marks free on the way from (x0, y0) to (x1, y1), in order, end cell excluded
    (H/map/OccGridMapBase.h:240-299): the error term starts at abs_da / 2, takes abs_db per major step and a minor step
    whenever it reaches abs_da; util::sign(0) is -1."""
    dx, dy = x1 - x0, y1 - y0
    sgx, sgy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    adx, ady = abs(dx), abs(dy)
    if adx >= ady:
        abs_da, abs_db, step_a, step_b = adx, ady, (sgx, 0), (0, sgy)
    else:
        abs_da, abs_db, step_a, step_b = ady, adx, (0, sgy), (sgx, 0)
    if abs_da == 0:
        return []  # begin == end: updateByScan skips the beam (:155)
    x, y, err = x0, y0, abs_da // 2
    out = [(x, y)]
    for _ in range(abs_da - 1):
        x, y = x + step_a[0], y + step_a[1]
        err += abs_db
        if err >= abs_da:
            x, y = x + step_b[0], y + step_b[1]
            err -= abs_da
        out.append((x, y))
    return out


def estimate_q(abs_da, abs_db):
    """k_lo_batch_rays' quotient q(c) = (abs_da / 2 + c * abs_db) / abs_da for c = 0 .. abs_da - 1 the way the kernel gets it:
    a float32 estimate, then four corrections by one -> (estimate, corrected, exact)"""
    c = np.arange(abs_da, dtype=np.int64)
    num = abs_da // 2 + c * abs_db
    assert num.max() < 2 ** 31
    rcp = F32(1.0) / F32(abs_da)
    q0 = (num.astype(F32) * rcp).astype(np.int64)
    q, rem = q0.copy(), num - q0 * abs_da
    for _ in range(2):
        low = rem < 0
        q[low] -= 1
        rem[low] += abs_da
    for _ in range(2):
        high = rem >= abs_da
        q[high] += 1
        rem[high] -= abs_da
    return q0, q, num // abs_da


# ---------------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------------
ODD = MapSpec(149, 147, 1.0, (0.0, 0.0))        # 18 full tiles + 5 cells wide, 18 full tiles + 3 cells high
ZERO2 = np.zeros(2, F32)


def _scan(pts, origo, pose):
    return (np.ascontiguousarray(pts, dtype=F32).reshape(-1, 2), np.asarray(origo, F32).copy(), np.asarray(pose, F32).copy())


def _finish(name, m, scans, routes, calls=None, notes=None):
    reach = np.array([stated_reach(p, o) for p, o, _ in scans], np.int64)
    return Scenario(name, m, scans, reach, tuple(routes), calls, notes)


def _box(r):
    """every offset (dx, dy) of the box |d| <= r, row by row, (0, 0) included"""
    v = np.arange(-r, r + 1)
    return np.stack(np.meshgrid(v, v, indexing="xy"), axis=-1).reshape(-1, 2)


def _unit_scans(start, offsets_per_scan):
    """cell length 1, offset 0, heading 0: the map coordinates of a point are pose + point, exactly"""
    pose = (float(start[0]), float(start[1]), 0.0)
    return [_scan(np.asarray(o, F32), ZERO2, pose) for o in offsets_per_scan]


def sweep(radius=70):
    scans, begins, offsets = [], [], []
    for start, r in (((74, 73), radius), ((71, 72), 9), ((77, 70), 9)):
        off = _box(r)
        off = off[(off != 0).any(axis=1)]
        scans += _unit_scans(start, off[:, None, :])
        begins += [start] * len(off)
        offsets.append(off)
    return _finish("sweep", ODD, scans, ROUTES, notes={"begins": np.array(begins), "offsets": offsets, "starts": 3})


# the four corners and two rim cells, then two starts 8 cells inside the far rim: their rays END on the last column and row
RIM_STARTS = ((0, 0), (148, 0), (0, 146), (148, 146), (74, 0), (0, 73), (140, 73), (74, 138))


def sweep_rim():
    sx, sy = ODD.sx, ODD.sy
    scans, begins, ends = [], [], []
    off = _box(20)
    off = off[(off != 0).any(axis=1)]
    for start in RIM_STARTS:
        scans += _unit_scans(start, off[:, None, :])
        begins += [start] * len(off)
        at = np.asarray(start) + off                # exact map coordinates; (int)(v + 0.5f) truncates toward zero, so
        ends.append(np.where(at < 0, at + 1, at))  # coordinate -1 lands in cell 0 and only -2 and below leave the map
    n_int = len(scans)
    # fractional end points at the truncation edges: (int)(x + 0.5f) truncates TOWARD ZERO, so column 0 takes the map
    # coordinates (-1.5, 0.5) and is 1.5 cells wide, and sx - 0.5 is the first coordinate beyond the last column
    fractions = []

    def below(v):
        return float(np.nextafter(F32(v), F32(-np.inf)))

    for axis, size, start in ((0, sx, (0, 73)), (1, sy, (74, 0))):
        for coord, cell in ((-1.6, None), (-1.4, 0), (-0.6, 0), (-0.4, 0), (size - 0.5, None), (below(size - 0.5), size - 1)):
            p = [0.0, 0.0]
            p[axis] = coord - start[axis]       # start[axis] is 0: the point IS the map coordinate
            p[1 - axis] = 7.0
            want = None
            if cell is not None:
                want = [0, 0]
                want[axis], want[1 - axis] = cell, start[1 - axis] + 7
            fractions.append({"scan": len(scans), "axis": axis, "coord": coord, "cell": None if want is None else tuple(want)})
            scans += _unit_scans(start, [[p]])
            begins.append(start)
    # a begin cell put at -0.7 by the pose: (int)(-0.7f + 0.5f) = 0, the cell is in the map
    fan = np.array([[10.7, 0.0], [5.7, 5.0], [0.7, -20.0], [30.7, 9.0], [0.7, 40.0], [-3.0, 2.0]], F32)
    inside = {"scan": len(scans), "begin": (0, 73)}
    scans.append(_scan(fan, ZERO2, (-0.7, 73.0, 0.0)))
    begins.append((0, 73))
    # begin cells outside the map: every beam is dropped
    outside = []
    for pose, b in (((-1.7, 73.0, 0.0), (-1, 73)), ((149.0, 73.0, 0.0), (149, 73)), ((74.0, 146.6, 0.0), (74, 147))):
        outside.append(len(scans))
        scans.append(_scan(fan + F32(3.0), ZERO2, pose))
        begins.append(b)
    return _finish("sweep_rim", ODD, scans, ROUTES,
                   notes={"begins": np.array(begins), "ends": np.concatenate(ends), "n_int": n_int, "fractions": fractions,
                          "inside": inside, "outside": outside})


SMALL = MapSpec(13, 12, 1.0, (0.0, 0.0))
SMALL_START = (6, 5)


def pairs():
    off = _box(5)
    idx = np.stack(np.meshgrid(np.arange(len(off)), np.arange(len(off)), indexing="ij"), axis=-1).reshape(-1, 2)
    return _finish("pairs", SMALL, _unit_scans(SMALL_START, off[idx]), ROUTES, notes={"offsets": off[idx]})


def triples():
    off = _box(2)
    n = len(off)
    idx = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3)
    return _finish("triples", SMALL, _unit_scans(SMALL_START, off[idx]), ROUTES, notes={"offsets": off[idx]})


BEAM_COUNTS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1081, 2048, 2049, 4096, 4097, 9000, 65536)
FAN_MAP = MapSpec(93, 77, 0.05, (1.3, 2.1))
FAN_ORIGO = (0.3, -0.2)


def _fan(rng, n, half=60.0):
    return rng.uniform(-half, half, (n, 2)).astype(F32)


def _fan_pose(rng, centre, spread):
    return (centre[0] + rng.uniform(-spread, spread), centre[1] + rng.uniform(-spread, spread), rng.uniform(-math.pi, math.pi))


def beam_counts(counts=BEAM_COUNTS):
    """every count once as a call of its own, once in the middle of a call of five whose other scans have one point"""
    rng = np.random.default_rng(505)
    scans, calls, big = [], [], []
    for n in counts:
        big.append(len(scans))
        scans.append(_scan(_fan(rng, n), FAN_ORIGO, _fan_pose(rng, (1.0, -0.3), 0.4)))
        calls.append(1)
        for k in range(5):
            if k == 2:
                big.append(len(scans))
            scans.append(_scan(_fan(rng, n if k == 2 else 1), FAN_ORIGO, _fan_pose(rng, (1.0, -0.3), 0.4)))
        calls.append(5)
    return _finish("beam_counts", FAN_MAP, scans, ROUTES, calls=tuple(calls), notes={"big": big, "counts": counts})


THIN_LENGTHS = (63, 64, 65, 255, 256, 257, 511, 512, 513, 32766, 32767)
LONG_LENGTHS = (65535, 65536, 65537, 69998)
MINORS = (0, 1, -1, 2, -2)


def long_thin(long_side, axis):
    """a map long_side x 5 (axis 0) or 5 x long_side (axis 1); rays along the long side from both ends, every length with
    every minor-axis offset; in a scan each length follows a shorter one and precedes one (the predecessor skip of
    logodds_mark_wave looks at beam i - 1, and not at all from abs_da = 65536 on)"""
    lengths = [v for v in THIN_LENGTHS + (LONG_LENGTHS if long_side > 65536 else ()) if v < long_side]
    m = MapSpec(long_side, 5, 1.0, (0.0, 0.0)) if axis == 0 else MapSpec(5, long_side, 1.0, (0.0, 0.0))
    scans = []
    order = lengths + lengths[::-1][1:]          # up, then down again
    for direction in (1, -1):
        start = [2, 2]
        start[axis] = 0 if direction > 0 else long_side - 1
        pose = (float(start[0]), float(start[1]), 0.0)
        for k, minor in enumerate(MINORS):
            beams = []
            for j, length in enumerate(order):
                p = [0.0, 0.0]
                p[axis] = direction * length
                p[1 - axis] = minor if k < 3 else MINORS[(j + k) % len(MINORS)]   # the last two scans mix the minors
                beams.append(p)
            scans.append(_scan(beams, ZERO2, pose))
    routes = ROUTES if long_side <= 32768 else SINGLE
    return _finish(f"long_thin_{'x' if axis == 0 else 'y'}{long_side}", m, scans, routes, notes={"lengths": lengths})


STEEP = MapSpec(8200, 4200, 1.0, (0.0, 0.0))


def long_steep():
    """from (50, 50): abs_da near 8100 and 6000, abs_db near 4100, 4001 and 2^24 / abs_da.  abs_da * abs_db passes 2^24, so
    (float)(abs_da / 2 + c * abs_db) is rounded and the float quotient of k_lo_batch_rays is off by one in places"""
    rays = []
    for da in (8084, 8092, 8088, 8098, 8106, 8100, 6000, 6001):
        # da / 2 and da / 4: every second (fourth) quotient is a whole number, which the float product lands just below
        for db in (da // 2, da // 4, 4100, 4001, (1 << 24) // da, (1 << 24) // da + 1, 4089, 3995):
            rays.append((da, db))
    assert len(rays) == 64
    off = np.array(rays, F32)
    scans = _unit_scans((50, 50), [off[k::4] for k in range(4)])
    return _finish("long_steep", STEEP, scans, ("single_pipe", "batch_plane"), notes={"rays": rays})


# ---------------------------------------------------------------------------------------------------------------------------
# knife edge: end points whose map coordinate + 0.5f is an ulp from an integer
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _libm():
    L = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for f in (L.cosf, L.sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return L


def pose_transform(m, level, pose):
    """-> (c, s, tx, ty, factor) float32 of updateByScan on a level, as the reference evaluates them: cosf / sinf of the C
    library, getMapCoordsPose (H/map/GridMapBase.h:238-242) with mapTworld = Scale * Translate (:278)"""
    cell = F32(m.cell)
    for _ in range(level):
        cell = F32(cell * F32(2.0))
    scale = F32(1.0) / cell
    t_x, t_y = scale * F32(m.offset[0]), scale * F32(m.offset[1])
    p = np.asarray(pose, F32)
    tx = F32(F32(scale * p[0]) + F32(F32(0.0) * p[1])) + t_x
    ty = F32(F32(F32(0.0) * p[0]) + F32(scale * p[1])) + t_y
    c, s = F32(_libm().cosf(float(p[2]))), F32(_libm().sinf(float(p[2])))
    return c, s, F32(tx), F32(ty), F32(0.5 ** level)


def _r32(v):
    return np.asarray(v, np.float64).astype(F32)


def _d(v):
    return np.asarray(v, np.float64)


def end_coord(tf, axis, px, py, how="ref"):
    """map coordinate + 0.5f of points (px, py) (float32 arrays) along `axis` on a level with transform tf.  "ref": the
    reference's order, float32 operation by operation (H/map/OccGridMapBase.h:145-149).  The others are what a compiler or
    a rewrite could make of it, each float32 rounding emulated in float64: "fma_first" fma(u, px, v * py), "fma_second"
    fma(v, py, u * px), "fold_half" + (t + 0.5f) in one addition, "factor_late" (u * px) * factor for u * (px * factor)."""
    c, s, tx, ty, factor = tf
    u, v, t = (c, F32(-s), tx) if axis == 0 else (s, c, ty)
    qx, qy = _r32(_d(px) * _d(factor)), _r32(_d(py) * _d(factor))
    if how == "factor_late":
        a, b = _r32(_d(_r32(_d(u) * _d(px))) * _d(factor)), _r32(_d(_r32(_d(v) * _d(py))) * _d(factor))
    else:
        a, b = _r32(_d(u) * _d(qx)), _r32(_d(v) * _d(qy))
    if how == "fma_first":
        e = _r32(_d(u) * _d(qx) + _d(b))
    elif how == "fma_second":
        e = _r32(_d(v) * _d(qy) + _d(a))
    else:
        e = _r32(_d(a) + _d(b))
    if how == "fold_half":
        return _r32(_d(e) + _d(_r32(_d(t) + 0.5)))
    return _r32(_d(_r32(_d(e) + _d(t))) + 0.5)


ALTERNATIVES = ("fma_first", "fma_second", "fold_half")


def _knife_search(m, level, pose, per_axis, rng):
    """Targeted search: for a cell border K along an axis and a place along the other, solve for the point whose map
    coordinate is K - 0.5, then try the floats next to it; a candidate is kept when its coordinate + 0.5f is within two ulps
    of K and the alternative evaluation whose turn it is puts it into the other cell."""
    tf = pose_transform(m, level, pose)
    c, s, tx, ty, factor = (float(v) for v in tf)
    sx, sy = m.sx >> level, m.sy >> level
    found, turn = [], 0
    for axis in (0, 1):
        got = 0
        for _ in range(20000):
            if got == per_axis:
                break
            size, other = (sx, sy) if axis == 0 else (sy, sx)
            how = ALTERNATIVES[turn % len(ALTERNATIVES)]
            if how == "fold_half":
                # (e + t) + 0.5f and e + (t + 0.5f) differ only where t + 0.5f is itself rounded, i.e. changes binade: the
                # poses put t just below a power of two B, and the border K lies in [B, 2B), where an ulp is what t + 0.5f lost
                B = 2 ** math.ceil(math.log2((tx, ty)[axis]))
                K = int(rng.integers(B + 1, min(2 * B - 1, size - 2) + 1))
            else:
                K = int(rng.integers(2, size - 1))
            mc = [0.0, 0.0]
            mc[axis], mc[1 - axis] = K - 0.5, rng.uniform(1.5, other - 2.5)
            ex, ey = mc[0] - tx, mc[1] - ty
            px, py = (c * ex + s * ey) / factor, (-s * ex + c * ey) / factor   # the rotation undone
            col = 0 if (abs(c) >= abs(s)) == (axis == 0) else 1                 # the coordinate that moves this axis most
            gain = max(abs(c), abs(s)) * factor                                 # d(coordinate) / d(that point coordinate)
            delta = float(np.spacing(F32(K))) / (4.0 * gain)                    # a quarter ulp of the result per candidate
            cand = np.repeat(np.array([[px, py]], np.float64), 65, axis=0)
            cand[:, col] += np.arange(-32, 33) * delta
            cand = cand.astype(F32)
            ref = end_coord(tf, axis, cand[:, 0], cand[:, 1])
            near = np.abs(_d(ref) - K) <= 2.0 * float(np.spacing(F32(K)))
            alt = end_coord(tf, axis, cand[:, 0], cand[:, 1], how)
            hit = np.flatnonzero(near & (ref.astype(np.int64) != alt.astype(np.int64)))
            if len(hit):
                found.append(cand[hit[0]])
                got += 1
                turn += 1
        assert got == per_axis, (level, axis, got)
    return np.array(found, F32)


KNIFE_L0 = MapSpec(149, 147, 0.05, (1.9, 2.3))
KNIFE_L1 = MapSpec(149, 147, 0.05, rep_offset(149, 147, 0.05), 2)
# (t_x, t_y, heading): where the pose lands in level coordinates, each just below a power of two (see _knife_search)
KNIFE_AT = {0: ((63.7, 63.8, 0.3), (63.6, 127.7, -1.1), (127.6, 63.9, 2.4), (127.8, 127.55, -2.9)),
            1: ((31.7, 31.6, 0.3), (31.8, 63.7, -1.1), (63.6, 31.9, 2.4), (63.9, 63.55, -2.9))}


@functools.lru_cache(maxsize=None)
def knife_edge(level):
    """128 points on four rotated poses; level 0 on a one-level map, level 1 on a two-level map (whose level 0 takes the
    same points)"""
    rng = np.random.default_rng(808 + level)
    m = KNIFE_L0 if level == 0 else KNIFE_L1
    scale = (1.0 / m.cell) / 2 ** level
    scans = []
    for at_x, at_y, heading in KNIFE_AT[level]:
        pose = [F32(at_x / scale - m.offset[0]), F32(at_y / scale - m.offset[1]), F32(heading)]
        for axis in (0, 1):  # ... and on an ODD multiple of its ulp, so that t + 0.5f is a tie and is rounded
            while int(round(float(pose_transform(m, level, pose)[2 + axis]) / float(np.spacing(F32((at_x, at_y)[axis]))))) % 2 == 0:
                pose[axis] = np.nextafter(pose[axis], F32(np.inf))
        pose = tuple(float(v) for v in pose)
        tf = pose_transform(m, level, pose)
        assert int(math.log2(float(tf[2]))) == int(math.log2(at_x)) and int(math.log2(float(tf[3]))) == int(math.log2(at_y))
        pts = _knife_search(m, level, pose, 16, rng)
        scans.append(_scan(pts, ZERO2, pose))
    # all four scans once more in one container each, reversed: the same borders met in the other beam order
    scans += [_scan(p[::-1], o, q) for p, o, q in scans]
    return _finish(f"knife_edge_l{level}", m, scans, ROUTES, notes={"level": level, "n_unique": 4})


JUST_ONCE = MapSpec(41, 37, 0.05, (0.0, 0.0))
JUST_ONCE_BEGIN = (20.0, 18.0)


def just_once_points():
    """k * 0.05, (k + 0.5) * 0.05 and the float neighbours of both for k = -20 .. 20 on each axis (round(p / 0.05) in double:
    ties go away from zero, and a neighbour of a tie goes either way), then NaN, +-Inf and 3e9 -> four containers"""
    k = np.arange(-20, 21).astype(np.float64)
    base = np.concatenate([k * 0.05, (k + 0.5) * 0.05]).astype(F32)
    vals = np.concatenate([base, np.nextafter(base, F32(np.inf)), np.nextafter(base, F32(-np.inf))])
    on_x = np.stack([vals, np.full_like(vals, 0.1)], axis=1)
    on_y = np.stack([np.full_like(vals, -0.15), vals], axis=1)
    rng = np.random.default_rng(909)
    both = np.stack([rng.permutation(vals), rng.permutation(vals)], axis=1)
    nan, inf = F32("nan"), F32("inf")
    odd = np.array([[0.5, 0.0], [nan, 0.1], [0.1, nan], [inf, 0.0], [0.0, -inf], [3e9, 0.0], [-3e9, 0.2], [nan, nan], [0.0, 0.5],
                    [-inf, inf], [0.3, -0.3]], F32)
    return [on_x.astype(F32), on_y.astype(F32), both.astype(F32), odd]


PYRAMID = MapSpec(149, 147, 0.05, rep_offset(149, 147, 0.05), 3)


def pyramid_odd():
    rng = np.random.default_rng(1010)
    centre = (0.0, 0.0)  # the offset is the map's middle
    scans = [_scan(_fan(rng, 300), FAN_ORIGO, _fan_pose(rng, centre, 0.5)) for _ in range(12)]
    return _finish("pyramid_odd", PYRAMID, scans, ROUTES, calls=(5, 1, 6))


NON_FINITE_MAP = MapSpec(200, 200, 0.05, (5.0, 5.0))


def non_finite_points():
    nan, inf = F32("nan"), F32("inf")
    return np.array([[40, 0], [nan, 3], [3, nan], [inf, 0], [0, -inf], [3e9, 0], [-3e9, 1], [1e20, 1e20], [0, 30], [nan, nan]], F32)


def non_finite_batched():
    rng = np.random.default_rng(1111)
    bad = non_finite_points()
    scans = []
    for k in range(40):
        pts = _fan(rng, 30, 80.0)
        if k % 4 != 3:   # three scans in four carry the list, cut in at a moving place
            at = int(rng.integers(0, len(pts) + 1))
            pts = np.concatenate([pts[:at], bad, pts[at:]])
        scans.append(_scan(pts, (0.0, 0.0), _fan_pose(rng, (0.0, 0.0), 1.0)))
    return _finish("non_finite_batched", NON_FINITE_MAP, scans, BATCHED, calls=(40,))


_BUILDERS = {
    "sweep": sweep, "sweep_rim": sweep_rim, "pairs": pairs, "triples": triples, "beam_counts": beam_counts,
    "long_thin_x32768": lambda: long_thin(32768, 0), "long_thin_y32768": lambda: long_thin(32768, 1),
    "long_thin_x70001": lambda: long_thin(70001, 0), "long_steep": long_steep,
    "knife_edge_l0": lambda: knife_edge(0), "knife_edge_l1": lambda: knife_edge(1),
    "pyramid_odd": pyramid_odd, "non_finite_batched": non_finite_batched,
}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def scenario(name):
    return _BUILDERS[name]()


ROUTES_OF = {
    "long_thin_x70001": SINGLE, "long_steep": ("single_pipe", "batch_plane"), "non_finite_batched": BATCHED,
}
ROUTE_CASES = tuple((n, r) for n in NAMES for r in ROUTES_OF.get(n, ROUTES))


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's side of a scenario
# ---------------------------------------------------------------------------------------------------------------------------
def make_oracle(oracle_lib, m, ref=False):
    if m.levels == 1:
        return (oracle_lib.RefHector if ref else oracle_lib.PortHector)(m.sx, m.sy, m.cell, m.offset)
    return (oracle_lib.RefHectorRep if ref else oracle_lib.PortHectorRep)(m.cell, m.sx, m.sy, m.levels)


def oracle_feed(o, m, scan):
    """one scan as EVERY route feeds it: on a pyramid the scan is matched first, so that the levels above 0 take it too
    (MapRepMultiMap::updateByScan feeds them from the container matchData cached, H/slam_main/MapRepMultiMap.h:174-191)"""
    pts, origo, pose = scan
    if m.levels > 1:
        o.matchData(pts, pose, origo)
    o.updateByScan(pts, origo, pose)


def oracle_planes(o, m):
    if m.levels == 1:
        return [o.logodds()], [o.occupancy_i8()]
    return [o.logodds(i) for i in range(m.levels)], [o.occupancy_i8(i) for i in range(m.levels)]


_EXPECTED = {}


def expected(oracle_lib, name):
    """-> {scans fed: (log-odds planes per level, occupancy per level)} at every checkpoint of the scenario; computed once"""
    if name not in _EXPECTED:
        sc = scenario(name)
        o = make_oracle(oracle_lib, sc.map)
        out, at = {}, set(checkpoints(sc))
        for k, scan in enumerate(sc.scans):
            oracle_feed(o, sc.map, scan)
            if k + 1 in at:
                out[k + 1] = oracle_planes(o, sc.map)
        _EXPECTED[name] = out
    return _EXPECTED[name]
