"""Scenarios for the Gauss-Newton matcher (MapRepMultiMap::matchData) away from the 1024^2 / 3-level / centred set-up every
other matcher test uses: non-square and odd-sized maps, offsets that leave hundreds of points outside the map, 1 and 5
levels, zero Hessians, a written border band probed at exactly 0.0 / -0.0 / lim / nextafter(lim), and the +-0.2 rad clamp of
the angular step -- and the routing of one (container, start pose) through every device form of the matcher.

Pure numpy plus the project's synth module; the oracle (oracle.pyoracle) and the device API are handed in by the caller, so
tests/test_gn_edges_oracle.py checks every scenario's preconditions on the CPU alone and tests/test_gn_edges_gpu.py runs the
same scenarios through the kernels."""
import functools
from typing import NamedTuple

import numpy as np

from lslam_amd import synth

f32 = np.float32
CELL = 0.05
HINT = np.array([0.06, -0.05, 0.02])  # start pose = truth + HINT, as in test_gauss_newton_kernel_variants_agree
N_LDS, N_MEM = 2000, 7200             # container lengths of k_gn_match_fast's two forms at 512 threads (1537..7168, > 7168)
ORDERED_MAX = 4266                    # the ordered kernel refuses longer containers (nine terms per point in LDS)
# pose 1e-4 of the oracle (the contract), H 1e-2 (parallel) / 1e-3 (ordered) of max(1, |H|max), parallel against ordered 5e-5
POSE_TOL, H_TOL_PARALLEL, H_TOL_ORDERED, PAR_VS_ORDERED_TOL = 1e-4, 1e-2, 1e-3, 5e-5
CONVERGES, STABLE = 0.03, 1e-5


class Geometry(NamedTuple):
    name: str
    sx: int
    sy: int
    levels: int
    off: tuple
    heading: float
    sides: tuple  # the sides of level 0 the query must leave at the true pose: of "x_lo", "x_hi", "y_lo", "y_hi"


GEOMETRIES = [
    Geometry("640x384-centre", 640, 384, 3, (16.0, 9.6), 0.0, ("x_hi", "y_lo", "y_hi")),
    Geometry("640x384-corner", 640, 384, 3, (4.0, 3.0), 0.0, ("x_lo", "y_lo")),
    Geometry("384x640-heading", 384, 640, 3, (3.0, 28.0), 0.5, ("x_lo", "x_hi", "y_hi")),
    Geometry("333x201-odd", 333, 201, 3, (8.0, 5.0), 0.0, ("x_hi", "y_lo", "y_hi")),
    Geometry("256x192", 256, 192, 3, (6.4, 4.8), 0.0, ("x_hi", "y_lo", "y_hi")),
    Geometry("400x400-1level", 400, 400, 1, (10.0, 10.0), 0.0, ("x_hi", "y_lo", "y_hi")),
    Geometry("400x400-5levels", 400, 400, 5, (10.0, 10.0), 0.0, ("x_hi", "y_lo", "y_hi")),
]
GEOMETRY_IDS = [g.name for g in GEOMETRIES]
ZERO_GEOMETRY = GEOMETRIES[4]  # the zero-Hessian cases live on the 256 x 192 map


def level_list(sx, sy, levels, cell=CELL):
    """[(sx, sy, cell)] as lslam_map_create builds them: sizes halve by integer division, cells double, and the list ends at
    a non-positive size."""
    out = []
    cl = f32(cell)
    for _ in range(levels):
        if sx <= 0 or sy <= 0:
            break
        out.append((sx, sy, float(cl)))
        sx //= 2
        sy //= 2
        cl = f32(cl * f32(2.0))
    return out


def map_xy(size_cell, off, pts, pose, factor=1.0):
    """Map coordinates of a container's points at a WORLD pose on one level, in the reference's float32 operation order
    (getMapCoordsPose, then getCompleteHessianDerivs' transform) -> (cx, cy, lim_x, lim_y)."""
    sx, sy, cell = size_cell
    sc = f32(1.0) / f32(cell)
    tx, ty = sc * f32(off[0]), sc * f32(off[1])
    p = np.asarray(pose, f32)
    e0 = (sc * p[0] + f32(0.0) * p[1]) + tx
    e1 = (f32(0.0) * p[0] + sc * p[1]) + ty
    c, s = f32(np.cos(p[2], dtype=f32)), f32(np.sin(p[2], dtype=f32))
    q = np.asarray(pts, f32).reshape(-1, 2) * f32(factor)
    cx = (c * q[:, 0] + (-s) * q[:, 1]) + e0
    cy = (s * q[:, 0] + c * q[:, 1]) + e1
    return cx, cy, f32(sx) - f32(2.0), f32(sy) - f32(2.0)


def outside(size_cell, off, pts, pose, factor=1.0):
    """-> {"x_lo": mask, ...} of pointOutOfMapBounds' four comparisons, and their union under "any"."""
    cx, cy, lx, ly = map_xy(size_cell, off, pts, pose, factor)
    m = {"x_lo": cx < 0, "x_hi": cx > lx, "y_lo": cy < 0, "y_hi": cy > ly}
    m["any"] = m["x_lo"] | m["x_hi"] | m["y_lo"] | m["y_hi"]
    return m


def replicate(base, n, rng):
    """A long container as test_gauss_newton_kernel_variants_agree makes it: the base scan replicated with 0.05-cell noise."""
    reps = -(-n // len(base))
    return np.concatenate([base + rng.normal(0.0, 0.05, base.shape).astype(f32) for _ in range(reps)])[:n].astype(f32)


class Case(NamedTuple):
    levels: list        # [(sx, sy, cell)]
    off: tuple
    scans: list         # [(points, pose)] the map is built from
    containers: dict    # name -> points [n, 2] float32
    begin: dict         # name -> start pose float32[3]
    truth: object       # float64[3] or None
    ranges: object      # the LaserScan behind containers["resident"] (lslam_map_set_scan), or None


@functools.lru_cache(maxsize=None)
def geometry_case(name):
    """The world of the existing tests; the map built from 6 scans at (0.1 k, 0.05 k, 0.02 k + heading); the query cast anew
    at the third pose, started at truth + HINT.  Containers: the scan itself ("scan"), the same LaserScan through the
    device's own projection ("resident"), the scan replicated to the two long forms ("lds", "mem") and its part close
    enough to the robot to lie inside every level ("near": the ordinary neighbour in a batch; too few points to be held to
    a tolerance, it is held to itself, bit for bit)."""
    g = GEOMETRIES[GEOMETRY_IDS.index(name)]
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=3)
    laser = synth.Laser()
    rng = np.random.default_rng(1)
    poses = [np.array([0.1 * k, 0.05 * k, 0.02 * k + g.heading]) for k in range(6)]
    scans = []
    for p in poses:
        r = synth.cast_scan(world, p, laser, 0.01, 0.0, rng)
        scans.append((synth.hector_points(r, laser, 1.0 / CELL, use_max=20.0), p.astype(f32)))
    truth = poses[2]
    r = synth.cast_scan(world, truth, laser, 0.01, 0.0, rng)
    scan = synth.hector_points(r, laser, 1.0 / CELL, use_max=20.0)
    resident, origo = synth.hector_project(r, laser, 1.0 / CELL)
    assert not origo.any()
    begin = (truth + HINT).astype(f32)
    levels = level_list(g.sx, g.sy, g.levels)
    # the reach (metres) within which a point stays inside every level at the start pose, less a quarter metre
    reach = min(min(begin[a] + g.off[a], (n - 2) * cell - (begin[a] + g.off[a])) for sx, sy, cell in levels for a, n in ((0, sx), (1, sy)))
    conts = {"scan": scan, "resident": resident, "lds": replicate(scan, N_LDS, rng), "mem": replicate(scan, N_MEM, rng),
             "near": scan[np.hypot(scan[:, 0], scan[:, 1]) < (reach - 0.25) / CELL]}
    return Case(levels, g.off, scans, conts, {k: begin for k in conts}, truth, r)


@functools.lru_cache(maxsize=None)
def zero_cases():
    """name -> (built, container, start pose): Hessians that are exactly zero.  `built` False: an untouched map (every cell
    0.5, every gradient 0); True: ZERO_GEOMETRY's map and a start pose that puts every point outside every level.  Lengths
    for the register, LDS and memory forms."""
    rng = np.random.default_rng(5)
    scan = geometry_case(ZERO_GEOMETRY.name).containers["scan"]
    far = np.array([100.0, 50.0, 0.2], f32)
    start = np.array([0.3337, -0.2221, 0.7], f32)
    out = {}
    for n, tag in ((500, "scan"), (N_LDS, "lds"), (N_MEM, "mem")):
        out["untouched-" + tag] = (False, rng.uniform(-100.0, 100.0, (n, 2)).astype(f32), start)
        out["outside-" + tag] = (True, scan if tag == "scan" else replicate(scan, n, rng), far)
    return out


BAND_SX, BAND_SY = 200, 120
BAND_OFF = (-0.0, -0.0)


@functools.lru_cache(maxsize=None)
def band_case():
    """A 200 x 120 single-level map whose border band is written, probed by a container that straddles all four edges.

    The offset is (-0.0, -0.0) and the start pose (-0.0, -0.0, +0.0): map coordinates are then the container's own
    coordinates (cos = 1, sin = +0, the pose's map image is (-0.0, -0.0)), so a point's coordinate IS what the in-map test
    sees, and -0.0 can be reached at all -- with any non-zero map translation x + t is never -0.0.  The map is built from the
    centre: walls three cells thick, one to three cells inside each edge, six updates.  The container is
    the four edges of the in-map region (0 and lim) sampled with +-3 cells of jitter across them, shifted by (0.3, -0.2) cells for the matcher to undo, plus points
    at exactly 0.0, -0.0, lim and nextafter(lim, +inf) in x and in y."""
    rng = np.random.default_rng(9)
    sx, sy = BAND_SX, BAND_SY
    centre = np.array([sx * CELL * 0.5, sy * CELL * 0.5, 0.0], f32)  # (5, 3) m = cell (100, 60)
    cxy = np.array([sx / 2, sy / 2])
    ring = []
    for d in (1, 2, 3):  # walls d cells inside each edge; every beam ends within 3 cells of an edge
        xs, ys = np.arange(d, sx - d), np.arange(d, sy - d)
        ring += [np.stack([xs, np.full_like(xs, d)], 1), np.stack([xs, np.full_like(xs, sy - 1 - d)], 1),
                 np.stack([np.full_like(ys, d), ys], 1), np.stack([np.full_like(ys, sx - 1 - d), ys], 1)]
    ring = np.concatenate(ring).astype(np.float64)
    scans = []
    for _ in range(6):
        ends = ring + rng.uniform(-0.3, 0.3, ring.shape)
        scans.append(((ends - cxy).astype(f32), centre))
    lim_x, lim_y = f32(sx - 2), f32(sy - 2)
    n_side = 140
    t = rng.uniform(0.0, 1.0, (4, n_side))
    j = rng.uniform(-3.0, 3.0, (4, n_side))
    walls = np.concatenate([
        np.stack([t[0] * (sx - 1), j[0]], 1), np.stack([t[1] * (sx - 1), float(lim_y) + j[1]], 1),
        np.stack([j[2], t[2] * (sy - 1)], 1), np.stack([float(lim_x) + j[3], t[3] * (sy - 1)], 1)])
    walls = (walls + np.array([0.3, -0.2])).astype(f32)
    up_x, up_y = np.nextafter(lim_x, f32(np.inf)), np.nextafter(lim_y, f32(np.inf))
    m = 24  # points per exact value: enough that misplacing one kind moves the result by far more than the tolerance
    ys, xs = rng.uniform(5.0, sy - 7.0, (4, m)), rng.uniform(5.0, sx - 7.0, (3, m))
    col = lambda x, y: np.stack([np.full(m, x, f32), y.astype(f32)], 1)
    row = lambda x, y: np.stack([x.astype(f32), np.full(m, y, f32)], 1)
    exact = np.concatenate([
        col(0.0, ys[0]),                    # x = +0.0
        col(-0.0, ys[1]),                   # x = -0.0: 1 * (-0.0) + (-0.0) * y (y > 0) + (-0.0)
        col(lim_x, ys[2]),                  # x = lim: the last in-map value, reads columns sx - 2 and sx - 1
        col(up_x, ys[3]),                   # one ulp beyond: out
        row(xs[0], 0.0),                    # y = +0.0
        np.full((8, 2), -0.0, f32),         # y = -0.0: (+0 * -0.0) + 1 * (-0.0) + (-0.0); x must be -0.0 too and comes out +0.0
        row(xs[1], lim_y), row(xs[2], up_y),
        np.array([[lim_x, lim_y], [0.0, 0.0], [up_x, up_y], [lim_x, up_y], [up_x, lim_y]], f32)]).astype(f32)
    pts = np.concatenate([exact, walls]).astype(f32)
    begin = np.array([-0.0, -0.0, 0.0], f32)
    conts = {"scan": pts, "lds": replicate_keep(pts, len(exact), N_LDS, rng), "mem": replicate_keep(pts, len(exact), N_MEM, rng)}
    return Case(level_list(sx, sy, 1), BAND_OFF, scans, conts, {k: begin for k in conts}, None, None), len(exact)


def replicate_keep(pts, n_exact, n, rng):
    """replicate(), with the first n_exact points of the first copy left exactly as they are."""
    out = replicate(pts, n, rng)
    out[:n_exact] = pts[:n_exact]
    return out


CLAMP_HALF, CLAMP_BEGIN = 8.37, (0.02, -0.02, 0.35)


@functools.lru_cache(maxsize=None)
def clamp_case():
    """The +-0.2 rad clamp of the angular step (ScanMatcher.h:127-131).  A 128^2 map, 3 levels, the robot at its centre in a
    square room of half-width 8.37 cells (0.42 m), drawn six times with +-0.2 cells of jitter; the container is the room's
    wall sampled every quarter cell (268 points), started 0.35 rad and 2 cm off.  The half-width is off the cell raster on
    purpose: with walls ON cell borders every point sits where the interpolated gradient jumps, and the returned Hessian
    differs by percents between two poses 1e-7 apart (seen on the device with a half-width of 8.0).  On the coarsest level the room is two cells
    wide: the lever arm is so short that a one-cell residual asks for more than 0.2 rad, and the first step is clamped.
    Found by a search over room sizes (5..24 cells), levels (1..3), arcs of the room, strides and heading errors
    (0.25..0.6 rad) for cases whose first step is clamped AND whose oracle result does not move under one-ulp changes of the
    start pose; dense scans of the arena never reach the clamp (first steps of ~0.015 rad)."""
    rng = np.random.default_rng(2)
    room = _room_points(CLAMP_HALF, 0.25)
    centre = np.zeros(3, f32)
    scans = [((room + rng.uniform(-0.2, 0.2, room.shape)).astype(f32), centre) for _ in range(6)]
    pts = room.astype(f32)
    return Case(level_list(128, 128, 3), (3.2, 3.2), scans, {"scan": pts}, {"scan": np.array(CLAMP_BEGIN, f32)}, np.zeros(3), None)


def _room_points(half, step):
    """Points (cells, robot at the centre) along the walls of a square room of half-width `half` cells."""
    s = np.arange(-half, half + 1e-9, step)
    return np.concatenate([np.stack([s, np.full_like(s, half)], 1), np.stack([s, np.full_like(s, -half)], 1),
                           np.stack([np.full_like(s, half), s], 1), np.stack([np.full_like(s, -half), s], 1)])


# ---- the oracle side ------------------------------------------------------------------------------------------------------
def oracle_levels(po, case, build=True):
    """PortHector levels of a case, fed its scans: level i takes pts * level_factor(i), like MapRepMultiMap's containers."""
    cpus = [po.PortHector(sx, sy, cell, case.off) for sx, sy, cell in case.levels]
    for c in cpus:
        c.setUpdateOccupiedFactor(0.9)
    if build:
        for pts, pose in case.scans:
            for i, c in enumerate(cpus):
                c.updateByScan(pts if i == 0 else pts * f32(po.PortHector.level_factor(i)), (0.0, 0.0), pose)
    return cpus


def ulp_neighbours(begin):
    """The start pose moved by one float32 ulp in each component, both signs."""
    b = np.asarray(begin, f32)
    out = []
    for k in range(3):
        for toward in (np.inf, -np.inf):
            q = b.copy()
            q[k] = np.nextafter(b[k], f32(toward))
            out.append(q)
    return out


def oracle_shift_under_ulps(po, cpus, pts, begin):
    """max |pose(begin +- 1 ulp) - pose(begin)| of the oracle: what a last-bit difference in a device form may legitimately
    grow into.  The scenarios are held to STABLE = 1e-5, a tenth of the 1e-4 the device forms are held to."""
    p0, _ = po.PortHector.match_data(cpus, pts, begin)
    return max(float(np.abs(po.PortHector.match_data(cpus, pts, q)[0] - p0).max()) for q in ulp_neighbours(begin))


# ---- the device side ------------------------------------------------------------------------------------------------------
# form -> (LSLAM_GN_THREADS at map creation, ordered_sums, admissible container length)
SINGLE_FORMS = {
    "ordered": (512, True, (1, ORDERED_MAX)),
    "reg512": (512, False, (1, 512 * 3)),
    "reg256": (256, False, (1, 256 * 5)),
    "reg1024": (1024, False, (1, 1024 * 2)),
    "fast-lds": (512, False, (512 * 3 + 1, 7168)),
    "fast-mem": (512, False, (7169, 65536)),
}
FORM_CONTAINER = {"ordered": "scan", "reg512": "scan", "reg256": "scan", "reg1024": "scan", "fast-lds": "lds", "fast-mem": "mem"}


class DeviceMaps:
    """One case's map on the device, three times over (LSLAM_GN_THREADS is read at map creation), built from the same scans
    at the same poses as the oracle's levels -- and the way to push one (container, start pose) through every form."""

    def __init__(self, ctx, api, monkeypatch, case, build=True):
        self.case, self.maps = case, {}
        sx, sy, cell = case.levels[0]
        for threads in (512, 256, 1024):
            monkeypatch.setenv("LSLAM_GN_THREADS", str(threads))
            m = api.OccGridMap(ctx, sx, sy, cell, case.off, levels=len(case.levels))
            monkeypatch.delenv("LSLAM_GN_THREADS")
            m.setUpdateOccupiedFactor(0.9)
            if build:
                for pts, pose in case.scans:
                    m.matchData(pose, pts)  # caches the container: updateByScan feeds the levels above 0 from it
                    m.updateByScan(pts, (0.0, 0.0), pose)
            self.maps[threads] = m

    def assert_planes_equal(self, cpus):
        for threads, m in self.maps.items():
            assert m.levels == len(cpus), (threads, m.levels)
            for i, c in enumerate(cpus):
                assert m.size(i) == (c.sx, c.sy), (threads, i, m.size(i))
                assert m.logodds(i).tobytes() == c.logodds().tobytes(), (threads, i)

    def match(self, form, pts, begin):
        """lslam_map_match_data through one of SINGLE_FORMS -> (pose[3], H[3,3])."""
        threads, ordered, (lo, hi) = SINGLE_FORMS[form]
        assert lo <= len(pts) <= hi, (form, len(pts))
        m = self.maps[threads]
        m.set_option("ordered_sums", int(ordered))
        try:
            return m.matchData(begin, pts)
        finally:
            m.set_option("ordered_sums", 0)

    def match_batch(self, entries, ordered):
        """lslam_map_match_batch over [(container, start pose)] -> (poses[B,3], H[B,3,3])."""
        m = self.maps[512]
        m.set_option("ordered_sums", int(ordered))
        try:
            return m.matchBatch(np.stack([b for _, b in entries]), [p for p, _ in entries])
        finally:
            m.set_option("ordered_sums", 0)

    def match_resident(self, api, ranges, begin):
        """lslam_map_set_scan -> lslam_map_match_container -> (the container the device projected, pose, H)."""
        m = self.maps[512]
        n = m.setScan(ranges, api.hector_scan(synth.Laser()))
        pts, origo = m.container()
        assert n == len(pts) and not origo.any()
        pose, H = m.matchContainer(begin)
        return pts, pose, H


def words(pose, H):
    """The 12 result floats as bytes."""
    return np.concatenate([np.asarray(pose, f32).ravel(), np.asarray(H, f32).ravel()]).tobytes()


def diffs(pose, H, pose_ref, H_ref):
    """-> (max |pose - ref|, max |H - ref| / max(1, |ref|max))"""
    return (float(np.abs(np.asarray(pose, np.float64) - pose_ref).max()),
            float(np.abs(np.asarray(H, np.float64) - H_ref).max() / max(1.0, float(np.abs(H_ref).max()))))
