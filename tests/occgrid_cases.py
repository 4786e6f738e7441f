"""Directed scenarios for the Karto hit/pass-counter occupancy grid (csrc/occupancy_grid.hip, occ_trace_beam of
csrc/occgrid_impl.hpp): every ray octant, the axes and diagonals, ray lengths on both sides of the 64-lane stride, clipped and
wholly outside rays, beam counts around the 256-thread and 4-beams-per-block boundaries, every beam class at its limits, the
box reduction with its extremum in a chosen lane and block, exact rounding ties and grids of 0 x 0 and w x 0 cells.

Pure numpy plus the project's synth module; the oracle (oracle.pyoracle) and the device API are handed in by the caller, so
tests/test_occgrid_cases_oracle.py checks every scenario's preconditions on the CPU alone and tests/test_occgrid_edges_gpu.py
runs the same scenarios through the kernels.

trace_line_counters() is a third statement of the same operation, next to the oracle's C and the kernel's closed form: the
reference's stepped TraceLine / AddScan / RayTrace (Karto.h:4680-4745, 5851-5942) written down from what they do -- the error
recurrence cell by cell, the two swaps, the validity test per cell, the extra pass + hit on a valid end point inside the grid."""
import functools
import math
import pathlib
import re
from typing import NamedTuple, Optional

import numpy as np

from lslam_amd import synth

BOX_BIG = 999999999999999999.99999  # BoundingBox2() (Karto.h:2765)
MIN_MARGIN = 1e-6                   # cells: what device sincos and glibc sin / cos may at most disagree by, with room to spare


@functools.lru_cache(maxsize=None)
def k_tol():
    """KT_TOLERANCE as the library spells it (csrc/karto_math.hpp)."""
    import lslam_amd
    text = (pathlib.Path(lslam_amd.__file__).resolve().parent / "csrc" / "karto_math.hpp").read_text()
    return float(re.search(r"constexpr double kTol = ([0-9.eE+-]+);", text).group(1))


class Scenario(NamedTuple):
    name: str
    laser: synth.Laser
    threshold: float
    ranges: np.ndarray              # [S, cols], cols >= the laser's beam count
    poses: np.ndarray               # [S, 3] SENSOR poses
    resolution: float
    box: Optional[np.ndarray]       # forced box (minx, miny, maxx, maxy) of a partial build; None: a whole build
    intent: Optional[tuple] = None  # (start cells [S, 2], end cells [S, 2]) a one-beam scenario is meant to produce
    groups: Optional[tuple] = None  # box_extremum: the scan subsets whose bounds are compared
    min_margin: float = MIN_MARGIN  # 0.0 for the exact-tie scenario only


# ---------------------------------------------------------------------------------------------------------------------------
# the third statement
# ---------------------------------------------------------------------------------------------------------------------------
def kround(v):
    """math::Round (Math.h:87-90): half away from zero."""
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


def num_beams(laser):
    """LaserRangeFinder::Update (Karto.h:4158-4160)"""
    return int(kround((laser.angle_max - laser.angle_min) / laser.angle_increment))


def beam_classes(sc):
    """-> (in_box, traced, end_valid, shortened) [S, n] bool: the comparisons of LocalizedRangeScan::Update (Karto.h:5382)
    and AddScan (Karto.h:5866-5885) on every reading."""
    n = num_beams(sc.laser)
    r = sc.ranges[:, :n]
    with np.errstate(invalid="ignore"):
        in_box = (r >= sc.laser.range_min) & (r <= sc.threshold)
        traced = ~((r <= sc.laser.range_min) | (r >= sc.laser.range_max) | np.isnan(r))
        end_valid = r < (sc.threshold - k_tol())
        shortened = traced & (r >= sc.threshold)
    return in_box, traced, end_valid & traced, shortened


def _points(sc):
    """World end point of every reading (math.cos / math.sin are the C library's, as in the oracle), the point AddScan
    traces to (shortened to the threshold) -> (raw [S, n, 2], traced-to [S, n, 2]); NaN where the reading is."""
    n = num_beams(sc.laser)
    S = len(sc.poses)
    raw = np.full((S, n, 2), np.nan)
    to = np.full((S, n, 2), np.nan)
    _, traced, _, shortened = beam_classes(sc)
    for s in range(S):
        sx, sy, sh = (float(v) for v in sc.poses[s])
        for i in range(n):
            r = float(sc.ranges[s, i])
            if math.isnan(r) or math.isinf(r):
                continue
            angle = sh + sc.laser.angle_min + i * sc.laser.angle_increment
            px = sx + (r * math.cos(angle))
            py = sy + (r * math.sin(angle))
            raw[s, i] = px, py
            if traced[s, i]:
                if shortened[s, i]:
                    ratio = sc.threshold / r
                    dx, dy = px - sx, py - sy
                    px = sx + ratio * dx
                    py = sy + ratio * dy
                to[s, i] = px, py
    return raw, to


def scan_bounds(sc, rows=None):
    """The box ComputeDimensions (Karto.h:5799-5817) derives from these scans: each sensor position and each filtered
    reading; no scans -> BoundingBox2()."""
    raw, _ = _points(sc)
    in_box, _, _, _ = beam_classes(sc)
    rows = range(len(sc.poses)) if rows is None else rows
    box = [BOX_BIG, BOX_BIG, -BOX_BIG, -BOX_BIG]
    for s in rows:
        pts = [(float(sc.poses[s, 0]), float(sc.poses[s, 1]))] + [tuple(p) for p in raw[s][in_box[s]]]
        for x, y in pts:
            box = [min(box[0], x), min(box[1], y), max(box[2], x), max(box[3], y)]
    return np.array(box)


def geometry(sc):
    """-> (w, h, stride, scale, ox, oy, raw_w, raw_h) of the scenario's grid (ComputeDimensions, Grid<T>::Resize
    Karto.h:4442); raw_w / raw_h are the values Round() sees."""
    box = sc.box if sc.box is not None else scan_bounds(sc)
    scale = 1.0 / sc.resolution
    raw_w, raw_h = (float(box[2]) - float(box[0])) * scale, (float(box[3]) - float(box[1])) * scale
    w, h = int(kround(raw_w)), int(kround(raw_h))
    return w, h, (w + 7) & ~7, scale, float(box[0]), float(box[1]), raw_w, raw_h


def _grid_coords(sc):
    """Grid coordinates BEFORE rounding: sensors [S, 2], traced-to points [S, n, 2] (NaN where nothing is traced)."""
    _, _, _, scale, ox, oy, _, _ = geometry(sc)
    _, to = _points(sc)
    off = np.array([ox, oy])
    return (sc.poses[:, :2] - off) * scale, (to - off) * scale


def _round_cells(a):
    return np.where(a >= 0.0, np.floor(a + 0.5), np.ceil(a - 0.5)).astype(np.int64)


def ray_cells(sc):
    """WorldToGrid (Karto.h:4237-4252) of every traced ray -> (scan index, beam index, x0, y0, x1, y1, end_valid), each [R]."""
    sensors, ends = _grid_coords(sc)
    _, traced, end_valid, _ = beam_classes(sc)
    s, i = np.nonzero(traced)
    start = _round_cells(sensors[s])
    end = _round_cells(ends[s, i])
    return s, i, start[:, 0], start[:, 1], end[:, 0], end[:, 1], end_valid[s, i]


def tie_margin(sc):
    """Smallest distance, in cells, of any grid coordinate the build rounds -- sensors, traced-to points, and the width and
    height of a whole build -- from a rounding tie (x.5)."""
    sensors, ends = _grid_coords(sc)
    _, traced, _, _ = beam_classes(sc)
    vals = [sensors[np.unique(np.nonzero(traced)[0])].ravel(), ends[traced].ravel()]
    if sc.box is None:
        vals.append(np.array(geometry(sc)[6:8]))
    v = np.concatenate(vals)
    if v.size == 0:
        return 0.5
    frac = np.abs(v) - np.floor(np.abs(v))
    return float(np.abs(frac - 0.5).min())


def trace_line(x0, y0, x1, y1):
    """Grid<T>::TraceLine (Karto.h:4680-4745), one ray, cell by cell -> [(x, y)] before any validity test."""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0 = y0, x0
        x1, y1 = y1, x1
    if x0 > x1:
        x0, x1 = x1, x0
        y0, y1 = y1, y0
    delta_x, delta_y = x1 - x0, abs(y1 - y0)
    error, y = 0, y0
    ystep = 1 if y0 < y1 else -1
    out = []
    for x in range(x0, x1 + 1):
        out.append((y, x) if steep else (x, y))
        error += delta_y
        if 2 * error >= delta_x:
            y += ystep
            error -= delta_x
    return out


def _trace_lines_lockstep(x0, y0, x1, y1, end_valid, w, h, stride):
    """trace_line over many rays at once: the same recurrence, every ray taking its step k together (rays that have ended sit
    out), then RayTrace's end point -> (pass, hit) planes [h * stride] uint32."""
    cells = max(h, 0) * stride
    cnt = np.zeros((2, cells), dtype=np.int64)
    if cells == 0 or len(x0) == 0:
        return cnt.astype(np.uint32)
    tx, ty = x1.copy(), y1.copy()
    steep = np.abs(y1 - y0) > np.abs(x1 - x0)
    x0, y0, x1, y1 = (np.where(steep, a, b) for a, b in ((y0, x0), (x0, y0), (y1, x1), (x1, y1)))
    swap = x0 > x1
    x0, x1, y0, y1 = (np.where(swap, a, b) for a, b in ((x1, x0), (x0, x1), (y1, y0), (y0, y1)))
    delta_x, delta_y = x1 - x0, np.abs(y1 - y0)
    ystep = np.where(y0 < y1, 1, -1)
    error, y = np.zeros_like(x0), y0.copy()
    for k in range(int(delta_x.max()) + 1):
        live = k <= delta_x
        x = x0 + k
        px, py = np.where(steep, y, x), np.where(steep, x, y)
        error = error + delta_y
        step = live & (2 * error >= delta_x)
        y = np.where(step, y + ystep, y)
        error = np.where(step, error - delta_x, error)
        ok = live & (px >= 0) & (px < w) & (py >= 0) & (py < h)
        np.add.at(cnt[0], (px + py * stride)[ok], 1)
    ok = end_valid & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    np.add.at(cnt[0], (tx + ty * stride)[ok], 1)
    np.add.at(cnt[1], (tx + ty * stride)[ok], 1)
    assert cnt.max() < 2 ** 32
    return cnt.astype(np.uint32)


def trace_line_counters(sc):
    """-> (dims (w, h, stride), counters uint32 [2, h * stride]: pass plane, hit plane) -- what PortKarto.occgrid_partial
    returns -- from the stepped TraceLine on integer cells."""
    w, h, stride = geometry(sc)[:3]
    _, _, x0, y0, x1, y1, end_valid = ray_cells(sc)
    return np.array([w, h, stride], dtype=np.int32), _trace_lines_lockstep(x0, y0, x1, y1, end_valid, w, h, stride)


def trace_line_counters_scalar(sc):
    """trace_line_counters one ray and one cell at a time: slow, and the most literal form; the CPU test holds the lockstep
    form to it."""
    w, h, stride = geometry(sc)[:3]
    cnt = np.zeros((2, max(h, 0) * stride), dtype=np.uint32)
    for _, _, x0, y0, x1, y1, valid in zip(*(a.tolist() for a in ray_cells(sc))):
        for x, y in trace_line(x0, y0, x1, y1):
            if 0 <= x < w and 0 <= y < h:
                cnt[0, x + y * stride] += 1
        if valid and 0 <= x1 < w and 0 <= y1 < h:
            cnt[0, x1 + y1 * stride] += 1
            cnt[1, x1 + y1 * stride] += 1
    return np.array([w, h, stride], dtype=np.int32), cnt


# ---------------------------------------------------------------------------------------------------------------------------
# the scenarios
# ---------------------------------------------------------------------------------------------------------------------------
ONE_BEAM = synth.Laser(n_ranges=1, angle_min=0.0, angle_increment=0.01, range_min=0.01, range_max=60.0)
SWEEP = 70                                        # |dx|, |dy| <= SWEEP: 141^2 scans, one of them of range zero
SWEEP_STARTS = [(80, 80), (73, 88), (89, 71)]     # the centre, then one towards -x +y and one towards +x -y
# sweep_clipped: the sensor stays on world cell (80, 80); (first cell of the box, w, h) -> the sensor's cell in the box
CLIP_BOXES = {
    "outside": ((93, 60), 49, 45),     # sensor on (-13, 20): every ray starts left of the box; w = 1 mod 8
    "first-cell": ((80, 80), 53, 37),  # sensor on (0, 0); w = 5 mod 8
    "last-cell": ((34, 50), 47, 31),   # sensor on (w - 1, h - 1); w = 7 mod 8
}
BEAM_COUNTS = [1, 3, 63, 64, 65, 255, 256, 257, 1081]
EXTREMUM_BEAMS = [0, 63, 64, 255, 256, 1023, 1024, 1080]  # (block, thread) of k_occ_points: first / last of a wave, a block


def _one_beam_scans(res, start_world, dx, dy):
    """One scan per (dx, dy): heading atan2(dy, dx), range hypot * res from the given world position."""
    theta = np.arctan2(dy, dx)
    ranges = (np.hypot(dx, dy) * res)[:, None]
    poses = np.stack([np.full(len(dx), start_world[0]), np.full(len(dx), start_world[1]), theta], 1)
    return ranges, poses


def _sweep_offsets():
    d = np.arange(-SWEEP, SWEEP + 1)
    dx, dy = (a.ravel() for a in np.meshgrid(d, d))
    return dx, dy


def _sweep_centre(cx, cy):
    res = 0.05
    dx, dy = _sweep_offsets()
    ranges, poses = _one_beam_scans(res, (cx * res, cy * res), dx, dy)
    start = np.stack([np.full(len(dx), cx), np.full(len(dx), cy)], 1)
    return Scenario(f"sweep_centre[{cx},{cy}]", ONE_BEAM, 20.0, ranges, poses, res, np.array([0.0, 0.0, 161 * res, 161 * res]),
                    intent=(start, start + np.stack([dx, dy], 1)))


def _sweep_clipped(key):
    res = 0.05
    (bx, by), w, h = CLIP_BOXES[key]
    dx, dy = _sweep_offsets()
    ranges, poses = _one_beam_scans(res, (80 * res, 80 * res), dx, dy)
    start = np.stack([np.full(len(dx), 80 - bx), np.full(len(dx), 80 - by)], 1)
    return Scenario(f"sweep_clipped[{key}]", ONE_BEAM, 20.0, ranges, poses, res,
                    np.array([bx * res, by * res, (bx + w) * res, (by + h) * res]), intent=(start, start + np.stack([dx, dy], 1)))


def _long_thin(axis):
    """Rays of +-1990..2000 cells along `axis` with up to 15 cells across, at 1 cm cells: 32 rounds of the 64-lane stride, and
    2 * k * deltaY up to 60 000."""
    res = 0.01
    along = np.concatenate([np.arange(1990, 2001), -np.arange(1990, 2001)])
    a, c = (v.ravel() for v in np.meshgrid(along, np.arange(-15, 16)))
    start_along = np.where(a > 0, 50, 2050)
    start = np.stack([start_along, np.full(len(a), 20)], 1)
    d = np.stack([a, c], 1)
    box = np.array([0.0, 0.0, 2100 * res, 40 * res])
    if axis == "y":
        start, d, box = start[:, ::-1], d[:, ::-1], box[[1, 0, 3, 2]]
    theta = np.arctan2(d[:, 1], d[:, 0])
    ranges = (np.hypot(d[:, 0], d[:, 1]) * res)[:, None]
    poses = np.stack([start[:, 0] * res, start[:, 1] * res, theta], 1)
    return Scenario(f"long_thin[{axis}]", ONE_BEAM, 30.0, ranges, poses, res, box, intent=(start, start + d))


def _keep_off_ties(make, ranges):
    """Moves any reading whose end point lies within 1e-3 cells of a rounding tie by 1.3 cm, until none does."""
    for _ in range(20):
        sc = make(ranges)
        _, ends = _grid_coords(sc)
        frac = np.abs(ends) - np.floor(np.abs(ends))
        near = (np.abs(frac - 0.5) < 1e-3).any(axis=2)
        if not near.any():
            return sc
        ranges = ranges.copy()
        ranges[:, :near.shape[1]][near] += 0.013
    raise AssertionError("cannot keep the scenario's end points off the rounding ties")


def _beam_counts(n, cols=None):
    """S scans of n beams (S * n no multiple of 4 wherever n allows it) with random readings of 0.2 .. 4 m from poses near
    the middle of a 203 x 197 grid; cols > n: the rows are longer than the laser's beam count and the surplus holds valid
    readings that would be traced if the row pitch were taken for the beam count."""
    S = 5 if n in (1, 3) else 3
    rng = np.random.default_rng(600 + n + (cols or 0))
    laser = synth.Laser(n_ranges=n, angle_min=-2.7, angle_increment=0.005, range_min=0.1, range_max=60.0)
    poses = np.stack([rng.integers(-400, 400, S) * 1e-3 + 0.0123, rng.integers(-400, 400, S) * 1e-3 - 0.0071,
                      rng.uniform(-math.pi, math.pi, S)], 1)
    ranges = rng.uniform(0.2, 4.0, (S, cols or n))
    name = f"beam_counts[{n}]" if cols is None else f"beam_counts[{n}of{cols}]"
    box = np.array([-5.0, -5.0, 5.15, 4.85])
    return _keep_off_ties(lambda r: Scenario(name, laser, 20.0, r, poses, 0.05, box), ranges)


def range_class_values(laser, threshold):
    """Every reading AddScan and LocalizedRangeScan::Update tell apart: the unordered ones, then just below, at and just above
    each limit."""
    vals = [np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0]
    for lim in (laser.range_min, threshold - k_tol(), threshold, laser.range_max):
        vals += [np.nextafter(lim, -np.inf), lim, np.nextafter(lim, np.inf)]
    return np.array(vals)


def _range_classes():
    """The readings of range_class_values on neighbouring beams of a 6 mrad fan, seen from one end of a 27 x 8 m box, and in
    reverse order from the other end looking back."""
    thr = 20.0
    laser = synth.Laser(n_ranges=18, angle_min=-0.05, angle_increment=0.006, range_min=0.1, range_max=60.0)
    vals = range_class_values(laser, thr)
    assert len(vals) == laser.n_ranges
    box = np.array([-3.0, -4.0, 24.05, 4.15])
    poses = np.array([[0.0131, 0.0177, 0.0], [21.0131 - 0.0262, 0.1177, math.pi]])
    return Scenario("range_classes", laser, thr, np.stack([vals, vals[::-1]]), poses, 0.05, box)


def _box_extremum():
    """Scans 0..7: everything NaN but beam EXTREMUM_BEAMS[k], which reads 7 m along heading 0.3 + k; scans 8..11: one reading
    each, of 9 m, due -x from beam 63, due -y from beam 256, due +x from beam 1023 and due +y from beam 1080 -- the four
    extremes of the joint box come from four scans and four blocks."""
    laser = synth.Laser()
    rows, poses = [], []

    def scan(beam, direction, r, at):
        row = np.full(laser.n_ranges, np.nan)
        row[beam] = r
        rows.append(row)
        poses.append([at[0], at[1], direction - (laser.angle_min + beam * laser.angle_increment)])

    for k, b in enumerate(EXTREMUM_BEAMS):
        scan(b, 0.3 + k, 7.0, (0.1 * k, -0.2 * k))
    for b, direction, at in ((63, math.pi, (0.3, 0.1)), (256, -math.pi / 2, (-0.2, 0.4)), (1023, 0.0, (0.1, -0.3)),
                             (1080, math.pi / 2, (0.2, 0.2))):
        scan(b, direction, 9.0, at)
    groups = tuple([k] for k in range(12)) + (list(range(8)), list(range(8, 12)), list(range(12)))
    return Scenario("box_extremum", laser, 20.0, np.array(rows), np.array(poses), 0.05, None, groups=groups)


TIE_W, TIE_H = 13, 5


def _exact_ties():
    """Cells of 1/8 m, heading 0, everything a multiple of 1/16 m: the grid coordinates are exact multiples of one half in
    every implementation, and sensors and end points sit on -1.5, -0.5, 0.5, 1.5 and on the far edge's w - 0.5 and h - 0.5."""
    res = 0.125
    ox, oy = 0.5, -0.25
    rows = []
    for sgx in (-1.5, -0.5, 0.5, 1.5):
        for egx in (-0.5, 0.5, 1.5, 2.5, TIE_W - 1.5, TIE_W - 0.5, TIE_W + 0.5):
            for sgy in (-1.5, -0.5, 0.5, 1.5, TIE_H - 1.5, TIE_H - 0.5):
                if egx > sgx:
                    rows.append((ox + sgx * res, oy + sgy * res, (egx - sgx) * res))
    rows = np.array(rows)
    poses = np.stack([rows[:, 0], rows[:, 1], np.zeros(len(rows))], 1)
    return Scenario("exact_ties", ONE_BEAM, 20.0, rows[:, 2:3].copy(), poses, res,
                    np.array([ox, oy, ox + TIE_W * res, oy + TIE_H * res]), min_margin=0.0)


def _degenerate(kind):
    if kind == "0x0":  # nothing but ignored readings from one position: the box is that position
        laser = synth.Laser(n_ranges=5)
        ranges = np.array([[np.nan, 0.05, 70.0, np.nan, 0.0]] * 2)
        return Scenario("degenerate[0x0]", laser, 20.0, ranges, np.array([[1.25, -0.5, 0.3], [1.25, -0.5, -1.0]]), 0.05, None)
    if kind == "wx0":  # readings along heading 0 from one line y = const: the box has no height
        ranges = np.array([[1.0131], [2.0177], [0.5113]])
        poses = np.array([[0.0, 0.75, 0.0], [0.4021, 0.75, 0.0], [-0.2017, 0.75, 0.0]])
        return Scenario("degenerate[wx0]", ONE_BEAM, 20.0, ranges, poses, 0.05, None)
    assert kind == "same-cell"  # one valid reading shorter than half a cell: a ray of one cell, traced and hit
    return Scenario("degenerate[same-cell]", ONE_BEAM, 20.0, np.array([[0.013]]), np.array([[0.1031, 0.0517, 0.7]]), 0.05,
                    np.array([0.0, 0.0, 0.25, 0.15]), intent=(np.array([[2, 1]]), np.array([[2, 1]])))


_BUILDERS = {}
for _c in SWEEP_STARTS:
    _BUILDERS[f"sweep_centre[{_c[0]},{_c[1]}]"] = functools.partial(_sweep_centre, *_c)
for _k in CLIP_BOXES:
    _BUILDERS[f"sweep_clipped[{_k}]"] = functools.partial(_sweep_clipped, _k)
for _a in ("x", "y"):
    _BUILDERS[f"long_thin[{_a}]"] = functools.partial(_long_thin, _a)
for _n in BEAM_COUNTS:
    _BUILDERS[f"beam_counts[{_n}]"] = functools.partial(_beam_counts, _n)
_BUILDERS["beam_counts[1000of1081]"] = functools.partial(_beam_counts, 1000, 1081)
_BUILDERS["range_classes"] = _range_classes
_BUILDERS["box_extremum"] = _box_extremum
_BUILDERS["exact_ties"] = _exact_ties
for _k in ("0x0", "wx0", "same-cell"):
    _BUILDERS[f"degenerate[{_k}]"] = functools.partial(_degenerate, _k)

NAMES = list(_BUILDERS)
WHOLE_BUILDS = ["degenerate[0x0]", "degenerate[wx0]"]                       # box None and counters compared
COUNTER_NAMES = [n for n in NAMES if n != "box_extremum"]                    # box_extremum compares scan_bounds only
SWEEP_CENTRE = "sweep_centre[80,80]"


@functools.lru_cache(maxsize=None)
def _built(name):
    return _BUILDERS[name]()


def scenario(name):
    return _built(name)


def as_whole_build(sc):
    """The same scans with the grid sized from them."""
    return sc._replace(name=sc.name + "/whole", box=None)
