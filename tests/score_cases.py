"""Scenarios for pose scoring (lslam_map_score_batch / lslam_map_pose_covariance_batch / lslam_map_score_lattice): the
smallest shapes at which it can go wrong.  Pure numpy; the recorder (tests/golden/make_score_golden.py) runs the reference on
them, tests/test_score_oracle.py checks on the CPU that every scenario is what it claims, tests/test_score_gpu.py runs them
through the kernels.

Maps
  main   96 x 80 cells of 0.05 m, 3 levels (48 x 40, 24 x 20), offset (2.3, 1.9): an L-shaped room with a box in it, drawn from
         five scans cast in it
  small  33 x 31 cells of 0.0625 m, 1 level, offset (-0.0, -0.0): a cross through cell (16, 15), drawn by four axis-aligned
         beams, so the plane is mirror-symmetric about column 16 and map coordinates are the container's own at the pose
         (-0.0, -0.0, 0) -- the band of tests/gn_edge_cases.py (exactly 0.0, -0.0, lim, nextafter(lim)) can be placed, and two
         lattice states either side of the column tie exactly

A QUERY is (map, container, world pose, level); every state of every batch and lattice below is one, and the golden file
holds the reference's residual and likelihood of each."""
import functools
import pathlib
from typing import NamedTuple

import numpy as np

f32 = np.float32
OCC_FACTOR = 0.9
SIZES = (0, 1, 63, 64, 65, 130, 257, 1081)
BIG = 65536
TRUTH = np.array([0.12, -0.07, 0.21], f32)
BATCH_SIZES = (1, 3, 4, 5, 9, 130)


class Map(NamedTuple):
    name: str
    sx: int
    sy: int
    cell: float
    levels: int
    off: tuple
    scans: list  # [(points [n,2] float32 in level-0 cells, world pose float32[3])]


def level_list(m: Map):
    """[(sx, sy, cell float32)] as lslam_map_create and MapRepMultiMap build them."""
    out, sx, sy, cl = [], m.sx, m.sy, f32(m.cell)
    for _ in range(m.levels):
        if sx <= 0 or sy <= 0:
            break
        out.append((sx, sy, cl))
        sx //= 2
        sy //= 2
        cl = f32(cl * f32(2.0))
    return out


# ---- the main map's world: wall segments in metres ---------------------------------------------------------------------------
def _segments():
    outer = [(-2.0, -1.6), (2.1, -1.6), (2.1, 1.7), (-2.0, 1.7)]
    segs = [(outer[i], outer[(i + 1) % 4]) for i in range(4)]
    box = [(0.6, 0.3), (1.1, 0.3), (1.1, 0.9), (0.6, 0.9)]
    segs += [(box[i], box[(i + 1) % 4]) for i in range(4)]
    segs += [((-2.0, -0.5), (-1.2, -0.5)), ((-1.2, -0.5), (-1.2, -1.6))]  # the corner that makes the room an L
    return np.array(segs, np.float64)


def cast(pose, n_beams=1081, fov=np.deg2rad(270.0), noise=0.0, rng=None):
    """A scan of the room from a world pose -> container points [n_beams, 2] float32, robot frame, level-0 cells of 0.05 m."""
    segs = _segments()
    a = np.linspace(-fov / 2, fov / 2, n_beams)
    d = np.stack([np.cos(a + pose[2]), np.sin(a + pose[2])], 1)  # [B,2]
    o = np.array([pose[0], pose[1]], np.float64)
    p, q = segs[:, 0], segs[:, 1]
    e = q - p  # [S,2]
    den = d[:, None, 0] * e[None, :, 1] - d[:, None, 1] * e[None, :, 0]
    w = p[None] - o  # [1,S,2]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (w[..., 0] * e[None, :, 1] - w[..., 1] * e[None, :, 0]) / den
        u = (w[..., 0] * d[:, None, 1] - w[..., 1] * d[:, None, 0]) / den
    t = np.where((den != 0) & (t > 1e-9) & (u >= 0) & (u <= 1), t, np.inf)
    r = t.min(1)
    assert np.isfinite(r).all()
    if noise:
        r = r + rng.normal(0.0, noise, r.shape)
    return (np.stack([r * np.cos(a), r * np.sin(a)], 1) / 0.05).astype(f32)


@functools.lru_cache(maxsize=None)
def maps():
    rng = np.random.default_rng(11)
    poses = [(0.0, 0.0, 0.0), (0.15, 0.1, 0.1), (-0.2, 0.05, -0.15), (0.1, -0.2, 0.3), (0.3, 0.2, 3.0)]
    main = Map("main", 96, 80, 0.05, 3, (2.3, 1.9), [(cast(p, noise=0.004, rng=rng), np.array(p, f32)) for p in poses])
    centre = np.array([16 * 0.0625, 15 * 0.0625, 0.0], f32)
    arms = [np.array([[x, y]], f32) for x, y in ((16.0, 0.0), (-16.0, 0.0), (0.0, 15.0), (0.0, -15.0))]
    small = Map("small", 33, 31, 0.0625, 1, (-0.0, -0.0), [(a, centre) for _ in range(3) for a in arms])
    return {"main": main, "small": small}


@functools.lru_cache(maxsize=None)
def containers():
    """name -> points [n,2] float32 (level-0 cells).  "n<k>": k points of the scan cast at TRUTH; "big": 65536 points, all inside
    the main map at TRUTH; "axis" / "band": the small map's."""
    rng = np.random.default_rng(12)
    scan = cast(P("truth").astype(np.float64), noise=0.004, rng=rng)
    out = {}
    for k in SIZES:
        idx = np.round(np.linspace(0, len(scan) - 1, k)).astype(int) if k else np.zeros(0, int)
        out["n%d" % k] = scan[idx].copy()
    out["big"] = derive_big(out["n1081"])
    # on the small map's mirror axis (robot-frame x = 0): a state a quarter cell left of column 16 and one a quarter cell right
    # of it see the same value at every point
    ys = np.concatenate([np.arange(-12.0, 12.5, 1.75), [13.5, -13.25]])
    out["axis"] = np.stack([np.zeros_like(ys), ys], 1).astype(f32)
    lim_x, lim_y = f32(33 - 2), f32(31 - 2)
    up_x, up_y = np.nextafter(lim_x, f32(np.inf)), np.nextafter(lim_y, f32(np.inf))
    out["band"] = np.array([
        [0.0, 15.0], [-0.0, 15.25], [lim_x, 15.0], [up_x, 15.0], [16.0, 0.0], [-0.0, -0.0], [16.5, lim_y], [16.0, up_y],
        [lim_x, lim_y], [up_x, up_y], [lim_x, up_y], [up_x, lim_y], [0.0, 0.0], [16.25, 15.5], [3.5, 15.0], [16.0, 4.75]], f32)
    return out


def derive_big(scan):
    """65536 points from the 1081-point scan by exact float32 products (copies shrunk toward the robot: all inside the map at
    TRUTH), so the golden file need not carry them."""
    reps = -(-BIG // len(scan))
    return np.concatenate([scan * f32(0.25 + k / 256.0) for k in range(reps)])[:BIG].astype(f32)


BAND_OUTSIDE = 5  # points of "band" beyond lim by one ulp in x or y


class Query(NamedTuple):
    map: str
    container: str
    pose: tuple  # world pose, float32 values
    level: int


def _q(map_, cont, pose, level):
    return Query(map_, cont, tuple(float(v) for v in np.asarray(pose, f32)), int(level))


# ---- the poses.  The reference turns a heading into a rotation with the C library's sinf / cosf, which are good to ~0.56 ulp,
# not correctly rounded: at about one heading in forty one of them is an ulp off the rounded double value, differently from
# one C library (and one CPU's FMA variant of it) to the next, and the reference's own result then moves in its last bits
# from host to host.  A recorded result pins something only where the reference is reproducible, so the recorder moves every
# heading it uses -- the sigma points' and every lattice plane's included -- up by a few ulps to the next float32 at which the
# recording host's sinf and cosf ARE the correctly rounded values (generate_poses), and stores the poses in the golden file;
# the tests take them from there (P), like the scans and containers.
_GENERATED = None  # the recorder sets this to generate_poses() before anything else is called


@functools.lru_cache(maxsize=None)
def _pose_table():
    if _GENERATED is not None:
        return _GENERATED
    z = np.load(GOLDEN)
    return {k[len("pose_"):]: z[k] for k in z.files if k.startswith("pose_")}


def P(name):
    return _pose_table()[name]


BATCH_CONTAINERS = ("n1081", "n0", "n257", "n130", "n65", "n64", "n63", "n1")  # an empty container between two full ones
RELOC_COUNTS, RELOC_STEPS, RELOC_LEVEL, RELOC_K = (17, 17, 13), (0.05, 0.05, 0.05), 1, 5  # +-8 cells, +-0.3 rad
COV_OFFSETS = {"n1081-L0": (0, 0, 0), "n1081-L1": (0, 0, 0), "n1081-L2": (0, 0, 0), "n63-L2": (0, 0, 0),
               "n257-L0": (0.03, 0.02, 0.01), "n65-L1": (-0.02, 0.03, -0.02), "n130-L0": (0.01, -0.02, 0.03)}
LATTICE_SHAPES = {  # name -> (map, container, counts, steps, level)
    "5x3x7": ("main", "n1081", (5, 3, 7), (0.05, 0.05, 0.02), 0),      # 105 states: no multiple of 64
    "1x1x1": ("main", "n1081", (1, 1, 1), (0.05, 0.05, 0.02), 1),
    "16x16x21": ("main", "n257", (16, 16, 21), (0.2, 0.2, 0.03), 2),
    "rim-off": ("main", "n1081", (3, 3, 1), (40.0, 40.0, 0.1), 0),     # every rim state pushes every point off the map
    "tie": ("small", "axis", (3, 1, 1), (0.015625, 0.25, 0.1), 0),     # states 0 and 2: a quarter cell either side of column 16
    "all-nan": ("main", "n0", (2, 2, 2), (0.05, 0.05, 0.02), 0),
    "reloc": ("main", "n1081", RELOC_COUNTS, RELOC_STEPS, RELOC_LEVEL),
}


def generate_poses():
    """The pose table, on the recording host (needs its C library): name -> float32 [3] or [n, 3]."""
    import ctypes
    import math

    m = ctypes.CDLL("libm.so.6")
    for fn in (m.sinf, m.cosf):
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]

    def good(h):
        x = float(f32(h))
        return f32(m.sinf(x)) == f32(math.sin(x)) and f32(m.cosf(x)) == f32(math.cos(x))

    def nudge(pose, others=lambda h: ()):
        p = np.array(pose, f32)
        while not (good(p[2]) and all(good(o) for o in others(p[2]))):
            p[2] = np.nextafter(p[2], f32(np.inf))
        return p

    sigma = lambda h: [h + f32(0.05), h - f32(0.05)]
    plane = lambda nt, dt: (lambda h: [h + f32(k - nt // 2) * f32(dt) for k in range(nt)])
    t = {}
    t["truth"] = nudge(TRUTH, lambda h: sigma(h) + plane(21, 0.03)(h))
    truth = t["truth"]
    t["part_out"] = nudge([1.2, 0.9, 0.21])    # part of the scan leaves every level
    t["all_out"] = nudge([30.0, 20.0, 0.2])    # every point outside every level
    t["headings"] = np.stack([nudge([0.1, 0.05, h]) for h in (3.14159, -3.1415925, 0.0)])
    t["band"] = np.array([-0.0, -0.0, 0.0], f32)
    t["axis"] = np.array([1.0, 0.9375, 0.0], f32)
    for L in (0, 1, 2):
        rng = np.random.default_rng(13 + L)
        poses = (truth + rng.uniform(-1.0, 1.0, (130, 3)) * np.array([0.3, 0.3, 0.25])).astype(f32)
        poses[0] = truth
        t["batch_L%d" % L] = np.stack([nudge(p) for p in poses])
    for k, off in COV_OFFSETS.items():
        t["cov_" + k] = nudge(truth + np.array(off, f32), sigma)
    centres = {"5x3x7": truth + np.array([0.02, -0.01, 0.01], f32), "1x1x1": truth, "16x16x21": truth, "rim-off": truth,
               "tie": t["axis"], "all-nan": truth, "reloc": truth + np.array([0.24, -0.18, 0.2], f32)}  # reloc: 6 cells, 0.2 rad off
    for k, c in centres.items():
        _, _, counts, steps, _ = LATTICE_SHAPES[k]
        t["lat_" + k] = nudge(c, plane(counts[2], steps[2]))
    return t


@functools.lru_cache(maxsize=None)
def singles():
    """name -> Query: the directed single states."""
    out = {}
    for k in SIZES:
        out["size-%d" % k] = _q("main", "n%d" % k, P("truth"), 0)
    out["size-big"] = _q("main", "big", P("truth"), 0)
    for L in (0, 1, 2):
        out["inside-L%d" % L] = _q("main", "n1081", P("truth"), L)
        out["part-out-L%d" % L] = _q("main", "n1081", P("part_out"), L)
        out["all-out-L%d" % L] = _q("main", "n1081", P("all_out"), L)
    for i, p in enumerate(P("headings")):  # near +pi, near -pi, 0
        out["heading-%d" % i] = _q("main", "n257", p, 0)
    out["band"] = _q("small", "band", P("band"), 0)
    out["axis"] = _q("small", "axis", P("axis"), 0)
    return out


@functools.lru_cache(maxsize=None)
def batch(level):
    """-> (container names, entry_container[130], poses[130,3]) of the 130-entry batch on one level; the smaller batches are
    its prefixes (1, 3, 4, 5, 9 entries), so they share its containers and straddle any block shape."""
    ec = np.array([e % len(BATCH_CONTAINERS) for e in range(130)], np.int32)
    ec[8:16] = 0  # one container shared by consecutive entries
    return BATCH_CONTAINERS, ec, P("batch_L%d" % level)


def batch_queries(level):
    names, ec, poses = batch(level)
    return [_q("main", names[c], p, level) for c, p in zip(ec, poses)]


class Lattice(NamedTuple):
    map: str
    container: str
    centre: tuple
    counts: tuple  # nx, ny, nt
    steps: tuple
    level: int


@functools.lru_cache(maxsize=None)
def lattices():
    c = lambda v: tuple(float(x) for x in np.asarray(v, f32))
    return {k: Lattice(m, cont, c(P("lat_" + k)), counts, c(steps), level) for k, (m, cont, counts, steps, level) in LATTICE_SHAPES.items()}


def lattice_poses(lat: Lattice) -> np.ndarray:
    """World poses of a lattice's states in the volume's order [nt][ny][nx] -> [N, 3] float32, by the expression the device
    evaluates: c + (float)(i - n/2) * d, integer division, product and sum rounded separately."""
    nx, ny, nt = lat.counts
    c, d = np.array(lat.centre, f32), np.array(lat.steps, f32)
    out = np.zeros((nt, ny, nx, 3), f32)
    for k in range(nt):
        for j in range(ny):
            for i in range(nx):
                out[k, j, i] = (c[0] + f32(i - nx // 2) * d[0], c[1] + f32(j - ny // 2) * d[1], c[2] + f32(k - nt // 2) * d[2])
    return out.reshape(-1, 3)


def lattice_queries(name):
    lat = lattices()[name]
    return [_q(lat.map, lat.container, p, lat.level) for p in lattice_poses(lat)]


@functools.lru_cache(maxsize=None)
def covariances():
    """name -> Query for getCovarianceForPose; only cases whose seven reference likelihoods are >= 0.2 (tests/test_score_oracle.py
    holds them to that)."""
    return {k: _q("main", k.split("-")[0], P("cov_" + k), int(k[-1])) for k in COV_OFFSETS}


COV_MIN_LIKELIHOOD = 0.2


@functools.lru_cache(maxsize=None)
def all_queries():
    """Every distinct state the golden file records, in a fixed order -> [Query]."""
    qs = list(singles().values())
    for L in (0, 1, 2):
        qs += batch_queries(L)
    for name in lattices():
        qs += lattice_queries(name)
    seen, out = set(), []
    for q in qs:
        if q not in seen:
            seen.add(q)
            out.append(q)
    return out


# ---- the recorded reference -------------------------------------------------------------------------------------------------
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "score_golden.npz"


class Golden:
    """tests/golden/score_golden.npz: the scans, planes and containers as recorded (the tests take them from here, not from the
    generators above, whose libm calls may round differently elsewhere) and the reference's results per query."""

    def __init__(self):
        z = np.load(GOLDEN)
        self.maps, self.planes = {}, {}
        for name, m in maps_shape().items():
            counts, pts, poses = z[name + "_scan_counts"], z[name + "_scan_points"], z[name + "_scan_poses"]
            first = np.concatenate([[0], np.cumsum(counts)])
            scans = [(pts[first[i]:first[i + 1]], poses[i]) for i in range(len(counts))]
            self.maps[name] = m._replace(scans=scans)
            for L, (sx, sy, _) in enumerate(level_list(m)):
                self.planes[name, L] = z["%s_plane_L%d" % (name, L)]
                assert self.planes[name, L].shape == (sy, sx)
        self.containers = {k[len("container_"):]: z[k] for k in z.files if k.startswith("container_")}
        self.containers["big"] = derive_big(self.containers["n1081"])
        qs = all_queries()
        self.q_pose = z["q_pose"]
        assert len(qs) == len(self.q_pose) and all(np.array(q.pose, f32).tobytes() == p.tobytes() for q, p in zip(qs, self.q_pose))
        self.index = {q: i for i, q in enumerate(qs)}
        self.residual, self.likelihood = z["q_residual"], z["q_likelihood"]
        self.cov = {name: (z["cov_%s_lik" % name], z["cov_%s_map" % name], z["cov_%s_world" % name]) for name in covariances()}
        self.ref_cpu_state_s = float(z["ref_cpu_state_s"])

    def ref(self, queries):
        """-> (residual[n], likelihood[n]) float32 of the reference for a list of queries."""
        i = np.array([self.index[q] for q in queries], int)
        return self.residual[i], self.likelihood[i]


def maps_shape():
    """The maps without their scans (sizes, cells, offsets): what does not depend on a generator."""
    return {"main": Map("main", 96, 80, 0.05, 3, (2.3, 1.9), []), "small": Map("small", 33, 31, 0.0625, 1, (-0.0, -0.0), [])}


@functools.lru_cache(maxsize=None)
def golden():
    return Golden()
