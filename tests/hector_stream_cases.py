"""Scenarios for the streamed HectorSlamProcessor (lslam_hector_*, api.HectorProcessor): HectorSlamProcessor::update
(H/slam_main/HectorSlamProcessor.h:81-108) over recorded stretches of scans.

  (a) chain60   the 60-scan chain of test_reference_hector_processor_on_gpu_map_rep: 1024^2, 0.05 m, 3 levels, truth
                (0.04 k, 0.015 k, 0.004 k), every scan started from the previous result
  (b) mapping25 that file's 25-scan mapping-only run at 512^2 (map_without_matching, the pose is the hint)
  (c) edges     a 12-scan chain of a 90-reading laser on a 256^2 map with 1 and with 3 levels: 90 is no multiple of 4,
                scan 5 has every range inf (an empty container in mid-chain), scans 7..10 are masked down to exactly 63, 64,
                65 and 1 valid points (one wave of beams less one, exactly one, one more; a single beam)
  (d) gate      pose pairs for util::poseDifferenceLargerThan (H/util/UtilFunctions.h:72-91) and its numpy restatement

Pure numpy plus the project's synth module; the oracle (oracle.pyoracle) and the device API are handed in by the caller:
tests/test_hector_stream_oracle.py checks each scenario's preconditions on the reference's own processor, without a GPU,
and tests/test_hector_stream_gpu.py runs the same scenarios through the kernels."""
import functools
import math
from typing import NamedTuple

import numpy as np

from lslam_amd import synth

f32 = np.float32
CELL = 0.05
FLT_MAX = np.finfo(np.float32).max
MIN_DIST, MIN_ANGLE = 0.4, 0.13  # HectorSlamProcessor.h:66-67
# the project's bounds for this path (tests/test_ref_drives_gpu.py:193-225): pose within 1e-4 of the reference's, covariance
# within 2e-3 of max(1, |cov|max), differing cells <= 0.002 of the reference's non-zero cells per level
POSE_TOL, COV_TOL, CELLS_TOL = 1e-4, 2e-3, 0.002
GATE_MARGIN = 1e-3  # ten times the pose contract: no pose difference the contract allows flips a decision of (a)


class Scenario(NamedTuple):
    n: int             # the map is n x n cells of CELL metres, centred
    levels: int
    laser: object
    ranges: object     # [n_scans, n_readings] float32, or None
    containers: list   # [n_i, 2] float32 per scan, level-0 cell units
    hints: object      # [n_scans, 3] float32, or None: chained from (0, 0, 0)
    no_match: bool
    truth: object      # [n_scans, 3]
    min_dist: float = MIN_DIST
    min_angle: float = MIN_ANGLE


def offset(n):
    """The map offset MapRepMultiMap gives startCoords (0.5, 0.5) (H/slam_main/MapRepMultiMap.h:57-93), in float32."""
    return (float(f32(CELL) * f32(n) * f32(0.5)),) * 2


@functools.lru_cache(maxsize=None)
def chain60():
    laser = synth.Laser()
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=5)
    truth = np.array([(0.04 * k, 0.015 * k, 0.004 * k) for k in range(60)])
    conts = [synth.hector_points(synth.cast_scan(world, t, laser), laser, 1.0 / CELL) for t in truth]
    return Scenario(1024, 3, laser, None, conts, None, False, truth)


@functools.lru_cache(maxsize=None)
def mapping25():
    laser = synth.Laser()
    world = synth.arena(size=30.0, n_axis=8, n_rot=3, seed=6)
    poses = np.array([[0.1 * k - 1.0, 0.05 * k, 0.03 * k] for k in range(25)], f32)
    conts = [synth.hector_points(synth.cast_scan(world, p, laser), laser, 1.0 / CELL, use_max=10.0) for p in poses]
    return Scenario(512, 3, laser, None, conts, poses, True, poses)


EDGE_EMPTY = 5
EDGE_MIN_DIST = 0.04  # setMapUpdateMinDistDiff for (c): its 0.01 m steps then update the map every few scans
EDGE_COUNTS = {7: 63, 8: 64, 9: 65, 10: 1}


def edge_world():
    """A 2.4 m x 2 m room around the start -- its walls are 20 to 24 cells away, so the hits of beams 3 degrees apart form
    closed lines in the map on every level and the matcher is as well-posed as with a dense laser: perturbing the points by
    2e-5 cells moves the reference's poses by 1e-6 (in rooms of 3.6 m and more the same perturbation moved them by
    centimetres, on either pyramid) -- with a 0.4 m doorway straight ahead, through which a few beams reach a wall at 8 m,
    outside the 256^2 map (it ends at +-6.4 m)."""
    a, b, g = 1.2, 1.0, 0.2
    segs = [[-a, -b, a, -b], [a, -b, a, -g], [a, g, a, b], [a, b, -a, b], [-a, b, -a, -b]] + synth.square_room(8.0).tolist()
    return np.asarray(segs, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def edges(levels):
    """Ranges are what the caller streams; the containers are synth.hector_project of them -- the host evaluation the device
    projection is held to, bit for bit (tests/test_logodds_gpu.py).  The single beam of scan 10 is one that ends OUTSIDE the
    map: a lone point inside it gives the reference a rank-one Hessian whose inverse is not finite, and its own matcher then
    indexes the map with a NaN pose; outside, the point adds nothing to H and the scan returns its start pose."""
    laser = synth.Laser(n_ranges=90, angle_min=math.radians(-135.0), angle_increment=math.radians(3.0))
    world = edge_world()
    truth = np.array([(0.01 * k, 0.004 * k, 0.002 * k) for k in range(12)])
    ranges = np.stack([synth.cast_scan(world, t, laser) for t in truth]).astype(f32)
    ranges[EDGE_EMPTY] = np.inf
    for k, keep in EDGE_COUNTS.items():
        valid = np.flatnonzero(_project(ranges[k], laser)[1])
        assert len(valid) >= keep, (k, len(valid))
        if keep == 1:
            kept = valid[[int(np.argmax(ranges[k, valid]))]]
            assert ranges[k, kept[0]] * 20.0 > 0.5 * 256 + 20, ranges[k, kept[0]]  # beyond the map from anywhere near its centre
        else:  # the beams in the middle of the fan
            first = (len(valid) - keep) // 2
            kept = valid[first:first + keep]
        drop = np.ones(laser.n_ranges, bool)
        drop[kept] = False
        ranges[k, drop] = np.inf
    conts = [synth.hector_project(r, laser, 1.0 / CELL)[0] for r in ranges]
    return Scenario(256, levels, laser, ranges, conts, None, False, truth, EDGE_MIN_DIST)


def _project(r, laser):
    """-> (points, mask of the readings that survive) of the node's projection and filters."""
    pts, _ = synth.hector_project(r, laser, 1.0 / CELL)
    keep = np.array([len(synth.hector_project(np.where(np.arange(len(r)) == i, r, np.inf).astype(f32), laser, 1.0 / CELL)[0]) == 1
                     for i in range(len(r))])
    return pts, keep


# ---- (d) the gate ---------------------------------------------------------------------------------------------------------
def gate_table():
    """[(pose1, pose2, min_dist, min_angle, what)]: distances 0.4 -+ 1e-3 with equal headings; heading differences alone."""
    rows = []
    for d in (0.4 - 1e-3, 0.4 + 1e-3):
        for ang in (0.0, 0.7, 2.0):
            rows.append(((d * math.cos(ang), d * math.sin(ang), 0.3), (0.0, 0.0, 0.3), MIN_DIST, MIN_ANGLE, "distance %.4f" % d))
            rows.append(((1.0 + d * math.cos(ang), -2.0 + d * math.sin(ang), -1.0), (1.0, -2.0, -1.0), MIN_DIST, MIN_ANGLE,
                         "distance %.4f, off origin" % d))
    for dth in (0.5, -0.5, 1.5, -1.5, math.pi - 1e-3, math.pi + 1e-3, -math.pi + 1e-3, -math.pi - 1e-3):
        rows.append(((0.0, 0.0, dth), (0.0, 0.0, 0.0), MIN_DIST, MIN_ANGLE, "heading %+.4f" % dth))
        rows.append(((0.1, 0.1, 0.25 + dth), (0.1, 0.1, 0.25), MIN_DIST, MIN_ANGLE, "heading %+.4f from 0.25" % dth))
    rows.append(((0.0, 0.0, 0.0), (FLT_MAX, FLT_MAX, FLT_MAX), MIN_DIST, MIN_ANGLE, "FLT_MAX"))
    rows.append(((3.0, -2.0, 1.0), (FLT_MAX, FLT_MAX, FLT_MAX), MIN_DIST, MIN_ANGLE, "FLT_MAX, off origin"))
    return rows


SUB_RADIAN = ("heading +0.5000", "heading -0.5000")  # rows where |wrapped difference| is in (0.13, 1): abs(int) says 0


def pose_distance(p, q):
    p, q = np.asarray(p, f32), np.asarray(q, f32)
    with np.errstate(over="ignore"):
        dx, dy = p[0] - q[0], p[1] - q[1]
        return f32(np.sqrt(dx * dx + dy * dy))


def gate(p, q, min_dist=MIN_DIST, min_angle=MIN_ANGLE, fabs=False):
    """util::poseDifferenceLargerThan in fp32 as oracle/shim/Eigen evaluates it: norm() = sqrt(dx*dx + dy*dy); the heading
    difference wrapped once by -+2 pi in double; then the unqualified abs(), which this toolchain resolves to abs(int) --
    the difference truncated toward zero (fabs=True: fabsf, what the source means)."""
    p, q = np.asarray(p, f32), np.asarray(q, f32)
    if pose_distance(p, q) > f32(min_dist):
        return True
    with np.errstate(over="ignore"):
        ad = f32(p[2] - q[2])
    if float(ad) > math.pi:
        ad = f32(float(ad) - math.pi * 2.0)
    elif float(ad) < -math.pi:
        ad = f32(float(ad) + math.pi * 2.0)
    if fabs:
        return bool(abs(ad) > f32(min_angle))
    return bool(f32(abs(int(ad))) > f32(min_angle))


# ---- runners ---------------------------------------------------------------------------------------------------------------
class RefRun(NamedTuple):
    updated: np.ndarray   # [n_scans] bool
    poses: np.ndarray     # [n_scans, 3] float32: lastScanMatchPose after each scan
    covs: np.ndarray      # [n_scans, 3, 3]
    last_update: np.ndarray  # [n_scans, 3]: lastMapUpdatePose BEFORE each scan's gate
    planes: list          # log-odds plane per level at the end


_REF = {}


def reference_run(po, key, sc, upto=None):
    """The scenario through the reference's own HectorSlamProcessor (oracle/_ref), once per session."""
    k = (key, upto)
    if k not in _REF:
        proc = po.RefHectorProcessor(CELL, sc.n, sc.n, (0.5, 0.5), sc.levels, p_free=0.4, p_occ=0.9)
        proc.L.href_proc_set_update_thresholds(proc.h, sc.min_dist, sc.min_angle)
        est = np.zeros(3, f32)
        last = np.full(3, FLT_MAX, f32)
        upd, poses, covs, lasts = [], [], [], []
        for i, pts in enumerate(sc.containers[:upto]):
            hint = est if sc.hints is None else sc.hints[i]
            did = proc.update(pts, hint, map_without_matching=sc.no_match)
            est, cov = proc.last_pose()
            lasts.append(last.copy())
            if did:
                last = est.copy()
            upd.append(did)
            poses.append(est.copy())
            covs.append(cov.copy())
        planes = [proc.logodds(lv) for lv in range(sc.levels)]
        for p in planes:
            p.setflags(write=False)
        _REF[k] = RefRun(np.array(upd), np.array(poses), np.array(covs), np.array(lasts), planes)
        proc.close()
    return _REF[k]


def device_map(api, ctx, sc):
    m = api.OccGridMap(ctx, sc.n, sc.n, CELL, offset(sc.n), levels=sc.levels)
    m.setUpdateFreeFactor(0.4)
    m.setUpdateOccupiedFactor(0.9)
    return m


def hold_to_reference(tag, ref, rec, planes, upto=None):
    """The bounds of tests/test_ref_drives_gpu.py:193-225 for records and planes; prints what it finds first."""
    n = len(rec) if upto is None else upto
    dp = np.abs(rec["pose"][:n] - ref.poses[:n]).max()
    scale = np.maximum(1.0, np.abs(ref.covs[:n]).reshape(n, -1).max(axis=1))
    dc = (np.abs(rec["cov"][:n] - ref.covs[:n]).reshape(n, -1).max(axis=1) / scale).max()
    cells = [(int(np.count_nonzero(a != b)), int(np.count_nonzero(a))) for a, b in zip(ref.planes, planes)]
    print("%s: worst |pose - reference| = %.3g, worst covariance difference (relative) = %.3g, differing / non-zero cells per "
          "level = %s, updates = %d" % (tag, dp, dc, cells, int(ref.updated[:n].sum())))
    assert np.array_equal(rec["updated"][:n] != 0, ref.updated[:n]), (tag, rec["updated"][:n], ref.updated[:n])
    assert dp <= POSE_TOL, tag
    assert dc <= COV_TOL, tag
    for lv, (differing, nonzero) in enumerate(cells):
        assert differing <= CELLS_TOL * nonzero, (tag, lv, differing, nonzero)
    return dp, cells
