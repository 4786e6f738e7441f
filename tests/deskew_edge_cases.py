"""Directed scenarios for the lesson5 de-skew (csrc/deskew.hip: k_deskew, k_deskew_batch, k_deskew_angles, the lslam_deskew
handle) and its consumer k_hector_cloud_container (csrc/logodds_map.hip), each built to sit on one branch or boundary that
the realistic sequences of tests/deskew_stream_cases.py never reach:

  imu_staging    five scans of one batch around the 256 IMU samples a block stages in LDS: 256, 257, 330, 12 and 300
                 samples -- one launch mixes the LDS and the HBM form, and the take-the-last-sample branch runs on the HBM form
  anchors        the first valid beam at 0, 255, 256, 511, 512, 599 and nowhere; one scan of 4097 beams (17 tiles) whose only
                 valid beam is the last
  window         readings exactly on range_min / range_max, one ulp outside, -inf, negative, NaN, +inf; +-0.0 with range_min
                 = 0; negative readings inside a window that starts below zero -- three geometries, so three calls
  epoch          edge_batch's scans 3, 4 and 5 at a ROS time base (1.7e9 s: one double ulp is 2.4e-7 s)
  mixed_flags    (use_imu, use_odom) = (1,1), (1,0), (0,1), (0,0), (1,1), (1,1) in one batch; the (0,1) scan owns no sample, the
                 (0,0) scan owns five that must be ignored
  cloud_filters  hand-made clouds for lslam_map_set_cloud: a point on, one ulp below and one ulp above every filter boundary,
                 non-finite coordinates, and keep patterns over clouds of 1 .. 3000 points for the compaction rounds of 1024

Every de-skew scenario follows deskew_stream_cases.edge_batch: 600 beams in a square room, a gyro with roll, pitch and yaw
rate, odometry with a z increment.  The room is 5 m x 5 m, half of edge_batch's: one ulp on each float32 cos / sin of every
transform, all at once, moves a coordinate by up to 5 ulps (tests/test_deskew_edges_oracle.py repeats the experiment; on
edge_batch's own 10 m room it gives 2.4e-6 m), and with every coordinate below 4 m, where one float32 ulp is 2.4e-7 m, that
is 1.2e-6 m: inside the 1.5e-6 m a scenario must leave under the 2e-6 m the device is held to.
A de-skew builder returns (ranges, params, imu_times, imu_rots, facts): one entry per scan (ranges is a list of float32
arrays -- a scenario may hold more than one geometry), facts["calls"] lists the scans that form one batched call each, the rest
of facts is what tests/test_deskew_edges_oracle.py asserts on the restatement alone.
Pure numpy plus the project's synth module and the api's parameter structs."""
import math

import numpy as np

from lslam_amd import api, synth

from deskew_restatement import restated_deskew

f32 = np.float32
N = 600
T0 = 2000.0
EPOCH_T0 = 1.7e9 + 0.123456
ODOM = (0.05, 0.012, 0.004)  # odom_incre_z is not zero
RANGE_MAX = 30.0
ROOM_HALF = 2.5


def laser(n=N):
    return synth.Laser(n_ranges=n, angle_min=math.radians(-135.0), angle_increment=math.radians(270.0 / n))


def room_ranges(k=0, n=N):
    """Scan k of the room: every beam returns (no dropout), every range below 3.95 m."""
    r = synth.cast_scan(synth.square_room(ROOM_HALF), (0.15 + 0.02 * k, -0.1 + 0.01 * k, 0.1 + 0.02 * k), laser(n), 0.01, 0.0,
                        np.random.default_rng(50 + k)).astype(f32)
    assert np.all(np.isfinite(r)) and 0.5 < r.min() and r.max() < 3.95
    return r


def params(t0, dt, n=N, use_imu=1, use_odom=1, range_min=None, range_max=RANGE_MAX, odom=ODOM):
    lz = laser(n)
    return api.DeskewParams(lz.angle_min, lz.angle_increment, lz.range_min if range_min is None else range_min, range_max, t0,
                            dt, int(use_imu), int(use_odom), t0 - 0.004, t0 + n * dt + 0.006, odom[0], odom[1], odom[2], 0.0)


def gyro(tau):
    """rad/s at tau seconds after the first sample: roll, pitch and yaw rate, none of them constant."""
    return np.array([0.2 * math.sin(40.0 * tau), -0.3 + 0.5 * tau, 0.6 + 2.0 * tau])


def integrate(times, rot0=(0.0, 0.0, 0.0)):
    """The integrated gyro samples PruneImuDeque would leave for these sample times."""
    rot = [list(rot0)]
    for k in range(1, len(times)):
        rot.append(list(np.array(rot[-1]) + gyro(times[k] - times[0]) * abs(times[k] - times[k - 1])))
    return rot


def khz(t_first, n, period=0.001):
    return [t_first + period * k for k in range(n)]


def beam_times(p, n=N):
    return p.scan_time_start + np.arange(n) * p.time_increment  # as the kernel computes them: t0 + i * dt in double


# ---- the scenarios -----------------------------------------------------------------------------------------------------------
STAGING_NAMES = ("lds256", "hbm257", "hbm330", "short12", "hbm300_short")


def imu_staging(t0=T0):
    t256 = khz(t0 - 0.003, 256)
    t257 = khz(t0 - 0.003, 257)
    t330 = khz(t0 - 0.003, 330)
    t12 = khz(t0 - 0.003, 12, 0.01)
    t300 = khz(t0 + 0.297 - 0.299, 300)
    times = [t256, t257, t330, t12, t300]
    sweeps = [0.2, 0.2, 0.3, 0.1, 0.33]  # hbm300_short: 0.55 ms per beam, the beams from 541 on lie beyond t0 + 0.297
    base = room_ranges(0)
    ranges = [base.copy(), base.copy(), room_ranges(2), room_ranges(3), room_ranges(4)]  # (lds256 and hbm257: the same scan)
    for r in ranges:
        r[7] = f32("nan")
    ps = [params(t0, s / N) for s in sweeps]
    rots = [integrate(t) for t in times]
    assert rots[0] == rots[1][:256]
    facts = {"calls": [list(range(5))], "names": STAGING_NAMES, "counts": [256, 257, 330, 12, 300]}
    return ranges, ps, times, rots, facts


ANCHORS = (0, 255, 256, 511, 512, 599, None)
LONG_N = 4097


def _blank(r, upto):
    """Everything before `upto` out of the window, in every way a reading can be."""
    junk = [f32("inf"), f32("nan"), f32(0.01), f32(45.0), f32("-inf"), f32(-1.0)]
    for i in range(upto):
        r[i] = junk[i % len(junk)]


def anchors(t0=T0):
    full = khz(t0 - 0.003, 12, 0.01)
    ranges, ps, times, rots = [], [], [], []
    for k, a in enumerate(ANCHORS):
        r = room_ranges(k)
        _blank(r, N if a is None else a)
        ranges.append(r)
        ps.append(params(t0, 0.1 / N))
        times.append(full)
        rots.append(integrate(full))
    r = room_ranges(1, LONG_N)
    _blank(r, LONG_N - 1)
    ranges.append(r)
    ps.append(params(t0, 0.1 / LONG_N, LONG_N))
    times.append(full)
    rots.append(integrate(full))
    facts = {"calls": [list(range(7)), [7]], "first_valid": list(ANCHORS) + [LONG_N - 1],
             "names": ["anchor_%s" % ("none" if a is None else a) for a in ANCHORS] + ["anchor_4096_of_4097"]}
    return ranges, ps, times, rots, facts


def window(t0=T0):
    full = khz(t0 - 0.003, 12, 0.01)
    ranges, ps, masks = [], [], []

    def scan(k, lo, hi, placed):
        """placed: {beam: (reading, valid)}; every other beam is inside the window."""
        r = room_ranges(k)
        want = np.ones(N, bool)
        for i, (v, ok) in placed.items():
            r[i] = v
            want[i] = ok
        ranges.append(r)
        ps.append(params(t0, 0.1 / N, range_min=lo, range_max=hi))
        masks.append(want)

    lo, hi = f32(0.2), f32(7.0)
    inf, up, down = f32("inf"), f32("inf"), f32("-inf")
    edge = {0: (lo, True), 1: (np.nextafter(lo, down), False), 10: (hi, True), 20: (np.nextafter(lo, down), False),
            30: (np.nextafter(hi, up), False), 40: (f32("-inf"), False), 50: (f32(-1.0), False), 60: (f32("nan"), False),
            70: (inf, False), 80: (np.nextafter(lo, up), True), 90: (np.nextafter(hi, down), True),
            # and across the tile edge of the block that finds the anchor and of the blocks that write
            255: (hi, True), 256: (np.nextafter(hi, up), False), 511: (np.nextafter(lo, down), False), 512: (lo, True),
            599: (hi, True)}
    scan(0, lo, hi, edge)
    zero = {0: (f32(-0.0), True), 3: (f32(0.0), True), 4: (f32(-0.0), True), 5: (np.nextafter(f32(0.0), down), False),
            6: (f32(1e-45), True), 300: (f32(0.0), True), 301: (f32(-1.0), False), 599: (f32(-0.0), True)}
    scan(1, f32(0.0), hi, zero)
    neg = {0: (f32(-1.0), True), 1: (np.nextafter(f32(-1.0), down), False), 2: (f32(-0.5), True), 3: (f32("-inf"), False),
           4: (f32(-0.0), True), 256: (f32(-1.0), True), 257: (f32(-1.5), False), 599: (np.nextafter(f32(-1.0), up), True)}
    scan(2, f32(-1.0), hi, neg)
    facts = {"calls": [[0], [1], [2]], "valid": masks, "names": ["window_0.2_7.0", "window_from_zero", "window_from_minus_one"]}
    return ranges, ps, [full] * 3, [integrate(full)] * 3, facts


EPOCH_NAMES = ("beams later than the last sample", "beam time equal to a sample time", "one non-monotone sample")


def epoch(t0=EPOCH_T0):
    """edge_batch's scans 3, 4 and 5 at a ROS stamp.  The first scan's samples start 3 ms AFTER the scan does, so its first
    beams take ComputeRotation's `f == 0` branch as well (edge_batch's start before the scan: no beam of it does)."""
    dt = 0.1 / N
    full = khz(t0 - 0.003, 12, 0.01)
    short = khz(t0 + 0.003, 6, 0.01)  # the last sample at t0 + 0.053: nearly half the beams lie beyond it
    exact = list(full)
    exact[4] = t0 + 240 * dt          # beam 240's time, computed as the kernel computes it
    bent = list(full)
    bent[5] = full[3] + 0.002         # goes back in time: the linear search stops where it stops
    times = [short, exact, bent]
    rots = [integrate(short, (0.01, -0.02, 0.03)), integrate(exact), integrate(bent)]
    ranges = [room_ranges(k) for k in range(3)]
    for r in ranges:
        r[7] = f32("nan")
    facts = {"calls": [[0, 1, 2]], "names": EPOCH_NAMES, "t0": t0, "dt": dt, "exact_beam": 240, "exact_sample": 4}
    return ranges, [params(t0, dt) for _ in range(3)], times, rots, facts


MIXED_FLAGS = ((1, 1), (1, 0), (0, 1), (0, 0), (1, 1), (1, 1))
MIXED_COUNTS = (12, 10, 0, 5, 11, 12)


def mixed_flags(t0=T0):
    ranges, ps, times, rots = [], [], [], []
    for k, ((ui, uo), c) in enumerate(zip(MIXED_FLAGS, MIXED_COUNTS)):
        r = room_ranges(k)
        r[7 + k] = f32("nan")
        r[0] = f32(0.01) if k % 2 else r[0]
        ranges.append(r)
        ps.append(params(t0 + 0.12 * k, 0.1 / N, use_imu=ui, use_odom=uo, odom=(0.05 + 0.01 * k, 0.012, 0.004 + 0.001 * k)))
        if c == 0:
            times.append(None)
            rots.append(None)
        elif not ui:  # samples a scan owns and does not use: large, so that reading them would show
            times.append(khz(t0 + 0.12 * k - 0.003, c, 0.01))
            rots.append([[1.0, -0.5, 0.7 + 0.1 * j] for j in range(c)])
        else:
            times.append(khz(t0 + 0.12 * k - 0.003, c, 0.01))
            rots.append(integrate(times[-1]))
    facts = {"calls": [list(range(6))], "flags": MIXED_FLAGS, "counts": MIXED_COUNTS,
             "names": ["imu%d_odom%d_%d_samples" % (ui, uo, c) for (ui, uo), c in zip(MIXED_FLAGS, MIXED_COUNTS)]}
    return ranges, ps, times, rots, facts


BUILDERS = {"imu_staging": imu_staging, "anchors": anchors, "window": window, "epoch": epoch, "mixed_flags": mixed_flags}
_SCN, _WANT = {}, {}


def scenario(name):
    """The scenario, built once per session and read-only from then on."""
    if name not in _SCN:
        out = BUILDERS[name]()
        for r in out[0]:
            r.setflags(write=False)
        _SCN[name] = out
    return _SCN[name]


def restate(p, r, times, rots):
    """restated_deskew for one scan of a scenario (a scan that owns no sample is given one it cannot read)."""
    return restated_deskew(r, p, times if times is not None else [0.0], rots if rots is not None else [[0.0, 0.0, 0.0]])


def restated(name):
    """[(xyz, valid)] per scan of the scenario by tests/deskew_restatement.py: computed once, shared by every test."""
    if name not in _WANT:
        ranges, ps, times, rots, _ = scenario(name)
        out = [restate(ps[k], ranges[k], times[k], rots[k]) for k in range(len(ps))]
        for w, v in out:
            w.setflags(write=False)
            v.setflags(write=False)
        _WANT[name] = out
    return _WANT[name]


def call_inputs(scn, idx):
    """The batched call over scans `idx` of a scenario -> (ranges [len(idx), n], params, imu_times, imu_rots)."""
    ranges, ps, times, rots, _ = scn
    return (np.stack([ranges[i] for i in idx]), [ps[i] for i in idx], [times[i] for i in idx], [rots[i] for i in idx])


# ---- cloud_filters -----------------------------------------------------------------------------------------------------------
Z_WINDOW = (0.5, 1.5)
LASER_POSES = {"identity": (0.0, 0.0, 0.0, 0.0), "posed": (0.21, -0.07, 0.35, 0.4)}


def _inexact_use_max():
    """A use_max whose square rounds UP in float32: d2 = (float)(u * u) is then above the double u * u the reference compares
    with (dropped), and not above the float32 product (a float32 comparison would keep it)."""
    for u in (3.3, 3.1, 3.2, 3.4, 3.6, 3.7):
        uf = float(f32(u))
        if float(f32(uf) * f32(uf)) > uf * uf:
            return u
    raise AssertionError("no candidate rounds up")


# min_dist, max_dist, use_max.  "issue": the configuration the cases were specified for (0.25, 16 and 9 are exact in float32).
# With use_max < max_dist a point next to sqr_max is dropped by use_max whatever sqr_max's comparison does, and with an exact
# use_max^2 the float32 and the double comparison agree; "far_use_max" and "inexact_use_max" make those two edges decide.
CLOUD_CFGS = {"issue": (0.5, 4.0, 3.0), "far_use_max": (0.5, 4.0, 5.0), "inexact_use_max": (0.5, 4.0, _inexact_use_max())}


def cloud_scan(cfg, pose):
    mn, mx, um = CLOUD_CFGS[cfg]
    return api.hector_scan(laser(), min_dist=mn, max_dist=mx, use_max=um, z_min=Z_WINDOW[0], z_max=Z_WINDOW[1],
                           laser_pose=LASER_POSES[pose])


def d2_of(x, y):
    return f32(f32(x) * f32(x)) + f32(f32(y) * f32(y))  # float32, products rounded before the sum (no contraction)


def point_with_d2(x, target):
    """(x, y >= 0) whose float32 x * x + y * y is exactly `target`."""
    x, target = f32(x), f32(target)
    rest = float(target) - float(f32(x * x))
    assert rest >= 0.0
    y = f32(math.sqrt(rest))
    cands = [y]
    lo = hi = y
    for _ in range(4096):
        lo, hi = np.nextafter(lo, f32("-inf")), np.nextafter(hi, f32("inf"))
        cands += [hi] + ([lo] if lo >= 0 else [])
    for c in cands:
        if d2_of(x, c) == target:
            return float(x), float(c)
    raise AssertionError("no y reaches d2 = %r from x = %r" % (target, x))


PASSING = (1.5, 1.0, 1.0)  # d2 = 3.25: inside every configuration's annulus, z inside the window


def named_points(cfg):
    """-> [(name, (x, y, z), valid, first failing test or None)] for the identity laser pose.  The z of a point that is not
    about z is 1.0; under the posed laser the z cases are decided by (float)((z + tz) - tz), so there the table holds for every
    point whose name does not start with "z_"."""
    mn, mx, um = CLOUD_CFGS[cfg]
    up, down = f32("inf"), f32("-inf")
    smin, smax = f32(mn) * f32(mn), f32(mx) * f32(mx)
    umf = f32(um)
    um2 = f32(umf * umf)  # d2 of the point (use_max, 0)
    um_exact = float(umf) * float(umf)
    P = []

    def add(name, x, y, z, fail, valid=1):
        P.append((name, (float(x), float(y), float(z)), valid, fail))

    def use_max_or(d2, otherwise=None):
        """What drops a point that passed the annulus and the x rule, if anything does."""
        return "use_max" if float(d2) > um_exact else otherwise

    add("sqr_min_at", mn, 0.0, 1.0, "annulus")
    add("sqr_min_below", *point_with_d2(np.nextafter(f32(mn), down), np.nextafter(smin, down)), 1.0, "annulus")
    add("sqr_min_above", *point_with_d2(mn, np.nextafter(smin, up)), 1.0, None)
    add("sqr_max_at", mx, 0.0, 1.0, "annulus")
    add("sqr_max_below", *point_with_d2(np.nextafter(f32(mx), down), np.nextafter(smax, down)), 1.0,
        use_max_or(np.nextafter(smax, down)))
    add("sqr_max_above", *point_with_d2(mx, np.nextafter(smax, up)), 1.0, "annulus")
    add("behind_at_half", -0.5, 0.5, 1.0, None)
    bx, by = point_with_d2(-0.5, np.nextafter(f32(0.5), down))
    add("behind_inside_half", bx, by, 1.0, "behind")
    add("behind_far", -1.5, 1.0, 1.0, None)
    add("plus_zero_x", 0.0, f32(0.7), 1.0, None)
    add("minus_zero_x", -0.0, f32(0.7), 1.0, None)
    in_annulus = lambda d2: smin < d2 < smax
    add("use_max_at", umf, 0.0, 1.0, use_max_or(um2) if in_annulus(um2) else "annulus")
    b = np.nextafter(um2, down)
    add("use_max_below", *point_with_d2(np.nextafter(umf, down), b), 1.0, use_max_or(b) if in_annulus(b) else "annulus")
    a = np.nextafter(um2, up)
    add("use_max_above", *point_with_d2(umf, a), 1.0, use_max_or(a) if in_annulus(a) else "annulus")
    zlo, zhi = f32(Z_WINDOW[0]), f32(Z_WINDOW[1])
    add("z_min_at", PASSING[0], PASSING[1], zlo, "z")
    add("z_min_inside", PASSING[0], PASSING[1], np.nextafter(zlo, up), None)
    add("z_min_outside", PASSING[0], PASSING[1], np.nextafter(zlo, down), "z")
    add("z_max_at", PASSING[0], PASSING[1], zhi, "z")
    add("z_max_inside", PASSING[0], PASSING[1], np.nextafter(zhi, down), None)
    add("z_max_outside", PASSING[0], PASSING[1], np.nextafter(zhi, up), "z")
    for c, cname in enumerate("xyz"):
        for v, vname in ((f32("nan"), "nan"), (f32("inf"), "plus_inf"), (f32("-inf"), "minus_inf")):
            p = list(PASSING)
            p[c] = v
            add("%s_%s" % (cname, vname), *p, "z" if cname == "z" else "annulus")
    add("passing", *PASSING, None)
    add("passing_but_invalid", *PASSING, "valid", valid=0)
    add("passing_again", 1.25, -1.0, 1.25, None)
    return P


def named_cloud(cfg):
    P = named_points(cfg)
    return (np.array([p[1] for p in P], f32), np.array([p[2] for p in P], np.uint8), [p[0] for p in P], [p[3] for p in P])


COMPACT_NS = (1, 1023, 1024, 1025, 2049, 3000)
COMPACT_PATTERNS = ("all", "none", "last", "first_of_round_2", "every_other", "random_30")


def keep_pattern(n, pattern):
    keep = np.zeros(n, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "first_of_round_2":
        if n <= 1024:
            return None  # there is no second round
        keep[1024] = True
    elif pattern == "every_other":
        keep[::2] = True
    elif pattern == "random_30":
        keep = np.random.default_rng(n).random(n) < 0.3
        keep[-1] = True  # (a last round of one point keeps it: kept points in every round)
    return keep


def compaction_clouds():
    """-> [(name, xyz [n, 3], valid [n], keep [n])]: points inside every filter where `keep`, and dropped in turn by valid = 0,
    the annulus, the z window and a NaN where not.  Ordered so that shorter clouds follow longer ones and sparse follow full."""
    out = []
    for n in (1025, 3000, 1, 2049, 1024, 1023):
        for pattern in COMPACT_PATTERNS:
            keep = keep_pattern(n, pattern)
            if keep is None:
                continue
            rng = np.random.default_rng(1000 + n)
            ang, rad = rng.uniform(-math.pi, math.pi, n), rng.uniform(0.8, 2.8, n)
            xyz = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(0.6, 1.4, n)], axis=1).astype(f32)
            valid = np.ones(n, np.uint8)
            drop = np.flatnonzero(~keep)
            valid[drop[0::4]] = 0
            xyz[drop[1::4], :2] *= f32(0.05)   # inside min_dist
            xyz[drop[2::4], 2] = f32(1.75)     # above the z window
            xyz[drop[3::4], 1] = f32("nan")
            out.append(("%d_%s" % (n, pattern), xyz, valid, keep))
    return out
