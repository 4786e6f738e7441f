"""tests/deskew_edge_cases.py held to what it claims, on the restatements alone (no GPU): every scenario has the property it
is named for, a deliberately wrong restatement gives another answer on it (a scenario no wrong kernel could fail is
worthless), the 2e-6 m the device is held to is reachable on it (one ulp on every float32 cos / sin moves the cloud by at
most 1.5e-6 m), and -- where the reference's own lesson5 is built -- the regime above 256 IMU samples is pinned to the
reference's own code.  Every test prints what it measured (pytest -s)."""
import math

import numpy as np
import pytest

from lslam_amd import api

import deskew_edge_cases as E
import deskew_restatement as R
from deskew_stream_cases import cloud_container

f32 = np.float32
SCALE = 1.0 / 0.05


@pytest.fixture(scope="module")
def po5(oracle_lib):
    if not oracle_lib.have_ref_lesson5():
        pytest.skip("oracle/_ref/liblesson5_ref.so not built (needs the reference's sources at build time)")
    return oracle_lib


# ---- a flag-switched copy of deskew_restatement.restated_deskew -----------------------------------------------------------
# One deliberate mistake at a time; `nudge` moves each of the six float32 cos / sin of every transform by one ulp at random;
# `trace[i]` receives the branch of ComputeRotation beam i took.  Without any of them it is restated_deskew, bit for bit.
DESKEW_MISTAKES = ("min_strict", "max_strict", "anchor_beam0", "no_rb", "clamp_off_by_one", "no_odom_z", "staging_cap_256",
                   "imu_flag_ignored")


def _get_transformation(x, y, z, roll, pitch, yaw, nudge):
    cs = [f32(math.cos(yaw)), f32(math.sin(yaw)), f32(math.cos(pitch)), f32(math.sin(pitch)), f32(math.cos(roll)),
          f32(math.sin(roll))]
    if nudge is not None:
        cs = [np.nextafter(v, f32("inf") if up else f32("-inf")) for v, up in zip(cs, nudge.random(6) < 0.5)]
    A, B, Cc, D, E_, F = cs
    DE, DF = D * E_, D * F
    L = np.array([[A * Cc, A * DF - B * E_, B * F + A * DE], [B * Cc, A * E_ + B * DF, B * DE - A * F], [-D, Cc * F, Cc * E_]],
                 dtype=np.float32)
    return L, np.array([x, y, z], dtype=np.float32)


def deskew_with(r, p, imu_time, imu_rot, mistake=None, nudge=None, trace=None):
    n = len(r)
    out = np.zeros((n, 3), np.float32)
    valid = np.zeros(n, bool)
    if imu_time is None:
        imu_time, imu_rot = [0.0], [[0.0, 0.0, 0.0]]
    last = len(imu_time) - 1
    if mistake == "clamp_off_by_one":
        last = max(last - 1, 0)
    if mistake == "staging_cap_256":
        last = min(last, 255)
    use_imu = p.use_imu or (mistake == "imu_flag_ignored" and last > 0)

    def transform_at(i):
        t = p.scan_time_start + i * p.time_increment
        rot = [f32(0)] * 3
        pos = [f32(0)] * 3
        if use_imu:
            f = 0
            while f < last:
                if t < imu_time[f]:
                    break
                f += 1
            if t > imu_time[f] or f == 0:
                rot = [f32(imu_rot[f][k]) for k in range(3)]
                if trace is not None:
                    trace[i] = "first" if not t > imu_time[f] else "last"
            else:
                b = f - 1
                rf = (t - imu_time[b]) / (imu_time[f] - imu_time[b])
                rb = (imu_time[f] - t) / (imu_time[f] - imu_time[b])
                if mistake == "no_rb":
                    rb = 0.0
                rot = [f32(imu_rot[f][k] * rf + imu_rot[b][k] * rb) for k in range(3)]
                if trace is not None:
                    trace[i] = ("between", b, f)
        if p.use_odom:
            rf = (t - p.start_odom_time) / (p.end_odom_time - p.start_odom_time)
            dz = 0.0 if mistake == "no_odom_z" else p.odom_incre_z
            pos = [f32(float(v) * rf) for v in (p.odom_incre_x, p.odom_incre_y, dz)]
        return _get_transformation(pos[0], pos[1], pos[2], float(rot[0]), float(rot[1]), float(rot[2]), nudge)

    start_inv = R.inverse(*transform_at(0)) if mistake == "anchor_beam0" else None
    for i in range(n):
        ri = r[i]
        lo, hi = f32(p.range_min), f32(p.range_max)
        below = ri <= lo if mistake == "min_strict" else ri < lo
        above = ri >= hi if mistake == "max_strict" else ri > hi
        if not np.isfinite(ri) or below or above:
            continue
        valid[i] = True
        a = float(f32(f32(p.angle_min) + f32(i) * f32(p.angle_increment)))
        px, py, pz = float(ri) * math.cos(a), float(ri) * math.sin(a), 1.0
        cur = transform_at(i)
        if start_inv is None:
            start_inv = R.inverse(*cur)
        L, t = R.mul(start_inv, cur)
        L, t = L.astype(np.float64), t.astype(np.float64)
        out[i] = [f32(((L[k, 0] * px + L[k, 1] * py) + L[k, 2] * pz) + t[k]) for k in range(3)]
    return out, valid


def run_with(name, **kw):
    ranges, ps, times, rots, _ = E.scenario(name)
    return [deskew_with(ranges[k], ps[k], times[k], rots[k], **kw) for k in range(len(ps))]


@pytest.mark.parametrize("name", list(E.BUILDERS))
def test_the_switched_copy_is_the_restatement(name):
    for (a, av), (b, bv) in zip(run_with(name), E.restated(name)):
        assert a.tobytes() == b.tobytes() and np.array_equal(av, bv)


# ---- the scenarios' own claims --------------------------------------------------------------------------------------------
def test_scenarios_follow_edge_batch():
    """600 beams in the 5 m room, gyro with roll, pitch and yaw, odometry with a z increment; one geometry per call."""
    for name in E.BUILDERS:
        ranges, ps, times, rots, facts = E.scenario(name)
        assert sorted(i for c in facts["calls"] for i in c) == list(range(len(ps))) and len(facts["names"]) == len(ps)
        for k, p in enumerate(ps):
            assert len(ranges[k]) in (E.N, E.LONG_N) and ranges[k].dtype == f32
            assert np.nanmax(np.where(np.isfinite(ranges[k]), ranges[k], 0)) < 45.5
            assert p.odom_incre_z != 0 and p.start_odom_time < p.scan_time_start < p.end_odom_time
            if p.use_imu:
                assert np.abs(np.asarray(rots[k])[-1]).min() > 1e-4, (name, k)  # roll, pitch and yaw all turned
        for c in facts["calls"]:
            g = {(ps[i].angle_min, ps[i].angle_increment, ps[i].range_min, ps[i].range_max, len(ranges[i])) for i in c}
            assert len(g) == 1
        for w, v in E.restated(name):  # every coordinate below 4 m: one float32 ulp is 2.4e-7 m (window: readings of 7 m)
            assert np.abs(w).max() < (4.0 if name != "window" else 7.1)


def test_imu_staging_claims():
    ranges, ps, times, rots, facts = E.scenario("imu_staging")
    want = E.restated("imu_staging")
    assert [len(t) for t in times] == facts["counts"] == [256, 257, 330, 12, 300]
    lds, hbm, big, _, short = range(5)
    for k in (lds, hbm):
        assert E.beam_times(ps[k]).max() < times[k][255]
    assert np.array_equal(ranges[lds], ranges[hbm], equal_nan=True)
    assert want[lds][0].tobytes() == want[hbm][0].tobytes() and np.array_equal(want[lds][1], want[hbm][1])
    trace = {}
    deskew_with(ranges[big], ps[big], times[big], rots[big], trace=trace)
    high = [i for i, b in trace.items() if b[0] == "between" and b[1] >= 256 and want[big][1][i]]
    beyond = int(np.count_nonzero((E.beam_times(ps[short]) > times[short][-1]) & want[short][1]))
    trace = {}
    deskew_with(ranges[short], ps[short], times[short], rots[short], trace=trace)
    took_last = sum(1 for i, b in trace.items() if b == "last" and want[short][1][i])
    print("hbm330: %d valid beams interpolate between samples of index >= 256; hbm300_short: %d valid beams later than the "
          "last sample (t0 + %.3f), %d take it" % (len(high), beyond, times[short][-1] - ps[short].scan_time_start, took_last))
    assert len(high) >= 50 and beyond >= 50 and took_last == beyond
    assert abs((times[short][-1] - ps[short].scan_time_start) - 0.297) < 1e-9


def test_anchor_claims():
    _, ps, _, _, facts = E.scenario("anchors")
    want = E.restated("anchors")
    firsts = [int(np.flatnonzero(v)[0]) if v.any() else None for _, v in want]
    print("first valid beams:", firsts)
    assert firsts == facts["first_valid"] == [0, 255, 256, 511, 512, 599, None, 4096]
    none = firsts.index(None)
    assert not want[none][0].any() and not want[none][1].any()
    assert len(want[7][1]) == 4097 == 16 * 256 + 1


def test_window_claims():
    ranges, ps, _, _, facts = E.scenario("window")
    want = E.restated("window")
    for k in range(3):
        assert np.array_equal(want[k][1], facts["valid"][k]), np.flatnonzero(want[k][1] != facts["valid"][k])
    r, p = ranges[0], ps[0]
    lo, hi = f32(p.range_min), f32(p.range_max)
    assert (lo, hi) == (f32(0.2), f32(7.0)) and r[0] == lo and want[0][1][0]  # the anchor sits on range_min
    bad = r[~want[0][1]]
    assert np.isnan(bad).any()
    for v in (np.nextafter(lo, f32(0)), np.nextafter(hi, f32(8)), -np.inf, -1.0, np.inf):
        assert float(v) in set(bad[~np.isnan(bad)].tolist())
    assert {float(lo), float(hi)} <= set(r[want[0][1]].tolist())
    z = ranges[1]
    assert ps[1].range_min == 0.0 and np.any((z == 0) & ~np.signbit(z) & want[1][1]) and np.any((z == 0) & np.signbit(z) & want[1][1])
    assert np.all(want[1][1][z == 0])
    assert ps[2].range_min == -1.0 and np.any((ranges[2] < 0) & want[2][1])
    assert len({(p.range_min, p.range_max) for p in ps}) == 3  # three geometries: three calls
    assert facts["calls"] == [[0], [1], [2]]


def test_epoch_claims():
    ranges, ps, times, rots, facts = E.scenario("epoch")
    want = E.restated("epoch")
    t0, dt = facts["t0"], facts["dt"]
    assert t0 == 1.7e9 + 0.123456 and np.spacing(t0) == 2.0 ** -22  # 2.4e-7 s per double ulp
    exact = times[1]
    assert exact[4] == t0 + 240 * dt and exact[3] < exact[4] < exact[5] and E.beam_times(ps[1])[240] == exact[4]
    assert want[1][1][240]
    assert np.any(np.diff(times[2]) < 0)
    taken = set()
    per_scan = []
    for k in range(3):
        trace = {}
        deskew_with(ranges[k], ps[k], times[k], rots[k], trace=trace)
        kinds = [b if isinstance(b, str) else "between" for i, b in trace.items() if want[k][1][i]]
        per_scan.append({s: kinds.count(s) for s in ("first", "between", "last")})
        taken |= set(kinds)
    print("valid beams per branch of ComputeRotation:", dict(zip(facts["names"], per_scan)))
    assert taken == {"first", "between", "last"}
    assert per_scan[0]["last"] > 200  # beams later than the last sample


def test_mixed_flags_claims():
    ranges, ps, times, rots, facts = E.scenario("mixed_flags")
    assert [(p.use_imu, p.use_odom) for p in ps] == [(1, 1), (1, 0), (0, 1), (0, 0), (1, 1), (1, 1)]
    counts = [0 if t is None else len(t) for t in times]
    assert counts == [12, 10, 0, 5, 11, 12]
    _, first, it, ir = api._deskew_inputs(ps, times, rots)
    assert first.tolist() == [0, 12, 22, 22, 27, 38, 50]  # the later scans' offsets depend on the two odd counts
    assert np.abs(np.asarray(rots[3])).min() >= 0.5       # what the (0,0) scan must ignore is not small
    want = E.restated("mixed_flags")
    w, v = want[3]  # the (0,0) scan: the plain projection
    a = (f32(ps[3].angle_min) + np.arange(E.N, dtype=f32) * f32(ps[3].angle_increment)).astype(np.float64)
    r = ranges[3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        plain = np.stack([(r * np.cos(a)).astype(f32), (r * np.sin(a)).astype(f32), np.ones(E.N, f32)], axis=1)
    plain[~v] = 0
    assert np.array_equal(w, plain)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------
SENSITIVE = [("window", "min_strict"), ("window", "max_strict"), ("anchors", "anchor_beam0"), ("anchors", "no_odom_z"),
             ("imu_staging", "no_rb"), ("imu_staging", "clamp_off_by_one"), ("imu_staging", "no_odom_z"),
             ("imu_staging", "staging_cap_256"), ("epoch", "no_rb"), ("epoch", "clamp_off_by_one"), ("epoch", "no_odom_z"),
             ("mixed_flags", "no_rb"), ("mixed_flags", "no_odom_z"), ("mixed_flags", "imu_flag_ignored")]


@pytest.mark.parametrize("name,mistake", SENSITIVE, ids=["%s-%s" % s for s in SENSITIVE])
def test_a_wrong_deskew_fails_the_scenario(name, mistake):
    """Another valid mask, or more than 2e-5 m (ten times the tolerance) on at least 10 beams of one scan."""
    assert mistake in DESKEW_MISTAKES
    facts = E.scenario(name)[4]
    masks, moved = [], []
    for (w, v), (g, gv) in zip(E.restated(name), run_with(name, mistake=mistake)):
        masks.append(not np.array_equal(v, gv))
        moved.append(int(np.count_nonzero(np.abs(w - g).max(axis=1) > 2e-5)) if not masks[-1] else 0)
    print("%s with %s: scans with another mask %s, beams moved by > 2e-5 m %s"
          % (name, mistake, [n for n, m in zip(facts["names"], masks) if m], dict(zip(facts["names"], moved))))
    assert any(masks) or max(moved) >= 10
    if mistake == "staging_cap_256":  # only the scans above 256 samples can tell
        assert [m >= 10 for m in moved] == [False, False, True, False, True]
    if mistake == "clamp_off_by_one" and name == "imu_staging":
        assert moved[4] >= 50
    if mistake == "anchor_beam0":
        assert moved[0] == 0 and min(moved[1:5]) >= 10


@pytest.mark.parametrize("name", list(E.BUILDERS))
def test_one_ulp_on_every_cos_and_sin_stays_inside_the_tolerance(name):
    """edge_batch's experiment on these scenarios: device and host differ in the last bit of the six float32 cos / sin of a
    transform; that may move the cloud by 1.5e-6 m at the most if 2e-6 m is to be a bound a right kernel meets."""
    worst = 0.0
    for seed in range(3):
        got = run_with(name, nudge=np.random.default_rng(700 + seed))
        for (w, v), (g, gv) in zip(E.restated(name), got):
            assert np.array_equal(v, gv)
            worst = max(worst, float(np.abs(w - g).max()))
    print("%s: one ulp on every cos / sin moves the cloud by %.3g m at the most" % (name, worst))
    assert worst <= 1.5e-6


# ---- the cloud container --------------------------------------------------------------------------------------------------
CONTAINER_MISTAKES = ("min_nonstrict", "max_nonstrict", "behind_x_nonstrict", "behind_half_nonstrict", "use_max_nonstrict",
                      "z_min_nonstrict", "z_max_nonstrict", "valid_ignored", "use_max_float32")


def container_with(xyz, valid, scan, scale_to_map, mistake=None, why=None):
    """A flag-switched copy of deskew_stream_cases.cloud_container; `why` receives the first failing test per point."""
    p = np.asarray(xyz, f32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    d2 = x * x + y * y
    smin, smax = f32(scan.sqr_laser_min_dist), f32(scan.sqr_laser_max_dist)
    with np.errstate(invalid="ignore"):
        ok_valid = np.ones(len(p), bool) if mistake == "valid_ignored" else np.asarray(valid, bool)
        ok_annulus = (d2 >= smin if mistake == "min_nonstrict" else d2 > smin) & (d2 <= smax if mistake == "max_nonstrict" else d2 < smax)
        behind = (x <= f32(0.0) if mistake == "behind_x_nonstrict" else x < f32(0.0)) & \
                 (d2 <= f32(0.5) if mistake == "behind_half_nonstrict" else d2 < f32(0.5))
        use_max = float(f32(scan.use_max_scan_range))
        if mistake == "use_max_float32":
            far = d2 > f32(scan.use_max_scan_range) * f32(scan.use_max_scan_range)
        elif mistake == "use_max_nonstrict":
            far = d2.astype(np.float64) >= use_max * use_max
        else:
            far = d2.astype(np.float64) > use_max * use_max
        yaw = float(f32(scan.laser_yaw))
        cy, sy = math.cos(yaw), math.sin(yaw)
        tx, ty, tz = (float(f32(v)) for v in (scan.laser_x, scan.laser_y, scan.laser_z))
        xd, yd, zd = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
        bx = (cy * xd + (-sy) * yd + 0.0 * zd) + tx
        by = (sy * xd + cy * yd + 0.0 * zd) + ty
        bz = (0.0 * xd + 0.0 * yd + 1.0 * zd) + tz
        zl = (bz - tz).astype(f32)
        zmin, zmax = f32(scan.laser_z_min), f32(scan.laser_z_max)
        ok_z = (zl >= zmin if mistake == "z_min_nonstrict" else zl > zmin) & (zl <= zmax if mistake == "z_max_nonstrict" else zl < zmax)
        keep = ok_valid & ok_annulus & ~behind & ~far & ok_z
        s = f32(scale_to_map)
        pts = np.stack([bx.astype(f32) * s, by.astype(f32) * s], axis=1)[keep]
    if why is not None:
        for i in range(len(p)):
            why.append("valid" if not ok_valid[i] else "annulus" if not ok_annulus[i] else "behind" if behind[i] else
                       "use_max" if far[i] else "z" if not ok_z[i] else None)
    return np.ascontiguousarray(pts, f32), keep


CLOUD_CASES = [(c, p) for c in E.CLOUD_CFGS for p in E.LASER_POSES]


@pytest.mark.parametrize("cfg,pose", CLOUD_CASES)
def test_named_points_are_kept_or_dropped_as_the_table_says(cfg, pose):
    xyz, valid, names, fails = E.named_cloud(cfg)
    scan = E.cloud_scan(cfg, pose)
    with np.errstate(invalid="ignore"):
        pts, origo = cloud_container(xyz, valid, scan, SCALE)
    why = []
    same, keep = container_with(xyz, valid, scan, SCALE, why=why)
    assert same.tobytes() == pts.tobytes() and len(pts) == keep.sum()  # the switched copy is the restatement
    table = dict(zip(names, fails))
    got = dict(zip(names, why))
    z_moved = []
    for k, name in enumerate(names):
        if pose == "posed" and name.startswith("z_"):
            # (float)((z + tz) - tz) need not be z: decided by the arithmetic, evaluated here with Python floats
            tz = float(f32(scan.laser_z))
            zl = f32((float(xyz[k, 2]) + tz) - tz)
            want = None if f32(E.Z_WINDOW[0]) < zl < f32(E.Z_WINDOW[1]) else "z"
            if not np.isnan(zl) and zl != xyz[k, 2]:
                z_moved.append(name)
            assert got[name] == want, (name, zl)
        else:
            assert got[name] == table[name], (name, xyz[k], got[name], table[name])
    print("%s, %s laser: %d of %d points kept; first failing test per point: %s; z changed by the round trip: %s"
          % (cfg, pose, len(pts), len(names), {w: why.count(w) for w in set(why)}, z_moved))
    assert set(why) == {None, "valid", "annulus", "behind", "use_max", "z"} or cfg == "far_use_max"
    assert {None, "valid", "annulus", "behind", "z"} <= set(why)
    if pose == "posed":
        assert np.abs(origo).min() > 1.0


def test_the_cases_of_the_issue_configuration():
    """min_dist 0.5, max_dist 4, use_max 3: the squares are exact in float32 and x = 0.5, 4, 3 reach them exactly."""
    xyz, valid, names, fails = E.named_cloud("issue")
    at = {n: k for k, n in enumerate(names)}
    d2 = xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]
    up, down = f32("inf"), f32("-inf")
    q = f32(0.25), f32(16.0), f32(9.0), f32(0.5)
    for stem, v in (("sqr_min", q[0]), ("sqr_max", q[1]), ("use_max", q[2])):
        assert d2[at[stem + "_at"]] == v and d2[at[stem + "_below"]] == np.nextafter(v, down)
        assert d2[at[stem + "_above"]] == np.nextafter(v, up)
    assert d2[at["behind_at_half"]] == q[3] and xyz[at["behind_at_half"], 0] == f32(-0.5)
    assert d2[at["behind_inside_half"]] == np.nextafter(q[3], down) and xyz[at["behind_inside_half"], 0] < 0
    for n in ("plus_zero_x", "minus_zero_x"):
        assert xyz[at[n], 0] == 0 and abs(float(d2[at[n]]) - 0.49) < 1e-7
    assert not np.signbit(xyz[at["plus_zero_x"], 0]) and np.signbit(xyz[at["minus_zero_x"], 0])
    kept = {n for n, f in zip(names, fails) if f is None}
    assert {"sqr_min_above", "behind_at_half", "plus_zero_x", "minus_zero_x", "use_max_at", "z_min_inside", "z_max_inside"} <= kept
    assert not kept & {"sqr_min_at", "sqr_min_below", "sqr_max_at", "sqr_max_above", "behind_inside_half", "use_max_above",
                       "z_min_at", "z_max_at", "passing_but_invalid"}
    assert not any(n[1:].startswith(("_nan", "_plus_inf", "_minus_inf")) and n in kept for n in names)
    assert sum(n[1:].startswith(("_nan", "_plus_inf", "_minus_inf")) for n in names) == 9
    # the two edges this configuration cannot decide are decided by the other two
    t = dict(zip(*E.named_cloud("far_use_max")[2:]))
    assert t["sqr_max_below"] is None and t["sqr_max_at"] == "annulus"
    t = dict(zip(*E.named_cloud("inexact_use_max")[2:]))
    assert t["use_max_at"] == "use_max" and t["use_max_below"] is None


@pytest.mark.parametrize("mistake", CONTAINER_MISTAKES)
def test_a_wrong_container_fails_the_named_points(mistake):
    changed = []
    for cfg, pose in CLOUD_CASES:
        xyz, valid, names, _ = E.named_cloud(cfg)
        scan = E.cloud_scan(cfg, pose)
        _, keep = container_with(xyz, valid, scan, SCALE)
        _, wrong = container_with(xyz, valid, scan, SCALE, mistake=mistake)
        changed.append(((cfg, pose), [n for n, a, b in zip(names, keep, wrong) if a != b]))
    print(mistake, "changes:", [c for c in changed if c[1]])
    assert any(c[1] for c in changed)
    assert dict(changed)[("issue", "identity")] or mistake in ("max_nonstrict", "use_max_float32")


def test_compaction_clouds_keep_what_they_say_in_every_round():
    clouds = E.compaction_clouds()
    seen = set()
    for pose in E.LASER_POSES:
        scan = E.cloud_scan("issue", pose)
        for name, xyz, valid, keep in clouds:
            pts, got = container_with(xyz, valid, scan, SCALE)
            assert np.array_equal(got, keep), (name, pose)
            with np.errstate(invalid="ignore"):
                assert cloud_container(xyz, valid, scan, SCALE)[0].tobytes() == pts.tobytes()
            n, pattern = name.split("_", 1)
            seen.add((int(n), pattern))
            if int(n) >= 1025 and pattern in ("all", "every_other", "random_30"):
                rounds = [int(keep[a:a + 1024].sum()) for a in range(0, len(keep), 1024)]
                assert min(rounds) >= 1, (name, rounds)
            if pattern == "first_of_round_2":
                assert np.flatnonzero(keep).tolist() == [1024]
            if pattern == "last":
                assert np.flatnonzero(keep).tolist() == [int(n) - 1]
    assert {n for n, _ in seen} == set(E.COMPACT_NS) and {p for _, p in seen} == set(E.COMPACT_PATTERNS)
    lengths = [len(c[1]) for c in clouds]
    assert any(a > b for a, b in zip(lengths, lengths[1:]))  # a shorter cloud follows a longer one


# ---- above 256 samples, against the reference's own code ---------------------------------------------------------------------
def _quat_yaw(yaw):
    return (0.0, 0.0, math.sin(0.5 * yaw), math.cos(0.5 * yaw))


def test_above_256_samples_the_restatement_equals_the_reference(po5):
    """A 0.3 s scan under a 1 kHz IMU through the reference's own callbacks: PruneImuDeque integrates more than 256 samples,
    and CorrectLaserScan's cloud is the restatement's to tests/test_deskew_pin.py's 1e-6 m, with equal valid masks."""
    lz = E.laser()
    r = E.room_ranges(0).copy()
    r[7] = f32("nan")
    r[0] = f32(0.01)
    r[40] = f32(45.0)
    t0, dur = 1000.0, 0.3
    node = po5.RefLesson5(True, True)
    for k in range(-30, 900):  # 1 kHz from 33 ms before the first scan to well after the second
        t = t0 - 0.0003 + 0.001 * k
        node.add_imu(t, tuple(E.gyro(0.001 * (k + 30))))
    for k in range(-3, 50):    # odometry at 50 Hz: a gentle arc
        t = t0 - 0.004 + 0.02 * k
        node.add_odom(t, (1.0 + 0.01 * k, 2.0 + 0.0004 * k * k, 0.0), _quat_yaw(0.3 + 0.02 * k))
    args = (lz.angle_min, lz.angle_increment, dur / E.N, lz.range_min, E.RANGE_MAX)
    assert node.scan(t0, *args, r) is None
    ref = node.scan(t0 + 0.4, *args, r[::-1].copy())
    node.close()
    assert ref is not None and np.array_equal(ref["ranges"], r, equal_nan=True)
    n_imu = len(ref["imu_time"])
    p = api.DeskewParams(ref["angle_min"], ref["angle_increment"], ref["range_min"], ref["range_max"], ref["scan_time_start"],
                         ref["time_increment"], 1, 1, ref["start_odom_time"], ref["end_odom_time"],
                         float(ref["odom_incre"][0]), float(ref["odom_incre"][1]), float(ref["odom_incre"][2]), 0.0)
    times, rots = list(ref["imu_time"]), [list(v) for v in ref["imu_rot"]]
    trace = {}
    want, want_valid = deskew_with(r, p, times, rots, trace=trace)
    again, _ = R.restated_deskew(r, p, times, rots)
    assert want.tobytes() == again.tobytes()
    high = sum(1 for i, b in trace.items() if b[0] == "between" and b[1] >= 256 and want_valid[i])
    d = np.abs(want - ref["xyz"])
    print("the reference integrated %d samples; %d valid beams interpolate between samples of index >= 256; worst "
          "|restatement - reference| = %.3g m, %.2f %% of the coordinates bit-equal" % (n_imu, high, d.max(), 100 * np.mean(d == 0)))
    assert n_imu > 256 and high >= 50
    assert np.array_equal(want_valid, ref["valid"]) and ref["valid"].sum() > 500
    assert d.max() <= 1e-6
    assert np.all(ref["xyz"][~ref["valid"]] == 0)
