"""The batched lesson5 de-skew (lslam_deskew_batch[_dev], csrc/deskew.hip: k_deskew_batch, k_deskew_angles) on the device:
every scan of a batch against lslam_deskew_scan for that scan alone, bit for bit; the edge cases of
tests/deskew_stream_cases.py against the numpy restatement (tests/deskew_restatement.py, the 2e-6 m of
tests/test_deskew_gpu.py); the 12-scan sequence against the reference's own clouds (the 4e-6 m of tests/test_deskew_pin.py);
the _dev form, the empty call, buffer growth and mixed geometry."""
import math

import numpy as np
import pytest

from lslam_amd import api, synth

import deskew_stream_cases as D
from deskew_restatement import restated_deskew

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def po5(oracle_lib):
    if not oracle_lib.have_ref_lesson5():
        pytest.skip("oracle/_ref/liblesson5_ref.so not built (needs the reference's sources at build time)")
    return oracle_lib


@pytest.fixture(scope="module")
def deskewer(ctx):
    d = api.Deskewer(ctx)
    yield d
    d.close()


def _scans(n_readings, n_scans, use_imu, use_odom, stride):
    """n_scans scans of n_readings beams in rows of `stride` floats (the rest is NaN and must never be read as a beam), with
    IMU sample counts that differ from scan to scan."""
    laser = synth.Laser(n_ranges=n_readings, angle_min=math.radians(-135.0),
                        angle_increment=math.radians(270.0 / max(n_readings, 2)))
    world = synth.arena(size=40.0, n_axis=10, n_rot=4, seed=5)
    rng = np.random.default_rng(100 + n_readings)
    ranges = np.full((n_scans, stride), np.nan, f32)
    params, times, rots = [], [], []
    dur = 0.1
    for k in range(n_scans):
        r = synth.cast_scan(world, (0.3 + 0.05 * k, -0.2, 0.1 + 0.02 * k), laser, 0.01, 0.02, rng).astype(f32)
        if n_readings > 8:
            r[3] = f32("nan")
            r[0] = f32(0.01) if k % 2 else r[0]
        ranges[k, :n_readings] = r
        t0 = 1000.0 + 0.12 * k
        params.append(api.DeskewParams(laser.angle_min, laser.angle_increment, laser.range_min, 30.0, t0, dur / n_readings,
                                       int(use_imu), int(use_odom), t0 - 0.004, t0 + dur + 0.006, 0.05 + 0.01 * k, 0.012, 0.001 * k,
                                       0.0))
        if use_imu:
            n_imu = 11 - (k % 3)
            t = [t0 - 0.003 + 0.01 * j for j in range(n_imu)]
            rot = [[0.0, 0.0, 0.0]]
            for j in range(1, n_imu):
                rot.append(list(np.array(rot[-1]) + np.array([0.02 * math.sin(j + k), -0.03, 0.6 + 0.05 * j]) * 0.01))
            times.append(t)
            rots.append(rot)
        else:
            times.append(None)
            rots.append(None)
    return laser, ranges, params, times, rots


@pytest.mark.parametrize("n_scans", [1, 7])
@pytest.mark.parametrize("n_readings", [1, 63, 64, 65, 257, 1081])
@pytest.mark.parametrize("use_imu,use_odom", [(True, True), (True, False), (False, True)])
def test_batch_equals_single_bit_for_bit(ctx, deskewer, n_readings, n_scans, use_imu, use_odom):
    """1. xyz and valid of every scan of a batch == lslam_deskew_scan for that scan alone; rows wider than the scan."""
    _, ranges, params, times, rots = _scans(n_readings, n_scans, use_imu, use_odom, stride=n_readings + 5)
    xyz, valid = deskewer.batch(ranges, params, times, rots, n_readings=n_readings)
    assert xyz.shape == (n_scans, n_readings, 3) and valid.shape == (n_scans, n_readings)
    assert valid.sum() >= n_scans * n_readings * 0.8 - 2
    for k in range(n_scans):
        one, v1 = D.single(ctx, ranges[k, :n_readings], params[k], times[k], rots[k])
        assert np.array_equal(valid[k], v1), k
        assert xyz[k].tobytes() == one.tobytes(), (k, np.abs(xyz[k] - one).max())


def test_without_motion_data_the_cloud_is_the_projection(ctx, deskewer):
    """1. (both off) the output is ((float)(r cos a), (float)(r sin a), 1.0f) exactly, a in float32 then widened; a scan that
    does not use the IMU may own no sample."""
    laser, ranges, params, times, rots = _scans(1081, 3, False, False, stride=1081)
    xyz, valid = deskewer.batch(ranges, params, times, rots)
    a = (f32(laser.angle_min) + np.arange(1081, dtype=f32) * f32(laser.angle_increment)).astype(np.float64)
    assert a.dtype == np.float64 and np.all(a == a.astype(f32))
    for k in range(3):
        r = ranges[k].astype(np.float64)
        with np.errstate(invalid="ignore"):
            want = np.stack([(r * np.cos(a)).astype(f32), (r * np.sin(a)).astype(f32), np.ones(1081, f32)], axis=1)
        want[~valid[k]] = 0
        assert np.all(xyz[k][valid[k], 2] == 1.0)
        assert np.array_equal(xyz[k], want), np.abs(xyz[k] - want).max()
        one, _ = D.single(ctx, ranges[k], params[k], None, None)
        assert xyz[k].tobytes() == one.tobytes()


@pytest.fixture(scope="module")
def edge_run(deskewer):
    laser, ranges, params, times, rots = D.edge_batch()
    xyz, valid = deskewer.batch(ranges, params, times, rots)
    want = [restated_deskew(ranges[k], params[k], times[k], rots[k]) for k in range(len(params))]
    return ranges, params, times, rots, xyz, valid, want


@pytest.mark.parametrize("k", range(6), ids=[n.replace(" ", "_") for n in D.EDGE_NAMES])
def test_edge_cases_inside_one_batch(edge_run, k):
    """2. each scan of the edge batch against the numpy restatement: valid equal, <= 2e-6 m."""
    ranges, params, times, rots, xyz, valid, want = edge_run
    w, wv = want[k]
    assert np.array_equal(valid[k], wv)
    d = np.abs(xyz[k] - w).max()
    print("%s: %d valid beams, worst |device - restatement| = %.3g m" % (D.EDGE_NAMES[k], int(wv.sum()), d))
    assert d <= 2e-6
    assert np.all(xyz[k][~wv] == 0)
    if k == 0:
        assert not wv.any() and not xyz[k].any()
    elif k == 1:
        assert int(np.flatnonzero(wv)[0]) == 300
    else:
        assert wv.sum() > 500
    if k == 3:  # the beams beyond the last sample take its rotation: the scenario has such beams
        t_last = times[k][-1]
        assert np.count_nonzero(params[k].scan_time_start + np.arange(D.EDGE_N) * params[k].time_increment > t_last) > 200
    if k == 5:
        assert np.any(np.diff(times[k]) < 0)


def test_permuting_the_scans_permutes_the_outputs(deskewer, edge_run):
    ranges, params, times, rots, xyz, valid, _ = edge_run
    perm = [4, 0, 5, 2, 1, 3]
    xyz2, valid2 = deskewer.batch(ranges[perm], [params[i] for i in perm], [times[i] for i in perm], [rots[i] for i in perm])
    assert xyz2.tobytes() == xyz[perm].tobytes() and np.array_equal(valid2, valid[perm])


@pytest.mark.parametrize("use_imu,use_odom", [(True, True), (True, False), (False, True)])
def test_sequence_against_the_reference(po5, deskewer, use_imu, use_odom):
    """3. the 12 scans as ONE batch against the reference's own CorrectLaserScan: <= 4e-6 m (tests/test_deskew_pin.py)."""
    _, seq = D.sequence12(po5, use_imu, use_odom)
    ranges, params, times, rots = D.batch_inputs(seq)
    xyz, valid = deskewer.batch(ranges, params, times, rots)
    worst = 0.0
    for k, s in enumerate(seq):
        assert np.array_equal(valid[k], s["valid"]), k
        worst = max(worst, float(np.abs(xyz[k] - s["xyz"]).max()))
        assert np.all(xyz[k][~s["valid"]] == 0)
    print("12 scans, imu=%d odom=%d: worst |device - reference| = %.3g m" % (use_imu, use_odom, worst))
    assert worst <= 4e-6


def test_dev_form_empty_call_growth_and_mixed_geometry(ctx):
    """4. _dev == host form bit for bit and waits for nothing; n_scans == 0 launches nothing; a repeated call grows no buffer;
    a call with two geometries is refused."""
    _, ranges, params, times, rots = _scans(257, 5, True, True, stride=260)
    d = api.Deskewer(ctx)
    assert d.stats() == {"scans": 0, "launches": 0, "growths": 0, "host_waits": 0}
    xyz0, valid0 = d.batch(np.zeros((0, 257), f32), [], [], [], n_readings=257)
    assert xyz0.shape == (0, 257, 3) and d.stats()["launches"] == 0 and d.stats()["growths"] == 0
    xyz, valid = d.batch(ranges, params, times, rots, n_readings=257)
    st1 = d.stats()
    assert st1["scans"] == 5 and st1["launches"] == 2 and st1["growths"] > 0 and st1["host_waits"] == 1  # table + batch
    xyz_b, valid_b = d.batch(ranges, params, times, rots, n_readings=257)
    st2 = d.stats()
    assert xyz_b.tobytes() == xyz.tobytes() and np.array_equal(valid_b, valid)
    assert st2["growths"] == st1["growths"] and st2["launches"] == st1["launches"] + 1 and st2["host_waits"] == 2
    # the _dev form: buffers of the caller's, nothing waited for
    n, nr, stride = 5, 257, 260
    d_r, d_xyz, d_v = ctx.alloc(n * stride * 4), ctx.alloc(n * nr * 12), ctx.alloc(n * nr)
    try:
        ctx.upload(d_r, np.ascontiguousarray(ranges))
        for _ in range(2):  # the second call: same shape, nothing grows
            d.batch_dev(nr, d_r, stride, params, times, rots, d_xyz, d_v)
        st3 = d.stats()
        assert st3["host_waits"] == st2["host_waits"] and st3["launches"] == st2["launches"] + 2
        assert st3["growths"] == st2["growths"]  # a shape the handle has seen, through whichever form
        got, got_v = np.zeros((n, nr, 3), f32), np.zeros((n, nr), np.uint8)
        ctx.download(d_xyz, got)
        ctx.download(d_v, got_v)
        assert got.tobytes() == xyz.tobytes() and np.array_equal(got_v.astype(bool), valid)
    finally:
        for p in (d_r, d_xyz, d_v):
            ctx.free(p)
    # one call, one geometry: each of the four fields
    for field, value in (("angle_min", -1.0), ("angle_increment", 0.01), ("range_min", 0.2), ("range_max", 25.0)):
        bad = [api.DeskewParams.from_buffer_copy(p) for p in params]
        setattr(bad[3], field, value)
        launches = d.stats()["launches"]
        with pytest.raises(api.LslamError):
            d.batch(ranges, bad, times, rots, n_readings=257)
        assert d.stats()["launches"] == launches
    # a scan that uses the IMU must own a sample
    with pytest.raises(api.LslamError):
        d.batch(ranges, params, [None] + times[1:], [None] + rots[1:], n_readings=257)
    d.close()
