"""Preconditions of tests/deskew_stream_cases.py, checked on the oracle alone (no GPU): the 12-scan sequence through the
reference's own LidarUndistortion has the properties the device tests rely on, the numpy restatement of the de-skew agrees
with the reference on every scan of it, and the numpy restatement of rosPointCloudToDataContainer (deskew_stream_cases.
cloud_container, written from lesson4/src/hector_mapping/hector_slam.cc:320-362; it lives in the support module because the
GPU tests hold lslam_map_set_cloud to it) keeps the points it should."""
import numpy as np
import pytest

from lslam_amd import synth

import deskew_stream_cases as D
from deskew_restatement import restated_deskew

f32 = np.float32


@pytest.fixture(scope="module")
def po5(oracle_lib):
    if not oracle_lib.have_ref_lesson5():
        pytest.skip("oracle/_ref/liblesson5_ref.so not built (needs the reference's sources at build time)")
    return oracle_lib


def test_sequence_has_the_properties_the_device_tests_need(po5):
    laser, seq = D.sequence12(po5)
    assert len(seq) == D.N_SCANS
    counts = [len(s["imu_time"]) for s in seq]
    firsts = [int(np.flatnonzero(s["valid"])[0]) for s in seq]
    valid = [int(s["valid"].sum()) for s in seq]
    print("IMU samples per scan:", counts, "first valid beam:", firsts, "valid beams:", valid)
    assert len(set(counts)) >= 3
    assert firsts[D.FRONT_GAP_SCAN] >= 256 and max(firsts[:D.FRONT_GAP_SCAN]) < 256
    assert min(valid) > 300
    for s in seq:  # one geometry: what a batched call requires
        assert (s["angle_min"], s["angle_increment"], s["range_min"], s["range_max"]) == \
               (seq[0]["angle_min"], seq[0]["angle_increment"], seq[0]["range_min"], seq[0]["range_max"])
        assert s["imu_time"][0] < s["scan_time_start"] and np.abs(s["imu_rot"][-1]).max() > 1e-3
        assert np.abs(s["odom_incre"][:2]).max() > 1e-3 and s["start_odom_time"] < s["scan_time_start"] < s["end_odom_time"]
    assert len({s["time_increment"] for s in seq}) == len(D.DURATIONS)


def test_restatement_equals_the_reference_on_every_scan(po5):
    """The bound tests/test_deskew_pin.py holds: <= 1e-6 m, > 99 % of the coordinates bit-equal."""
    _, seq = D.sequence12(po5)
    for k, s in enumerate(seq):
        want, want_valid = restated_deskew(s["ranges"], s["params"], s["times"], s["rots"])
        assert np.array_equal(want_valid, s["valid"]), k
        d = np.abs(want - s["xyz"])
        assert d.max() <= 1e-6, (k, d.max())
        assert np.mean(d == 0) > 0.99, (k, np.mean(d == 0))
        assert np.all(s["xyz"][~s["valid"]] == 0)


def test_cloud_container_restatement_and_the_z_window(po5):
    """lesson5 transforms (x, y, 1.0): with a window that contains 1 every scan keeps > 300 points, in beam order; the node's
    default window (-1, 1) drops them all."""
    laser, seq = D.sequence12(po5)
    scale = 1.0 / 0.05
    for s in seq:
        assert np.all(s["xyz"][s["valid"], 2] == 1.0)  # yaw rate only: exactly the 1.0 the reference transforms
        pts, origo = D.cloud_container(s["xyz"], s["valid"], D.hector_scan(laser, (-1.0, 2.0)), scale)
        assert len(pts) > 300 and origo.tolist() == [0.0, 0.0]
        none, _ = D.cloud_container(s["xyz"], s["valid"], D.hector_scan(laser, (-1.0, 1.0)), scale)
        assert len(none) == 0
    # identity laser pose: the container is the kept beams' (x, y) * scale, in order
    s = seq[0]
    sc = D.hector_scan(laser)
    pts, _ = D.cloud_container(s["xyz"], s["valid"], sc, scale)
    x, y = s["xyz"][:, 0], s["xyz"][:, 1]
    d2 = x * x + y * y
    keep = s["valid"] & (d2 > f32(sc.sqr_laser_min_dist)) & (d2 <= f32(20.0) * f32(20.0)) & ~((x < 0) & (d2 < f32(0.5)))
    assert np.array_equal(pts, np.stack([x[keep] * f32(scale), y[keep] * f32(scale)], axis=1))
    # and against the project's host evaluation of the node's own pre-processing of a raw scan (projectLaser's cloud has
    # z = 0, the window is the default): the same container, bit for bit
    r = s["ranges"]
    want, _ = synth.hector_project(r, laser, scale)
    a = np.float64(f32(laser.angle_min)) + np.arange(len(r), dtype=np.float64) * np.float64(f32(laser.angle_increment))
    ok = np.isfinite(r) & (r >= f32(laser.range_min)) & (r < f32(30.0))
    with np.errstate(invalid="ignore"):
        cloud = np.stack([(r.astype(np.float64) * np.cos(a)).astype(f32), (r.astype(np.float64) * np.sin(a)).astype(f32),
                          np.zeros(len(r), f32)], axis=1)
    cloud[~ok] = 0
    got, _ = D.cloud_container(cloud, ok, D.hector_scan(laser, (-1.0, 1.0)), scale)
    assert len(want) > 300 and np.array_equal(got, want)
