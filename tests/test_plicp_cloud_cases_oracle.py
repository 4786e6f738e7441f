"""The cloud scenarios of PL-ICP (tests/plicp_cloud_cases.py) on the CPU alone: tools/plicp_cpu.py's cloud_to_ldp feeds sm_icp
the points as they stand, the per-iteration restatement iterated is sm_icp on them too, every scenario is what it claims, and
the new points() route is held to the old one bit for bit.  No GPU.

Known motions on float32 clouds: the worst error of sm_icp over the carried-over scenarios that know and recover their motion is
6.48e-8 (m or rad; r_known_motion_1081_5), against <= 1e-6 asserted for the ranges form; allowed here and on the device is
2 x 6.5e-8 = 1.3e-7 (plicp_cloud_cases.RECOVERY_BOUND)."""
import math

import numpy as np
import pytest

import plicp_cases as K
import plicp_cloud_cases as C
from tools import plicp_cpu as P


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_iterated_is_sm_icp_on_clouds(name):
    direct, res, its, near = C.expected(name)
    assert res["valid"] == direct["valid"] and res["iterations"] == direct["iterations"] and res["nvalid"] == direct["nvalid"]
    assert np.array_equal(res["x"], direct["x"]) and res["error"] == direct["error"]


@pytest.mark.parametrize("name", C.NAMES)
def test_case_is_what_it_claims(name):
    c = C.by_name()[name]
    direct, res, its, near = C.expected(name)
    assert c.claim(res, its[0], c), (name, res, its[0].exit)
    if c.same_as:  # exactly the result of the case it restates another way
        other = C.expected(c.same_as)[0]
        assert np.array_equal(other["x"], direct["x"]) and other["error"] == direct["error"]
        assert (other["valid"], other["iterations"], other["nvalid"]) == (direct["valid"], direct["iterations"], direct["nvalid"])
        assert np.array_equal(C.expected(c.same_as)[2][0].flags, its[0].flags)


def test_scenarios_are_all_there():
    assert C.SCENARIOS == sorted(set(K.SCENARIOS) | set(C.CLOUD_ONLY))
    assert [n[2:] for n in C.NAMES if n.startswith("r_")] == K.NAMES      # every ranges scenario is carried over
    assert {len(C.by_name()[f"tiles_{n}"].ref_xyz) for n in (255, 256, 257, 2048)} == {255, 256, 257, 2048}
    for side in ("ref", "sens"):
        assert [C.expected(f"few_{side}_{v}")[2][0].exit == "few_valid" for v in (0, 1, 2, 3)] == [True, True, True, False]


def test_carried_over_clouds_follow_the_stated_conversion():
    for c in K.cases():
        cc = C.by_name()["r_" + c.name]
        L = c.laser
        for ranges, xyz, valid in ((c.ref, cc.ref_xyz, cc.ref_valid), (c.sens, cc.sens_xyz, cc.sens_valid)):
            ldp = c.ldp(ranges)
            assert np.array_equal(valid, ldp.valid)                        # the node's rule
            pts = ldp.points()
            ok = ldp.valid == 1
            assert np.array_equal(xyz[ok, :2], pts[ok].astype(np.float32))  # computed in float64, then rounded
            assert not xyz[~ok].any() and not xyz[:, 2].any()              # invalid points are (0, 0, 0); z = 0


def test_known_motions_are_recovered_within_the_measured_bound():
    worst, at = 0.0, None
    for name in C.NAMES:
        if not C.recovering(name):
            continue
        c = C.by_name()[name]
        e = C.expected(name)[0]["x"] - c.truth
        w = max(math.hypot(e[0], e[1]), abs(math.remainder(e[2], 2 * math.pi)))
        if w > worst:
            worst, at = w, name
    print("worst error of sm_icp on the float32 clouds:", worst, at, "allowed:", C.RECOVERY_BOUND)
    assert sum(C.recovering(n) for n in C.NAMES) == 21
    assert worst <= C.WORST_MEASURED, (worst, at)                           # the figure the bound was derived from still stands
    assert C.RECOVERY_BOUND == 2 * C.WORST_MEASURED


@pytest.mark.parametrize("name", K.NAMES)
def test_the_points_route_is_the_ranges_route_bit_for_bit(name):
    """cloud_to_ldp of a ranges-built Ldp's own float64 points gives sm_icp's result on the ranges Ldp exactly."""
    c = K.by_name()[name]
    ref, sens = c.ldp(c.ref), c.ldp(c.sens)
    want = K.expected(name)[0]
    got = P.sm_icp(c.params(), P.cloud_to_ldp(ref.points(), ref.valid), P.cloud_to_ldp(sens.points(), sens.valid), c.guess)
    assert (got["valid"], got["iterations"], got["nvalid"]) == (want["valid"], want["iterations"], want["nvalid"])
    assert np.array_equal(got["x"], want["x"]) and got["error"] == want["error"]


def test_cloud_to_ldp_rules():
    xyz = np.array([[1, 2, np.nan], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0], [3, 4, 5], [-np.inf, np.nan, 1]], np.float32)
    ldp = P.cloud_to_ldp(xyz)
    assert ldp.valid.tolist() == [1, 0, 0, 1, 1, 0] and ldp.valid.dtype == np.int8
    assert np.array_equal(ldp.points()[[0, 3, 4]], np.array([[1.0, 2.0], [0.0, 0.0], [3.0, 4.0]])) and ldp.points().dtype == np.float64
    assert P.cloud_to_ldp(xyz, np.array([0, 1, 1, 1, 2, 1], np.uint8)).valid.tolist() == [0, 0, 0, 1, 1, 0]
    third = np.float32(1.0) / np.float32(3.0)
    assert P.cloud_to_ldp(np.array([[third, third, 0]], np.float32)).points()[0, 0] == float(third)   # widened, not recomputed
    old = P.laser_scan_to_ldp([1.0, 50.0, 2.0], 0.0, 0.1, 0.1, 30.0)
    assert old.xy is None and old.points().shape == (3, 2)                 # the ranges path is unchanged
