"""The keyframe-odometry logs (tests/plicp_odometry_restatement.py) on the CPU alone: the 40-scan log drives every keyframe
rule, tracks the truth, and keeps every threshold comparison 1e-6 away from its threshold, so the device's flags can be
compared one for one (tests/test_plicp_odom_gpu.py).  No GPU."""
import math

import numpy as np
import pytest

import plicp_odometry_restatement as O

MARGIN = 1e-6


def _relative(poses, k):
    return O.mul(O.inv(tuple(poses[0])), tuple(poses[k]))


@pytest.mark.parametrize("which", ["keyframe", "offset"])
def test_the_log_drives_every_keyframe_rule(which):
    log, steps = O.run(which)
    assert len(steps) == 40 and steps[0].flags == 3
    assert all(s.valid == 1 for s in steps[1:])
    fresh = [bool(s.flags & 2) for s in steps]
    by = {"angle": 0, "count": 0, "distance": 0}
    count = 0
    for k, s in enumerate(steps[1:], 1):  # which rule fired, re-derived from the margins the restatement recorded
        m = {name: (v, t) for name, v, t in s.margins}
        count += 1
        if m["angle"][0] > m["angle"][1]:
            by["angle"] += 1
        elif count == 10:
            by["count"] += 1
            count = 0
        elif m["distance"][0] > m["distance"][1]:
            by["distance"] += 1
        else:
            assert not fresh[k]
            continue
        assert fresh[k]
    print(which, "keyframes by rule:", by)
    assert by["distance"] >= 3 and by["angle"] >= 2 and by["count"] >= 1
    assert any(fresh[1:15]) and any(fresh[15:28]) and any(fresh[28:])


@pytest.mark.parametrize("which", ["keyframe", "offset", "invalid"])
def test_every_threshold_comparison_keeps_its_margin(which):
    """NewKeyframeNeeded's angle and distance tests keep 1e-6 from their thresholds.  GetPrediction's speed test cannot: a
    robot that stands or turns on the spot has v = 0 +- the match's noise over dt, and 0 is exactly 1e-6 from the threshold
    1e-6, so no such speed can be 1e-6 clear of it.  What it must keep is the side it is on: the device's x differs from the
    restatement's by ~1e-11 (tests/test_plicp_gpu.py), its v = x / dt by ~1e-10 at dt = 0.1 s; half the threshold, 5e-7, is
    5 000 times that."""
    log, steps = O.run(which)
    kf = [abs(v - t) for s in steps for name, v, t in s.margins if name != "speed"]
    speeds = [v for s in steps for name, v, t in s.margins if name == "speed"]
    print(which, "closest keyframe comparison:", min(kf), "speeds nearest the threshold:", sorted(speeds, key=lambda v: abs(v - 1e-6))[:3])
    assert min(kf) >= MARGIN
    assert all(abs(v - 1e-6) >= 5e-7 for v in speeds), speeds


@pytest.mark.parametrize("which", ["keyframe", "offset"])
def test_the_restatement_tracks_the_truth(which):
    log, steps = O.run(which)
    worst = 0.0
    for k, s in enumerate(steps):
        want = _relative(log.poses, k)
        e = (s.base_in_odom[0] - want[0], s.base_in_odom[1] - want[1], math.remainder(s.base_in_odom[2] - want[2], 2 * math.pi))
        worst = max(worst, math.hypot(e[0], e[1]), abs(e[2]))
    print(which, "worst pose error:", worst)
    assert worst <= len(steps) * 1e-6


def test_the_invalid_log_has_an_invalid_match_that_leaves_the_pose():
    log, steps = O.run("invalid")
    bad = [k for k, s in enumerate(steps) if k and not s.valid]
    assert bad and bad[0] == 6
    assert steps[6].base_in_odom == steps[5].base_in_odom               # corr_ch = identity, the state untouched
    assert not steps[6].flags & 2 or steps[6].margins                   # NewKeyframeNeeded still ran (the count moved on)
    assert any(s.valid for s in steps[1:6])
