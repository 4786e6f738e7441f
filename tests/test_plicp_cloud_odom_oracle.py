"""The keyframe-odometry logs as clouds (tests/plicp_cloud_odometry_restatement.py) on the CPU alone: they still drive every
keyframe rule and keep their margins, a take pattern gives exactly the restatement over the taken scans, and the truth is
tracked.  No GPU.

Truth on float32 clouds: the worst pose error of the restatement over the 40-scan logs is 1.43e-7 (keyframe) and 1.41e-7 (offset),
m or rad, whichever is larger (printed below; WORST_TRUTH_ERROR holds the larger, rounded up); the device is allowed 2 x that."""
import numpy as np
import pytest

import plicp_cloud_odometry_restatement as CO
import plicp_odometry_restatement as O
from plicp_cloud_odometry_restatement import PATTERNS, WORST_TRUTH_ERROR, truth_error

MARGIN = 1e-6
SPEED_MARGIN = 1e-9


@pytest.mark.parametrize("which", ["keyframe", "offset"])
def test_the_cloud_log_drives_every_keyframe_rule(which):
    lg, steps = CO.run(which)
    assert len(steps) == 40 and steps[0].flags == 3 and all(s.valid == 1 for s in steps[1:])
    fresh = [bool(s.flags & 2) for s in steps]
    by = {"angle": 0, "count": 0, "distance": 0}
    count = 0
    for k, s in enumerate(steps[1:], 1):
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
    # and they are the ranges log's keyframes, one for one
    assert fresh == [bool(s.flags & 2) for s in O.run(which)[1]]


def test_the_invalid_cloud_log_has_an_invalid_match_that_leaves_the_pose():
    lg, steps = CO.run("invalid")
    assert [k for k, s in enumerate(steps) if k and not s.valid][0] == 6
    assert steps[6].base_in_odom == steps[5].base_in_odom and any(s.valid for s in steps[1:6])


def _margins(steps):
    steps = [s for s in steps if s is not None]
    kf = [abs(v - t) for s in steps for name, v, t in s.margins if name != "speed"]
    speeds = [v for s in steps for name, v, t in s.margins if name == "speed"]
    return min(kf), speeds


@pytest.mark.parametrize("which", ["keyframe", "offset", "invalid"])
def test_every_threshold_comparison_keeps_its_margin(which):
    closest, speeds = _margins(CO.run(which)[1])
    print(which, "closest keyframe comparison:", closest)
    assert closest >= MARGIN and all(abs(v - 1e-6) >= 5e-7 for v in speeds), (closest, speeds)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("which", ["keyframe", "offset"])
def test_a_take_pattern_is_the_restatement_over_the_taken_scans(which, pattern):
    lg, take, steps = CO.run_taken(which, pattern)
    assert [s is None for s in steps] == [t == 0 for t in take]
    kept = np.flatnonzero(take)
    only = CO.CloudOdometry(base_to_laser=lg.base_to_laser)              # a node that never saw the refused callbacks
    want = [only.process((lg.xyz[k], lg.valid[k]), lg.stamps[k]) for k in kept]
    got = [steps[k] for k in kept]
    for a, b in zip(got, want):
        assert (a.flags, a.valid, a.iterations, a.nvalid, a.base_in_odom) == (b.flags, b.valid, b.iterations, b.nvalid, b.base_in_odom)
        assert np.array_equal(a.x, b.x)
    assert got[0].flags == 3                                              # initialised by its first TAKEN scan
    assert all(s.valid == 1 for s in got[1:])
    closest, speeds = _margins(steps)
    near = min(abs(v - 1e-6) for v in speeds)
    print(which, pattern, "closest keyframe comparison:", closest, "closest speed to 1e-6:", near, "truth error:",
          truth_error(lg, [s and s.base_in_odom for s in steps]))
    # GetPrediction's speed test: on float32 clouds a standing robot's v = (match noise ~1e-7 m) / dt is of the threshold's size,
    # 1e-6, and with refusals in between comes as near as 3.6e-7 (measured, printed above), inside the 5e-7 the full logs keep.
    # What it must keep is its side: the device's x differs from the restatement's by
    # ~1e-12 (tests/test_plicp_cloud_gpu.py), its v = x / dt by ~1e-11 at dt = 0.1 s; 1e-9 is 100 times that.
    assert closest >= MARGIN and near >= SPEED_MARGIN, (closest, near)


def test_the_patterns_are_what_they_say():
    lg, steps = CO.run("keyframe")
    p = CO.patterns(40)
    assert p["first_two"][:3].tolist() == [0, 0, 1] and p["last"][-2:].tolist() == [1, 0]
    gap = np.flatnonzero(p["across_keyframe"] == 0)
    assert len(gap) == 5 and any(steps[k].flags & 2 for k in gap)       # a keyframe of the full run falls into the gap
    assert p["all_three"][[0, 1, 4, 8, 17, 39]].tolist() == [0] * 6     # and isolated refusals besides


@pytest.mark.parametrize("which", ["keyframe", "offset"])
def test_the_restatement_tracks_the_truth_on_clouds(which):
    lg, steps = CO.run(which)
    worst = truth_error(lg, [s.base_in_odom for s in steps])
    print(which, "worst pose error on float32 clouds:", worst)
    assert worst <= WORST_TRUTH_ERROR
