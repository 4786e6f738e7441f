"""Preconditions of the scenarios in tests/hector_stream_cases.py, checked on the reference's own HectorSlamProcessor
(oracle/_ref) alone, and the numpy restatement of the update gate against the reference's -- no GPU."""
import numpy as np
import pytest

from lslam_amd import synth

import hector_stream_cases as S


@pytest.fixture(scope="module")
def po(oracle_lib):
    if not oracle_lib.have_ref_hector():
        pytest.skip("oracle/_ref/libhector_ref.so not built (needs the reference's sources at build time)")
    return oracle_lib


def margins(ref, min_dist):
    d = np.array([S.pose_distance(p, q) for p, q in zip(ref.poses, ref.last_update)])
    return np.abs(d - np.float32(min_dist))


def test_chain60_decisions_are_well_separated(po):
    """(a): the reference makes 4-10 updates, leaves scans without one, and every scan's distance to lastMapUpdatePose is at
    least 1e-3 -- ten times the pose contract -- away from 0.4: no pose difference the contract allows flips a decision.
    The heading never decides: the chain turns by 0.24 rad in all, which abs(int) truncates to 0."""
    sc = S.chain60()
    ref = S.reference_run(po, "a", sc)
    assert 4 <= ref.updated.sum() <= 10 and not ref.updated.all()
    m = margins(ref, sc.min_dist)
    print("chain60: updates at", np.flatnonzero(ref.updated).tolist(), "smallest |distance - 0.4| =", m.min())
    assert m.min() >= S.GATE_MARGIN
    assert np.abs(ref.poses[:, 2]).max() < 1.0
    for k in range(len(ref.poses)):
        assert S.gate(ref.poses[k], ref.last_update[k], sc.min_dist, sc.min_angle) == ref.updated[k], k


def test_mapping25_updates_level_0_only(po):
    sc = S.mapping25()
    ref = S.reference_run(po, "b", sc)
    assert ref.updated.all() and ref.poses.tobytes() == sc.hints.tobytes()
    assert np.count_nonzero(ref.planes[0]) > 1000 and not ref.planes[1].any() and not ref.planes[2].any()


@pytest.mark.parametrize("levels", [1, 3])
def test_edges_are_what_they_claim(po, levels):
    """(c): the counts the projection yields, an empty scan that returns its hint and updates nothing, a lone beam that ends
    outside the map and moves nothing, decisions as far from the threshold as (a)'s, and updates with odd counts."""
    sc = S.edges(levels)
    assert sc.laser.n_ranges % 4 != 0
    counts = [len(c) for c in sc.containers]
    assert counts[S.EDGE_EMPTY] == 0 and not np.isfinite(sc.ranges[S.EDGE_EMPTY]).any()
    for k, want in S.EDGE_COUNTS.items():
        assert counts[k] == want, (k, counts[k])
    assert sorted(S.EDGE_COUNTS.values()) == [1, 63, 64, 65]
    for k, c in enumerate(sc.containers):  # the containers are the host evaluation of the device's projection
        assert c.tobytes() == synth.hector_project(sc.ranges[k], sc.laser, 1.0 / S.CELL)[0].tobytes()
    ref = S.reference_run(po, ("c", levels), sc)
    assert np.isfinite(ref.poses).all() and np.isfinite(ref.covs).all()
    e = S.EDGE_EMPTY
    assert ref.poses[e].tobytes() == ref.poses[e - 1].tobytes() and not ref.updated[e]
    assert ref.covs[e].tobytes() == ref.covs[e - 1].tobytes()
    lone = [k for k, v in S.EDGE_COUNTS.items() if v == 1][0]
    assert ref.poses[lone].tobytes() == ref.poses[lone - 1].tobytes()
    assert 2 <= ref.updated.sum() < len(ref.updated)
    m = margins(ref, sc.min_dist)[1:]
    print("edges, %d level(s): updates at" % levels, np.flatnonzero(ref.updated).tolist(), "smallest margin", m.min())
    assert m.min() >= S.GATE_MARGIN


def test_gate_restatement_equals_the_reference(po):
    """(d): the numpy gate equals href_pose_difference_larger_than on every row; the fabsf form differs from it exactly on
    the sub-radian heading rows."""
    differs = []
    for p, q, d, a, what in S.gate_table():
        want = po.href_pose_difference_larger_than(p, q, d, a)
        assert S.gate(p, q, d, a) == want, (what, want)
        if S.gate(p, q, d, a, fabs=True) != want:
            differs.append(what)
    assert sorted(differs) == sorted(w for _, _, _, _, w in S.gate_table() if w.startswith(S.SUB_RADIAN))
    assert len(differs) == 4
