"""lesson5's synchronisation restated in Python (tests/msync_restatement.py) against the reference's own node
(oracle/_ref/liblesson5_ref.so through po.RefLesson5) on every scenario of tests/msync_cases.py -- which scans are corrected,
imu_time_ / imu_rot_* and odom_incre bit for bit (both sides use the host libm), the odometry stamps -- plus: every scenario is
what it claims, every switched mistake of the restatement gives another answer somewhere, and the scans left out of the
reference comparison are exactly the flagged ones of `no_lead` and `window_sizes`.  CPU only."""
import numpy as np
import pytest

import msync_cases as mc
import msync_restatement as mr


@pytest.fixture(scope="module")
def po(oracle_lib):
    if not oracle_lib.have_ref_lesson5():
        pytest.skip("oracle/_ref not built (needs the reference's sources at build time)")
    return oracle_lib


def combos(name):
    return mc.FLAG_COMBINATIONS if name == "flags" else ((True, True),)


def flagged(recs):
    return [k for k, r in enumerate(recs) if r["status"] in (mr.IMU_NO_LEAD_SAMPLE, mr.IMU_OVERFLOW)]


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_restatement_is_the_reference_node(po, name):
    case = mc.CASES[name]()
    assert 64 <= case["ranges"].shape[1] <= 360 and len(case["scan_t"]) <= 40
    assert np.abs(case["odom_pos"]).max() < 16.0
    for use_imu, use_odom in combos(name):
        recs = mr.run(case, use_imu=use_imu, use_odom=use_odom)
        refs = mc.run_reference(po, case, use_imu, use_odom)
        left_out = flagged(recs) + list(range(case["ref_callbacks"], len(recs)))
        compared = 0
        for k, (r, g) in enumerate(zip(recs, refs)):
            if k in left_out:
                continue
            assert (g is not None) == (r["status"] == mr.CORRECTED), (name, k, r["status"])
            if g is None:
                continue
            compared += 1
            assert g["scan_time_start"] == r["scan_time_start"] and g["time_increment"] == r["time_increment"], (name, k)
            if use_imu:
                assert len(g["imu_time"]) == r["n_imu"], (name, k)
                assert g["imu_time"].tobytes() == r["imu_time"].tobytes(), (name, k)
                assert g["imu_rot"].tobytes() == r["imu_rot"].tobytes(), (name, k)
            if use_odom:
                assert (g["start_odom_time"], g["end_odom_time"]) == (r["start_odom_time"], r["end_odom_time"]), (name, k)
                assert g["odom_incre"].tobytes() == r["odom_incre"].tobytes(), (name, k, g["odom_incre"], r["odom_incre"])
        assert compared >= 5, (name, compared)


def test_only_the_flagged_scans_are_left_out():
    """The reference's result is not defined for IMU_NO_LEAD_SAMPLE, and it may not be given the 2001-sample window; nothing
    else is excluded from the comparison above."""
    out = {}
    for name in sorted(mc.CASES):
        case = mc.CASES[name]()
        for use_imu, use_odom in combos(name):
            recs = mr.run(case, use_imu=use_imu, use_odom=use_odom)
            left = sorted(set(flagged(recs)) | set(range(case["ref_callbacks"], len(recs))))
            if left:
                out[name] = [(k, recs[k]["status"]) for k in left]
    assert out == {"no_lead": [(6, mr.IMU_NO_LEAD_SAMPLE)], "window_sizes": [(7, mr.IMU_OVERFLOW)]}, out


def statuses(name, **kw):
    return [r["status"] for r in mr.run(mc.CASES[name](), **kw)]


def test_every_scenario_is_what_it_claims():
    C, W = mr.CORRECTED, mr.WAIT_IMU
    assert statuses("steady") == [mr.QUEUED] + [C] * 13
    c = mc.CASES["interleaved"]()
    assert statuses("interleaved") == [mr.QUEUED] + [C] * 15
    assert len(set(np.diff(c["imu_seen"]))) > 2 and len(set(np.diff(c["odom_seen"]))) > 2
    assert not np.array_equal(c["imu_seen"] * len(c["odom_t"]), c["odom_seen"] * len(c["imu_t"]))
    # imu_gap: a refusal, then edge 1 (corrected, no sample), then the refusal of a front later than the start
    recs = mr.run(mc.CASES["imu_gap"]())
    st = [r["status"] for r in recs]
    edge1 = [k for k, r in enumerate(recs) if r["status"] == C and r["n_imu"] == 0]
    assert len(edge1) == 1 and W in st[:edge1[0]] and st[edge1[0] + 1] == W, st
    assert not recs[edge1[0]]["imu_rot"].size
    # no_lead: edge 2 once, and the scans around it are corrected
    st = statuses("no_lead")
    assert st.count(mr.IMU_NO_LEAD_SAMPLE) == 1 and set(st) == {mr.QUEUED, C, mr.IMU_NO_LEAD_SAMPLE}, st
    # sparse_odom: a stale end message (older than the start message) and a stale start message (popped already)
    c = mc.CASES["sparse_odom"]()
    recs = mr.run(c)
    assert all(r["status"] == C for r in recs[1:])
    assert any(0 <= r["end_odom_index"] < r["start_odom_index"] for r in recs)
    assert any(0 <= r["start_odom_index"] < r["odom_front"] for r in recs)
    assert any(r["end_odom_index"] == -1 and r["start_odom_index"] >= 0 for r in recs)  # and at first the default end message
    # default_start
    c = mc.CASES["default_start"]()
    recs = mr.run(c)
    assert c["odom_t"][0] == c["scan_t"][0] and recs[1]["status"] == C
    assert recs[1]["start_odom_index"] == -1 and recs[1]["start_odom_time"] == 0.0 and recs[1]["end_odom_index"] >= 0
    end3 = c["scan_t"][3] + float(c["scan_tinc"][3]) * 63.0
    assert recs[4]["end_odom_time"] == end3
    # front_strides
    recs = mr.run(mc.CASES["front_strides"]())
    assert all(r["status"] == C for r in recs[1:])
    assert tuple(np.diff([r["imu_front"] for r in recs])[1:]) == mc.FRONT_STRIDES
    # window_sizes
    recs = mr.run(mc.CASES["window_sizes"]())
    assert tuple(r["n_imu"] for r in recs[1:-1]) == mc.WINDOW_SIZES[:-1] and recs[-1]["status"] == mr.IMU_OVERFLOW
    assert mc.WINDOW_SIZES[-2:] == (mr.QUEUE_LENGTH, mr.QUEUE_LENGTH + 1)
    # non_monotone
    c = mc.CASES["non_monotone"]()
    assert (np.diff(c["imu_t"]) < 0).sum() == 1 and (np.diff(c["odom_t"]) < 0).sum() == 1
    st = statuses("non_monotone")
    assert W in st and mr.WAIT_ODOM in st and st.count(C) >= 5, st
    # epoch
    assert mc.CASES["epoch"]()["scan_t"].min() > 1.7e9 and statuses("epoch") == [mr.QUEUED] + [C] * 9
    # flags: the late odometry refuses a scan only where the odometry is used
    for use_imu, use_odom in mc.FLAG_COMBINATIONS:
        st = statuses("flags", use_imu=use_imu, use_odom=use_odom)
        assert (mr.WAIT_ODOM in st) == use_odom and W not in st, (use_imu, use_odom, st)
    # odom_wait: the IMU pops of a scan the odometry step refuses stay made
    recs = mr.run(mc.CASES["odom_wait"]())
    waits = [k for k, r in enumerate(recs) if r["status"] == mr.WAIT_ODOM]
    assert waits and all(recs[k]["imu_front"] > recs[k - 1]["imu_front"] and recs[k]["odom_front"] == recs[k - 1]["odom_front"]
                         for k in waits)


def answer(recs):
    return [(r["status"], r["scan_time_start"], r["imu_front"], r["odom_front"], r["start_odom_index"], r["end_odom_index"],
             r["imu_time"].tobytes(), r["imu_rot"].tobytes(), r["odom_incre"].tobytes()) for r in recs]


@pytest.mark.parametrize("mistake", mr.MISTAKES)
def test_each_mistake_gives_another_answer(mistake):
    shows = [name for name in sorted(mc.CASES) if answer(mr.run(mc.CASES[name](), mistakes=(mistake,))) != answer(mr.run(mc.CASES[name]()))]
    print(mistake, shows)
    assert shows, mistake


def test_the_libm_allowance_is_small():
    """odom_incre's allowance for another libm (tests/test_msync_gpu.py): per scan, from the restatement alone."""
    worst = 0.0
    for name in ("steady", "sparse_odom", "default_start"):
        for r in mr.run(mc.CASES[name]()):
            if r["status"] == mr.CORRECTED:
                a = mr.odom_increment_allowance(r["start_pose"], r["end_pose"])
                assert (a >= 0).all() and (a < 1e-3).all(), (name, a)  # (0 where start and end are one message)
                worst = max(worst, a.max())
    print("largest allowance (m):", worst)
    assert worst > 0
