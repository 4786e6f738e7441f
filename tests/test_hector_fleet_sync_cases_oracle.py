"""The preconditions of tests/test_hector_fleet_sync_gpu.py, held on the CPU from hector_sync_cases.STATUSES alone (which
tests/test_hector_sync_cases_oracle.py holds to the restatement of lesson5's node): what the fleets of
tests/hector_fleet_sync_cases.py are said to contain is asserted here, not discovered on the GPU."""
import numpy as np

import hector_fleet_sync_cases as F
import hector_sync_cases as H


def test_the_members_of_ragged64_share_one_laser_header():
    headers = [tuple(float(v) for v in H.case(mb.log)["laser"]) for mb in F.members("ragged64")]
    assert headers[0] == headers[1] == headers[2], headers
    assert {H.case(mb.log)["ranges"].shape[1] for mb in F.members("ragged64")} == {64}
    for name in F.FLEETS:  # one n_readings and one header per fleet, and every member's log fits its steps
        assert len({H.case(mb.log)["ranges"].shape[1] for mb in F.members(name)}) == 1, name
        assert len({tuple(float(v) for v in H.case(mb.log)["laser"]) for mb in F.members(name)}) == 1, name
        assert all(mb.first + F.callbacks(mb) <= F.steps(name) for mb in F.members(name)), name
    assert H.case("wide")["ranges"].shape[1] == 1081 and H.case("imu_gap")["ranges"].shape[1] == 96


def test_what_the_steps_of_ragged64_hold():
    s, a = F.statuses("ragged64"), F.active("ragged64")
    assert s.shape == (14, 3)
    assert s[8].tolist() == [-2, -3, -4]  # three refusals of three kinds: nobody is taken
    assert any((row == 1).all() for row in s)  # some step takes everybody
    assert s[0].tolist() == [0, F.INACTIVE, F.INACTIVE]  # only a queued scan
    assert [int(np.flatnonzero(a[:, m])[0]) for m in range(3)] == [0, 2, 1]  # members 1 and 2 join after step 0
    assert [int(np.flatnonzero(a[:, m])[-1]) for m in range(3)] == [13, 11, 8]  # and leave before the end
    last2 = s[:, 2][a[:, 2]]
    assert last2[-1] == -4 and last2[-2] == 1  # member 2's last callback is refused
    # test 6: in steps [8, 10) members 0 and 2 have callbacks, all refused, and member 1 takes one; in [12, 14) 1 and 2 sit out
    assert (s[8:10, 0] < 0).all() and s[8:10, 2].tolist() == [-4, F.INACTIVE] and (s[8:10, 1] == 1).any()
    assert not a[12:14, 1:].any() and a[12:14, 0].all()
    assert {m.levels for m in F.members("ragged64")} == {2, 3} and len({m.map_n for m in F.members("ragged64")}) == 2


def test_every_refusal_kind_occurs_and_the_chunk_ends_fall_into_runs():
    kinds = set()
    for name in F.FLEETS:
        kinds |= {int(v) for v in F.statuses(name).ravel() if v < 0 and v != F.INACTIVE}
    assert kinds == {-1, -2, -3, -4}, kinds
    ends = np.cumsum(F.CHUNKS).tolist()
    assert ends == [1, 5, 6, 9, 14] and ends[-1] == F.steps("ragged64")
    s = F.statuses("ragged64")
    assert s[4, 0] < 0 and s[5, 0] < 0 and s[8, 0] < 0 and s[9, 0] < 0  # ends 5 and 9: inside member 0's runs of refusals
    assert (s[8] < 0).all() and ends[3] == 9  # ... and right behind the step that takes nobody
    assert 0 < F.CONTINUE_AT < 14 and F.active("ragged64")[F.CONTINUE_AT - 1].all() and F.active("ragged64")[F.CONTINUE_AT].all()
    assert {m.levels for m in F.members("wide2")} == {2, 3}


def test_step_arrays_and_spread_place_every_callback_at_its_step():
    r, t, ti, iseen, oseen, act = F.step_arrays("ragged64")
    assert r.shape == (14, 3, 64) and act.tolist() == F.active("ragged64").tolist()
    for m, mb in enumerate(F.members("ragged64")):
        c = H.case(mb.log)
        assert np.array_equal(t[act[:, m], m], c["scan_t"]) and np.array_equal(iseen[act[:, m], m], c["imu_seen"])
        assert np.array_equal(r[act[:, m], m], c["ranges"], equal_nan=True)
        assert not t[~act[:, m], m].any()
    part = F.step_arrays("ragged64", 5, 9)
    assert np.array_equal(part[1], t[5:9]) and np.array_equal(part[5], act[5:9])
    sp = F.spread("ragged64", [np.arange(F.callbacks(mb)) + 100 * m for m, mb in enumerate(F.members("ragged64"))], fill=-1)
    assert sp[:, 1].tolist() == [-1, -1] + list(range(100, 110)) + [-1, -1]
