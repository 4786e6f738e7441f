"""Preconditions of the fleets in tests/hector_fleet_cases.py, without a GPU: what tests/test_hector_fleet_gpu.py relies on when
it holds a fleet to its members run alone."""
import numpy as np
import pytest

import hector_fleet_cases as F

FLEETS = {"hetero": F.hetero, "rolled3": lambda: F.rolled(3), "rolled1": lambda: F.rolled(1), "mapping": F.mapping,
          "ragged": F.ragged}


@pytest.fixture(params=sorted(FLEETS))
def fleet(request):
    return FLEETS[request.param]()


def test_form_thresholds():
    """The register form's last and the staged form's first container length per LSLAM_GN_THREADS, restated."""
    assert F.REG_LIMIT == {256: 256 * 5, 512: 512 * 3, 1024: 1024 * 2} == {256: 1280, 512: 1536, 1024: 2048}
    for threads, limit in F.REG_LIMIT.items():
        assert F.form_of(threads, limit) == "reg%d" % threads
        assert F.form_of(threads, limit + 1) == "fast-lds"
        assert F.form_of(threads, 0) == "reg%d" % threads
    assert F.form_of(512, 7168) == "fast-lds" and F.form_of(512, 7169) == "fast-mem"
    assert 2 * 7168 * 4 == 56 * 1024


def test_shapes_and_active_steps(fleet):
    R = len(fleet.members)
    assert fleet.active.shape == (fleet.n_steps, R)
    assert fleet.active.any(axis=0).all()  # every member has at least one active step
    covered = sorted(k for lo, hi in fleet.calls for k in range(lo, hi))
    assert covered == list(range(fleet.n_steps))
    for r, m in enumerate(fleet.members):
        assert len(m.containers) == fleet.n_steps
        for k in range(fleet.n_steps):  # inactive entries have n_points == 0: there is no container at all
            assert (m.containers[k] is None) == (not fleet.active[k, r])
        if m.ranges is not None:
            assert m.ranges.shape[0] == fleet.n_steps and m.ranges.dtype == np.float32
        if m.hints is not None:
            assert np.asarray(m.hints).shape == (fleet.n_steps, 3)


def test_solo_and_fleet_calls_launch_the_same_form(fleet):
    """Per call of the scenario: the fleet call's capacity (its longest container; the readings in the ranges form) and every
    member's own selects the same form of the matcher, at every LSLAM_GN_THREADS -- the condition of the bit-equality
    contract."""
    for lo, hi in fleet.calls:
        cap = fleet.capacity(lo, hi)
        for threads in F.REG_LIMIT:
            for r, m in enumerate(fleet.members):
                solo = fleet.solo_capacity(r, lo, hi)
                if solo is not None:
                    assert F.form_of(threads, solo) == F.form_of(threads, cap), (lo, hi, r, solo, cap)
                if m.ranges is not None:
                    n_readings = m.ranges.shape[1]
                    assert F.form_of(threads, n_readings) == F.form_of(threads, cap)


def test_hetero_members_differ():
    fl = F.hetero()
    assert [(m.sc.n, m.sc.levels) for m in fl.members] == [(256, 3), (256, 1), (1024, 3)]
    counts = [len(c) for c in fl.members[0].containers]
    assert counts[F.S.EDGE_EMPTY] == 0 and [counts[k] for k in sorted(F.S.EDGE_COUNTS)] == [63, 64, 65, 1]
    assert max(counts) <= 90 < max(len(c) for c in fl.members[2].containers) <= 1081  # (of 1081 beams)
    assert fl.n_steps == 12


def test_rolled_members_differ():
    fl = F.rolled(3)
    for r in range(1, 3):
        assert not np.array_equal(fl.members[r].ranges, fl.members[0].ranges)
        assert np.array_equal(fl.members[r].ranges[0], fl.members[0].ranges[r])


def test_ragged_mask():
    fl = F.ragged()
    assert len(fl.members) == 5
    assert not fl.active[F.RAGGED_EMPTY_STEP].any()                       # one step with no active member
    assert fl.active[np.arange(len(fl.active)) != F.RAGGED_EMPTY_STEP].any(axis=1).all()
    member, call = F.RAGGED_IDLE
    lo, hi = fl.calls[call]
    assert not fl.active[lo:hi, member].any()                             # one member inactive for a whole call
    assert fl.active[:lo, member].any() or fl.active[hi:, member].any()
    for c, (lo, hi) in enumerate(fl.calls):                               # ... and nobody else is
        idle = [r for r in range(5) if not fl.active[lo:hi, r].any()]
        assert idle == ([member] if c == call else [])
    assert len({int(fl.active[:, r].sum()) for r in range(5)}) > 2        # different scan rates
