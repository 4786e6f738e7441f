"""tests/hector_loc_cases.py is what it claims, in numpy (no GPU): the forms its calls select on both sides of the comparison,
the take patterns, and which entries are empty, long and short."""
import numpy as np

import hector_fleet_cases as F
import hector_loc_cases as L
import hector_stream_cases as S
import hector_sync_cases as H


def test_log_order_is_a_permutation_with_long_empty_short_in_a_row():
    sc = S.edges(3)
    assert sorted(L.LOG_ORDER) == list(range(len(sc.containers)))
    n = [len(c) for c in sc.containers]
    a, b, c = L.LONG_EMPTY_SHORT
    assert n[a] > 64 and n[b] == 0 and n[c] == 1  # more than one wave of points, none, one
    for r in range(L.MAX_R):
        order = L.log_order(r)
        k = order.index(a)
        assert order[k:k + 3] == [a, b, c], (r, order)  # consecutive for every tracker: no roll wraps the three around the end
    assert sorted(n[k] for k in S.EDGE_COUNTS) == [1, 63, 64, 65]


def test_calls_are_1_2_7_and_2_steps_and_cover_the_log():
    assert [hi - lo for lo, hi in L.CALLS] == [1, 2, 7, 2]
    assert L.CALLS[0][0] == 0 and L.CALLS[-1][1] == len(L.LOG_ORDER)
    assert all(a[1] == b[0] for a, b in zip(L.CALLS, L.CALLS[1:]))
    for levels in (1, 3):
        for R in (1, 3, 5):
            fleet = L.logs(levels, R)
            assert fleet.active.shape == (12, R) and fleet.active.all()
            for r, mb in enumerate(fleet.members):
                assert mb.sc.levels == levels and mb.ranges.shape == (12, 90)
                assert [len(c) for c in mb.containers] == [len(mb.sc.containers[k]) for k in L.log_order(r)]
            # the ranges form's capacity is the laser's readings on both sides: the register form at every block size
            assert {F.form_of(t, 90) for t in (256, 512, 1024)} == {"reg256", "reg512", "reg1024"}


def test_form_cases_select_the_same_form_on_both_sides():
    for name, (threads, pad, form) in L.FORMS.items():
        fleet = L.form_logs(name)
        (lo, hi), = fleet.calls
        cap = fleet.capacity(lo, hi)
        assert F.form_of(threads, cap) == form, (name, cap)
        for r in range(L.FORM_R):
            assert F.form_of(threads, fleet.solo_capacity(r, lo, hi)) == form, (name, r)
        lens = {len(c) for mb in fleet.members for c in mb.containers}
        assert len(lens) > 1, name  # containers of more than one length in every call
        if pad is not None:
            assert cap == pad
    assert F.REG_LIMIT[512] < L.FORMS["lds512"][1] <= 2000
    assert L.FORMS["mem512"][1] > F.LDS_LIMIT
    assert max(len(c) for c in S.chain60().containers[:L.FORM_STEPS]) <= F.REG_LIMIT[256]


def test_ragged_mask_has_the_three_situations():
    fleet = F.ragged()
    assert not fleet.active[F.RAGGED_EMPTY_STEP].any()              # a step nobody takes
    idle, call = F.RAGGED_IDLE
    lo, hi = fleet.calls[call]
    assert not fleet.active[lo:hi, idle].any() and fleet.active[:lo, idle].any()   # idle for a whole call, after having run
    rates = fleet.active.sum(axis=0)
    assert len(set(rates.tolist())) >= 3                             # different rates


def test_take_logs_have_isolated_refusals_and_runs_of_refusals():
    a, b = (L.status_take(name) for name in L.TAKE_LOGS)
    runs = lambda t: [len(s) for s in "".join("x" if v else "." for v in t).split("x") if s]  # noqa: E731
    assert not a[0] and not b[0]                      # the first callback is only queued
    assert set(runs(a[1:])) == {1}                    # isolated
    assert {2, 3} <= set(runs(b[1:]))                 # runs
    assert len(H.TAKE_PATTERNS["mixed"]) == len(a)    # tracker 1's bytes in the two-tracker call over the first log


def test_far_hint_puts_every_point_out_of_bounds():
    sc = S.edges(3)
    h = L.hint_far(sc)
    reach = max(float(np.abs(c).max()) for c in sc.containers if len(c))
    for lv in range(sc.levels):
        scale = 1.0 / (S.CELL * 2 ** lv)
        centre = scale * float(h[0]) + scale * S.offset(sc.n)[0]
        assert centre - reach > sc.n / 2 ** lv  # the whole container lies right of the level's last column
