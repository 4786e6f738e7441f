"""The ICP scenarios (tests/icp_cases.py) on the CPU alone, by tools/icp_cpu.py: every scenario is what it claims to be, the
discrete decisions keep their distance from flipping -- so that a device result can be compared decision by decision
(tests/test_icp_gpu.py) -- and the helper switched to one mistake at a time changes the answer of at least one case.  No GPU.

A source point of an iteration is UNDECIDED when a target point with different coordinates lies within 1e-9 (1 + d2) of the
best; an iteration count is NEAR when |mse - prev| lies within 1e-15 of absolute_mse (orders of magnitude above the fp64
rounding of an mse of about 1e-3)."""
import numpy as np
import pytest

import icp_cases as K
from tools import icp_cpu as I

UNDECIDED_POINTS_CAP = 0.01   # of a case's source points
UNDECIDED_CASES_CAP = 0.25    # of the cases
CLEAN = ("identical", "rigid_copy", "stop_transform", "stop_abs_mse", "stop_rel_mse", "stop_iterations")


@pytest.mark.parametrize("name", K.NAMES)
def test_case_is_what_it_claims(name):
    c = K.by_name()[name]
    res = K.expected(name)
    print(name, {k: v for k, v in res.items() if k != "trace"}, "truth", c.truth)
    assert c.claim(res, c), name


@pytest.mark.parametrize("name", K.NAMES)
def test_decisions_keep_their_margins(name):
    c = K.by_name()[name]
    und, near = K.margins(name)
    n_und = int(und.any(axis=0).sum())
    print(name, "source points", c.n, "undecided", n_und, "near", near)
    assert n_und <= UNDECIDED_POINTS_CAP * c.n, (name, n_und, c.n)
    if name in CLEAN:
        assert n_und == 0 and not near, (name, n_und, near)


def test_few_cases_hang_on_a_margin():
    hanging = [n for n in K.NAMES if not K.decided(n)]
    print("cases with an undecided point or a near count:", hanging)
    assert len(hanging) <= UNDECIDED_CASES_CAP * len(K.NAMES), hanging
    total = sum(int(K.margins(n)[0].sum()) for n in K.NAMES)
    print("undecided (point, iteration)s in all:", total)


def test_scenarios_are_all_there():
    assert K.SCENARIOS == sorted(["sizes", "pairs", "identical", "all_invalid", "rigid_copy", "duplicates", "few", "gate",
                                  "first_guess", "skip_invalid", "stop_rules", "window"])
    assert [c.n for c in K.cases() if c.scenario == "sizes"] == list(K.SIZES)
    assert sorted(c.n for c in K.cases() if c.scenario == "pairs") == [64] * 3 + [360] * 3 + [1081] * 3
    states = {K.expected(c.name)["state"] for c in K.cases()}
    assert states == {I.STATE_ITERATIONS, I.STATE_TRANSFORM, I.STATE_ABS_MSE, I.STATE_REL_MSE, I.STATE_FEW}, states


def test_rigid_copy_is_recovered():
    res = K.expected("rigid_copy")
    e = np.abs(res["x"] - np.array(K.RIGID_TRUTH))
    print("rigid_copy: error", e, "iterations", res["iterations"], "state", res["state"])
    # (at the fixed point the last increment is rounding noise: exactly the identity, rule (b), or not, rule (c))
    assert e.max() < 1e-6 and res["iterations"] == 3 and res["state"] in (I.STATE_TRANSFORM, I.STATE_ABS_MSE)


def test_window_ends_are_exclusive():
    L = K.PK.LASER64
    r = K.window_scan(L)
    xyz, valid = K.cloud(L, r)
    nan_xyz, nan_valid = K.cloud(L, r, invalid_as_nan=1)
    assert np.array_equal(valid, nan_valid)
    assert list(valid[3:16]) == [0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert np.all(xyz[valid == 0] == 0.0) and np.all(np.isnan(nan_xyz[valid == 0]))
    assert np.array_equal(xyz[valid == 1], nan_xyz[valid == 1]) and np.all(xyz[:, 2] == 0.0)
    ang = np.float32(L.angle_min) + np.float32(5) * np.float32(L.angle_increment)
    assert xyz[5, 0] == np.float32(np.float64(r[5]) * np.cos(np.float64(ang)))


def _answer(res):
    return (tuple(res["x"]), res["iterations"], res["state"], res["ncorr"], res["converged"], res["mse"], res["fitness"],
            tuple(res["trace"][0].corr))


@pytest.mark.parametrize("mistake", I.MISTAKES)
def test_every_mistake_changes_an_answer(mistake):
    changed = [n for n in K.NAMES if K.by_name()[n].n <= 360 and _answer(K.expected(n, mistake)) != _answer(K.expected(n))]
    print(mistake, "changes", changed)
    assert changed, mistake
    # and it matters: a pose, a count or a state moves somewhere, not only an index among equal points
    moved = [n for n in changed if _answer(K.expected(n, mistake))[:5] != _answer(K.expected(n))[:5]]
    assert moved, mistake
