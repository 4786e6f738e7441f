"""tools/plicp_cpu.py's closed-form point-to-line solve against the minimum of the cost it claims to minimise
(tests/plicp_minimum.py: long-double sums, the stationary angles of dC/dtheta by lattice and bisection, no quartic), on the
kept correspondences of the iterations of tests/plicp_solve_cases.py.  No GPU.

Bound.  Measured max |helper - reference| over the cases: 3.2e-15 (noisy_360_s0.002_0; 1.8e-16 .. 1.2e-15 on the others: the
helper's sums, its inverse and np.roots are double, the reference is long double), allowed 8 x that, never above 1e-9.  The
helper's cost is never above the reference's by more than 1e-12 of it.  A helper whose polynomial agrees with the Lagrange
condition only at lambda = 0 -- what `hp[0] ** 2 * p1 * p1` gave, which numpy turns into an element-wise product -- misses by
6.1e-5 .. 1.1e-3 on the new cases: test_polynomial_that_agrees_only_at_zero_misses_every_new_case keeps the cases able to
tell."""
import math

import numpy as np
import pytest

import plicp_minimum as M
import plicp_solve_cases as S
from tools import plicp_cpu as P

MEASURED_HELPER = 3.2e-15         # the measured maximum over S.IDS (see above)
HELPER_BOUND = 8 * MEASURED_HELPER
assert HELPER_BOUND <= 1e-9


def _pose_distance(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    d[2] = abs(math.remainder(a[2] - b[2], 2 * math.pi))
    return float(d.max())


@pytest.mark.parametrize("name,k", S.IDS)
def test_case_keeps_its_conditions(name, k):
    pr = S.problem(name, k)
    n_und = int(pr.it.undecided.sum())
    print(name, k, "kept", len(pr.p), "directions", S.directions(pr.nrm), "e0/e1", S.conditioning(pr.p, pr.q, pr.nrm),
          "gap", pr.gap, "undecided", n_und, pr.it.case_undecided)
    assert pr.it.sol is not None and pr.it.exit is None
    assert len(pr.p) >= S.MIN_KEPT
    assert S.directions(pr.nrm) >= S.MIN_DIRECTIONS
    assert S.conditioning(pr.p, pr.q, pr.nrm) >= S.MIN_CONDITIONING
    assert pr.gap >= S.MIN_GAP
    assert not pr.it.case_undecided
    assert n_und <= S.MAX_UNDECIDED


@pytest.mark.parametrize("name,k", S.IDS)
def test_helper_solves_to_the_minimum_of_its_cost(name, k):
    pr = S.problem(name, k)
    sol = P._solve_point_to_line(pr.p, pr.q, pr.nrm)
    assert sol is not None
    d = _pose_distance(sol, pr.x)
    c_helper = M.cost(sol, pr.p, pr.q, pr.nrm)
    print(name, k, "max |helper - reference|", d, "cost", c_helper, "reference", pr.cost)
    assert d <= HELPER_BOUND, (name, k, d)
    assert c_helper <= pr.cost * (1 + 1e-12) + 1e-300, (name, k, c_helper, pr.cost)


def test_restatement_solves_the_same_problem():
    """The kept correspondences rebuilt from the iteration's j1, j2 and flags are the ones the restatement solved."""
    for name, k in S.IDS:
        pr = S.problem(name, k)
        assert _pose_distance(P._solve_point_to_line(pr.p, pr.q, pr.nrm), pr.it.sol) <= 1e-12, (name, k)


def _solve_agreeing_only_at_zero(p, q, nrm):
    """The helper's solve with the polynomial (2L+2e0)^2 (2L+2e1)^2 - 4 (hp0^2+hp1^2) L - 4 (hp0^2 e1^2 + hp1^2 e0^2), which
    equals the Lagrange condition's only at L = 0, built from the helper's own e and hp; the root choice is the helper's."""
    ainv, bb, g, s2, h, e, v, hp = P._reduce_point_to_line(p, q, nrm)
    p0 = np.poly1d([2.0, 2.0 * e[0]])
    p1 = np.poly1d([2.0, 2.0 * e[1]])
    wrong = np.poly1d([4.0 * (hp[0] ** 2 + hp[1] ** 2), 4.0 * (hp[0] ** 2 * e[1] ** 2 + hp[1] ** 2 * e[0] ** 2)])
    best = None
    for lam in np.roots((p0 * p0 * p1 * p1 - wrong).coeffs):
        if abs(lam.imag) > 1e-9 * max(1.0, abs(lam.real)):
            continue
        u = v @ (-hp / (2.0 * e + 2.0 * lam.real))
        u = u / np.linalg.norm(u)
        cost = u @ s2 @ u + h @ u
        if best is None or cost < best[0]:
            best = (cost, u)
    u = best[1]
    t = -ainv @ (bb @ u + 0.5 * g[:2])
    return np.array([t[0], t[1], math.atan2(u[1], u[0])])


@pytest.mark.parametrize("name", S.NEW)
def test_polynomial_that_agrees_only_at_zero_misses_every_new_case(name):
    pr = S.problem(name, 0)
    old_miss = _pose_distance(_solve_agreeing_only_at_zero(pr.p, pr.q, pr.nrm), pr.x)
    print(name, "old polynomial misses the reference by", old_miss)
    assert S.by_name()[name].case.claim(old_miss), (name, old_miss)


def test_cases_are_all_there():
    assert [c.name for c in S.cases() if not c.new] == S.EXISTING
    assert len(S.NEW) == 6
    assert len(S.IDS) == len(S.EXISTING) + 3 * len(S.LATER_ITERATIONS) + len(S.NEW)
