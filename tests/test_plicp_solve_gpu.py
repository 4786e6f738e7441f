"""The device's closed-form point-to-line solve (pl_solve in csrc/plicp.hip, through lslam_plicp_debug_iteration) against the
minimum of the cost it claims to minimise (tests/plicp_minimum.py), on the iterations of tests/plicp_solve_cases.py: large
residuals, where the Lagrange multiplier is far from zero.  The iteration's discrete decisions must be the restatement's
first, so that the device solves over the kept set the reference minimises over.

Bound.  Measured max |x_out - reference| on the MI355X over the cases: 8.4e-16 (solve_moved_object; 4.2e-17 .. 7.9e-16 on the
others: the device's sums are double, the reference's long double), allowed 8 x that, never above 1e-7.  The same cases
through a solve whose polynomial agrees with the Lagrange condition only at lambda = 0 miss by 2e-7 .. 5e-3
(tests/test_plicp_solve_oracle.py)."""
import math

import numpy as np
import pytest

import plicp_solve_cases as S
from lslam_amd import api

pytestmark = pytest.mark.gpu

MEASURED_DEVICE = 8.4e-16         # the measured maximum over S.IDS (see above)
DEVICE_BOUND = 8 * MEASURED_DEVICE
assert DEVICE_BOUND <= 1e-7


@pytest.fixture(scope="module")
def device(ctx):
    """Every (case, x_in) once, one matcher per laser: (name, k) -> debug_iteration's (j1, j2, flags, x_out)."""
    out, matchers = {}, {}
    try:
        for sc in S.cases():
            c = sc.case
            key = (id(c.laser), tuple(sorted(c.overrides.items())))
            if key not in matchers:
                matchers[key] = api.PlicpMatcher(ctx, api.plicp_params(**c.overrides), laser=c.laser)
            for k, x_in in enumerate(sc.x_ins):
                out[(sc.name, k)] = matchers[key].debug_iteration(c.ref, c.sens, x_in)
    finally:
        for m in matchers.values():
            m.close()
    return out


@pytest.mark.parametrize("name,k", S.IDS)
def test_device_solves_to_the_minimum_of_its_cost(device, name, k):
    pr = S.problem(name, k)
    j1, j2, flags, x_out = device[(name, k)]
    decided = ~pr.it.undecided
    assert np.array_equal(flags & 1, pr.it.flags & 1)
    assert np.array_equal(j1[decided], pr.it.j1[decided])
    assert np.array_equal(j2[decided], pr.it.j2[decided])
    assert np.array_equal(flags[decided], pr.it.flags[decided])
    d = np.abs(x_out - pr.x)
    d[2] = abs(math.remainder(x_out[2] - pr.x[2], 2 * math.pi))
    print(name, k, "max |x_out - reference|", d.max())
    assert d.max() <= DEVICE_BOUND, (name, k, d)
