"""The PL-ICP scenarios (tests/plicp_cases.py) on the CPU alone: the per-iteration restatement (tests/plicp_restatement.py)
iterated IS tools/plicp_cpu.py's sm_icp, every scenario is what it claims to be, and the discrete decisions of its first
iteration keep their distance from flipping -- so that a device result can be compared decision by decision
(tests/test_plicp_gpu.py).  No GPU."""
import numpy as np
import pytest

import plicp_cases as K
import plicp_restatement as R

UNDECIDED_CAP = 0.005  # of a case's sens readings


@pytest.mark.parametrize("name", K.NAMES)
def test_restatement_iterated_is_sm_icp(name):
    direct, res, its, near = K.expected(name)
    assert res["valid"] == direct["valid"] and res["iterations"] == direct["iterations"] and res["nvalid"] == direct["nvalid"]
    assert np.array_equal(res["x"], direct["x"])                       # exactly: the same expressions in the same order
    assert res["error"] == direct["error"]


@pytest.mark.parametrize("name", K.NAMES)
def test_case_is_what_it_claims(name):
    c = K.by_name()[name]
    direct, res, its, near = K.expected(name)
    assert c.claim(res, its[0], c), (name, res, its[0].exit)


@pytest.mark.parametrize("name", K.NAMES)
def test_decisions_keep_their_margins(name):
    c = K.by_name()[name]
    direct, res, its, near = K.expected(name)
    it1 = its[0]
    n_sens = int((it1.flags & 1).sum())
    n_und = int(it1.undecided.sum())
    print(name, "sens readings", n_sens, "undecided", n_und, "case-level", it1.case_undecided, "near epsilon", near)
    assert n_und <= UNDECIDED_CAP * max(n_sens, 1), (name, n_und, n_sens)
    assert not it1.case_undecided, (name, it1.case_undecided)           # an exit may not hang on a margin
    assert not res.get("valid_undecided", False), name                  # nor `valid`
    # the exits' counts: 3 survivors against 2 is an integer decision; what could move it are the readings counted above


def test_scenarios_are_all_there():
    assert K.SCENARIOS == sorted(["known_motion", "noisy", "identity", "guessed", "beam_counts", "holes", "far", "rejected",
                                  "too_few", "modes", "empty"])
    counts = {s: sum(c.scenario == s for c in K.cases()) for s in K.SCENARIOS}
    assert counts["known_motion"] == 16
    its = [K.expected(c.name)[0]["iterations"] for c in K.cases() if c.scenario == "noisy"]
    assert 10 in its, its                                               # pairs that run all 10 iterations
    quick = [K.expected(c.name)[0]["iterations"] for c in K.cases() if c.scenario == "known_motion"]
    assert max(quick) <= 5, quick
    for s in K.SCENARIOS:  # at most one case per scenario whose iteration count hangs on epsilon
        assert sum(K.expected(c.name)[3] for c in K.cases() if c.scenario == s) <= 1, s
