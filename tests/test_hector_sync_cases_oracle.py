"""The preconditions of tests/test_hector_sync_gpu.py, held on the CPU: the restatement of lesson5's node
(tests/msync_restatement.py, itself pinned to the reference's node by tests/test_msync_cases_oracle.py) gives exactly the
status rows of tests/hector_sync_cases.py on every log, so that the GPU tests' claims -- isolated refusals, runs of refusals
of both kinds, a refused last callback, a refusal right behind the first taken scan, chunk ends inside the runs -- are
asserted here, not discovered there."""
import numpy as np
import pytest

import hector_sync_cases as H
import msync_restatement as mr


@pytest.mark.parametrize("name", sorted(H.STATUSES))
def test_the_restatement_gives_the_status_rows(name):
    c = H.case(name)
    got = [int(r["status"]) for r in mr.run(c)]
    assert got == H.STATUSES[name], (name, got)
    assert len(got) == len(c["scan_t"]) == len(c["ranges"])


def test_what_the_rows_are_for():
    s = H.STATUSES
    assert all(row[0] == 0 and row[1] == 1 for row in s.values())  # callback 0 queues; the first taken scan is callback 1
    assert set(s["steady"][1:]) == {1} and set(s["wide"][1:]) == {1} and H.case("wide")["ranges"].shape == (6, 1081)
    g = s["imu_gap"]
    assert g[2] < 0  # right behind the first taken scan
    assert all(not (g[k] < 0 and g[k + 1] < 0) for k in range(len(g) - 1)) and sum(v < 0 for v in g) == 3  # isolated
    n = s["non_monotone"]
    assert n[4:6] == [-1, -1] and n[7:10] == [-1, -2, -2] and n[3] == n[6] == n[10] == 1  # runs of two and three, both kinds
    assert s["window_sizes"][-1] == -4 and s["window_sizes"][-2] == 1
    assert s["no_lead"].count(-3) == 1
    # the split of the chunking test: behind the queued callback, inside the first run, just past it, inside the second run
    ends = np.cumsum(H.CHUNKS).tolist()
    assert ends == [1, 5, 6, 9, 14] == ends[:4] + [len(n)]
    assert n[0] == 0 and n[4] < 0 and n[5] < 0 and n[6] == 1 and n[8] < 0 and n[9] < 0
    assert {len(p) for p in H.TAKE_PATTERNS.values()} == {12} and H.TAKE_PATTERNS["mixed"] == [1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 1, 0]
    assert set(H.LEVELS.values()) == {2, 3} and set(H.LEVELS) == set(s)
