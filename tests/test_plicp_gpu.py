"""lesson3's PL-ICP on the device (csrc/plicp.hip, api.PlicpMatcher) against tools/plicp_cpu.py's sm_icp and its per-iteration
restatement (tests/plicp_restatement.py) on the scenarios of tests/plicp_cases.py: the discrete decisions of one iteration
reading by reading, the solved pose, the full runs, and the batch forms byte for byte.

Bounds.  x of one iteration (debug_iteration) against the restatement: measured max |device - restatement| over the cases
5.4e-13 (beam_counts_65; the sums are taken in another order, the 2x2 eigen-decomposition and the roots by other routes),
allowed 8 x that, as the solve's conditioning varies with the geometry; never above 1e-7.  Full runs: the project's contract,
1e-4 m / 1e-4 rad (measured 2.0e-13, on a 63-reading pair; 2.1e-14 on the full scans).  Known motions: 1e-6 m / 1e-6 rad, what
tests/test_plicp.py holds the CPU helper to."""
import math

import numpy as np
import pytest

import plicp_cases as K
from lslam_amd import api
from tools import plicp_cpu as P

pytestmark = pytest.mark.gpu

X_ITERATION_BOUND = 8 * 5.4e-13   # 8 x the measured maximum (see above)
assert X_ITERATION_BOUND <= 1e-7
X_CONTRACT = 1e-4


def _matcher(ctx, c):
    return api.PlicpMatcher(ctx, api.plicp_params(**c.overrides), laser=c.laser)


@pytest.fixture(scope="module")
def device(ctx):
    """Every case once: name -> (debug_iteration's (j1, j2, flags, x_out), the full run's record)."""
    out = {}
    for c in K.cases():
        m = _matcher(ctx, c)
        try:
            dbg = m.debug_iteration(c.ref, c.sens, c.guess)
            rec = m.match_batch(np.stack([c.ref, c.sens]), [0], [1], [c.guess])[0]
        finally:
            m.close()
        out[c.name] = (dbg, rec)
    return out


@pytest.mark.parametrize("name", K.NAMES)
def test_one_iteration_takes_the_restatements_decisions(device, name):
    c = K.by_name()[name]
    it1 = K.expected(name)[2][0]
    (j1, j2, flags, x_out), _ = device[name]
    decided = ~it1.undecided
    print(name, "undecided readings skipped:", int(it1.undecided.sum()))
    assert np.array_equal(flags & 1, it1.flags & 1)                    # validity has no margin
    assert np.array_equal(j1[decided], it1.j1[decided])
    assert np.array_equal(j2[decided], it1.j2[decided])
    assert np.array_equal(flags[decided], it1.flags[decided])
    if it1.sol is None:
        assert np.all(np.isnan(x_out)), (name, it1.exit, x_out)
    else:
        d = np.abs(x_out - it1.sol)
        d[2] = abs(math.remainder(x_out[2] - it1.sol[2], 2 * math.pi))
        print(name, "max |x_out - restatement|", d.max())
        assert d.max() <= X_ITERATION_BOUND, (name, d)


@pytest.mark.parametrize("name", K.NAMES)
def test_full_run_equals_sm_icp(device, name):
    direct, res, its, near = K.expected(name)
    rec = device[name][1]
    d = np.abs(rec["x"] - direct["x"])
    d[2] = abs(math.remainder(rec["x"][2] - direct["x"][2], 2 * math.pi))
    print(name, "iterations", int(rec["iterations"]), direct["iterations"], "max |x - sm_icp|", d.max(), "near epsilon", near)
    assert d[0] <= X_CONTRACT and d[1] <= X_CONTRACT and d[2] <= X_CONTRACT, (name, d)
    if near:  # a step landed within 1e-9 of epsilon: the iteration count is undecided, x is not
        return
    assert (int(rec["valid"]), int(rec["iterations"]), int(rec["nvalid"])) == (direct["valid"], direct["iterations"], direct["nvalid"])
    if direct["iterations"] == 0:
        assert math.isinf(rec["error"]) and np.all(rec["x"] == 0.0)   # sm_icp's early exits: the zero result
    else:
        assert rec["error"] == pytest.approx(direct["error"], rel=1e-6, abs=1e-12)


@pytest.mark.parametrize("name", [n for n in K.NAMES if n.startswith("known_motion")])
def test_known_motion_is_recovered(device, name):
    c = K.by_name()[name]
    rec = device[name][1]
    e = rec["x"] - c.truth
    print(name, "error", math.hypot(e[0], e[1]), abs(e[2]), "iterations", int(rec["iterations"]))
    assert rec["valid"] == 1 and math.hypot(e[0], e[1]) < 1e-6 and abs(math.remainder(e[2], 2 * math.pi)) < 1e-6


def test_exact_duplicates_tie_every_distance(ctx):
    """The same scan on both sides: every distance is exactly zero, so the trimmed cut falls among equals and goes by sens
    order here (numpy's sort leaves another subset; the counts and the answer are the same)."""
    c = K.by_name()["holes_ends"]
    ldp = c.ldp(c.ref)
    want = P.sm_icp(P.PlicpParams(), ldp, ldp)
    m = _matcher(ctx, c)
    try:
        rec = m.match_batch(np.stack([c.ref]), [0], [0])[0]
        j1, j2, flags, x_out = m.debug_iteration(c.ref, c.ref)
    finally:
        m.close()
    assert (rec["valid"], rec["iterations"], rec["nvalid"]) == (want["valid"], want["iterations"], want["nvalid"])
    assert np.abs(rec["x"]).max() < 1e-9 and np.abs(x_out).max() < 1e-9
    valid = np.flatnonzero(flags & 1)
    assert np.array_equal(j1[valid], valid)                             # every reading finds itself
    kept = np.flatnonzero(flags & 4)
    accepted = np.flatnonzero(flags & 2)
    assert len(kept) == want["nvalid"] and np.array_equal(kept, accepted[:len(kept)])  # the FIRST ones in sens order


# ---- batches -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scans360():
    cs = [c for c in K.cases() if c.scenario == "known_motion" and c.laser is K.LASER360]
    return np.stack([r for c in cs for r in (c.ref, c.sens)])            # 16 scans: (2k, 2k + 1) are a pair


def _pairs(n_pairs, n_scans):
    k = np.arange(n_pairs)
    ref = (2 * (k % (n_scans // 2))).astype(np.int32)
    return ref, ref + 1


@pytest.fixture(scope="module")
def m360(ctx):
    m = api.PlicpMatcher(ctx, laser=K.LASER360)
    yield m
    m.close()


@pytest.mark.parametrize("n_pairs", [1, 3, 67])
def test_a_pair_is_the_same_alone_and_in_a_batch(m360, scans360, n_pairs):
    ref, sens = _pairs(n_pairs, len(scans360))
    batch = m360.match_batch(scans360, ref, sens)
    assert np.all(batch["valid"] == 1)
    for b in sorted({0, n_pairs // 2, n_pairs - 1}):
        alone = m360.match_batch(scans360[[ref[b], sens[b]]], [0], [1])
        assert alone.tobytes() == batch[b:b + 1].tobytes(), b
    for b in range(n_pairs):  # the same pair at another position
        assert batch[b].tobytes() == batch[b % 8].tobytes()


def test_three_hundred_small_pairs_pass_the_cu_count(ctx):
    laser = K.LASER64
    rng = np.random.default_rng(21)
    scans = []
    for k in range(8):
        a, b, _ = K.pair(laser, rng, motion=(0.05, -0.03, 0.02))
        scans += [a, b]
    scans = np.stack(scans)
    ref, sens = _pairs(300, len(scans))
    m = api.PlicpMatcher(ctx, laser=laser)
    try:
        batch = m.match_batch(scans, ref, sens)
        firsts = m.match_batch(scans, ref[:8], sens[:8])
        for k in range(8):
            ldp = [P.laser_scan_to_ldp(scans[i], laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max)
                   for i in (2 * k, 2 * k + 1)]
            want = P.sm_icp(P.PlicpParams(), ldp[0], ldp[1])
            assert (firsts[k]["valid"], firsts[k]["iterations"], firsts[k]["nvalid"]) == (want["valid"], want["iterations"],
                                                                                        want["nvalid"])
            assert np.abs(firsts[k]["x"] - want["x"]).max() <= X_CONTRACT
    finally:
        m.close()
    for b in range(300):
        assert batch[b].tobytes() == firsts[b % 8].tobytes(), b


def test_host_form_equals_dev_form(ctx, m360, scans360):
    ref, sens = _pairs(67, len(scans360))
    guess = np.zeros((67, 3))
    guess[:, 0] = 0.01
    host = m360.match_batch(scans360, ref, sens, guess)
    p_r, p_g, p_o = ctx.alloc(scans360.nbytes), ctx.alloc(guess.nbytes), ctx.alloc(67 * 48)
    try:
        ctx.upload(p_r, scans360)
        ctx.upload(p_g, guess)
        before = m360.stats()
        m360.match_batch_dev(len(scans360), 360, p_r, 360, ref, sens, p_g, p_o)
        after = m360.stats()
        ctx.synchronize()
        dev = np.zeros(67, api.PLICP_RECORD)
        ctx.download(p_o, dev)
        assert after["host_waits"] == before["host_waits"], "the _dev form makes no host wait"
        assert after["launches"] == before["launches"] + 1 and after["pairs"] == before["pairs"] + 67
        assert dev.tobytes() == host.tobytes()
        m360.match_batch_dev(len(scans360), 360, p_r, 360, ref, sens, None, p_o)   # NULL first guess = zeros
        ctx.synchronize()
        ctx.download(p_o, dev)
        assert dev.tobytes() == m360.match_batch(scans360, ref, sens).tobytes()
    finally:
        for p in (p_r, p_g, p_o):
            ctx.free(p)


def test_match_consecutive_is_match_batch(m360, scans360):
    k = np.arange(len(scans360) - 1, dtype=np.int32)
    assert m360.match_consecutive(scans360).tobytes() == m360.match_batch(scans360, k, k + 1).tobytes()
    wide = np.full((len(scans360), 400), 7.0, np.float32)                 # a stride beyond the scan: the tail is not read
    wide[:, :360] = scans360
    assert m360.match_consecutive(wide, n_readings=360).tobytes() == m360.match_batch(scans360, k, k + 1).tobytes()


def test_refusals_leave_the_outputs_untouched(ctx, m360, scans360):
    sentinel = np.frombuffer(bytes(range(48)) * 2, api.PLICP_RECORD).copy()
    for ref, sens in (([0, 16], [1, 1]), ([0, 0], [1, -1])):
        out = sentinel.copy()
        with pytest.raises(api.LslamError) as e:
            m360.match_batch(scans360, ref, sens, out=out)
        assert e.value.code == -1 and out.tobytes() == sentinel.tobytes()
    out = sentinel.copy()
    with pytest.raises(api.LslamError) as e:
        m360.match_batch(np.ones((2, 2049), np.float32), [0, 0], [1, 1], out=out)
    assert e.value.code == -8 and out.tobytes() == sentinel.tobytes()
    bare = api.PlicpMatcher(ctx)                                          # no laser set
    try:
        with pytest.raises(api.LslamError) as e:
            bare.match_batch(scans360, [0, 0], [1, 1], out=out)
        assert e.value.code == -1 and out.tobytes() == sentinel.tobytes()
        with pytest.raises(api.LslamError) as e:
            bare.debug_iteration(scans360[0], scans360[1])
        assert e.value.code == -1
    finally:
        bare.close()
    L, r = m360.L, np.ascontiguousarray(scans360)
    idx = np.zeros(2, np.int32)
    for args in ((None, 360, 2, idx.ctypes.data, idx.ctypes.data, out.ctypes.data), (r.ctypes.data, 360, 2, None, idx.ctypes.data, out.ctypes.data),
                 (r.ctypes.data, 360, 2, idx.ctypes.data, idx.ctypes.data, None), (r.ctypes.data, 100, 2, idx.ctypes.data, idx.ctypes.data, out.ctypes.data)):
        assert L.lslam_plicp_match_batch(m360.h, 16, 360, args[0], args[1], args[2], args[3], args[4], None, args[5]) == -1
    assert out.tobytes() == sentinel.tobytes()
    before = m360.stats()
    assert len(m360.match_batch(scans360, [], [])) == 0 and m360.stats() == before   # n_pairs == 0 launches nothing


def test_repeated_shape_allocates_nothing(ctx, scans360):
    m = api.PlicpMatcher(ctx, laser=K.LASER360)
    try:
        ref, sens = _pairs(67, len(scans360))
        first = m.match_batch(scans360, ref, sens)
        s1 = m.stats()
        second = m.match_batch(scans360, ref, sens)
        s2 = m.stats()
        assert first.tobytes() == second.tobytes()
        assert s1["growths"] > 0 and s2["growths"] == s1["growths"]
        assert (s1["host_waits"], s2["host_waits"]) == (1, 2), "the host form waits once, at its end"
        assert (s1["launches"], s2["launches"]) == (1, 2) and s2["pairs"] == 134
        m.match_batch(scans360, ref[:5], sens[:5])                        # a smaller batch fits what is there
        assert m.stats()["growths"] == s1["growths"]
    finally:
        m.close()


def test_zero_iterations_return_the_first_guess(ctx):
    c = K.by_name()["known_motion_360_0"]
    guess = (0.01, -0.02, 0.003)
    want = P.sm_icp(P.PlicpParams(max_iterations=0), c.ldp(c.ref), c.ldp(c.sens), guess)
    m = api.PlicpMatcher(ctx, api.plicp_params(max_iterations=0), laser=c.laser)
    try:
        rec = m.match_batch(np.stack([c.ref, c.sens]), [0], [1], [guess])[0]
    finally:
        m.close()
    assert (want["valid"], want["iterations"], want["nvalid"]) == (0, 0, 0) and math.isinf(want["error"])
    assert (rec["valid"], rec["iterations"], rec["nvalid"]) == (0, 0, 0) and math.isinf(rec["error"])
    assert np.array_equal(rec["x"], np.array(guess)) and np.array_equal(want["x"], np.array(guess))
