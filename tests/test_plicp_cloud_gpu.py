"""The cloud forms of lesson3's PL-ICP on the device (csrc/plicp.hip's k_plicp_match_clouds / k_plicp_debug_clouds,
api.PlicpMatcher.match_clouds[_dev] / debug_iteration_clouds) against tools/plicp_cpu.py's sm_icp on cloud_to_ldp and its
per-iteration restatement, on the scenarios of tests/plicp_cloud_cases.py.

Bounds.  x of one iteration against the restatement: measured max |device - restatement| over the cases on the first run
3.32e-13 (r_beam_counts_64), allowed 8 x 3.4e-13 as tests/test_plicp_gpu.py does, never
above 1e-7.  Full runs: the project's contract, 1e-4 m / 1e-4 rad (measured 2.2e-13, r_beam_counts_63).  Known motions: plicp_cloud_cases.RECOVERY_BOUND = 1.3e-7, twice the worst error of sm_icp on these
float32 clouds measured on the CPU (tests/test_plicp_cloud_cases_oracle.py)."""
import math

import numpy as np
import pytest

import plicp_cloud_cases as C
from lslam_amd import api
from tools import plicp_cpu as P

pytestmark = pytest.mark.gpu

X_ITERATION_BOUND = 8 * 3.4e-13   # 8 x the measured maximum (see above)
assert X_ITERATION_BOUND <= 1e-7
X_CONTRACT = 1e-4


@pytest.fixture(scope="module")
def device(ctx):
    """Every case once: name -> (debug_iteration_clouds' (j1, j2, flags, x_out), the full run's record)."""
    out = {}
    for c in C.cases():
        m = api.PlicpMatcher(ctx, api.plicp_params(**c.overrides))          # no laser: a cloud needs none
        try:
            dbg = m.debug_iteration_clouds(c.ref_xyz, c.sens_xyz, c.guess, c.ref_valid, c.sens_valid)
            if c.ref_valid is None or c.sens_valid is None:                    # the batch takes one valid block, or none
                assert c.ref_valid is None and c.sens_valid is None or c.name == "valid_null_ref_only"
                valid = None if c.sens_valid is None else np.stack([np.ones_like(c.sens_valid), c.sens_valid])
            else:
                valid = np.stack([c.ref_valid, c.sens_valid])
            rec = m.match_clouds(np.stack([c.ref_xyz, c.sens_xyz]), [0], [1], valid, [c.guess])[0]
        finally:
            m.close()
        out[c.name] = (dbg, rec)
    return out


@pytest.mark.parametrize("name", C.NAMES)
def test_one_iteration_takes_the_restatements_decisions(device, name):
    it1 = C.expected(name)[2][0]
    (j1, j2, flags, x_out), _ = device[name]
    decided = ~it1.undecided
    print(name, "undecided points skipped:", int(it1.undecided.sum()))
    assert np.array_equal(flags & 1, it1.flags & 1)                    # participation has no margin
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


@pytest.mark.parametrize("name", C.NAMES)
def test_full_run_equals_sm_icp(device, name):
    direct, res, its, near = C.expected(name)
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


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.recovering(n) and "known_motion" in n])
def test_known_motion_is_recovered(device, name):
    c = C.by_name()[name]
    rec = device[name][1]
    e = rec["x"] - c.truth
    print(name, "error", math.hypot(e[0], e[1]), abs(e[2]), "iterations", int(rec["iterations"]))
    assert rec["valid"] == 1 and math.hypot(e[0], e[1]) < C.RECOVERY_BOUND and abs(math.remainder(e[2], 2 * math.pi)) < C.RECOVERY_BOUND


def test_cases_that_restate_another_give_its_bytes(device):
    for c in C.cases():
        if c.same_as:
            assert device[c.name][1].tobytes() == device[c.same_as][1].tobytes(), c.name
            assert np.array_equal(device[c.name][0][2], device[c.same_as][0][2]), c.name


# ---- batches -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def clouds360():
    """16 clouds, (2k, 2k + 1) a known-motion pair, and their valid bytes with holes of another length per cloud."""
    cs = [C.by_name()[f"r_known_motion_360_{k}"] for k in range(8)]
    xyz = np.stack([x for c in cs for x in (c.ref_xyz, c.sens_xyz)])
    valid = np.stack([v for c in cs for v in (c.ref_valid, c.sens_valid)]).copy()
    for k in range(16):
        valid[k, 20 * k:20 * k + 3 * k] = 0
    return xyz, valid


def _pairs(n_pairs, n_clouds):
    k = np.arange(n_pairs)
    ref = (2 * (k % (n_clouds // 2))).astype(np.int32)
    return ref, ref + 1


@pytest.fixture(scope="module")
def m(ctx):
    m = api.PlicpMatcher(ctx)
    yield m
    m.close()


def test_a_pair_is_the_same_alone_and_in_a_batch_of_five(m, clouds360):
    xyz, valid = clouds360
    ref, sens = np.array([0, 2, 4, 6, 8], np.int32), np.array([1, 3, 5, 7, 9], np.int32)
    assert len({int(valid[i].sum()) for i in range(10)}) >= 9              # neighbours of other lengths of validity
    batch = m.match_clouds(xyz, ref, sens, valid)
    assert np.all(batch["valid"] == 1)
    for b in range(5):
        alone = m.match_clouds(xyz[[ref[b], sens[b]]], [0], [1], valid[[ref[b], sens[b]]])
        assert alone.tobytes() == batch[b:b + 1].tobytes(), b
        ldps = [P.cloud_to_ldp(xyz[i], valid[i]) for i in (ref[b], sens[b])]
        want = P.sm_icp(P.PlicpParams(), ldps[0], ldps[1])
        assert (batch[b]["valid"], batch[b]["iterations"], batch[b]["nvalid"]) == (want["valid"], want["iterations"], want["nvalid"])
        assert np.abs(batch[b]["x"] - want["x"]).max() <= X_CONTRACT
    again = m.match_clouds(xyz, sens[::-1].copy() - 1, sens[::-1].copy(), valid)  # the same pairs at other positions
    assert again[::-1].tobytes() == batch.tobytes()


def test_host_form_equals_dev_form(ctx, m, clouds360):
    xyz, valid = clouds360
    ref, sens = _pairs(67, len(xyz))
    guess = np.zeros((67, 3))
    guess[:, 0] = 0.01
    host = m.match_clouds(xyz, ref, sens, valid, guess)
    p_x, p_v, p_g, p_o = ctx.alloc(xyz.nbytes), ctx.alloc(valid.nbytes), ctx.alloc(guess.nbytes), ctx.alloc(67 * 48)
    try:
        ctx.upload(p_x, xyz)
        ctx.upload(p_v, valid)
        ctx.upload(p_g, guess)
        before = m.stats()
        m.match_clouds_dev(len(xyz), 360, p_x, p_v, ref, sens, p_g, p_o)
        after = m.stats()
        ctx.synchronize()
        dev = np.zeros(67, api.PLICP_RECORD)
        ctx.download(p_o, dev)
        assert after["host_waits"] == before["host_waits"], "the _dev form makes no host wait"
        assert after["launches"] == before["launches"] + 1 and after["pairs"] == before["pairs"] + 67
        assert dev.tobytes() == host.tobytes()
        m.match_clouds_dev(len(xyz), 360, p_x, None, ref, sens, None, p_o)   # NULL valid = every point, NULL guess = zeros
        ctx.synchronize()
        ctx.download(p_o, dev)
        assert dev.tobytes() == m.match_clouds(xyz, ref, sens).tobytes()
        s1 = m.stats()
        assert m.match_clouds(xyz, ref, sens, valid, guess).tobytes() == host.tobytes()
        s2 = m.stats()
        assert s2["growths"] == s1["growths"] and s2["host_waits"] == s1["host_waits"] + 1 and s2["launches"] == s1["launches"] + 1
    finally:
        for p in (p_x, p_v, p_g, p_o):
            ctx.free(p)


def test_refusals_leave_the_outputs_untouched(m, clouds360):
    xyz, valid = clouds360
    sentinel = np.frombuffer(bytes(range(48)) * 2, api.PLICP_RECORD).copy()
    for ref, sens in (([0, 16], [1, 1]), ([0, 0], [1, -1])):               # a pair index out of range
        out = sentinel.copy()
        with pytest.raises(api.LslamError) as e:
            m.match_clouds(xyz, ref, sens, valid, out=out)
        assert e.value.code == -1 and out.tobytes() == sentinel.tobytes()
    out = sentinel.copy()
    with pytest.raises(api.LslamError) as e:                                # 2049 points
        m.match_clouds(np.ones((2, 2049, 3), np.float32), [0, 0], [1, 1], out=out)
    assert e.value.code == -8 and out.tobytes() == sentinel.tobytes()
    with pytest.raises(api.LslamError) as e:
        m.debug_iteration_clouds(np.ones((2049, 3), np.float32), np.ones((2049, 3), np.float32))
    assert e.value.code == -8
    L, x = m.L, np.ascontiguousarray(xyz)
    idx = np.zeros(2, np.int32)
    for args in ((None, idx.ctypes.data, idx.ctypes.data, out.ctypes.data), (x.ctypes.data, None, idx.ctypes.data, out.ctypes.data),
                 (x.ctypes.data, idx.ctypes.data, None, out.ctypes.data), (x.ctypes.data, idx.ctypes.data, idx.ctypes.data, None)):
        for fn in (L.lslam_plicp_match_clouds, L.lslam_plicp_match_clouds_dev):
            assert fn(m.h, 16, 360, args[0], None, 2, args[1], args[2], None, args[3]) == -1   # NULL
    assert L.lslam_plicp_debug_iteration_clouds(m.h, x.ctypes.data, None, None, None, 360, None, None, None, None, None) == -1
    assert out.tobytes() == sentinel.tobytes()
    before = m.stats()
    assert len(m.match_clouds(xyz, [], [])) == 0 and m.stats() == before   # n_pairs == 0 launches nothing
