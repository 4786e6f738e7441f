"""lesson2's point-to-point ICP on the device (csrc/icp.hip, api.IcpMatcher) against tools/icp_cpu.py on the scenarios of
tests/icp_cases.py: the conversion reading by reading, the decisions of one iteration point by point, the solved increment, the
full runs, and the batch forms byte for byte.

Bounds.  The increment of one iteration (debug_iteration) and x of a full run against the helper, on the cases that are neither
near nor undecided: measured max |device - helper| over the cases on the MI355X 3.5e-18 for the increment (stop_transform) and
2.5e-16 for x (pair_360_drop_target; 25 of the 36 cases agree bit for bit) -- the helper sums in the kernel's order, so what is
left is cos / sin / atan2 coming from another libm -- allowed 8 x the larger, as the fit's conditioning varies with the
geometry; never above 1e-7.  On the other cases x is held to the project's contract, 1e-4 m / 1e-4 rad (measured 0 on both).
fitness and mse: a relative 1e-9 (measured at most 1e-11, on rigid_copy's mse of 1.6e-15).  Conversion: valid byte-equal,
coordinates within one float32 ulp (device and host cos may round a double differently at a float32 boundary; measured: 0 of
77 247 coordinates differ at all)."""
import math

import numpy as np
import pytest

import icp_cases as K
from lslam_amd import api
from tools import icp_cpu as I

pytestmark = pytest.mark.gpu

MEASURED_MAX = 2.5e-16            # max |device - helper| of inc and of x over the decided cases, on the MI355X
X_BOUND = 8 * MEASURED_MAX
assert X_BOUND <= 1e-7
X_CONTRACT = 1e-4
REL = 1e-9


def _matcher(ctx, c):
    return api.IcpMatcher(ctx, api.icp_params(**c.overrides), laser=c.laser)


def _valid(c):
    return None if c.src_valid is None else np.stack([c.src_valid, c.tgt_valid])


def _dx(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    d[2] = abs(math.remainder(a[2] - b[2], 2 * math.pi))
    return d


@pytest.fixture(scope="module")
def device(ctx):
    """Every case once: name -> (debug_iteration's (corr, d2, inc, mse, ncorr), the full run's record), through the clouds form."""
    out = {}
    for c in K.cases():
        m = _matcher(ctx, c)
        try:
            dbg = m.debug_iteration(c.src, c.tgt, c.guess, c.src_valid, c.tgt_valid)
            rec = m.match_clouds(np.stack([c.src, c.tgt]), [0], [1], _valid(c), [c.guess])[0]
        finally:
            m.close()
        out[c.name] = (dbg, rec)
    return out


# ---- conversion -------------------------------------------------------------------------------------------------------------

def _ulps(a, b):
    """Distance in float32 steps between two finite float32 arrays."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("invalid_as_nan", [0, 1])
def test_conversion_is_the_helpers(ctx, invalid_as_nan):
    differing = total = 0
    for n in sorted({c.n for c in K.cases() if c.laser is not None}):
        group = [c for c in K.cases() if c.laser is not None and c.n == n]
        laser = group[0].laser
        scans = np.stack([r for c in group for r in (c.src_ranges, c.tgt_ranges)] + ([K.window_scan(laser)] if n >= 16 else []))
        m = api.IcpMatcher(ctx, api.icp_params(invalid_as_nan=invalid_as_nan), laser=laser)
        try:
            xyz, valid = m.convert(scans)
        finally:
            m.close()
        for k, r in enumerate(scans):
            want_xyz, want_valid = K.cloud(laser, r, invalid_as_nan)
            assert np.array_equal(valid[k], want_valid), (n, k)
            bad = want_valid == 0
            if invalid_as_nan:
                assert np.all(np.isnan(xyz[k][bad]))
            else:
                assert np.all(xyz[k][bad] == 0.0)
            ok = ~bad
            u = _ulps(xyz[k][ok], want_xyz[ok])
            assert u.size == 0 or u.max() <= 1, (n, k, u.max())
            assert np.all(xyz[k][ok][:, 2] == 0.0)
            differing += int((u > 0).sum())
            total += int(u.size)
    print("coordinates that differ at all (by one float32 ulp):", differing, "of", total)


# ---- one iteration ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.NAMES)
def test_one_iteration_takes_the_helpers_decisions(device, name):
    it1 = K.expected(name)["trace"][0]
    und = K.margins(name)[0][0]
    (corr, d2, inc, mse, ncorr), _ = device[name]
    print(name, "undecided points skipped:", int(und.sum()))
    assert np.array_equal(corr[~und], it1.corr[~und])
    if tuple(K.by_name()[name].guess) == (0.0, 0.0, 0.0):
        assert np.array_equal(d2[~und], it1.d2[~und])                    # the same expressions on the same bits
    else:                                                                # cos / sin of the guess come from another libm
        assert np.allclose(d2[~und], it1.d2[~und], rtol=REL, atol=0.0)
    assert ncorr == it1.ncorr
    if it1.inc is None:
        assert np.all(np.isnan(inc)), (name, inc)
        return
    d = _dx(inc, it1.inc)
    print(name, "max |inc - helper|", d.max(), "mse", mse, it1.mse)
    assert d.max() <= (X_CONTRACT if und.any() else X_BOUND), (name, d)
    assert mse == pytest.approx(it1.mse, rel=REL, abs=0.0)


# ---- full runs --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.NAMES)
def test_full_run_is_the_helpers(device, name):
    want = K.expected(name)
    rec = device[name][1]
    d = _dx(rec["x"], want["x"])
    decided = K.decided(name)
    print(name, "decided", decided, "iterations", int(rec["iterations"]), want["iterations"], "state", int(rec["state"]),
          "max |x - helper|", d.max(), "fitness", rec["fitness"], want["fitness"], "mse", rec["mse"], want["mse"])
    assert d.max() <= X_CONTRACT, (name, d)
    if not decided:
        return
    assert (int(rec["converged"]), int(rec["iterations"]), int(rec["state"]), int(rec["ncorr"])) == \
        (want["converged"], want["iterations"], want["state"], want["ncorr"])
    assert d.max() <= X_BOUND, (name, d)
    assert rec["fitness"] == pytest.approx(want["fitness"], rel=REL, abs=0.0)
    assert rec["mse"] == pytest.approx(want["mse"], rel=REL, abs=0.0)
    assert rec["reserved"] == 0.0


@pytest.mark.parametrize("name", ["identical", "all_invalid"])
def test_identical_clouds_give_bit_exact_zeros(device, name):
    (corr, d2, inc, mse, ncorr), rec = device[name]
    assert (int(rec["converged"]), int(rec["iterations"]), int(rec["state"])) == (1, 1, I.STATE_TRANSFORM)
    assert rec["x"].tobytes() == np.zeros(3).tobytes()                    # +0.0, bit for bit
    assert rec["mse"] == 0.0 and rec["fitness"] == 0.0 and np.all(d2 == 0.0) and np.all(inc == 0.0)
    if name == "all_invalid":
        assert np.all(corr == 0)                                          # every distance ties: the lowest index


def test_rigid_copy_is_recovered(device):
    rec = device["rigid_copy"][1]
    e = _dx(rec["x"], np.array(K.RIGID_TRUTH))
    print("rigid_copy: error", e, "iterations", int(rec["iterations"]), "state", int(rec["state"]))
    assert e.max() < 1e-6 and rec["converged"] == 1


def test_exact_ties_go_to_the_lowest_index(device):
    corr = device["tie_midway"][0][0]
    assert corr[5] == 5                                                   # midway between targets 5 and 6, exactly
    first = device["duplicates"][0][0]
    assert not np.any(np.isin(first, (11, 12, 201))) and (np.any(first == 10) or np.any(first == 200))


def test_more_than_2048_points_are_refused(ctx):
    m = api.IcpMatcher(ctx, laser=K.PK.LASER360)
    sentinel = np.frombuffer(bytes(range(64)), api.ICP_RECORD).copy()
    try:
        out = sentinel.copy()
        with pytest.raises(api.LslamError) as e:
            m.match_batch(np.ones((2, 2049), np.float32), [0], [1], out=out)
        assert e.value.code == -8 and out.tobytes() == sentinel.tobytes()
        with pytest.raises(api.LslamError) as e:
            m.match_clouds(np.ones((2, 2049, 3), np.float32), [0], [1], out=out)
        assert e.value.code == -8 and out.tobytes() == sentinel.tobytes()
        with pytest.raises(api.LslamError) as e:
            m.debug_iteration(np.ones((2049, 3), np.float32), np.ones((2049, 3), np.float32))
        assert e.value.code == -8
    finally:
        m.close()


# ---- forms ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scans360():
    cs = [c for c in K.cases() if c.laser is K.PK.LASER360][:8]
    return np.stack([r for c in cs for r in (c.src_ranges, c.tgt_ranges)])   # 16 scans: (2k, 2k + 1) are a pair


def _pairs(n_pairs, n_scans):
    k = np.arange(n_pairs)
    src = (2 * (k % (n_scans // 2))).astype(np.int32)
    return src, src + 1


@pytest.fixture(scope="module")
def m360(ctx):
    m = api.IcpMatcher(ctx, laser=K.PK.LASER360)
    yield m
    m.close()


def test_ranges_form_equals_clouds_form_on_the_converters_output(m360, scans360):
    src, tgt = _pairs(11, len(scans360))
    xyz, valid = m360.convert(scans360)
    a = m360.match_batch(scans360, src, tgt)
    assert a.tobytes() == m360.match_clouds(xyz, src, tgt, valid).tobytes()
    assert a.tobytes() == m360.match_clouds(xyz, src, tgt).tobytes()     # without skip_invalid the valid bytes are not read
    assert np.all(a["iterations"] >= 1)
    wide = np.full((len(scans360), 400), 7.0, np.float32)                # a stride beyond the scan: the tail is not read
    wide[:, :360] = scans360
    assert m360.match_batch(wide, src, tgt, n_readings=360).tobytes() == a.tobytes()


@pytest.mark.parametrize("n_pairs", [3, 70])
def test_a_pair_is_the_same_alone_and_in_a_batch(m360, scans360, n_pairs):
    src, tgt = _pairs(n_pairs, len(scans360))
    batch = m360.match_batch(scans360, src, tgt)
    for b in sorted({0, n_pairs // 2, n_pairs - 1}):
        alone = m360.match_batch(scans360[[src[b], tgt[b]]], [0], [1])
        assert alone.tobytes() == batch[b:b + 1].tobytes(), b
    for b in range(n_pairs):  # the same pair at another position
        assert batch[b].tobytes() == batch[b % 8].tobytes()


def test_host_forms_equal_dev_forms(ctx, m360, scans360):
    src, tgt = _pairs(70, len(scans360))
    guess = np.zeros((70, 3))
    guess[:, 0] = 0.01
    host = m360.match_batch(scans360, src, tgt, guess)
    xyz, valid = m360.convert(scans360)
    p_r, p_g, p_o = ctx.alloc(scans360.nbytes), ctx.alloc(guess.nbytes), ctx.alloc(70 * 64)
    p_x, p_v = ctx.alloc(xyz.nbytes), ctx.alloc(valid.nbytes)
    try:
        ctx.upload(p_r, scans360)
        ctx.upload(p_g, guess)
        before = m360.stats()
        m360.match_batch_dev(len(scans360), 360, p_r, 360, src, tgt, p_g, p_o)
        after = m360.stats()
        ctx.synchronize()
        dev = np.zeros(70, api.ICP_RECORD)
        ctx.download(p_o, dev)
        assert after["host_waits"] == before["host_waits"], "the _dev form makes no host wait"
        assert after["launches"] == before["launches"] + 2 and after["pairs"] == before["pairs"] + 70   # conversion + match
        assert dev.tobytes() == host.tobytes()
        m360.match_batch_dev(len(scans360), 360, p_r, 360, src, tgt, None, p_o)   # NULL first guess = zeros
        ctx.synchronize()
        ctx.download(p_o, dev)
        assert dev.tobytes() == m360.match_batch(scans360, src, tgt).tobytes()
        # the converter and the clouds form in HBM
        before = m360.stats()
        m360.convert_dev(len(scans360), 360, p_r, 360, p_x, p_v)
        m360.match_clouds_dev(len(scans360), 360, p_x, p_v, src, tgt, p_g, p_o)
        after = m360.stats()
        ctx.synchronize()
        assert after["host_waits"] == before["host_waits"] and after["launches"] == before["launches"] + 2
        got_xyz, got_valid = np.zeros_like(xyz), np.zeros_like(valid)
        ctx.download(p_x, got_xyz)
        ctx.download(p_v, got_valid)
        ctx.download(p_o, dev)
        assert got_xyz.tobytes() == xyz.tobytes() and got_valid.tobytes() == valid.tobytes()
        assert dev.tobytes() == host.tobytes()
    finally:
        for p in (p_r, p_g, p_o, p_x, p_v):
            ctx.free(p)


def test_refusals_leave_the_outputs_untouched(ctx, m360, scans360):
    sentinel = np.frombuffer(bytes(range(64)) * 2, api.ICP_RECORD).copy()
    xyz, valid = m360.convert(scans360)
    for src, tgt in (([0, 16], [1, 1]), ([0, 0], [1, -1])):
        out = sentinel.copy()
        with pytest.raises(api.LslamError) as e:
            m360.match_batch(scans360, src, tgt, out=out)
        assert e.value.code == -1 and out.tobytes() == sentinel.tobytes()
        with pytest.raises(api.LslamError) as e:
            m360.match_clouds(xyz, src, tgt, out=out)
        assert e.value.code == -1 and out.tobytes() == sentinel.tobytes()
    out = sentinel.copy()
    bare = api.IcpMatcher(ctx)                                            # no laser set: the ranges forms are refused
    try:
        with pytest.raises(api.LslamError) as e:
            bare.match_batch(scans360, [0, 0], [1, 1], out=out)
        assert e.value.code == -1 and out.tobytes() == sentinel.tobytes()
        with pytest.raises(api.LslamError) as e:
            bare.convert(scans360)
        assert e.value.code == -1
        assert bare.match_clouds(xyz, [0], [1]).tobytes() == m360.match_clouds(xyz, [0], [1]).tobytes()   # clouds need none
    finally:
        bare.close()
    L, r = m360.L, np.ascontiguousarray(scans360)
    idx = np.zeros(2, np.int32)
    for args in ((None, 360, 2, idx.ctypes.data, idx.ctypes.data, out.ctypes.data), (r.ctypes.data, 360, 2, None, idx.ctypes.data, out.ctypes.data),
                 (r.ctypes.data, 360, 2, idx.ctypes.data, None, out.ctypes.data), (r.ctypes.data, 360, 2, idx.ctypes.data, idx.ctypes.data, None),
                 (r.ctypes.data, 100, 2, idx.ctypes.data, idx.ctypes.data, out.ctypes.data)):
        assert L.lslam_icp_match_batch(m360.h, 16, 360, args[0], args[1], args[2], args[3], args[4], None, args[5]) == -1
    assert L.lslam_icp_match_clouds(m360.h, 16, 360, None, None, 2, idx.ctypes.data, idx.ctypes.data, None, out.ctypes.data) == -1
    assert out.tobytes() == sentinel.tobytes()
    before = m360.stats()
    assert len(m360.match_batch(scans360, [], [])) == 0 and len(m360.match_clouds(xyz, [], [])) == 0
    assert m360.stats() == before                                         # n_pairs == 0 launches nothing
    with pytest.raises(api.LslamError) as e:
        api.IcpMatcher(ctx, api.icp_params(max_iterations=0))
    assert e.value.code == -1


def test_repeated_shape_allocates_nothing(ctx, scans360):
    m = api.IcpMatcher(ctx, laser=K.PK.LASER360)
    try:
        src, tgt = _pairs(70, len(scans360))
        first = m.match_batch(scans360, src, tgt)
        s1 = m.stats()
        second = m.match_batch(scans360, src, tgt)
        s2 = m.stats()
        assert first.tobytes() == second.tobytes()
        assert s1["growths"] > 0 and s2["growths"] == s1["growths"]
        assert (s1["host_waits"], s2["host_waits"]) == (1, 2), "the host form waits once, at its end"
        assert (s1["launches"], s2["launches"]) == (2, 4) and s2["pairs"] == 140
        m.match_batch(scans360, src[:5], tgt[:5])                         # a smaller batch fits what is there
        assert m.stats()["growths"] == s1["growths"]
    finally:
        m.close()
