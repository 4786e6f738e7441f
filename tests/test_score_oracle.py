"""Pose scoring on the CPU: the numpy restatement (tests/score_restatement.py) against the recorded reference
(tests/golden/score_golden.npz, tests/golden/make_score_golden.py), bit for bit; the planes the plain-C oracle builds from the
recorded scans against the recorded planes, byte for byte; every scenario of tests/score_cases.py being what it claims; E_ref,
from which tests/test_score_gpu.py takes its bound; and the re-localisation case checked with the oracle alone."""
import numpy as np
import pytest

import score_cases as S
import score_restatement as R

f32 = np.float32


@pytest.fixture(scope="module")
def g():
    return S.golden()


@pytest.fixture(scope="module")
def lv():
    return R.levels()


@pytest.fixture(scope="module")
def oracle_levels(oracle_lib, g):
    """map name -> [PortHector per level] fed the recorded scans the way MapRepMultiMap feeds its levels."""
    po, out = oracle_lib, {}
    for name, m in g.maps.items():
        cpus = [po.PortHector(sx, sy, float(cell), m.off) for sx, sy, cell in S.level_list(m)]
        for c in cpus:
            c.setUpdateOccupiedFactor(S.OCC_FACTOR)
        for pts, pose in m.scans:
            for i, c in enumerate(cpus):
                c.updateByScan(pts if i == 0 else pts * f32(po.PortHector.level_factor(i)), (0.0, 0.0), pose)
        out[name] = cpus
    return out


def groups(queries):
    out = {}
    for i, q in enumerate(queries):
        out.setdefault((q.map, q.container, q.level), []).append(i)
    return out


def test_oracle_planes_equal_the_recorded_planes(g, oracle_levels):
    for name, cpus in oracle_levels.items():
        for L, c in enumerate(cpus):
            assert c.logodds().tobytes() == g.planes[name, L].tobytes(), (name, L)
    assert all((g.planes["main", L] != 0).any() for L in range(3))


def test_restatement_equals_the_reference_bit_for_bit(g, lv):
    qs = S.all_queries()
    for (m, c, L), idx in groups(qs).items():
        res, lik = R.score_world(lv[m, L], g.containers[c], np.array([qs[i].pose for i in idx], f32))
        assert res.tobytes() == g.residual[idx].tobytes(), (m, c, L)
        assert lik.tobytes() == g.likelihood[idx].tobytes(), (m, c, L)


def test_covariance_restatement_equals_the_reference_bit_for_bit(g, lv):
    for name, q in S.covariances().items():
        lik, cm, cw = R.pose_covariance(lv[q.map, q.level], g.containers[q.container], np.array(q.pose, f32))
        ref_lik, ref_cm, ref_cw = g.cov[name]
        assert (ref_lik >= S.COV_MIN_LIKELIHOOD).all(), (name, ref_lik)  # the precondition of every covariance case
        assert lik.tobytes() == ref_lik.tobytes(), name
        assert cm.tobytes() == ref_cm.tobytes(), name
        assert cw.tobytes() == ref_cw.tobytes(), name
        assert np.isfinite(ref_cm).all() and (np.diag(ref_cm) > 0).all(), name


def outside_count(lv, g, q):
    L = lv[q.map, q.level]
    _, out = R.terms(L, g.containers[q.container], L.map_pose(np.array([q.pose], f32)))
    return int(out.sum())


def test_scenarios_are_what_they_claim(g, lv):
    s = S.singles()
    assert [len(g.containers["n%d" % k]) for k in S.SIZES] == list(S.SIZES) and len(g.containers["big"]) == S.BIG
    for k in S.SIZES:
        assert outside_count(lv, g, s["size-%d" % k]) == 0
    assert outside_count(lv, g, s["size-big"]) == 0  # all 65536 inside the map
    for L in (0, 1, 2):
        # (the room's far walls lie past the coarsest level's limit of sx - 2, sy - 2 cells: there "inside" keeps three quarters)
        assert outside_count(lv, g, s["inside-L%d" % L]) == (0 if L < 2 else 269)
        assert 100 < outside_count(lv, g, s["part-out-L%d" % L]) < 1081 - 100
        assert outside_count(lv, g, s["all-out-L%d" % L]) == 1081
        res, lik = g.ref([s["all-out-L%d" % L]])
        assert res[0] == 1081.0 and lik[0] == 0.0
    res, lik = g.ref([s["size-0"]])
    assert res[0] == 0.0 and np.isnan(lik[0])  # 0 / 0
    h = [s["heading-%d" % i].pose[2] for i in range(3)]
    assert 0 < np.pi - h[0] < 1e-5 and 0 < h[1] + np.pi < 1e-5 and h[2] == 0.0
    # the band: map coordinates are the container's own, one ulp beyond lim is outside, exactly 0.0 / -0.0 / lim inside
    q = s["band"]
    L = lv["small", 0]
    e = L.map_pose(np.array([q.pose], f32))
    assert e.tobytes() == np.array([[-0.0, -0.0, 0.0]], f32).tobytes()
    t, out = R.terms(L, g.containers["band"], e)
    assert int(out.sum()) == S.BAND_OUTSIDE and (t[0][out[0]] == 1.0).all()
    assert not out[0][[0, 1, 2, 4, 5, 6, 8, 12]].any()
    assert (t[0][~out[0]] != 0.5).any()  # the band reads written cells


def test_batches_mix_containers_and_poses(g):
    names, ec, poses = S.batch(0)
    assert names[1] == "n0" and list(ec[:3]) == [0, 1, 2]          # an empty container between two full ones
    assert len(set(ec)) == len(names) and (ec[8:16] == 0).all()    # distinct and shared containers in one call
    assert max(S.BATCH_SIZES) == len(poses) == 130
    for L in (0, 1, 2):
        _, lik = g.ref(S.batch_queries(L))
        assert np.isnan(lik[ec == 1]).all() and np.isfinite(lik[ec != 1]).all()


def test_lattices_are_what_they_claim(g, lv):
    lat = S.lattices()
    assert np.prod(lat["5x3x7"].counts) == 105 and np.prod(lat["16x16x21"].counts) == 5376
    vol = {k: g.ref(S.lattice_queries(k))[1] for k in lat}
    # rim-off: every state but the centre has every point off the map
    for i, q in enumerate(S.lattice_queries("rim-off")):
        assert (outside_count(lv, g, q) == 1081) == (i != 4)
    assert R.best_state(vol["rim-off"])[0] == 4 and (np.delete(vol["rim-off"], 4) == 0.0).all()
    # tie: a mirror-symmetric plane, a container on the mirror axis, states a quarter cell either side of it
    plane = g.planes["small", 0]
    assert plane.tobytes() == plane[:, ::-1].tobytes() and (g.containers["axis"][:, 0] == 0).all()
    e = lv["small", 0].map_pose(S.lattice_poses(lat["tie"]))
    assert list(e[:, 0]) == [15.75, 16.0, 16.25] and (e[:, 1] == 15.0).all()
    assert vol["tie"][0] == vol["tie"][2] > vol["tie"][1]
    assert R.best_state(vol["tie"])[0] == 0  # the lowest index of the two
    assert np.isnan(vol["all-nan"]).all() and R.best_state(vol["all-nan"])[0] == -1
    for k in ("5x3x7", "16x16x21", "reloc"):
        i, v = R.best_state(vol[k])
        assert v == np.nanmax(vol[k]) and (vol[k][:i] < v).all()
    # the device API states the lattice's poses with the same expression
    from lslam_amd import api

    for k, l in lat.items():
        assert api.OccGridMap.lattice_poses(l.centre, l.counts, l.steps).tobytes() == S.lattice_poses(l).tobytes(), k


def test_e_ref_and_the_float64_restatement(g):
    """E_ref = worst |reference - float64| likelihood; the default mode's bound is max(4 E_ref, FLOOR)."""
    res64, lik64 = R.float64_all()
    e = R.e_ref()
    print("E_ref %.3e  floor %.3e  bound %.3e" % (e, R.FLOOR, R.bound()))
    # the reference's sequential float32 sum: at most n/2 ulps of a residual <= n, i.e. n * 2^-24 / 2 relative to n
    assert 0.0 < e <= S.BIG * 2.0 ** -25
    qs = S.all_queries()
    n = np.array([len(g.containers[q.container]) for q in qs])
    assert (np.abs(g.residual - res64)[n > 0] <= e * n[n > 0] * 1.0000001).all()
    assert R.bound() >= R.FLOOR > 0


def test_relocalise_case_with_the_oracle_alone(g, lv, oracle_lib, oracle_levels):
    """The reference's arithmetic alone meets what tests/test_score_gpu.py asks of OccGridMap.relocalise: lattice on level 1 ->
    the k best states -> matchData from each -> likelihood on level 0; the best lands on matchData started at the truth."""
    po, cpus = oracle_lib, oracle_levels["main"]
    lat = S.lattices()["reloc"]
    pts = g.containers[lat.container]
    truth = S.P("truth")
    centre = np.array(lat.centre, f32)
    assert abs(np.hypot(*(centre[:2] - truth[:2])) / 0.05 - 6.0) < 0.01 and abs(centre[2] - truth[2] - 0.2) < 1e-6
    vol = g.ref(S.lattice_queries("reloc"))[1]
    order = np.argsort(-vol, kind="stable")[:S.RELOC_K]
    starts = S.lattice_poses(lat)[order]
    poses = np.stack([po.PortHector.match_data(cpus, pts, b)[0] for b in starts])
    _, lik = R.score_world(lv["main", 0], pts, poses)
    want, _ = po.PortHector.match_data(cpus, pts, truth)
    best = poses[int(np.argmax(lik))]
    d = np.abs(best.astype(np.float64) - want)
    print("relocalise (oracle): best", best, "from truth", want, "likelihoods", lik)
    assert d[:2].max() <= 1e-4 and d[2] <= 1e-4, (best, want)
    assert np.abs(want - truth).max() < 0.02
