"""Pose scoring on the device (lslam_map_score_batch / lslam_map_pose_covariance_batch / lslam_map_score_lattice and their _dev
twins) against the recorded reference (tests/golden/score_golden.npz) and the restatement (tests/score_restatement.py) on the
scenarios of tests/score_cases.py.

  ordered mode   residuals, likelihoods, the seven likelihoods, cov_map and cov_world equal the reference BIT FOR BIT, every
                 case, through all three forms, host and _dev
  default mode   |likelihood - float64| <= max(4 E_ref, floor) (score_restatement.bound: E_ref is the reference's own worst
                 distance from float64, the floor the hardware exp / rcp of gn_prob_f), residuals the same x n; the covariance
                 is the fp32 restatement of the device's own seven likelihoods, bit for bit
  independence   an entry of the 130-entry batch equals the same entry scored alone, the lattice volume equals scoreBatch on
                 host-generated poses, host equals _dev -- bit for bit, both modes
  purity, refusals, relocalise

Worst default-mode differences measured on the MI355X are in DESIGN.md 4.19."""
import ctypes as C

import numpy as np
import pytest

import score_cases as S
import score_restatement as R
from lslam_amd import api

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARGUMENT = -1
MODES = ("ordered", "default")
FORMS = ("host", "dev")


def build_map(ctx, m):
    """The map on the device from the recorded scans, every level fed the scan like MapRepMultiMap's."""
    d = api.OccGridMap(ctx, m.sx, m.sy, m.cell, m.off, levels=m.levels)
    d.setUpdateOccupiedFactor(S.OCC_FACTOR)
    for pts, pose in m.scans:
        if m.levels > 1:
            d.matchData(pose, pts)  # caches the container: updateByScan feeds the levels above 0 from it
        d.updateByScan(pts, (0.0, 0.0), pose)
    return d


class Env:
    def __init__(self, ctx):
        self.ctx, self.g, self.lv = ctx, S.golden(), R.levels()
        self.maps = {name: build_map(ctx, m) for name, m in self.g.maps.items()}
        for (name, L), plane in self.g.planes.items():  # the precondition of everything below
            assert self.maps[name].logodds(L).tobytes() == plane.tobytes(), (name, L)
        self.cache = {}

    def mode(self, mode):
        for m in self.maps.values():
            m.set_option("ordered_sums", int(mode == "ordered"))

    # ---- the three forms, host or _dev, on a list of queries of one map and level ------------------------------------------
    def _pack(self, queries):
        names = sorted({q.container for q in queries})
        ec = np.array([names.index(q.container) for q in queries], np.int32)
        return [self.g.containers[n] for n in names], ec, np.array([q.pose for q in queries], f32)

    def _dev(self, arrays, outs, call):
        """Uploads `arrays`, allocates `outs` (numpy arrays to fill), runs call(*pointers), synchronises, downloads."""
        ctx, ptrs = self.ctx, []
        try:
            for a in list(arrays) + list(outs):
                ptrs.append(ctx.alloc(max(a.nbytes, 16)))
            for p, a in zip(ptrs, arrays):
                if a.nbytes:
                    ctx.upload(p, a)
            call(*ptrs)
            ctx.synchronize()
            for p, a in zip(ptrs[len(arrays):], outs):
                if a.nbytes:
                    ctx.download(p, a)
        finally:
            for p in ptrs:
                ctx.free(p)

    def batch(self, queries, form="host"):
        m, L = self.maps[queries[0].map], queries[0].level
        conts, ec, poses = self._pack(queries)
        if form == "host":
            return m.scoreBatch(poses, conts, ec, level=L)
        counts = np.array([len(c) for c in conts], np.int32)
        pts = np.ascontiguousarray(np.concatenate(conts), f32)
        res, lik = np.zeros(len(poses), f32), np.zeros(len(poses), f32)
        self._dev([pts, poses], [res, lik], lambda dp, dw, dr, dl: m.scoreBatch_dev(len(poses), dp, counts, ec, dw, L, dr, dl))
        return res, lik

    def cov(self, queries, form="host"):
        m, L = self.maps[queries[0].map], queries[0].level
        conts, ec, poses = self._pack(queries)
        if form == "host":
            return m.poseCovarianceBatch(poses, conts, ec, level=L)
        counts = np.array([len(c) for c in conts], np.int32)
        pts = np.ascontiguousarray(np.concatenate(conts), f32)
        n = len(poses)
        lik, cm, cw = np.zeros((n, 7), f32), np.zeros((n, 9), f32), np.zeros((n, 9), f32)
        self._dev([pts, poses], [lik, cm, cw],
                  lambda dp, dw, dl, dm, dv: m.poseCovarianceBatch_dev(n, dp, counts, ec, dw, L, dl, dm, dv))
        return lik, cm.reshape(-1, 3, 3), cw.reshape(-1, 3, 3)

    def lattice(self, lat, form="host"):
        m, pts = self.maps[lat.map], self.g.containers[lat.container]
        if form == "host":
            return m.scoreLattice(pts, lat.centre, lat.counts, lat.steps, lat.level)
        nx, ny, nt = lat.counts
        vol, bi, bl = np.zeros(nx * ny * nt, f32), np.zeros(1, np.int32), np.zeros(1, f32)
        self._dev([np.ascontiguousarray(pts, f32)], [vol, bi, bl],
                  lambda dp, dv, di, dl: m.scoreLattice_dev(dp, len(pts), lat.centre, lat.counts, lat.steps, lat.level, dv, di, dl))
        return vol.reshape(nt, ny, nx), int(bi[0]), bl[0]

    def all_states(self, mode, form):
        """(residual[Q], likelihood[Q]) of every recorded query through the batch form: one call per map and level."""
        key = (mode, form)
        if key not in self.cache:
            self.mode(mode)
            qs = S.all_queries()
            res, lik = np.zeros(len(qs), f32), np.zeros(len(qs), f32)
            calls = {}
            for i, q in enumerate(qs):
                calls.setdefault((q.map, q.level), []).append(i)
            for idx in calls.values():
                res[idx], lik[idx] = self.batch([qs[i] for i in idx], form)
            self.cache[key] = (res, lik)
        return self.cache[key]


@pytest.fixture(scope="module")
def env(ctx):
    e = Env(ctx)
    yield e
    e.mode("default")
    for m in e.maps.values():
        m.close()


def bits(a):
    """The float32 words of `a`, every NaN as one word: 0 / 0 is -NaN on the reference's x86 host and +NaN on the device, and
    a NaN's sign and payload are not part of its value."""
    a = np.array(a, f32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def same(a, b):
    return bits(a).tobytes() == bits(b).tobytes()


# ---- ordered mode: the reference, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_ordered_batch_equals_the_reference(env, form):
    res, lik = env.all_states("ordered", form)
    bad = np.nonzero((bits(res) != bits(env.g.residual)) | (bits(lik) != bits(env.g.likelihood)))[0]
    qs = S.all_queries()
    assert not len(bad), (len(bad), [(qs[i], res[i], env.g.residual[i]) for i in bad[:3]])


@pytest.mark.parametrize("form", FORMS)
def test_ordered_lattice_equals_the_reference(env, form):
    env.mode("ordered")
    for name, lat in S.lattices().items():
        vol, bi, bl = env.lattice(lat, form)
        ref = env.g.ref(S.lattice_queries(name))[1]
        assert vol.shape == lat.counts[::-1] and same(vol, ref), name
        want_i, want_v = R.best_state(ref)
        assert bi == want_i and same(bl, want_v), (name, bi, want_i)
    assert env.lattice(S.lattices()["tie"], form)[1] == 0 and env.lattice(S.lattices()["all-nan"], form)[1] == -1


@pytest.mark.parametrize("form", FORMS)
def test_ordered_covariance_equals_the_reference(env, form):
    env.mode("ordered")
    by_level = {}
    for name, q in S.covariances().items():
        by_level.setdefault(q.level, []).append(name)
    for names in by_level.values():
        lik, cm, cw = env.cov([S.covariances()[n] for n in names], form)
        for k, n in enumerate(names):
            ref_lik, ref_cm, ref_cw = env.g.cov[n]
            assert same(lik[k], ref_lik) and same(cm[k], ref_cm) and same(cw[k], ref_cw), n


# ---- default mode: within the bound of the float64 restatement ---------------------------------------------------------------
def test_default_batch_within_the_bound(env):
    res, lik = env.all_states("default", "host")
    res64, lik64 = R.float64_all()
    qs = S.all_queries()
    n = np.array([len(env.g.containers[q.container]) for q in qs], np.float64)
    assert (np.isnan(lik) == np.isnan(lik64)).all() and (res[n == 0] == 0).all()
    d_lik = np.abs(lik.astype(np.float64) - lik64)
    d_res = np.abs(res.astype(np.float64) - res64)
    bound = R.bound()
    worst = int(np.nanargmax(d_lik))
    print("default mode: worst |likelihood - float64| %.3e at %s; worst residual difference / n %.3e; E_ref %.3e, bound %.3e"
          % (d_lik[worst], qs[worst], np.max(d_res[n > 0] / n[n > 0]), R.e_ref(), bound))
    small = n <= 1081
    print("  containers <= 1081 points: worst %.3e; reference's own worst there %.3e"
          % (np.nanmax(d_lik[small]), np.nanmax(np.abs(env.g.likelihood[small] - lik64[small]))))
    assert np.nanmax(d_lik) <= bound
    assert (d_res <= bound * n).all()
    assert same(env.all_states("default", "dev")[0], res) and same(env.all_states("default", "dev")[1], lik)


def test_default_covariance(env):
    env.mode("default")
    worst = 0.0
    for name, q in S.covariances().items():
        lik, cm, cw = env.cov([q])
        lv, pts = env.lv[q.map, q.level], env.g.containers[q.container]
        sp = R.sigma_points(lv.map_pose(np.array([q.pose], f32))[0])
        _, lik64 = R.score64(lv, pts, None, states=sp)
        worst = max(worst, float(np.abs(lik[0] - lik64).max()))
        assert np.abs(lik[0] - lik64).max() <= R.bound(), name
        want_cm, want_cw = R.covariance(sp, lik[0], lv.cell)  # the device's own likelihoods through the fp32 restatement
        assert same(cm[0], want_cm) and same(cw[0], want_cw), name
        dl, dm, dw = env.cov([q], "dev")
        assert same(dl, lik) and same(dm, cm) and same(dw, cw), name
        # the seven states are the batch form's: world pose -> raster, then the sigma offsets
        assert same(lik[0, 6], env.batch([q])[1][0]), name
    print("default mode: worst |sigma likelihood - float64| %.3e" % worst)


# ---- independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_an_entry_does_not_depend_on_its_batch(env, mode):
    env.mode(mode)
    for L in (0, 1, 2):
        qs = S.batch_queries(L)
        res, lik = env.batch(qs)
        for b in S.BATCH_SIZES:  # 1, 3, 4, 5, 9, 130 entries: prefixes straddle the block shape
            r, l = env.batch(qs[:b])
            assert same(r, res[:b]) and same(l, lik[:b]), (L, b)
        alone = range(130) if L == 0 else (0, 1, 2, 63, 64, 129)
        for e in alone:
            r, l = env.batch([qs[e]])
            assert same(r, res[e]) and same(l, lik[e]), (L, e)
        rev_r, rev_l = env.batch(qs[::-1])  # the same entries in other blocks and lanes
        assert same(rev_r[::-1], res) and same(rev_l[::-1], lik), L


@pytest.mark.parametrize("mode", MODES)
def test_lattice_equals_batch_on_host_generated_poses(env, mode):
    env.mode(mode)
    for name, lat in S.lattices().items():
        vol, bi, bl = env.lattice(lat)
        _, lik = env.batch(S.lattice_queries(name))
        assert same(vol, lik), name
        want_i, want_v = R.best_state(vol)
        assert bi == want_i and same(bl, want_v), (name, bi, want_i)
        dvol, dbi, dbl = env.lattice(lat, "dev")
        assert same(dvol, vol) and dbi == bi and same(dbl, bl), name
    assert env.lattice(S.lattices()["tie"])[1] == 0       # two equal best states: the lower index
    assert env.lattice(S.lattices()["all-nan"])[1] == -1  # every likelihood NaN


# ---- purity --------------------------------------------------------------------------------------------------------------------
def test_queries_change_nothing(env, ctx):
    """Planes, lslam_map_cached_points and the cached container (what the next updateByScan feeds to the levels above 0) are
    what they were, after every form in both modes: a twin map that ran none of them ends up with the same planes."""
    m = env.g.maps["main"]
    a, twin = build_map(ctx, m), build_map(ctx, m)
    try:
        before = [a.logodds(L).tobytes() for L in range(3)]
        cached = a.cached_points()
        assert cached == len(m.scans[-1][0])
        qs, lat, cq = S.batch_queries(1)[:9], S.lattices()["5x3x7"], S.covariances()["n257-L0"]
        conts = [env.g.containers[q.container] for q in qs]
        poses = np.array([q.pose for q in qs], f32)
        for ordered in (0, 1):
            a.set_option("ordered_sums", ordered)
            a.scoreBatch(poses, conts, level=1)
            a.poseCovarianceBatch([cq.pose], [env.g.containers[cq.container]], level=0)
            a.scoreLattice(env.g.containers[lat.container], lat.centre, lat.counts, lat.steps, lat.level)
            assert a.cached_points() == cached
            assert [a.logodds(L).tobytes() for L in range(3)] == before
        a.set_option("ordered_sums", 0)
        other, pose = env.g.containers["n257"], S.P("truth")
        for x in (a, twin):
            x.updateByScan(other, (0.0, 0.0), pose)  # levels above 0 take the CACHED container
        for L in range(3):
            assert a.logodds(L).tobytes() == twin.logodds(L).tobytes(), L
        # a pending pipelined apply is enqueued first: the same call after a synchronise gives the same bits
        first = a.scoreBatch(poses, conts, level=1)
        ctx.synchronize()
        again = a.scoreBatch(poses, conts, level=1)
        twin.logodds(1)  # the twin: the same update, applied and read back before it is asked
        assert same(first[1], again[1]) and same(first[1], twin.scoreBatch(poses, conts, level=1)[1])
    finally:
        a.close()
        twin.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(env, ctx):
    env.mode("default")
    m, L = env.maps["main"], env.maps["main"].L
    L.lslam_last_error.restype = C.c_char_p
    c0, c1 = env.g.containers["n63"], env.g.containers["n65"]
    pts = np.ascontiguousarray(np.concatenate([c0, c1]), f32)
    counts = np.array([63, 65], np.int32)
    poses = np.tile(S.P("truth"), (3, 1)).astype(f32)
    res, lik = np.full(3, 7.0, f32), np.full(3, 7.0, f32)
    lik7, cm, cw = np.full((3, 7), 7.0, f32), np.full((3, 9), 7.0, f32), np.full((3, 9), 7.0, f32)
    vol, bi, bl = np.full(8, 7.0, f32), np.full(1, 7, np.int32), np.full(1, 7.0, f32)
    ok_ec = np.array([0, 1, 0], np.int32)

    def score(n, ec, level, cnt=counts):
        return L.lslam_map_score_batch(m.h, n, 2, pts.ctypes.data, cnt.ctypes.data, None if ec is None else ec.ctypes.data,
                                       poses.ctypes.data, level, res.ctypes.data, lik.ctypes.data)

    def cov(n, ec, level):
        return L.lslam_map_pose_covariance_batch(m.h, n, 2, pts.ctypes.data, counts.ctypes.data, ec.ctypes.data, poses.ctypes.data,
                                                 level, lik7.ctypes.data, cm.ctypes.data, cw.ctypes.data)

    def lattice(cnt, level):
        n3, d3 = np.array(cnt, np.int32), np.array([0.05, 0.05, 0.02], f32)
        return L.lslam_map_score_lattice(m.h, c0.ctypes.data, len(c0), poses.ctypes.data, n3.ctypes.data, d3.ctypes.data, level,
                                         vol.ctypes.data, bi.ctypes.data, bl.ctypes.data)

    def refused(rc):
        assert rc == ERR_INVALID_ARGUMENT, rc
        assert len(L.lslam_last_error(ctx.h) or b"") > 0
        for a in (res, lik, lik7, cm, cw, vol, bi, bl):
            assert (a == 7).all()

    for level in (-1, 3, 8):  # a level outside the pyramid
        refused(score(3, ok_ec, level))
        refused(cov(3, ok_ec, level))
        refused(lattice((2, 2, 2), level))
    for bad in ([0, 2, 1], [0, -1, 1]):  # a container index out of range
        refused(score(3, np.array(bad, np.int32), 0))
        refused(cov(3, np.array(bad, np.int32), 0))
    refused(score(3, None, 0))  # NULL indices, 2 containers != 3 entries
    refused(score(2, None, 0, np.array([5, -1], np.int32)))
    for cnt in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):  # a lattice with a non-positive count
        refused(lattice(cnt, 0))
    assert score(0, ok_ec, 0) == 0 and cov(0, ok_ec, 0) == 0  # n_entries == 0: fine, nothing launched
    for a in (res, lik, lik7, cm, cw):
        assert (a == 7).all()
    assert score(3, ok_ec, 2) == 0 and (lik != 7).all()  # and the map still answers


# ---- relocalise ------------------------------------------------------------------------------------------------------------------
def test_relocalise(env):
    """The scan taken at a known pose, a lattice of +-8 cells / +-0.3 rad around a centre 6 cells and 0.2 rad away: the best
    returned pose is what matchData gives when started at the true pose, to the project's 1e-4 m / 1e-4 rad."""
    env.mode("default")
    m, lat = env.maps["main"], S.lattices()["reloc"]
    pts, truth = env.g.containers[lat.container], S.P("truth")
    twin = build_map(env.ctx, env.g.maps["main"])  # matchData caches its container: keep the shared map as it is
    try:
        want, _ = twin.matchData(truth, pts)
    finally:
        twin.close()
    cached = m.cached_points()
    poses, lik, covs = m.relocalise(pts, lat.centre, lat.counts, lat.steps, lat.level, S.RELOC_K)
    assert poses.shape == (S.RELOC_K, 3) and lik.shape == (S.RELOC_K,) and covs.shape == (S.RELOC_K, 3, 3)
    assert (np.diff(lik) <= 0).all() and lik[0] == lik.max() and lik[0] > 0.9
    d = np.abs(poses[0].astype(np.float64) - want)
    print("relocalise: best", poses[0], "matchData from the truth", want, "likelihoods", lik)
    assert d[:2].max() <= 1e-4 and d[2] <= 1e-4, (poses[0], want)
    assert m.cached_points() == cached
