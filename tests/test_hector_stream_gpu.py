"""The streamed HectorSlamProcessor (lslam_hector_*, csrc/logodds_map.hip: k_hs_match_*, k_hs_mark, k_hs_apply) on the scenarios
of tests/hector_stream_cases.py, against the reference's own HectorSlamProcessor (oracle/_ref) and against the host-driven
loop of the same library.  Bounds against the reference are the project's for this path (tests/test_ref_drives_gpu.py:193-225):
the same update decisions, poses within 1e-4, covariance within 2e-3 of max(1, |cov|max), differing cells <= 0.002 of the
non-zero cells per level.  Every test prints what it measured (pytest -s)."""
import numpy as np
import pytest

from lslam_amd import api

import gn_edge_cases as E
import hector_stream_cases as S

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def po(oracle_lib):
    if not oracle_lib.have_ref_hector():
        pytest.skip("oracle/_ref/libhector_ref.so not built (needs the reference's sources at build time)")
    return oracle_lib


def stream(ctx, sc, chunks=None, upto=None, form="points", options=()):
    """-> (map, processor, records) after the scenario went through the processor in calls of `chunks` scans."""
    m = S.device_map(api, ctx, sc)
    h = api.HectorProcessor(m)
    h.set_update_thresholds(sc.min_dist, sc.min_angle)
    for name, value in options:
        h.set_option(name, value)
    n = len(sc.containers) if upto is None else upto
    recs, k = [], 0
    for c in (chunks or [n]):
        hints = None if sc.hints is None else sc.hints[k:k + c]
        flags = [1] * c if sc.no_match else None
        if form == "points":
            recs.append(h.process_many_points(sc.containers[k:k + c], hints, flags))
        else:
            recs.append(h.process_many(sc.ranges[k:k + c], api.hector_scan(sc.laser), hints, flags))
        k += c
    assert k == n
    return m, h, np.concatenate(recs)


def planes(m):
    return [m.logodds(lv) for lv in range(m.levels)]


@pytest.fixture(scope="module")
def chain60_one_call(ctx):
    sc = S.chain60()
    m, h, rec = stream(ctx, sc)
    return sc, m, h, rec, planes(m), h.state(), h.stats()


def test_chain_against_the_reference_processor(po, chain60_one_call):
    """1. (a) in one chained call of 60: decisions, poses, covariances and planes within the bounds of the module docstring."""
    sc, m, h, rec, pl, _, _ = chain60_one_call
    ref = S.reference_run(po, "a", sc)
    S.hold_to_reference("chain60, one call", ref, rec, pl)
    assert np.array_equal(rec["n_points"], [len(c) for c in sc.containers])
    assert np.abs(rec["pose"][-1] - sc.truth[-1]).max() < 0.05


def test_chain_against_the_host_driven_loop(po, ctx, chain60_one_call):
    """2. (a) per scan on a second map of the same library: matchData, the reference's own gate on the host, updateByScan.  The
    matcher's arithmetic is the same, so whatever differs comes from the update geometry's cos / sin (host cosf / sinf there,
    (float)cos((double)) on the device).  The contract is the assertion: same decisions, poses within 1e-4; the bit
    differences are reported."""
    sc, _, _, rec, pl, _, _ = chain60_one_call
    m = S.device_map(api, ctx, sc)
    est, last = np.zeros(3, f32), np.full(3, S.FLT_MAX, f32)
    poses, upd = [], []
    for pts in sc.containers:
        est, _ = m.matchData(est, pts)
        did = po.href_pose_difference_larger_than(est, last, sc.min_dist, sc.min_angle)
        if did:
            m.updateByScan(pts, (0.0, 0.0), est)
            last = est.copy()
        poses.append(est.copy())
        upd.append(did)
    poses = np.array(poses)
    pose_bits = int(np.count_nonzero(poses.view(np.uint32) != rec["pose"].view(np.uint32)))
    cells = [int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))) for a, b in zip(planes(m), pl)]
    print("streamed against host-driven loop: pose words that differ = %d of %d, worst |pose difference| = %.3g, plane "
          "words that differ per level = %s" % (pose_bits, poses.size, np.abs(poses - rec["pose"]).max(), cells))
    assert np.array_equal(np.array(upd), rec["updated"] != 0)
    assert np.abs(poses - rec["pose"]).max() <= S.POSE_TOL
    m.close()


@pytest.mark.parametrize("chunks", [[1] * 60, [7, 13, 40]], ids=["60x1", "7+13+40"])
def test_chunking_changes_nothing(ctx, chain60_one_call, chunks):
    """3. (a) as one call of 60, as 60 calls of 1 and as 7 + 13 + 40: records, planes and state bit-identical; one host
    synchronisation per call."""
    sc, _, _, rec, pl, state, stats = chain60_one_call
    assert (stats["calls"], stats["host_syncs"], stats["scans"]) == (1, 1, 60)
    m, h, rec2 = stream(ctx, sc, chunks)
    assert rec2.tobytes() == rec.tobytes()
    for a, b in zip(planes(m), pl):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(h.state(), state):
        assert a.tobytes() == b.tobytes()
    st = h.stats()
    assert (st["calls"], st["host_syncs"], st["scans"]) == (len(chunks), len(chunks), 60)
    assert st["map_updates"] == stats["map_updates"] == int((rec["updated"] != 0).sum())
    m.close()


def test_mapping_only(po, ctx):
    """4. (b) with every flag set: level 0 bit-equal to the reference processor's, the levels above 0 all zero (nothing was
    ever matched, so nothing is cached for them), every record updated with its hint as pose, bit for bit."""
    sc = S.mapping25()
    ref = S.reference_run(po, "b", sc)
    m, h, rec = stream(ctx, sc)
    pl = planes(m)
    assert pl[0].tobytes() == ref.planes[0].tobytes()
    assert np.count_nonzero(pl[0]) > 1000
    for lv in range(1, sc.levels):
        assert not pl[lv].any() and not ref.planes[lv].any()
    assert (rec["updated"] == 1).all()
    assert rec["pose"].tobytes() == sc.hints.tobytes()
    assert h.stats()["map_updates"] == 25 and m.cached_points() == 0
    m.close()


@pytest.mark.parametrize("levels", [1, 3])
def test_edges(po, ctx, levels):
    """5. (c) on both pyramids against the reference processor; the empty scan in mid-chain."""
    sc = S.edges(levels)
    ref = S.reference_run(po, ("c", levels), sc)
    m, h, rec = stream(ctx, sc)
    S.hold_to_reference("edges, %d level(s)" % levels, ref, rec, planes(m))
    assert np.array_equal(rec["n_points"], [len(c) for c in sc.containers])
    e = rec[S.EDGE_EMPTY]
    assert e["n_points"] == 0 and e["updated"] == 0
    assert e["pose"].tobytes() == rec[S.EDGE_EMPTY - 1]["pose"].tobytes()
    # the state after it is unchanged except lastScanMatchPose: stop a second run right behind the empty scan
    m2, h2, rec2 = stream(ctx, sc, upto=S.EDGE_EMPTY + 1)
    m1, h1, rec1 = stream(ctx, sc, upto=S.EDGE_EMPTY)
    (p2, c2, u2), (p1, c1, u1) = h2.state(), h1.state()
    assert c2.tobytes() == c1.tobytes() and u2.tobytes() == u1.tobytes() and p2.tobytes() == p1.tobytes()
    assert rec2[-1]["cov"].tobytes() == rec1[-1]["cov"].tobytes()
    for a, b in zip(planes(m2), planes(m1)):
        assert a.tobytes() == b.tobytes()
    for x in (m, m1, m2):
        x.close()


@pytest.mark.parametrize("levels", [1, 3])
def test_ranges_form(ctx, levels):
    """6. (c)'s ranges through process_many: records and planes bit-identical to process_many_points fed with what
    lslam_map_set_scan + lslam_map_read_container give for each scan."""
    sc = S.edges(levels)
    probe = S.device_map(api, ctx, sc)
    scan = api.hector_scan(sc.laser)
    conts, origos = [], []
    for r in sc.ranges:
        n = probe.setScan(r, scan)
        pts, origo = probe.container()
        assert len(pts) == n
        conts.append(pts)
        origos.append(origo)
    probe.close()
    assert [len(c) for c in conts] == [len(c) for c in sc.containers]
    m_r, h_r, rec_r = stream(ctx, sc, form="ranges")
    m_p = S.device_map(api, ctx, sc)
    h_p = api.HectorProcessor(m_p)
    h_p.set_update_thresholds(sc.min_dist, sc.min_angle)
    rec_p = h_p.process_many_points(conts, origos_xy=np.array(origos))
    assert rec_r.tobytes() == rec_p.tobytes()
    for a, b in zip(planes(m_r), planes(m_p)):
        assert a.tobytes() == b.tobytes()
    assert h_r.stats()["calls"] == 1
    # the resident container of lslam_map_set_scan is the last streamed scan's
    pts, _ = m_r.container()
    assert pts.tobytes() == conts[-1].tobytes()
    m_r.close()
    m_p.close()


def test_gate_options_thresholds_and_reset(ctx):
    """7. A two-scan chain that turns 0.5 rad in place after the first update: the default gate (abs(int)) does not update,
    FABS_ANGLE_GATE does; changed thresholds are honoured; reset restores FLT_MAX, zero state and an empty map."""
    sc = S.chain60()
    pts = sc.containers[0]
    c, s = np.cos(f32(0.5)), np.sin(f32(0.5))
    turned = np.ascontiguousarray(pts @ np.array([[c, -s], [s, c]], f32))  # the scan as seen after turning by +0.5 rad
    hints = np.array([[0, 0, 0], [0, 0, 0.5]], f32)
    got = {}
    for fabs in (0, 1):
        m = S.device_map(api, ctx, sc)
        h = api.HectorProcessor(m)
        h.set_option("fabs_angle_gate", fabs)
        rec = h.process_many_points([pts, turned], hints)
        got[fabs] = rec
        assert abs(rec["pose"][1][2] - 0.5) < 0.05 and np.abs(rec["pose"][1][:2]).max() < 0.1, rec["pose"]
        if fabs:
            m.close()
            continue
        # thresholds: a heading bound no truncated difference exceeds / a distance bound any distance exceeds
        h.set_update_thresholds(0.4, -1.0)
        assert h.process_many_points([turned], hints[1:])["updated"][0] == 1  # abs(int) = 0 > -1
        h.set_update_thresholds(-1.0, 0.13)
        assert h.process_many_points([turned], hints[1:])["updated"][0] == 1  # distance 0 > -1
        h.set_update_thresholds(0.4, 0.13)
        assert h.process_many_points([turned], hints[1:])["updated"][0] == 0
        assert m.logodds(0).any()
        cov_before = h.state()[1]
        assert cov_before.any()
        h.reset()
        pose, cov, upd = h.state()
        assert not pose.any() and (upd == S.FLT_MAX).all()
        assert cov.tobytes() == cov_before.tobytes()  # HectorSlamProcessor::reset leaves lastScanMatchCov alone
        unmatched = h.process_many_points([pts], hints[:1], [1])  # no match: the record carries the covariance kept
        assert unmatched["cov"][0].tobytes() == cov_before.tobytes() and unmatched["updated"][0] == 1
        h.reset()
        assert not any(p.any() for p in planes(m))
        assert h.process_many_points([pts], hints[:1])["updated"][0] == 1  # FLT_MAX: the first scan updates again
        m.close()
    assert got[0]["updated"].tolist() == [1, 0]
    assert got[1]["updated"].tolist() == [1, 1]
    assert got[0]["pose"].tobytes() == got[1]["pose"].tobytes()


def test_interop_with_the_host_driven_calls(po, ctx):
    """8. The first 30 scans of (a) streamed, the other 30 through matchData / updateByScan on the same map: the cached
    container is the last streamed scan's, and the run ends within the bounds of test 1.  An ordered-sums map is refused."""
    sc = S.chain60()
    ref = S.reference_run(po, "a", sc)
    m, h, rec = stream(ctx, sc, upto=30)
    assert m.cached_points() == len(sc.containers[29])
    est, _, last = h.state()
    out = np.zeros(60, api.HECTOR_RECORD)
    out[:30] = rec
    for k in range(30, 60):
        pts = sc.containers[k]
        est, cov = m.matchData(est, pts)
        did = po.href_pose_difference_larger_than(est, last, sc.min_dist, sc.min_angle)
        if did:
            m.updateByScan(pts, (0.0, 0.0), est)
            last = est.copy()
        out[k]["pose"], out[k]["cov"], out[k]["updated"] = est, cov, did
    S.hold_to_reference("30 streamed + 30 host-driven", ref, out, planes(m))
    m.set_option("ordered_sums", 1)
    with pytest.raises(api.LslamError) as e:
        h.process_many_points(sc.containers[:1])
    assert e.value.code == -8  # LSLAM_ERR_UNSUPPORTED
    m.close()


@pytest.fixture(scope="module")
def gn_maps(ctx):
    """The smallest map of tests/gn_edge_cases.py's geometries, built once under each LSLAM_GN_THREADS."""
    case = E.geometry_case("256x192")
    with pytest.MonkeyPatch.context() as mp:
        dev = E.DeviceMaps(ctx, api, mp, case)
    yield case, dev
    for m in dev.maps.values():
        m.close()


@pytest.mark.parametrize("form", ["reg256", "reg512", "reg1024", "fast-lds", "fast-mem"])
def test_streamed_match_is_match_data_bit_for_bit(gn_maps, form):
    """9. The streamed match IS lslam_map_match_data: one container and start pose through matchData and then, on the same
    map, through a streamed call of one scan with that pose as its hint (the call's capacity is the container's size, so
    both launch the same form; matchData changes no plane, so both see the same map).  The record's 3 pose words and 9
    covariance words equal matchData's, as uint32."""
    case, dev = gn_maps
    pts, begin = case.containers[E.FORM_CONTAINER[form]], case.begin[E.FORM_CONTAINER[form]]
    pose, H = dev.match(form, pts, begin)
    # the streamed scan passes the gate and updates the shared map AFTER its match: the next form's pair sees that map, both halves
    h = api.HectorProcessor(dev.maps[E.SINGLE_FORMS[form][0]])
    rec = h.process_many_points([pts], pose_hints=[begin])[0]
    h.close()
    assert rec["n_points"] == len(pts)
    got = np.concatenate([rec["pose"].ravel(), rec["cov"].ravel()]).view(np.uint32)
    want = np.concatenate([np.asarray(pose, f32).ravel(), np.asarray(H, f32).ravel()]).view(np.uint32)
    assert np.array_equal(got, want), (form, len(pts), got, want)


def test_what_the_kernels_cannot_take_is_refused(ctx):
    """LSLAM_ERR_UNSUPPORTED, before anything is enqueued: more than 65536 readings or points per scan, a pyramid deeper than
    the matcher's 8 levels.  The processor stays usable."""
    sc = S.edges(3)
    m = S.device_map(api, ctx, sc)
    h = api.HectorProcessor(m)
    too_many = (1 << 16) + 1
    with pytest.raises(api.LslamError) as e:
        h.process_many(np.full((1, too_many), np.inf, f32), api.hector_scan(sc.laser))
    assert e.value.code == -8
    with pytest.raises(api.LslamError) as e:
        h.process_many_points([np.zeros((too_many, 2), f32)])
    assert e.value.code == -8
    assert h.stats()["calls"] == 0 and not m.logodds(0).any()
    assert h.process_many_points(sc.containers[:1])["updated"][0] == 1
    deep = api.OccGridMap(ctx, 512, 512, S.CELL, S.offset(512), levels=9)
    assert deep.levels == 9
    hd = api.HectorProcessor(deep)
    with pytest.raises(api.LslamError) as e:
        hd.process_many_points(sc.containers[:1])
    assert e.value.code == -8
    deep.close()
    m.close()
