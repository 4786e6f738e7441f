"""lesson5's de-skewed cloud into the Hector map on the device: lslam_map_set_cloud (k_hector_cloud_container) against the
numpy restatement of rosPointCloudToDataContainer, and the streamed processor's third input form
(lslam_hector_process_many_deskewed, api.HectorProcessor.process_deskewed) against the container form fed the same
containers, against the host-driven loop of the same library, and across chunkings.  The 12-scan sequence of
tests/deskew_stream_cases.py on 512^2 maps of 2 and 3 levels.  Every test prints what it measured (pytest -s)."""
import numpy as np
import pytest

from lslam_amd import api

import deskew_stream_cases as D
import hector_stream_cases as S

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def po(oracle_lib):
    if not (oracle_lib.have_ref_lesson5() and oracle_lib.have_ref_hector()):
        pytest.skip("oracle/_ref not built (needs the reference's sources at build time)")
    return oracle_lib


@pytest.fixture(scope="module")
def clouds(po, ctx):
    """The sequence, its de-skewed clouds (lslam_deskew_scan per scan) and -- test 1's path -- the containers setCloud makes
    of them, read back."""
    laser, seq = D.sequence12(po)
    scan = D.hector_scan(laser)
    m = D.device_map(ctx, 2)
    xyz, valid, conts = [], [], []
    for s in seq:
        x, v = D.single(ctx, s["ranges"], s["params"], s["times"], s["rots"])
        n = m.setCloud(x, v, scan)
        pts, origo = m.container()
        assert len(pts) == n and origo.tolist() == [0.0, 0.0]
        xyz.append(x)
        valid.append(v)
        conts.append(pts)
    m.close()
    return laser, seq, scan, xyz, valid, conts


def planes(m):
    return [m.logodds(lv) for lv in range(m.levels)]


def stream(ctx, laser, seq, scan, levels, chunks=None, ranges=None):
    m = D.device_map(ctx, levels)
    h = D.processor(m)
    r, params, times, rots = D.batch_inputs(seq)
    r = r if ranges is None else ranges
    recs, k = [], 0
    for c in (chunks or [len(seq)]):
        recs.append(h.process_deskewed(r[k:k + c], scan, params[k:k + c], times[k:k + c], rots[k:k + c]))
        k += c
    assert k == len(seq)
    return m, h, np.concatenate(recs)


@pytest.fixture(scope="module", params=[2, 3], ids=["2_levels", "3_levels"])
def one_call(request, ctx, clouds):
    laser, seq, scan, *_ = clouds
    m, h, rec = stream(ctx, laser, seq, scan, request.param)
    return request.param, m, h, rec, planes(m), h.state(), h.stats()


def test_set_cloud_equals_the_restatement(ctx, clouds):
    """1. setCloud's container == the numpy restatement, bit for bit, order and count: every scan of the sequence (1081 beams:
    two compaction rounds), a non-trivial laser pose, an invalid beam whose zeroed point would pass the filters, the node's
    default z window."""
    laser, seq, scan, xyz, valid, conts = clouds
    m = D.device_map(ctx, 2)
    scale = m.getScaleToMap()
    for k in range(len(seq)):
        want, _ = D.cloud_container(xyz[k], valid[k], scan, scale)
        assert len(want) > 300 and conts[k].shape == want.shape and conts[k].tobytes() == want.tobytes(), k
    assert len(xyz[0]) == 1081 and valid[0][:1024].any() and valid[0][1024:].any()  # kept beams in both rounds of 1024
    posed = D.hector_scan(laser, laser_pose=(0.21, -0.07, 0.35, 0.4))
    n = m.setCloud(xyz[3], valid[3], posed)
    got, origo = m.container()
    want, want_origo = D.cloud_container(xyz[3], valid[3], posed, scale)
    assert n == len(want) > 300 and got.tobytes() == want.tobytes() and origo.tobytes() == want_origo.tobytes()
    assert np.abs(origo).min() > 1.0
    # sqr_laser_min_dist < 0: the zeroed point of an invalid beam (d2 = 0, z = 0) passes every filter -- and must be absent
    lax = D.hector_scan(laser)
    lax.sqr_laser_min_dist = -1.0
    assert len(D.cloud_container(xyz[0], np.ones(1081, bool), lax, scale)[0]) > len(D.cloud_container(xyz[0], valid[0], lax, scale)[0])
    n = m.setCloud(xyz[0], valid[0], lax)
    want, _ = D.cloud_container(xyz[0], valid[0], lax, scale)
    assert n == len(want) > 300 and m.container()[0].tobytes() == want.tobytes()
    # the node's default window (-1, 1): lesson5's z = 1 is outside it
    assert m.setCloud(xyz[0], valid[0], D.hector_scan(laser, (-1.0, 1.0))) == 0
    assert m.container()[0].shape == (0, 2)
    assert m.setCloud(np.zeros((0, 3), f32), np.zeros(0, np.uint8), scan) == 0
    m.close()


def test_deskewed_form_equals_the_container_form(ctx, clouds, one_call):
    """2. process_deskewed == process_many_points fed the containers of test 1's path: records and planes bit-identical (the
    same kernels on the same inputs); afterwards the map's resident container is the last scan's."""
    laser, seq, scan, xyz, valid, conts = clouds
    levels, m, h, rec, pl, state, stats = one_call
    m2 = D.device_map(ctx, levels)
    h2 = D.processor(m2)
    rec2 = h2.process_many_points(conts)
    print("%d levels: points per scan %s, updates %s" % (levels, rec["n_points"].tolist(), rec["updated"].tolist()))
    assert np.array_equal(rec["n_points"], [len(c) for c in conts]) and rec["n_points"].min() > 300
    assert rec.tobytes() == rec2.tobytes()
    for a, b in zip(pl, planes(m2)):
        assert a.tobytes() == b.tobytes()
    assert 2 <= int((rec["updated"] != 0).sum()) < len(seq) and np.count_nonzero(pl[0]) > 1000
    for a, b in zip(state, h2.state()):
        assert a.tobytes() == b.tobytes()
    got, origo = m.container()
    assert got.tobytes() == conts[-1].tobytes() and origo.tolist() == [0.0, 0.0]
    assert m.cached_points() == m2.cached_points() == len(conts[-1])
    m2.close()


def test_against_the_host_driven_loop(po, ctx, clouds, one_call):
    """3. per scan on a second map: deskew_scan -> setCloud -> matchContainer -> the reference's own gate on the host ->
    updateByContainer.  Same decisions, poses within hector_stream_cases.POSE_TOL."""
    laser, seq, scan, xyz, valid, conts = clouds
    levels, _, _, rec, pl, _, _ = one_call
    m = D.device_map(ctx, levels)
    est, last = np.zeros(3, f32), np.full(3, S.FLT_MAX, f32)
    poses, upd = [], []
    for s in seq:
        x, v = D.single(ctx, s["ranges"], s["params"], s["times"], s["rots"])
        if m.setCloud(x, v, scan) > 0:
            est, _ = m.matchContainer(est)
        did = po.href_pose_difference_larger_than(est, last, D.MIN_DIST, S.MIN_ANGLE)
        if did:
            m.updateByContainer(est)
            last = est.copy()
        poses.append(est.copy())
        upd.append(did)
    poses = np.array(poses)
    cells = [int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))) for a, b in zip(planes(m), pl)]
    print("%d levels, streamed against host-driven loop: worst |pose difference| = %.3g, plane words that differ per level = %s"
          % (levels, np.abs(poses - rec["pose"]).max(), cells))
    assert np.array_equal(np.array(upd), rec["updated"] != 0)
    assert np.abs(poses - rec["pose"]).max() <= S.POSE_TOL
    m.close()


@pytest.mark.parametrize("chunks", [[1] * 12, [5, 7]], ids=["12x1", "5+7"])
def test_chunking_changes_nothing(ctx, clouds, one_call, chunks):
    """4. one call of 12, 12 calls of 1 and 5 + 7: records, planes and state bit-identical; one host synchronisation per call."""
    laser, seq, scan, *_ = clouds
    levels, _, _, rec, pl, state, stats = one_call
    assert (stats["calls"], stats["host_syncs"], stats["scans"]) == (1, 1, 12)
    m, h, rec2 = stream(ctx, laser, seq, scan, levels, chunks)
    assert rec2.tobytes() == rec.tobytes()
    for a, b in zip(planes(m), pl):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(h.state(), state):
        assert a.tobytes() == b.tobytes()
    st = h.stats()
    assert (st["calls"], st["host_syncs"], st["scans"]) == (len(chunks), len(chunks), 12)
    assert st["map_updates"] == stats["map_updates"] == int((rec["updated"] != 0).sum())
    m.close()


def test_a_scan_without_a_valid_beam_in_mid_stream(ctx, clouds):
    """5. scan 5 with every range out of the window: an empty container, as in the container form today -- no match, no update,
    the pose of the scan before it; and the records are those of the container form fed an empty container there."""
    laser, seq, scan, xyz, valid, conts = clouds
    r = np.stack([s["ranges"] for s in seq])
    r[5] = np.inf
    m, h, rec = stream(ctx, laser, seq, scan, 3, ranges=r)
    e = rec[5]
    assert e["n_points"] == 0 and e["updated"] == 0
    assert e["pose"].tobytes() == rec[4]["pose"].tobytes() and e["cov"].tobytes() == rec[4]["cov"].tobytes()
    m2 = D.device_map(ctx, 3)
    h2 = D.processor(m2)
    rec2 = h2.process_many_points(conts[:5] + [np.zeros((0, 2), f32)] + conts[6:])
    assert rec.tobytes() == rec2.tobytes()
    for a, b in zip(planes(m), planes(m2)):
        assert a.tobytes() == b.tobytes()
    m.close()
    m2.close()
