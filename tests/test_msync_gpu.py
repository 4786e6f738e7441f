"""lslam_msync on the device against the reference's own lesson5 node (po.RefLesson5) and against the Python restatement
(tests/msync_restatement.py, pinned to the node on the CPU by tests/test_msync_cases_oracle.py), on the scenarios of
tests/msync_cases.py: records equal, integrated IMU samples bit for bit, odom_incre within the allowance the restatement
derives per scan for another libm, clouds within the de-skew's pinned 4e-6 m of the node's and bit for bit those of
lslam_deskew_batch fed the device's own windows; chunked calls, the _dev form, reset, growth and refusals.

Measured on the MI355X: every output but odom_incre is bit for bit; odom_incre differed from the host-libm value by at most
4.8e-7 m, a quarter of its allowance at the most (allowances up to 7.6e-6 m); clouds within 7.2e-7 m of the node's."""
import ctypes as C
import functools

import numpy as np
import pytest

import msync_cases as mc
import msync_restatement as mr
from lslam_amd import api

pytestmark = pytest.mark.gpu
CLOUD_CONTRACT = 4e-6  # tests/test_deskew_pin.py


@pytest.fixture(scope="module")
def po(oracle_lib):
    if not oracle_lib.have_ref_lesson5():
        pytest.skip("oracle/_ref not built (needs the reference's sources at build time)")
    return oracle_lib


def combos(name):
    return mc.FLAG_COMBINATIONS if name == "flags" else ((True, True),)


@functools.lru_cache(maxsize=None)
def restated(name, use_imu, use_odom):
    return mr.run(mc.CASES[name](), use_imu=use_imu, use_odom=use_odom)


def push_all(ms, case, imu_from=0, imu_to=None, odom_from=0, odom_to=None):
    ms.push_imu(case["imu_t"][imu_from:imu_to], case["imu_w"][imu_from:imu_to])
    ms.push_odom(case["odom_t"][odom_from:odom_to], case["odom_pos"][odom_from:odom_to], case["odom_quat"][odom_from:odom_to])


def call(ms, case, lo=0, hi=None):
    return ms.scans(case["laser"], case["ranges"][lo:hi], case["scan_t"][lo:hi], case["scan_tinc"][lo:hi], case["imu_seen"][lo:hi],
                    case["odom_seen"][lo:hi])


_DEVICE = {}


def device(ctx, name, use_imu=True, use_odom=True):
    """One whole-log call per (scenario, flags), shared by the tests: (xyz, valid, records, (imu_first, imu_time, imu_rot))."""
    key = (name, use_imu, use_odom)
    if key not in _DEVICE:
        case = mc.CASES[name]()
        ms = api.MotionSync(ctx, use_imu, use_odom)
        push_all(ms, case)
        xyz, valid, rec = call(ms, case)
        win = ms.read_windows(len(rec))
        ms.close()
        for a in (xyz, valid, rec) + win:
            a.setflags(write=False)
        _DEVICE[key] = (xyz, valid, rec, win)
    return _DEVICE[key]


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_records_windows_and_clouds(po, ctx, name):
    case = mc.CASES[name]()
    worst_incre, worst_share, worst_cloud = 0.0, 0.0, 0.0
    for use_imu, use_odom in combos(name):
        want = restated(name, use_imu, use_odom)
        refs = mc.run_reference(po, case, use_imu, use_odom)
        xyz, valid, rec, (first, wt, wr) = device(ctx, name, use_imu, use_odom)
        assert len(rec) == len(want)
        for k, (r, d) in enumerate(zip(want, rec)):
            where = (name, use_imu, use_odom, k)
            # against the restatement: every scan, the flagged and overflow ones included
            assert d["status"] == r["status"], where
            assert (d["scan_time_start"], d["time_increment"]) == (r["scan_time_start"], r["time_increment"]), where
            if use_imu:
                assert d["imu_front"] == r["imu_front"] and d["n_imu"] == r["n_imu"], where
                assert first[k + 1] - first[k] == r["n_imu"], where
                assert wt[first[k]:first[k + 1]].tobytes() == r["imu_time"].tobytes(), where
                assert wr[first[k]:first[k + 1]].tobytes() == r["imu_rot"].tobytes(), where
            if use_odom:
                assert (d["odom_front"], d["start_odom_index"], d["end_odom_index"]) == \
                    (r["odom_front"], r["start_odom_index"], r["end_odom_index"]), where
                assert (d["start_odom_time"], d["end_odom_time"]) == (r["start_odom_time"], r["end_odom_time"]), where
            if r["status"] != mr.CORRECTED:
                assert not xyz[k].any() and not valid[k].any(), where
                continue
            if use_odom:  # tolerance parity: the device libm is not glibc
                allow = mr.odom_increment_allowance(r["start_pose"], r["end_pose"])
                diff = np.abs(d["odom_incre"].astype(np.float64) - r["odom_incre"].astype(np.float64))
                worst_incre = max(worst_incre, diff.max())
                worst_share = max(worst_share, (diff[allow > 0] / allow[allow > 0]).max() if (allow > 0).any() else 0.0)
                assert (diff <= allow).all(), (where, diff, allow)
            # against the reference's own node
            g = refs[k] if k < len(refs) else None
            if g is None:
                continue
            if use_imu:
                assert wt[first[k]:first[k + 1]].tobytes() == g["imu_time"].tobytes(), where
                assert wr[first[k]:first[k + 1]].tobytes() == g["imu_rot"].tobytes(), where
            if use_odom:
                assert (d["start_odom_time"], d["end_odom_time"]) == (g["start_odom_time"], g["end_odom_time"]), where
            assert np.array_equal(valid[k], g["valid"]), where
            ours, theirs = xyz[k][g["valid"]].astype(np.float64), g["xyz"][g["valid"]].astype(np.float64)
            # (start and end odometry message being one message, the node divides 0 by 0 at :441: NaN in both clouds)
            assert np.array_equal(np.isnan(ours), np.isnan(theirs)), where
            err = np.abs(ours - theirs)[~np.isnan(theirs)].max(initial=0.0)
            worst_cloud = max(worst_cloud, err)
            assert err <= CLOUD_CONTRACT, (where, err)
            assert not xyz[k][~g["valid"]].any(), where
    print(name, "odom_incre: worst |device - host libm| %.3g m, worst share of the allowance %.3g; clouds: worst %.3g m"
          % (worst_incre, worst_share, worst_cloud))


def test_an_empty_window_is_corrected_with_zero_rotation(ctx):
    """Edge 1: no sample from start - 0.1 to the scan's end -> n_imu 0, and the cloud is the de-skew's for a single sample of
    rotation 0 (what the node's reset arrays amount to)."""
    case = mc.CASES["imu_gap"]()
    xyz, valid, rec, (first, _, _) = device(ctx, "imu_gap")
    ks = [k for k in range(len(rec)) if rec["status"][k] == mr.CORRECTED and rec["n_imu"][k] == 0]
    assert len(ks) == 1 and first[ks[0] + 1] == first[ks[0]]
    k = ks[0]
    p = params_of(case, rec[k], True, True)
    x1, v1 = api.Deskewer(ctx).batch(case["ranges"][k - 1:k], [p], [np.zeros(1)], [np.zeros((1, 3))])
    assert xyz[k].tobytes() == x1[0].tobytes() and np.array_equal(valid[k], v1[0])
    p.use_imu = 0
    x0, _ = api.Deskewer(ctx).batch(case["ranges"][k - 1:k], [p])
    assert xyz[k].tobytes() == x0[0].tobytes()


def params_of(case, d, use_imu, use_odom):
    return api.DeskewParams(*case["laser"], float(d["scan_time_start"]), float(d["time_increment"]), int(use_imu), int(use_odom),
                            float(d["start_odom_time"]), float(d["end_odom_time"]), *[float(v) for v in d["odom_incre"]], 0.0)


@pytest.mark.parametrize("name", ["steady", "imu_gap", "sparse_odom", "window_sizes", "flags"])
def test_clouds_are_the_batched_deskew_of_the_device_windows(ctx, name):
    case = mc.CASES[name]()
    dk = api.Deskewer(ctx)
    for use_imu, use_odom in combos(name):
        xyz, valid, rec, (first, wt, wr) = device(ctx, name, use_imu, use_odom)
        ks = [k for k in range(len(rec)) if rec["status"][k] == mr.CORRECTED]
        params = [params_of(case, rec[k], use_imu, use_odom) for k in ks]
        times = [wt[first[k]:first[k + 1]] if first[k + 1] > first[k] else np.zeros(1) for k in ks]
        rots = [wr[first[k]:first[k + 1]] if first[k + 1] > first[k] else np.zeros((1, 3)) for k in ks]
        x, v = dk.batch(case["ranges"][[k - 1 for k in ks]], params, times if use_imu else None, rots if use_imu else None)
        assert x.tobytes() == xyz[ks].tobytes(), (name, use_imu, use_odom)
        assert np.array_equal(v, valid[ks])
    dk.close()


@pytest.mark.parametrize("name", ["interleaved", "non_monotone", "front_strides"])
@pytest.mark.parametrize("chunk", [1, 7])
def test_chunked_calls_with_pushes_between_them(ctx, name, chunk):
    """Calls of 1 / 7 messages, the IMU and odometry messages pushed as they arrive between the calls: byte for byte the
    records and clouds of the one call over the whole log."""
    case = mc.CASES[name]()
    xyz, valid, rec, _ = device(ctx, name)
    ms = api.MotionSync(ctx)
    got, ni, no = [], 0, 0
    for lo in range(0, len(rec), chunk):
        hi = min(lo + chunk, len(rec))
        to_i, to_o = int(case["imu_seen"][hi - 1]), int(case["odom_seen"][hi - 1])
        push_all(ms, case, ni, to_i, no, to_o)
        ni, no = to_i, to_o
        got.append(call(ms, case, lo, hi))
    st = ms.stats()
    ms.close()
    assert np.concatenate([g[2] for g in got]).tobytes() == rec.tobytes()
    assert np.concatenate([g[0] for g in got]).tobytes() == xyz.tobytes()
    assert np.array_equal(np.concatenate([g[1] for g in got]), valid)
    n_calls = len(got)
    assert st["callbacks"] == len(rec) and st["launches"] == 3 * n_calls
    assert st["corrected"] == int((rec["status"] == mr.CORRECTED).sum()) and st["refused"] == int((rec["status"] < 0).sum())


def test_the_dev_form_is_the_host_form(ctx):
    case = mc.CASES["interleaved"]()
    xyz, valid, rec, _ = device(ctx, "interleaved")
    n_msgs, n = case["ranges"].shape
    stride = n + 5
    padded = np.full((n_msgs, stride), np.float32(7.0))
    padded[:, :n] = case["ranges"]
    d_r, d_x, d_v, d_rec = ctx.alloc(padded.nbytes), ctx.alloc(xyz.nbytes), ctx.alloc(n_msgs * n), ctx.alloc(rec.nbytes)
    try:
        ctx.upload(d_r, padded)
        ms = api.MotionSync(ctx)
        push_all(ms, case)
        before = ms.stats()["host_waits"]
        ms.scans_dev(case["laser"], n, d_r, stride, case["scan_t"], case["scan_tinc"], d_x, d_v, d_rec, case["imu_seen"],
                     case["odom_seen"])
        ctx.synchronize()
        assert ms.stats()["host_waits"] == before  # the call itself waited for nothing
        x, v, r = np.zeros_like(xyz), np.zeros((n_msgs, n), np.uint8), np.zeros_like(rec)
        ctx.download(d_x, x), ctx.download(d_v, v), ctx.download(d_rec, r)
        ms.close()
    finally:
        for p in (d_r, d_x, d_v, d_rec):
            ctx.free(p)
    assert x.tobytes() == xyz.tobytes() and np.array_equal(v.astype(bool), valid) and r.tobytes() == rec.tobytes()


def test_reset_reproduces_a_fresh_handle_and_a_seen_shape_grows_nothing(ctx):
    case = mc.CASES["odom_wait"]()
    xyz, valid, rec, win = device(ctx, "odom_wait")
    ms = api.MotionSync(ctx)
    push_all(ms, case)
    a = call(ms, case)
    grown = ms.stats()["growths"] + ms.deskewer.stats()["growths"]
    assert grown > 0
    ms.reset()
    assert ms.stats()["callbacks"] == 0 and ms.stats()["corrected"] == 0
    push_all(ms, case)
    b = call(ms, case)
    win_b = ms.read_windows(len(rec))
    assert ms.stats()["growths"] + ms.deskewer.stats()["growths"] == grown  # a second call of a seen shape
    ms.close()
    for got in (a, b):
        assert got[2].tobytes() == rec.tobytes() and got[0].tobytes() == xyz.tobytes() and np.array_equal(got[1], valid)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(win, win_b))


def test_refusals_leave_state_and_outputs_untouched(ctx):
    case = mc.CASES["steady"]()
    xyz, valid, rec, _ = device(ctx, "steady")
    n_msgs, n = case["ranges"].shape
    half = n_msgs // 2
    ms = api.MotionSync(ctx)
    push_all(ms, case)
    first = call(ms, case, 0, half)
    L, laser = ms.L, api.MsyncLaser(*[float(v) for v in case["laser"]])
    t = np.ascontiguousarray(case["scan_t"][half:])
    ti = np.ascontiguousarray(case["scan_tinc"][half:])
    r = np.ascontiguousarray(case["ranges"][half:])
    m = len(t)
    ox, ov, orec = np.full((m, n, 3), np.float32(5.0)), np.full((m, n), np.uint8(9)), np.zeros(m, api.MSYNC_RECORD)
    orec["status"] = 77
    good_i, good_o = np.ascontiguousarray(case["imu_seen"][half:]), np.ascontiguousarray(case["odom_seen"][half:])

    def refused(n_readings=n, seen_i=good_i, seen_o=good_o, deskew=ms.deskewer.h, hdr=laser, stride=n):
        rc = L.lslam_msync_scans(ms.h, deskew, C.byref(hdr) if hdr is not None else None, m, n_readings, r.ctypes.data, stride,
                                 t.ctypes.data, ti.ctypes.data, seen_i.ctypes.data, seen_o.ctypes.data, ox.ctypes.data,
                                 ov.ctypes.data, orec.ctypes.data)
        assert rc == -1, rc  # LSLAM_ERR_INVALID_ARGUMENT
        assert (ox == 5.0).all() and (ov == 9).all() and (orec["status"] == 77).all()

    refused(n_readings=n - 1)  # not the first scan's scan_count_
    refused(seen_i=good_i[::-1].copy())  # decreasing
    refused(seen_o=np.full(m, case["odom_seen"][half - 1] - 1))  # below what the previous call was given
    refused(seen_i=np.full(m, len(case["imu_t"]) + 1))  # more than was pushed
    refused(deskew=None)
    refused(hdr=None)
    refused(stride=n - 1)
    before = ms.stats()
    second = call(ms, case, half, None)
    assert ms.stats()["callbacks"] == before["callbacks"] + m == n_msgs
    ms.close()
    assert np.concatenate([first[2], second[2]]).tobytes() == rec.tobytes()
    assert np.concatenate([first[0], second[0]]).tobytes() == xyz.tobytes()
