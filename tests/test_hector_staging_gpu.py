"""The input staging of the streamed Hector processor and its fleet (lslam_hector_process_many*, lslam_hector_fleet_process_many*):
what one shared host stage can get wrong and no other test reaches.

  1. rows with ranges_stride > n_readings, the padding NaN, against the same rows packed -- through HectorProcessor /
     HectorFleet.process_synced(n_readings=...), and through the library handle for the forms whose Python wrappers always
     pass stride == n_readings
  2. the host cloud form with and without valid bytes and take flags against process_many_clouds_dev on the same data
     uploaded by the test
  3. a call of 1 and then a call of 5 on one handle (the pinned and the device buffers regrow in between) against one call of
     6 on a fresh handle

Every case compares the records as bytes and hector_sync_cases.snapshot (every level's plane, state(), container(), its origo,
cached_points()) of two runs on fresh maps: no tolerance.  Shapes: 6 scans or steps, R = 2, the 360 beams of
hector_sync_cases' "steady" and the 64 of its "window_sizes", the 90 of hector_stream_cases.edges and the 600 of
deskew_stream_cases.edge_batch."""
import ctypes as C

import numpy as np
import pytest

from lslam_amd import api

import deskew_stream_cases as D
import hector_stream_cases as S
import hector_sync_cases as H

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 6
PAD = 5
LEVELS = (3, 2)                 # of the fleet's two members (and the single processor runs on the first)
TAKE = [1, 0, 1, 1, 0, 1]


def padded(r):
    """[..., n] -> [..., n + PAD] with NaN behind every row"""
    out = np.full(r.shape[:-1] + (r.shape[-1] + PAD,), np.nan, f32)
    out[..., :r.shape[-1]] = r
    return out


def same(a, b, what=""):
    for k in a:
        assert a[k] == b[k], (what, k)


class Single:
    def __init__(self, ctx, levels=LEVELS[0], n=D.MAP_N, min_dist=D.MIN_DIST):
        self.m = api.OccGridMap(ctx, n, n, S.CELL, S.offset(n), levels=levels)
        self.m.setUpdateFreeFactor(0.4)
        self.m.setUpdateOccupiedFactor(0.9)
        self.h = api.HectorProcessor(self.m)
        self.h.set_update_thresholds(min_dist, S.MIN_ANGLE)

    def snapshot(self):
        return [H.snapshot(self.m, self.h)]

    def close(self):
        self.m.close()


class Fleet:
    def __init__(self, ctx, n=D.MAP_N, min_dist=D.MIN_DIST):
        self.members = [Single(ctx, lv, n, min_dist) for lv in LEVELS]
        self.fleet = api.HectorFleet([s.h for s in self.members])

    def snapshot(self):
        return [s.snapshot()[0] for s in self.members]

    def close(self):
        for s in self.members:
            s.close()  # (closes its processor, and that its fleets)


def hold(got, want, what):
    """(records, ..., [snapshot per member]) of two runs"""
    for a, b in zip(got[:-1], want[:-1]):
        assert a.tobytes() == b.tobytes(), what
    assert len(got[-1]) == len(want[-1])
    for sa, sb in zip(got[-1], want[-1]):
        same(sa, sb, what)


# ---- 1: strided rows ------------------------------------------------------------------------------------------------------
def edge_ranges():
    sc = S.edges(3)
    return sc, np.ascontiguousarray(sc.ranges[:N])


def run_process_many(ctx, r):
    sc, _ = edge_ranges()
    s = Single(ctx, n=sc.n, min_dist=sc.min_dist)
    scan = api.hector_scan(sc.laser)
    out = np.zeros(N, api.HECTOR_RECORD)
    s.h.ctx.check(s.h.L.lslam_hector_process_many(
        s.h.h, C.byref(scan), N, sc.laser.n_ranges, r.ctypes.data, r.shape[-1], None, None, out.ctypes.data))
    got = (out, s.snapshot())
    s.close()
    return got


def run_fleet_process_many(ctx, r):
    sc, _ = edge_ranges()
    f = Fleet(ctx, n=sc.n, min_dist=sc.min_dist)
    scan = api.hector_scan(sc.laser)
    out = np.zeros((N, 2), api.HECTOR_RECORD)
    f.fleet.ctx.check(f.fleet.L.lslam_hector_fleet_process_many(
        f.fleet.h, C.byref(scan), N, sc.laser.n_ranges, r.ctypes.data, r.shape[-1], None, None, None, out.ctypes.data))
    got = (out, f.snapshot())
    f.close()
    return got


def run_deskewed(ctx, r):
    laser, _, params, times, rots = D.edge_batch()
    s = Single(ctx)
    scan = D.hector_scan(laser)
    arr, first, it, ir = api._deskew_inputs(params, times, rots)
    out = np.zeros(N, api.HECTOR_RECORD)
    s.h.ctx.check(s.h.L.lslam_hector_process_many_deskewed(
        s.h.h, C.byref(scan), N, D.EDGE_N, r.ctypes.data, r.shape[-1], C.addressof(arr), first.ctypes.data, it.ctypes.data,
        ir[0].ctypes.data, ir[1].ctypes.data, ir[2].ctypes.data, None, None, out.ctypes.data))
    got = (out, s.snapshot())
    s.close()
    return got


def steady():
    c = H.case("steady")
    return c, H.scan_args(c, 0, N)


def node(ctx, c):
    ms = api.MotionSync(ctx, c["use_imu"], c["use_odom"])
    H.push_all(ms, c)
    return ms


def run_synced(ctx, r):
    c, (_, t, ti, iseen, oseen) = steady()
    s = Single(ctx)
    ms = node(ctx, c)
    rec, srec = s.h.process_synced(ms, c["laser"], r, H.hector_scan(c), t, ti, iseen, oseen, n_readings=c["ranges"].shape[1])
    got = (rec, srec, s.snapshot())
    ms.close()
    s.close()
    return got


def run_fleet_synced(ctx, r):
    c, (_, t, ti, iseen, oseen) = steady()
    f = Fleet(ctx)
    nodes = [node(ctx, c) for _ in LEVELS]
    two = lambda a: np.ascontiguousarray(np.stack([a, a], 1))  # noqa: E731  ([n, ...] -> [n, R, ...]: both robots hear one log)
    rec, srec = f.fleet.process_synced(nodes, c["laser"], r, H.hector_scan(c), two(t), two(ti), two(iseen), two(oseen),
                                       n_readings=c["ranges"].shape[1])
    got = (rec, srec, f.snapshot())
    for ms in nodes:
        ms.close()
    f.close()
    return got


def _rows(form):
    """-> the form's packed rows: [N, n_readings], or [N, R, n_readings] for the fleet"""
    if form in ("process_many", "fleet_process_many"):
        r = edge_ranges()[1]
    elif form == "deskewed":
        r = np.ascontiguousarray(D.edge_batch()[1], f32)
    else:
        r = np.ascontiguousarray(steady()[1][0], f32)
    assert len(r) == N
    if form == "fleet_process_many":
        r = np.stack([r, r[::-1]], 1)  # the second robot drives the stretch backwards
    elif form == "fleet_synced":
        r = np.stack([r, r], 1)        # (its callbacks' stamps tie a log's scans to their order)
    return np.ascontiguousarray(r)


RUNNERS = {"process_many": run_process_many, "deskewed": run_deskewed, "fleet_process_many": run_fleet_process_many,
           "synced": run_synced, "fleet_synced": run_fleet_synced}


@pytest.mark.parametrize("form", sorted(RUNNERS))
def test_strided_rows_equal_packed_rows(ctx, form):
    """1. ranges_stride = n_readings + 5 with NaN in the padding gives the bytes of the packed rows."""
    r = _rows(form)
    nr = r.shape[-1]
    wide = padded(r)
    assert wide.shape[-1] == nr + PAD and np.isnan(wide[..., nr:]).all() and wide.flags.c_contiguous
    want = RUNNERS[form](ctx, r)
    got = RUNNERS[form](ctx, wide)
    rec = want[0]
    print(form, "points", rec["n_points"].reshape(-1).tolist(), "updates", rec["updated"].reshape(-1).tolist())
    assert rec["n_points"].max() > 40 and (rec["updated"] != 0).any()
    hold(got, want, form)


# ---- 2, 3: the host cloud form --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clouds(ctx):
    """window_sizes' six CORRECTED callbacks as MotionSync.scans gives them: 64-point clouds; the fleet's second member hears
    them in reverse order, and takes what the first does not."""
    c = H.case("window_sizes")
    ms = node(ctx, c)
    xyz, valid, srec = ms.scans(c["laser"], *H.scan_args(c, 0, N + 1))
    ms.close()
    assert srec["status"].tolist() == [0] + [1] * N and xyz.shape == (N + 1, 64, 3)
    x, v = np.ascontiguousarray(xyz[1:], f32), np.ascontiguousarray(valid[1:]).astype(bool)
    # every fifth point that is a point is declared invalid, another fifth in every scan: the valid bytes, and which row they
    # belong to, then decide what the container holds
    v &= (np.arange(64)[None, :] + np.arange(N)[:, None]) % 5 != 2
    assert (v.sum(1) >= 40).all() and (v.sum(1) <= 52).all()
    t = np.array(TAKE, bool)
    out = {"scan": H.hector_scan(c), "x": x, "v": v, "t": t,
           "X": np.ascontiguousarray(np.stack([x, x[::-1]], 1)), "V": np.ascontiguousarray(np.stack([v, v[::-1]], 1)),
           "T": np.ascontiguousarray(np.stack([t, ~t], 1))}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


class Uploaded:
    """host arrays in HBM for the length of a with block"""

    def __init__(self, ctx, *arrays):
        self.ctx, self.arrays, self.ptrs = ctx, arrays, []

    def __enter__(self):
        for a in self.arrays:
            if a is None:
                self.ptrs.append(None)
                continue
            a = np.ascontiguousarray(a)
            p = self.ctx.alloc(a.nbytes)
            self.ctx.upload(p, a)
            self.ptrs.append(p)
        return self.ptrs

    def __exit__(self, *exc):
        for p in self.ptrs:
            if p is not None:
                self.ctx.free(p)


COMBINATIONS = [(False, False), (True, False), (False, True), (True, True)]
IDS = ["plain", "valid", "take", "valid_take"]


@pytest.mark.parametrize("with_valid,with_take", COMBINATIONS, ids=IDS)
def test_host_cloud_form_equals_the_dev_form(ctx, clouds, with_valid, with_take):
    """2. process_many_clouds(valid or None, take or None) == process_many_clouds_dev on the same arrays uploaded here."""
    x, scan = clouds["x"], clouds["scan"]
    v = clouds["v"] if with_valid else None
    t = clouds["t"] if with_take else None
    a = Single(ctx)
    got = (a.h.process_many_clouds(x, scan, v, take=t), a.snapshot())
    a.close()
    b = Single(ctx)
    with Uploaded(ctx, x, None if v is None else v.astype(np.uint8), None if t is None else t.astype(np.int32)) as (dx, dv, dt):
        want = (b.h.process_many_clouds_dev(N, 64, dx, dv, dt, 1, scan), b.snapshot())
    b.close()
    rec = want[0]
    print("valid", with_valid, "take", with_take, "points", rec["n_points"].tolist(), "updates", rec["updated"].tolist())
    taken = clouds["t"] if with_take else np.ones(N, bool)
    assert all(H.not_taken(r) for r in rec[~taken]) and (rec["updated"] != 0).any()
    assert ((rec["n_points"][taken] > 30) & ((rec["n_points"][taken] <= 52) == with_valid)).all()  # the valid bytes decide
    hold(got, want, "single")


@pytest.mark.parametrize("with_valid,with_take", COMBINATIONS, ids=IDS)
def test_fleet_host_cloud_form_equals_the_dev_form(ctx, clouds, with_valid, with_take):
    """2, for the fleet: one block per member in HBM, member m's row of step k being k rows into it."""
    X, scan = clouds["X"], clouds["scan"]
    V = clouds["V"] if with_valid else None
    T = clouds["T"] if with_take else None
    a = Fleet(ctx)
    got = (a.fleet.process_many_clouds(X, scan, V, take=T), a.snapshot())
    a.close()
    b = Fleet(ctx)
    blocks = []
    for m in range(2):
        blocks += [X[:, m], None if V is None else V[:, m].astype(np.uint8), None if T is None else T[:, m].astype(np.int32)]
    with Uploaded(ctx, *blocks) as p:
        want = (b.fleet.process_many_clouds_dev(N, 64, p[0::3], None if V is None else p[1::3], None if T is None else p[2::3], 1,
                                                scan), b.snapshot())
    b.close()
    rec = want[0]
    print("valid", with_valid, "take", with_take, "points", rec["n_points"].tolist(), "updates", rec["updated"].tolist())
    taken = clouds["T"] if with_take else np.ones((N, 2), bool)
    assert all(H.not_taken(r) for r in rec[~taken]) and (rec["updated"] != 0).any()
    assert ((rec["n_points"][taken] > 30) & ((rec["n_points"][taken] <= 52) == with_valid)).all()  # the valid bytes decide
    hold(got, want, "fleet")


def test_regrowth_between_two_calls(ctx, clouds):
    """3. 1 scan, then 5 on the same handle, equals 6 in one call on a fresh one."""
    x, v, t, scan = clouds["x"], clouds["v"], clouds["t"], clouds["scan"]
    a = Single(ctx)
    first = a.h.process_many_clouds(x[:1], scan, v[:1], take=t[:1])
    rest = a.h.process_many_clouds(x[1:], scan, v[1:], take=t[1:])
    got = (np.concatenate([first, rest]), a.snapshot())
    a.close()
    b = Single(ctx)
    want = (b.h.process_many_clouds(x, scan, v, take=t), b.snapshot())
    b.close()
    assert (want[0]["n_points"][t] > 30).all()
    hold(got, want, "single")


def test_fleet_regrowth_between_two_calls(ctx, clouds):
    """3, for the fleet: 1 step, then 5."""
    X, V, T, scan = clouds["X"], clouds["V"], clouds["T"], clouds["scan"]
    a = Fleet(ctx)
    first = a.fleet.process_many_clouds(X[:1], scan, V[:1], take=T[:1])
    rest = a.fleet.process_many_clouds(X[1:], scan, V[1:], take=T[1:])
    got = (np.concatenate([first, rest]), a.snapshot())
    a.close()
    b = Fleet(ctx)
    want = (b.fleet.process_many_clouds(X, scan, V, take=T), b.snapshot())
    b.close()
    assert (want[0]["n_points"][T] > 30).all()
    hold(got, want, "fleet")
