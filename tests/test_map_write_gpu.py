"""lslam_map_write_logodds[_dev] (api.OccGridMap.write_logodds / write_logodds_dev / save / load): the inverse of the plane
readers.  Map A is mapping25's first 15 scans through HectorProcessor (512^2 x 3 levels), built once; every comparison is of
bytes.  The continuation test is the one of the "untouched by the current scan" rule: A's key planes carry the epochs of its 15
scans, a written-to map's carry none (or a junk scan's), and the same further updates must give the same planes."""
import numpy as np
import pytest

from lslam_amd import api

import hector_stream_cases as S

pytestmark = pytest.mark.gpu
f32 = np.float32
BUILT, CONTINUED = 15, 8  # scans of mapping25 that build A; further scans applied to A and to its copies
INVALID = -1


def planes(m):
    return [m.logodds(lv).tobytes() for lv in range(m.levels)]


@pytest.fixture(scope="module")
def built(ctx):
    sc = S.mapping25()
    a = S.device_map(api, ctx, sc)
    h = api.HectorProcessor(a)
    rec = h.process_many_points(sc.containers[:BUILT], sc.hints[:BUILT], [1] * BUILT)
    assert (rec["updated"] == 1).all()
    want = [a.logodds(lv) for lv in range(a.levels)]
    for p in want:
        p.setflags(write=False)
    assert np.count_nonzero(want[0]) > 100  # (mapping without matching caches no container: the levels above 0 stay empty)
    yield sc, a, want
    a.close()


def copy_of(ctx, sc, a, want, how):
    b = S.device_map(api, ctx, sc)
    for lv in range(a.levels):
        if how == "host":
            b.write_logodds(lv, want[lv])
        else:
            b.write_logodds_dev(lv, a.cells_dev_ptr(lv))
    return b


@pytest.mark.parametrize("how", ["host", "dev"])
def test_round_trip(ctx, built, how):
    """1. every level read from A and written into a fresh map of the same geometry reads back byte-equal; the same through
    write_logodds_dev from A's cells_dev_ptr.  A is unchanged, the copy's containers and counters are a fresh map's."""
    sc, a, want = built
    b = copy_of(ctx, sc, a, want, how)
    assert planes(b) == [p.tobytes() for p in want]
    assert planes(a) == [p.tobytes() for p in want]
    assert b.cached_points() == 0 and len(b.container()[0]) == 0
    b.close()


def continue_on(m, sc, batch):
    """matchData + updateByScan of scans BUILT .. BUILT + CONTINUED at the scenario's poses -> the matchData results, as bytes."""
    out = []
    ks = range(BUILT, BUILT + CONTINUED)
    for k in ks:
        pose, cov = m.matchData(sc.hints[k], sc.containers[k])
        out.append(pose.tobytes() + cov.tobytes())
        if not batch:
            m.updateByScan(sc.containers[k], (0.0, 0.0), sc.hints[k])
    if batch:
        m.updateByScans([sc.containers[k] for k in ks], (0.0, 0.0), [sc.hints[k] for k in ks])
    return out


@pytest.mark.parametrize("batch", [False, True], ids=["pipelined", "batch"])
@pytest.mark.parametrize("how", ["host", "dev", "pending"])
def test_continuation(ctx, built, how, batch):
    """2. the same further matchData + updateByScan sequence on a twin of A that LIVED A's history and on a map that was only
    WRITTEN A's planes: every level byte-equal, every matchData bit-equal -- through the pipelined single update and through
    lslam_map_update_batch.  `pending`: the copy first takes a junk scan whose pipelined apply is still pending when the planes
    are written over it (the write flushes it first, and its marks in the key planes must mean nothing to the next scan)."""
    sc, a, want = built
    twin = S.device_map(api, ctx, sc)  # A's history again (A itself stays what the other tests read)
    api.HectorProcessor(twin).process_many_points(sc.containers[:BUILT], sc.hints[:BUILT], [1] * BUILT)
    assert planes(twin) == [p.tobytes() for p in want]
    if how == "pending":
        b = S.device_map(api, ctx, sc)
        b.matchData((0.0, 0.0, 0.0), sc.containers[3])
        b.updateByScan(sc.containers[3], (0.0, 0.0), (0.3, 0.2, 1.0))  # its apply is pending now
        for lv in range(b.levels):
            b.write_logodds(lv, want[lv])
        assert planes(b) == [p.tobytes() for p in want]
    else:
        b = copy_of(ctx, sc, a, want, how)
    ra, rb = continue_on(twin, sc, batch), continue_on(b, sc, batch)
    pa, pb = planes(twin), planes(b)
    assert ra == rb
    assert pa == pb
    assert pa != [p.tobytes() for p in want]  # (the continuation did change the map)
    twin.close()
    b.close()


def test_special_values_survive(ctx):
    """3. NaN (two payloads), +-inf, -0.0 and a denormal in a few cells come back bit for bit."""
    m = api.OccGridMap(ctx, 64, 48, S.CELL, (1.0, 1.0), levels=2)
    for lv in range(2):
        sx, sy = m.size(lv)
        bits = np.zeros((sy, sx), np.uint32)
        bits[0, 0], bits[1, 2], bits[3, 5] = 0x7FC00000, 0x7F800001, 0xFFC12345   # quiet, signalling, negative NaN
        bits[2, 2], bits[2, 3], bits[4, 4], bits[5, 1] = 0x7F800000, 0xFF800000, 0x80000000, 0x00000001
        bits[sy - 1, sx - 1] = 0x3F800000
        m.write_logodds(lv, bits.view(f32))
        assert m.logodds(lv).tobytes() == bits.tobytes(), lv
    m.close()


def test_refusals_leave_the_map_unchanged(ctx, built):
    """4. a NULL pointer, a level out of range, and -- _dev -- a host pointer: LSLAM_ERR_INVALID_ARGUMENT, planes as before."""
    sc, a, want = built
    L = api.lib()
    host = np.ones_like(want[0])
    for level, ptr in ((0, None), (-1, host.ctypes.data), (a.levels, host.ctypes.data)):
        assert L.lslam_map_write_logodds(a.h, level, ptr) == INVALID
        assert L.lslam_map_write_logodds_dev(a.h, level, ptr if ptr is None else a.cells_dev_ptr(0)) == INVALID
    assert L.lslam_map_write_logodds_dev(a.h, 0, host.ctypes.data) == INVALID  # pageable host memory
    with pytest.raises(ValueError):
        a.write_logodds(0, want[1])  # a plane of another level's size never reaches the library
    assert planes(a) == [p.tobytes() for p in want]


def test_save_and_load(ctx, built, tmp_path):
    """5. save -> load into a fresh map of the same geometry: byte-equal; another geometry or depth is refused."""
    sc, a, want = built
    path = tmp_path / "map.npz"
    a.save(path)
    b = S.device_map(api, ctx, sc)
    b.load(path)
    assert planes(b) == [p.tobytes() for p in want]
    b.close()
    for other in (api.OccGridMap(ctx, sc.n, sc.n, S.CELL, S.offset(sc.n), levels=sc.levels - 1),
                  api.OccGridMap(ctx, sc.n, sc.n, 2 * S.CELL, S.offset(sc.n), levels=sc.levels),
                  api.OccGridMap(ctx, sc.n // 2, sc.n, S.CELL, S.offset(sc.n), levels=sc.levels)):
        with pytest.raises(ValueError):
            other.load(path)
        assert not other.logodds(0).any()
        other.close()
