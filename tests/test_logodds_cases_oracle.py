"""The scenarios of tests/logodds_cases.py are what they claim to be -- checked on the CPU with the oracle and plain
geometry, so that no test of tests/test_logodds_edges_gpu.py can pass vacuously -- and, where the reference's own headers
are built, oracle/hector_oracle.c equals them bit for bit on these scenarios too: they are where the restatement and the
kernels could share a mistake (util::sign(0) = -1 on axis rays, truncation toward zero in (int)(x + 0.5f), the x86 cast of
out-of-range values)."""
import ctypes as C
import functools

import numpy as np
import pytest

import logodds_cases as E
from lslam_amd import api

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------
def test_scenarios_have_the_stated_shapes():
    for name in E.NAMES:
        sc = E.scenario(name)
        assert sc.routes == tuple(E.ROUTES_OF.get(name, E.ROUTES)), name
        assert len(sc.reach) == len(sc.scans) and max(len(p) for p, _, _ in sc.scans) <= E.MAX_POINTS
        assert E.call_cuts(sc)[-1] == len(sc.scans) and E.checkpoints(sc)[-1] == len(sc.scans)
    assert len(E.scenario("sweep").scans) == 19880 + 2 * 360
    assert len(E.scenario("pairs").scans) == 121 ** 2 and len(E.scenario("triples").scans) == 25 ** 3
    odd = E.scenario("sweep").map
    assert (odd.sx, odd.sy) == (149, 147) and odd.sx % 8 == 5 and odd.sy % 8 == 3          # overhanging tiles 5 wide, 3 high
    assert E.level_dims(E.scenario("pyramid_odd").map) == [(149, 147), (74, 73), (37, 36)]
    # more than 300 batched calls on one map: the 6-bit pool epoch (cleared every 63 rounds) wraps several times
    assert len(E.call_cuts(E.scenario("sweep"))) - 1 > 300
    st = E.scenario("long_steep")
    assert len(st.scans) * 16 == 64 and abs(st.map.sx - 8200) < 100 and abs(st.map.sy - 4200) < 100


def test_beam_counts_straddle_every_switch():
    """k_lo_batch_hits_lds builds a scan's hash in LDS while slots * 8 <= 64 KB, slots the power of two >= 2 * the longest
    scan of the group (update_batch_impl): 4096 points -> 8192 slots = 64 KB, the largest LDS case; 4097 -> 16384 slots, the
    first for the global-memory k_lo_batch_hits."""
    def slots(n):
        s = 64
        while s < 2 * n:
            s *= 2
        return s
    assert slots(4096) * 8 == 64 * 1024 and slots(4097) * 8 > 64 * 1024 and slots(2049) * 8 == 64 * 1024 > slots(2048) * 8
    sc = E.scenario("beam_counts")
    big = sc.notes["big"]
    assert [len(sc.scans[k][0]) for k in big[0::2]] == list(E.BEAM_COUNTS) == [len(sc.scans[k][0]) for k in big[1::2]]
    cuts = E.call_cuts(sc)
    for alone, inside in zip(big[0::2], big[1::2]):
        assert alone in cuts and alone + 1 in cuts                                       # a call of its own
        a = max(c for c in cuts if c <= inside)
        b = min(c for c in cuts if c > inside)
        assert b - a == 5 and a < inside < b - 1
        assert [len(sc.scans[k][0]) for k in range(a, b) if k != inside] == [1] * 4      # the other scans have one point
    assert {4096, 4097, 65536} <= set(E.BEAM_COUNTS) and E.MAX_POINTS == 65536


def test_long_thin_lengths_and_the_predecessor_guard():
    for name, side in (("long_thin_x32768", 32768), ("long_thin_y32768", 32768), ("long_thin_x70001", 70001)):
        sc = E.scenario(name)
        axis = 1 if "_y" in name else 0
        assert (sc.map.sx, sc.map.sy)[axis] == side and (sc.map.sx, sc.map.sy)[1 - axis] == 5
        seen, minors = set(), set()
        for pts, _, pose in sc.scans:
            length = np.abs(pts[:, axis]).astype(int)
            seen |= set(length.tolist())
            minors |= set(pts[:, 1 - axis].astype(int).tolist())
            end = pose[axis] + pts[:, axis]
            assert end.min() >= 0 and end.max() <= side - 1
            if side > 65536:  # a ray past the abs_da < 65536 guard after a shorter one and before one
                k = int(np.flatnonzero(length >= 65536)[0])
                assert 0 < k < len(length) - 1 and length[k - 1] < 65536 and (length[k + 1:] < 65536).any()
        want = {63, 64, 65, 255, 256, 257, 511, 512, 513, 32766, 32767}
        assert seen == (want | {65535, 65536, 65537, 69998} if side > 65536 else want)
        assert minors == {0, 1, -1, 2, -2}


# ---------------------------------------------------------------------------------------------------------------------------
# sweep: octants, from the end offsets alone
# ---------------------------------------------------------------------------------------------------------------------------
def test_sweep_covers_every_octant_and_length():
    off = E.scenario("sweep").notes["offsets"][0]
    dx, dy = off[:, 0], off[:, 1]
    adx, ady = np.abs(dx), np.abs(dy)
    for sgx in (1, -1):
        for sgy in (1, -1):
            for xmajor in (True, False):  # the eight octants, strictly inside
                inside = (dx * sgx > 0) & (dy * sgy > 0) & ((adx > ady) if xmajor else (ady > adx))
                assert inside.sum() > 1000, (sgx, sgy, xmajor)
            assert ((dx * sgx > 0) & (dy * sgy > 0) & (adx == ady)).sum() == 70   # the four diagonals
    for axis_rays in ((dy == 0) & (dx > 0), (dy == 0) & (dx < 0), (dx == 0) & (dy > 0), (dx == 0) & (dy < 0)):
        assert axis_rays.sum() == 70                                              # both axes, both ways: sign(0) = -1 matters
    major = np.maximum(adx, ady)
    assert set(major.tolist()) == set(range(1, 71))                               # every length on either side of 64
    assert (major == 63).any() and (major == 64).any() and (major == 65).any()


@functools.lru_cache(maxsize=None)
def visited(x0, y0, x1, y1):
    return frozenset(E.stepped_cells(x0, y0, x1, y1))


def test_stepped_traversal_equals_the_oracle(oracle_lib):
    """one ray per octant, axis and diagonal on a fresh map each: the cells the oracle lowered are stepped_cells()'"""
    for dx, dy in ((9, 4), (4, 9), (-9, 4), (-4, 9), (9, -4), (4, -9), (-9, -4), (-4, -9), (7, 0), (-7, 0), (0, 7), (0, -7),
                   (6, 6), (-6, 6), (6, -6), (-6, -6), (64, 1), (1, -65), (70, 69)):
        o = oracle_lib.PortHector(149, 147, 1.0, (0.0, 0.0))
        o.updateByScan(np.array([[dx, dy]], F32), (0.0, 0.0), (74.0, 73.0, 0.0))
        a = o.logodds()
        ys, xs = np.nonzero(a < 0)
        assert set(zip(xs.tolist(), ys.tolist())) == set(visited(74, 73, 74 + dx, 73 + dy)), (dx, dy)
        ys, xs = np.nonzero(a > 0)
        assert list(zip(xs.tolist(), ys.tolist())) == [(74 + dx, 73 + dy)]


# ---------------------------------------------------------------------------------------------------------------------------
# sweep_rim
# ---------------------------------------------------------------------------------------------------------------------------
def one_scan_on_a_fresh_map(oracle_lib, sc, k):
    o = E.make_oracle(oracle_lib, sc.map)
    E.oracle_feed(o, sc.map, sc.scans[k])
    return o.logodds()


def test_sweep_rim_effects(oracle_lib):
    sc = E.scenario("sweep_rim")
    sx, sy = sc.map.sx, sc.map.sy
    ends = sc.notes["ends"]
    outside = (ends[:, 0] < 0) | (ends[:, 0] >= sx) | (ends[:, 1] < 0) | (ends[:, 1] >= sy)
    last = ~outside & ((ends[:, 0] == sx - 1) | (ends[:, 1] == sy - 1))
    assert outside.sum() >= 100 and last.sum() >= 100 and (~outside).sum() >= 100
    # ... which the oracle agrees with, beam by beam (a sample: every 7th scan)
    for k in range(0, sc.notes["n_int"], 7):
        a = one_scan_on_a_fresh_map(oracle_lib, sc, k)
        if outside[k] or tuple(ends[k]) == tuple(sc.notes["begins"][k]):   # (begin == end: the beam is skipped, :155)
            assert not a.any(), k
        else:
            assert a[ends[k, 1], ends[k, 0]] > 0 and (a > 0).sum() == 1, k
    # the fractional coordinates at the truncation edges
    assert len(sc.notes["fractions"]) == 12
    for f in sc.notes["fractions"]:
        a = one_scan_on_a_fresh_map(oracle_lib, sc, f["scan"])
        if f["cell"] is None:
            assert not a.any(), f
        else:
            ys, xs = np.nonzero(a > 0)
            assert list(zip(xs.tolist(), ys.tolist())) == [f["cell"]], f
    by_coord = {(f["axis"], f["coord"]): f["cell"] for f in sc.notes["fractions"]}
    assert [f["cell"] for f in sc.notes["fractions"] if f["coord"] not in (-1.6, -1.4, -0.6, -0.4, 148.5, 146.5)] == [(148, 80), (81, 146)]
    assert by_coord[(0, -1.4)] == (0, 80) and by_coord[(0, -1.6)] is None and by_coord[(1, -1.4)] == (81, 0)
    assert by_coord[(0, 148.5)] is None and by_coord[(1, 146.5)] is None
    # a begin cell put at -0.7 by the pose is cell 0; a begin cell outside the map drops every beam
    a = one_scan_on_a_fresh_map(oracle_lib, sc, sc.notes["inside"]["scan"])
    assert a[73, 0] < 0 and (a > 0).sum() >= 3
    for k in sc.notes["outside"]:
        assert not one_scan_on_a_fresh_map(oracle_lib, sc, k).any(), k


# ---------------------------------------------------------------------------------------------------------------------------
# pairs, triples: beam order
# ---------------------------------------------------------------------------------------------------------------------------
def order_kinds(offsets):
    """-> per scan: (a hit cell crossed by an earlier beam, a hit cell crossed only by a later beam, two beams ending in one
    cell, beam 1 visiting a cell of beam 0 besides the begin cell), from stepped_cells() alone"""
    x0, y0 = E.SMALL_START
    out = np.zeros((len(offsets), 4), bool)
    for k, beams in enumerate(offsets):
        beams = [(int(dx), int(dy)) for dx, dy in beams if dx or dy]   # begin == end: the beam is skipped (:155)
        cells = [visited(x0, y0, x0 + dx, y0 + dy) for dx, dy in beams]
        ends = [(x0 + dx, y0 + dy) for dx, dy in beams]
        for j, e in enumerate(ends):
            if e in ends[:j]:
                out[k, 2] = True
                continue  # not the first beam ending here
            before = any(e in c for c in cells[:j])
            after = any(e in c for c in cells[j + 1:])
            out[k, 0] |= before
            out[k, 1] |= after and not before
        if len(beams) >= 2 and len(offsets[k]) == len(beams):
            out[k, 3] = len((cells[0] & cells[1]) - {(x0, y0)}) > 0
    return out


def test_beam_order_coverage():
    """pairs and triples together hold at least 1000 scans of each order of hitting and crossing; pairs alone at least 1000
    on which the predecessor skip of logodds_mark_wave fires; triples the order ender, crosser, ender in every direction"""
    kp, kt = order_kinds(E.scenario("pairs").notes["offsets"]), order_kinds(E.scenario("triples").notes["offsets"])
    crossed_earlier, crossed_later_only, same_end, _ = kp.sum(axis=0) + kt.sum(axis=0)
    assert crossed_earlier >= 1000 and crossed_later_only >= 1000 and same_end >= 1000, (kp.sum(axis=0), kt.sum(axis=0))
    assert (kp.sum(axis=0)[:3] >= 100).all() and (kt.sum(axis=0)[:3] >= 1000).all()
    assert kp[:, 3].sum() >= 1000
    x0, y0 = E.SMALL_START
    directions = set()
    for beams in E.scenario("triples").notes["offsets"]:
        (a, b, c) = [(int(dx), int(dy)) for dx, dy in beams]
        if a == c and a != (0, 0) and b != (0, 0) and (x0 + a[0], y0 + a[1]) in visited(x0, y0, x0 + b[0], y0 + b[1]):
            directions.add(a)  # beam 0 ends in a cell, beam 1 crosses it, beam 2 ends there again
    assert len(directions) == 8, directions  # the eight neighbours of the begin cell: a box of 2 has no other crossed ends


def test_pairs_reach_the_clamp(oracle_lib):
    top = max(float(p[0][0].max()) for p in E.expected(oracle_lib, "pairs").values())
    assert 50.0 <= top < 50.0 + 0.41  # updateSetOccupied adds below 50 only (H/map/GridMapLogOdds.h:108-114)


# ---------------------------------------------------------------------------------------------------------------------------
# long_steep: the float quotient
# ---------------------------------------------------------------------------------------------------------------------------
def test_long_steep_makes_the_float_quotient_wrong():
    wrong = 0
    for da, db in E.scenario("long_steep").notes["rays"]:
        assert da >= db and 50 + da < E.STEEP.sx and 50 + db < E.STEEP.sy
        q0, q, exact = E.estimate_q(da, db)
        assert np.array_equal(q, exact)          # the corrections mend it
        assert np.abs(q0 - exact).max() <= 2     # ... and are enough
        wrong += int((q0 != exact).sum())
    assert wrong >= 100, wrong


# ---------------------------------------------------------------------------------------------------------------------------
# knife_edge
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
def test_knife_edge_points_sit_on_cell_borders(oracle_lib, level):
    sc = E.scenario(f"knife_edge_l{level}")
    m = sc.map
    changed = {how: 0 for how in E.ALTERNATIVES + ("factor_late",)}
    n_points = 0
    for pts, origo, pose in sc.scans[:sc.notes["n_unique"]]:
        tf = E.pose_transform(m, level, pose)
        vx, vy = E.end_coord(tf, 0, pts[:, 0], pts[:, 1]), E.end_coord(tf, 1, pts[:, 0], pts[:, 1])
        # the float64 emulation of the reference's order IS float32 arithmetic in that order
        c, s, tx, ty, factor = tf
        px, py = pts[:, 0] * factor, pts[:, 1] * factor
        assert np.array_equal(vx, ((c * px + (-s) * py) + tx) + F32(0.5)) and np.array_equal(vy, ((s * px + c * py) + ty) + F32(0.5))
        ulps = np.minimum(np.abs(vx - np.round(vx)) / np.spacing(np.round(vx)), np.abs(vy - np.round(vy)) / np.spacing(np.round(vy)))
        assert (ulps <= 2.0).all()
        # ... and the oracle puts every point's hit where that arithmetic says (one beam on a fresh level each)
        cells = np.stack([vx.astype(np.int64), vy.astype(np.int64)], axis=1)
        sxl, syl = m.sx >> level, m.sy >> level
        assert (cells >= 0).all() and (cells[:, 0] < sxl).all() and (cells[:, 1] < syl).all()
        cell_l = float(F32(m.cell) * F32(2 ** level))
        for i in range(0, len(pts), 3):
            o = oracle_lib.PortHector(sxl, syl, cell_l, m.offset)
            o.updateByScan(pts[i:i + 1] * factor, origo * factor, pose)
            ys, xs = np.nonzero(o.logodds() > 0)
            assert list(zip(xs.tolist(), ys.tolist())) == [tuple(cells[i])], (i, cells[i])
        for how in changed:
            ax, ay = E.end_coord(tf, 0, pts[:, 0], pts[:, 1], how), E.end_coord(tf, 1, pts[:, 0], pts[:, 1], how)
            changed[how] += int(((ax.astype(np.int64) != cells[:, 0]) | (ay.astype(np.int64) != cells[:, 1])).sum())
        n_points += len(pts)
    assert n_points == 128
    for how in E.ALTERNATIVES:
        assert changed[how] >= 32, changed
    # (c * px) * factor against c * (px * factor): the factor of a pyramid level is a power of two (MapRepMultiMap.h:161), and
    # scaling by one commutes with every float32 rounding short of underflow -- this rewrite cannot move a point, on any level
    assert changed["factor_late"] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# just_once
# ---------------------------------------------------------------------------------------------------------------------------
def test_just_once_rounds_half_away_from_zero_in_double(oracle_lib):
    m = E.JUST_ONCE
    bx, by = (int(v) for v in E.JUST_ONCE_BEGIN)
    ties = below = above = 0
    for pts in E.just_once_points()[:3]:
        for p in pts:
            o = oracle_lib.PortHector(m.sx, m.sy, m.cell, m.offset)
            o.updateByScanJustOnce(p[None, :], (0.0, 0.0), E.JUST_ONCE_BEGIN, 0.05)
            r = [float(v) / 0.05 for v in p]                      # float / double, in double (:202-203)
            cell = [b + int(np.floor(abs(v) + 0.5) * np.sign(v)) for b, v in zip((bx, by), r)]   # round(): half away from zero
            frac = [abs(v) % 1.0 - 0.5 for v in r]
            ties += any(f == 0.0 for f in frac)
            below += any(-1e-5 < f < 0.0 for f in frac)
            above += any(0.0 < f < 1e-5 for f in frac)
            ys, xs = np.nonzero(o.logodds() > 0)
            got = list(zip(xs.tolist(), ys.tolist()))
            inside = 0 <= cell[0] < m.sx and 0 <= cell[1] < m.sy and (cell[0], cell[1]) != (bx, by)
            assert got == ([tuple(cell)] if inside else []), (p, cell, got)
    # 0.05 is no float: (k + 0.5) * 0.05f / 0.05 is k + 0.5 only by luck, but its float neighbours straddle it closely
    assert ties >= 1 and below >= 40 and above >= 40, (ties, below, above)
    o = oracle_lib.PortHector(m.sx, m.sy, m.cell, m.offset)
    o.updateByScanJustOnce(E.just_once_points()[3], (0.0, 0.0), E.JUST_ONCE_BEGIN, 0.05)
    assert (o.logodds() > 0).sum() == 3  # NaN, +-Inf and 3e9 are dropped; the three finite points are not


# ---------------------------------------------------------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------------------------------------------------------
def plan(sx, sy, begins, counts, reach, budget):
    L = api.lib()
    L.lslam_map_plan_batch_windows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                               C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    k = len(counts)
    b = np.ascontiguousarray(begins, dtype=np.int32).reshape(k, 2)
    n = np.ascontiguousarray(counts, dtype=np.int32)
    r = np.ascontiguousarray(reach, dtype=np.float64)
    win, base, rnd = np.zeros((k, 4), np.int32), np.zeros(k, np.uint32), np.zeros(k, np.int32)
    rc = L.lslam_map_plan_batch_windows(sx, sy, k, b.ctypes.data, n.ctypes.data, r.ctypes.data, 1.0, budget, win.ctypes.data,
                                        base.ctypes.data, rnd.ctypes.data, None)
    return rc, win


def test_window_coverage():
    """what the batch_windows route relies on: at a 1 MB budget the host measures the reach on these maps, a 64-scan call of
    sweep takes two rounds or more, and most windows of sweep_rim are smaller than the map (clipped by its rim)"""
    sw, rim = E.scenario("sweep"), E.scenario("sweep_rim")
    m = sw.map
    assert E.host_measures_reach(m) and E.host_measures_reach(E.scenario("long_thin_x32768").map)
    assert E.host_measures_reach(E.NON_FINITE_MAP) and not E.host_measures_reach(E.SMALL) and not E.host_measures_reach(E.FAN_MAP)
    reach = [E.host_reach(p, o) for p, o, _ in sw.scans[:64]]
    rc, _ = plan(m.sx, m.sy, sw.notes["begins"][:64], [1] * 64, reach, E.MB)
    assert rc >= 2
    whole = ((m.sx + 7) // 8) * ((m.sy + 7) // 8)
    reach = [E.host_reach(p, o) for p, o, _ in rim.scans]
    rc, win = plan(m.sx, m.sy, rim.notes["begins"], [len(p) for p, _, _ in rim.scans], reach, E.MB)
    size = win[:, 2].astype(np.int64) * win[:, 3]
    assert rc >= 1 and ((size > 0) & (size < whole)).sum() >= len(rim.scans) // 2
    # ... and the stated reach (the hint of the batch_dev_hint route) is never below what the host would measure itself
    for sc in (sw, rim, E.scenario("beam_counts")):
        for k in range(0, len(sc.scans), 97):
            assert sc.reach[k] + 2 >= E.host_reach(*sc.scans[k][:2]) - 1.0 or E.host_reach(*sc.scans[k][:2]) > 1e9


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle against the reference's own headers on the directed scenarios
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hpo(oracle_lib):
    if not oracle_lib.have_ref_hector():
        pytest.skip("oracle/_ref/libhector_ref.so not built (needs /root/reference)")
    return oracle_lib


def pin(hpo, sc):
    m = sc.map
    ref, port = E.make_oracle(hpo, m, ref=True), E.make_oracle(hpo, m)
    for scan in sc.scans:
        E.oracle_feed(ref, m, scan)
        E.oracle_feed(port, m, scan)
    if m.levels == 1:
        assert np.count_nonzero(ref.logodds()) > 0
        assert ref.logodds().tobytes() == port.logodds().tobytes(), sc.name
        assert np.array_equal(ref.update_index(), port.update_index()), sc.name
        assert np.array_equal(ref.occupancy_i8(), port.occupancy_i8()), sc.name
    else:
        for lv in range(m.levels):
            assert ref.level_info(lv)[:2] == E.level_dims(m)[lv]
            assert np.count_nonzero(ref.logodds(lv)) > 0
            assert ref.logodds(lv).tobytes() == port.logodds(lv).tobytes(), (sc.name, lv)


@pytest.mark.parametrize("name", ["sweep_20", "sweep_rim", "pairs", "triples", "beam_counts_4097", "knife_edge_l0", "knife_edge_l1",
                                  "pyramid_odd"])
def test_oracle_equals_the_reference(hpo, name):
    if name == "sweep_20":
        sc = E.sweep(20)
    elif name == "beam_counts_4097":
        sc = E.beam_counts(tuple(n for n in E.BEAM_COUNTS if n <= 4097))
    else:
        sc = E.scenario(name)
    pin(hpo, sc)


def test_oracle_just_once_equals_the_reference(hpo):
    """the reference's demo variant is fixed to a 1600 x 1600 map, begin (800, 800) and 0.05 m cells"""
    ref, port = hpo.RefHector(1600, 1600, 0.05, (0.0, 0.0)), hpo.PortHector(1600, 1600, 0.05, (0.0, 0.0))
    for pts in E.just_once_points():
        ref.updateByScanJustOnce(pts)
        port.updateByScanJustOnce(pts)
    assert np.count_nonzero(ref.logodds()) > 100
    assert ref.logodds().tobytes() == port.logodds().tobytes()
    assert np.array_equal(ref.update_index(), port.update_index())
