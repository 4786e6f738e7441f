"""The preconditions of tests/test_gn_edges_gpu.py, checked on the CPU restatement of the reference's matcher alone (oracle
PortHector.match_data): every scenario of tests/gn_edge_cases.py really has the points outside the map, the zero Hessian, the
exact boundary values or the clamped step it is named after, and the reference's own result is well-posed there -- so a GPU
test that passes has compared the kernels with something."""
import numpy as np
import pytest

import gn_edge_cases as E

f32 = np.float32
ZERO9 = np.zeros(9, f32).tobytes()


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def converges_and_is_stable(po, cpus, pts, begin, truth):
    p, H = po.PortHector.match_data(cpus, pts, begin)
    assert np.hypot(*(p[:2] - truth[:2])) < E.CONVERGES, (p, truth)
    shift = E.oracle_shift_under_ulps(po, cpus, pts, begin)
    assert shift < E.STABLE, shift
    return p, H


@pytest.mark.parametrize("name", E.GEOMETRY_IDS)
def test_geometry_preconditions(po, name):
    """Per geometry: >= 100 points of the query outside level 0 at the true pose, at least one beyond each side the geometry
    is meant to exercise; every container the GPU test holds to a tolerance converges to within 0.03 m of truth and does
    not move by 1e-5 when the start pose moves by one float32 ulp; the neighbour container lies inside every level."""
    g = E.GEOMETRIES[E.GEOMETRY_IDS.index(name)]
    case = E.geometry_case(name)
    assert len(case.levels) == g.levels
    out = E.outside(case.levels[0], case.off, case.containers["scan"], case.truth)
    assert out["any"].sum() >= 100, int(out["any"].sum())
    for side in g.sides:
        assert out[side].any(), side
    cpus = E.oracle_levels(po, case)
    for i, c in enumerate(cpus):
        assert np.count_nonzero(c.logodds()) > 100, i
    for k in ("scan", "resident", "lds", "mem"):
        pts = case.containers[k]
        assert 700 <= len(case.containers["scan"]) <= 256 * 5  # one scan, and short enough for every register form
        assert E.outside(case.levels[0], case.off, pts, case.truth)["any"].sum() >= 100, k
        converges_and_is_stable(po, cpus, pts, case.begin[k], case.truth)
    assert len(case.containers["lds"]) == E.N_LDS and len(case.containers["mem"]) == E.N_MEM
    near = case.containers["near"]
    assert len(near) >= 64
    for i, lv in enumerate(case.levels):
        assert not E.outside(lv, case.off, near, case.begin["near"], po.PortHector.level_factor(i))["any"].any(), i


def test_all_four_sides_are_left_by_some_geometry():
    assert {s for g in E.GEOMETRIES for s in g.sides} == {"x_lo", "x_hi", "y_lo", "y_hi"}


def test_level_sizes():
    """Odd sizes halve by integer division on every level; five levels of a 400^2 map all exist; the list ends at a
    non-positive size."""
    odd = E.geometry_case("333x201-odd").levels
    assert [(sx, sy) for sx, sy, _ in odd] == [(333, 201), (166, 100), (83, 50)]
    assert [c for _, _, c in odd] == [float(f32(0.05)), float(f32(0.1)), float(f32(0.2))]
    five = E.geometry_case("400x400-5levels").levels
    assert [(sx, sy) for sx, sy, _ in five] == [(400, 400), (200, 200), (100, 100), (50, 50), (25, 25)]
    assert len(E.level_list(5, 3, 4)) == 2  # (5, 3), (2, 1), then sy = 0


def test_zero_hessian_cases(po):
    """Untouched map, and every point outside every level: all nine H words are +0.0, and the pose is NOT the start pose's
    bytes (the float32 round trip through the levels moves it), so `return the input` cannot pass the GPU test."""
    base = E.geometry_case(E.ZERO_GEOMETRY.name)
    built, empty = E.oracle_levels(po, base), E.oracle_levels(po, base, build=False)
    assert not any(c.logodds().any() for c in empty)
    moved = {}
    for k, (is_built, pts, begin) in E.zero_cases().items():
        if is_built:
            for i, lv in enumerate(base.levels):
                assert E.outside(lv, base.off, pts, begin, po.PortHector.level_factor(i))["any"].all(), (k, i)
        p, H = po.PortHector.match_data(built if is_built else empty, pts, begin)
        assert H.tobytes() == ZERO9, (k, H)
        assert p[2] == begin[2]
        moved[k] = p.tobytes() != begin.tobytes()
    assert all(moved.values()), moved
    p, _ = po.PortHector.match_data(empty, *E.zero_cases()["untouched-scan"][1:])
    assert np.allclose(p - E.zero_cases()["untouched-scan"][2], (-2.98e-7, -2.53e-7, 0.0), atol=1e-9)


def test_band_preconditions(po):
    """The 200 x 120 map's border band is written on all four sides; at the start pose the container has points at exactly
    +0.0, -0.0, lim and nextafter(lim, +inf) in x and in y, points within 3 cells on both sides of every edge, at least a
    quarter inside and a quarter outside; H[0,0] and H[1,1] of the oracle are non-zero.  Without the exact points the
    oracle does not move under one-ulp changes of the start pose; WITH them it moves by 20 times the device tolerance when
    the ulp pushes the points at 0.0 out of the map -- which is what lets the GPU test see a form that misplaces them."""
    case, n_exact = E.band_case()
    assert case.levels == [(E.BAND_SX, E.BAND_SY, float(f32(E.CELL)))]
    cpus = E.oracle_levels(po, case)
    lo = cpus[0].logodds()
    for band in (lo[1:4], lo[-4:-1], lo[:, 1:4], lo[:, -4:-1]):
        assert np.count_nonzero(band) > 300
    for k, pts in case.containers.items():
        begin = case.begin[k]
        assert begin.tobytes() == np.array([-0.0, -0.0, 0.0], f32).tobytes()
        cx, cy, lx, ly = E.map_xy(case.levels[0], case.off, pts, begin)
        assert np.array_equal(cx, pts[:, 0]) and np.array_equal(cy, pts[:, 1])  # map coordinates ARE the points
        for v, lim in ((cx, lx), (cy, ly)):
            assert ((v == 0) & ~np.signbit(v)).any() and ((v == 0) & np.signbit(v)).any()
            assert (v == lim).any() and (v == np.nextafter(lim, f32(np.inf))).any()
            for edge in (f32(0.0), lim):
                assert ((v > edge - 3) & (v < edge)).sum() >= 20 and ((v > edge) & (v < edge + 3)).sum() >= 20
        out = E.outside(case.levels[0], case.off, pts, begin)
        assert 4 * out["any"].sum() >= len(pts) and 4 * (~out["any"]).sum() >= len(pts), int(out["any"].sum())
        for side in ("x_lo", "x_hi", "y_lo", "y_hi"):
            assert out[side].sum() >= 10, side
        p, H = po.PortHector.match_data(cpus, pts, begin)
        assert H[0, 0] != 0 and H[1, 1] != 0 and np.isfinite(p).all() and np.isfinite(H).all()
    pts, begin = case.containers["scan"], case.begin["scan"]
    assert E.oracle_shift_under_ulps(po, cpus, pts[n_exact:], begin) < E.STABLE
    assert E.oracle_shift_under_ulps(po, cpus, pts, begin) > 10 * E.POSE_TOL


def test_clamp_is_reached(po):
    """The first Gauss-Newton step on the coarsest level moves the heading by exactly float32(0.2) (one iteration:
    max_iterations = 0 is the reference's `1 + maxIterations` loop run once), the full match still converges to the truth and
    is stable under one-ulp changes of the start pose."""
    case = E.clamp_case()
    cpus = E.oracle_levels(po, case)
    pts, begin = case.containers["scan"], case.begin["scan"]
    top = len(cpus) - 1
    p1, _ = cpus[top].match_level(pts, begin, 0, po.PortHector.level_factor(top))
    assert p1[2] == f32(begin[2] - f32(0.2)), (p1, begin)
    for i, lv in enumerate(case.levels):
        assert not E.outside(lv, case.off, pts, begin, po.PortHector.level_factor(i))["any"].any()
    p, _ = converges_and_is_stable(po, cpus, pts, begin, case.truth)
    assert abs(p[2]) < 1e-3
    # the returned H is summed at the estimate the LAST iteration starts from; no point may sit within 1e-3 cells of a cell
    # border there (the gradient jumps at borders; the device forms are within ~1e-5 cells of the oracle's estimate)
    tmp = begin
    for lv in range(top, 0, -1):
        tmp, _ = cpus[lv].match_level(pts, tmp, 3, po.PortHector.level_factor(lv))
    last, _ = cpus[0].match_level(pts, tmp, 4)
    cx, cy, _, _ = E.map_xy(case.levels[0], case.off, pts, last)
    assert min(np.abs(cx - np.round(cx)).min(), np.abs(cy - np.round(cy)).min()) > 1e-3
