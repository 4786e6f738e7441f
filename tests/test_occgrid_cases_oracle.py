"""The preconditions of tests/test_occgrid_edges_gpu.py, checked without a GPU: for every scenario of tests/occgrid_cases.py the
plain-C oracle (PortKarto.occgrid_partial / occgrid_bounds / occgrid_from_scans) equals the stepped TraceLine written down in
occgrid_cases.trace_line_counters word for word, no rounded coordinate lies within 1e-6 cells of a tie (except where the
scenario is about exact ties), and the scenario really holds the rays, clippings, beam classes and degenerate sizes it is
named after -- so a GPU test that passes has compared the kernels with something.  The whole builds are also held to the
reference's own compiled OccupancyGrid::CreateFromScans where that is built."""
import pathlib
import re

import numpy as np
import pytest

import occgrid_cases as E


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def port_of(po, sc):
    return po.PortKarto(po.default_cfg(), po.laser_struct(sc.laser, sc.threshold))


def oracle_counters(po, sc):
    """-> (dims, counters, box) of the scenario on the plain-C oracle; a whole build goes through occgrid_bounds' box."""
    port = port_of(po, sc)
    box = sc.box if sc.box is not None else port.occgrid_bounds(sc.ranges, sc.poses)
    d, cnt = port.occgrid_partial(sc.ranges, sc.poses, sc.resolution, box)
    return d, cnt, box


@pytest.mark.parametrize("name", E.COUNTER_NAMES)
def test_oracle_equals_the_stepped_trace_line(po, name):
    sc = E.scenario(name)
    assert E.num_beams(sc.laser) == sc.laser.n_ranges == port_of(po, sc).num_beams <= sc.ranges.shape[1]
    assert E.tie_margin(sc) >= sc.min_margin
    d, cnt, box = oracle_counters(po, sc)
    ed, ecnt = E.trace_line_counters(sc)
    assert np.array_equal(d, ed), (d, ed)
    assert cnt.shape == ecnt.shape and np.array_equal(cnt, ecnt)
    if sc.box is None:
        assert np.array_equal(box, E.scan_bounds(sc))
        exp, off = port_of(po, sc).occgrid_from_scans(sc.ranges, sc.poses, sc.resolution)
        assert exp.shape == (d[1], d[0]) and np.array_equal(off, box[:2])
        assert np.array_equal(exp, port_of(po, sc).occgrid_update(d, cnt))


def test_the_lockstep_form_equals_the_ray_by_ray_form():
    """trace_line_counters steps all rays together; one sweep (every octant, lengths 0..70) and the clipped one with negative
    starts are also traced one ray and one cell at a time."""
    for name in (E.SWEEP_CENTRE, "sweep_clipped[outside]", "exact_ties", "range_classes"):
        sc = E.scenario(name)
        d, cnt = E.trace_line_counters(sc)
        sd, scnt = E.trace_line_counters_scalar(sc)
        assert np.array_equal(d, sd) and np.array_equal(cnt, scnt), name


def test_k_tol_is_the_oracles(po):
    text = (pathlib.Path(po.__file__).resolve().parent / "karto_oracle.c").read_text()
    assert float(re.search(r"#define KT_TOLERANCE (\S+)", text).group(1)) == E.k_tol() == 1e-6


def ends_on_intended_cells(sc):
    s, i, x0, y0, x1, y1, _ = E.ray_cells(sc)
    start, end = sc.intent
    assert np.array_equal(np.stack([x0, y0], 1), start[s]) and np.array_equal(np.stack([x1, y1], 1), end[s])
    return s, x0, y0, x1, y1


@pytest.mark.parametrize("name", [n for n in E.NAMES if n.startswith("sweep_centre")])
def test_sweep_centre_preconditions(po, name):
    sc = E.scenario(name)
    d, cnt, _ = oracle_counters(po, sc)
    assert d.tolist() == [161, 161, 168]
    s, x0, y0, x1, y1 = ends_on_intended_cells(sc)
    n = (2 * E.SWEEP + 1) ** 2
    assert len(sc.ranges) == n == 19881 and len(s) == n - 1            # the zero range is there, and is not traced
    assert (sc.ranges == 0.0).sum() == 1
    dx, dy = x1 - x0, y1 - y0
    octants = {(int(a > 0) - int(a < 0), int(b > 0) - int(b < 0), abs(b) > abs(a)) for a, b in zip(dx.tolist(), dy.tolist())}
    assert len(octants) == 12                                           # the 8 octants and the 4 half-axes
    assert ((dx == 0) | (dy == 0)).sum() == 4 * E.SWEEP and (np.abs(dx) == np.abs(dy)).sum() == 4 * E.SWEEP
    assert set(np.maximum(np.abs(dx), np.abs(dy)).tolist()) == set(range(1, E.SWEEP + 1)) and E.SWEEP > 65
    assert min(x0.min(), y0.min(), x1.min(), y1.min()) >= 0 and max(x1.max(), y1.max()) <= 160   # nothing is clipped
    cx, cy = sc.intent[0][0]
    assert cnt[0, cx + cy * 168] == n - 1 == 19880                      # thousands of increments on the sensor's cell
    assert cnt[1].sum() == n - 1
    if name == E.SWEEP_CENTRE:
        assert cnt[0].sum() == 974120


@pytest.mark.parametrize("name", [n for n in E.NAMES if n.startswith("sweep_clipped")])
def test_sweep_clipped_preconditions(po, name):
    sc = E.scenario(name)
    key = name[len("sweep_clipped["):-1]
    (bx, by), w, h = E.CLIP_BOXES[key]
    d, cnt, _ = oracle_counters(po, sc)
    assert d.tolist() == [w, h, (w + 7) & ~7] and w % 8 == {"outside": 1, "first-cell": 5, "last-cell": 7}[key]
    s, x0, y0, x1, y1 = ends_on_intended_cells(sc)
    inside = (x1 >= 0) & (x1 < w) & (y1 >= 0) & (y1 < h)
    assert 100 < inside.sum() < len(s) - 100                           # end points really are dropped
    assert cnt[1].sum() == inside.sum()                                 # and those outside add no hit
    assert (x1 < 0).any() and (x1 >= w).any() and (y1 < 0).any() and (y1 >= h).any()
    sensor = (int(x0[0]), int(y0[0]))
    assert sensor == {"outside": (-13, 20), "first-cell": (0, 0), "last-cell": (w - 1, h - 1)}[key]
    if key == "outside":
        # rays that start outside and end inside, rays that cross the whole box, rays that never touch it
        assert (inside.sum() > 100) and ((x1 >= w) & (y1 >= 0) & (y1 < h)).any() and (x1 < 0).any()
        assert cnt[0].sum() > cnt[1].sum() > 0


@pytest.mark.parametrize("name", ["long_thin[x]", "long_thin[y]"])
def test_long_thin_preconditions(po, name):
    sc = E.scenario(name)
    d, cnt, _ = oracle_counters(po, sc)
    assert d.tolist() == ([2100, 40, 2104] if name == "long_thin[x]" else [40, 2100, 40])
    s, x0, y0, x1, y1 = ends_on_intended_cells(sc)
    along, across = (x1 - x0, y1 - y0) if name == "long_thin[x]" else (y1 - y0, x1 - x0)
    assert np.abs(along).min() == 1990 and np.abs(along).max() == 2000 and (along > 0).any() and (along < 0).any()
    assert set(across.tolist()) == set(range(-15, 16))
    assert 2 * 2000 * 15 > 2 ** 15 and 2000 // 64 >= 31
    assert cnt[1].sum() == len(s) == 2 * 11 * 31                       # every ray stays inside


def test_beam_counts_preconditions():
    for n in E.BEAM_COUNTS:
        sc = E.scenario(f"beam_counts[{n}]")
        S = len(sc.ranges)
        assert sc.ranges.shape == (S, n) and (n % 4 == 0 or (S * n) % 4 != 0) and S >= 3
        w, h, stride = E.geometry(sc)[:3]
        assert (w, h, stride) == (203, 197, 208)
        _, _, x0, y0, x1, y1, valid = E.ray_cells(sc)
        assert len(x0) == S * n and valid.all()
        assert min(x0.min(), x1.min(), y0.min(), y1.min()) >= 0 and max(x0.max(), x1.max()) < w and max(y0.max(), y1.max()) < h
    assert {n % 256 for n in E.BEAM_COUNTS} >= {0, 1, 255} and {n % 64 for n in E.BEAM_COUNTS} >= {0, 1, 63}


def test_surplus_columns_would_change_the_result(po):
    sc = E.scenario("beam_counts[1000of1081]")
    assert sc.ranges.shape == (3, 1081) and sc.laser.n_ranges == 1000
    _, cnt, _ = oracle_counters(po, sc)
    packed = sc._replace(ranges=np.ascontiguousarray(sc.ranges.reshape(-1)[:3000].reshape(3, 1000)))  # pitch taken for 1000
    _, wrong, _ = oracle_counters(po, packed)
    assert not np.array_equal(cnt, wrong)
    _, right, _ = oracle_counters(po, sc._replace(ranges=np.ascontiguousarray(sc.ranges[:, :1000])))
    assert np.array_equal(cnt, right)


def test_range_classes_preconditions(po):
    sc = E.scenario("range_classes")
    in_box, traced, valid, shortened = E.beam_classes(sc)
    assert np.array_equal(sc.ranges[1], sc.ranges[0][::-1], equal_nan=True)
    for row in range(2):
        skipped = ~traced[row] & ~in_box[row]
        box_only = ~traced[row] & in_box[row]
        with_hit = traced[row] & valid[row]
        without_hit = traced[row] & ~valid[row] & ~shortened[row]
        short = shortened[row]
        counts = [int(m.sum()) for m in (skipped, box_only, with_hit, without_hit, short)]
        # NaN, +-inf, -1, -0, 0, below min, at and above max | min itself | above min, below thr - tol | thr - tol, its upper
        # neighbour, below thr | thr, above thr, below max
        assert counts == [9, 1, 2, 3, 3], counts
        r = sc.ranges[row]
        assert r[box_only][0] == sc.laser.range_min
        assert sorted(r[without_hit].tolist()) == [20.0 - E.k_tol(), np.nextafter(20.0 - E.k_tol(), np.inf), np.nextafter(20.0, 0.0)]
        assert sorted(r[short].tolist()) == [20.0, np.nextafter(20.0, np.inf), np.nextafter(60.0, 0.0)]
    d, cnt, _ = oracle_counters(po, sc)
    assert cnt[1].sum() == 4                                            # two hits per scan, every traced end is in the box
    _, _, x0, y0, x1, y1, _ = E.ray_cells(sc)
    assert min(x1.min(), y1.min()) >= 0 and x1.max() < d[0] and y1.max() < d[1] and np.abs(x1 - x0).max() >= 399


def test_box_extremum_preconditions(po):
    sc = E.scenario("box_extremum")
    port = port_of(po, sc)
    assert sc.ranges.shape == (12, 1081) and (np.isfinite(sc.ranges).sum(axis=1) == 1).all()
    assert [int(np.nonzero(np.isfinite(r))[0][0]) for r in sc.ranges[:8]] == E.EXTREMUM_BEAMS
    for rows in sc.groups:
        assert np.array_equal(port.occgrid_bounds(sc.ranges[rows], sc.poses[rows]), E.scan_bounds(sc, rows)), rows
    raw, _ = E._points(sc)
    ends = raw[np.isfinite(sc.ranges)]                                 # [12, 2]: the one end point of each scan
    joint = E.scan_bounds(sc, range(8, 12))
    who = [int(np.argmin(ends[8:, 0])), int(np.argmin(ends[8:, 1])), int(np.argmax(ends[8:, 0])), int(np.argmax(ends[8:, 1]))]
    assert who == [0, 1, 2, 3]                                          # four scans hold the four extremes ...
    assert joint.tolist() == [ends[8, 0], ends[9, 1], ends[10, 0], ends[11, 1]]
    beams = [int(np.nonzero(np.isfinite(r))[0][0]) for r in sc.ranges[8:]]
    assert len({b // 256 for b in beams}) == 4                          # ... from four blocks of k_occ_points
    for k in range(8):                                                  # alone, each box is the sensor and the one point
        b = E.scan_bounds(sc, [k])
        assert b.tolist() == [min(sc.poses[k, 0], ends[k, 0]), min(sc.poses[k, 1], ends[k, 1]),
                              max(sc.poses[k, 0], ends[k, 0]), max(sc.poses[k, 1], ends[k, 1])]


def test_exact_ties_preconditions(po):
    sc = E.scenario("exact_ties")
    assert E.tie_margin(sc) == 0.0
    sensors, ends = E._grid_coords(sc)
    both = np.concatenate([sensors.ravel(), ends.ravel()])
    assert np.array_equal(both * 2, np.round(both * 2)) and (np.abs(both * 2) % 2 == 1).all()   # every one an exact x.5
    assert {-1.5, -0.5, 0.5, 1.5, E.TIE_W - 0.5} <= set(ends[:, 0, 0].tolist()) | set(sensors[:, 0].tolist())
    assert {-1.5, -0.5, 0.5, 1.5, E.TIE_H - 0.5} <= set(sensors[:, 1].tolist())
    d, cnt, _ = oracle_counters(po, sc)
    assert d.tolist() == [E.TIE_W, E.TIE_H, 16]
    _, _, x0, y0, x1, y1, _ = E.ray_cells(sc)
    # away from zero: -0.5 -> -1 leaves the grid on the near side, w - 0.5 -> w on the far side, 0.5 -> 1 skips cell 0
    assert set(x0.tolist()) == {-2, -1, 1, 2} and E.TIE_W in x1.tolist() and -1 in x1.tolist() and 0 not in x1.tolist()
    assert set(y0.tolist()) == {-2, -1, 1, 2, E.TIE_H - 1, E.TIE_H}
    assert not cnt[0].reshape(E.TIE_H, 16)[0].any() and cnt[0].reshape(E.TIE_H, 16)[1].any()


def test_degenerate_preconditions(po):
    for name, dims in (("degenerate[0x0]", (0, 0)), ("degenerate[wx0]", (52, 0))):
        sc = E.scenario(name)
        assert sc.box is None and name in E.WHOLE_BUILDS
        exp, off = port_of(po, sc).occgrid_from_scans(sc.ranges, sc.poses, sc.resolution)
        assert exp.shape == dims[::-1]
        d, cnt, _ = oracle_counters(po, sc)
        assert tuple(d[:2]) == dims and cnt.shape == (2, 0)
    in_box, traced, _, _ = E.beam_classes(E.scenario("degenerate[0x0]"))
    assert not in_box.any() and not traced.any()
    assert E.beam_classes(E.scenario("degenerate[wx0]"))[1].all()
    sc = E.scenario("degenerate[same-cell]")
    ends_on_intended_cells(sc)
    d, cnt, _ = oracle_counters(po, sc)
    assert d.tolist() == [5, 3, 8] and cnt.sum() == 3 and cnt[0, 2 + 8] == 2 and cnt[1, 2 + 8] == 1


# ---- the reference's own compiled code on the whole builds ----
@pytest.fixture(scope="module")
def ref_po(oracle_lib):
    if not oracle_lib.have_ref():
        pytest.skip("oracle/_ref/libkarto_ref.so not built (needs the reference tree)")
    return oracle_lib


@pytest.mark.parametrize("name", E.WHOLE_BUILDS + [E.SWEEP_CENTRE + "/whole"])
def test_whole_builds_equal_the_reference(ref_po, name):
    """OccupancyGrid::CreateFromScans of the reference itself (robot pose = sensor pose, no laser offset) classifies every
    cell as the oracle does, on a grid of the same size and offset."""
    po = ref_po
    sc = E.as_whole_build(E.scenario(name[:-len("/whole")])) if name.endswith("/whole") else E.scenario(name)
    c, l = po.default_cfg(), po.laser_struct(sc.laser, sc.threshold)
    a, oa = po.RefKarto(c, l).occgrid_from_scans(sc.ranges, sc.poses, sc.resolution)
    b, ob = po.PortKarto(c, l).occgrid_from_scans(sc.ranges, sc.poses, sc.resolution)
    assert a is not None and a.shape == b.shape and np.array_equal(oa, ob)
    assert np.array_equal(a, b)
    if name.endswith("/whole"):
        assert a.shape == (2 * E.SWEEP, 2 * E.SWEEP) and (a == 100).sum() > 1000 and (a == 255).sum() > 1000
        d, cnt = E.trace_line_counters(sc)
        assert np.array_equal(b, po.PortKarto(c, l).occgrid_update(d, cnt))
