"""CPU side of the correlation-grid scenarios (tests/corrgrid_cases.py): every scenario is what it claims to be, and three
statements of the operation agree on it -- the literal Python walk + numpy smear of the scenario library, the plain-C oracle
(PortKarto) and, where oracle/_ref is built, the reference's own ScanMatcher (RefKarto).  The margins that keep a scenario
from resting on the last bit of a sine are conditions on the INPUTS and are asserted here, so the GPU test
(tests/test_corrgrid_edges_gpu.py) can compare bit for bit."""
import functools
import math

import numpy as np
import pytest

import corrgrid_cases as cc

SCENARIOS = cc.all_scenarios()
IDS = [s.name for s in SCENARIOS]


def oracle_cfg(oracle_lib, cfg):
    return oracle_lib.default_cfg(search_size=cfg.search, resolution=cfg.resolution, smear_deviation=cfg.smear)


@functools.lru_cache(maxsize=None)
def _port(oracle_lib, cfg, laser):
    return oracle_lib.PortKarto(oracle_cfg(oracle_lib, cfg), oracle_lib.laser_struct(laser, cfg.threshold))


@functools.lru_cache(maxsize=None)
def _ref(oracle_lib, cfg, laser):
    return oracle_lib.RefKarto(oracle_cfg(oracle_lib, cfg), oracle_lib.laser_struct(laser, cfg.threshold))


def same_points(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def walks_of(port, sc, mutate=None):
    pts = [port.point_readings(sc.ranges[b], sc.poses[b]) for b in range(len(sc.poses))]
    return pts, [cc.find_valid_walk(p, sc.center[:2], mutate) for p in pts]


@pytest.mark.parametrize("cfg", list(cc.CONFIGS.values()), ids=list(cc.CONFIGS))
def test_configurations_select_the_forms(oracle_lib, cfg):
    """kernel size, off-centre 100s, strides: the table the scenarios are built on"""
    port = _port(oracle_lib, cfg, cc.POINT_LASER)
    gi, g = port.grid_info(), cc.geometry(cfg)
    assert gi["kernel_size"] == cfg.kernel
    for key, mine in (("width", "width"), ("height", "height"), ("stride", "stride"), ("roi_w", "roi"), ("roi_x", "border")):
        assert gi[key] == g[mine], key
    k = port.kernel()
    assert np.array_equal(k, cc.smear_kernel(cfg))
    hk = cfg.kernel // 2
    assert k[hk, hk] == 100 and int((k == 100).sum()) - 1 == cfg.off100
    if cfg.off100:
        assert k[hk, hk + 1] == k[hk, hk - 1] == k[hk + 1, hk] == k[hk - 1, hk] == 100
    if cfg.name in cc.EXPECTED_STRIDES:
        roi, stride = cc.EXPECTED_STRIDES[cfg.name]
        assert (gi["roi_w"], gi["stride"]) == (roi, stride)
        assert stride % 16 == (stride * gi["height"]) % 16 == (0 if stride == 176 else 8)
    if oracle_lib.have_ref():
        ref = _ref(oracle_lib, cfg, cc.POINT_LASER)
        assert np.array_equal(ref.kernel(), k) and ref.grid_info()["stride"] == gi["stride"]


def test_beam_counts_and_routes_are_all_there():
    assert sorted(s.laser.n_ranges for s in SCENARIOS if s.family == "beam_counts") == sorted(cc.BEAM_COUNTS)
    assert {s.route for s in SCENARIOS} == {"gather", "listed", "serial"}
    assert {s.cfg.name for s in SCENARIOS if s.family == "rims"} == set(cc.CONFIGS)
    assert cc.by_name("beam_counts/n2047").route == "gather" and cc.by_name("beam_counts/n2048").route == "listed"


@pytest.mark.parametrize("sc", SCENARIOS, ids=IDS)
def test_three_statements_agree(oracle_lib, sc):
    port = _port(oracle_lib, sc.cfg, sc.laser)
    assert port.num_beams == sc.laser.n_ranges
    pts, walks = walks_of(port, sc)
    for b, (p, w) in enumerate(zip(pts, walks)):
        assert same_points(port.find_valid_points(p, sc.center[:2]), p[w["valid"]]), b
    port.set_base_scans(sc.ranges, sc.poses, sc.center)
    mine = cc.smear_grid(sc.cfg, sc.center, [p[w["valid"]] for p, w in zip(pts, walks)], kernel=port.kernel())
    assert np.array_equal(port.grid(), mine)
    assert np.array_equal(port.grid_info()["offset"], np.array(cc.grid_offset(sc.cfg, sc.center)))
    if oracle_lib.have_ref():
        ref = _ref(oracle_lib, sc.cfg, sc.laser)
        for b, (p, w) in enumerate(zip(pts, walks)):
            assert same_points(ref.point_readings(sc.ranges[b], sc.poses[b]), p), b
            assert same_points(ref.find_valid_points(sc.ranges[b], sc.poses[b], sc.center[:2]), p[w["valid"]]), b
        ref.set_base_scans(sc.ranges, sc.poses, sc.center)
        assert np.array_equal(ref.grid(), mine)


@pytest.mark.parametrize("sc", SCENARIOS, ids=IDS)
def test_margins(oracle_lib, sc):
    """No scenario rests on the last bit of a sine: d^2 off the threshold, ss off zero, cell coordinates off the
    half-integers, infinite points off the quadrant boundaries.  Exempt: the values that are exact by construction."""
    port = _port(oracle_lib, sc.cfg, sc.laser)
    pts, walks = walks_of(port, sc)
    ox, oy = cc.grid_offset(sc.cfg, sc.center)
    scale = cc.geometry(sc.cfg)["scale"]
    for b, (p, w) in enumerate(zip(pts, walks)):
        d2 = w["d2"][np.isfinite(w["d2"])]
        near = np.abs(d2 - 0.1 * 0.1) <= cc.D2_MARGIN
        ss = w["ss"][np.isfinite(w["ss"])]
        zero = np.abs(ss) <= cc.SS_MARGIN
        if sc.exact:
            assert (d2[near] == 0.1 * 0.1).all() and int(near.sum()) == sc.claims.get("d2_tie", 0)
            assert (ss[zero] == 0.0).all() and int(zero.sum()) == (1 if "ss_zero_at" in sc.claims else 0)
        else:
            assert not near.any() and not zero.any(), (b, d2[near], ss[zero])
        r = sc.ranges[b]
        ang = cc.beam_angles(sc.laser, float(sc.poses[b][2]))
        for i in np.flatnonzero(np.isinf(r)):
            assert abs(math.cos(ang[i])) > 1e-6 and abs(math.sin(ang[i])) > 1e-6
        for i in w["valid"]:
            if sc.exact and (i == 0 or r[i] == 0.0):
                continue
            for t in (cc.cell_coordinate(p[i][0], ox, scale), cc.cell_coordinate(p[i][1], oy, scale)):
                if math.isfinite(t):
                    assert abs(abs(t - math.floor(t)) - 0.5) > cc.CELL_MARGIN, (b, i, t)


@pytest.mark.parametrize("sc", SCENARIOS, ids=IDS)
def test_claims(oracle_lib, sc):
    port = _port(oracle_lib, sc.cfg, sc.laser)
    pts, walks = walks_of(port, sc)
    w, p, c = walks[0], pts[0], sc.claims
    g = cc.geometry(sc.cfg)
    port.set_base_scans(sc.ranges, sc.poses, sc.center)
    grid = port.grid()
    roi_view = grid[g["border"]:g["border"] + g["roi"], g["border"]:g["border"] + g["roi"]]
    n = sc.laser.n_ranges
    if "anchors" in c:
        assert w["anchors"] == c["anchors"]  # the successor offset / the chain length
    if "valid" in c:
        assert w["valid"] == c["valid"]
    if "chain_between" in c:
        assert c["chain_between"][0] <= len(w["anchors"]) <= c["chain_between"][1]
    if c.get("kept") == "all":
        assert len(w["runs"]) >= 3 and all(k for _, _, k in w["runs"])
    if c.get("kept") == "none":
        assert len(w["runs"]) >= 3 and not any(k for _, _, k in w["runs"]) and not grid.any()
    if "kept_scans" in c:
        for wb, kept in zip(walks, c["kept_scans"]):
            assert len(wb["runs"]) >= 3 and all(k == kept for _, _, k in wb["runs"])
    if "alternations" in c:
        flags = [k for _, _, k in w["runs"]]
        assert sum(a != b for a, b in zip(flags, flags[1:])) >= c["alternations"]
    if "first_run_kept" in c:
        assert w["runs"][0][2] == c["first_run_kept"] and w["runs"][0][0] == 0
    if "first_valid" in c:
        assert w["anchors"][0] == c["first_valid"]
    if "valid_starts_at" in c:
        assert w["valid"][0] == c["valid_starts_at"]  # the very first run starts at index 0, whatever lies there
    if "nan_in_valid" in c:
        has = bool(np.isnan(p[w["valid"]]).any())
        assert has == c["nan_in_valid"]
        if has:  # host: (int) of NaN is INT_MIN, the point fails IsUpTo -- ROI cell (0, 0) and its footprint stay zero
            hk = g["hk"]
            assert not grid[:g["border"] + hk + 1, :g["border"] + hk + 1].any()
            assert grid.any()
    if c.get("inf_in_valid"):
        assert np.isinf(p[w["valid"]]).any()
    if "inf_classes" in c:
        inf = p[np.isinf(p).any(axis=1)]
        assert len({(np.sign(x), np.sign(y)) for x, y in inf}) >= c["inf_classes"]
    if "ss_zero_at" in c:
        assert w["ss"][c["ss_zero_at"]] == 0.0 and tuple(p[0]) == tuple(sc.poses[0][:2]) == tuple(sc.center[:2])
    if "last_valid_before" in c:
        assert max(w["valid"]) < c["last_valid_before"] <= w["anchors"][-1]
    if "d2_tie" in c:
        assert int((w["d2"] == 0.1 * 0.1).sum()) == c["d2_tie"]
    if "cells" in c:
        ys, xs = np.nonzero(roi_view == 100)
        assert sorted(zip(xs.tolist(), ys.tolist())) == [tuple(x) for x in c["cells"]] or sc.cfg.off100
        for kx, ky in c["cells"]:
            assert roi_view[ky, kx] == 100
        assert len(c["cells"]) >= 4
    if "last_chunk" in c:
        kx, ky = c["last_chunk"]
        assert (kx, ky) in c["cells"] and cc.flat_index(sc.cfg, kx, ky) == max(cc.flat_index(sc.cfg, x, y) for x, y in c["cells"])
        assert cc.flat_index(sc.cfg, kx, ky) + (g["hk"] + 2) * g["stride"] >= g["data_size"]  # its footprint ends in the last rows
    if sc.family == "rims":
        assert sum(1 for wb in walks if wb["valid"] == [0]) == len(walks)  # outside cells: a valid point and no cell
        if not sc.cfg.off100:
            assert int((roi_view == 100).sum()) == len(c["cells"]) < len(walks)
        phases = {cc.flat_index(sc.cfg, kx, ky) % 16 for kx, ky in c["cells"]}
        assert {0, 15} <= phases
    if "cell_x" in c:
        ox, _ = cc.grid_offset(sc.cfg, sc.center)
        t = cc.cell_coordinate(p[0][0], ox, g["scale"])
        assert p[0][0] == sc.ranges[0][0] and p[0][1] == 0.0  # beam 0 at angle 0 from the origin: exact
        assert (2.0 * t == math.floor(2.0 * t) and math.floor(2.0 * t) % 2 == 1) == c["tie"] and cc.kround(t) == c["cell_x"]
        ys, xs = np.nonzero(roi_view == 100)
        assert xs.tolist() == ([c["cell_x"]] if 0 <= c["cell_x"] < g["roi"] else [])
    if "same_cell" in c:
        ox, oy = cc.grid_offset(sc.cfg, sc.center)
        cells = {(cc.world_to_cell(p[i][0], ox, g["scale"]), cc.world_to_cell(p[i][1], oy, g["scale"])) for i in c["same_cell"]}
        assert len(cells) == 1 and set(c["same_cell"]) <= set(w["valid"])
    if "order_pair" in c:
        other = cc.by_name(c["order_pair"])
        port.set_base_scans(other.ranges, other.poses, other.center)
        assert grid.any() and not np.array_equal(port.grid(), grid)
    if "kernel" in c:
        assert port.grid_info()["kernel_size"] == c["kernel"] and grid.any()


MUTATIONS = ("first_run", ">=", "ss<=0", "last_run", "nan_cell0")


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_each_mistake_changes_an_answer(oracle_lib, mutation):
    """The walk with one mistake at a time -- first run started at the first valid point, >= at the threshold, ss <= 0
    dropped, the last run kept, a NaN point setting cell 0 -- must differ from the true walk on at least one scenario."""
    caught = []
    for sc in SCENARIOS:
        if sc.laser.n_ranges > 300:
            continue
        port = _port(oracle_lib, sc.cfg, sc.laser)
        pts, good = walks_of(port, sc)
        if mutation == "nan_cell0":
            lists = [p[w["valid"]] for p, w in zip(pts, good)]
            if not np.array_equal(cc.smear_grid(sc.cfg, sc.center, lists), cc.smear_grid(sc.cfg, sc.center, lists, nan_sets_cell0=True)):
                caught.append(sc.name)
        else:
            _, bad = walks_of(port, sc, mutation)
            if any(a["valid"] != b["valid"] for a, b in zip(good, bad)):
                caught.append(sc.name)
    assert caught, mutation
    print(mutation, "caught by", len(caught), "scenarios, e.g.", caught[:4])


def test_epoch_sequence_shows_a_missing_reset(oracle_lib):
    """The 258-rebuild sequence of the epoch-wrap test on a model of the mark plane: with the reset at the wrap every rebuild
    sees its own window's cells; without it the cells of C1 and C2, tagged once with the epochs 1 and 2, come back at the
    rebuilds 257 and 258 -- so the device test's grids there tell the two apart.  (A and B alone could not: they re-tag
    their own cells at every rebuild, and no byte of the plane still holds 1 or 2 when the epoch wraps.)"""
    laser, cfg, windows, center = cc.epoch_windows()
    port = _port(oracle_lib, cfg, laser)
    centres = {}
    for key, (r, p) in windows.items():
        port.set_base_scans(r, p, center)
        ys, xs = np.nonzero(port.grid() == 100)
        centres[key] = set(zip(xs.tolist(), ys.tolist()))
    c1, c2 = centres["A+C1"] - centres["A"], centres["B+C2"] - centres["B"]
    assert centres["A"] and centres["B"] and c1 and c2 and not centres["empty"]
    assert centres["A"] <= centres["A+C1"] and centres["B"] <= centres["B+C2"]
    for x, y in ((centres["A"], centres["B"]), (c1, centres["A"] | centres["B"]), (c2, centres["A"] | centres["B"] | c1)):
        assert all(abs(ax - bx) > 2 or abs(ay - by) > 2 for ax, ay in x for bx, by in y)  # footprints disjoint at 3 x 3
    seq = cc.epoch_sequence()
    assert len(seq) == 258 and dict(seq)[1] == "A+C1" and dict(seq)[256] == "B" and dict(seq)[100] == "empty"
    good = cc.mark_plane_model(centres, seq)
    assert all(good[i] == centres[key] for i, key in seq)
    bad = cc.mark_plane_model(centres, seq, reset=False)
    assert all(bad[i] == centres[key] for i, key in seq if i <= 256)
    assert bad[257] == centres["B"] | c1 and bad[258] == centres["A"] | c2
    assert {257, 258} <= set(cc.EPOCH_CHECKS)
