"""lesson4 GMapping count map, CPU side: the restatement (tests/gmapping_restatement.py) equals the fixture recorded from the
reference's own map classes (tests/golden/gmapping_golden.npz); where the reference and g++ are present, the live driver
equals the restatement too (gridLine exhaustively for offsets up to 40 cells); the C ABI exports the new entry points."""
import ctypes
import pathlib
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE / "golden"))

import gmapping_restatement as gr  # noqa: E402

GOLDEN = HERE / "golden" / "gmapping_golden.npz"
REFERENCE = pathlib.Path("/root/reference")
NODE_GEO = gr.Geometry(-40.0, -40.0, 40.0, 40.0, 0.05)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _same_counters(st: gr.MapState, d, prefix: str):
    v, n, ax, ay = gr.unpack_counters(d, prefix, st.visits.shape)
    assert np.array_equal(st.visits, v)
    assert np.array_equal(st.n, n)
    assert np.array_equal(st.acc_x.view(np.uint32), ax.view(np.uint32))
    assert np.array_equal(st.acc_y.view(np.uint32), ay.view(np.uint32))


def test_geometry_of_the_node_box(golden):
    sx, sy, w, h, x2, y2, px, py = golden["node_hdr"]
    assert (NODE_GEO.size_x, NODE_GEO.size_y, NODE_GEO.width, NODE_GEO.height) == (sx, sy, w, h) == (1600, 1600, 1600, 1600)
    assert (NODE_GEO.size_x2, NODE_GEO.size_y2, NODE_GEO.patches_x, NODE_GEO.patches_y) == (x2, y2, px, py) == (800, 800, 50, 50)
    pad = gr.Geometry(-40.0, -40.0, 41.0, 41.0, 0.05)
    assert (pad.size_x, pad.width, pad.size_x2) == tuple(golden["pad_hdr"][[0, 2, 4]]) == (1600, 1620, 810)


def test_angle_cache_equals_golden(golden):
    am, ai = golden["node_angle"]
    c, s = gr.angle_cache(len(golden["node_ranges"]), am, ai)
    assert c.tobytes() == golden["node_cos"].tobytes() and s.tobytes() == golden["node_sin"].tobytes()


def test_node_callback_equals_golden(golden):
    am, ai = golden["node_angle"]
    st, pub = gr.node_callback(golden["node_ranges"], am, ai)
    _same_counters(st, golden, "node_")
    assert np.array_equal(st.mask, golden["node_mask"])
    assert np.array_equal(pub, golden["node_data"])
    # NaN, +-inf, 0, 35 and 29.995 (> maxRange as float32) are skipped; 25, 25.0001, 27 and 29.98 are lines without a hit
    assert st.stats[1] == 1081 - 6 and st.stats[2] == st.stats[1] - 4
    assert golden["ref_cpu_callback_s"].shape == (2,) and golden["ref_cpu_callback_s"][0] > 0


def test_padded_box_equals_golden(golden):
    am, ai = golden["node_angle"]
    st, pub = gr.node_callback(golden["node_ranges"], am, ai, dict(xmax=41.0, ymax=41.0))
    _same_counters(st, golden, "pad_")
    assert pub.shape == (1620, 1620) and np.array_equal(pub, golden["pad_data"])
    assert (pub[:, 1600:] == 0).all() and (pub[1600:, :] == 0).all()


@pytest.mark.parametrize("case", ["acc", "multi"])
def test_accumulation_equals_golden(golden, case):
    ang = golden["node_angle"] if case == "acc" else golden["multi_angle"]
    r = golden[case + "_ranges"]
    st = gr.MapState(NODE_GEO)
    c, s = gr.angle_cache(r.shape[1], *ang)
    st.integrate(r, golden[case + "_poses"], c, s, 30 - 0.01, 25.0)
    _same_counters(st, golden, case + "_")
    assert np.array_equal(st.mask, golden[case + "_mask"])
    if case == "multi":
        assert st.n.max() == r.size  # every crafted hit in one cell


def test_grid_line_equals_golden(golden):
    pairs, cnt, pts = golden["line_pairs"], golden["line_counts"], golden["line_points"]
    off = np.concatenate([[0], np.cumsum(cnt)])
    for i, p in enumerate(pairs.tolist()):
        assert np.array_equal(np.array(gr.grid_line(tuple(p[:2]), tuple(p[2:]))), pts[off[i]:off[i + 1]]), p
    _, x, y, last = gr.line_cells_closed(pairs[:, 0], pairs[:, 1], pairs[:, 2], pairs[:, 3])
    assert np.array_equal(np.stack([x, y], 1), pts)
    assert last.sum() == len(pairs)


def test_closed_form_equals_stepped_sweep():
    """The device's closed-form line (line_cells_closed mirrors it) against the stepped gridLine, every offset to 40."""
    d = np.arange(-40, 41)
    dx, dy = np.meshgrid(d, d)
    for x0, y0 in [(0, 0), (7, -3), (-13, 22)]:
        p1x, p1y = x0 + dx.ravel(), y0 + dy.ravel()
        _, x, y, _ = gr.line_cells_closed(np.full(p1x.size, x0), np.full(p1x.size, y0), p1x, p1y)
        ref = np.concatenate([np.array(gr.grid_line((x0, y0), (a, b))) for a, b in zip(p1x.tolist(), p1y.tolist())])
        assert np.array_equal(np.stack([x, y], 1), ref)


def test_c_round_is_half_away_from_zero():
    v = np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999999999999994, -2.4999999999999996])
    assert gr.c_round(v).tolist() == [1.0, -1.0, 2.0, -2.0, 3.0, 0.0, -2.0]


# ---- the live reference (where it exists) ---------------------------------------------------------------------------------
def _live_driver(tmp_path):
    if not (REFERENCE / "lesson4" / "include" / "lesson4" / "gmapping" / "grid" / "map.h").exists() or not shutil.which("g++"):
        pytest.skip("the reference's lesson4 headers or g++ are not on this machine")
    import make_gmapping_golden as mk

    return mk, mk.build_driver(REFERENCE, tmp_path)


def test_live_driver_grid_line_sweep(tmp_path):
    mk, exe = _live_driver(tmp_path)
    d = np.arange(-40, 41)
    dx, dy = np.meshgrid(d, d)
    for x0, y0 in [(0, 0), (5, 9), (-17, 3), (800, 800)]:
        pairs = np.stack([np.full(dx.size, x0), np.full(dx.size, y0), x0 + dx.ravel(), y0 + dy.ravel()], 1)
        lines = mk.run_lines(exe, tmp_path, pairs)
        for p, l in zip(pairs.tolist(), lines):
            assert np.array_equal(l, np.array(gr.grid_line(tuple(p[:2]), tuple(p[2:])))), p


def test_live_driver_equals_restatement(tmp_path):
    mk, exe = _live_driver(tmp_path)
    laser, r = mk.node_scan()
    am, ai = np.float32(laser.angle_min), np.float32(laser.angle_increment)
    node = mk.run_map(exe, tmp_path, (-40.0, -40.0, 40.0, 40.0, 0.05), r, am, ai, node=True)
    st, pub = gr.node_callback(r, am, ai)
    assert np.array_equal(node["visits"], st.visits) and np.array_equal(node["n"], st.n)
    assert node["acc_x"].tobytes() == st.acc_x.tobytes() and node["acc_y"].tobytes() == st.acc_y.tobytes()
    assert np.array_equal(node["mask"], st.mask) and np.array_equal(node["data"], pub)
    c, s = gr.angle_cache(len(r), am, ai)
    assert node["cos"].tobytes() == c.tobytes() and node["sin"].tobytes() == s.tobytes()
    # poses around the map centre, several scans into one map
    rng = np.random.default_rng(5)
    poses = np.stack([rng.uniform(-5, 5, 6), rng.uniform(-5, 5, 6), rng.uniform(-4, 4, 6)], 1)
    rr = np.stack([r] * 6)
    acc = mk.run_map(exe, tmp_path, (-40.0, -40.0, 40.0, 40.0, 0.05), rr, am, ai, poses=poses, node=False)
    st = gr.MapState(NODE_GEO)
    st.integrate(rr, poses, c, s, 30 - 0.01, 25.0)
    assert np.array_equal(acc["visits"], st.visits) and np.array_equal(acc["n"], st.n)
    assert acc["acc_x"].tobytes() == st.acc_x.tobytes() and acc["acc_y"].tobytes() == st.acc_y.tobytes()
    assert np.array_equal(acc["mask"], st.mask)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
GMAP_SYMBOLS = ["lslam_gmap_create", "lslam_gmap_destroy", "lslam_gmap_info", "lslam_gmap_set_laser", "lslam_gmap_angle_cache",
                "lslam_gmap_reset", "lslam_gmap_integrate", "lslam_gmap_compute_map", "lslam_gmap_read_counters",
                "lslam_gmap_read_patch_mask", "lslam_gmap_read_ros_i8", "lslam_gmap_stats"]


def test_gmap_entry_points_are_exported():
    from lslam_amd import api

    L = api.lib()
    assert L.lslam_abi_version() == 5
    for name in GMAP_SYMBOLS:
        assert hasattr(L, name), name
    header = (HERE.parent / "include" / "lslam_gpu.h").read_text()
    for name in GMAP_SYMBOLS:
        assert name + "(" in header, name


def test_gmap_calls_without_a_context_fail():
    from lslam_amd import api

    L = api.lib()
    h = ctypes.c_void_p()
    assert L.lslam_gmap_create(None, -1.0, -1.0, 1.0, 1.0, 0.05, ctypes.byref(h)) == -1
    assert L.lslam_gmap_integrate(None, 1, None, None) == -1
    assert L.lslam_gmap_stats(None, None) == -1
