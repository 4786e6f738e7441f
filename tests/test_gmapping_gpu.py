"""lesson4 GMapping count map on the device (lslam_gmap_*, csrc/gmapping_map.hip) against the fixture recorded from the
reference's own map classes and against the restatement (tests/gmapping_restatement.py): bit for bit everywhere --
visits, n, the raw float32 bits of acc, the patch mask, the published int8 grid."""
import math
import pathlib
import sys

import numpy as np
import pytest

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import gmapping_restatement as gr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = HERE / "golden" / "gmapping_golden.npz"
MAX_R, MAX_U = 30 - 0.01, 25.0


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def node_map(ctx, golden):
    from lslam_amd import api

    m = api.GMappingMap(ctx)
    am, ai = golden["node_angle"]
    m.set_laser(len(golden["node_ranges"]), am, ai, MAX_R, MAX_U)
    yield m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _equal_golden(m, d, prefix):
    v, n, ax, ay = m.counters()
    gv, gn, gax, gay = gr.unpack_counters(d, prefix, v.shape)
    assert np.array_equal(v, gv)
    assert np.array_equal(n, gn)
    assert np.array_equal(_bits(ax), _bits(gax))
    assert np.array_equal(_bits(ay), _bits(gay))
    assert np.array_equal(m.patch_mask(), d[prefix + "mask"])


def _equal_state(m, st: gr.MapState):
    v, n, ax, ay = m.counters()
    assert np.array_equal(v, st.visits)
    assert np.array_equal(n, st.n)
    assert np.array_equal(_bits(ax), _bits(st.acc_x))
    assert np.array_equal(_bits(ay), _bits(st.acc_y))
    assert np.array_equal(m.patch_mask(), st.mask)
    s = m.stats()
    assert [s["scans"], s["beams"], s["hits"], s["dropped"]] == st.stats


def test_node_callback_equals_golden(node_map, golden):
    m = node_map
    assert (m.info["map_size_x"], m.info["width"], m.info["size_x2"], m.info["patches_x"]) == (1600, 1600, 800, 50)
    c, s = m.angle_cache()
    assert c.tobytes() == golden["node_cos"].tobytes() and s.tobytes() == golden["node_sin"].tobytes()
    pub = m.compute_map(golden["node_ranges"], 0.25)
    assert np.array_equal(pub, golden["node_data"])
    _equal_golden(m, golden, "node_")
    # a second callback of the node is the same map (the node builds a fresh one per scan)
    assert np.array_equal(m.compute_map(golden["node_ranges"], 0.25), golden["node_data"])
    _equal_golden(m, golden, "node_")


def test_compute_map_equals_reset_integrate_publish(node_map, golden):
    m = node_map
    pub = m.compute_map(golden["node_ranges"], 0.3)
    m.reset()
    m.integrate(golden["node_ranges"])
    assert np.array_equal(m.ros_i8(0.3), pub)
    st, ref = gr.node_callback(golden["node_ranges"], *golden["node_angle"], cfg=dict(occ_thresh=0.3))
    assert np.array_equal(pub, ref)


def test_accumulate_sequence_equals_golden(node_map, golden):
    m = node_map
    m.reset()
    m.integrate(golden["acc_ranges"], golden["acc_poses"])
    _equal_golden(m, golden, "acc_")
    assert m.stats()["scans"] == 16 and m.stats()["dropped"] == 0


def test_batch_equals_single_scans(node_map, golden):
    m = node_map
    m.reset()
    m.integrate(golden["acc_ranges"], golden["acc_poses"])
    batch = m.counters(), m.patch_mask(), m.stats()
    m.reset()
    for r, p in zip(golden["acc_ranges"], golden["acc_poses"]):
        m.integrate(r[None], p[None])
    one = m.counters(), m.patch_mask(), m.stats()
    for a, b in zip(batch[0], one[0]):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(batch[1], one[1]) and batch[2] == one[2]


def test_reset_then_integrate_equals_fresh_map(ctx, node_map, golden):
    from lslam_amd import api

    m = node_map
    m.integrate(golden["acc_ranges"][:4], golden["acc_poses"][:4])  # something to reset
    m.reset()
    assert not m.patch_mask().any() and not m.counters()[0].any()
    m.integrate(golden["acc_ranges"][4:9], golden["acc_poses"][4:9])
    fresh = api.GMappingMap(ctx)
    fresh.set_laser(len(golden["node_ranges"]), *golden["node_angle"], MAX_R, MAX_U)
    fresh.integrate(golden["acc_ranges"][4:9], golden["acc_poses"][4:9])
    for a, b in zip(m.counters(), fresh.counters()):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(m.patch_mask(), fresh.patch_mask()) and m.stats() == fresh.stats()
    fresh.close()


def _multi_map(ctx, n_beams, angle):
    from lslam_amd import api

    m = api.GMappingMap(ctx)
    m.set_laser(n_beams, *angle, MAX_R, MAX_U)
    return m


def test_multi_hit_order_is_bit_exact(ctx, golden):
    r = golden["multi_ranges"]
    m = _multi_map(ctx, r.shape[1], golden["multi_angle"])
    m.integrate(r, golden["multi_poses"])
    _equal_golden(m, golden, "multi_")
    m.close()


def test_one_cell_hit_by_4096_scans(ctx):
    """4096 scans x 2 beams end in the cell around (-7.3, 12.1): one 8192-long ordered float sum per component."""
    rng = np.random.default_rng(17)
    S = 4096
    poses = np.stack([rng.uniform(-1, 1, S), rng.uniform(-1, 1, S), np.zeros(S)], 1)
    ranges = np.zeros((S, 2), np.float32)
    for s in range(S):
        tx, ty = -7.3 + rng.uniform(-0.01, 0.01), 12.1 + rng.uniform(-0.01, 0.01)
        poses[s, 2] = math.atan2(ty - poses[s, 1], tx - poses[s, 0])
        ranges[s] = math.hypot(tx - poses[s, 0], ty - poses[s, 1]) + rng.uniform(-0.01, 0.01, 2)
    m = _multi_map(ctx, 2, (0.0, 0.0))
    m.integrate(ranges, poses)
    st = gr.MapState(gr.Geometry(-40.0, -40.0, 40.0, 40.0, 0.05))
    c, s = gr.angle_cache(2, 0.0, 0.0)
    st.integrate(ranges, poses, c, s, MAX_R, MAX_U)
    assert st.n.max() == 2 * S
    _equal_state(m, st)
    m.close()


def _special(rng, n):
    r = rng.uniform(0.02, 32.0, n).astype(np.float32)
    pick = rng.random(n)
    r[pick < 0.03] = np.nan
    r[(pick >= 0.03) & (pick < 0.05)] = np.inf
    r[(pick >= 0.05) & (pick < 0.07)] = 0.0
    r[(pick >= 0.07) & (pick < 0.09)] = 25.0
    r[(pick >= 0.09) & (pick < 0.12)] = rng.uniform(0.0, 0.05, int(((pick >= 0.09) & (pick < 0.12)).sum()))
    return r


def test_fuzz_equals_restatement(ctx):
    rng = np.random.default_rng(2024)
    from lslam_amd import api

    for trial in range(3):
        nb = int(rng.integers(50, 400))
        am, ai = np.float32(rng.uniform(-3.2, 0)), np.float32(rng.uniform(0.001, 0.03))
        box = (-12.0 - trial, -10.0, 9.5 + trial, 11.25, 0.05 + 0.01 * trial)
        m = api.GMappingMap(ctx, *box)
        m.set_laser(nb, am, ai, 12.0, 8.0)
        S = int(rng.integers(3, 12))
        poses = np.stack([rng.uniform(-8, 8, S), rng.uniform(-8, 8, S), rng.uniform(-7, 7, S)], 1)
        ranges = np.stack([_special(rng, nb) for _ in range(S)])
        m.integrate(ranges, poses)
        st = gr.MapState(gr.Geometry(*box))
        c, s = gr.angle_cache(nb, am, ai)
        st.integrate(ranges, poses, c, s, 12.0, 8.0)
        _equal_state(m, st)
        assert np.array_equal(m.ros_i8(0.25), st.publish(0.25))
        m.close()


def test_out_of_map_poses_are_clipped_and_counted(ctx):
    from lslam_amd import api

    box = (-5.0, -5.0, 5.0, 5.0, 0.05)
    m = api.GMappingMap(ctx, *box)
    rng = np.random.default_rng(8)
    nb = 180
    m.set_laser(nb, -math.pi, 2 * math.pi / nb, 20.0, 15.0)
    poses = np.array([[4.0, 4.5, 0.3], [-9.0, 0.0, 0.0], [30.0, -30.0, 1.0], [0.0, 0.0, 2.0]])
    ranges = rng.uniform(0.5, 14.0, (4, nb)).astype(np.float32)
    m.integrate(ranges, poses)
    st = gr.MapState(gr.Geometry(*box))
    c, s = gr.angle_cache(nb, -math.pi, 2 * math.pi / nb)
    st.integrate(ranges, poses, c, s, 20.0, 15.0)
    assert st.stats[3] > 0
    _equal_state(m, st)
    m.close()


def test_padded_box_equals_golden(ctx, golden):
    from lslam_amd import api

    m = api.GMappingMap(ctx, -40.0, -40.0, 41.0, 41.0, 0.05)
    m.set_laser(len(golden["node_ranges"]), *golden["node_angle"], MAX_R, MAX_U)
    assert (m.info["map_size_x"], m.info["width"], m.info["height"], m.info["size_x2"]) == (1600, 1620, 1620, 810)
    pub = m.compute_map(golden["node_ranges"], 0.25)
    assert np.array_equal(pub, golden["pad_data"])
    _equal_golden(m, golden, "pad_")
    m.close()


def test_invalid_arguments_are_rejected(ctx, golden):
    from lslam_amd import api

    for box in [(-1.0, -1.0, 1.0, 1.0, 0.0), (-1.0, -1.0, 1.0, 1.0, -0.05), (1.0, -1.0, 1.0, 1.0, 0.05),
                (-1.0, 1.0, 1.0, -1.0, 0.05), (-0.5, -0.5, 0.5, 0.5, 0.05), (-40.0, -40.0, 40.0, 40.0, float("nan"))]:
        with pytest.raises(api.LslamError) as e:
            api.GMappingMap(ctx, *box)
        assert e.value.code == -1, box
    # 1599.5 cells: the published grid (1599) would be narrower than the 1600-cell storage
    with pytest.raises(api.LslamError) as e:
        api.GMappingMap(ctx, -40.0, -40.0, 39.975, 40.0, 0.05)
    assert e.value.code == -8
    # storage of 65536^2 cells would not fit the 32-bit cell keys: refused before anything is allocated
    for box in [(0.0, 0.0, 65536.0, 65536.0, 1.0), (0.0, 0.0, 65535.5, 100.0, 1.0), (0.0, 0.0, 100.0, 65504.5, 1.0)]:
        with pytest.raises(api.LslamError) as e:
            api.GMappingMap(ctx, *box)
        assert e.value.code == -8, box
    m = api.GMappingMap(ctx)
    with pytest.raises(api.LslamError) as e:  # no laser yet
        m.ctx.check(m.L.lslam_gmap_integrate(m.h, 1, golden["node_ranges"].ctypes.data, None))
    assert e.value.code == -1
    for bad in [(0, 0.0, 0.01, 30.0, 25.0), (10, 0.0, 0.01, 0.0, 25.0), (10, 0.0, 0.01, 30.0, -1.0)]:
        with pytest.raises(api.LslamError):
            m.set_laser(*bad)
    m.set_laser(len(golden["node_ranges"]), *golden["node_angle"], MAX_R, MAX_U)
    with pytest.raises(api.LslamError) as e:
        m.integrate(golden["node_ranges"][None], np.array([[0.0, 0.0, float("nan")]]))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        m.integrate(np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError):  # an empty 1-D array is one scan of no readings, not n_beams of them
        m.integrate(np.zeros(0, np.float32))
    with pytest.raises(ValueError):
        m.compute_map(np.zeros(0, np.float32))
    m.integrate(np.zeros((0, len(golden["node_ranges"])), np.float32))  # no scans: nothing to do
    # more than 2^28 readings in one call: refused before the ranges are read
    with pytest.raises(api.LslamError) as e:
        m.ctx.check(m.L.lslam_gmap_integrate(m.h, (1 << 28) // len(golden["node_ranges"]) + 1,
                                             golden["node_ranges"].ctypes.data, None))
    assert e.value.code == -1
    m.close()


def test_grid_line_sweep_through_the_device(ctx):
    """Every endpoint offset |dx|, |dy| <= 40 from three starts, one single-beam scan each, through lslam_gmap_integrate:
    the visits and hits equal the stepped gridLine of the restatement (the fixture's gridLine traces pin that one)."""
    from lslam_amd import api

    box = (-5.0, -5.0, 5.0, 5.0, 0.05)
    geo = gr.Geometry(*box)
    d = np.arange(-40, 41)
    dx, dy = (a.ravel() for a in np.meshgrid(d, d))
    keep = (dx != 0) | (dy != 0)  # a zero range is filtered
    dx, dy = dx[keep], dy[keep]
    for cx, cy in [(100, 100), (57, 143), (141, 60)]:
        x0, y0 = (cx - geo.size_x2) * 0.05, (cy - geo.size_y2) * 0.05
        theta = np.arctan2(dy, dx)
        ranges = (np.hypot(dx, dy) * 0.05).astype(np.float32)[:, None]
        poses = np.stack([np.full(len(dx), x0), np.full(len(dx), y0), theta], 1)
        # the endpoints land on the intended cells
        px, py = geo.world2map(x0 + ranges[:, 0].astype(np.float64) * np.cos(theta),
                               y0 + ranges[:, 0].astype(np.float64) * np.sin(theta))
        assert np.array_equal(px, cx + dx) and np.array_equal(py, cy + dy)
        m = api.GMappingMap(ctx, *box)
        m.set_laser(1, 0.0, 0.0, 20.0, 10.0)
        m.integrate(ranges, poses)
        v, n, _, _ = m.counters()
        ev = np.zeros_like(v)
        en = np.zeros_like(n)
        for a, b in zip(dx.tolist(), dy.tolist()):
            pts = gr.grid_line((cx, cy), (cx + a, cy + b))
            assert pts[-1] == (cx + a, cy + b)
            for x, y in pts[:-1]:
                ev[y, x] += 1
            ev[cy + b, cx + a] += 1
            en[cy + b, cx + a] += 1
        assert np.array_equal(v, ev) and np.array_equal(n, en)
        m.close()


def test_long_lines_take_the_64_bit_path(ctx):
    """Lines of ~40 000 cells (beyond the 32-bit division's 32767) on a 40192 x 32 storage equal the restatement."""
    from lslam_amd import api

    box = (0.0, 0.0, 2010.0, 1.65, 0.05)
    m = api.GMappingMap(ctx, *box)
    assert (m.info["map_size_x"], m.info["map_size_y"]) == (40192, 32)
    nb, am, ai = 8, np.float32(0.0), np.float32(3.5e-5)
    m.set_laser(nb, am, ai, 2005.0, 2005.0)
    poses = np.array([[2.0, 0.1, 0.0], [2004.0, 1.4, math.pi]])
    ranges = np.array([[1995.0, 1990.5, 1800.0, 1500.25, 2000.0, 1999.0, 1700.0, 1980.0]] * 2, np.float32)
    m.integrate(ranges, poses)
    st = gr.MapState(gr.Geometry(*box))
    c, s = gr.angle_cache(nb, am, ai)
    st.integrate(ranges, poses, c, s, 2005.0, 2005.0)
    assert st.visits.sum() > 2 * nb * 32768
    _equal_state(m, st)
    m.close()
