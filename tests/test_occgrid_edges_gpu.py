"""The occupancy-grid kernels (k_occ_points, k_occ_trace / occ_trace_beam, k_occ_update, k_occ_add) on the directed scenarios
of tests/occgrid_cases.py: hit and pass counters word for word against the plain-C oracle, which
tests/test_occgrid_cases_oracle.py holds to the stepped TraceLine on the same scenarios -- every octant, lane-stride and block
boundaries, clipped rays, every beam class at its limits, exact rounding ties, empty grids -- then the cell rules on every
(pass, hit) pair up to 40 and the counter merge.  All integer work: every comparison is exact."""
import numpy as np
import pytest

import occgrid_cases as E
from lslam_amd import api

pytestmark = pytest.mark.gpu


def port_of(oracle_lib, sc):
    return oracle_lib.PortKarto(oracle_lib.default_cfg(), oracle_lib.laser_struct(sc.laser, sc.threshold))


def ros_of(data):
    """karto_slam.cc:546-569: unknown -> -1, occupied -> 100, free -> 0"""
    return np.where(data == 0, -1, np.where(data == 100, 100, 0)).astype(np.int8)


def check_cells(g, port, dims, counters):
    exp = port.occgrid_update(dims, counters)
    assert g.data().shape == exp.shape
    assert np.array_equal(g.data(), exp)
    assert np.array_equal(g.ros_data(), ros_of(exp))


@pytest.mark.parametrize("name", E.COUNTER_NAMES)
def test_counters_equal_the_oracle(ctx, oracle_lib, name):
    sc = E.scenario(name)
    port, lp = port_of(oracle_lib, sc), api.laser_params(sc.laser, sc.threshold)
    if sc.box is None:
        box = port.occgrid_bounds(sc.ranges, sc.poses)
        g = api.OccupancyGrid.CreateFromScans(ctx, lp, sc.ranges, sc.poses, sc.resolution)
    else:
        box = sc.box
        g = api.OccupancyGrid.CreatePartial(ctx, lp, sc.ranges, sc.poses, sc.resolution, box)
    dims, cnt = port.occgrid_partial(sc.ranges, sc.poses, sc.resolution, box)
    w, h, off, res = g.info()
    assert (w, h) == (dims[0], dims[1]) and res == sc.resolution
    assert np.array_equal(off, box[:2])
    got = g.export_counters()
    assert got.shape == cnt.shape and got.dtype == cnt.dtype
    assert np.array_equal(got, cnt)
    check_cells(g, port, dims, cnt)
    g.close()


def test_box_extremum_bounds(ctx, oracle_lib):
    """The shared-memory and atomicCAS box reduction with the one valid reading in the first and last lane of a wave and of
    a block, each scan alone and together, and the four extremes coming from four scans and four blocks."""
    sc = E.scenario("box_extremum")
    port, lp = port_of(oracle_lib, sc), api.laser_params(sc.laser, sc.threshold)
    for rows in sc.groups:
        got = api.OccupancyGrid.scan_bounds(ctx, lp, sc.ranges[rows], sc.poses[rows])
        assert np.array_equal(got, port.occgrid_bounds(sc.ranges[rows], sc.poses[rows])), rows


def empty_grid(ctx, w, h):
    g = api.OccupancyGrid.CreatePartial(ctx, api.laser_params(E.ONE_BEAM, 20.0), np.zeros((0, 1)), np.zeros((0, 3)), 0.05,
                                        [0.0, 0.0, w * 0.05, h * 0.05])
    assert g.info()[:2] == (w, h)
    return g


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_cell_rules(ctx, oracle_lib, on_device):
    """UpdateCell on every (pass, hit) pair up to 40 -- pass 2 and 3 on both sides of MinPassThrough, ratios at 1/10, 2/20,
    3/30, 4/40 and their neighbours -- on a 41-wide grid whose rows are 48 words apart, then on counters at 2^31 and
    2^32 - 1."""
    import torch
    port = port_of(oracle_lib, E.scenario("exact_ties"))
    n, stride = 41, 48
    g = empty_grid(ctx, n, n)
    assert g.counter_words() == 2 * n * stride and not g.export_counters().any() and not g.data().any()
    small = np.zeros((2, n, stride), dtype=np.uint32)
    small[0, :, :n] = np.arange(n)[None, :]   # pass = column
    small[1, :, :n] = np.arange(n)[:, None]   # hit = row
    big = np.zeros_like(small)
    big[0, 0, :4] = [2 ** 32 - 1, 2 ** 32 - 1, 2 ** 31, 2 ** 31]
    big[1, 0, :4] = [0, 2 ** 32 - 1, 0, 2 ** 31]
    for cnt in (small, big):
        if on_device:
            t = torch.from_numpy(cnt.view(np.int32).reshape(-1)).to("cuda:0")
            torch.cuda.synchronize()
            g.import_counters_dev(t.data_ptr())
        else:
            g.import_counters(cnt)
        assert np.array_equal(g.export_counters(), cnt.reshape(2, -1))
        check_cells(g, port, [n, n, stride], cnt.reshape(2, -1))
    # what the oracle says at the limits, spelled out: row = hit, column = pass
    exp = port.occgrid_update([n, n, stride], small.reshape(2, -1))
    assert exp[1, 2] == 0 and exp[1, 3] == 100 and exp[0, 2] == 0 and exp[0, 3] == 255
    assert [int(exp[k, 10 * k]) for k in (1, 2, 3, 4)] == [255] * 4          # exactly one tenth: not above it
    assert [int(exp[k, 10 * k - 1]) for k in (1, 2, 3, 4)] == [100] * 4 and [int(exp[k, 10 * k + 1]) for k in (1, 2, 3)] == [255] * 3
    assert port.occgrid_update([n, n, stride], big.reshape(2, -1))[0, :4].tolist() == [255, 100, 255, 100]
    g.close()


def test_shards_accumulate_to_the_unsplit_counters(ctx, oracle_lib):
    """sweep_centre's scans in three unequal shards, one of them empty, added up with import_counters(accumulate=True):
    k_occ_add over 54 096 words, no multiple of its 256 threads."""
    sc = E.scenario(E.SWEEP_CENTRE)
    port, lp = port_of(oracle_lib, sc), api.laser_params(sc.laser, sc.threshold)
    dims, cnt = port.occgrid_partial(sc.ranges, sc.poses, sc.resolution, sc.box)
    cuts = [(0, 7001), (7001, 7001), (7001, len(sc.ranges))]
    parts = [api.OccupancyGrid.CreatePartial(ctx, lp, sc.ranges[a:b], sc.poses[a:b], sc.resolution, sc.box) for a, b in cuts]
    assert parts[0].counter_words() == cnt.size and cnt.size % 256 != 0
    assert not parts[1].export_counters().any()
    assert parts[0].export_counters().any() and not np.array_equal(parts[0].export_counters(), cnt)
    total = empty_grid(ctx, 161, 161)
    for p in parts:
        total.import_counters(p.export_counters(), accumulate=True)
    assert np.array_equal(total.export_counters(), cnt)
    check_cells(total, port, dims, cnt)
    for g in parts + [total]:
        g.close()
