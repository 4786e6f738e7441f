"""The coarse response kernels that only lslam_matcher_set_option selects -- k_resp_rows_mw (rows_waves 2 / 4 / 8), the
LDS-staged phase B (lds_staged), the instrumented twins (collect_stats) and the occ == nullptr path of every rows kernel
(row_occupancy 0) -- against the oracle, bit for bit.

Every case builds ONE batch and compares in two steps:
  (a) default options: the numerators of min(S, nq) + 40 seeded-random scans equal the oracle's lattices
      (kor_correlate_scan, pinned to the reference's CorrelateScan by test_oracle_vs_ref.py) and their records its match;
  (b) each option: the WHOLE numerator array and the WHOLE record array are byte-identical to the default run, and
      coarse_form_launches() shows that the intended form -- not one of the dispatch's silent fallbacks -- took the
      coarse launches (all forms go out under the one profile name resp_rows_coarse).
Everything is integer sums or records derived from them: no tolerances.  The counters of the instrumented twins
(lslam_matcher_read_stats / read_beam_stats, the source of the README's pruning percentages) are checked against a count
made on the CPU from the oracle's lookup table, lattice and grid."""
import ctypes
import math

import numpy as np
import pytest

from lslam_amd import api, synth

from test_matcher_gpu import _assert_result, half_cell_boundary_scan, make_pair

pytestmark = pytest.mark.gpu

RES = 0.05                      # every case stays at 0.05 m cells (coarse lattice step = 2 cells = 0.1 m)
ANGLES = (0.349, 0.0349)        # default coarse angle offset / resolution: 21 candidate angles
COARSE_FORMS = ("generic", "rows_linear", "rows_tiled", "rows_multiwave", "rows_lds_staged", "rows_stats_linear",
                "rows_stats_tiled", "rows_stats_lds_staged", "big")
OPTIONAL_FORMS = COARSE_FORMS[3:8]
DEFAULTS = {"rows_waves": 1, "lds_staged": 0, "collect_stats": 0, "row_occupancy": 1, "pipeline_depth": 1}
INT_MAX = np.iinfo(np.int32).max


def _kround(v):  # math::Round (Math.h) as the oracle restates it
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


class _Case:
    """One matcher pair (oracle + device, same grid) and one batch.  default(S) runs the first S scans with default
    options, ONCE, anchors that run to the oracle (step (a)) and returns its read-only (numerators, records)."""

    def __init__(self, port, gm, ranges, poses, nq, search_size=1.0, angles=ANGLES):
        self.port, self.gm, self.nq, self.angles = port, gm, nq, angles
        self.ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        self.poses = np.ascontiguousarray(poses, dtype=np.float64)
        side = int(_kround(search_size / RES) + 1)
        self.off = 0.5 * (side - 1) * RES  # Mapper.cpp:229-230, the oracle's own expression
        self.nx = int(math.floor(self.off * 2.0 / (2 * RES) + 0.5) + 1)
        self.block_rows = 11 if self.nx <= 12 else 8  # lattice rows one pass of k_resp_rows<3,11> / <4,8> holds
        self._oracle, self._runs, self._counts = {}, {}, None

    def oracle(self, q):
        if q not in self._oracle:
            r, p = self.ranges[q], self.poses[q]
            _, _, _, st, sums = self.port.correlate_scan(r, p, p, self.off, 2 * RES, *self.angles, True, False, want_sums=True)
            assert st == 0, (q, st)
            assert sums.shape == (self.nx, self.nx, sums.shape[2])
            self._oracle[q] = (sums, self.port.match(r, p))
        return self._oracle[q]

    def run(self, S, fine=False):
        r, p = self.ranges[:S], self.poses[:S]
        out = [self.gm.coarse_sums_batch(r, p), self.gm.match_batch(r, p)]
        if fine:
            out += list(self.gm.fine_sums_batch(r, p))
        return out

    def default(self, S):
        if S not in self._runs:
            sums, recs = self.run(S)
            assert sums.shape[:3] == (S, self.nx, self.nx) and sums.any()
            rng = np.random.default_rng(1000 + S)
            check = np.unique(np.concatenate([np.arange(min(S, self.nq)), rng.integers(0, S, size=40)]))
            for q in check:
                o_sums, (mean, cov, resp) = self.oracle(int(q))
                assert np.array_equal(sums[q], o_sums), q
                _assert_result(recs[q], mean, cov, resp)
            sums.flags.writeable = False
            recs.flags.writeable = False
            self._runs[S] = (sums, recs)
        return self._runs[S]

    def scrub(self, S):
        """The workspaces still hold the numerators of the last run -- of this very batch, as a rule, so a kernel that
        skipped part of its output would be covered by the right values left behind.  A batch of S unreadable scans
        leaves zeros instead."""
        blind = np.full_like(self.ranges[:S], np.nan)
        assert not self.gm.coarse_sums_batch(blind, self.poses[:S]).any()
        self.gm.match_batch(blind, self.poses[:S])

    def with_options(self, S, opts, fine=False):
        """The same batch with `opts` set: (arrays of run(), launches per form of that run).  Options are put back."""
        self.scrub(S)
        before = self.gm.coarse_form_launches()
        try:
            for k, v in opts.items():
                self.gm.set_option(k, v)
            out = self.run(S, fine)
        finally:
            for k in opts:
                self.gm.set_option(k, DEFAULTS[k])
        after = self.gm.coarse_form_launches()
        return out, {k: after[k] - before[k] for k in after}

    def check_same(self, S, opts, form, fine=False):
        """Step (b): byte-identical to the default run, through `form` and no other coarse form."""
        want = list(self.default(S))
        if fine:
            want += list(self.gm.fine_sums_batch(self.ranges[:S], self.poses[:S]))
        got, launches = self.with_options(S, opts, fine)
        # one coarse pass in coarse_sums_batch, one in match_batch (one more with the fine numerators)
        assert {k: launches[k] for k in COARSE_FORMS if launches[k]} == {form: 3 if fine else 2}, launches
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (opts, np.argwhere(g != w)[:4] if g.dtype.names is None else None)

    # ---- the CPU side of the instrumented counters ---------------------------------------------------------------------
    def lattice_origin(self, q):
        """Flat index of the first candidate (xi = yi = 0) of scan q's coarse lattice (Mapper.cpp:385-386 as the oracle
        restates it), having checked that the lattice is uniform: 2 cells from candidate to candidate."""
        gi = self.port.grid_info()
        scale, border = 1.0 / RES, gi["roi_x"]
        cx, cy = self.poses[q][0], self.poses[q][1]
        g = [[int(_kround(((c + (-self.off + i * (2 * RES))) - o) * scale)) + border for i in range(self.nx)]
             for c, o in ((cx, gi["offset"][0]), (cy, gi["offset"][1]))]
        for axis in g:
            assert axis == [axis[0] + 2 * i for i in range(self.nx)], axis
        return g[0][0] + g[1][0] * gi["stride"]

    def row_starts(self, q):
        """(f, readable): f[a, b, j] = flat index of the first cell of lattice row j of beam b at angle a (the oracle's
        lookup table + the lattice origin); readable[a, b] = the table holds the beam (a finite reading)."""
        r, p = self.ranges[q], self.poses[q]
        tbl = self.port.compute_offsets(r, p, p[2], *self.angles)
        stride = self.port.grid_info()["stride"]
        readable = tbl != INT_MAX
        f = (self.lattice_origin(q) + np.where(readable, tbl, 0).astype(np.int64))[:, :, None] + \
            (2 * stride * np.arange(self.nx, dtype=np.int64))[None, None, :]
        return f, readable

    def cpu_counts(self, S):
        """Per scan, what one instrumented coarse pass must count (include/lslam_gpu.h, LSLAM_OPT_COLLECT_STATS):
          rows         lattice rows with a candidate inside [0, dataSize) (the reference's 1-D check, Mapper.cpp:841-845)
          rows_nz      those whose nX candidate bytes really hold a non-zero: pruning may never drop one of them
          pairs        readable beam x angle pairs, once per block of lattice rows the kernel takes in one pass
          pairs_in     those with a row of that block inside the index range: what is left to queue without pruning
          pairs_nz     those with a really non-zero row in that block
          beams, beams_nz   readable beams; those with a really non-zero row at any angle
          below, above      rows with a candidate below flat index 0 / past dataSize (search centres near the grid's edge)"""
        if self._counts is None:
            self._counts = self._count_all()
        return {k: v[:S] for k, v in self._counts.items()}

    def _count_all(self):
        S = len(self.ranges)
        grid = self.port.grid().reshape(-1)
        data, pad = grid.size, 2 * (self.nx - 1)
        gp = np.concatenate([np.zeros(pad, bool), grid != 0, np.zeros(pad, bool)])
        row_nz = np.zeros(data + pad, bool)  # [f + pad]: any of grid[f], grid[f + 2], ... grid[f + 2 (nX - 1)] non-zero
        for i in range(self.nx):
            row_nz |= gp[2 * i: 2 * i + data + pad]
        keys = ("rows", "rows_nz", "pairs", "pairs_in", "pairs_nz", "beams", "beams_nz", "below", "above")
        out = {k: np.zeros(S, dtype=np.int64) for k in keys}
        for q in range(S):
            f, readable = self.row_starts(q)
            inr = (f >= -pad) & (f < data) & readable[:, :, None]
            nz = inr & row_nz[np.clip(f + pad, 0, data + pad - 1)]
            out["rows"][q], out["rows_nz"][q] = inr.sum(), nz.sum()
            for j0 in range(0, self.nx, self.block_rows):
                out["pairs"][q] += readable.sum()
                out["pairs_in"][q] += inr[:, :, j0:j0 + self.block_rows].any(axis=2).sum()
                out["pairs_nz"][q] += nz[:, :, j0:j0 + self.block_rows].any(axis=2).sum()
            out["beams"][q] = readable.any(axis=0).sum()
            out["beams_nz"][q] = nz.any(axis=(0, 2)).sum()
            out["below"][q] = ((f < 0) & readable[:, :, None]).sum()
            out["above"][q] = ((f + pad >= data) & readable[:, :, None]).sum()
        return out

    def cpu_sums(self, q):
        """The oracle's numerators of scan q rebuilt from row_starts(): pins the CPU count's geometry to the oracle."""
        grid = self.port.grid().reshape(-1)
        f, readable = self.row_starts(q)
        idx = f[:, :, :, None] + 2 * np.arange(self.nx, dtype=np.int64)  # [a, b, yi, xi]
        ok = (idx >= 0) & (idx < grid.size) & readable[:, :, None, None]
        vals = np.where(ok, grid[np.clip(idx, 0, grid.size - 1)], 0).astype(np.int64)
        return vals.sum(axis=1).transpose(1, 2, 0)  # [yi, xi, a]


def _spread_batch(wl, S, seed):
    """The construction of test_coarse_sums_of_whole_batches_bit_exact: the repeats get poses of their own, 1 % NaN."""
    nq = len(wl.query_ranges)
    idx = np.arange(S) % nq
    poses = wl.query_poses[idx].copy()
    rng = np.random.default_rng(seed)
    far = np.arange(S) >= nq
    poses[far, :2] += rng.uniform(-0.4, 0.4, size=(int(far.sum()), 2))
    poses[far, 2] += rng.uniform(-0.3, 0.3, size=int(far.sum()))
    ranges = wl.query_ranges[idx].copy()
    ranges[rng.random(ranges.shape) < 0.01] = np.nan
    return ranges, poses


def _case_a(ctx, oracle_lib, wl):
    """A: the standard 11 x 11 x 21 lattice at S = 100 -- padded to 104 scans (tail blocks with s >= S), 104 * 21 = 2184
    waves >= kTileMinWaves (tiled planes), 21 angles (a partial last group for W = 2, 4 and 8).  Its first 40 scans are
    the small batch: beam slices on the linear planes."""
    port, gm = make_pair(ctx, oracle_lib)
    port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
    gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
    return _Case(port, gm, *_spread_batch(wl, 100, 100), nq=len(wl.query_ranges))


def _case_b(ctx, oracle_lib, wl):
    """B: search space 1.4 m -> 15 x 15 x 21 (lattice rows of 13..16 positions: the <4,8> family, two passes of 8 rows)."""
    kw = dict(search_size=1.4)
    port, gm = make_pair(ctx, oracle_lib, cfg_kw=kw)
    port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
    gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
    c = _Case(port, gm, *_spread_batch(wl, 100, 101), nq=len(wl.query_ranges), **kw)
    assert 13 <= c.nx <= 16
    return c


def _case_c(ctx, oracle_lib, wl):
    """C: coarse angle offset 2 x resolution -> 5 candidate angles, fewer than the 8 waves of a block (one group, three idle
    waves).  409 scans: the smallest batch that is no multiple of 8 whose padded size keeps 5 angles at or above
    kTileMinWaves = 2048 waves (416 * 5 = 2080; 408 * 5 = 2040 would fall back to beam slices)."""
    angles = (2 * 0.0349, 0.0349)
    laser = synth.Laser()
    port = oracle_lib.PortKarto(oracle_lib.default_cfg(coarse_angle_offset=angles[0], coarse_angle_resolution=angles[1]),
                                oracle_lib.laser_struct(laser))
    gm = api.ScanMatcher(ctx, api.baseline_config(coarse_search_angle_offset=angles[0], coarse_angle_resolution=angles[1]),
                         api.laser_params(laser))
    port.set_base_scans(wl.base_ranges, wl.base_poses, wl.center_pose)
    gm.AddScans(wl.base_ranges, wl.base_poses, wl.center_pose)
    return _Case(port, gm, *_spread_batch(wl, 409, 102), nq=len(wl.query_ranges), angles=angles)


def _case_d(heading):
    def build(ctx, oracle_lib, wl):
        """D: the scan of test_beams_on_half_cell_boundaries -- every beam parked for the fp64 decision at candidate angle
        10 of 21.  A table cell does not depend on where the sensor stands, only on its heading, so the second half of the
        batch searches around centres of its own and still parks every beam."""
        laser = synth.Laser()
        port, gm = make_pair(ctx, oracle_lib, laser)
        r = half_cell_boundary_scan(laser)
        base_poses = np.array([[1.0, 2.0, heading], [1.05, 2.0, heading], [1.0, 1.95, heading]])
        center = np.array([1.03, 1.98, heading])
        port.set_base_scans(np.stack([r, r, r]), base_poses, center)
        gm.AddScans(np.stack([r, r, r]), base_poses, center)
        S = 100
        poses = np.tile(center, (S, 1))
        poses[S // 2:, :2] += np.random.default_rng(103).uniform(-0.3, 0.3, size=(S - S // 2, 2))
        return _Case(port, gm, np.tile(r, (S, 1)), poses, nq=1)
    return build


def _case_e(ctx, oracle_lib, wl):
    """E: search centres next to the grid's first and last rows (the `edge` pose of test_loop_closure_size_lattice, at
    both ends): candidate rows hang over flat index 0 or run past dataSize.  The grid is a seeded sprinkle of smear values
    installed on both sides (a real window leaves its rim empty: every sum there would be 0)."""
    port, gm = make_pair(ctx, oracle_lib)
    gi = port.grid_info()
    rng = np.random.default_rng(104)
    grid = np.zeros((gi["height"], gi["stride"]), dtype=np.uint8)
    hit = rng.random((gi["height"], gi["width"])) < 0.004
    grid[:, :gi["width"]][hit] = rng.choice(np.array([6, 25, 100], dtype=np.uint8), size=int(hit.sum()))
    offset = np.array([-50.0, -50.0])
    port.set_grid(grid, offset)
    gm.set_grid(grid, offset)
    S = 100
    ranges, _ = _spread_batch(wl, S, 104)
    lo = offset + 0.5 + np.array([0.3, 0.2])                      # 0.5 = half the search space
    hi = offset + (gi["roi_w"] - 1) * RES - 0.5 - np.array([0.3, 0.2])
    poses = np.empty((S, 3))
    inward = np.where(np.arange(S)[:, None] % 2 == 0, 1.0, -1.0)  # even scans at the low corner, odd ones at the high
    poses[:, :2] = np.where(inward > 0, lo, hi) + inward * rng.uniform(0.0, 0.4, size=(S, 2))
    poses[:, 2] = rng.uniform(-math.pi, math.pi, size=S)
    c = _Case(port, gm, ranges, poses, nq=40)
    for q in range(S):  # keep a scan only where the oracle accepts it: inward a cell at a time, 20 cells at the most
        for _ in range(21):
            p = c.poses[q]
            st = port.correlate_scan(c.ranges[q], p, p, c.off, 2 * RES, *ANGLES, True, False)[3]
            if st == 0:
                break
            c.poses[q, :2] += inward[q] * RES
        assert st == 0, q
    counts = c.cpu_counts(S)
    assert counts["below"][0::2].sum() > 0 and counts["above"][1::2].sum() > 0  # rows really leave the index range
    assert (counts["rows"] < c.nx * counts["pairs"]).any()                        # and whole rows are outside it
    return c


def _case_many_beams(ctx, oracle_lib, wl):
    """The laser of test_many_beam_laser: 2881 beams > 64 * kMaxBeamsPerLane, so every batch splits its beams."""
    n, thr = 2881, 20.0
    laser = synth.Laser(n_ranges=n, angle_min=math.radians(-180.0), angle_increment=math.radians(0.125), range_max=30.0)
    port = oracle_lib.PortKarto(oracle_lib.default_cfg(), oracle_lib.laser_struct(laser, thr))
    gm = api.ScanMatcher(ctx, api.baseline_config(range_threshold=thr), api.laser_params(laser, thr))
    world = synth.arena(size=40.0, n_axis=12, n_rot=4, seed=21)
    mb = synth.make_match_workload(n_base=6, n_query=4, seed=21, laser=laser, world=world, query_spread=2.0)
    port.set_base_scans(mb.base_ranges, mb.base_poses, mb.center_pose)
    gm.AddScans(mb.base_ranges, mb.base_poses, mb.center_pose)
    return _Case(port, gm, *_spread_batch(mb, 100, 105), nq=len(mb.query_ranges))


_BUILDERS = {"A": _case_a, "B": _case_b, "C": _case_c, "D0": _case_d(0.0), "D90": _case_d(math.pi / 2), "E": _case_e,
             "many_beams": _case_many_beams}


@pytest.fixture(scope="module")
def cases(ctx, oracle_lib, workload_spread):
    built = {}

    def get(name):
        if name not in built:
            built[name] = _BUILDERS[name](ctx, oracle_lib, workload_spread)
        return built[name]

    yield get
    for c in built.values():
        c.gm.close()
        c.port.close()


# ---- rows_waves: k_resp_rows_mw<3,11,W> / <4,8,W> ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,W", [(n, 100, w) for n in ("A", "B", "D0", "D90") for w in (2, 4, 8)] +
                         [("C", 409, 8), ("E", 100, 4)])
def test_rows_waves(cases, name, S, W):
    c = cases(name)
    if name == "C":
        assert c.default(S)[0].shape[3] == 5  # fewer angles than waves per block
    c.check_same(S, {"rows_waves": W}, "rows_multiwave")


def test_rows_waves_falls_back_beyond_2048_beams(cases):
    """More than 64 * kMaxBeamsPerLane beams: the multi-wave form does not take beam slices, the one-wave form on the linear
    planes runs whatever rows_waves says -- the counter shows it, the results do not change."""
    c = cases("many_beams")
    assert c.gm.num_beams > 2048
    c.check_same(100, {"rows_waves": 4}, "rows_linear")


# ---- lds_staged: k_resp_rows<3,11,false,*,true> on the LINEAR planes ------------------------------------------------------
@pytest.mark.parametrize("name,form", [("A", "rows_lds_staged"), ("D0", "rows_lds_staged"), ("D90", "rows_lds_staged"),
                                       ("E", "rows_lds_staged"), ("B", "rows_tiled")])
def test_lds_staged(cases, name, form):
    """Lattice rows of 13..16 positions (B) have no LDS-staged form: there the option must change nothing, launches included."""
    cases(name).check_same(100, {"lds_staged": 1}, form)


# ---- row_occupancy 0: the occ == nullptr path of the rows kernels ---------------------------------------------------------
@pytest.mark.parametrize("name,S,form", [("A", 100, "rows_tiled"), ("B", 100, "rows_tiled"), ("E", 100, "rows_tiled"),
                                         ("A", 40, "rows_linear"), ("B", 40, "rows_linear")])
def test_row_occupancy_off(cases, name, S, form):
    """40 scans: beam slices on the linear planes (slices > 1), and the fine pass behind them (k_resp_rows<1,4>)."""
    cases(name).check_same(S, {"row_occupancy": 0}, form, fine=(S == 40))


# ---- collect_stats: the instrumented twins and their counters ---------------------------------------------------------------
def _read_counters(gm):
    out = (ctypes.c_uint64 * 4)()
    gm.ctx.check(gm.L.lslam_matcher_read_stats(gm.h, out))
    return [int(v) for v in out]


def _expect_counters(stats, counts, passes, pruned=True):
    """stats = ScanMatcher.read_stats() after `passes` instrumented passes over the scans counted in `counts`."""
    tot = {k: int(v.sum()) for k, v in counts.items()}
    assert 0 < tot["rows_nz"] < tot["rows"] and 0 < tot["pairs_nz"] < tot["pairs"]  # the brackets below are not vacuous
    assert stats["rows_in_range"] == passes * tot["rows"]
    assert stats["beam_angles"] == passes * tot["pairs"]
    if pruned:  # a bit of the bitmap covers a window of bytes from the row's start: it may keep a zero row, never drop a non-zero one
        assert passes * tot["rows_nz"] <= stats["rows_live"] <= stats["rows_in_range"]
        assert passes * tot["pairs_nz"] <= stats["beam_angles_queued"] <= passes * tot["pairs_in"] <= stats["beam_angles"]
        assert stats["rows_live"] < stats["rows_in_range"]  # and it does prune
    else:
        assert stats["rows_live"] == stats["rows_in_range"]
        assert stats["beam_angles_queued"] == passes * tot["pairs_in"]
    # per (scan, beam) flags, OR-ed over angles and passes
    assert stats["beams_readable"] == tot["beams"]
    assert tot["beams_nz"] <= stats["beams_live_in_some_angle"] <= stats["beams_readable"]


@pytest.mark.parametrize("name,S,opts,form", [
    ("A", 100, {}, "rows_stats_tiled"), ("B", 100, {}, "rows_stats_tiled"),
    ("A", 40, {}, "rows_stats_linear"), ("B", 40, {}, "rows_stats_linear"),
    ("A", 100, {"lds_staged": 1}, "rows_stats_lds_staged"), ("A", 40, {"row_occupancy": 0}, "rows_stats_linear"),
    ("D0", 40, {"row_occupancy": 0}, "rows_stats_linear")])
def test_collect_stats(cases, name, S, opts, form):
    """A's and B's lasers read up to 60 m: some of their beams end beyond the grid's last row, so their batches also count
    rows outside the index range; D0's beams all stay inside it, and without pruning every readable pair is queued."""
    c = cases(name)
    gm = c.gm
    sums, recs = c.default(S)
    counts = c.cpu_counts(S)
    if name == "D0":
        assert (counts["pairs_in"] == counts["pairs"]).all() and (counts["rows"] == c.nx * counts["pairs"]).all()
    else:
        assert counts["rows"].sum() < c.nx * counts["pairs"].sum() // (-(-c.nx // c.block_rows))
    assert np.array_equal(c.cpu_sums(0), c.oracle(0)[0])  # the CPU count reads the oracle's rows
    pruned = opts.get("row_occupancy", 1) == 1
    c.scrub(S)
    before = gm.coarse_form_launches()
    try:
        for k, v in opts.items():
            gm.set_option(k, v)
        gm.set_option("collect_stats", 1)
        assert _read_counters(gm) == [0, 0, 0, 0]
        got = gm.coarse_sums_batch(c.ranges[:S], c.poses[:S])       # one instrumented pass
        once = gm.read_stats()
        assert got.tobytes() == sums.tobytes()
        _expect_counters(once, counts, 1, pruned)
        got = gm.match_batch(c.ranges[:S], c.poses[:S])             # the same pass again: the counters accumulate
        twice = gm.read_stats()
        assert got.tobytes() == recs.tobytes()
        _expect_counters(twice, counts, 2, pruned)
        for k in ("rows_in_range", "rows_live", "beam_angles", "beam_angles_queued"):
            assert twice[k] == 2 * once[k], k
        for k in ("beams_readable", "beams_live_in_some_angle"):
            assert twice[k] == once[k], k
        if "lds_staged" in opts:
            assert once["lds_drains_staged"] + once["lds_drains_global"] > 0
        else:
            assert once["lds_drains_staged"] == once["lds_drains_global"] == 0
        gm.set_option("collect_stats", 0)   # off and on again clears them
        gm.set_option("collect_stats", 1)
        assert _read_counters(gm) == [0, 0, 0, 0]
    finally:
        gm.set_option("collect_stats", 0)
        for k in opts:
            gm.set_option(k, DEFAULTS[k])
    after = gm.coarse_form_launches()
    assert {k: after[k] - before[k] for k in COARSE_FORMS if after[k] != before[k]} == {form: 2}


def test_stats_carry_over_a_larger_batch(cases):
    """40 scans (linear twin), then 100 (tiled twin): the second batch outgrows the per-(scan, beam) flag words, which are
    reallocated -- the four counters collected so far must survive that."""
    c = cases("A")
    gm = c.gm
    counts = c.cpu_counts(100)
    head = {k: v[:40] for k, v in counts.items()}
    try:
        gm.set_option("collect_stats", 1)
        gm.match_batch(c.ranges[:40], c.poses[:40])
        small = gm.read_stats()
        _expect_counters(small, head, 1)
        gm.match_batch(c.ranges, c.poses)
        both = gm.read_stats()
    finally:
        gm.set_option("collect_stats", 0)
    assert both["rows_in_range"] == int(head["rows"].sum() + counts["rows"].sum())
    assert both["beam_angles"] == int(head["pairs"].sum() + counts["pairs"].sum())
    assert both["rows_live"] >= small["rows_live"] + int(counts["rows_nz"].sum())
    assert both["rows_live"] <= both["rows_in_range"]
    assert small["beam_angles_queued"] + int(counts["pairs_nz"].sum()) <= both["beam_angles_queued"]
    assert both["beam_angles_queued"] <= int(head["pairs_in"].sum() + counts["pairs_in"].sum())
    assert both["beams_readable"] == int(counts["beams"].sum())  # the flags are those of the batch that sized them


# ---- option hygiene ---------------------------------------------------------------------------------------------------------
def test_option_values(cases):
    gm = cases("A").gm
    for name, values in (("rows_waves", (2, 4, 8, 1)), ("lds_staged", (1, 0)), ("collect_stats", (1, 0)),
                         ("row_occupancy", (0, 1))):
        for v in values:
            gm.set_option(name, v)
            assert gm.get_option(name) == v
        assert gm.get_option(name) == DEFAULTS[name]
    gm.set_option("rows_waves", 4)
    try:
        for bad in (0, 3, 16):
            with pytest.raises(api.LslamError) as e:
                gm.set_option("rows_waves", bad)
            assert e.value.code == -1  # LSLAM_ERR_INVALID_ARGUMENT
            assert gm.get_option("rows_waves") == 4
    finally:
        gm.set_option("rows_waves", 1)


def test_untouched_matcher_runs_no_optional_form(ctx, cases):
    """A matcher whose options were never set: 100 scans through the tiled one-wave kernel, 40 through beam slices on the
    linear planes, each with one fine pass behind it -- and nothing through a form only an option selects."""
    c = cases("A")
    gm = api.ScanMatcher(ctx, api.baseline_config(), c.gm.laser)
    gi = c.port.grid_info()
    gm.set_grid(c.port.grid(), gi["offset"])
    assert not any(gm.coarse_form_launches().values())
    big = gm.match_batch(c.ranges, c.poses)
    launches = gm.coarse_form_launches()
    assert {k: v for k, v in launches.items() if v and k in COARSE_FORMS} == {"rows_tiled": 1}
    small = gm.match_batch(c.ranges[:40], c.poses[:40])
    launches = gm.coarse_form_launches()
    assert {k: v for k, v in launches.items() if v and k in COARSE_FORMS} == {"rows_tiled": 1, "rows_linear": 1}
    assert launches["fine_rows"] + launches["fine_tile3"] == 2
    assert set(launches) == set(api.COARSE_FORMS) and not any(launches[k] for k in OPTIONAL_FORMS)
    assert big.tobytes() == c.default(100)[1].tobytes() and small.tobytes() == c.default(40)[1].tobytes()
    gm.close()


def test_rows_waves_switched_between_pipelined_steps(ctx, cases):
    """Two pipelined steps (pipeline_depth 2) of the same batch, rows_waves switched from 1 to 4 between them: the first goes
    out through the one-wave kernel, the second through k_resp_rows_mw<3,11,4>, both give the records of the plain run."""
    c = cases("A")
    gm = c.gm
    S, n = 100, c.ranges.shape[1]
    want = c.default(S)[1]
    d_r, d_p = ctx.alloc(c.ranges.nbytes), ctx.alloc(S * 24)
    d_o = [ctx.alloc(S * 112), ctx.alloc(S * 112)]
    ctx.upload(d_r, c.ranges)
    ctx.upload(d_p, c.poses)
    ctx.synchronize()
    c.scrub(S)
    before, steps = gm.coarse_form_launches(), gm.pipelined_steps
    try:
        gm.set_option("pipeline_depth", 2)
        gm.match_batch_dev(S, d_r, n, d_p, d_o[0], dtype="f64")
        gm.set_option("rows_waves", 4)
        gm.match_batch_dev(S, d_r, n, d_p, d_o[1], dtype="f64")
        ctx.synchronize()
        assert gm.pipelined_steps == steps + 2
        for d in d_o:
            out = np.zeros(S, dtype=api.RESULT_DTYPE)
            ctx.download(d, out)
            assert out.tobytes() == want.tobytes()
    finally:
        gm.set_option("rows_waves", 1)
        gm.set_option("pipeline_depth", 1)
        for p in [d_r, d_p] + d_o:
            ctx.free(p)
    after = gm.coarse_form_launches()
    assert {k: after[k] - before[k] for k in COARSE_FORMS if after[k] != before[k]} == {"rows_tiled": 1, "rows_multiwave": 1}
