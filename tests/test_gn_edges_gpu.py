"""Every device form of the Gauss-Newton matcher (csrc/logodds_map.hip: ordered k_gn_match, k_gn_match_reg at 256 / 512 / 1024
threads, k_gn_match_fast with its points in LDS and in memory, k_gn_match_batch and its ordered twin, and the resident
container's launch path) on the scenarios of tests/gn_edge_cases.py: non-square and odd-sized maps with hundreds of points
outside, 1 and 5 levels, zero Hessians (bit for bit), a written border band probed at exactly 0.0 / -0.0 / lim /
nextafter(lim), and a clamped angular step.  The reference is the CPU restatement of the reference's matcher
(oracle PortHector.match_data); tests/test_gn_edges_oracle.py checks, without a GPU, that each scenario is what it claims
to be and well-posed for that reference.

Bounds, the project's own: pose within 1e-4 of the oracle, H within 1e-2 (parallel sums) / 1e-3 (ordered) of max(1, |H|max),
parallel against ordered within 5e-5.  Every test prints its worst differences (pytest -s)."""
import numpy as np
import pytest

from lslam_amd import api

import gn_edge_cases as E

pytestmark = pytest.mark.gpu
f32 = np.float32
ZERO9 = np.zeros(9, f32).tobytes()
SCAN_FORMS = ["ordered", "reg512", "reg256", "reg1024"]
ALL_FORMS = SCAN_FORMS + ["fast-lds", "fast-mem"]


class Rig:
    """One case: oracle levels and device maps built from the same scans, planes byte-equal on every level before any match."""

    def __init__(self, ctx, po, case, build=True):
        self.po, self.case = po, case
        self.cpus = E.oracle_levels(po, case, build)
        with pytest.MonkeyPatch.context() as mp:
            self.dev = E.DeviceMaps(ctx, api, mp, case, build)
        self.dev.assert_planes_equal(self.cpus)
        self._oracle, self._ordered = {}, {}

    def oracle(self, key, pts, begin):
        if key not in self._oracle:
            self._oracle[key] = self.po.PortHector.match_data(self.cpus, pts, begin)
        return self._oracle[key]

    def ordered(self, key, pts, begin):
        if key not in self._ordered:
            self._ordered[key] = self.dev.match("ordered", pts, begin)
        return self._ordered[key]

    def hold(self, tag, key, pts, begin, pose, H, ordered):
        """The bounds of the module docstring for one result; prints what it found first."""
        p_o, H_o = self.oracle(key, pts, begin)
        dp, dH = E.diffs(pose, H, p_o, H_o)
        line = "%s: |pose - oracle| = %.3g, |H - oracle| rel = %.3g" % (tag, dp, dH)
        dpo = None
        if not ordered and len(pts) <= E.ORDERED_MAX:
            dpo, dHo = E.diffs(pose, H, *self.ordered(key, pts, begin))
            line += ", |pose - ordered| = %.3g, |H - ordered| rel = %.3g" % (dpo, dHo)
        print(line)
        assert np.isfinite(pose).all() and np.isfinite(H).all(), tag
        assert dp <= E.POSE_TOL, (tag, pose, p_o)
        assert dH <= (E.H_TOL_ORDERED if ordered else E.H_TOL_PARALLEL), tag
        if dpo is not None:
            assert dpo <= E.PAR_VS_ORDERED_TOL and dHo <= E.H_TOL_PARALLEL, tag

    def hold_forms(self, tag, forms, conts, begins):
        for form in forms:
            k = E.FORM_CONTAINER[form]
            pose, H = self.dev.match(form, conts[k], begins[k])
            self.hold("%s %s" % (tag, form), k, conts[k], begins[k], pose, H, form == "ordered")


@pytest.fixture(scope="module", params=E.GEOMETRY_IDS)
def geo(request, ctx, oracle_lib):
    return request.param, Rig(ctx, oracle_lib, E.geometry_case(request.param))


@pytest.mark.parametrize("form", ALL_FORMS)
def test_geometry_single_call(geo, form):
    """a. One query, >= 100 of its points outside level 0, through every single-call form."""
    name, rig = geo
    rig.hold_forms(name, [form], rig.case.containers, rig.case.begin)


def test_geometry_resident_container(geo):
    """a. lslam_map_set_scan -> lslam_map_match_container: the container the device projects is the host's, bit for bit;
    the match is held to the oracle on that container."""
    name, rig = geo
    pts, pose, H = rig.dev.match_resident(api, rig.case.ranges, rig.case.begin["resident"])
    assert pts.tobytes() == rig.case.containers["resident"].tobytes()
    rig.hold(name + " resident", "resident", pts, rig.case.begin["resident"], pose, H, False)


@pytest.mark.parametrize("ordered", [False, True], ids=["batch", "batch-ordered"])
def test_geometry_batch(geo, ordered):
    """a. The scenario's containers in one batch, waves with outside points beside in-map neighbours in the same block.  The
    scenario's entries are held to the oracle; the neighbours (too few points for a tolerance) to themselves: what they
    give in a batch of their own, bit for bit."""
    name, rig = geo
    c, b = rig.case.containers, rig.case.begin
    near2 = (b["near"] + np.array([0.01, 0.02, -0.01], f32)).astype(f32)
    entries = [(c["near"], b["near"]), (c["scan"], b["scan"]), (c["near"], near2), (c["lds"], b["lds"]),
               (c["scan"], b["scan"]), (c["near"], b["near"])]
    keys = [None, "scan", None, "lds", "scan", None]
    if not ordered:  # (the ordered kernel refuses 7200 points)
        entries.append((c["mem"], b["mem"]))
        keys.append("mem")
    poses, Hs = rig.dev.match_batch(entries, ordered)
    for i, k in enumerate(keys):
        if k:
            rig.hold("%s %s[%d] %s" % (name, "batch-ordered" if ordered else "batch", i, k), k, *entries[i], poses[i], Hs[i], ordered)
    alone = [i for i, k in enumerate(keys) if k is None]
    p_a, H_a = rig.dev.match_batch([entries[i] for i in alone], ordered)
    for j, i in enumerate(alone):
        assert E.words(p_a[j], H_a[j]) == E.words(poses[i], Hs[i]), i


# ---- b. zero Hessians, bit for bit -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zero(ctx, oracle_lib):
    case = E.geometry_case(E.ZERO_GEOMETRY.name)
    return {True: Rig(ctx, oracle_lib, case), False: Rig(ctx, oracle_lib, case, build=False)}


def zero_oracle(rig, pts, begin):
    p, H = rig.po.PortHector.match_data(rig.cpus, pts, begin)
    assert H.tobytes() == ZERO9 and p.tobytes() != np.asarray(begin, f32).tobytes()
    return E.words(p, H)


@pytest.mark.parametrize("kind", ["untouched", "outside"])
@pytest.mark.parametrize("form", ALL_FORMS + ["batch", "batch-ordered", "resident"])
def test_zero_hessian_bit_for_bit(zero, kind, form):
    """b. An untouched map, and a built map with every point outside every level: no sum takes part, so every form returns
    the oracle's 3 pose floats (which are not the start pose's) and nine +0.0 words, byte for byte."""
    tag = {"fast-lds": "lds", "fast-mem": "mem"}.get(form, "scan")
    built, pts, begin = E.zero_cases()["%s-%s" % (kind, tag)]
    rig = zero[built]
    if form == "resident":
        pts, pose, H = rig.dev.match_resident(api, rig.case.ranges, begin)
        assert len(pts) > 700
    elif form.startswith("batch"):
        poses, Hs = rig.dev.match_batch([(pts, begin)], form == "batch-ordered")
        pose, H = poses[0], Hs[0]
    else:
        pose, H = rig.dev.match(form, pts, begin)
    assert E.words(pose, H) == zero_oracle(rig, pts, begin), (form, kind, pose, H)


@pytest.mark.parametrize("ordered", [False, True], ids=["batch", "batch-ordered"])
def test_zero_hessian_entry_beside_ordinary_ones(zero, ordered):
    """b. Containers wholly outside every level at entries 1 and 6 of a batch of 7 (the second wave of the first block, the
    third of the second) among ordinary ones: the outside entries return the oracle's 12 floats byte for byte, the
    neighbours what they return without them."""
    rig = zero[True]
    c, b = rig.case.containers, rig.case.begin
    _, far_pts, far = E.zero_cases()["outside-scan"]
    _, far_lds, _ = E.zero_cases()["outside-lds"]
    inside = [(c["scan"], b["scan"]), (c["near"], b["near"]), (c["lds"], b["lds"]), (c["scan"], b["scan"]), (c["near"], b["near"])]
    entries = inside[:1] + [(far_pts, far)] + inside[1:] + [(far_lds, far)]
    spots = (1, 6)
    poses, Hs = rig.dev.match_batch(entries, ordered)
    for i in spots:
        assert E.words(poses[i], Hs[i]) == zero_oracle(rig, *entries[i]), (i, poses[i], Hs[i])
    p_in, H_in = rig.dev.match_batch(inside, ordered)
    rest = [i for i in range(len(entries)) if i not in spots]
    for j, i in enumerate(rest):
        assert E.words(p_in[j], H_in[j]) == E.words(poses[i], Hs[i]), i
    rig.hold("zero-batch neighbour", "scan", *inside[0], poses[0], Hs[0], ordered)


# ---- c. the boundary band --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def band(ctx, oracle_lib):
    return Rig(ctx, oracle_lib, E.band_case()[0])


@pytest.mark.parametrize("form", ALL_FORMS + ["batch", "batch-ordered"])
def test_boundary_band(band, form):
    """c. A 200 x 120 single-level map whose border band is written (planes byte-equal), a container straddling all four
    edges with points at exactly +0.0, -0.0, lim and nextafter(lim, +inf) in x and y at the start pose: every form within
    the bounds of (a) of the oracle, every returned float finite."""
    c, b = band.case.containers, band.case.begin
    if form.startswith("batch"):
        ordered = form == "batch-ordered"
        entries = [(c["scan"], b["scan"]), (c["lds"], b["lds"])] + ([] if ordered else [(c["mem"], b["mem"])])
        poses, Hs = band.dev.match_batch(entries, ordered)
        for i, k in enumerate(["scan", "lds", "mem"][: len(entries)]):
            band.hold("band %s[%d]" % (form, i), k, *entries[i], poses[i], Hs[i], ordered)
    else:
        band.hold_forms("band", [form], c, b)


# ---- d. the clamp of the angular step --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clamp(ctx, oracle_lib):
    return Rig(ctx, oracle_lib, E.clamp_case())


@pytest.mark.parametrize("form", SCAN_FORMS + ["batch", "batch-ordered"])
def test_clamped_angular_step(clamp, form):
    """d. A start pose 0.35 rad off whose first step on the coarsest level is clamped to 0.2 rad (checked on the oracle in
    test_gn_edges_oracle.test_clamp_is_reached): every form within the bounds of (a), and back at the truth."""
    pts, begin = clamp.case.containers["scan"], clamp.case.begin["scan"]
    if form.startswith("batch"):
        ordered = form == "batch-ordered"
        poses, Hs = clamp.dev.match_batch([(pts, begin), (pts, begin)], ordered)
        assert E.words(poses[0], Hs[0]) == E.words(poses[1], Hs[1])
        pose, H = poses[0], Hs[0]
    else:
        ordered = form == "ordered"
        pose, H = clamp.dev.match(form, pts, begin)
    clamp.hold("clamp " + form, "scan", pts, begin, pose, H, ordered)
    assert np.hypot(pose[0], pose[1]) < E.CONVERGES and abs(pose[2]) < 1e-3, pose
