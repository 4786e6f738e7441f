"""The Hector fleet (lslam_hector_fleet_*, api.HectorFleet; csrc/logodds_map.hip: k_hf_project, k_hf_match_*, k_hf_mark,
k_hf_apply) on the fleets of tests/hector_fleet_cases.py.  The yardstick everywhere is BIT EQUALITY with the members run alone
through lslam_hector_process_many[_points] on fresh maps and processors of the same construction -- the path
tests/test_hector_stream_gpu.py holds to the reference's own processor -- so no tolerance appears here.

The library has no reader for the cached container (MapRepMultiMap::dataContainers), only its size: it is compared through
what it is for -- one more host-driven updateByScan at a fixed pose, whose levels above 0 are fed from it, then the planes
as bytes (`probe`)."""
import numpy as np
import pytest

from lslam_amd import api

import gn_edge_cases as E
import hector_fleet_cases as F
import hector_stream_cases as S

pytestmark = pytest.mark.gpu
f32 = np.float32
PROBE_POSE = np.array([0.3, -0.2, 0.1], f32)


def make(ctx, mb):
    m = S.device_map(api, ctx, mb.sc)
    h = api.HectorProcessor(m)
    h.set_update_thresholds(mb.sc.min_dist, mb.sc.min_angle)
    return m, h


def close(pairs):
    for m, _ in pairs:
        m.close()  # (closes its processors, and those their fleets)


def solo_call(fleet, r, h, lo, hi, form):
    """Member r's own call over its active scans of steps [lo, hi) -> records (None: it has none)."""
    mb = fleet.members[r]
    idx = [k for k in range(lo, hi) if fleet.active[k, r]]
    if not idx:
        return None
    hints = None if mb.hints is None else np.asarray(mb.hints)[idx]
    flags = [1] * len(idx) if mb.no_match else None
    if form == "points":
        return h.process_many_points([mb.containers[k] for k in idx], hints, flags)
    return h.process_many(mb.ranges[idx], api.hector_scan(mb.sc.laser), hints, flags)


def fleet_call(fleet, fl, lo, hi, form):
    """Steps [lo, hi) of the scenario through the fleet -> HECTOR_RECORD[hi - lo, R]."""
    mbs = fleet.members
    act = None if fleet.active[lo:hi].all() else fleet.active[lo:hi]
    hints = None if mbs[0].hints is None else np.stack([[mb.hints[k] for mb in mbs] for k in range(lo, hi)])
    flags = 1 if mbs[0].no_match else None
    if form == "points":
        return fl.process_many_points([[mb.containers[k] for mb in mbs] for k in range(lo, hi)], hints, flags, act)
    ranges = np.stack([[mb.ranges[k] for mb in mbs] for k in range(lo, hi)])
    return fl.process_many(ranges, api.hector_scan(mbs[0].sc.laser), hints, flags, act)


def run_solo(ctx, fleet, form, calls=None):
    pairs, recs = [], []
    for r, mb in enumerate(fleet.members):
        m, h = make(ctx, mb)
        got = [solo_call(fleet, r, h, lo, hi, form) for lo, hi in (calls or fleet.calls)]
        pairs.append((m, h))
        recs.append(np.concatenate([g for g in got if g is not None]))
    return pairs, recs


def run_fleet(ctx, fleet, form, calls=None):
    pairs = [make(ctx, mb) for mb in fleet.members]
    fl = api.HectorFleet([h for _, h in pairs])
    assert fl.size == len(pairs)
    rec = np.concatenate([fleet_call(fleet, fl, lo, hi, form) for lo, hi in (calls or fleet.calls)])
    return pairs, fl, rec


def planes(m):
    return [m.logodds(lv).tobytes() for lv in range(m.levels)]


def snapshot(m, h, resident=False):
    """Everything of a member the equivalence contract names, as bytes; the probe comes last (it changes the map)."""
    st = h.stats()
    s = {"state": b"".join(np.ascontiguousarray(a).tobytes() for a in h.state()), "planes": planes(m),
         "cached_points": m.cached_points(), "counters": (st["scans"], st["map_updates"])}
    if resident:
        pts, origo = m.container()
        s["resident"] = (pts.tobytes(), np.asarray(origo, f32).tobytes())
    sc_pts = S.edges(3).containers[0]
    m.updateByScan(sc_pts, (0.0, 0.0), PROBE_POSE)
    s["probe"] = planes(m)
    return s


def hold_to_solo(fleet, rec, fleet_pairs, solo_pairs, solo_recs, resident=False):
    assert rec.shape == fleet.active.shape
    for r in range(len(fleet.members)):
        mine = rec[:, r]
        assert np.ascontiguousarray(mine[fleet.active[:, r]]).tobytes() == solo_recs[r].tobytes(), r
        idle = mine[~fleet.active[:, r]]
        assert (idle["n_points"] == -1).all()
        blank = idle.copy()
        blank["n_points"] = 0
        assert not np.frombuffer(blank.tobytes(), np.uint8).any()  # all zero but the count
        a, b = snapshot(*fleet_pairs[r], resident=resident), snapshot(*solo_pairs[r], resident=resident)
        for key in a:
            assert a[key] == b[key], (r, key)
        assert any(np.frombuffer(p, f32).any() for p in a["planes"]), r  # (the scenario did map something)


# ---- 1. heterogeneous chain, container form ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hetero_solo(ctx):
    fleet = F.hetero()
    pairs, recs = run_solo(ctx, fleet, "points")
    snaps = [snapshot(m, h) for m, h in pairs]
    close(pairs)
    return fleet, recs, snaps


def hold_hetero(fleet, rec, pairs, recs, snaps):
    for r in range(3):
        assert np.ascontiguousarray(rec[:, r]).tobytes() == recs[r].tobytes(), r
        a = snapshot(*pairs[r])
        for key in a:
            assert a[key] == snaps[r][key], (r, key)


def test_heterogeneous_chain(ctx, hetero_solo):
    """1. 256^2 x 3 levels, 256^2 x 1 level and 1024^2 x 3 levels in one call of 12 steps: records, state, every plane, the
    cached container, the members' counters -- and 3 launches per step, one wait."""
    fleet, recs, snaps = hetero_solo
    pairs, fl, rec = run_fleet(ctx, fleet, "points")
    st = fl.stats()
    print("fleet stats", st, "member stats", [h.stats() for _, h in pairs])
    assert (st["steps"], st["scans"], st["calls"], st["host_syncs"], st["launches"]) == (12, 36, 1, 1, 3 * 12)
    assert st["map_updates"] == int((rec["updated"] != 0).sum()) > 3
    for _, h in pairs:  # the fleet counts calls and waits, not the member
        assert (h.stats()["calls"], h.stats()["host_syncs"]) == (0, 0)
    assert rec["n_points"][:, 2].max() > 700 and rec["n_points"][S.EDGE_EMPTY, 0] == 0
    hold_hetero(fleet, rec, pairs, recs, snaps)
    close(pairs)


# ---- 2. ranges form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 1])
def test_ranges_form(ctx, R):
    """2. edges(3)'s readings, member r's rolled by r scans: equal to process_many alone, the resident container of every
    member's map included; 4 launches per step; a second call of the same geometry waits once."""
    fleet = F.rolled(R)
    solo_pairs, solo_recs = run_solo(ctx, fleet, "ranges")
    pairs, fl, rec = run_fleet(ctx, fleet, "ranges")
    st = fl.stats()
    print("fleet stats", st)
    assert st["launches"] == 4 * fleet.n_steps and st["calls"] == 1 and 1 <= st["host_syncs"] <= 2
    again = fleet_call(fleet, fl, 0, 2, "ranges")
    st2 = fl.stats()
    assert st2["host_syncs"] - st["host_syncs"] == 1 and st2["launches"] - st["launches"] == 4 * 2
    for r, (_, h) in enumerate(solo_pairs):
        assert solo_call(fleet, r, h, 0, 2, "ranges").tobytes() == np.ascontiguousarray(again[:, r]).tobytes()
    hold_to_solo(fleet, rec, pairs, solo_pairs, solo_recs, resident=True)
    close(pairs + solo_pairs)


# ---- 3. mapping only ----------------------------------------------------------------------------------------------------------
def test_mapping_only(ctx):
    """3. mapping25 with hints and map_without_matching (the geometry's rotation is the host's cosf / sinf of the hint), member
    r starting r scans in: planes bit-equal to the members alone, every record its hint."""
    fleet = F.mapping()
    solo_pairs, solo_recs = run_solo(ctx, fleet, "points")
    pairs, fl, rec = run_fleet(ctx, fleet, "points")
    assert (rec["updated"] == 1).all()
    for r, mb in enumerate(fleet.members):
        assert np.ascontiguousarray(rec["pose"][:, r]).tobytes() == np.ascontiguousarray(mb.hints, f32).tobytes()
    assert planes(pairs[0][0])[0] != planes(pairs[1][0])[0]  # (the members did map different scans)
    hold_to_solo(fleet, rec, pairs, solo_pairs, solo_recs)
    close(pairs + solo_pairs)


# ---- 4. ragged ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["points", "ranges"])
def test_ragged(ctx, form):
    """4. Five members under the mask of the cases module, in two calls: each member equals its active column run alone; the
    step nobody takes changes no byte; the member that sits the second call out keeps state, planes and counters."""
    fleet = F.ragged()
    solo_pairs, solo_recs = run_solo(ctx, fleet, form)
    pairs = [make(ctx, mb) for mb in fleet.members]
    fl = api.HectorFleet([h for _, h in pairs])
    (lo0, hi0), (lo1, hi1) = fleet.calls
    k = F.RAGGED_EMPTY_STEP
    assert lo0 < k < hi0
    recs = [fleet_call(fleet, fl, lo0, k, form)]
    before = [(planes(m), h.state(), h.stats(), m.cached_points(), m.container()[0].tobytes()) for m, h in pairs]
    recs.append(fleet_call(fleet, fl, k, k + 1, form))  # the step nobody takes, as a call of its own
    after = [(planes(m), h.state(), h.stats(), m.cached_points(), m.container()[0].tobytes()) for m, h in pairs]
    for b, a in zip(before, after):
        assert b[0] == a[0] and all(x.tobytes() == y.tobytes() for x, y in zip(b[1], a[1])) and b[2:] == a[2:]
    recs.append(fleet_call(fleet, fl, k + 1, hi0, form))
    idle, _ = F.RAGGED_IDLE
    m_i, h_i = pairs[idle]
    before = (planes(m_i), [x.tobytes() for x in h_i.state()], h_i.stats(), m_i.cached_points(), m_i.container()[0].tobytes())
    recs.append(fleet_call(fleet, fl, lo1, hi1, form))
    after = (planes(m_i), [x.tobytes() for x in h_i.state()], h_i.stats(), m_i.cached_points(), m_i.container()[0].tobytes())
    assert before == after
    rec = np.concatenate(recs)
    assert (rec["n_points"][k] == -1).all()
    assert fl.stats()["calls"] == 4 and fl.stats()["scans"] == int(fleet.active.sum())
    hold_to_solo(fleet, rec, pairs, solo_pairs, solo_recs, resident=form == "ranges")
    close(pairs + solo_pairs)


# ---- 5. chunking and interop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [[(k, k + 1) for k in range(12)], [(0, 5), (5, 12)]], ids=["12x1", "5+7"])
def test_chunking_changes_nothing(ctx, hetero_solo, calls):
    """5a. The heterogeneous chain as 12 calls of one step and as 5 + 7: bit-identical to one call (which test 1 holds to the
    members alone)."""
    fleet, recs, snaps = hetero_solo
    pairs, fl, rec = run_fleet(ctx, fleet, "points", calls)
    st = fl.stats()
    assert (st["calls"], st["host_syncs"], st["launches"]) == (len(calls), len(calls), 36)
    hold_hetero(fleet, rec, pairs, recs, snaps)
    close(pairs)


def test_members_stay_usable_between_fleet_calls(ctx, hetero_solo):
    """5b. Steps 0-5 by the fleet, 6-8 by each member's own process_many_points, 9-11 by the fleet again."""
    fleet, recs, snaps = hetero_solo
    pairs = [make(ctx, mb) for mb in fleet.members]
    fl = api.HectorFleet([h for _, h in pairs])
    first = fleet_call(fleet, fl, 0, 6, "points")
    own = np.stack([solo_call(fleet, r, h, 6, 9, "points") for r, (_, h) in enumerate(pairs)], axis=1)
    last = fleet_call(fleet, fl, 9, 12, "points")
    rec = np.concatenate([first, own, last])
    for r in range(3):
        assert np.ascontiguousarray(rec[:, r]).tobytes() == recs[r].tobytes(), r
        a = snapshot(*pairs[r])
        for key in a:
            if key != "counters":
                assert a[key] == snaps[r][key], (r, key)
        assert pairs[r][1].stats()["scans"] == 12 and pairs[r][1].stats()["calls"] == 1
    close(pairs)


def test_a_host_driven_match_data_between_two_calls_is_seen(ctx):
    """5c. lslam_map_match_data on one member's map between two fleet calls replaces its cached container; the next call's
    scan, taken without matching, feeds the levels above 0 from it -- exactly as the member alone does."""
    fleet = F.rolled(2)
    other = S.edges(3).containers[7]  # 63 points: not what any member cached last
    hint = np.array([0.05, 0.02, 0.01], f32)

    def run(through_fleet):
        pairs = [make(ctx, mb) for mb in fleet.members]
        fl = api.HectorFleet([h for _, h in pairs])
        if through_fleet:
            fleet_call(fleet, fl, 0, 6, "points")
        else:
            for r, (_, h) in enumerate(pairs):
                solo_call(fleet, r, h, 0, 6, "points")
        m0 = pairs[0][0]
        upper = planes(m0)[1:]
        m0.matchData(pairs[0][1].state()[0], other)
        assert m0.cached_points() == len(other)
        conts = [mb.containers[6] for mb in fleet.members]
        if through_fleet:
            rec = fl.process_many_points([conts], np.stack([[hint, hint]]), 1)[0]
        else:
            rec = np.concatenate([h.process_many_points([c], [hint], [1]) for (_, h), c in zip(pairs, conts)])
        assert (rec["updated"] == 1).all() and m0.cached_points() == len(other)
        out = [planes(m) for m, _ in pairs]
        assert out[0][1:] != upper  # (the levels above 0 were updated, from the container matchData cached)
        close(pairs)
        return rec.tobytes(), out

    assert run(True) == run(False)


# ---- 6. every matcher form ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gn_maps3(ctx):
    """Three equal sets of tests/gn_edge_cases.py's smallest map under each LSLAM_GN_THREADS: two for a fleet, one alone."""
    case = E.geometry_case("256x192")
    with pytest.MonkeyPatch.context() as mp:
        sets = [E.DeviceMaps(ctx, api, mp, case) for _ in range(3)]
    yield case, sets
    for dev in sets:
        for m in dev.maps.values():
            m.close()


@pytest.mark.parametrize("form", ["reg256", "reg512", "reg1024", "fast-lds", "fast-mem"])
def test_every_matcher_form(gn_maps3, form):
    """6. A fleet of two processors on two equal maps takes one step with the form's container and start pose; both records'
    12 pose / covariance words equal the processor alone on a third equal map.  (All three maps take the same update
    afterwards, so they stay equal for the next form.)"""
    case, sets = gn_maps3
    threads, _, (lo, hi) = E.SINGLE_FORMS[form]
    pts, begin = case.containers[E.FORM_CONTAINER[form]], case.begin[E.FORM_CONTAINER[form]]
    assert lo <= len(pts) <= hi and F.form_of(threads, len(pts)) == form
    hs = [api.HectorProcessor(dev.maps[threads]) for dev in sets]
    fl = api.HectorFleet(hs[:2])
    rec = fl.process_many_points([[pts, pts]], pose_hints=[[begin, begin]])[0]
    alone = hs[2].process_many_points([pts], pose_hints=[begin])[0]
    assert fl.stats()["launches"] == 3
    want = np.concatenate([alone["pose"].ravel(), alone["cov"].ravel()]).view(np.uint32)
    for r in range(2):
        assert rec[r]["n_points"] == len(pts)
        got = np.concatenate([rec[r]["pose"].ravel(), rec[r]["cov"].ravel()]).view(np.uint32)
        assert np.array_equal(got, want), (form, r, got, want)
    assert np.abs(alone["pose"] - np.asarray(begin, f32)).max() > 0  # (the match moved the pose: not a no-op)
    for h in hs:
        h.close()


# ---- 7. options and thresholds are the member's ------------------------------------------------------------------------------
def test_options_and_thresholds_are_the_members(ctx):
    """7. The two-scan chain of tests/test_hector_stream_gpu.py's gate test (a turn of 0.5 rad in place): the member with
    FABS_ANGLE_GATE and thresholds 0.04 / 0.13 updates twice, the member with the defaults once -- in one fleet."""
    sc = S.chain60()
    pts = sc.containers[0]
    c, s = np.cos(f32(0.5)), np.sin(f32(0.5))
    turned = np.ascontiguousarray(pts @ np.array([[c, -s], [s, c]], f32))
    hints = np.array([[0, 0, 0], [0, 0, 0.5]], f32)

    def members():
        pairs = []
        for fabs in (1, 0):
            m = S.device_map(api, ctx, sc)
            h = api.HectorProcessor(m)
            if fabs:
                h.set_option("fabs_angle_gate", 1)
                h.set_update_thresholds(0.04, 0.13)
            pairs.append((m, h))
        return pairs

    solo = members()
    want = [h.process_many_points([pts, turned], hints) for _, h in solo]
    pairs = members()
    fl = api.HectorFleet([h for _, h in pairs])
    rec = fl.process_many_points([[pts, pts], [turned, turned]], np.stack([hints, hints], axis=1))
    assert rec["updated"][:, 0].tolist() == [1, 1] and rec["updated"][:, 1].tolist() == [1, 0]
    for r in range(2):
        assert np.ascontiguousarray(rec[:, r]).tobytes() == want[r].tobytes()
        assert planes(pairs[r][0]) == planes(solo[r][0])
    close(pairs + solo)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, monkeypatch):
    """8. What a fleet cannot be made of, and what a call cannot take: the documented code, nothing enqueued (calls unchanged,
    no plane touched), and the fleet then takes a step normally."""
    sc = S.edges(3)
    mb = F.rolled(2).members
    pairs = [make(ctx, m) for m in mb]
    (m0, h0), (m1, h1) = pairs

    def refused(code, what):
        with pytest.raises(api.LslamError) as e:
            what()
        assert e.value.code == code, (e.value.code, str(e.value))

    refused(-1, lambda: api.HectorFleet([h0, h0]))                       # the same processor twice
    twin = api.HectorProcessor(m0)
    refused(-1, lambda: api.HectorFleet([h0, twin]))                     # two processors on one map
    twin.close()
    m1.set_option("ordered_sums", 1)
    refused(-8, lambda: api.HectorFleet([h0, h1]))                       # an ordered-sums map
    m1.set_option("ordered_sums", 0)
    deep = api.OccGridMap(ctx, 512, 512, S.CELL, S.offset(512), levels=9)
    hd = api.HectorProcessor(deep)
    refused(-8, lambda: api.HectorFleet([h0, hd]))                       # a pyramid deeper than the matcher's 8 levels
    monkeypatch.setenv("LSLAM_GN_THREADS", "256")
    other = S.device_map(api, ctx, sc)
    monkeypatch.delenv("LSLAM_GN_THREADS")
    ho = api.HectorProcessor(other)
    refused(-8, lambda: api.HectorFleet([h0, ho]))                       # maps created under different LSLAM_GN_THREADS

    fl = api.HectorFleet([h0, h1])
    scan = api.hector_scan(sc.laser)
    too_many = (1 << 16) + 1
    refused(-8, lambda: fl.process_many(np.full((1, 2, too_many), np.inf, f32), scan))
    refused(-8, lambda: fl.process_many_points([[np.zeros((too_many, 2), f32), sc.containers[0]]]))
    refused(-1, lambda: fl.process_many_points([[sc.containers[0], sc.containers[1]]], active=[[1, 0]]))  # not active, with points
    m1.set_option("ordered_sums", 1)                                     # ... set after the fleet was made
    refused(-8, lambda: fl.process_many_points([[sc.containers[0], sc.containers[1]]]))
    m1.set_option("ordered_sums", 0)
    st = fl.stats()
    assert st["calls"] == 0 and st["launches"] == 0 and st["host_syncs"] == 0
    for m, h in pairs:
        assert not any(np.frombuffer(p, f32).any() for p in planes(m)) and h.stats()["scans"] == 0
    rec = fl.process_many_points([[sc.containers[0], sc.containers[1]]])
    assert (rec["updated"] == 1).all() and fl.stats()["calls"] == 1
    assert all(np.frombuffer(planes(m)[0], f32).any() for m, _ in pairs)
    for m in (deep, other, m0, m1):
        m.close()
