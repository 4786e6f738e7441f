"""The Hector fleet's gated forms on the device: api.HectorFleet.process_many_clouds[_dev] (de-skewed clouds with a take word
per entry) and process_synced (R lesson5 nodes in front of R processors, the synchronisation of all of them in one launch per
kernel), on the fleets of tests/hector_fleet_sync_cases.py.

The yardstick everywhere is BIT EQUALITY with the members run alone through HectorProcessor.process_many_clouds /
process_synced on fresh maps, processors and nodes of the same construction -- the paths tests/test_hector_sync_gpu.py holds to
the reference -- so no tolerance appears here: the fleet's kernels run the device bodies of the single chain on the same
inputs.  Compared: records, msync records, hector_sync_cases.snapshot (every level's plane, state(), container(),
cached_points()), the members' scans / map_updates and the nodes' callbacks / corrected / refused.  Every test prints what it
measured (pytest -s)."""
import numpy as np
import pytest

from lslam_amd import api

import deskew_stream_cases as D
import hector_fleet_sync_cases as F
import hector_stream_cases as S
import hector_sync_cases as H

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = -1
S_LAUNCHES = 5  # rows, walk, windows, k_deskew_batch, blank
NODE_KEYS = ("callbacks", "corrected", "refused")


def make(ctx, mb):
    m = api.OccGridMap(ctx, mb.map_n, mb.map_n, S.CELL, S.offset(mb.map_n), levels=mb.levels)
    m.setUpdateFreeFactor(0.4)
    m.setUpdateOccupiedFactor(0.9)
    return m, D.processor(m)


def node(ctx, c):
    ms = api.MotionSync(ctx, c["use_imu"], c["use_odom"])
    H.push_all(ms, c)
    return ms


class Session:
    """Fresh maps, processors and nodes for every member of a fleet, and the fleet over them."""

    def __init__(self, ctx, name, nodes=True):
        self.name, self.mbs = name, F.members(name)
        self.cases = [H.case(mb.log) for mb in self.mbs]
        self.pairs = [make(ctx, mb) for mb in self.mbs]
        self.nodes = [node(ctx, c) for c in self.cases] if nodes else []
        self.scan = H.hector_scan(self.cases[0])
        self.laser = self.cases[0]["laser"]
        self.fleet = api.HectorFleet([h for _, h in self.pairs])

    def alone(self, lo, hi, hints=None, flags=None):
        """Every member's own process_synced over its callbacks of steps [lo, hi) -> [(rec, srec) or None] per member."""
        out = []
        for m, mb in enumerate(self.mbs):
            a, b = F.span(mb, lo, hi)
            if a == b:
                out.append(None)
                continue
            at = slice(mb.first + a, mb.first + b)
            r, t, ti, iseen, oseen = H.scan_args(self.cases[m], a, b)
            out.append(self.pairs[m][1].process_synced(
                self.nodes[m], self.laser, r, self.scan, t, ti, iseen, oseen,
                pose_hints=None if hints is None else hints[at, m], map_without_matching=None if flags is None else flags[at, m]))
        return out

    def together(self, lo, hi, hints=None, flags=None, **changed):
        """Steps [lo, hi) through the fleet -> (rec [n, R], srec [n, R])."""
        r, t, ti, iseen, oseen, act = F.step_arrays(self.name, lo, hi)
        a = {"syncs": self.nodes, "ranges": r, "stamps": t, "time_increments": ti, "imu_seen": iseen, "odom_seen": oseen}
        a.update(changed)
        return self.fleet.process_synced(a["syncs"], self.laser, a["ranges"], self.scan, a["stamps"], a["time_increments"],
                                         a["imu_seen"], a["odom_seen"], None if hints is None else hints[lo:hi],
                                         None if flags is None else flags[lo:hi], act)

    def state(self):
        """Per member: snapshot, the counters a scan moves, and the node's."""
        out = []
        for m, (mp, h) in enumerate(self.pairs):
            st = h.stats()
            ns = self.nodes[m].stats() if self.nodes else {}
            out.append((H.snapshot(mp, h), (st["scans"], st["map_updates"]), tuple(ns.get(k) for k in NODE_KEYS)))
        return out

    def close(self):
        for ms in self.nodes:
            ms.close()
        for mp, _ in self.pairs:
            mp.close()  # (closes its processors, and those their fleets)


def per_member(name, rec, lo=0, hi=None):
    """[n, R] of steps [lo, hi) -> per member the rows of its callbacks; every other row must be the not-taken one."""
    act = F.active(name)[lo:hi]
    out = []
    for m in range(act.shape[1]):
        out.append(np.ascontiguousarray(rec[act[:, m], m]))
        idle = rec[~act[:, m], m]
        if rec.dtype == api.HECTOR_RECORD:
            assert all(H.not_taken(r) for r in idle), m
        else:
            assert not np.frombuffer(np.ascontiguousarray(idle).tobytes(), np.uint8).any(), m  # msync records: all zero
    return out


def same(a, b, what=""):
    """two Session.state() lists, member by member and field by field"""
    assert len(a) == len(b)
    for m, ((sa, ca, na), (sb, cb, nb)) in enumerate(zip(a, b)):
        for k in sa:
            assert sa[k] == sb[k], (what, m, k)
        assert ca == cb, (what, m, ca, cb)
        assert na == nb, (what, m, na, nb)


_ALONE = {}


def alone_run(ctx, name, hints=None, flags=None, key=None):
    """The all-alone run of a fleet, once per session -> ([rec per member], [srec per member], state)."""
    key = (name, key)
    if key not in _ALONE:
        s = Session(ctx, name)
        got = s.alone(0, F.steps(name), hints, flags)
        _ALONE[key] = ([g[0] for g in got], [g[1] for g in got], s.state())
        s.close()
    return _ALONE[key]


def hold(name, rec, srec, state, want, lo=0, hi=None, what=""):
    recs, srecs = per_member(name, rec, lo, hi), per_member(name, srec, lo, hi)
    for m in range(len(recs)):
        assert recs[m].tobytes() == want[0][m].tobytes(), (what, m)
        assert srecs[m].tobytes() == want[1][m].tobytes(), (what, m)
    same(state, want[2], what)


# ---- 1, 2: clouds ---------------------------------------------------------------------------------------------------------
PATTERNS = ("mixed", "none", "first_not")  # one per member of ragged64


@pytest.fixture(scope="module")
def clouds(ctx):
    """ragged64: every member's clouds from its own MotionSync.scans, its take bytes, and its own process_many_clouds."""
    name = "ragged64"
    xyz, valid, take, recs = [], [], [], []
    s = Session(ctx, name)
    for m, mb in enumerate(s.mbs):
        x, v, srec = s.nodes[m].scans(s.laser, *H.scan_args(s.cases[m]))
        assert srec["status"].tolist() == H.STATUSES[mb.log]
        t = np.resize(np.array(H.TAKE_PATTERNS[PATTERNS[m]], bool), len(x))
        recs.append(s.pairs[m][1].process_many_clouds(x, s.scan, v, take=t))
        for a in (x, v, t):
            a.setflags(write=False)
        xyz.append(x)
        valid.append(v)
        take.append(t)
    s.nodes, nodes = [], s.nodes  # (the clouds' route has no node: state() compares the processors)
    out = {"xyz": xyz, "valid": valid, "take": take, "want": (recs, s.state()), "scan": s.scan,
           "X": F.spread(name, xyz), "V": F.spread(name, valid), "T": F.spread(name, take), "act": F.active(name)}
    for ms in nodes:
        ms.close()
    s.close()
    assert [int(t.sum()) for t in take] == [6, 0, 7] and all(r["n_points"].max() > 40 for r in (recs[0], recs[2]))
    return out


def hold_clouds(rec, state, clouds, what):
    got = per_member("ragged64", rec)
    for m in range(3):
        assert got[m].tobytes() == clouds["want"][0][m].tobytes(), (what, m)
        assert all(H.not_taken(r) for r in got[m][~clouds["take"][m]]), (what, m)
    same(state, clouds["want"][1], what)


def upload(ctx, arr):
    a = np.ascontiguousarray(arr)
    p = ctx.alloc(max(a.nbytes, 4))
    ctx.upload(p, a)
    return p


def test_cloud_form_equals_the_members_alone(ctx, clouds):
    """1. process_many_clouds on ragged64 == each member's own process_many_clouds; host take bytes mixed / none / first_not;
    the member of which nothing is taken keeps the snapshot of a fresh one; _dev at take stride 1 (words > 1, 0 and
    negative) and at stride 22 inside uploaded MSYNC_RECORD arrays equals the host form."""
    X, V, T, act, scan = (clouds[k] for k in ("X", "V", "T", "act", "scan"))
    s = Session(ctx, "ragged64", nodes=False)
    fresh = s.state()
    rec = s.fleet.process_many_clouds(X, scan, V, T, active=act)
    state = s.state()
    hold_clouds(rec, state, clouds, "host form")
    same(state[1:2], fresh[1:2], "nothing taken")
    st = s.fleet.stats()
    assert (st["steps"], st["scans"], st["calls"], st["host_syncs"], st["launches"]) == (14, 13, 1, 1, 4 * 14), st
    assert st["map_updates"] == sum(int((r["updated"] != 0).sum()) for r in clouds["want"][0])
    s.close()
    steps = np.arange(14)
    for stride in (1, api.MSYNC_RECORD.itemsize // 4):
        ptrs = []
        for m in range(3):
            if stride == 1:
                words = np.where(T[:, m], steps % 3 + 1, -(steps % 3)).astype(np.int32)
            else:
                words = np.zeros(14, api.MSYNC_RECORD)
                words["status"] = np.where(T[:, m], api.MSYNC_CORRECTED, [api.MSYNC_QUEUED, api.MSYNC_WAIT_IMU] * 7)
                words["n_imu"] = np.where(T[:, m], -5, 7)  # the word next to the status says the opposite
            ptrs.append((upload(ctx, X[:, m]), upload(ctx, V[:, m].astype(np.uint8)), upload(ctx, words)))
        s2 = Session(ctx, "ragged64", nodes=False)
        dev = s2.fleet.process_many_clouds_dev(14, 64, [p[0] for p in ptrs], [p[1] for p in ptrs], [p[2] for p in ptrs], stride,
                                               scan, active=act)
        assert dev.tobytes() == rec.tobytes(), stride
        hold_clouds(dev, s2.state(), clouds, "_dev, stride %d" % stride)
        s2.close()
        for p in sum(ptrs, ()):
            ctx.free(p)
    print("taken per member", [int(t.sum()) for t in clouds["take"]], "updates", [r["updated"].tolist() for r in clouds["want"][0]])


def test_active_and_take_compose(ctx, clouds):
    """2. an entry with active == 0 gives the not-taken record whatever its take word says, and its cloud and take word are
    not read: the rows of such entries hold a real cloud and take = 1 here (an address that would differ in the output, not
    one that faults), host form and _dev.  And masking a scan with `active` equals refusing it with its take word."""
    X, V, T, act, scan = (clouds[k] for k in ("X", "V", "T", "act", "scan"))
    X2, V2, T2 = X.copy(), V.copy(), T.copy()
    for m in range(3):
        k_real = int(np.flatnonzero(clouds["want"][0][m]["n_points"] > 40)[0]) if m != 1 else 1
        X2[~act[:, m], m], V2[~act[:, m], m], T2[~act[:, m], m] = clouds["xyz"][m][k_real], clouds["valid"][m][k_real], True
    assert (~act).sum() == 10 and V2[~act].any(1).all()
    s = Session(ctx, "ragged64", nodes=False)
    rec = s.fleet.process_many_clouds(X2, scan, V2, T2, active=act)
    assert all(H.not_taken(r) for r in rec[~act])
    hold_clouds(rec, s.state(), clouds, "poisoned rows, host form")
    s.close()
    ptrs = [(upload(ctx, X2[:, m]), upload(ctx, V2[:, m].astype(np.uint8)), upload(ctx, T2[:, m].astype(np.int32))) for m in range(3)]
    s = Session(ctx, "ragged64", nodes=False)
    dev = s.fleet.process_many_clouds_dev(14, 64, [p[0] for p in ptrs], [p[1] for p in ptrs], [p[2] for p in ptrs], 1, scan, active=act)
    assert dev.tobytes() == rec.tobytes()
    hold_clouds(dev, s.state(), clouds, "poisoned rows, _dev")
    s.close()
    # the same scans dropped by the host's mask, every take word 1 (NULL valid / take entries for member 1: all valid, all taken)
    s = Session(ctx, "ragged64", nodes=False)
    masked = s.fleet.process_many_clouds_dev(14, 64, [p[0] for p in ptrs], [p[1] for p in ptrs], None, 1, scan, active=act & T)
    assert all(H.not_taken(r) for r in masked[~(act & T)]) and masked[act & T].tobytes() == rec[act & T].tobytes()
    same(s.state(), clouds["want"][1], "masked by active")
    s.close()
    for p in sum(ptrs, ()):
        ctx.free(p)


# ---- 3 .. 9: the nodes in front --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(F.FLEETS))
def test_synced_form_equals_the_members_alone(ctx, name):
    """3. process_synced == every member's own process_synced alone, on fresh handles."""
    want = alone_run(ctx, name)
    s = Session(ctx, name)
    rec, srec = s.together(0, F.steps(name))
    status = np.where(F.active(name), srec["status"], F.INACTIVE)
    print(name, "status per step", status.tolist(), "points", rec["n_points"].tolist())
    assert status.tolist() == F.statuses(name).tolist()
    hold(name, rec, srec, s.state(), want, what=name)
    taken = status == 1
    assert all(H.not_taken(r) for r in rec[~taken]) and (rec["n_points"][taken] > 40).all()
    st = s.fleet.stats()
    assert (st["steps"], st["scans"], st["calls"], st["host_syncs"]) == (F.steps(name), int(taken.sum()), 1, 1), st
    assert [h.stats()["calls"] for _, h in s.pairs] == [0] * len(s.pairs)  # the fleet counts the calls
    assert [ms.stats()["launches"] for ms in s.nodes] == [0] * len(s.nodes)  # ... and the synchronisation's launches
    if name == "wide2":
        assert (rec["n_points"][taken] > 1024).all()
    if name == "ragged64":
        assert not taken[8].any() and not taken[0].any() and taken[3].all()
    for ms in s.nodes:  # the windows live in the fleet's buffer
        with pytest.raises(api.LslamError) as e:
            ms.read_windows(1)
        assert e.value.code == -8, e.value
    s.close()


def test_chunking_changes_nothing(ctx):
    """4. ragged64 in calls of 1, 4, 1, 3 and 5 steps == one call of 14 == the members alone."""
    name = "ragged64"
    want = alone_run(ctx, name)
    s = Session(ctx, name)
    recs, srecs, k = [], [], 0
    for size in F.CHUNKS:
        a, b = s.together(k, k + size)
        recs.append(a)
        srecs.append(b)
        k += size
    assert k == F.steps(name)
    hold(name, np.concatenate(recs), np.concatenate(srecs), s.state(), want, what="chunks")
    st, ss = s.fleet.stats(), s.fleet.sync_stats()
    assert st["calls"] == st["host_syncs"] == ss["calls"] == ss["host_waits"] == len(F.CHUNKS)
    assert st["launches"] == 4 * 14 and ss["launches"] == S_LAUNCHES * len(F.CHUNKS)
    s.close()


@pytest.mark.parametrize("fleet_first", [True, False], ids=["fleet_then_alone", "alone_then_fleet"])
def test_continuation_both_ways(ctx, fleet_first):
    """5. a fleet call of 7 steps and then every member alone, and the members alone for 7 steps and then the fleet, both
    equal the all-alone run: either route leaves the nodes' queues, sticky messages and queued scans as the other expects."""
    name, cut, n = "ragged64", F.CONTINUE_AT, F.steps("ragged64")
    want = alone_run(ctx, name)
    s = Session(ctx, name)
    if fleet_first:
        rec, srec = s.together(0, cut)
        first = list(zip(per_member(name, rec, 0, cut), per_member(name, srec, 0, cut)))
        second = s.alone(cut, n)
    else:
        first = s.alone(0, cut)
        rec, srec = s.together(cut, n)
        second = list(zip(per_member(name, rec, cut, n), per_member(name, srec, cut, n)))
    for m in range(3):
        parts = [p for p in (first[m], second[m]) if p is not None]
        assert np.concatenate([p[0] for p in parts]).tobytes() == want[0][m].tobytes(), m
        assert np.concatenate([p[1] for p in parts]).tobytes() == want[1][m].tobytes(), m
    same(s.state(), want[2], "continued")
    s.close()


def test_a_member_of_which_nothing_is_taken_is_unchanged(ctx):
    """6. steps [8, 10): every callback of members 0 and 2 is refused on the device; steps [12, 14): members 1 and 2 sit the
    call out.  Each keeps every snapshot byte and its scans / map_updates, with state to lose."""
    name = "ragged64"
    want = alone_run(ctx, name)
    s = Session(ctx, name)
    a = [s.together(0, 8)]
    before = s.state()
    a.append(s.together(8, 10))
    after = s.state()
    for m in (0, 2):
        assert before[m][0] == after[m][0] and before[m][1] == after[m][1], m
        assert before[m][0]["cached_points"] > 40 and any(np.frombuffer(p, f32).any() for p in before[m][0]["planes"])
        assert after[m][2][2] > before[m][2][2]  # (the node did count its refusals)
    assert after[1][1][0] == before[1][1][0] + 1  # member 1 took its one corrected scan
    a.append(s.together(10, 12))
    before = s.state()
    a.append(s.together(12, 14))
    after = s.state()
    for m in (1, 2):
        assert before[m] == after[m], m
    assert after[0][1][0] == before[0][1][0] + 2
    hold(name, np.concatenate([x[0] for x in a]), np.concatenate([x[1] for x in a]), after, want, what="8 + 2 + 2 + 2")
    s.close()


def test_launch_and_wait_accounting(ctx):
    """7. 4 launches of the fleet's chain per step; S = 5 launches of the synchronisation per call whatever R is; one host wait
    per call; a repeated shape grows no buffer."""
    per_fleet = {}
    for name in ("ragged64", "solo"):
        s = Session(ctx, name)
        s.together(0, 12)
        st, ss = s.fleet.stats(), s.fleet.sync_stats()
        assert st["launches"] == 4 * 12 and (st["calls"], st["host_syncs"]) == (1, 1), (name, st)
        assert (ss["calls"], ss["launches"], ss["host_waits"]) == (1, S_LAUNCHES, 1), (name, ss)
        per_fleet[name] = ss
        # the same shape again, on fresh nodes with the same messages (the processors go on): nothing grows
        for ms in s.nodes:
            ms.close()
        s.nodes = [node(ctx, c) for c in s.cases]
        s.together(0, 12)
        again = s.fleet.sync_stats()
        assert again["growths"] == ss["growths"] and (again["calls"], again["launches"], again["host_waits"]) == (2, 2 * S_LAUNCHES, 2)
        assert s.fleet.stats()["launches"] == 2 * 4 * 12
        s.close()
    assert per_fleet["ragged64"]["launches"] == per_fleet["solo"]["launches"] == S_LAUNCHES
    print(per_fleet)


def test_refusals_change_nothing(ctx):
    """8. a duplicated node, an n_readings that differs from one member's first scan, decreasing imu_seen for member 2 only:
    LSLAM_ERR_INVALID_ARGUMENT, every snapshot, counter and node unchanged; the valid call afterwards equals the
    never-refused run."""
    name, n = "ragged64", F.steps("ragged64")
    want = alone_run(ctx, name)
    s = Session(ctx, name)
    first = s.together(0, 1)  # member 0's first scan: its scan_count is 64 from here on; members 1 and 2 have seen none
    r, t, ti, iseen, oseen, act = F.step_arrays(name, 1, n)

    # The library has no reader for a node's `seen` counters.  They are held through what they decide: msync_check_scans refuses
    # an imu_seen / odom_seen below the handle's last one, so if any refused call had advanced a member's `seen` (to the last
    # entry of its column, which is above the first), the valid call at the end -- the ORIGINAL arrays, whose first entries
    # are the smallest -- would be refused as decreasing instead of giving the never-refused run's bytes.  The precondition
    # is asserted below: every member's columns do rise over the call.
    for m in range(3):
        col = np.flatnonzero(act[:, m])
        assert iseen[col[-1], m] > iseen[col[0], m] and oseen[col[-1], m] > oseen[col[0], m], m

    def refused(**changed):
        before, st, ss = s.state(), s.fleet.stats(), s.fleet.sync_stats()
        with pytest.raises(api.LslamError) as e:
            s.together(1, n, **changed)
        assert e.value.code == INVALID, e.value
        same(s.state(), before, sorted(changed))
        assert s.fleet.stats() == st and s.fleet.sync_stats() == ss
        return str(e.value)

    print(refused(syncs=[s.nodes[0], s.nodes[1], s.nodes[0]]))
    print(refused(ranges=np.ascontiguousarray(r[:, :, :63])))
    down = iseen.copy()
    mine = np.flatnonzero(act[:, 2])
    assert down[mine[2], 2] > 1
    down[mine[3], 2] = down[mine[2], 2] - 1
    print(refused(imu_seen=down))
    rest = s.together(1, n)
    hold(name, np.concatenate([first[0], rest[0]]), np.concatenate([first[1], rest[1]]), s.state(), want, what="after the refusals")
    s.close()


def test_with_and_without_matching(ctx):
    """9. wide2 with explicit hints and map_without_matching on every other step equals the members alone; a taken entry
    mapped without matching has its hint as its pose and updates the map."""
    name, n = "wide2", F.steps("wide2")
    k = np.arange(n, dtype=f32)[:, None] + np.array([0.0, 0.5], f32)[None, :]
    hints = np.stack([0.02 * k, -0.015 * k, 0.01 * k], 2).astype(f32)
    flags = np.broadcast_to((np.arange(n) % 2 == 1)[:, None], (n, 2)).copy()
    want = alone_run(ctx, name, hints, flags, key="hints")
    s = Session(ctx, name)
    rec, srec = s.together(0, n, hints, flags)
    hold(name, rec, srec, s.state(), want, what="hints")
    taken = srec["status"] == 1
    assert (taken & flags).sum() >= 4 and (taken & ~flags).sum() >= 4
    for i, m in zip(*np.nonzero(taken & flags)):
        assert rec["pose"][i, m].tobytes() == hints[i, m].tobytes() and rec["updated"][i, m] == 1
    s.close()


def test_a_reset_node_continues_with_a_longer_scan(ctx):
    """10. lslam_msync_reset forgets the node's scan_count but keeps its buffers.  A node that went through the fleet with 96
    beams, is reset and continues through a fleet with 1081 beams gets a queued-scan row that is long enough: the run equals
    a fresh node's alone, bit for bit."""
    want = alone_run(ctx, "wide1")
    short = Session(ctx, "solo")
    short.together(0, 4)
    ms, short.nodes = short.nodes[0], []
    short.close()
    ms.reset()
    s = Session(ctx, "wide1")
    s.nodes[0].close()
    s.nodes = [ms]
    H.push_all(ms, s.cases[0])
    assert s.cases[0]["ranges"].shape[1] == 1081 > 4 * 96
    rec, srec = s.together(0, F.steps("wide1"))
    hold("wide1", rec, srec, s.state(), want, what="after the reset")
    assert (rec["n_points"][1:, 0] > 1024).all()
    s.close()


def test_a_refused_longer_scan_keeps_the_resident_container(ctx, clouds):
    """11. a member whose resident container holds a 64-beam scan is offered two 1081-beam clouds and the take words refuse
    both: the container's buffer has to grow for the call, and its points, count and origo are still what they were."""
    k = int(np.flatnonzero(clouds["want"][0][0]["n_points"] > 40)[0])
    s = Session(ctx, "solo", nodes=False)
    rec = s.fleet.process_many_clouds(clouds["xyz"][0][k][None, None], clouds["scan"], clouds["valid"][0][k][None, None])
    assert rec["n_points"][0, 0] > 40 and rec["updated"][0, 0] == 1
    before = s.state()
    assert len(before[0][0]["container"]) == 8 * rec["n_points"][0, 0]
    big = np.ones((2, 1, 1081, 3), f32)
    rec2 = s.fleet.process_many_clouds(big, clouds["scan"], None, take=np.zeros((2, 1), bool))
    assert all(H.not_taken(r) for r in rec2.ravel())
    same(s.state(), before, "after the refused longer scans")
    s.close()
