"""lesson1's corner extraction on the CPU: the numpy restatement (tests/feature_restatement.py) equals what the reference's own
compiled ScanCallback published (tests/golden/features_golden.npz) -- pick sets, image bits and counts -- for every pinned case
of tests/feature_cases.py, its pick counts per sector for `ties`, and every case is what it claims to be.  No device needed."""
import pathlib
import sys

import numpy as np
import pytest

import feature_cases as F
import feature_restatement as R

ROOT = pathlib.Path(__file__).resolve().parent.parent
u32 = np.uint32


@pytest.fixture(scope="module")
def gold():
    return F.golden()


@pytest.fixture(scope="module")
def restated(gold):
    return {name: [R.extract(row[:g.case.n], g.case.threshold) for row in g.case.ranges] for name, g in gold.items()}


@pytest.mark.parametrize("name", F.NAMES)
def test_restatement_equals_the_reference(gold, restated, name):
    g = gold[name]
    c = g.case
    if c.pinned:
        ref_image = F.image_from_picks(g)
    for k, ex in enumerate(restated[name]):
        row = c.ranges[k, :c.n]
        assert ex.n_valid == int(np.isfinite(row).sum())
        if not c.pinned:  # the picks across the cut-off follow the reference's std::sort; its COUNTS are pinned
            assert np.array_equal(ex.per_sector, g.per_sector[k]), (name, k)
            continue
        assert ex.cutoff_ties == 0, (name, k)
        assert np.array_equal(ex.image.view(u32), ref_image[k].view(u32)), (name, k)
        shown = F.visible(row, ex.index.ravel())
        assert np.array_equal(shown, g.picks[k]), (name, k)
        assert np.array_equal(np.bincount(R.sector_of_beams(row, shown), minlength=6), g.per_sector[k]), (name, k)
        # (a pick whose range is +0.0f cannot be seen in a published image: only shapes_odd has such ranges)
        if name != "shapes_odd":
            assert np.array_equal(ex.per_sector, g.per_sector[k]), (name, k)
            assert len(shown) == int(ex.per_sector.sum())


def test_the_generated_cases_are_the_recorded_ones(gold):
    """The golden's inputs are what tests/feature_cases.py builds (shapes, thresholds, and the bits of the cases numpy alone
    makes; the synth scans go through the host's libm and may differ in a last bit on another machine)."""
    built = {c.name: c for c in F.build()}
    assert tuple(built) == F.NAMES == tuple(gold)
    for name, g in gold.items():
        b = built[name]
        assert (b.ranges.shape, b.n, b.threshold, b.pinned) == (g.case.ranges.shape, g.case.n, g.case.threshold, g.case.pinned)
        if name not in ("arena", "room", "threshold_0", "stride"):
            assert np.array_equal(b.ranges.view(u32), g.case.ranges.view(u32)), name


def test_every_case_is_what_it_claims(gold, restated):
    fin = lambda name: np.isfinite(gold[name].case.ranges[:, :gold[name].case.n]).sum(axis=1).tolist()  # noqa: E731
    assert gold["arena"].case.ranges.shape == (40, 1081)
    assert any(n < 1081 for n in fin("arena"))  # dropouts and no-returns: the compaction moves indices
    over = [int(ex.max_candidates > R.PICKS) for ex in restated["arena"]]
    assert sum(over) >= 10, "many arena scans have a sector over the cut-off"
    quiet, loud = restated["room"]
    assert int(quiet.per_sector.sum()) < 20 and np.all(loud.per_sector == R.PICKS) and loud.max_candidates > 100
    # sector_end: beam 179 is element e of sector 0 with c = 1.44, picked FIRST, and 19 of the 30 spikes go with it
    se = restated["sector_end"][0]
    assert se.n_valid == 1080 and se.index[0, 0] == 179 and se.per_sector[0] == 20
    assert abs(float(se.curvature[179]) - 1.44) < 1e-4
    spikes = np.nonzero(gold["sector_end"].case.ranges[0, :160] > 5.5)[0]
    assert len(spikes) == 30 and len(set(se.index[0, 1:].tolist()) & set(spikes.tolist())) == 19
    top20 = np.argsort(-se.curvature[:179], kind="stable")[:20]
    assert set(top20.tolist()) != set(se.index[0].tolist()), "a plain top 20 of [s, e) is another set"
    assert 179 in gold["sector_end"].picks[0]
    assert fin("small_counts") == list(F.SMALL_COUNTS)
    sc = restated["small_counts"]
    assert all(int(ex.per_sector.sum()) == 0 for ex in sc[:5])       # fewer than 11 finite beams: no curvature at all
    assert int(np.count_nonzero(sc[5].curvature)) == 1               # 11: exactly one
    assert int(sc[10].per_sector.sum()) > 0
    for n in F.SHAPES:
        assert fin(f"shapes_{n}") == [n]
    odd = gold["shapes_odd"].case.ranges
    assert fin("shapes_odd") == [0, 0, 257] and np.all(np.isposinf(odd[0])) and np.all(np.isnan(odd[1]))
    assert (odd[2] == 0).sum() == 40 and (odd[2] < 0).sum() > 50
    assert gold["threshold"].case.threshold == pytest.approx(0.05) and gold["threshold_0"].case.threshold == 0.0
    assert all(100 < ex.max_candidates for ex in restated["threshold"])
    assert restated["threshold_0"][0].max_candidates > 100
    assert restated["ties"][0].cutoff_ties == 6 and np.all(gold["ties"].per_sector == R.PICKS)
    st = gold["stride"].case
    assert st.ranges.shape[1] == st.n + 11 and np.all(np.isnan(st.ranges[:, st.n:]))
    assert np.array_equal(st.ranges[:, :st.n].view(u32), gold["arena"].case.ranges[4:7].view(u32))


def test_tie_rule_of_the_restatement(gold):
    """Among equal curvatures the higher compacted index ranks first (all beams of `ties` are finite: compacted = original)."""
    ex = R.extract(gold["ties"].case.ranges[0], 1.0)
    equal_pairs = 0
    for j in range(6):
        e = 1080 * (j + 1) // 6 - 1
        row = ex.index[j][ex.index[j] >= 0]
        body = row[1:] if row[0] == e else row
        keys = [(-float(ex.curvature[b]), -int(b)) for b in body]
        assert keys == sorted(keys), j
        equal_pairs += sum(k0[0] == k1[0] for k0, k1 in zip(keys[:-1], keys[1:]))
    assert equal_pairs > 0


def test_reference_rebuilt_in_place_republishes_a_case(tmp_path, gold):
    reference = pathlib.Path("/root/reference")
    if not (reference / "lesson1" / "src" / "feature_detection.cc").is_file():
        pytest.skip("the reference's source is not on this machine")
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import make_features_golden as M

    exe = M.build_driver(reference, tmp_path)
    g = gold["sector_end"]
    published, _ = M.run(exe, tmp_path, g.case.ranges, g.case.threshold)
    assert np.array_equal(published.view(u32), F.image_from_picks(g).view(u32))
    g = gold["threshold"]
    published, _ = M.run(exe, tmp_path, g.case.ranges, g.case.threshold)
    assert np.array_equal(published.view(u32), F.image_from_picks(g).view(u32))
