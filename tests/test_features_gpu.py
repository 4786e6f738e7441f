"""lesson1's corner extraction on the device (csrc/features.hip, api.FeatureExtractor) against the reference's own published
picks (tests/golden/features_golden.npz) and against the numpy restatement (tests/feature_restatement.py), bit for bit: the
tolerance is zero -- integer selection over float32 arithmetic with a fixed evaluation order."""
import numpy as np
import pytest

import feature_cases as F
import feature_restatement as R
from lslam_amd import api

pytestmark = pytest.mark.gpu
u32 = np.uint32


@pytest.fixture(scope="module")
def gold():
    return F.golden()


@pytest.fixture(scope="module")
def restated(gold):
    return {name: R.extract_batch(g.case.ranges, g.case.n, g.case.threshold) for name, g in gold.items()}


@pytest.fixture(scope="module")
def fx(ctx):
    f = api.FeatureExtractor(ctx)
    yield f
    f.close()


@pytest.fixture(scope="module")
def device(gold, fx):
    """Every case through the host form, once: name -> (image, index, records, curvature)."""
    out = {}
    for name, g in gold.items():
        fx.set_threshold(g.case.threshold)
        out[name] = fx.extract(g.case.ranges, g.case.n)
    fx.set_threshold(1.0)
    return out


def _equal(a, b):
    """Bit for bit, every array of two extract() results."""
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        elif x.dtype == np.float32:
            assert np.array_equal(x.view(u32), y.view(u32))
        else:
            assert np.array_equal(x, y)


@pytest.mark.parametrize("name", F.NAMES)
def test_device_equals_the_reference(gold, device, name):
    g = gold[name]
    c = g.case
    image, index, rec, _ = device[name]
    assert image.shape == (len(c.ranges), c.n) and index.shape == (len(c.ranges), 6, 20)
    if not c.pinned:  # `ties`: the reference's pick COUNTS
        assert np.array_equal(rec["per_sector"], g.per_sector)
        return
    assert np.array_equal(image.view(u32), F.image_from_picks(g).view(u32))
    for k in range(len(c.ranges)):
        row = c.ranges[k, :c.n]
        assert rec["n_valid"][k] == int(np.isfinite(row).sum())
        for j in range(6):  # out_index as sets per sector (what a published image shows of them)
            shown = F.visible(row, index[k, j])
            want = g.picks[k][R.sector_of_beams(row, g.picks[k]) == j]
            assert np.array_equal(shown, want), (name, k, j)
        if name != "shapes_odd":  # (no +0.0f range anywhere: every pick shows)
            assert np.array_equal(rec["per_sector"][k], g.per_sector[k]), (name, k)
    assert np.array_equal(rec["n_corners"], rec["per_sector"].sum(axis=1))


@pytest.mark.parametrize("name", F.NAMES)
def test_device_equals_the_restatement(restated, device, name):
    r_image, r_index, r_valid, r_sector, r_curv = restated[name]
    image, index, rec, curv = device[name]
    assert np.array_equal(curv.view(u32), r_curv.view(u32))      # the arithmetic, apart from the selection
    assert np.array_equal(index, r_index)                        # slot for slot, the -1 padding included
    assert np.array_equal(image.view(u32), r_image.view(u32))
    assert np.array_equal(rec["n_valid"], r_valid) and np.array_equal(rec["per_sector"], r_sector)
    assert np.array_equal(rec["n_corners"], r_sector.sum(axis=1))
    assert np.array_equal((index >= 0).sum(axis=2), r_sector)


def test_sector_end_is_no_plain_top_20(device):
    _, index, rec, _ = device["sector_end"]
    assert index[0, 0, 0] == 179 and rec["per_sector"][0, 0] == 20


@pytest.mark.parametrize("name", ["arena", "small_counts", "shapes_odd", "threshold", "ties", "stride"])
def test_each_scan_of_a_batch_equals_the_scan_alone(gold, device, fx, name):
    c = gold[name].case
    fx.set_threshold(c.threshold)
    try:
        for k in range(len(c.ranges)):
            _equal(fx.extract(c.ranges[k:k + 1], c.n), [a[k:k + 1] for a in device[name]])
    finally:
        fx.set_threshold(1.0)


def _run_dev(ctx, fx, ranges, n, want_image=True, want_curv=True):
    B, stride = ranges.shape
    sizes = dict(r=max(ranges.nbytes, 4), image=max(B * n * 4, 4), index=B * 120 * 4, rec=B * 32, curv=max(B * n * 4, 4))
    p = {k: ctx.alloc(v) for k, v in sizes.items()}
    try:
        if ranges.size:
            ctx.upload(p["r"], ranges)
        fx.extract_dev(B, n, p["r"], stride, p["image"] if want_image else None, p["index"], p["rec"],
                       p["curv"] if want_curv else None)
        waits = fx.stats()["host_waits"]
        ctx.synchronize()
        image, curv = np.zeros((B, n), np.float32), np.zeros((B, n), np.float32)
        index, rec = np.zeros((B, 6, 20), np.int32), np.zeros(B, api.FEATURE_RECORD)
        if want_image and image.size:
            ctx.download(p["image"], image)
        if want_curv and curv.size:
            ctx.download(p["curv"], curv)
        ctx.download(p["index"], index)
        ctx.download(p["rec"], rec)
    finally:
        for v in p.values():
            ctx.free(v)
    return (image if want_image else None, index, rec, curv if want_curv else None), waits


@pytest.mark.parametrize("name", ["arena", "small_counts", "shapes_1500", "stride"])
def test_host_form_equals_dev_form(ctx, gold, device, fx, name):
    c = gold[name].case
    before = fx.stats()
    got, waits = _run_dev(ctx, fx, c.ranges, c.n)
    _equal(got, device[name])
    after = fx.stats()
    assert waits == before["host_waits"], "the _dev form makes no host wait"
    assert after["growths"] == before["growths"], "the _dev form owns no buffer"
    assert after["launches"] == before["launches"] + 1 and after["scans"] == before["scans"] + len(c.ranges)


def test_null_outputs_leave_the_others_unchanged(ctx, gold, device, fx):
    c = gold["arena"].case
    full = device["arena"]
    for wi, wc in ((False, True), (True, False), (False, False)):
        got = fx.extract(c.ranges, c.n, want_image=wi, want_curvature=wc)
        _equal(got, (full[0] if wi else None, full[1], full[2], full[3] if wc else None))
        got, _ = _run_dev(ctx, fx, c.ranges, c.n, wi, wc)
        _equal(got, (full[0] if wi else None, full[1], full[2], full[3] if wc else None))


def test_repeated_shape_allocates_nothing(ctx, gold):
    c = gold["arena"].case
    f = api.FeatureExtractor(ctx)
    try:
        first = f.extract(c.ranges, c.n)
        s1 = f.stats()
        second = f.extract(c.ranges, c.n)
        s2 = f.stats()
        _equal(first, second)
        assert s1["growths"] > 0 and s2["growths"] == s1["growths"]
        assert (s1["host_waits"], s2["host_waits"]) == (1, 2), "the host form waits once, at its end"
        assert (s1["launches"], s2["launches"]) == (1, 2) and s2["scans"] == 2 * len(c.ranges)
        f.extract(c.ranges[:7], c.n)  # a smaller batch fits what is there
        assert f.stats()["growths"] == s1["growths"]
    finally:
        f.close()


def test_stride_tail_is_not_read_as_beams(gold, device, fx):
    c = gold["stride"].case
    other = c.ranges.copy()
    other[:, c.n:] = 7.0  # finite where the case has NaN: nothing may change
    _equal(fx.extract(other, c.n), device["stride"])
    _equal(fx.extract(np.ascontiguousarray(c.ranges[:, :c.n])), device["stride"])


def test_error_codes_and_empty_calls(ctx, fx):
    with pytest.raises(api.LslamError) as e:
        fx.extract(np.ones((2, 1501), np.float32))
    assert e.value.code == -8  # LSLAM_ERR_UNSUPPORTED
    for bad in (-1.0, float("nan"), -1e-30):
        with pytest.raises(api.LslamError) as e:
            fx.set_threshold(bad)
        assert e.value.code == -1  # LSLAM_ERR_INVALID_ARGUMENT
    with pytest.raises(api.LslamError) as e:
        api.FeatureExtractor(ctx, edge_threshold=-2.0)
    assert e.value.code == -1
    fx.set_threshold(0.0)
    fx.set_threshold(1.0)
    before = fx.stats()
    image, index, rec, curv = fx.extract(np.zeros((0, 1081), np.float32))  # n_scans == 0: launches nothing
    assert fx.stats() == before and image.shape == (0, 1081) and len(rec) == 0
    image, index, rec, curv = fx.extract(np.zeros((3, 0), np.float32))     # n_readings == 0: every scan empty
    assert np.all(index == -1) and np.all(rec["n_valid"] == 0) and np.all(rec["n_corners"] == 0)
    assert np.all(rec["per_sector"] == 0) and image.shape == (3, 0)
    assert fx.stats()["scans"] == before["scans"] + 3
