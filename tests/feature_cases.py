"""Scenarios for lesson1's corner extraction on the device (csrc/features.hip), built from fixed seeds and kept small.

tests/golden/features_golden.npz holds, for every case, the input ranges and what the reference's own compiled ScanCallback
published for them (tests/golden/make_features_golden.py); tests/test_features_oracle.py holds the numpy restatement
(tests/feature_restatement.py) to it on the CPU, tests/test_features_gpu.py holds the kernel to both.

    arena         40 scans x 1081 beams of synth.arena() from free poses; odd scans sigma = 0.01 noise, k % 4 > 1 1 % dropouts
    room          a noise-free square_room scan (few picks) and one with sigma = 0.3 (every sector over the cut-off)
    sector_end    1080 beams of 5.0, thirty spikes of +1..3 in [10, 160), beam 179 (the LAST element of sector 0) +0.12 ->
                  c = 1.44: the reference picks beam 179 and only 19 of the spikes; a plain "top 20" fails it
    small_counts  n = 80 with exactly 0, 1, 6, 7, 10, 11, 12, 13, 23, 64, 65 finite beams at random places: skipped sectors,
                  no curvature at all, exactly one curvature, the wave boundary
    shapes_<n>    n = 1, 63, 64, 65, 255, 256, 257, 1500, all finite, uniform in [1, 30]
    shapes_odd    n = 257: all +inf, all NaN, and one scan with zero and negative ranges
    threshold     4 scans of 5.0 + N(0, 0.05) at threshold 0.05 (about 125 candidates per sector)
    threshold_0   one noisy arena scan at threshold 0
    ties          1080 beams of 5.0, every 7th at 8.0: a cut-off tie in all six sectors -- NOT pinned to the reference's picks
                  (they follow its std::sort), only to its pick counts
    stride        3 arena scans in rows of n + 11, the tail columns NaN: they must not be read as beams
"""
import functools
import pathlib
from typing import NamedTuple

import numpy as np

from lslam_amd import synth

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "features_golden.npz"
SMALL_COUNTS = (0, 1, 6, 7, 10, 11, 12, 13, 23, 64, 65)
SHAPES = (1, 63, 64, 65, 255, 256, 257, 1500)
f32 = np.float32


class Case(NamedTuple):
    name: str
    ranges: np.ndarray   # [n_scans, stride] float32
    n: int               # n_readings <= stride
    threshold: float
    pinned: bool         # picks pinned to the reference's (False: only its pick counts)


def _arena_scans():
    rng = np.random.default_rng(7)
    world = synth.arena()
    scans = []
    for k in range(40):
        while True:
            x, y = rng.uniform(-35, 35, 2)
            if synth.point_is_free(world, x, y):
                break
        scans.append(synth.cast_scan(world, (x, y, rng.uniform(-3, 3)), noise_sigma=0.01 if k % 2 else 0.0,
                                     dropout=0.01 if k % 4 > 1 else 0.0, rng=rng))
    return np.stack(scans).astype(f32)


@functools.lru_cache(maxsize=None)
def build() -> tuple:
    """Every case from its seed (what the golden's generator records)."""
    out = []
    arena = _arena_scans()
    out.append(Case("arena", arena, arena.shape[1], 1.0, True))
    rng = np.random.default_rng(11)
    sq = synth.square_room()
    room = np.stack([synth.cast_scan(sq, (0.0, 0.0, 0.0)),
                     synth.cast_scan(sq, (0.3, 0.1, 0.05), noise_sigma=0.3, rng=rng)]).astype(f32)
    out.append(Case("room", room, room.shape[1], 1.0, True))
    rng = np.random.default_rng(3)
    a = np.full(1080, 5.0, f32)
    pos = rng.choice(np.arange(10, 160, 4), 30, replace=False)
    a[pos] += rng.uniform(1.0, 3.0, 30).astype(f32)
    a[179] += f32(0.12)
    out.append(Case("sector_end", a[None, :], 1080, 1.0, True))
    rng = np.random.default_rng(5)
    small = np.full((len(SMALL_COUNTS), 80), np.inf, f32)
    for k, c in enumerate(SMALL_COUNTS):
        small[k, rng.choice(80, c, replace=False)] = rng.uniform(0.5, 9.0, c).astype(f32)
    small[2, ~np.isfinite(small[2])] = np.nan   # (both kinds of non-finite beam)
    small[5, ~np.isfinite(small[5])] = -np.inf
    out.append(Case("small_counts", small, 80, 1.0, True))
    rng = np.random.default_rng(13)
    for n in SHAPES:
        out.append(Case(f"shapes_{n}", rng.uniform(1.0, 30.0, (1, n)).astype(f32), n, 1.0, True))
    odd = np.zeros((3, 257), f32)
    odd[0] = np.inf
    odd[1] = np.nan
    odd[2] = rng.uniform(-2.0, 2.0, 257).astype(f32)
    odd[2, rng.choice(257, 40, replace=False)] = 0.0
    out.append(Case("shapes_odd", odd, 257, 1.0, True))
    rng = np.random.default_rng(17)
    out.append(Case("threshold", (5.0 + rng.normal(0.0, 0.05, (4, 1081))).astype(f32), 1081, 0.05, True))
    out.append(Case("threshold_0", arena[1:2].copy(), arena.shape[1], 0.0, True))
    t = np.full(1080, 5.0, f32)
    t[7::7] = 8.0
    out.append(Case("ties", t[None, :], 1080, 1.0, False))
    n = arena.shape[1]
    wide = np.full((3, n + 11), np.nan, f32)
    wide[:, :n] = arena[4:7]
    out.append(Case("stride", wide, n, 1.0, True))
    return tuple(out)


NAMES = ("arena", "room", "sector_end", "small_counts") + tuple(f"shapes_{n}" for n in SHAPES) + (
    "shapes_odd", "threshold", "threshold_0", "ties", "stride")


class Golden(NamedTuple):
    case: Case               # with the ranges the generator recorded
    picks: list              # per scan: sorted original beam indices whose PUBLISHED range is not +0.0f (None when not pinned)
    per_sector: np.ndarray   # [n_scans, 6] picks per sector (of the same beams; of all picks for `ties`)


@functools.lru_cache(maxsize=None)
def golden() -> dict:
    """name -> Golden, read from the .npz alone."""
    z = np.load(GOLDEN)
    out = {}
    for name in NAMES:
        ranges = z[f"{name}_ranges"]
        n, thr, pinned = int(z[f"{name}_n"]), float(z[f"{name}_threshold"]), bool(z[f"{name}_pinned"])
        picks = None
        if pinned:
            flat, first = z[f"{name}_picks"], z[f"{name}_first"]
            picks = [flat[first[k]:first[k + 1]] for k in range(len(ranges))]
        out[name] = Golden(Case(name, ranges, n, thr, pinned), picks, z[f"{name}_per_sector"])
    return out


def image_from_picks(g: Golden) -> np.ndarray:
    """The reference's published image [n_scans, n], rebuilt from the recorded picks."""
    c = g.case
    img = np.zeros((len(c.ranges), c.n), f32)
    for k, p in enumerate(g.picks):
        img[k, p] = c.ranges[k, p]
    return img


def visible(ranges_row, beams) -> np.ndarray:
    """The beams of `beams` (>= 0) whose range is not +0.0f: the picks a published image shows."""
    b = np.asarray(beams, np.int64)
    b = b[b >= 0]
    return np.sort(b[np.asarray(ranges_row, f32).view(np.uint32)[b] != 0])
