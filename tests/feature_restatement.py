"""lesson1's corner extraction (LaserScan::ScanCallback) restated in numpy float32, with this library's tie rule.  Written
from the semantics in include/lslam_gpu.h, not from the reference's text; tests/test_features_oracle.py holds it to what the
reference's own compiled source published (tests/golden/features_golden.npz), tests/test_features_gpu.py holds the kernel to it.

    compaction   the finite beams, in order: v[0..count), map[i] = original beam index
    curvature    5 <= i < count-5: d = v[i-5]+...+v[i-1] - v[i]*10 + v[i+1]+...+v[i+5], left to right, every operation
                 rounded to float32; c[i] = d*d; 0 elsewhere
    sectors      j = 0..5: s = count*j//6, e = count*(j+1)//6 - 1; skipped when s >= e
    selection    element e first when c[e] > thr (it uses one of the 20 slots), then the largest c > thr of [s, e) in
                 descending order; among EQUAL curvatures the HIGHER compacted index first
"""
from typing import NamedTuple

import numpy as np

SECTORS, PICKS, MAX_READINGS = 6, 20, 1500
f32 = np.float32


class Extract(NamedTuple):
    image: np.ndarray       # [n] float32: the range of every pick at its beam, +0.0 elsewhere
    index: np.ndarray       # [6, 20] int32: original beam indices in pick order, -1 = unused
    n_valid: int
    per_sector: np.ndarray  # [6] int32
    curvature: np.ndarray   # [n] float32: c at the original beam index, 0 elsewhere
    cutoff_ties: int        # sectors in which equal curvatures straddle the cut-off (there the tie rule decides)
    max_candidates: int     # the most c > thr any sector's [s, e) holds


def curvature(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, f32)
    count = len(v)
    c = np.zeros(count, f32)
    if count < 11:
        return c
    m = count - 10
    w = [v[k:k + m] for k in range(11)]  # w[k][q] = v[q + k]; the centre i = q + 5
    with np.errstate(over="ignore", invalid="ignore"):
        d = w[0] + w[1]  # (float32 arrays: every operation rounds to float32)
        d = d + w[2]
        d = d + w[3]
        d = d + w[4]
        d = d - w[5] * f32(10)
        for k in range(6, 11):
            d = d + w[k]
        c[5:count - 5] = d * d
    return c


def extract(ranges, threshold=1.0) -> Extract:
    r = np.ascontiguousarray(ranges, f32)
    thr = f32(threshold)
    n = len(r)
    beam = np.nonzero(np.isfinite(r))[0]
    v = r[beam]
    count = len(v)
    c = curvature(v)
    image = np.zeros(n, f32)
    index = np.full((SECTORS, PICKS), -1, np.int32)
    per_sector = np.zeros(SECTORS, np.int32)
    ties = most = 0
    for j in range(SECTORS):
        s, e = count * j // 6, count * (j + 1) // 6 - 1
        if s >= e:
            continue
        picks = [e] if c[e] > thr else []
        body = np.arange(s, e)
        cand = body[c[body] > thr]
        most = max(most, len(cand))
        order = sorted(cand.tolist(), key=lambda i: (-float(c[i]), -i))  # (float64 of a float32 keeps the order and the ties)
        room = PICKS - len(picks)
        if len(order) > room and c[order[room - 1]] == c[order[room]]:
            ties += 1
        picks += order[:room]
        per_sector[j] = len(picks)
        index[j, :len(picks)] = beam[picks]
        image[beam[picks]] = r[beam[picks]]
    curv = np.zeros(n, f32)
    curv[beam] = c
    return Extract(image, index, count, per_sector, curv, ties, most)


def extract_batch(ranges, n_readings=None, threshold=1.0):
    """[B, stride] -> (image [B, n], index [B, 6, 20], n_valid [B], per_sector [B, 6], curvature [B, n])."""
    r = np.asarray(ranges, f32)
    n = r.shape[1] if n_readings is None else n_readings
    ex = [extract(row[:n], threshold) for row in r]
    return (np.stack([x.image for x in ex]).reshape(len(ex), n), np.stack([x.index for x in ex]),
            np.array([x.n_valid for x in ex], np.int32), np.stack([x.per_sector for x in ex]),
            np.stack([x.curvature for x in ex]).reshape(len(ex), n))


def sector_of_beams(ranges, beams) -> np.ndarray:
    """The sector each of `beams` (original indices of FINITE beams of one scan) lies in."""
    r = np.asarray(ranges, f32)
    fin = np.isfinite(r)
    comp = np.cumsum(fin) - 1  # original -> compacted index
    count = int(fin.sum())
    ends = np.array([count * (j + 1) // 6 - 1 for j in range(SECTORS)])
    return np.searchsorted(ends, comp[np.asarray(beams, np.int64)])
