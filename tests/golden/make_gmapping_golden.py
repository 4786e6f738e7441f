"""Regenerates tests/golden/gmapping_golden.npz from the reference's own GMapping map classes.

Compiles gmapping_ref_driver.cpp (next to this file) against the reference's lesson4 headers with g++ -O2
-ffp-contract=off into a temporary directory and records:
  node_*    one lesson4_gmapping_node callback (defaults: +-40 m, 0.05 m, maxRange 29.99, maxUrange 25, occ_thresh 0.25) on a
            1081-beam synth scan with NaN, +-inf, 0, > maxRange, == maxUrange, between the two and sub-cell readings
  pad_*     the same scan on an 81 m box (a 1620-wide published grid over 1600-wide storage)
  acc_*     16 scans at poses accumulated into one map
  multi_*   a crafted case whose acc sums depend on the order of the float additions (asserted below)
  line_*    gridLine traces of random endpoint pairs
  node_cos / node_sin   the angle cache
  ref_cpu_callback_s    the reference's CPU time per callback ON THE HOST THAT RAN THIS SCRIPT (best, mean), not a GPU figure

    python tests/golden/make_gmapping_golden.py [--reference /path/to/reference]
"""
from __future__ import annotations

import argparse
import math
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import lslam  # noqa: E402,F401
import gmapping_restatement as gr  # noqa: E402
from lslam_amd import synth  # noqa: E402

OUT = HERE / "gmapping_golden.npz"


def build_driver(reference: pathlib.Path, tmp: pathlib.Path) -> pathlib.Path:
    exe = tmp / "gmapping_ref_driver"
    subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-I", str(reference / "lesson4" / "include"), "-o", str(exe),
                    str(HERE / "gmapping_ref_driver.cpp")], check=True)
    return exe


def run_lines(exe, tmp, pairs: np.ndarray):
    """-> list of (num_points x 2) int arrays"""
    fin, fout = tmp / "lines.in", tmp / "lines.out"
    with open(fin, "wb") as f:
        np.array([len(pairs)], np.int32).tofile(f)
        np.ascontiguousarray(pairs, np.int32).tofile(f)
    subprocess.run([str(exe), "line", str(fin), str(fout)], check=True)
    raw, out, i = np.fromfile(fout, np.int32), [], 0
    for _ in range(len(pairs)):
        n = int(raw[i])
        out.append(raw[i + 1:i + 1 + 2 * n].reshape(n, 2))
        i += 1 + 2 * n
    return out


def run_map(exe, tmp, box, ranges, angle_min, angle_inc, poses=None, node=True, reps=0, max_range=30 - 0.01,
            max_use_range=25.0, occ_thresh=0.25):
    """-> dict(hdr, cos, sin, visits, n, acc_x, acc_y, mask, dropped, times, data)"""
    ranges = np.atleast_2d(np.asarray(ranges, np.float32))
    s, nb = ranges.shape
    poses = np.zeros((s, 3)) if poses is None else np.asarray(poses, np.float64)
    fin, fout = tmp / "map.in", tmp / "map.out"
    with open(fin, "wb") as f:
        np.array([*box, max_range, max_use_range, occ_thresh], np.float64).tofile(f)
        np.array([angle_min, angle_inc], np.float32).tofile(f)
        np.array([nb, s, int(node), reps], np.int32).tofile(f)
        poses.tofile(f)
        ranges.tofile(f)
    subprocess.run([str(exe), "map", str(fin), str(fout)], check=True)
    b = fout.read_bytes()
    o = 0

    def take(dt, count):
        nonlocal o
        a = np.frombuffer(b, dt, count, o)
        o += a.nbytes
        return a

    hdr = take(np.int32, 8)
    sx, sy, w, h, _, _, px, py = (int(v) for v in hdr)
    r = dict(hdr=hdr.copy(), cos=take(np.float64, nb).copy(), sin=take(np.float64, nb).copy())
    r["visits"] = take(np.int32, sx * sy).reshape(sy, sx)
    r["n"] = take(np.int32, sx * sy).reshape(sy, sx)
    r["acc_x"] = take(np.float32, sx * sy).reshape(sy, sx)
    r["acc_y"] = take(np.float32, sx * sy).reshape(sy, sx)
    r["mask"] = take(np.uint8, px * py).reshape(py, px).copy()
    r["dropped"] = int(take(np.int64, 1)[0])
    r["times"] = take(np.float64, 2).copy()
    if node:
        r["data"] = take(np.int8, w * h).reshape(h, w).copy()
    assert o == len(b)
    return r


def node_scan():
    """1081-beam synth scan in a small arena, with the special readings the node's filter and clamp distinguish."""
    laser = synth.Laser()
    world = synth.arena(size=30.0, n_axis=6, n_rot=2, seed=5)
    r = synth.cast_scan(world, (0.0, 0.0, 0.0), laser).astype(np.float32)
    special = {10: np.nan, 11: np.inf, 12: -np.inf, 13: 0.0, 14: 35.0, 15: 29.995, 16: 25.0, 17: 27.0, 18: 29.98,
               19: 0.01, 20: 0.03, 21: 0.024, 22: 0.026, 500: 0.074, 501: 0.076, 700: 24.9999, 701: 25.0001, 800: -1.0}
    for i, v in special.items():
        r[i] = v
    return laser, r


def accumulate_case(laser):
    world = synth.arena(size=30.0, n_axis=6, n_rot=2, seed=5)
    rng = np.random.default_rng(11)
    poses = np.stack([np.linspace(-3.0, 4.0, 16) + rng.uniform(-0.2, 0.2, 16), np.linspace(2.0, -2.5, 16),
                      rng.uniform(-math.pi, math.pi, 16)], axis=1)
    ranges = np.stack([synth.cast_scan(world, tuple(p), laser) for p in poses]).astype(np.float32)
    ranges[3, 100:110] = np.nan
    ranges[7, 200:205] = 40.0
    return ranges, poses


def multi_hit_case():
    """64 scans x 4 beams that all end in the cell around (3.0, 1.0): 256 hits whose float32 sums depend on their order."""
    rng = np.random.default_rng(3)
    n_scans, nb = 64, 4
    poses = np.stack([rng.uniform(-0.5, 0.5, n_scans), rng.uniform(-0.5, 0.5, n_scans), np.zeros(n_scans)], axis=1)
    ranges = np.zeros((n_scans, nb), np.float32)
    for s in range(n_scans):
        tx, ty = 3.0 + rng.uniform(-0.01, 0.01), 1.0 + rng.uniform(-0.01, 0.01)
        poses[s, 2] = math.atan2(ty - poses[s, 1], tx - poses[s, 0])
        base = math.hypot(tx - poses[s, 0], ty - poses[s, 1])
        ranges[s] = base + rng.uniform(-0.01, 0.01, nb)
    return ranges, poses, 0.0, 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    ref = pathlib.Path(args.reference)
    out = {}
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        exe = build_driver(ref, tmp)
        box = (-40.0, -40.0, 40.0, 40.0, 0.05)
        laser, r = node_scan()
        am, ai = np.float32(laser.angle_min), np.float32(laser.angle_increment)
        node = run_map(exe, tmp, box, r, am, ai, node=True, reps=20)
        out.update(node_ranges=r, node_angle=np.array([am, ai], np.float32), node_hdr=node["hdr"], node_cos=node["cos"],
                   node_sin=node["sin"], node_mask=node["mask"], node_data=node["data"],
                   ref_cpu_callback_s=node["times"])
        out.update(gr.pack_counters("node_", node["visits"], node["n"], node["acc_x"], node["acc_y"]))
        pad = run_map(exe, tmp, (-40.0, -40.0, 41.0, 41.0, 0.05), r, am, ai, node=True)
        out.update(pad_hdr=pad["hdr"], pad_mask=pad["mask"], pad_data=pad["data"])
        out.update(gr.pack_counters("pad_", pad["visits"], pad["n"], pad["acc_x"], pad["acc_y"]))

        ar, ap_ = accumulate_case(laser)
        acc = run_map(exe, tmp, box, ar, am, ai, poses=ap_, node=False)
        assert acc["dropped"] == 0
        out.update(acc_ranges=ar, acc_poses=ap_, acc_mask=acc["mask"])
        out.update(gr.pack_counters("acc_", acc["visits"], acc["n"], acc["acc_x"], acc["acc_y"]))

        mr, mp, mam, mai = multi_hit_case()
        multi = run_map(exe, tmp, box, mr, mam, mai, poses=mp, node=False)
        cell = np.unravel_index(np.argmax(multi["n"]), multi["n"].shape)
        assert multi["n"][cell] == mr.size, "every crafted hit must land in one cell"
        # the recorded sum is the in-order one, and another order gives other bits
        fx, fy = _hits_in_order(mr, mp, mam, mai)

        def fsum(vals):
            acc = np.float32(0)
            for v in vals:
                acc = np.float32(acc + v)
            return acc

        assert fsum(fx) == multi["acc_x"][cell] and fsum(fy) == multi["acc_y"][cell]
        others = [fsum(v[o]).view(np.uint32) != fsum(v).view(np.uint32) for v in (fx, fy)
                  for o in (slice(None, None, -1), np.argsort(v, kind="stable"))]
        assert any(others), "the crafted sums must depend on the order"
        out.update(multi_ranges=mr, multi_poses=mp, multi_angle=np.array([mam, mai], np.float32), multi_mask=multi["mask"])
        out.update(gr.pack_counters("multi_", multi["visits"], multi["n"], multi["acc_x"], multi["acc_y"]))

        rng = np.random.default_rng(7)
        pairs = rng.integers(-60, 61, size=(3000, 4)).astype(np.int32)
        pairs[:200, 2:] = pairs[:200, :2] + rng.integers(-3, 4, size=(200, 2))  # short lines, ties, single points
        d = rng.integers(-40, 41, size=200)
        pairs[200:400, 2] = pairs[200:400, 0] + d  # |dx| == |dy|
        pairs[200:400, 3] = pairs[200:400, 1] + d * rng.choice([-1, 1], size=200)
        lines = run_lines(exe, tmp, pairs)
        out.update(line_pairs=pairs, line_counts=np.array([len(l) for l in lines], np.int32),
                   line_points=np.concatenate(lines).astype(np.int16))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes); reference CPU per callback on this host: best "
          f"{node['times'][0] * 1e3:.2f} ms, mean {node['times'][1] * 1e3:.2f} ms")


def _hits_in_order(ranges, poses, angle_min, angle_inc):
    """The float32 endpoints of the multi-hit case in (scan, beam) order, from the restatement's formula."""
    cos_i, sin_i = gr.angle_cache(ranges.shape[1], angle_min, angle_inc)
    fx, fy = [], []
    for s in range(ranges.shape[0]):
        x, y, th = poses[s]
        sn, c = gr.sincos(th)
        d = ranges[s].astype(np.float64)
        fx.extend((x + d * (c * cos_i - sn * sin_i)).astype(np.float32))
        fy.extend((y + d * (sn * cos_i + c * sin_i)).astype(np.float32))
    return np.array(fx, np.float32), np.array(fy, np.float32)


if __name__ == "__main__":
    main()
