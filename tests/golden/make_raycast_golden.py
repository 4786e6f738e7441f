"""Regenerates tests/golden/raycast_golden.npz from the reference's own compiled karto::OccupancyGrid::RayCast.

Compiles raycast_ref_driver.cpp (next to this file) against the reference's open_karto headers and library sources with
g++ -O2 -ffp-contract=off into a temporary directory and records, for every scenario of tests/raycast_cases.py:
  <name>_rays   float64 [n, 4]  x, y, heading, maxRange as handed to RayCast
  <name>_dist   float64 [n]     what RayCast returned
  <name>_stop   int64 [n]       the stopping index (round(distance / delta)), -1 for a ray that returned maxRange
and the grid the fan and scan_form scenarios run on:
  scan_ranges / scan_poses      the synth scans it is built from (as generated on the host that ran this script)
  scan_cells / scan_off         the cells and offset CreateFromScans gives for them (the plain-C oracle's, which the suite pins
                                to the reference and to the device)
  ref_cpu_ray_s                 the reference's CPU time per ray of scan_form (maxRange 12, 0.05 m cells) ON THE HOST THAT RAN
                                THIS SCRIPT, best of 5 passes -- not a GPU figure

    python tests/golden/make_raycast_golden.py [--reference /path/to/reference]
"""
from __future__ import annotations

import argparse
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
import raycast_cases as R  # noqa: E402
from oracle import pyoracle  # noqa: E402

OUT = HERE / "raycast_golden.npz"


def build_driver(reference: pathlib.Path, tmp: pathlib.Path) -> pathlib.Path:
    karto = reference / "lesson6" / "lib" / "open_karto"
    exe = tmp / "raycast_ref_driver"
    subprocess.run(["g++", "-std=c++14", "-O2", "-DNDEBUG", "-ffp-contract=off", "-w", "-I", str(ROOT / "oracle" / "shim"),
                    "-I", str(karto / "include"), "-o", str(exe), str(HERE / "raycast_ref_driver.cpp"),
                    str(karto / "src" / "Karto.cpp"), str(karto / "src" / "Mapper.cpp"), "-lpthread"], check=True)
    return exe


def run(exe, tmp, g: R.Grid, rays: np.ndarray, reps: int = 0):
    fin, fout = tmp / "rc.in", tmp / "rc.out"
    with open(fin, "wb") as f:
        np.array([g.w, g.h, len(rays)], np.int32).tofile(f)
        np.array([g.ox, g.oy, g.res], np.float64).tofile(f)
        np.ascontiguousarray(g.cells, np.uint8).tofile(f)
        np.ascontiguousarray(rays, np.float64).tofile(f)
    subprocess.run([str(exe), str(fin), str(fout), str(reps)], check=True)
    b = fout.read_bytes()
    n = len(rays)
    dist = np.frombuffer(b, np.float64, n, 0).copy()
    stop = np.frombuffer(b, np.int64, n, 8 * n).copy()
    per_ray = float(np.frombuffer(b, np.float64, 1, 16 * n)[0])
    assert len(b) == 16 * n + 8
    return dist, stop, per_ray


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    pyoracle.build("restate")
    laser, ranges, poses = R.scan_world()
    port = pyoracle.PortKarto(pyoracle.default_cfg(), pyoracle.laser_struct(laser, R.SCAN_THRESHOLD))
    cells, off = port.occgrid_from_scans(ranges, poses, R.RES)
    grid = R.scan_grid(cells, off)
    out = dict(scan_ranges=ranges, scan_poses=poses, scan_cells=cells, scan_off=np.asarray(off, np.float64))
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        exe = build_driver(pathlib.Path(args.reference), tmp)
        for name in R.NAMES:
            sc = R.scenario(name, grid if name in ("fan", "scan_form") else None)
            dist, stop, per_ray = run(exe, tmp, sc.grid, sc.rays, reps=5 if name == "scan_form" else 0)
            out.update({f"{name}_rays": sc.rays, f"{name}_dist": dist, f"{name}_stop": stop})
            if name == "scan_form":
                out["ref_cpu_ray_s"] = np.array(per_ray)
            print(f"{name}: {len(sc.rays)} rays, {int((stop >= 0).sum())} stopped, grid {sc.grid.w} x {sc.grid.h}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes); reference CPU per ray (scan_form) on this host: "
          f"{float(out['ref_cpu_ray_s']) * 1e9:.0f} ns")


if __name__ == "__main__":
    main()
