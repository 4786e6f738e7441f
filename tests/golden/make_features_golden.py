"""Regenerates tests/golden/features_golden.npz from the reference's own compiled lesson1 LaserScan::ScanCallback.

Compiles features_ref_driver.cpp (next to this file), which #includes the reference's lesson1/src/feature_detection.cc
unmodified behind the ROS stand-ins of oracle/shim, with g++ -O2 -ffp-contract=off into a temporary directory and records, for
every case of tests/feature_cases.py:
  <name>_ranges      float32 [n_scans, stride]  the input (as generated on the host that ran this script)
  <name>_n, <name>_threshold, <name>_pinned
  <name>_picks       int32, <name>_first int64 [n_scans + 1]: per scan the sorted original beam indices whose PUBLISHED range
                     is not +0.0f -- index lists, not images, to stay small (pinned cases only)
  <name>_per_sector  int32 [n_scans, 6]: those picks per sector; for `ties` the pick counts are all that is recorded
  ref_cpu_scan_s     the reference's CPU time per scan of `arena` ON THE HOST THAT RAN THIS SCRIPT, best of 5 passes -- not a
                     GPU figure
and ASSERTS that no pinned case has equal curvatures across a cut-off in any sector (the cap is zero: there the reference's
picks follow its std::sort and no rule of ours).  If a regenerated input ever breaks that, change its seed.

    python tests/golden/make_features_golden.py [--reference /path/to/reference]
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
import feature_cases as F  # noqa: E402
import feature_restatement as R  # noqa: E402

OUT = HERE / "features_golden.npz"
CUTOFF_TIE_CAP = 0


def build_driver(reference: pathlib.Path, tmp: pathlib.Path) -> pathlib.Path:
    src = reference / "lesson1" / "src" / "feature_detection.cc"
    if not src.is_file():
        raise FileNotFoundError(src)
    exe = tmp / "features_ref_driver"
    subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-w", "-I", str(ROOT / "oracle" / "shim"),
                    "-I", str(ROOT / "oracle" / "shim" / "ros_pcl"), f'-DFEATURE_DETECTION_CC="{src}"',
                    "-o", str(exe), str(HERE / "features_ref_driver.cpp")], check=True)
    return exe


def run(exe, tmp, ranges: np.ndarray, threshold: float, reps: int = 0):
    """ranges [n_scans, n] -> (published [n_scans, n] float32, CPU seconds per scan)."""
    fin, fout = tmp / "feat.in", tmp / "feat.out"
    r = np.ascontiguousarray(ranges, np.float32)
    with open(fin, "wb") as f:
        np.array([r.shape[0], r.shape[1], reps], np.int32).tofile(f)
        np.array([threshold], np.float32).tofile(f)
        r.tofile(f)
    subprocess.run([str(exe), str(fin), str(fout)], check=True)
    b = fout.read_bytes()
    assert len(b) == 4 * r.size + 8
    return np.frombuffer(b, np.float32, r.size, 0).reshape(r.shape).copy(), float(np.frombuffer(b, np.float64, 1, 4 * r.size)[0])


def record(exe, tmp, case: F.Case, reps: int = 0):
    rows = np.ascontiguousarray(case.ranges[:, :case.n])
    published, per_scan = run(exe, tmp, rows, case.threshold, reps)
    out = {f"{case.name}_ranges": case.ranges, f"{case.name}_n": np.array(case.n), f"{case.name}_threshold": np.array(case.threshold),
           f"{case.name}_pinned": np.array(case.pinned)}
    picks, per_sector, ties = [], np.zeros((len(rows), R.SECTORS), np.int32), 0
    for k, row in enumerate(rows):
        p = np.nonzero(published[k].view(np.uint32))[0]
        assert np.array_equal(published[k, p].view(np.uint32), row[p].view(np.uint32)), (case.name, k)
        picks.append(p.astype(np.int32))
        per_sector[k] = np.bincount(R.sector_of_beams(row, p), minlength=R.SECTORS)
        ties += R.extract(row, case.threshold).cutoff_ties
    if case.pinned:
        assert ties <= CUTOFF_TIE_CAP, f"{case.name}: {ties} sectors with equal curvatures across the cut-off: change the seed"
        out[f"{case.name}_picks"] = np.concatenate(picks) if picks else np.zeros(0, np.int32)
        out[f"{case.name}_first"] = np.concatenate([[0], np.cumsum([len(p) for p in picks])]).astype(np.int64)
    out[f"{case.name}_per_sector"] = per_sector
    print(f"{case.name}: {len(rows)} scans x {case.n}, threshold {case.threshold}, {int(per_sector.sum())} published picks, "
          f"{ties} cut-off ties")
    return out, per_scan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        exe = build_driver(pathlib.Path(args.reference), tmp)
        for case in F.build():
            rec, per_scan = record(exe, tmp, case, reps=5 if case.name == "arena" else 0)
            out.update(rec)
            if case.name == "arena":
                out["ref_cpu_scan_s"] = np.array(per_scan)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes); reference CPU per scan (arena) on this host: "
          f"{float(out['ref_cpu_scan_s']) * 1e6:.1f} us")


if __name__ == "__main__":
    main()
