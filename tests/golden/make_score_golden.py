"""Regenerates tests/golden/score_golden.npz from the reference's own compiled OccGridMapUtil.

Compiles score_ref_driver.cpp (next to this file) against the reference's lesson4 headers, in place, and oracle/shim/Eigen with
g++ -O2 -ffp-contract=off into a temporary directory; the driver builds each map of tests/score_cases.py with the reference's
GridMap::updateByScan / DataContainer::setFrom and answers every query with its getResidualForState, getLikelihoodForState,
getCovarianceForPose and getCovMatrixWorldCoords.  Recorded:
  <map>_scan_counts / _scan_points / _scan_poses   the scans each map is built from (as generated on the host that ran this)
  <map>_plane_L<i>                                 the resulting log-odds plane of every level
  container_<name>                                 the containers ("big" is derived from n1081 by exact float32 products)
  pose_<name>                                      the pose table of score_cases.generate_poses() (headings at which this
                                                   host's sinf / cosf are correctly rounded: see tests/score_cases.py)
  q_pose / q_residual / q_likelihood               per query of score_cases.all_queries(), in its order
  cov_<name>_lik / _map / _world                   the seven likelihoods, covMatrixMap and the world-scaled matrix per case
  ref_cpu_state_s                                  the reference's CPU time per 1081-point getLikelihoodForState ON THE HOST THAT
                                                   RAN THIS SCRIPT, best of 5 passes -- not a GPU figure

    python tests/golden/make_score_golden.py [--reference /path/to/reference]
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
sys.path.insert(0, str(ROOT / "tests"))

import score_cases as S  # noqa: E402

OUT = HERE / "score_golden.npz"
f32 = np.float32


def build_driver(reference: pathlib.Path, tmp: pathlib.Path) -> pathlib.Path:
    exe = tmp / "score_ref_driver"
    subprocess.run(["g++", "-std=c++14", "-O2", "-DNDEBUG", "-ffp-contract=off", "-w", "-I", str(ROOT / "oracle" / "shim"),
                    "-I", str(reference / "lesson4" / "include"), "-o", str(exe), str(HERE / "score_ref_driver.cpp")], check=True)
    return exe


def run(exe, tmp, m: S.Map, conts, queries, covs, reps):
    fin, fout = tmp / "sc.in", tmp / "sc.out"
    with open(fin, "wb") as f:
        np.array([m.levels, m.sx, m.sy, len(m.scans), len(queries) + len(covs)], np.int32).tofile(f)
        np.array([m.cell, m.off[0], m.off[1], S.OCC_FACTOR], f32).tofile(f)
        for pts, pose in m.scans:
            np.array([len(pts)], np.int32).tofile(f)
            np.ascontiguousarray(pts, f32).tofile(f)
            np.ascontiguousarray(pose, f32).tofile(f)
        for kind, qs in ((0, queries), (1, covs)):
            for q in qs:
                pts = conts[q.container]
                np.array([kind, q.level, len(pts)], np.int32).tofile(f)
                np.ascontiguousarray(pts, f32).tofile(f)
                np.array(q.pose, f32).tofile(f)
    subprocess.run([str(exe), str(fin), str(fout), str(reps)], check=True)
    b = fout.read_bytes()
    at, planes = 0, []
    for sx, sy, _ in S.level_list(m):
        planes.append(np.frombuffer(b, f32, sx * sy, at).reshape(sy, sx).copy())
        at += 4 * sx * sy
    rl = np.frombuffer(b, f32, 2 * len(queries), at).reshape(-1, 2).copy()
    at += 8 * len(queries)
    cv = np.frombuffer(b, f32, 25 * len(covs), at).reshape(-1, 25).copy()
    at += 100 * len(covs)
    per_state = float(np.frombuffer(b, np.float64, 1, at)[0])
    assert at + 8 == len(b)
    return planes, rl, cv, per_state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    S._GENERATED = S.generate_poses()
    maps, conts = S.maps(), S.containers()
    queries, covs = S.all_queries(), S.covariances()
    out = {"container_" + k: v for k, v in conts.items() if k != "big"}
    out.update({"pose_" + k: v for k, v in S._GENERATED.items()})
    out["q_pose"] = np.array([q.pose for q in queries], f32)
    res, lik = np.zeros(len(queries), f32), np.zeros(len(queries), f32)
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        exe = build_driver(pathlib.Path(args.reference), tmp)
        for name, m in maps.items():
            idx = [i for i, q in enumerate(queries) if q.map == name]
            cn = [k for k, q in covs.items() if q.map == name]
            planes, rl, cv, per_state = run(exe, tmp, m, conts, [queries[i] for i in idx], [covs[k] for k in cn],
                                            5 if name == "main" else 0)
            res[idx], lik[idx] = rl[:, 0], rl[:, 1]
            out[name + "_scan_counts"] = np.array([len(p) for p, _ in m.scans], np.int32)
            out[name + "_scan_points"] = np.concatenate([p for p, _ in m.scans]).astype(f32)
            out[name + "_scan_poses"] = np.array([w for _, w in m.scans], f32)
            for L, p in enumerate(planes):
                out["%s_plane_L%d" % (name, L)] = p
            for k, row in zip(cn, cv):
                out["cov_%s_lik" % k], out["cov_%s_map" % k], out["cov_%s_world" % k] = row[:7], row[7:16].reshape(3, 3), row[16:].reshape(3, 3)
                print("cov %-10s likelihoods %s" % (k, np.array2string(row[:7], precision=3)))
            if name == "main":
                out["ref_cpu_state_s"] = np.array(per_state)
            print(f"{name}: {len(idx)} states, {len(cn)} covariances, planes {[p.shape for p in planes]}, "
                  f"{int(sum((p != 0).sum() for p in planes))} cells written")
    out["q_residual"], out["q_likelihood"] = res, lik
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes); reference CPU per 1081-point state on this host: "
          f"{float(out['ref_cpu_state_s']) * 1e6:.2f} us")


if __name__ == "__main__":
    main()
