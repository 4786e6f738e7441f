"""`python bench.py` without --full: only the headline's K timed steps run, and --dump-outputs writes what the last of
them computed -- the fields of every scan's result record, float64 -- the same from run to run."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
FIELDS = {"pose": (3,), "response": (), "covariance": (3, 3), "status": (), "flags": ()}


def run_plain(tmp_path, tag):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                           "LSLAM_BENCH_BACKEND", "LSLAM_BENCH_FORCE_DIST", "LSLAM_BENCH_SHARE_GPU")}
    out, rec = tmp_path / tag, tmp_path / f"{tag}.npy"
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--batch", "1024",
                        "--dump-outputs", str(out), "--dump-results", str(rec)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), out, np.load(rec)


def test_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    from lslam_amd import api

    line, out, rec = run_plain(tmp_path, "a")
    assert line["full"] is False and line["steps"] == 7 and line["warmup"] == 2
    assert line["metric"].startswith("scan-matches/sec") and line["unit"] == "scan-matches/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1024 * 1e3 / line["ms_per_step"], rel=5e-3)  # ms_per_step is rounded to 0.1 us
    for k in ("roofline", "cpu_baseline", "secondary", "sustained", "pipelined_leg", "plain", "pruning",
              "kernel_ms_one_instrumented_plain_step"):
        assert line[k] is None, k  # behind --full
    assert line["results_ok"] == 1024
    rec = rec.view(api.RESULT_DTYPE).reshape(-1)
    assert sorted(p.stem for p in out.glob("*.npy")) == sorted(FIELDS)
    for name, shape in FIELDS.items():
        a = np.load(out / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape == (1024, *shape), name
        assert np.array_equal(a, rec[name].astype(np.float64)), name  # the records the timed step wrote, field by field
    # same arguments, same inputs: a second run computes the same outputs
    _, out_b, _ = run_plain(tmp_path, "b")
    for name in FIELDS:
        assert np.load(out / f"{name}.npy").tobytes() == np.load(out_b / f"{name}.npy").tobytes(), name
