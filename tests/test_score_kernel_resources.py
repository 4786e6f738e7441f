"""The pose-scoring kernels (csrc/logodds_map.hip: k_ms_*) stay out of scratch memory and within 128 VGPRs, read from the
compiler's own resource report (no GPU needed: hipcc cross-compiles; the file is compiled once for the module).

128 VGPRs: k_ms_score runs one wave per state, four states per block, and lives -- like k_gn_match_batch -- on four resident
waves per SIMD covering one another's round trips to L2 for the map cells; the other kernels are held to the same figure.
k_ms_score keeps nothing in LDS (no barrier: a state's result cannot depend on its neighbours in the block)."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "creating-2d-laser-slam-from-scratch_amd" / "csrc" / "logodds_map.hip"
KERNELS = {"k_ms_score<2>", "k_ms_score<4>", "k_ms_score<8>", "k_ms_score_ordered", "k_ms_best", "k_ms_cov"}
MAX_VGPRS = 128


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not pathlib.Path(hipcc).exists():
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("resources") / "logodds_map.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
           "-o", str(out), str(SRC)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    name, seen = None, {}
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\S+):", line)
        if m:
            k = re.search(r"\d+(k_ms_[a-z_0-9]*?)(?:ILi(\d+)E|E)", m.group(1))
            name = (k.group(1) + ("<%s>" % k.group(2) if k.group(2) else "")) if k else None
            continue
        m = re.search(r"; (ScratchSize|NumVgprs|LDSByteSize): (\d+)", line)
        if name and m:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
    for k in sorted(seen):
        print(k, seen[k])
    return seen


@pytest.mark.timeout(600)
def test_score_kernel_resources(report):
    assert set(report) == KERNELS, sorted(report)  # exactly the shipped kernels: no second partition rides along
    for k, v in report.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["NumVgprs"] <= MAX_VGPRS, (k, v)
    for k in ("k_ms_score<2>", "k_ms_score<4>", "k_ms_score<8>"):
        assert report[k]["LDSByteSize"] == 0, (k, report[k])
