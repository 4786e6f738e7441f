"""The batched Gauss-Newton matcher's kernels (csrc/logodds_map.hip) stay out of scratch memory and within the registers
their launch shape is meant for, read from the compiler's own resource report (no GPU needed: hipcc cross-compiles).

Bounds, from the launch shape and not from what the compiler happened to produce:
  scratch  0 bytes, both kernels
  VGPRs    <= 128: a gfx950 SIMD holds 512 per lane, so four waves per SIMD stay resident -- the wave-per-entry kernel
           lives on other waves covering a wave's L2 round trips
  LDS      k_gn_match_batch (one wave per entry, no barrier): none.  k_gn_match_batch_ordered keeps the single ordered
           call's layout (nine terms per point, sized at launch) and is not bound here."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SRC = ROOT / "creating-2d-laser-slam-from-scratch_amd" / "csrc" / "logodds_map.hip"
KERNELS = {"k_gn_match_batch", "k_gn_match_batch_ordered"}


@pytest.mark.timeout(600)
def test_gn_batch_kernel_resources(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not pathlib.Path(hipcc).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "logodds_map.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
           "-o", str(out), str(SRC)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    name, seen = None, {}
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\S+):", line)
        if m:
            k = re.search(r"\d+(k_gn_match_batch[a-z_0-9]*?)(E|I)", m.group(1))
            name = k.group(1) if k else None
            continue
        m = re.search(r"; (ScratchSize|NumVgprs|LDSByteSize): (\d+)", line)
        if name and m:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert set(seen) == KERNELS, seen  # exactly the shipped kernels: no second partition rides along
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["NumVgprs"] <= 128, (k, v)
    assert seen["k_gn_match_batch"]["LDSByteSize"] == 0, seen
