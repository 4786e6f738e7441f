"""The PL-ICP kernels (csrc/plicp.hip) stay out of scratch memory and inside their LDS budget, read from the compiler's own
report in the device assembly (no GPU needed: hipcc cross-compiles).  Resource metadata only."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "creating-2d-laser-slam-from-scratch_amd" / "csrc"
WANT = {"k_plicp_match", "k_plicp_debug", "k_plicp_odom"}
# per reading (2048 of them): ref and sens points 4 x 8, the distance 8, the doubles' minimum / the survivors' distances 8, the
# owner / rank 4, five 16-bit index arrays 10, the flag byte 1 = 63 bytes; and the reduction scratch and counters
LDS_BUDGET = 2048 * 63 + 1024


@pytest.mark.timeout(600)
def test_plicp_kernels_use_no_scratch_and_fit_their_lds_budget(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not pathlib.Path(hipcc).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "plicp.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
           "-o", str(out), str(CSRC / "plicp.hip")]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    name, seen = None, {}
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\S+):", line)
        if m:
            k = re.search(r"_GLOBAL__N_1(\d+)(k_\w+)", m.group(1))
            name = k.group(2)[:int(k.group(1))] if k else None
            name = name if name in WANT else None
            continue
        m = re.search(r"; (ScratchSize|NumVgprs|LDSByteSize): (\d+)", line)
        if name and m:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
    print(seen)
    assert set(seen) == WANT, seen
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDSByteSize"] <= LDS_BUDGET, (k, v)
