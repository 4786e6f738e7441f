"""Register / scratch budget of the MFMA forms of the coarse response kernel (LSLAM_OPT_ROWS_MFMA), from the compiler's own
report (no GPU needed: hipcc cross-compiles), and the instruction the form exists for.

k_resp_rows<NXD, NYC, TILED, MFMA = true, STATS, LDSB> and k_resp_rows_mw<NXD, NYC, WAVES, MFMA = true> keep one int32x4
accumulator per lattice row; like the packed forms (test_kernel_resources.py) they are held to 4 waves per SIMD without scratch,
the instrumented twins included.  The default body, <3, 11, tiled>, must really sum on the matrix pipe."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "creating-2d-laser-slam-from-scratch_amd" / "csrc"


@pytest.mark.timeout(900)
def test_mfma_forms_stay_out_of_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not pathlib.Path(hipcc).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "scan_matcher.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
           "-o", str(out), str(CSRC / "scan_matcher.hip")]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    name, seen, mfma = None, {}, {}
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\S+):", line)  # a function label
        if m:
            # Li3ELi11ELb1ELb1ELb0ELb0E = <3, 11, TILED, MFMA, STATS, LDSB>; _mw: Li3ELi11ELi2ELb1E = <3, 11, WAVES, MFMA>
            k = re.search(r"(k_resp_rows(?:_mw)?)I(\w+?)EEv", m.group(1))
            name = k.group(1) + "<" + k.group(2) + ">" if k else None
            continue
        if not name:
            continue
        m = re.search(r"; (NumVgprs|ScratchSize|Occupancy): (\d+)", line)
        if m:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
        elif re.match(r"\s+v_mfma_i32_16x16x64_i8\s", line):
            mfma[name] = mfma.get(name, 0) + 1
    rows = {k: v for k, v in seen.items() if re.fullmatch(r"k_resp_rows<Li\d+ELi\d+ELb[01]ELb1ELb[01]ELb0E>", k)}
    multi = {k: v for k, v in seen.items() if re.fullmatch(r"k_resp_rows_mw<Li\d+ELi\d+ELi\d+ELb1E>", k)}
    # <3,11> and <4,8>, tiled and linear, each with its instrumented twin; <3,11> and <4,8> at 2, 4 and 8 waves per block
    assert len(rows) == 8 and len(multi) == 6, seen
    for k, v in {**rows, **multi}.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 4, (k, v)
        assert v["NumVgprs"] <= 128, (k, v)
        assert mfma.get(k, 0) >= 1, k
    # the default body: every inlined drain sums its 11 lattice rows with one MFMA each
    assert mfma["k_resp_rows<Li3ELi11ELb1ELb1ELb0ELb0E>"] >= 11
    # and no packed form picked the instruction up
    assert not [k for k in mfma if k not in rows and k not in multi], mfma
