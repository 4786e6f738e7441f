"""lesson2's ICP in the C ABI: declared in the header, exported by the built library, refused without a handle, a 64-byte
record, the defaults, and the header states its standing and its tie rule.  No device needed."""
import math
import pathlib
import re
import subprocess
import sys

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ["lslam_icp_params_defaults", "lslam_icp_create", "lslam_icp_destroy", "lslam_icp_set_laser", "lslam_icp_convert_batch",
           "lslam_icp_convert_batch_dev", "lslam_icp_match_batch", "lslam_icp_match_batch_dev", "lslam_icp_match_clouds",
           "lslam_icp_match_clouds_dev", "lslam_icp_debug_iteration", "lslam_icp_stats"]


def test_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name in SYMBOLS:
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
    assert L.lslam_abi_version() == 5 and "#define LSLAM_ABI_VERSION 5" in header
    assert re.search(r"#define\s+LSLAM_ICP_MAX_POINTS\s+2048\b", header) and api.ICP_MAX_POINTS == 2048
    flat = re.sub(r"[\s*/]+", " ", header).lower()
    assert flat.count("parity with the reference is unpinned") == 2    # lesson3's and lesson2's
    assert "among equal distances the lowest target index wins" in flat
    assert "literal origin points" in flat and "2-d closed form" in flat and "fp64 on the original points" in flat
    assert "skip_invalid = 1 is the opt-in" in flat


def test_defaults_are_pcls():
    p = api.icp_params()
    dbl_max = sys.float_info.max
    assert (p.max_iterations, p.max_correspondence_distance, p.transformation_epsilon, p.euclidean_fitness_epsilon,
            p.absolute_mse) == (10, math.sqrt(dbl_max), 0.0, -dbl_max, 1e-12)
    assert (p.skip_invalid, p.invalid_as_nan, p.reserved) == (0, 0, 0)
    from tools import icp_cpu
    q = icp_cpu.IcpParams()
    assert all(getattr(p, k) == getattr(q, k) for k in ("max_iterations", "max_correspondence_distance", "transformation_epsilon",
                                                        "euclidean_fitness_epsilon", "absolute_mse", "skip_invalid", "invalid_as_nan"))


def test_calls_without_a_handle_are_refused():
    L = api.lib()
    assert L.lslam_icp_create(None, None, None) == -1  # LSLAM_ERR_INVALID_ARGUMENT
    assert L.lslam_icp_set_laser(None, 0.0, 0.1, 0.1, 30.0) == -1
    assert L.lslam_icp_stats(None, None) == -1
    for fn in (L.lslam_icp_convert_batch, L.lslam_icp_convert_batch_dev):
        assert fn(None, 0, 0, None, 0, None, None) == -1
        assert fn(None, 2, 360, None, 360, None, None) == -1
    for fn in (L.lslam_icp_match_batch, L.lslam_icp_match_batch_dev):
        assert fn(None, 0, 0, None, 0, 0, None, None, None, None) == -1
        assert fn(None, 2, 360, None, 360, 1, None, None, None, None) == -1
    for fn in (L.lslam_icp_match_clouds, L.lslam_icp_match_clouds_dev):
        assert fn(None, 0, 0, None, None, 0, None, None, None, None) == -1
        assert fn(None, 2, 360, None, None, 1, None, None, None, None) == -1
    assert L.lslam_icp_debug_iteration(None, None, None, None, None, 0, None, None, None, None, None, None) == -1
    L.lslam_icp_destroy(None)  # a no-op
    L.lslam_icp_params_defaults(None)


def test_the_record_is_64_bytes(tmp_path):
    assert api.ICP_RECORD.itemsize == 64 and api.ICP_RECORD.fields["converged"][1] == 40
    assert api.ICP_RECORD.fields["state"][1] == 52 and api.ICP_RECORD.fields["reserved"][1] == 56
    src = tmp_path / "rec.c"
    src.write_text('#include <stddef.h>\n#include "lslam_gpu.h"\n'
                   '_Static_assert(sizeof(lslam_icp_record) == 64, "64 bytes");\n'
                   '_Static_assert(offsetof(lslam_icp_record, fitness) == 24, "fitness at 24");\n'
                   '_Static_assert(offsetof(lslam_icp_record, mse) == 32, "mse at 32");\n'
                   '_Static_assert(offsetof(lslam_icp_record, converged) == 40, "converged at 40");\n'
                   '_Static_assert(offsetof(lslam_icp_record, iterations) == 44, "iterations at 44");\n'
                   '_Static_assert(offsetof(lslam_icp_record, ncorr) == 48, "ncorr at 48");\n'
                   '_Static_assert(offsetof(lslam_icp_record, state) == 52, "state at 52");\n'
                   '_Static_assert(offsetof(lslam_icp_record, reserved) == 56, "reserved at 56");\n'
                   '_Static_assert(sizeof(lslam_icp_params) == 48, "48 bytes");\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), "-fsyntax-only", str(src)], check=True)
