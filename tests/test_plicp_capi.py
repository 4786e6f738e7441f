"""lesson3's PL-ICP in the C ABI: declared in the header, exported by the built library, refused without a handle, a 48-byte
record, the header states its standing and its tie rule.  No device needed."""
import pathlib
import re
import subprocess

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ["lslam_plicp_params_defaults", "lslam_plicp_create", "lslam_plicp_destroy", "lslam_plicp_set_laser",
           "lslam_plicp_match_batch", "lslam_plicp_match_batch_dev", "lslam_plicp_debug_iteration", "lslam_plicp_stats",
           "lslam_plicp_odom_create", "lslam_plicp_odom_destroy", "lslam_plicp_odom_set_laser", "lslam_plicp_odom_reset",
           "lslam_plicp_odom_state", "lslam_plicp_odom_process_many", "lslam_plicp_odom_stats"]


def test_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name in SYMBOLS:
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
    assert L.lslam_abi_version() == 5 and "#define LSLAM_ABI_VERSION 5" in header
    assert re.search(r"#define\s+LSLAM_PLICP_MAX_READINGS\s+2048\b", header) and api.PLICP_MAX_READINGS == 2048
    flat = re.sub(r"[\s*/]+", " ", header).lower()
    assert "parity with the reference is unpinned" in flat
    assert "among equal distances the lower sens order ranks first" in flat
    assert "here corr_ch is the identity" in flat                     # the invalid-match rule
    assert "a negative speed predicts nothing" in flat                # the literal prediction


def test_defaults_are_the_nodes():
    p = api.plicp_params()
    assert (p.max_angular_correction_deg, p.max_linear_correction, p.max_iterations, p.epsilon_xy, p.epsilon_theta) == \
        (45.0, 1.0, 10, 0.000001, 0.000001)
    assert (p.max_correspondence_dist, p.use_point_to_line_distance, p.outliers_maxPerc, p.outliers_adaptive_order,
            p.outliers_adaptive_mult, p.outliers_remove_doubles) == (1.0, 1, 0.90, 0.7, 2.0, 1)


def test_calls_without_a_handle_are_refused():
    L = api.lib()
    assert L.lslam_plicp_create(None, None, None) == -1  # LSLAM_ERR_INVALID_ARGUMENT
    assert L.lslam_plicp_set_laser(None, 0.0, 0.1, 0.1, 30.0) == -1
    assert L.lslam_plicp_stats(None, None) == -1
    for fn in (L.lslam_plicp_match_batch, L.lslam_plicp_match_batch_dev):
        assert fn(None, 0, 0, None, 0, 0, None, None, None, None) == -1
        assert fn(None, 2, 360, None, 360, 1, None, None, None, None) == -1
    assert L.lslam_plicp_debug_iteration(None, None, None, 0, None, None, None, None, None) == -1
    L.lslam_plicp_destroy(None)  # a no-op
    assert L.lslam_plicp_odom_create(None, None, 1, 0.1, 0.087, 10, None, None) == -1
    assert L.lslam_plicp_odom_set_laser(None, 0.0, 0.1, 0.1, 30.0) == -1
    assert L.lslam_plicp_odom_reset(None) == -1 and L.lslam_plicp_odom_state(None, None) == -1
    assert L.lslam_plicp_odom_stats(None, None) == -1
    assert L.lslam_plicp_odom_process_many(None, 1, 360, None, 360, None, None, None) == -1
    L.lslam_plicp_odom_destroy(None)


def test_the_record_is_48_bytes(tmp_path):
    assert api.PLICP_RECORD.itemsize == 48 and api.PLICP_RECORD.fields["valid"][1] == 32
    assert api.PLICP_ODOM_RECORD.itemsize == 80 and api.PLICP_ODOM_RECORD.fields["base_in_odom"][1] == 48
    src = tmp_path / "rec.c"
    src.write_text('#include <stddef.h>\n#include "lslam_gpu.h"\n'
                   '_Static_assert(sizeof(lslam_plicp_record) == 48, "48 bytes");\n'
                   '_Static_assert(offsetof(lslam_plicp_record, error) == 24, "error at 24");\n'
                   '_Static_assert(offsetof(lslam_plicp_record, nvalid) == 40, "nvalid at 40");\n'
                   '_Static_assert(sizeof(lslam_plicp_params) == 80, "80 bytes");\n'
                   '_Static_assert(sizeof(lslam_plicp_odom_record) == 80, "80 bytes");\n'
                   '_Static_assert(offsetof(lslam_plicp_odom_record, base_in_odom) == 48, "base_in_odom at 48");\n'
                   '_Static_assert(sizeof(lslam_plicp_odom_track) == 80, "80 bytes");\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), "-fsyntax-only", str(src)], check=True)
