"""The cloud forms of lesson3's PL-ICP in the C ABI: declared in the header, exported by the built library, refused without a
handle or without their arrays, and the header states the rules a cloud is read by.  No device needed."""
import pathlib
import re

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ["lslam_plicp_match_clouds", "lslam_plicp_match_clouds_dev", "lslam_plicp_debug_iteration_clouds",
           "lslam_plicp_odom_process_many_clouds", "lslam_plicp_odom_process_many_clouds_dev"]


def test_the_five_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
    flat = re.sub(r"[\s*/]+", " ", header).lower()
    assert flat.count("scan_match_plicp.cc:220-300") >= 2 and "plicp_odometry.cc" in flat
    for rule in ("and x[i], y[i] are finite", "the float32 values widened", "z is ignored, nan included", "no range window",
                 "the reading index is i", "taken iff the word is > 0", "changes nothing of its track"):
        assert rule in flat, rule


def test_the_python_layer_has_the_five_methods():
    for cls, names in ((api.PlicpMatcher, ("match_clouds", "match_clouds_dev", "debug_iteration_clouds")),
                       (api.PlicpOdometry, ("process_many_clouds", "process_many_clouds_dev"))):
        for n in names:
            assert callable(getattr(cls, n)), n


def test_calls_without_a_handle_or_arrays_are_refused():
    L = api.lib()
    for fn in (L.lslam_plicp_match_clouds, L.lslam_plicp_match_clouds_dev):
        assert fn(None, 0, 0, None, None, 0, None, None, None, None) == -1  # LSLAM_ERR_INVALID_ARGUMENT
        assert fn(None, 2, 360, None, None, 1, None, None, None, None) == -1
    assert L.lslam_plicp_debug_iteration_clouds(None, None, None, None, None, 0, None, None, None, None, None) == -1
    assert L.lslam_plicp_odom_process_many_clouds(None, 1, 360, None, None, None, None, None, None) == -1
    assert L.lslam_plicp_odom_process_many_clouds_dev(None, 1, 360, None, None, None, 22, None, None, None) == -1
