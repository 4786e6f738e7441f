"""The map write and the Hector localiser in the C ABI: declared in the header, exported by the built library, and arguments
refused before anything touches a device -- no GPU needed."""
import ctypes as C
import pathlib
import re

import numpy as np

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("lslam_map_write_logodds", "lslam_map_write_logodds_dev", "lslam_hector_loc_create", "lslam_hector_loc_destroy",
           "lslam_hector_loc_size", "lslam_hector_loc_set_poses", "lslam_hector_loc_state", "lslam_hector_loc_set_option",
           "lslam_hector_loc_process_many", "lslam_hector_loc_process_many_points", "lslam_hector_loc_process_many_clouds",
           "lslam_hector_loc_process_many_clouds_dev", "lslam_hector_loc_stats")
INVALID = -1  # LSLAM_ERR_INVALID_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    assert re.search(r"typedef\s+struct\s+lslam_hector_loc\s+lslam_hector_loc\s*;", header)
    assert re.search(r"LSLAM_HECTOR_LOC_OPT_MAX_STEPS_PER_LAUNCH\s*=\s*1\b", header)
    for name in SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    assert L.lslam_abi_version() == 5  # additive: the ABI version does not move
    assert re.search(r"#define\s+LSLAM_ABI_VERSION\s+5\b", header)
    assert hasattr(api, "HectorLocaliser")
    for method in ("write_logodds", "write_logodds_dev", "save", "load"):
        assert hasattr(api.OccGridMap, method), method
    for method in ("process_many", "process_many_points", "process_many_clouds", "process_many_clouds_dev", "set_poses", "state",
                   "stats", "set_option"):
        assert hasattr(api.HectorLocaliser, method), method


def test_map_write_refuses_null_without_a_device():
    L = api.lib()
    plane = np.zeros(4, np.float32)
    assert L.lslam_map_write_logodds(None, 0, plane.ctypes.data) == INVALID
    assert L.lslam_map_write_logodds(None, -1, plane.ctypes.data) == INVALID
    assert L.lslam_map_write_logodds(None, 0, None) == INVALID
    assert L.lslam_map_write_logodds_dev(None, 0, plane.ctypes.data) == INVALID
    assert L.lslam_map_write_logodds_dev(None, 0, None) == INVALID


def test_localiser_refuses_null_negative_and_out_of_range_without_a_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.lslam_hector_loc_create(None, 1, C.byref(h)) == INVALID
    assert L.lslam_hector_loc_create(None, 0, C.byref(h)) == INVALID    # n_trackers < 1
    assert L.lslam_hector_loc_create(None, -2, C.byref(h)) == INVALID
    assert L.lslam_hector_loc_create(None, 1, None) == INVALID
    assert not h.value
    L.lslam_hector_loc_destroy(None)  # a no-op
    assert L.lslam_hector_loc_size(None) == INVALID
    p = np.zeros(3, np.float32)
    cov = np.zeros(9, np.float32)
    assert L.lslam_hector_loc_set_poses(None, 0, 1, p.ctypes.data) == INVALID
    assert L.lslam_hector_loc_set_poses(None, -1, 1, p.ctypes.data) == INVALID
    assert L.lslam_hector_loc_set_poses(None, 0, -1, p.ctypes.data) == INVALID
    assert L.lslam_hector_loc_state(None, 0, p.ctypes.data, cov.ctypes.data) == INVALID
    assert L.lslam_hector_loc_state(None, -1, p.ctypes.data, cov.ctypes.data) == INVALID
    assert L.lslam_hector_loc_set_option(None, 1, 4) == INVALID
    scan = api.HectorScan()
    r = np.zeros(8, np.float32)
    n = np.array([4], np.int32)
    out = np.zeros(1, api.HECTOR_RECORD)
    o = out.ctypes.data
    assert L.lslam_hector_loc_process_many(None, C.byref(scan), 1, 8, r.ctypes.data, 8, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many(None, C.byref(scan), 0, 8, r.ctypes.data, 8, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many(None, C.byref(scan), -1, 8, r.ctypes.data, 8, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many(None, C.byref(scan), 1, -8, r.ctypes.data, 8, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many(None, C.byref(scan), 1, 0, r.ctypes.data, 8, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many_points(None, 1, r.ctypes.data, n.ctypes.data, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many_points(None, -1, None, None, None, None, None) == INVALID
    assert L.lslam_hector_loc_process_many_clouds(None, C.byref(scan), 1, 2, r.ctypes.data, None, None, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many_clouds(None, C.byref(scan), -1, 2, r.ctypes.data, None, None, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many_clouds(None, C.byref(scan), 1, -2, r.ctypes.data, None, None, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many_clouds_dev(None, C.byref(scan), 1, 2, None, None, None, 1, None, None, o) == INVALID
    assert L.lslam_hector_loc_process_many_clouds_dev(None, C.byref(scan), 1, -2, None, None, None, 0, None, None, o) == INVALID
    assert L.lslam_hector_loc_stats(None, None) == INVALID
    st = (C.c_int64 * 6)()
    assert L.lslam_hector_loc_stats(None, st) == INVALID
