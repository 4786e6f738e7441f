"""The Hector fleet in the C ABI: declared in the header, exported by the built library, and arguments refused before anything
touches a device -- no GPU needed."""
import ctypes as C
import pathlib
import re

import numpy as np

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("lslam_hector_fleet_create", "lslam_hector_fleet_destroy", "lslam_hector_fleet_size", "lslam_hector_fleet_process_many",
           "lslam_hector_fleet_process_many_points", "lslam_hector_fleet_stats")
INVALID = -1  # LSLAM_ERR_INVALID_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    assert re.search(r"typedef\s+struct\s+lslam_hector_fleet\s+lslam_hector_fleet\s*;", header)  # the seventh name: the handle
    for name in SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    assert L.lslam_abi_version() == 5  # additive: the ABI version does not move
    assert hasattr(api, "HectorFleet")


def test_null_and_negative_arguments_are_refused_without_a_device():
    L = api.lib()
    f = C.c_void_p()
    members = (C.c_void_p * 2)(None, None)
    assert L.lslam_hector_fleet_create(None, 1, C.byref(f)) == INVALID
    assert L.lslam_hector_fleet_create(members, 2, None) == INVALID
    assert L.lslam_hector_fleet_create(members, 0, C.byref(f)) == INVALID   # n_members < 1
    assert L.lslam_hector_fleet_create(members, -3, C.byref(f)) == INVALID
    assert L.lslam_hector_fleet_create(members, 2, C.byref(f)) == INVALID   # NULL members
    assert not f.value
    L.lslam_hector_fleet_destroy(None)  # a no-op
    assert L.lslam_hector_fleet_size(None) == INVALID
    scan = api.HectorScan()
    r = np.zeros(8, np.float32)
    n = np.array([4], np.int32)
    assert L.lslam_hector_fleet_process_many(None, C.byref(scan), 1, 8, r.ctypes.data, 8, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many(None, C.byref(scan), 0, 0, None, 0, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many(None, C.byref(scan), -1, 8, r.ctypes.data, 8, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many(None, C.byref(scan), 1, -8, r.ctypes.data, 8, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many_points(None, 1, r.ctypes.data, n.ctypes.data, None, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many_points(None, -1, None, None, None, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_stats(None, None) == INVALID
    out = (C.c_int64 * 6)()
    assert L.lslam_hector_fleet_stats(None, out) == INVALID
