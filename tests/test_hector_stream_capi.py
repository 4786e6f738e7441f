"""The streamed HectorSlamProcessor in the C ABI: declared in the header, exported by the built library, a 64-byte record, and
arguments refused before anything touches a device -- no GPU needed."""
import ctypes as C
import pathlib
import re

import numpy as np

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("lslam_hector_create", "lslam_hector_destroy", "lslam_hector_reset", "lslam_hector_set_update_thresholds",
           "lslam_hector_set_option", "lslam_hector_process_many", "lslam_hector_process_many_points", "lslam_hector_state",
           "lslam_hector_stats")
INVALID = -1  # LSLAM_ERR_INVALID_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name in SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    assert "HectorSlamProcessor.h:57-117" in header  # the entries cite the reference lines they restate
    assert L.lslam_abi_version() == 5


def test_record_is_64_bytes():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    body = re.search(r"typedef struct lslam_hector_record \{(.*?)\} lslam_hector_record;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    words = 0
    for kind, name, dim in re.findall(r"(float|int32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", body):
        words += int(dim or 1)
    assert words * 4 == 64
    assert api.HECTOR_RECORD.itemsize == 64
    assert [api.HECTOR_RECORD.fields[k][1] for k in ("pose", "cov", "updated", "n_points")] == [0, 12, 48, 52]


def test_null_and_negative_arguments_are_refused_without_a_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.lslam_hector_create(None, C.byref(h)) == INVALID
    assert L.lslam_hector_create(None, None) == INVALID
    L.lslam_hector_destroy(None)  # a no-op
    assert L.lslam_hector_reset(None) == INVALID
    assert L.lslam_hector_set_update_thresholds(None, 0.4, 0.13) == INVALID
    assert L.lslam_hector_set_option(None, 1, 1) == INVALID
    scan = api.HectorScan()
    r = np.zeros(8, np.float32)
    n = np.array([4], np.int32)
    assert L.lslam_hector_process_many(None, C.byref(scan), 1, 8, r.ctypes.data, 8, None, None, None) == INVALID
    assert L.lslam_hector_process_many(None, C.byref(scan), 0, 0, None, 0, None, None, None) == INVALID
    assert L.lslam_hector_process_many(None, C.byref(scan), -1, 8, r.ctypes.data, 8, None, None, None) == INVALID
    assert L.lslam_hector_process_many_points(None, 1, r.ctypes.data, n.ctypes.data, None, None, None, None) == INVALID
    assert L.lslam_hector_process_many_points(None, -1, None, None, None, None, None, None) == INVALID
    assert L.lslam_hector_state(None, None, None, None) == INVALID
    assert L.lslam_hector_stats(None, None) == INVALID
