"""The Hector fleet's gated forms in the C ABI: lslam_hector_fleet_process_many_clouds, _clouds_dev, _synced and
lslam_hector_fleet_sync_stats are declared in the header, exported by the built library, bound by api.HectorFleet, and refuse
NULL handles without a device -- no GPU needed."""
import ctypes as C
import pathlib
import re

import numpy as np

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("lslam_hector_fleet_process_many_clouds", "lslam_hector_fleet_process_many_clouds_dev",
           "lslam_hector_fleet_process_many_synced", "lslam_hector_fleet_sync_stats")
INVALID = -1  # LSLAM_ERR_INVALID_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?lslam_hector_fleet\s*\*\s*f\s*," % name, header), name
        assert hasattr(L, name), name
    assert re.search(r"lslam_hector_fleet_process_many_synced\s*\(\s*lslam_hector_fleet\s*\*\s*f,\s*struct\s+lslam_msync\s*\*\s*const\s*\*\s*syncs",
                     header)
    assert re.search(r"const\s+float\s*\*\s*const\s*\*\s*xyz_dev,\s*const\s+uint8_t\s*\*\s*const\s*\*\s*valid_dev,\s*"
                     r"const\s+int32_t\s*\*\s*const\s*\*\s*take_dev,\s*int\s+take_stride", header)
    assert L.lslam_abi_version() == 5  # additive: the ABI version does not move
    for name in ("process_many_clouds", "process_many_clouds_dev", "process_synced", "sync_stats"):
        assert callable(getattr(api.HectorFleet, name)), name
    text = (ROOT / "include" / "lslam_adapters.hpp").read_text()
    for name in ("updateManyClouds", "updateManyCloudsDev", "updateManySynced"):
        assert re.search(r"\bvoid\s+(HectorSlamFleetGpu::)?%s\s*\(" % name, text[text.index("class HectorSlamFleetGpu"):]), name


def test_calls_without_a_handle_are_refused_without_a_device():
    L = api.lib()
    scan, hdr = api.HectorScan(), api.MsyncLaser()
    x = np.zeros(24, np.float32)
    ptrs = (C.c_void_p * 2)(None, None)
    out = (C.c_int64 * 4)()
    assert L.lslam_hector_fleet_process_many_clouds(None, C.byref(scan), 1, 8, x.ctypes.data, None, None, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many_clouds(None, C.byref(scan), -1, 8, x.ctypes.data, None, None, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many_clouds_dev(None, C.byref(scan), 1, 8, ptrs, None, None, 1, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many_clouds_dev(None, C.byref(scan), 0, 0, None, None, None, 0, None, None, None, None) == INVALID
    t = np.zeros(1, np.float64)
    ti = np.zeros(1, np.float32)
    assert L.lslam_hector_fleet_process_many_synced(None, ptrs, C.byref(scan), C.byref(hdr), 1, 8, x.ctypes.data, 8, t.ctypes.data,
                                                    ti.ctypes.data, None, None, None, None, None, None, None) == INVALID
    assert L.lslam_hector_fleet_process_many_synced(None, None, None, None, 1, 1, None, 1, None, None, None, None, None, None, None,
                                                    None, None) == INVALID
    assert L.lslam_hector_fleet_sync_stats(None, out) == INVALID
    assert L.lslam_hector_fleet_sync_stats(None, None) == INVALID
