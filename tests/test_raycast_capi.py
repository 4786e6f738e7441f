"""The batched ray cast in the C ABI: declared in the header beside the other lslam_occgrid_* entry points, each citing the
reference's RayCast, exported by the built library, and arguments refused before anything touches a device -- no GPU needed."""
import ctypes as C
import pathlib
import re

import numpy as np

from lslam_amd import api, synth

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("lslam_occgrid_ray_cast", "lslam_occgrid_ray_cast_dev", "lslam_occgrid_ray_cast_scans", "lslam_occgrid_ray_cast_scans_dev",
           "lslam_occgrid_ray_cast_stats")
INVALID = -1  # LSLAM_ERR_INVALID_ARGUMENT


def test_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    section = header[header.index("int lslam_livemap_stats"):header.index("int lslam_occgrid_ray_cast_stats")]
    assert section.count("Karto.h:5717-5755") >= len(SYMBOLS)   # every entry cites the reference's RayCast
    assert header.index("lslam_occgrid_create_from_scans") < header.index("lslam_occgrid_ray_cast") < header.index("lslam_map_create")
    assert L.lslam_abi_version() == 5  # additive: the ABI version does not move
    for cls in (api.OccupancyGrid, api._OccupancyGridView):   # LiveMap.grid() inherits them
        for method in ("ray_cast", "ray_cast_scans", "ray_cast_stats", "ray_cast_dev", "ray_cast_scans_dev"):
            assert callable(getattr(cls, method)), (cls, method)


def test_null_and_negative_arguments_are_refused_without_a_device():
    L = api.lib()
    p, out = np.zeros((2, 3)), np.zeros(2)
    laser = api.laser_params(synth.Laser())
    for fn in (L.lslam_occgrid_ray_cast, L.lslam_occgrid_ray_cast_dev):
        assert fn(None, 2, p.ctypes.data, None, 1.0, out.ctypes.data) == INVALID
        assert fn(None, -1, p.ctypes.data, None, 1.0, out.ctypes.data) == INVALID
        assert fn(None, 2, None, None, 1.0, None) == INVALID
        assert fn(None, 0, None, None, 1.0, None) == INVALID
    for fn in (L.lslam_occgrid_ray_cast_scans, L.lslam_occgrid_ray_cast_scans_dev):
        assert fn(None, laser, 2, p.ctypes.data, 1.0, out.ctypes.data, 1081) == INVALID
        assert fn(None, None, -2, None, 1.0, None, 0) == INVALID
    st = (C.c_int64 * 4)()
    assert L.lslam_occgrid_ray_cast_stats(None, st) == INVALID
    assert L.lslam_occgrid_ray_cast_stats(None, None) == INVALID
