"""The live occupancy map's C ABI (lslam_frontend_livemap_create / lslam_livemap_*): exported, and its argument checks answer
without a device.  CPU only."""
import ctypes as C

from lslam_amd import api

INVALID = -1  # LSLAM_ERR_INVALID_ARGUMENT
NAMES = ("lslam_frontend_livemap_create", "lslam_livemap_destroy", "lslam_livemap_update", "lslam_livemap_grid",
         "lslam_livemap_stats")


def test_livemap_symbols_are_exported():
    L = api.lib()
    assert [n for n in NAMES if not hasattr(L, n)] == []
    assert L.lslam_abi_version() == 5


def test_livemap_null_arguments_need_no_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.lslam_frontend_livemap_create(None, 0.05, C.byref(h)) == INVALID
    assert not h.value
    # a NULL `out` is refused before the front-end is looked at (the handle is never dereferenced)
    not_a_frontend = C.create_string_buffer(64)
    assert L.lslam_frontend_livemap_create(C.cast(not_a_frontend, C.c_void_p), 0.05, None) == INVALID
    assert L.lslam_livemap_update(None) == INVALID
    assert L.lslam_livemap_stats(None, None) == INVALID
    assert L.lslam_livemap_grid(None) is None
    L.lslam_livemap_destroy(None)  # no-op
