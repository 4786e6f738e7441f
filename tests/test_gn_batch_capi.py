"""The batched Gauss-Newton match in the C ABI: declared in the header, exported by the built library, refused without a
map -- no device needed."""
import ctypes as C
import pathlib
import re

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("lslam_map_match_batch", "lslam_map_match_batch_dev")


def test_batch_match_is_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*lslam_map\s*\*" % name, header), name
        assert hasattr(L, name), name
    assert L.lslam_abi_version() == 5


def test_batch_match_without_a_map_is_refused():
    L = api.lib()
    one = (C.c_float * 12)()
    cnt = (C.c_int32 * 1)(0)
    for name in SYMBOLS:
        fn = getattr(L, name)
        assert fn(None, 1, 1, None, cnt, None, one, one, None) == -1  # LSLAM_ERR_INVALID_ARGUMENT
        assert fn(None, 0, 0, None, None, None, None, None, None) == -1
