"""lslam_msync in the C ABI: declared in the header with the reference lines each entry stands for, exported by the built
library, the record and header structs of the size the bindings assume, and argument refusals that need no device."""
import ctypes as C
import pathlib
import re

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = {
    "lslam_msync_create": r"int\s+lslam_msync_create\s*\(\s*lslam_context\s*\*\s*\w+,\s*int\s+use_imu,\s*int\s+use_odom,\s*lslam_msync\s*\*\*",
    "lslam_msync_destroy": r"void\s+lslam_msync_destroy\s*\(\s*lslam_msync\s*\*",
    "lslam_msync_reset": r"int\s+lslam_msync_reset\s*\(\s*lslam_msync\s*\*",
    "lslam_msync_push_imu": r"int\s+lslam_msync_push_imu\s*\(\s*lslam_msync\s*\*\s*\w+,\s*int\s+n,\s*const\s+double\s*\*\s*stamps,\s*const\s+double\s*\*\s*gyro_xyz",
    "lslam_msync_push_odom": r"int\s+lslam_msync_push_odom\s*\(\s*lslam_msync\s*\*\s*\w+,\s*int\s+n,\s*const\s+double\s*\*\s*stamps,\s*const\s+double\s*\*\s*pos_xyz,\s*const\s+double\s*\*\s*quat_xyzw",
    "lslam_msync_scans": r"int\s+lslam_msync_scans\s*\(\s*lslam_msync\s*\*\s*\w+,\s*lslam_deskew\s*\*",
    "lslam_msync_scans_dev": r"int\s+lslam_msync_scans_dev\s*\(\s*lslam_msync\s*\*\s*\w+,\s*lslam_deskew\s*\*",
    "lslam_msync_read_windows": r"int\s+lslam_msync_read_windows\s*\(\s*lslam_msync\s*\*",
    "lslam_msync_stats": r"int\s+lslam_msync_stats\s*\(\s*lslam_msync\s*\*",
}


def header():
    return (ROOT / "include" / "lslam_gpu.h").read_text()


def test_symbols_are_declared_and_exported():
    text, L = header(), api.lib()
    for name, decl in SYMBOLS.items():
        assert re.search(r"\b" + decl, text), name
        assert hasattr(L, name), name


def test_the_section_cites_the_reference_lines():
    text = header()
    a = text.index("lesson5 IMU / odometry synchronisation")
    section = text[a:text.index("lesson4 GMapping hit/visit count map")]
    for lines in (":82-86", ":89-93", ":96-125", ":142-156", ":182-188", ":191-197", ":257-263", ":266-272", ":237", ":301-302",
                  ":332-334"):
        assert lines in section, lines


def test_statuses_and_struct_sizes():
    text = header()
    for name, value in (("QUEUED", 0), ("CORRECTED", 1), ("WAIT_IMU", -1), ("WAIT_ODOM", -2), ("IMU_NO_LEAD_SAMPLE", -3),
                        ("IMU_OVERFLOW", -4), ("QUEUE_LENGTH", 2000)):
        m = re.search(r"#define\s+LSLAM_MSYNC_%s\s+\(?(-?\d+)\)?" % name, text)
        assert m and int(m.group(1)) == value, name
        assert getattr(api, "MSYNC_" + name) == value
    assert api.MSYNC_RECORD.itemsize == 88 and C.sizeof(api.MsyncLaser) == 16
    fields = re.search(r"typedef struct lslam_msync_record \{(.*?)\} lslam_msync_record;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip().split("[")[0] for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(api.MSYNC_RECORD.names), names
    assert api.MSYNC_RECORD.fields["imu_front"][1] == 56 and api.MSYNC_RECORD.fields["odom_incre"][1] == 40


def test_calls_without_a_handle_are_refused():
    L = api.lib()
    INVALID = -1  # LSLAM_ERR_INVALID_ARGUMENT
    assert L.lslam_msync_create(None, 1, 1, None) == INVALID
    h = C.c_void_p()
    assert L.lslam_msync_create(None, 1, 1, C.byref(h)) == INVALID and not h
    assert L.lslam_msync_reset(None) == INVALID
    assert L.lslam_msync_push_imu(None, 1, None, None) == INVALID
    assert L.lslam_msync_push_odom(None, 1, None, None, None) == INVALID
    for fn in (L.lslam_msync_scans, L.lslam_msync_scans_dev):
        assert fn(None, None, None, 0, 0, None, 0, None, None, None, None, None, None, None) == INVALID
    assert L.lslam_msync_read_windows(None, None, None, None, 0) == INVALID
    assert L.lslam_msync_stats(None, None) == INVALID
    L.lslam_msync_destroy(None)  # a no-op


def test_the_product_links_nothing_from_the_oracle():
    import subprocess

    from lslam_amd import build
    out = subprocess.run(["ldd", str(build.build_library())], capture_output=True, text=True).stdout
    assert "oracle" not in out and "_ref" not in out, out
