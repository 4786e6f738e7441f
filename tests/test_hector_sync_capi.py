"""The gated forms of the streamed processor in the C ABI: lslam_hector_process_many_clouds, _clouds_dev and _synced are
declared in the header with the signatures the bindings assume and the reference lines they stand for, exported by the built
library, and refuse NULL handles without a device."""
import pathlib
import re

from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
S = r"\s*"
P = r"\s*\*\s*"  # a pointer declarator
SYMBOLS = {
    "lslam_hector_process_many_clouds":
        r"int\s+lslam_hector_process_many_clouds\s*\(" + S + "lslam_hector" + P + r"h," + S + r"const\s+lslam_hector_scan" + P +
        r"scan," + S + r"int\s+n_scans," + S + r"int\s+n_points," + S + r"const\s+float" + P + r"xyz," + S + r"const\s+uint8_t" + P +
        r"valid," + S + r"const\s+uint8_t" + P + r"take," + S + r"const\s+float" + P + r"pose_hints," + S + r"const\s+uint8_t" + P +
        r"map_without_matching," + S + "lslam_hector_record" + P + r"out" + S + r"\)",
    "lslam_hector_process_many_clouds_dev":
        r"int\s+lslam_hector_process_many_clouds_dev\s*\(" + S + "lslam_hector" + P + r"h," + S + r"const\s+lslam_hector_scan" + P +
        r"scan," + S + r"int\s+n_scans," + S + r"int\s+n_points," + S + r"const\s+float" + P + r"xyz_dev," + S +
        r"const\s+uint8_t" + P + r"valid_dev," + S + r"const\s+int32_t" + P + r"take_dev," + S + r"int\s+take_stride," + S +
        r"const\s+float" + P + r"pose_hints," + S + r"const\s+uint8_t" + P + r"map_without_matching," + S + "lslam_hector_record" +
        P + r"out" + S + r"\)",
    "lslam_hector_process_many_synced":
        r"int\s+lslam_hector_process_many_synced\s*\(" + S + "lslam_hector" + P + r"h," + S + r"(struct\s+)?lslam_msync" + P +
        r"sync," + S + r"const\s+lslam_hector_scan" + P + r"scan," + S + r"const\s+(struct\s+)?lslam_msync_laser" + P + r"laser," +
        S + r"int\s+n_msgs," + S + r"int\s+n_readings," + S + r"const\s+float" + P + r"ranges," + S + r"int\s+ranges_stride," + S +
        r"const\s+double" + P + r"stamps," + S + r"const\s+float" + P + r"time_increments," + S + r"const\s+int64_t" + P +
        r"imu_seen," + S + r"const\s+int64_t" + P + r"odom_seen," + S + r"const\s+float" + P + r"pose_hints," + S +
        r"const\s+uint8_t" + P + r"map_without_matching," + S + "lslam_hector_record" + P + r"out," + S +
        r"(struct\s+)?lslam_msync_record" + P + r"sync_records" + S + r"\)",
}


def header():
    return (ROOT / "include" / "lslam_gpu.h").read_text()


def section(text):
    a = text.index("GATED forms")
    return text[a:text.index("getLastScanMatchPose / getLastScanMatchCovariance", a)]


def test_symbols_are_declared_and_exported():
    text, L = section(header()), api.lib()
    for name, decl in SYMBOLS.items():
        assert re.search(r"\b" + decl, text), name
        assert hasattr(L, name), name


def test_the_section_stands_next_to_the_deskewed_form_and_cites_the_reference_lines():
    text = header()
    assert text.index("int lslam_hector_process_many_deskewed") < text.index("GATED forms") < text.index("int lslam_hector_state")
    sec = section(text)
    for lines in ("HectorSlamProcessor.h:81-108", "hector_slam.cc:320-362", "lidar_undistortion.cc:96-125", ":142-156"):
        assert lines in sec, lines
    assert "n_points = -1" in sec and "sizeof(lslam_msync_record) / 4 (22)" in sec
    assert api.MSYNC_RECORD.itemsize // 4 == 22 and api.MSYNC_RECORD.fields["status"][1] == 0
    assert api.MSYNC_CORRECTED == 1 and api.MSYNC_QUEUED == 0


def test_calls_without_a_handle_are_refused():
    L = api.lib()
    INVALID = -1  # LSLAM_ERR_INVALID_ARGUMENT
    assert L.lslam_hector_process_many_clouds(None, None, 1, 1, None, None, None, None, None, None) == INVALID
    assert L.lslam_hector_process_many_clouds_dev(None, None, 1, 1, None, None, None, 1, None, None, None) == INVALID
    assert L.lslam_hector_process_many_synced(None, None, None, None, 1, 1, None, 1, None, None, None, None, None, None, None,
                                              None) == INVALID


def test_the_bindings_exist():
    for name in ("process_many_clouds", "process_many_clouds_dev", "process_synced"):
        assert callable(getattr(api.HectorProcessor, name)), name
    text = (ROOT / "include" / "lslam_adapters.hpp").read_text()
    for name in ("updateManyClouds", "updateManyCloudsDev", "updateManySynced"):
        assert re.search(r"\bvoid\s+(HectorSlamProcessorGpu::)?%s\s*\(" % name, text), name
