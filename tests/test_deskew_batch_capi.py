"""The batched de-skew, the cloud -> container call and the streamed processor's de-skewed form in the C ABI: declared in the
header, exported by the built library, refused without a handle -- and the C++ adapters over them (lslam::
LidarUndistortionGpu, HectorSlamProcessorGpu::updateManyDeskewed, include/lslam_adapters.hpp) compile stand-alone with g++
and link against liblslam_gpu.so.  No device needed; on a GPU box the little program also runs a batch."""
import pathlib
import re

import pytest

import adapter_demo
from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = {
    "lslam_deskew_create": r"int\s+lslam_deskew_create\s*\(\s*lslam_context\s*\*",
    "lslam_deskew_destroy": r"void\s+lslam_deskew_destroy\s*\(\s*lslam_deskew\s*\*",
    "lslam_deskew_stats": r"int\s+lslam_deskew_stats\s*\(\s*const\s+lslam_deskew\s*\*",
    "lslam_deskew_batch": r"int\s+lslam_deskew_batch\s*\(\s*lslam_deskew\s*\*",
    "lslam_deskew_batch_dev": r"int\s+lslam_deskew_batch_dev\s*\(\s*lslam_deskew\s*\*",
    "lslam_map_set_cloud": r"int\s+lslam_map_set_cloud\s*\(\s*lslam_map\s*\*",
    "lslam_hector_process_many_deskewed": r"int\s+lslam_hector_process_many_deskewed\s*\(\s*lslam_hector\s*\*",
}


def test_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name, decl in SYMBOLS.items():
        assert re.search(r"\b" + decl, header), name
        assert hasattr(L, name), name
    assert L.lslam_abi_version() == 5
    assert "#define LSLAM_ABI_VERSION 5" in header or re.search(r"LSLAM_ABI_VERSION\s*=?\s*5\b", header)


def test_calls_without_a_handle_are_refused():
    L = api.lib()
    assert L.lslam_deskew_create(None, None) == -1  # LSLAM_ERR_INVALID_ARGUMENT
    assert L.lslam_deskew_stats(None, None) == -1
    for fn in (L.lslam_deskew_batch, L.lslam_deskew_batch_dev):
        assert fn(None, 0, 0, None, 0, None, None, None, None, None, None, None, None) == -1
    assert L.lslam_map_set_cloud(None, None, None, 0, None, None) == -1
    assert L.lslam_hector_process_many_deskewed(None, None, 0, 0, None, 0, None, None, None, None, None, None, None, None, None) == -1
    L.lslam_deskew_destroy(None)  # a no-op


SRC = r'''
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>
#include "lslam_adapters.hpp"
int main(int argc, char**) {
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    const int n = 360, B = 3;
    std::vector<float> ranges((size_t)B * n);
    for (int k = 0; k < B; k++)
      for (int i = 0; i < n; i++) {  // a square room, 6 m a side, seen from its middle
        double a = -3.14159265358979 + i * (2.0 * 3.14159265358979 / n), c = std::cos(a), s = std::sin(a);
        ranges[(size_t)k * n + i] = (float)(3.0 / std::fmax(std::fabs(c), std::fabs(s)));
      }
    std::vector<lslam_deskew_params> params(B);
    std::vector<int32_t> first(B + 1, 0);
    std::vector<double> t, rx, ry, rz;
    for (int k = 0; k < B; k++) {
      lslam_deskew_params& p = params[k];
      std::memset(&p, 0, sizeof p);
      p.angle_min = -3.14159265f; p.angle_increment = (float)(2.0 * 3.14159265358979 / n);
      p.range_min = 0.1f; p.range_max = 30.0f;
      p.scan_time_start = 10.0 + 0.12 * k; p.time_increment = 0.1 / n;
      p.use_imu = 1; p.use_odom = 1;
      p.start_odom_time = p.scan_time_start - 0.004; p.end_odom_time = p.scan_time_start + 0.1;
      p.odom_incre_x = 0.05f; p.odom_incre_y = 0.01f;
      for (int j = 0; j < 11 + k; j++) {
        t.push_back(p.scan_time_start - 0.003 + 0.01 * j); rx.push_back(0.0); ry.push_back(0.0); rz.push_back(0.004 * j);
      }
      first[k + 1] = (int32_t)t.size();
    }
    std::vector<float> xyz((size_t)B * n * 3), one((size_t)n * 3);
    std::vector<uint8_t> valid((size_t)B * n), v1(n);
    lslam::LidarUndistortionGpu deskew(ctx);
    deskew.CorrectLaserScans(B, n, ranges.data(), n, params.data(), first.data(), t.data(), rx.data(), ry.data(), rz.data(),
                             xyz.data(), valid.data());
    for (int k = 0; k < B; k++) {  // every scan of the batch == the single call, bit for bit
      rc = lslam_deskew_scan(ctx, ranges.data() + (size_t)k * n, n, &params[k], t.data() + first[k], rx.data() + first[k],
                             ry.data() + first[k], rz.data() + first[k], first[k + 1] - first[k], one.data(), v1.data());
      bad += rc != LSLAM_OK;
      bad += std::memcmp(one.data(), xyz.data() + (size_t)k * n * 3, one.size() * sizeof(float)) != 0;
      bad += std::memcmp(v1.data(), valid.data() + (size_t)k * n, n) != 0;
    }
    int64_t st[4];
    deskew.stats(st);
    std::printf("deskew: %lld scans, %lld launches, %lld growths, %lld waits\n", (long long)st[0], (long long)st[1],
                (long long)st[2], (long long)st[3]);
    bad += st[0] != B;
    lslam::HectorSlamProcessorGpu proc(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 2);
    lslam_hector_scan hs;
    std::memset(&hs, 0, sizeof hs);
    hs.sqr_laser_min_dist = 0.16f; hs.sqr_laser_max_dist = 900.0f; hs.use_max_scan_range = 20.0f;
    hs.laser_z_min = -1.0f; hs.laser_z_max = 2.0f;  // lesson5's cloud has z = 1
    std::vector<lslam_hector_record> rec(B);
    proc.updateManyDeskewed(hs, B, n, ranges.data(), n, params.data(), first.data(), t.data(), rx.data(), ry.data(), rz.data(),
                            nullptr, nullptr, rec.data());
    for (int k = 0; k < B; k++) {
      std::printf("scan %d: %d points, pose %.4f %.4f %.4f, updated %d\n", k, rec[k].n_points, rec[k].pose[0], rec[k].pose[1],
                  rec[k].pose[2], rec[k].updated);
      bad += rec[k].n_points != n;
      bad += !(std::isfinite(rec[k].pose[0]) && std::isfinite(rec[k].pose[1]) && std::isfinite(rec[k].pose[2]));
    }
    bad += rec[0].updated != 1;
    bool threw = false;  // one call, one geometry
    params[1].range_max = 25.0f;
    try {
      deskew.CorrectLaserScans(B, n, ranges.data(), n, params.data(), first.data(), t.data(), rx.data(), ry.data(), rz.data(),
                               xyz.data(), valid.data());
    } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
  }
  lslam_destroy(ctx);
  std::printf("deskew adapters %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_deskew_adapters_compile_and_link(tmp_path):
    exe = adapter_demo.build(tmp_path, "deskew_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_deskew_adapters_run_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "deskew_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "deskew adapters ok" in r.stdout
