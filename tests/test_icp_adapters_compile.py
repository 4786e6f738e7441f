"""The C++ adapters over lesson2's ICP (lslam::ScanMatchICPGpu, lslam::ScanToPointCloud2ConverterGpu,
include/lslam_adapters.hpp) compile stand-alone with g++ and link against liblslam_gpu.so.  No device needed; on a GPU box the
little program also converts a scan and matches a pair."""
import pytest

import adapter_demo

SRC = r'''
#include <cstdio>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "lslam_adapters.hpp"
static float room(double x, double y, double th, double a) {  // a 6 m square room seen from (x, y, th)
  double c = std::cos(th + a), s = std::sin(th + a);
  double tx = ((c > 0 ? 3.0 : -3.0) - x) / c, ty = ((s > 0 ? 3.0 : -3.0) - y) / s;
  return (float)std::fmin(tx, ty);
}
int main(int argc, char**) {
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    const int n = 360;
    const double pi = 3.14159265358979323846, inc = 2.0 * pi / n;
    std::vector<float> scans(3 * (size_t)n);
    const double pose[3][3] = {{0, 0, 0}, {0.02, 0.01, 0.004}, {0.04, 0.02, 0.008}};
    for (int k = 0; k < 3; k++)
      for (int i = 0; i < n; i++) scans[(size_t)k * n + i] = room(pose[k][0], pose[k][1], pose[k][2], -pi + i * inc);
    scans[7] = std::numeric_limits<float>::infinity();  // an invalid reading: the origin for the matcher, NaN for the converter
    lslam::ScanMatchICPGpu icp(ctx, -pi, inc, 0.1, 30.0);
    lslam_icp_record r, batch[2];
    bad += icp.ScanCallback(scans.data(), n, &r) ? 1 : 0;  // the first scan: nothing to match
    icp.MatchConsecutive(3, n, scans.data(), n, batch);
    for (int k = 1; k < 3; k++) {
      bad += icp.ScanCallback(scans.data() + (size_t)k * n, n, &r) ? 0 : 1;
      bad += std::memcmp(&r, &batch[k - 1], sizeof r) != 0;  // the callback == the batch, byte for byte
      std::printf("scan %d: converged %d, state %d, %d iterations, %d correspondences, x = %.6f %.6f %.6f\n", k, r.converged, r.state,
                  r.iterations, r.ncorr, r.x[0], r.x[1], r.x[2]);
      bad += r.converged != 1 || r.ncorr != n || std::fabs(r.x[2] + 0.004) > 0.01 || std::hypot(r.x[0], r.x[1]) > 0.1;
    }
    int64_t st[4];
    icp.stats(st);
    bad += st[0] != 4 || st[1] != 6;  // 4 pairs; a conversion and a match launch per call
    bool threw = false;
    try {
      std::vector<float> big(2 * 2049, 1.0f);
      const int32_t a = 0, b = 1;
      icp.MatchPairs(2, 2049, big.data(), 2049, 1, &a, &b, nullptr, &r);
    } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
    lslam::ScanToPointCloud2ConverterGpu conv(ctx, -pi, inc, 0.1, 30.0);
    std::vector<float> xyz(3 * (size_t)n);
    std::vector<uint8_t> valid(n);
    conv.ScanCallback(scans.data(), n, xyz.data(), valid.data());
    bad += valid[7] != 0 || !std::isnan(xyz[21]) || !std::isnan(xyz[23]) || valid[8] != 1 || xyz[26] != 0.0f;
    bad += std::fabs(xyz[24] - scans[8] * std::cos((float)-pi + 8 * (float)inc)) > 1e-5;
  }
  lslam_destroy(ctx);
  std::printf("icp adapters %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_icp_adapters_compile_and_link(tmp_path):
    exe = adapter_demo.build(tmp_path, "icp_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_icp_adapters_run_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "icp_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "icp adapters ok" in r.stdout
