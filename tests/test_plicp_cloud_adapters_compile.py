"""The cloud forms in the C++ adapters (lslam::ScanMatchPLICPGpu::MatchClouds[Dev], lslam::PlicpOdometryGpu::ProcessClouds[Dev],
include/lslam_adapters.hpp) compile stand-alone with g++ and link against liblslam_gpu.so.  No device needed; on a GPU box the
little program also matches clouds against their ranges and runs a gated odometry."""
import pytest

import adapter_demo

SRC = r'''
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>
#include "lslam_adapters.hpp"
static float room(double x, double y, double th, double a) {  // a 6 m square room seen from (x, y, th)
  double c = std::cos(th + a), s = std::sin(th + a);
  double tx = ((c > 0 ? 3.0 : -3.0) - x) / c, ty = ((s > 0 ? 3.0 : -3.0) - y) / s;
  return (float)std::fmin(tx, ty);
}
int main(int argc, char**) {
  // the Dev forms only have to compile and link here
  void (lslam::ScanMatchPLICPGpu::*dev1)(int, int, const float*, const uint8_t*, int, const int32_t*, const int32_t*, const double*,
                                         lslam_plicp_record*) = &lslam::ScanMatchPLICPGpu::MatchCloudsDev;
  void (lslam::PlicpOdometryGpu::*dev2)(int, int, const float* const*, const uint8_t* const*, const int32_t* const*, int,
                                        const double*, const uint8_t*, lslam_plicp_odom_record*) =
      &lslam::PlicpOdometryGpu::ProcessCloudsDev;
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return (argc > 1 || !dev1 || !dev2) ? 1 : 0; }
  int bad = 0;
  {
    const int n = 360, K = 4;
    const double pi = 3.14159265358979323846, inc = 2.0 * pi / n;
    std::vector<float> xyz(K * (size_t)n * 3, 0.0f);
    std::vector<uint8_t> valid(K * (size_t)n, 1);
    const double pose[K][3] = {{0, 0, 0}, {0.05, 0.02, 0.01}, {0.1, 0.04, 0.02}, {0.15, 0.06, 0.03}};
    for (int k = 0; k < K; k++)
      for (int i = 0; i < n; i++) {
        const double a = -pi + i * inc, r = room(pose[k][0], pose[k][1], pose[k][2], a);
        xyz[((size_t)k * n + i) * 3] = (float)(r * std::cos(a));
        xyz[((size_t)k * n + i) * 3 + 1] = (float)(r * std::sin(a));
      }
    lslam::ScanMatchPLICPGpu plicp(ctx, -pi, inc, 0.1, 30.0);
    const int32_t ref[3] = {0, 1, 2}, sens[3] = {1, 2, 3};
    lslam_plicp_record with[3], without[3];
    plicp.MatchClouds(K, n, xyz.data(), valid.data(), 3, ref, sens, nullptr, with);
    plicp.MatchClouds(K, n, xyz.data(), nullptr, 3, ref, sens, nullptr, without);
    bad += std::memcmp(with, without, sizeof with) != 0;  // all-ones bytes == no bytes
    for (int k = 0; k < 3; k++) {
      std::printf("pair %d: valid %d, %d iterations, %d correspondences, x = %.6f %.6f %.6f\n", k, with[k].valid, with[k].iterations,
                  with[k].nvalid, with[k].x[0], with[k].x[1], with[k].x[2]);
      bad += with[k].valid != 1 || std::fabs(with[k].x[2] - 0.01) > 1e-4;
    }
    // the odometry: callback 1 refused through take
    lslam::PlicpOdometryGpu odo(ctx, 1, -pi, inc, 0.1, 30.0);
    const double stamps[K] = {0.0, 0.1, 0.2, 0.3};
    const uint8_t take[K] = {1, 0, 1, 1};
    lslam_plicp_odom_record rec[K];
    odo.ProcessClouds(K, n, xyz.data(), valid.data(), take, stamps, nullptr, rec);
    bad += rec[0].flags != 3 || rec[1].iterations != -1 || rec[2].valid != 1 || rec[3].valid != 1;
    bad += std::fabs(rec[3].base_in_odom[0] - 0.15) > 1e-4 || std::fabs(rec[3].base_in_odom[2] - 0.03) > 1e-4;
    bool threw = false;
    try {
      std::vector<float> ranges(n, 1.0f);
      odo.ScanCallback(ranges.data(), n, 0.4, rec);  // a range call after a cloud call
    } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
    threw = false;
    try {
      std::vector<float> big(2 * 2049 * 3, 1.0f);
      const int32_t a = 0, b = 1;
      plicp.MatchClouds(2, 2049, big.data(), nullptr, 1, &a, &b, nullptr, with);
    } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
  }
  lslam_destroy(ctx);
  std::printf("plicp cloud adapter %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_plicp_cloud_adapter_compiles_and_links(tmp_path):
    exe = adapter_demo.build(tmp_path, "plicp_cloud_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_plicp_cloud_adapter_runs_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "plicp_cloud_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plicp cloud adapter ok" in r.stdout
