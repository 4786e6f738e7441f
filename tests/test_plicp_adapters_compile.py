"""The C++ adapter over lesson3's PL-ICP (lslam::ScanMatchPLICPGpu, include/lslam_adapters.hpp) compiles stand-alone with g++
and links against liblslam_gpu.so.  No device needed; on a GPU box the little program also matches a pair."""
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
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    const int n = 360;
    const double pi = 3.14159265358979323846, inc = 2.0 * pi / n;
    std::vector<float> scans(3 * (size_t)n);
    const double pose[3][3] = {{0, 0, 0}, {0.1, 0.05, 0.02}, {0.2, 0.1, 0.04}};
    for (int k = 0; k < 3; k++)
      for (int i = 0; i < n; i++) scans[(size_t)k * n + i] = room(pose[k][0], pose[k][1], pose[k][2], -pi + i * inc);
    lslam::ScanMatchPLICPGpu plicp(ctx, -pi, inc, 0.1, 30.0);
    lslam_plicp_record r, batch[2];
    bad += plicp.ScanCallback(scans.data(), n, &r) ? 1 : 0;  // the first scan: nothing to match
    plicp.MatchConsecutive(3, n, scans.data(), n, batch);
    for (int k = 1; k < 3; k++) {
      bad += plicp.ScanCallback(scans.data() + (size_t)k * n, n, &r) ? 0 : 1;
      bad += std::memcmp(&r, &batch[k - 1], sizeof r) != 0;  // the callback == the batch, byte for byte
      std::printf("scan %d: valid %d, %d iterations, %d correspondences, x = %.6f %.6f %.6f\n", k, r.valid, r.iterations, r.nvalid,
                  r.x[0], r.x[1], r.x[2]);
      bad += r.valid != 1 || std::fabs(r.x[2] - 0.02) > 1e-4;
    }
    int64_t st[4];
    plicp.stats(st);
    bad += st[0] != 4 || st[1] != 3;
    bool threw = false;
    try {
      std::vector<float> big(2 * 2049, 1.0f);
      const int32_t a = 0, b = 1;
      plicp.MatchPairs(2, 2049, big.data(), 2049, 1, &a, &b, nullptr, &r);
    } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
  }
  lslam_destroy(ctx);
  std::printf("plicp adapter %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_plicp_adapter_compiles_and_links(tmp_path):
    exe = adapter_demo.build(tmp_path, "plicp_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_plicp_adapter_runs_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "plicp_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plicp adapter ok" in r.stdout
