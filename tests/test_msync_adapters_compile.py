"""lslam::LidarUndistortionGpu's node shape (ImuCallback, OdomCallback, ScanCallback, ScanCallbacks; include/
lslam_adapters.hpp) compiles stand-alone with g++ and links against liblslam_gpu.so.  No device needed; on a GPU box the little
program also runs a log through the callbacks, one message at a time and as a stretch, and compares the two."""
import pytest

import adapter_demo

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
    const int n = 90, S = 6;
    const double kPi = 3.14159265358979;
    lslam_msync_laser laser = {(float)-kPi, (float)(2.0 * kPi / n), 0.1f, 30.0f};
    std::vector<float> ranges((size_t)S * n);
    std::vector<double> stamps(S);
    std::vector<float> tinc(S, (float)(0.08 / (n - 1)));
    for (int k = 0; k < S; k++) {
      stamps[k] = 10.0 + 0.1 * k;
      for (int i = 0; i < n; i++) {
        double a = -kPi + i * (2.0 * kPi / n);
        ranges[(size_t)k * n + i] = (float)(3.0 / std::fmax(std::fabs(std::cos(a)), std::fabs(std::sin(a))));
      }
    }
    std::vector<double> it, iw, ot, op, oq;
    for (int j = 0; j < 260; j++) { it.push_back(9.7 + 0.005 * j); iw.push_back(0.0); iw.push_back(0.0); iw.push_back(0.5); }
    for (int j = 0; j < 28; j++) {
      double t = 9.7 + 0.05 * j, yaw = 0.3 * (t - 9.7);
      ot.push_back(t);
      op.push_back(1.0 + 0.5 * (t - 9.7)); op.push_back(-1.0); op.push_back(0.0);
      oq.push_back(0.0); oq.push_back(0.0); oq.push_back(std::sin(yaw / 2)); oq.push_back(std::cos(yaw / 2));
    }
    lslam::LidarUndistortionGpu one(ctx, true, true), many(ctx);
    for (size_t j = 0; j < it.size(); j++) one.ImuCallback(it[j], iw[3 * j], iw[3 * j + 1], iw[3 * j + 2]);
    for (size_t j = 0; j < ot.size(); j++) one.OdomCallback(ot[j], &op[3 * j], &oq[4 * j]);
    many.ImuCallbacks((int)it.size(), it.data(), iw.data());
    many.OdomCallbacks((int)ot.size(), ot.data(), op.data(), oq.data());
    lslam::LidarUndistortionGpu::Clouds all = many.ScanCallbacks(laser, S, n, ranges.data(), n, stamps.data(), tinc.data());
    std::vector<float> xyz((size_t)n * 3);
    std::vector<uint8_t> valid(n);
    for (int k = 0; k < S; k++) {
      lslam_msync_record r = one.ScanCallback(laser, n, ranges.data() + (size_t)k * n, stamps[k], tinc[k], xyz.data(), valid.data());
      std::printf("callback %d: status %d, %d samples, incre %.6f %.6f\n", k, r.status, r.n_imu, r.odom_incre[0], r.odom_incre[1]);
      bad += r.status != (k == 0 ? LSLAM_MSYNC_QUEUED : LSLAM_MSYNC_CORRECTED);
      bad += std::memcmp(&r, &all.records[k], sizeof r) != 0;
      bad += std::memcmp(xyz.data(), all.xyz.data() + (size_t)k * n * 3, xyz.size() * sizeof(float)) != 0;
      bad += std::memcmp(valid.data(), all.valid.data() + (size_t)k * n, n) != 0;
      if (k > 0) bad += !(valid[0] == 1 && std::isfinite(xyz[0]) && r.n_imu > 10 && r.odom_incre[0] > 0.01f);
    }
    int64_t st[6];
    many.syncStats(st);
    bad += !(st[0] == S && st[1] == S - 1 && st[2] == 0 && st[3] == 3);
    bool threw = false;  // scan_count_ is the first scan's
    try {
      many.ScanCallbacks(laser, 1, n - 1, ranges.data(), n, stamps.data(), tinc.data());
    } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
    many.Reset();
    many.syncStats(st);
    bad += st[0] != 0;
  }
  lslam_destroy(ctx);
  std::printf("msync adapters %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_msync_adapters_compile_and_link(tmp_path):
    exe = adapter_demo.build(tmp_path, "msync_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_msync_adapters_run_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "msync_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "msync adapters ok" in r.stdout
