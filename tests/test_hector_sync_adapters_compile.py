"""lslam::HectorSlamProcessorGpu's gated forms (updateManyClouds, updateManyCloudsDev, updateManySynced; include/
lslam_adapters.hpp) compile stand-alone with g++ and link against liblslam_gpu.so.  No device needed; on a GPU box the little
program also runs a log with a refused scan through the three and compares their records."""
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
    lslam_hector_scan scan = {laser.angle_min, laser.angle_increment, laser.range_min, laser.range_max, 30.0f, 0.16f, 900.0f, 20.0f,
                              -1.0f, 2.0f, 0.0f, 0.0f, 0.0f, 0.0f};
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
    // IMU at 200 Hz with a hole over scan 2 (10.2 .. 10.28 s) that reaches callback 3: PruneImuDeque refuses that scan
    std::vector<double> it, iw, ot, op, oq;
    for (int j = 0; j < 260; j++) {
      double t = 9.7 + 0.005 * j;
      if (t > 10.15 && t < 10.45) continue;
      it.push_back(t); iw.push_back(0.0); iw.push_back(0.0); iw.push_back(0.5);
    }
    for (int j = 0; j < 28; j++) {
      double t = 9.7 + 0.05 * j, yaw = 0.3 * (t - 9.7);
      ot.push_back(t);
      op.push_back(1.0 + 0.5 * (t - 9.7)); op.push_back(-1.0); op.push_back(0.0);
      oq.push_back(0.0); oq.push_back(0.0); oq.push_back(std::sin(yaw / 2)); oq.push_back(std::cos(yaw / 2));
    }
    lslam::LidarUndistortionGpu nodeA(ctx), nodeB(ctx);
    for (lslam::LidarUndistortionGpu* node : {&nodeA, &nodeB}) {
      node->ImuCallbacks((int)it.size(), it.data(), iw.data());
      node->OdomCallbacks((int)ot.size(), ot.data(), op.data(), oq.data());
    }
    lslam::HectorSlamProcessorGpu a(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 2), b(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 2),
        c(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 2);
    std::vector<lslam_hector_record> ra(S), rb(S), rc3(S);
    std::vector<lslam_msync_record> sa(S);
    a.updateManySynced(nodeA, scan, laser, S, n, ranges.data(), n, stamps.data(), tinc.data(), nullptr, nullptr, nullptr, nullptr,
                       ra.data(), sa.data());
    lslam::LidarUndistortionGpu::Clouds cl = nodeB.ScanCallbacks(laser, S, n, ranges.data(), n, stamps.data(), tinc.data());
    bool take[S];
    int taken = 0, refused = 0;
    for (int k = 0; k < S; k++) {
      take[k] = cl.records[k].status == LSLAM_MSYNC_CORRECTED;
      taken += take[k];
      refused += cl.records[k].status < 0;
      std::printf("callback %d: status %d, record n_points %d updated %d\n", k, sa[k].status, ra[k].n_points, ra[k].updated);
    }
    b.updateManyClouds(scan, S, n, cl.xyz.data(), cl.valid.data(), take, nullptr, nullptr, rb.data());
    void *dx = nullptr, *dv = nullptr, *dr = nullptr;
    bad += lslam_dev_alloc(ctx, cl.xyz.size() * sizeof(float), &dx) != LSLAM_OK;
    bad += lslam_dev_alloc(ctx, cl.valid.size(), &dv) != LSLAM_OK;
    bad += lslam_dev_alloc(ctx, (size_t)S * sizeof(lslam_msync_record), &dr) != LSLAM_OK;
    bad += lslam_dev_upload(ctx, dx, cl.xyz.data(), cl.xyz.size() * sizeof(float)) != LSLAM_OK;
    bad += lslam_dev_upload(ctx, dv, cl.valid.data(), cl.valid.size()) != LSLAM_OK;
    bad += lslam_dev_upload(ctx, dr, cl.records.data(), (size_t)S * sizeof(lslam_msync_record)) != LSLAM_OK;
    c.updateManyCloudsDev(scan, S, n, (const float*)dx, (const uint8_t*)dv, &((const lslam_msync_record*)dr)->status,
                          (int)(sizeof(lslam_msync_record) / 4), nullptr, nullptr, rc3.data());
    bad += std::memcmp(sa.data(), cl.records.data(), (size_t)S * sizeof(lslam_msync_record)) != 0;
    bad += std::memcmp(ra.data(), rb.data(), (size_t)S * sizeof(lslam_hector_record)) != 0;
    bad += std::memcmp(ra.data(), rc3.data(), (size_t)S * sizeof(lslam_hector_record)) != 0;
    bad += !(taken >= 2 && refused >= 1 && taken + refused == S - 1);
    for (int k = 0; k < S; k++) bad += take[k] ? !(ra[k].n_points > 50) : !(ra[k].n_points == -1 && ra[k].updated == 0);
    lslam_dev_free(ctx, dx);
    lslam_dev_free(ctx, dv);
    lslam_dev_free(ctx, dr);
  }
  lslam_destroy(ctx);
  std::printf("hector sync adapters %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_hector_sync_adapters_compile_and_link(tmp_path):
    exe = adapter_demo.build(tmp_path, "hector_sync_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_hector_sync_adapters_run_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "hector_sync_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hector sync adapters ok" in r.stdout
