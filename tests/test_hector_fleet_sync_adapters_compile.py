"""lslam::HectorSlamFleetGpu's gated forms (updateManyClouds, updateManyCloudsDev, updateManySynced; include/
lslam_adapters.hpp) compile stand-alone with g++ and link against liblslam_gpu.so.  No device needed; on a GPU box the little
program also runs two robots -- the second one step late -- through the three and compares their records with the members'
own updateManySynced."""
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
    const int n = 90, S = 6, R = 2, T = S + 1;  // robot 1 starts one step late: T steps
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
    lslam::LidarUndistortionGpu alone0(ctx), alone1(ctx), fleet0(ctx), fleet1(ctx), host0(ctx), host1(ctx);
    for (lslam::LidarUndistortionGpu* node : {&alone0, &alone1, &fleet0, &fleet1, &host0, &host1}) {
      node->ImuCallbacks((int)it.size(), it.data(), iw.data());
      node->OdomCallbacks((int)ot.size(), ot.data(), op.data(), oq.data());
    }
    // the members alone
    lslam::HectorSlamProcessorGpu a0(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 2), a1(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 3);
    std::vector<lslam_hector_record> r0(S), r1(S);
    std::vector<lslam_msync_record> s0(S), s1(S);
    a0.updateManySynced(alone0, scan, laser, S, n, ranges.data(), n, stamps.data(), tinc.data(), nullptr, nullptr, nullptr, nullptr,
                        r0.data(), s0.data());
    a1.updateManySynced(alone1, scan, laser, S, n, ranges.data(), n, stamps.data(), tinc.data(), nullptr, nullptr, nullptr, nullptr,
                        r1.data(), s1.data());
    // the fleet: robot 0 on steps 0 .. S-1, robot 1 on steps 1 .. S
    lslam::HectorSlamProcessorGpu b0(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 2), b1(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 3);
    lslam::HectorSlamProcessorGpu* members[R] = {&b0, &b1};
    lslam::HectorSlamFleetGpu fleet(ctx, members, R);
    std::vector<float> fr((size_t)T * R * n, 0.f), ft((size_t)T * R, 0.f);
    std::vector<double> fs((size_t)T * R, 0.0);
    std::vector<uint8_t> act((size_t)T * R, 0);
    for (int k = 0; k < S; k++)
      for (int m = 0; m < R; m++) {
        const size_t i = (size_t)(k + m) * R + m;
        std::memcpy(&fr[i * n], &ranges[(size_t)k * n], n * sizeof(float));
        fs[i] = stamps[k]; ft[i] = tinc[k]; act[i] = 1;
      }
    lslam::LidarUndistortionGpu* nodes[R] = {&fleet0, &fleet1};
    std::vector<lslam_hector_record> fo((size_t)T * R);
    std::vector<lslam_msync_record> fq((size_t)T * R);
    fleet.updateManySynced(nodes, scan, laser, T, n, fr.data(), n, fs.data(), ft.data(), nullptr, nullptr, nullptr, nullptr, act.data(),
                           fo.data(), fq.data());
    int taken = 0, refused = 0;
    for (int k = 0; k < S; k++) {
      bad += std::memcmp(&fo[(size_t)k * R], &r0[k], sizeof r0[k]) != 0;
      bad += std::memcmp(&fo[(size_t)(k + 1) * R + 1], &r1[k], sizeof r1[k]) != 0;
      bad += std::memcmp(&fq[(size_t)k * R], &s0[k], sizeof s0[k]) != 0;
      bad += std::memcmp(&fq[(size_t)(k + 1) * R + 1], &s1[k], sizeof s1[k]) != 0;
      taken += s0[k].status == LSLAM_MSYNC_CORRECTED;
      refused += s0[k].status < 0;
      std::printf("callback %d: status %d, record n_points %d updated %d\n", k, s0[k].status, r0[k].n_points, r0[k].updated);
    }
    bad += !(taken >= 2 && refused >= 1);
    bad += !(fo[1].n_points == -1 && fo[(size_t)S * R].n_points == -1);  // (step 0, robot 1) and (step S, robot 0): not active
    int64_t st[6], ss[4];
    fleet.stats(st);
    fleet.syncStats(ss);
    bad += !(st[5] == 4 * T && ss[0] == 1 && ss[1] == 5 && ss[3] == 1);
    // the cloud forms on the clouds the nodes' own host form gives, on fresh processors
    lslam::LidarUndistortionGpu::Clouds c0 = host0.ScanCallbacks(laser, S, n, ranges.data(), n, stamps.data(), tinc.data());
    lslam::LidarUndistortionGpu::Clouds c1 = host1.ScanCallbacks(laser, S, n, ranges.data(), n, stamps.data(), tinc.data());
    std::vector<float> fx((size_t)T * R * n * 3, 0.f);
    std::vector<uint8_t> fv((size_t)T * R * n, 0), take((size_t)T * R, 0);
    for (int k = 0; k < S; k++)
      for (int m = 0; m < R; m++) {
        const lslam::LidarUndistortionGpu::Clouds& c = m ? c1 : c0;
        const size_t i = (size_t)(k + m) * R + m;
        std::memcpy(&fx[i * n * 3], &c.xyz[(size_t)k * n * 3], (size_t)n * 3 * sizeof(float));
        std::memcpy(&fv[i * n], &c.valid[(size_t)k * n], (size_t)n);
        take[i] = c.records[k].status == LSLAM_MSYNC_CORRECTED;
      }
    lslam::HectorSlamFleetGpu fleet2(ctx, R, 0.05f, 512, 512, 0.5f, 0.5f, 2);
    std::vector<lslam_hector_record> go((size_t)T * R), gd((size_t)T * R);
    fleet2.updateManyClouds(scan, T, n, fx.data(), fv.data(), take.data(), nullptr, nullptr, act.data(), go.data());
    for (int k = 0; k < S; k++) bad += std::memcmp(&go[(size_t)k * R], &r0[k], sizeof r0[k]) != 0;  // (robot 0: the 2-level map)
    // ... and from HBM: one block per member, step-major rows, the take words inside uploaded lslam_msync_records
    lslam::HectorSlamFleetGpu fleet3(ctx, R, 0.05f, 512, 512, 0.5f, 0.5f, 2);
    void *dx[R], *dv[R], *dr[R];
    const float* px[R]; const uint8_t* pv[R]; const int32_t* pt[R];
    for (int m = 0; m < R; m++) {
      std::vector<float> x((size_t)T * n * 3);
      std::vector<uint8_t> v((size_t)T * n);
      std::vector<lslam_msync_record> q((size_t)T);
      std::memset(q.data(), 0, q.size() * sizeof q[0]);
      for (int k = 0; k < T; k++) {
        const size_t i = (size_t)k * R + m;
        std::memcpy(&x[(size_t)k * n * 3], &fx[i * n * 3], (size_t)n * 3 * sizeof(float));
        std::memcpy(&v[(size_t)k * n], &fv[i * n], (size_t)n);
        q[(size_t)k].status = take[i] ? LSLAM_MSYNC_CORRECTED : LSLAM_MSYNC_WAIT_IMU;
      }
      bad += lslam_dev_alloc(ctx, x.size() * sizeof(float), &dx[m]) != LSLAM_OK;
      bad += lslam_dev_alloc(ctx, v.size(), &dv[m]) != LSLAM_OK;
      bad += lslam_dev_alloc(ctx, q.size() * sizeof q[0], &dr[m]) != LSLAM_OK;
      bad += lslam_dev_upload(ctx, dx[m], x.data(), x.size() * sizeof(float)) != LSLAM_OK;
      bad += lslam_dev_upload(ctx, dv[m], v.data(), v.size()) != LSLAM_OK;
      bad += lslam_dev_upload(ctx, dr[m], q.data(), q.size() * sizeof q[0]) != LSLAM_OK;
      px[m] = (const float*)dx[m]; pv[m] = (const uint8_t*)dv[m]; pt[m] = &((const lslam_msync_record*)dr[m])->status;
    }
    fleet3.updateManyCloudsDev(scan, T, n, px, pv, pt, (int)(sizeof(lslam_msync_record) / 4), nullptr, nullptr, act.data(), gd.data());
    bad += std::memcmp(go.data(), gd.data(), go.size() * sizeof go[0]) != 0;
    for (int m = 0; m < R; m++) {
      lslam_dev_free(ctx, dx[m]);
      lslam_dev_free(ctx, dv[m]);
      lslam_dev_free(ctx, dr[m]);
    }
  }
  lslam_destroy(ctx);
  std::printf("hector fleet sync adapters %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_hector_fleet_sync_adapters_compile_and_link(tmp_path):
    exe = adapter_demo.build(tmp_path, "hector_fleet_sync_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_hector_fleet_sync_adapters_run_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "hector_fleet_sync_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hector fleet sync adapters ok" in r.stdout
