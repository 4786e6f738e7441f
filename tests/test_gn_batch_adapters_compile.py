"""MapRepGpu::matchDataBatch (include/lslam_adapters.hpp) compiles stand-alone with g++ and links against
liblslam_gpu.so; on a GPU box the little program also runs a batch through it and compares with matchData."""
import pytest

import adapter_demo

SRC = r'''
#include <cstdio>
#include <cmath>
#include <vector>
#include "lslam_adapters.hpp"
int main(int argc, char**) {
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    lslam::MapRepGpu map(ctx, 0.05f, 512, 512, 3, 0.5f, 0.5f);
    std::vector<float> pts;  // a square room, 6 m a side, seen from its middle (map-cell units)
    for (int i = 0; i < 720; i++) {
      double a = i * (2.0 * 3.14159265358979 / 720.0), c = std::cos(a), s = std::sin(a);
      double r = 3.0 / std::fmax(std::fabs(c), std::fabs(s)) / 0.05;
      pts.push_back((float)(r * c)); pts.push_back((float)(r * s));
    }
    const float origo[2] = {0, 0}, pose[3] = {0, 0, 0};
    float p1[3], c1[9];
    for (int k = 0; k < 4; k++) {
      map.matchData(pose, pts.data(), 720, origo, p1, c1);
      map.updateByScan(pts.data(), 720, origo, pose);
    }
    const float begins[3][3] = {{0.04f, -0.03f, 0.01f}, {-0.05f, 0.02f, -0.02f}, {0.0f, 0.0f, 0.0f}};
    const int32_t n_points[1] = {720}, entry_container[3] = {0, 0, 0};
    float poses[9], covs[27];
    map.matchDataBatch(3, &begins[0][0], 1, pts.data(), n_points, entry_container, poses, covs);
    for (int e = 0; e < 3; e++) {
      map.matchData(begins[e], pts.data(), 720, origo, p1, c1);
      for (int q = 0; q < 3; q++) bad += !(std::fabs(poses[3 * e + q] - p1[q]) <= 1e-4f);
      std::printf("entry %d: %.5f %.5f %.5f\n", e, poses[3 * e], poses[3 * e + 1], poses[3 * e + 2]);
    }
    bool threw = false;
    const int32_t wrong[3] = {0, 1, 0};
    try { map.matchDataBatch(3, &begins[0][0], 1, pts.data(), n_points, wrong, poses, nullptr); } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
  }
  lslam_destroy(ctx);
  std::printf("batch %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_match_data_batch_adapter_compiles_and_links(tmp_path):
    exe = adapter_demo.build(tmp_path, "gn_batch_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_match_data_batch_adapter_runs_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "gn_batch_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch ok" in r.stdout
