"""MapRepGpu::getLikelihoodForStates / getCovarianceForPoses / scoreLattice (include/lslam_adapters.hpp) compile stand-alone
with g++ and link against liblslam_gpu.so; on a GPU box the little program also runs the three and holds them to one another."""
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
    const float states[3][3] = {{0.0f, 0.0f, 0.0f}, {0.2f, -0.1f, 0.05f}, {100.0f, 100.0f, 0.0f}};
    const int32_t n_points[1] = {720}, entry_container[3] = {0, 0, 0};
    float lik[3], res[3];
    map.getLikelihoodForStates(3, &states[0][0], 1, pts.data(), n_points, entry_container, 0, lik, res);
    std::printf("likelihoods %.4f %.4f %.4f\n", lik[0], lik[1], lik[2]);
    bad += !(lik[0] > 0.5f && lik[0] > lik[1] && lik[2] == 0.0f && res[2] == 720.0f);
    float l7[7], cm[9], cw[9];
    map.getCovarianceForPoses(1, states[0], 1, pts.data(), n_points, nullptr, 0, l7, cm, cw);
    bad += std::memcmp(&l7[6], &lik[0], sizeof(float)) != 0;  // the seventh sigma point is the pose itself
    bad += !(cm[0] > 0.0f && cm[4] > 0.0f && cm[8] > 0.0f && std::fabs(cw[0] - cm[0] * 0.0025f) <= 1e-6f * cm[0]);
    const int32_t counts[3] = {3, 3, 3};
    const float steps[3] = {0.2f, 0.2f, 0.05f};
    float vol[27], best_lik = 0.0f;
    const int best = map.scoreLattice(pts.data(), 720, states[0], counts, steps, 0, vol, &best_lik);
    bad += !(best == 13 && std::memcmp(&vol[13], &lik[0], sizeof(float)) == 0 && best_lik == vol[13]);
    bool threw = false;
    try { map.getLikelihoodForStates(3, &states[0][0], 1, pts.data(), n_points, entry_container, 3, lik); } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
  }
  lslam_destroy(ctx);
  std::printf("score %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_score_adapters_compile_and_link(tmp_path):
    exe = adapter_demo.build(tmp_path, "score_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_score_adapters_run_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "score_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "score ok" in r.stdout
