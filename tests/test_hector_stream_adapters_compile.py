"""lslam::HectorSlamProcessorGpu (include/lslam_adapters.hpp) compiles stand-alone with g++, links against liblslam_gpu.so and
has the reference's update(dataContainer, poseHintWorld, map_without_matching = false) shape; on a GPU box the little program
also maps and matches a few scans through it."""
import pytest

import adapter_demo

SRC = r'''
#include <cstdio>
#include <cmath>
#include <vector>
#include "lslam_adapters.hpp"
struct Vec2 { float v[2]; float operator[](int i) const { return v[i]; } };
struct Container {  // the surface of hectorslam::DataContainer that update() reads
  std::vector<Vec2> pts; Vec2 origo{{0.f, 0.f}};
  int getSize() const { return (int)pts.size(); }
  const Vec2& getVecEntry(int i) const { return pts[(size_t)i]; }
  const Vec2& getOrigo() const { return origo; }
};
struct Vec3 { float v[3]; float operator[](int i) const { return v[i]; } };
// the reference's signature (HectorSlamProcessor.h:81), the third argument defaulted
void (lslam::HectorSlamProcessorGpu::*kUpdate)(const Container&, const Vec3&, bool) = &lslam::HectorSlamProcessorGpu::update<Container, Vec3>;
int main(int argc, char**) {
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    lslam::HectorSlamProcessorGpu proc(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 3);
    Container c;  // a square room, 6 m a side, seen from its middle (map-cell units)
    for (int i = 0; i < 720; i++) {
      double a = i * (2.0 * 3.14159265358979 / 720.0), co = std::cos(a), si = std::sin(a);
      double r = 3.0 / std::fmax(std::fabs(co), std::fabs(si)) / 0.05;
      c.pts.push_back(Vec2{{(float)(r * co), (float)(r * si)}});
    }
    proc.setUpdateFactorOccupied(0.9f);
    Vec3 hint{{0.f, 0.f, 0.f}};
    for (int k = 0; k < 4; k++) proc.update(c, hint, true);   // mapping only: the pose is the hint, the map is updated
    Vec3 near{{0.02f, -0.01f, 0.005f}};
    proc.update(c, near);                 // matched back to the mapped pose; too close to it for an update
    float pose[3], upd[3];
    proc.getLastScanMatchPose(pose);
    proc.getLastMapUpdatePose(upd);
    for (int q = 0; q < 3; q++) bad += !(std::fabs(pose[q]) < 0.01f) + !(upd[q] == 0.0f);
    std::vector<float> plane(512 * 512);
    proc.mapRep().readLogOdds(0, plane.data());
    int hits = 0;
    for (float v : plane) hits += v > 0.0f;
    bad += !(hits > 400);
    std::printf("pose %.5f %.5f %.5f, occupied cells %d\n", pose[0], pose[1], pose[2], hits);
  }
  lslam_destroy(ctx);
  std::printf("processor %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_processor_adapter_compiles_and_links(tmp_path):
    exe = adapter_demo.build(tmp_path, "hector_stream_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_processor_adapter_runs_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "hector_stream_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "processor ok" in r.stdout
