"""lslam::HectorSlamFleetGpu (include/lslam_adapters.hpp) compiles stand-alone with g++ and links against liblslam_gpu.so: a
fleet that owns its processors, a fleet that borrows the caller's, update() for one step in the reference's container and
pose shapes.  Compile-only: without a GPU the little program reports "no device" and exits 0."""
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
// one step for every member, in the shapes of HectorSlamProcessor::update (HectorSlamProcessor.h:81)
void (lslam::HectorSlamFleetGpu::*kUpdate)(const Container*, const Vec3*, bool, const bool*, lslam_hector_record*) =
    &lslam::HectorSlamFleetGpu::update<Container, Vec3>;
int main(int argc, char**) {
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    Container room;  // a square room, 6 m a side, seen from its middle (map-cell units)
    for (int i = 0; i < 720; i++) {
      double a = i * (2.0 * 3.14159265358979 / 720.0), co = std::cos(a), si = std::sin(a);
      double r = 3.0 / std::fmax(std::fabs(co), std::fabs(si)) / 0.05;
      room.pts.push_back(Vec2{{(float)(r * co), (float)(r * si)}});
    }
    lslam::HectorSlamFleetGpu fleet(ctx, 3, 0.05f, 512, 512, 0.5f, 0.5f, 3);
    for (int r = 0; r < fleet.size(); r++) fleet.member(r).setUpdateFactorOccupied(0.9f);
    std::vector<Container> conts(3, room);
    std::vector<Vec3> hints(3, Vec3{{0.f, 0.f, 0.f}});
    const bool two[3] = {true, false, true};
    lslam_hector_record rec[3];
    fleet.update(conts.data(), hints.data(), true, two, rec);  // mapping only; member 1 sits the step out
    bad += !(rec[0].updated == 1 && rec[1].n_points == -1 && rec[2].n_points == 720);
    fleet.update(conts.data(), hints.data());
    float pose[3];
    fleet.member(0).getLastScanMatchPose(pose);
    bad += !(std::fabs(pose[0]) < 0.01f && std::fabs(pose[1]) < 0.01f);
    int64_t st[6];
    fleet.stats(st);
    bad += !(st[0] == 2 && st[1] == 5 && st[3] == 2 && st[4] == 2 && st[5] == 6);
    // the caller's own processors, of different maps, borrowed
    lslam::HectorSlamProcessorGpu a(ctx, 0.05f, 512, 512, 0.5f, 0.5f, 3), b(ctx, 0.1f, 256, 256, 0.5f, 0.5f, 1);
    lslam::HectorSlamProcessorGpu* both[2] = {&a, &b};
    lslam::HectorSlamFleetGpu borrowed(ctx, both, 2);
    borrowed.update(conts.data(), hints.data(), true);
    std::vector<float> plane(256 * 256);
    b.mapRep().readLogOdds(0, plane.data());
    int hits = 0;
    for (float v : plane) hits += v > 0.0f;
    bad += !(hits > 100);
    std::printf("steps %lld, launches %lld, occupied cells of the borrowed member %d\n", (long long)st[0], (long long)st[5], hits);
  }
  lslam_destroy(ctx);
  std::printf("fleet %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_fleet_adapter_compiles_and_links(tmp_path):
    exe = adapter_demo.build(tmp_path, "hector_fleet_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0; with one it runs
    assert "no device" in r.stdout or "fleet ok" in r.stdout, r.stdout
