"""lslam::HectorLocalizerGpu and MapRepGpu::writeLogOdds[Dev] (include/lslam_adapters.hpp) compile stand-alone with g++ and
link against liblslam_gpu.so: a map built by updateByScan, snapshot into a second map in HBM, three trackers localising on the
copy in the reference's container and pose shapes.  Compile-only: without a GPU the little program reports "no device" and
exits 0."""
import adapter_demo

SRC = r'''
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>
#include "lslam_adapters.hpp"
struct Vec2 { float v[2]; float operator[](int i) const { return v[i]; } };
struct Container {  // the surface of hectorslam::DataContainer that update() reads
  std::vector<Vec2> pts;
  int getSize() const { return (int)pts.size(); }
  const Vec2& getVecEntry(int i) const { return pts[(size_t)i]; }
};
struct Vec3 { float v[3]; float operator[](int i) const { return v[i]; } };
void (lslam::HectorLocalizerGpu::*kUpdate)(const Container*, const Vec3*, const bool*, lslam_hector_record*) =
    &lslam::HectorLocalizerGpu::update<Container, Vec3>;
int main(int argc, char**) {
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    Container room;  // a square room, 6 m a side, seen from its middle (map-cell units)
    std::vector<float> flat;
    for (int i = 0; i < 720; i++) {
      double a = i * (2.0 * 3.14159265358979 / 720.0), co = std::cos(a), si = std::sin(a);
      double r = 3.0 / std::fmax(std::fabs(co), std::fabs(si)) / 0.05;
      room.pts.push_back(Vec2{{(float)(r * co), (float)(r * si)}});
      flat.push_back((float)(r * co));
      flat.push_back((float)(r * si));
    }
    lslam::MapRepGpu built(ctx, 0.05f, 512, 512, 3, 0.5f, 0.5f), copy(ctx, 0.05f, 512, 512, 3, 0.5f, 0.5f);
    built.setUpdateFactorOccupied(0.9f);
    const float zero2[2] = {0.f, 0.f}, zero3[3] = {0.f, 0.f, 0.f};
    float pose[3], cov[9];
    built.matchData(zero3, flat.data(), 720, zero2, pose, cov);  // caches the container for the levels above 0
    for (int k = 0; k < 3; k++) built.updateByScan(flat.data(), 720, zero2, zero3);
    std::vector<float> a(512 * 512), b(512 * 512);
    copy.writeLogOddsDev(0, (const float*)lslam_map_cells_dev_ptr(built.handle(), 0));  // level 0 in HBM, the others by the host
    for (int lv = 1; lv < 3; lv++) {
      built.readLogOdds(lv, a.data());
      copy.writeLogOdds(lv, a.data());
    }
    built.readLogOdds(0, a.data());
    copy.readLogOdds(0, b.data());
    bad += std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) != 0;
    lslam::HectorLocalizerGpu loc(ctx, copy, 3);
    const float start[9] = {0.02f, 0.f, 0.f, 0.f, 0.03f, 0.f, 0.f, 0.f, 0.01f};
    loc.setPoses(0, 3, start);
    std::vector<Container> conts(3, room);
    const bool two[3] = {true, false, true};
    lslam_hector_record rec[3];
    loc.update<Container, Vec3>(conts.data(), nullptr, two, rec);  // chained from the poses set; tracker 1 sits the step out
    bad += !(rec[0].n_points == 720 && rec[1].n_points == -1 && rec[2].n_points == 720 && rec[0].updated == 0);
    bad += !(std::fabs(rec[0].pose[0]) < 0.015f && std::fabs(rec[0].pose[1]) < 0.015f);  // started 0.02 m off
    loc.getLastScanMatchPose(1, pose);
    bad += !(pose[0] == 0.f && pose[1] == 0.03f);  // untouched
    int64_t st[6];
    loc.stats(st);
    bad += !(st[0] == 1 && st[1] == 2 && st[2] == 1 && st[3] == 1 && st[4] == 1 && st[5] == 1);
    copy.readLogOdds(0, b.data());
    bad += std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) != 0;  // the map is only read
    std::printf("pose %g %g %g, launches %lld\n", rec[0].pose[0], rec[0].pose[1], rec[0].pose[2], (long long)st[4]);
  }
  lslam_destroy(ctx);
  std::printf("localizer %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_localizer_adapter_compiles_and_links(tmp_path):
    exe = adapter_demo.build(tmp_path, "hector_loc_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0; with one it runs
    assert "no device" in r.stdout or "localizer ok" in r.stdout, r.stdout
