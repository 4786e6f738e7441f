"""lslam::OccupancyGridRayCaster (include/lslam_adapters.hpp) compiles stand-alone with g++ and links against liblslam_gpu.so,
and integration/karto_occupancy_grid_gpu.hpp -- the old CreateOccupancyGridFromScans and the overload that also hands back the
live device grid -- compiles with the reference's own Karto.h present.  Compile-only: without a GPU the little program reports
"no device" and exits 0."""
import pathlib
import subprocess

import pytest

import adapter_demo

ROOT = pathlib.Path(__file__).resolve().parent.parent
KARTO = pathlib.Path("/root/reference/lesson6/lib/open_karto")
SRC = r'''
#include <cmath>
#include <cstdio>
#include <vector>
#include "lslam_adapters.hpp"
// the reference's shape with plain doubles
double (lslam::OccupancyGridRayCaster::*kRayCast)(double, double, double, double) const = &lslam::OccupancyGridRayCaster::RayCast;
int main(int argc, char**) {
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    // a 3 m square room seen from its middle by a 1440-beam laser (several beams through every cell: a cell passed twice or less stays unknown), one scan
    lslam_laser laser = {-3.14159265358979, 3.14159265358979, 2.0 * 3.14159265358979 / 1440.0, 0.1, 30.0, 20.0, 0.0, 0.0, 0.0};
    std::vector<double> ranges(1440), pose(3, 0.0);
    for (int i = 0; i < 1440; i++) {
      double a = laser.minimum_angle + i * laser.angular_resolution;
      ranges[i] = 1.5 / std::fmax(std::fabs(std::cos(a)), std::fabs(std::sin(a)));
    }
    lslam_occgrid* og = nullptr;
    rc = lslam_occgrid_create_from_scans(ctx, &laser, 1, ranges.data(), 1440, pose.data(), 0.05, &og);
    bad += rc != LSLAM_OK;
    lslam::OccupancyGridRayCaster caster(ctx, og);
    const double d = caster.RayCast(0.0, 0.0, 0.3, 5.0);
    bad += !(d > 1.2 && d < 1.8);   // the wall, not maxRange
    std::vector<lslam::Pose2> poses(3);
    poses[1].heading = 1.0; poses[2].x = 0.4; poses[2].heading = -2.0;
    std::vector<double> many = caster.RayCastMany(poses, 5.0), per = caster.RayCastMany(poses, std::vector<double>(3, 5.0));
    bad += !(many.size() == 3 && many == per && many[0] > 1.2 && many[0] < 1.7);
    int beams = 0;
    std::vector<double> scans = caster.RayCastScans(laser, poses, 5.0, &beams);
    bad += !(beams == 1440 && scans.size() == 3 * 1440);
    double worst = 0.0;   // the map predicts the scan it was built from to within a few cells
    for (int i = 0; i < 1440; i++) worst = std::fmax(worst, std::fabs(scans[i] - ranges[i]));
    bad += !(worst < 0.25);
    std::vector<int64_t> st = caster.Stats();
    bad += !(st[0] == 4 && st[1] == 1 + 3 + 3 + 3 * 1440 && st[2] == 1 && st[3] > 0);
    std::printf("RayCast %.4f, worst |predicted - measured| %.4f, samples %lld\n", d, worst, (long long)st[3]);
    lslam_occgrid_destroy(og);
  }
  lslam_destroy(ctx);
  std::printf("raycaster %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''
KARTO_SRC = r'''
#include "karto_occupancy_grid_gpu.hpp"
#include "lslam_adapters.hpp"
// the call site's function keeps its signature; the overload also hands back the device grid
karto::OccupancyGrid* (*kOld)(lslam_context*, const karto::LocalizedRangeScanVector&, kt_double) = &lslam::CreateOccupancyGridFromScans;
karto::OccupancyGrid* (*kNew)(lslam_context*, const karto::LocalizedRangeScanVector&, kt_double, lslam_occgrid**) =
    &lslam::CreateOccupancyGridFromScans;
double probe(lslam_context* ctx, const karto::LocalizedRangeScanVector& scans, const karto::Pose2& p) {
  lslam_occgrid* og = NULL;
  karto::OccupancyGrid* host = lslam::CreateOccupancyGridFromScans(ctx, scans, 0.05, &og);
  if (!host) return -1.0;
  const double on_host = host->RayCast(p, 12.0);   // the reference's own, on the copy
  const double on_device = lslam::OccupancyGridRayCaster(ctx, og).RayCast(p.GetX(), p.GetY(), p.GetHeading(), 12.0);
  delete host;
  lslam_occgrid_destroy(og);
  return on_host - on_device;
}
'''


def test_raycaster_adapter_compiles_and_links(tmp_path):
    exe = adapter_demo.build(tmp_path, "raycaster_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0; with one it runs
    assert "no device" in r.stdout or "raycaster ok" in r.stdout, r.stdout


def test_integration_overload_compiles_against_the_references_header(tmp_path):
    if not (KARTO / "include" / "open_karto" / "Karto.h").exists():
        pytest.skip("the reference's headers are absent")
    src = tmp_path / "karto_raycast_seam.cpp"
    src.write_text(KARTO_SRC)
    subprocess.run(["g++", "-std=c++14", "-O1", "-w", "-I", str(ROOT / "oracle" / "shim"), "-I", str(KARTO / "include"),
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "integration"), "-c", str(src), "-o", str(tmp_path / "seam.o")],
                   check=True)
