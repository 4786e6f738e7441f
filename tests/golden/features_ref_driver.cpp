// Drives the reference's own lesson1 LaserScan::ScanCallback (lesson1/src/feature_detection.cc) over a block of scans and
// writes what it PUBLISHES.  Our own source: the reference's file is only #included at build time, from the path
// tests/golden/make_features_golden.py passes as -DFEATURE_DETECTION_CC="\"...\"", behind the ROS stand-ins of oracle/shim.
//   in : int32 n_scans, n_readings, reps; float32 edge_threshold; n_scans x n_readings float32 ranges
//   out: n_scans x n_readings float32 (corner_scan.ranges' first n_readings entries); float64 CPU seconds per scan, the best
//        of `reps` passes over the block (0 when reps == 0)
// The headers the reference's file relies on without including them come first; the stand-in's Publisher::publish does
// nothing, so a macro copies the message out on its way in; edge_threshold_ is private and has no setter.
#include <algorithm>
#include <map>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include <ros/ros.h>
#include <sensor_msgs/LaserScan.h>

namespace ros {
inline void spin() {}
}  // namespace ros

static sensor_msgs::LaserScan g_published;
template <class M>
static const M& keep_published(const M& m) {
  g_published = m;
  return m;
}
#define publish(x) publish(keep_published(x))
#define private public
#define main ref_main
#include FEATURE_DETECTION_CC
#undef main
#undef private
#undef publish

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[3];
  float thr = 0.f;
  if (std::fread(hdr, sizeof(int32_t), 3, in) != 3 || std::fread(&thr, sizeof(float), 1, in) != 1) return 2;
  const int n_scans = hdr[0], n = hdr[1], reps = hdr[2];
  if (n_scans < 0 || n < 0 || n > max_scan_count) return 2;
  std::vector<float> ranges((size_t)n_scans * n);
  if (std::fread(ranges.data(), sizeof(float), ranges.size(), in) != ranges.size()) return 2;
  std::fclose(in);

  LaserScan node;
  node.edge_threshold_ = thr;
  std::vector<std::shared_ptr<sensor_msgs::LaserScan>> msgs;
  for (int k = 0; k < n_scans; k++) {
    auto m = std::make_shared<sensor_msgs::LaserScan>();
    m->ranges.assign(ranges.begin() + (size_t)k * n, ranges.begin() + (size_t)(k + 1) * n);
    msgs.push_back(m);
  }
  std::vector<float> out((size_t)n_scans * n);
  for (int k = 0; k < n_scans; k++) {
    node.ScanCallback(msgs[k]);
    std::copy(g_published.ranges.begin(), g_published.ranges.begin() + n, out.begin() + (size_t)k * n);
  }
  double best = 0.0;
  for (int r = 0; r < reps && n_scans > 0; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < n_scans; k++) node.ScanCallback(msgs[k]);
    const double per = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / n_scans;
    if (r == 0 || per < best) best = per;
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(out.data(), sizeof(float), out.size(), o);
  std::fwrite(&best, sizeof(double), 1, o);
  std::fclose(o);
  return 0;
}
