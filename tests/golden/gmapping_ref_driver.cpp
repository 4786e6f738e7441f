// Drives the reference's GMapping map classes (lesson4/include/lesson4/gmapping/grid: ScanMatcherMap, PointAccumulator,
// HierarchicalArray2D, GridLineTraversal) through the lesson4_gmapping_node callback sequence, restated here:
// CreateCache once, then per callback a fresh ScanMatcherMap, the ComputeMap loop (filter, clamp, endpoint, gridLine,
// active area, setActiveArea + allocActiveArea, free updates, then hits) and the PublishMap loop.  Built and run by
// make_gmapping_golden.py and tests/test_gmapping_pin.py against the reference's headers; nothing here is linked into
// the library.
//
//   driver line <in> <out>   in: int32 n, n x (x0, y0, x1, y1); out: per pair int32 num_points, then the points
//   driver map <in> <out>    in: see read_map_input; out: see the end of run_map
//
// Beyond the node (our contract): several scans at poses into ONE map (endpoint
// x + d (c cos_i - s sin_i), y + d (s cos_i + c sin_i)), cells outside the storage skipped and counted, and the published
// width taken with the double delta (the node's float32 MapMetaData.resolution gives 1599 columns for a 1600-cell storage
// and its loop then writes past data's end).
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "lesson4/gmapping/grid/gridlinetraversal.h"
#include "lesson4/gmapping/grid/map.h"

using namespace gmapping;

namespace {

FILE* open_or_die(const char* path, const char* mode) {
  FILE* f = std::fopen(path, mode);
  if (!f) {
    std::perror(path);
    std::exit(2);
  }
  return f;
}
template <typename T>
void rd(FILE* f, T* p, size_t n) {
  if (std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short input\n");
    std::exit(2);
  }
}
template <typename T>
void wr(FILE* f, const T* p, size_t n) {
  std::fwrite(p, sizeof(T), n, f);
}

int run_lines(const char* in, const char* out) {
  FILE* fi = open_or_die(in, "rb");
  int32_t n;
  rd(fi, &n, 1);
  std::vector<int32_t> q(4 * (size_t)n);
  rd(fi, q.data(), q.size());
  std::fclose(fi);
  FILE* fo = open_or_die(out, "wb");
  for (int i = 0; i < n; i++) {
    GridLineTraversalLine line;
    GridLineTraversal::gridLine(IntPoint(q[4 * i], q[4 * i + 1]), IntPoint(q[4 * i + 2], q[4 * i + 3]), &line);
    const int32_t np = line.num_points;
    wr(fo, &np, 1);
    for (int k = 0; k < np; k++) {
      const int32_t xy[2] = {line.points[k].x, line.points[k].y};
      wr(fo, xy, 2);
    }
  }
  std::fclose(fo);
  return 0;
}

struct MapInput {
  double xmin, ymin, xmax, ymax, delta, max_range, max_use_range, occ_thresh;
  float angle_min, angle_increment;
  int32_t n_beams, n_scans, node, reps;  // node: one scan at the origin on a fresh map, published; reps: timed repeats
  std::vector<double> poses;             // n_scans x (x, y, theta), ignored for node
  std::vector<float> ranges;             // n_scans x n_beams
};

MapInput read_map_input(const char* path) {
  MapInput m;
  FILE* f = open_or_die(path, "rb");
  double d[8];
  rd(f, d, 8);
  m.xmin = d[0]; m.ymin = d[1]; m.xmax = d[2]; m.ymax = d[3]; m.delta = d[4];
  m.max_range = d[5]; m.max_use_range = d[6]; m.occ_thresh = d[7];
  float a[2];
  rd(f, a, 2);
  m.angle_min = a[0]; m.angle_increment = a[1];
  int32_t h[4];
  rd(f, h, 4);
  m.n_beams = h[0]; m.n_scans = h[1]; m.node = h[2]; m.reps = h[3];
  m.poses.resize(3 * (size_t)m.n_scans);
  rd(f, m.poses.data(), m.poses.size());
  m.ranges.resize((size_t)m.n_scans * m.n_beams);
  rd(f, m.ranges.data(), m.ranges.size());
  std::fclose(f);
  return m;
}

struct Result {
  std::set<IntPoint, pointcomparator<int>> patches;  // union of every scan's active area
  int64_t dropped = 0;
};

bool inside(const ScanMatcherMap& map, const IntPoint& p) {
  return p.x >= 0 && p.y >= 0 && p.x < map.getMapSizeX() && p.y < map.getMapSizeY();
}

// one scan at pose lp into `map`, the node's ComputeMap order: lines and hits first, the active area allocated, all free
// updates of the scan, then its hits in beam order
void integrate_scan(ScanMatcherMap& map, const MapInput& in, const std::vector<double>& a_cos, const std::vector<double>& a_sin,
                    const float* ranges, const OrientedPoint& lp, Result& res) {
  const double c = std::cos(lp.theta), s = std::sin(lp.theta);
  const IntPoint p0 = map.world2map(Point(lp.x, lp.y));
  std::vector<GridLineTraversalLine> lines;
  std::vector<Point> hits;
  HierarchicalArray2D<PointAccumulator>::PointSet active;
  for (int i = 0; i < in.n_beams; i++) {
    double d = ranges[i];
    if (d > in.max_range || d == 0.0 || !std::isfinite(d)) continue;
    if (d > in.max_use_range) d = in.max_use_range;
    Point phit(lp.x, lp.y);
    phit.x += d * (c * a_cos[i] - s * a_sin[i]);
    phit.y += d * (s * a_cos[i] + c * a_sin[i]);
    const IntPoint p1 = map.world2map(phit);
    GridLineTraversalLine line;
    GridLineTraversal::gridLine(p0, p1, &line);
    lines.push_back(line);
    for (int k = 0; k < line.num_points - 1; k++)
      if (inside(map, line.points[k])) active.insert(map.storage().patchIndexes(line.points[k]));
    if (d < in.max_use_range) {
      if (inside(map, p1)) active.insert(map.storage().patchIndexes(p1));
      hits.push_back(phit);
    }
  }
  map.storage().setActiveArea(active, true);
  map.storage().allocActiveArea();
  res.patches.insert(active.begin(), active.end());
  for (const auto& line : lines)
    for (int k = 0; k < line.num_points - 1; k++) {
      if (!inside(map, line.points[k])) {
        res.dropped++;
        continue;
      }
      map.cell(line.points[k]).update(false, Point(0, 0));
    }
  for (const auto& hit : hits) {
    const IntPoint p1 = map.world2map(hit);
    if (!inside(map, p1)) {
      res.dropped++;
      continue;
    }
    map.cell(p1).update(true, hit);
  }
}

int run_map(const char* in_path, const char* out_path) {
  const MapInput in = read_map_input(in_path);
  // CreateCache: angle_min + i * angle_increment on float32 message fields with an unsigned i, widened to double; g++ -O2
  // makes one sincos call of the cos / sin pair, as it does in the node
  std::vector<double> a_cos, a_sin;
  for (unsigned int i = 0; i < (unsigned)in.n_beams; i++) {
    double angle = in.angle_min + i * in.angle_increment;
    a_cos.push_back(std::cos(angle));
    a_sin.push_back(std::sin(angle));
  }
  const Point center((in.xmin + in.xmax) / 2.0, (in.ymin + in.ymax) / 2.0);
  const uint32_t width = (uint32_t)((in.xmax - in.xmin) / in.delta), height = (uint32_t)((in.ymax - in.ymin) / in.delta);
  std::vector<int8_t> data((size_t)width * height);  // map_.data.resize: zeros

  auto callback = [&](ScanMatcherMap& map, Result& res) {
    if (in.node) {
      integrate_scan(map, in, a_cos, a_sin, in.ranges.data(), OrientedPoint(0, 0, 0.0), res);
      for (int x = 0; x < map.getMapSizeX(); x++)
        for (int y = 0; y < map.getMapSizeY(); y++) {
          const double occ = map.cell(IntPoint(x, y));
          data[(size_t)width * y + x] = occ < 0 ? -1 : (occ > in.occ_thresh ? 100 : 0);
        }
    } else {
      for (int s = 0; s < in.n_scans; s++)
        integrate_scan(map, in, a_cos, a_sin, in.ranges.data() + (size_t)s * in.n_beams,
                       OrientedPoint(in.poses[3 * s], in.poses[3 * s + 1], in.poses[3 * s + 2]), res);
    }
  };

  ScanMatcherMap map(center, in.xmin, in.ymin, in.xmax, in.ymax, in.delta);
  if (width < (uint32_t)map.getMapSizeX() || height < (uint32_t)map.getMapSizeY()) {
    std::fprintf(stderr, "published grid narrower than the storage\n");
    return 3;
  }
  Result res;
  callback(map, res);
  // the node's cost per callback on this host: a fresh map, ComputeMap, PublishMap
  double best = 0.0, total = 0.0;
  for (int r = 0; r < in.reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    ScanMatcherMap m2(center, in.xmin, in.ymin, in.xmax, in.ymax, in.delta);
    Result r2;
    callback(m2, r2);
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    total += dt;
    best = r == 0 ? dt : std::fmin(best, dt);
  }

  const int sx = map.getMapSizeX(), sy = map.getMapSizeY();
  const int px = sx >> map.storage().getPatchMagnitude(), py = sy >> map.storage().getPatchMagnitude();
  FILE* f = open_or_die(out_path, "wb");
  const int32_t hdr[8] = {sx, sy, (int32_t)width, (int32_t)height, (int32_t)map.world2map(center).x,
                          (int32_t)map.world2map(center).y, px, py};
  wr(f, hdr, 8);
  wr(f, a_cos.data(), a_cos.size());
  wr(f, a_sin.data(), a_sin.size());
  std::vector<int32_t> visits((size_t)sx * sy), n((size_t)sx * sy);
  std::vector<float> ax((size_t)sx * sy), ay((size_t)sx * sy);
  const ScanMatcherMap& cmap = map;  // the const cell() reads, allocating nothing
  for (int y = 0; y < sy; y++)
    for (int x = 0; x < sx; x++) {
      const PointAccumulator& c = cmap.cell(IntPoint(x, y));
      const size_t i = (size_t)y * sx + x;
      visits[i] = c.visits; n[i] = c.n; ax[i] = c.acc.x; ay[i] = c.acc.y;
    }
  wr(f, visits.data(), visits.size());
  wr(f, n.data(), n.size());
  wr(f, ax.data(), ax.size());
  wr(f, ay.data(), ay.size());
  std::vector<uint8_t> mask((size_t)px * py, 0);
  for (const auto& p : res.patches) mask[(size_t)p.y * px + p.x] = 1;
  wr(f, mask.data(), mask.size());
  wr(f, &res.dropped, 1);
  const double t[2] = {best, in.reps ? total / in.reps : 0.0};
  wr(f, t, 2);
  if (in.node) wr(f, data.data(), data.size());
  std::fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "line")) return run_lines(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "map")) return run_map(argv[2], argv[3]);
  std::fprintf(stderr, "usage: %s line|map <in> <out>\n", argv[0]);
  return 1;
}
