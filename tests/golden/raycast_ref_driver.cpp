// Our own driver around the reference's karto::OccupancyGrid::RayCast (Karto.h:5717-5755), for
// tests/golden/make_raycast_golden.py: builds an OccupancyGrid(w, h, offset, resolution), writes the given cell bytes through
// GetDataPointer / GetWidthStep, calls RayCast for every given ray and writes what it returned.
//
//   raycast_ref_driver <in> <out> [reps]
//   in : int32 w, h, n;  float64 ox, oy, resolution;  uint8 cells[h * w] (row-major, GridStates);  float64 rays[n][4] = x, y,
//        heading, maxRange
//   out: float64 distance[n];  int64 stop[n] = round(distance / delta) of a ray that returned less than maxRange, else -1
//        (delta as the reference derives it; the rounding makes the index independent of its last bits);
//        float64 seconds_per_ray = best of `reps` timed passes over all rays on THIS host's CPU (0 without reps)
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "open_karto/Karto.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int reps = argc > 3 ? atoi(argv[3]) : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[3];
  double geo[3];
  if (fread(hdr, sizeof hdr, 1, f) != 1 || fread(geo, sizeof geo, 1, f) != 1) return 4;
  const int w = hdr[0], h = hdr[1], n = hdr[2];
  std::vector<uint8_t> cells((size_t)w * h);
  std::vector<double> rays((size_t)n * 4);
  if (!cells.empty() && fread(cells.data(), 1, cells.size(), f) != cells.size()) return 4;
  if (n > 0 && fread(rays.data(), sizeof(double), rays.size(), f) != rays.size()) return 4;
  fclose(f);

  karto::OccupancyGrid grid(w, h, karto::Vector2<kt_double>(geo[0], geo[1]), geo[2]);
  kt_int8u* data = grid.GetDataPointer();
  const size_t step = (size_t)grid.GetWidthStep();
  for (int y = 0; y < h; y++) memcpy(data + y * step, &cells[(size_t)y * w], (size_t)w);

  std::vector<double> dist(n);
  std::vector<int64_t> stop(n);
  const double scale = 1.0 / geo[2];
  for (int i = 0; i < n; i++) {
    const double* r = &rays[4 * (size_t)i];
    dist[i] = grid.RayCast(karto::Pose2(r[0], r[1], r[2]), r[3]);
    const double xs = 1 + fabs(r[3] * cos(r[2])) * scale, ys = 1 + fabs(r[3] * sin(r[2])) * scale;
    const double delta = r[3] / (xs > ys ? xs : ys);
    stop[i] = dist[i] < r[3] ? (int64_t)llround(dist[i] / delta) : -1;
  }
  double best = 0.0;
  for (int k = 0; k < reps && n > 0; k++) {
    volatile double sink = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; i++) {
      const double* r = &rays[4 * (size_t)i];
      sink = sink + grid.RayCast(karto::Pose2(r[0], r[1], r[2]), r[3]);
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / n;
    if (k == 0 || s < best) best = s;
  }
  f = fopen(argv[2], "wb");
  if (!f) return 5;
  fwrite(dist.data(), sizeof(double), dist.size(), f);
  fwrite(stop.data(), sizeof(int64_t), stop.size(), f);
  fwrite(&best, sizeof best, 1, f);
  fclose(f);
  return 0;
}
