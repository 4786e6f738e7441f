// What the one-shot occupancy grid (occupancy_grid.hip) and the live map over the front-end's resident scans
// (livemap.hip) share: the grid handle, its geometry (ComputeDimensions), the beam filter parameters, the closed-form
// TraceLine of one beam -- one definition each, so both paths produce the bits already pinned to the reference -- and the
// narrow view of a front-end the live map reads (the front-end itself lives in scan_matcher.hip's translation unit).
#pragma once

#include <algorithm>

#include "common.hpp"
#include "karto_math.hpp"

struct lslam_frontend;

namespace lslam {

struct OccLaser {
  double min_angle, ang_res, min_range, max_range, range_threshold;
  int n_beams;
};

inline OccLaser occ_laser(const lslam_laser* laser) {
  OccLaser l;
  l.min_angle = laser->minimum_angle;
  l.ang_res = laser->angular_resolution;
  l.min_range = laser->minimum_range;
  l.max_range = laser->maximum_range;
  l.range_threshold = laser->range_threshold;
  l.n_beams = (int)(uint32_t)kround((laser->maximum_angle - laser->minimum_angle) / laser->angular_resolution);
  return l;
}

struct OccGeom {
  int w, h, stride;
  double scale, ox, oy;
};

constexpr double kBoxBig = 999999999999999999.99999;  // BoundingBox2() (Karto.h:2765)

// ComputeDimensions (Karto.h:5799-5817) of the box {minx, miny, maxx, maxy}
inline OccGeom occ_geom(const double bbox[4], double resolution) {
  OccGeom g;
  g.scale = 1.0 / resolution;
  g.w = (int)kround((bbox[2] - bbox[0]) * g.scale);
  g.h = (int)kround((bbox[3] - bbox[1]) * g.scale);
  g.ox = bbox[0];
  g.oy = bbox[1];
  g.stride = (g.w + 7) & ~7;  // Grid<kt_int32u>::Resize (Karto.h:4442)
  return g;
}

// UpdateCell (Karto.h:5950-5965) of one cell from its two counters: MinPassThrough = 2, OccupancyThreshold = 0.1
// (:5636-5637).  GridStates (Karto.h:4193-4198): 0 unknown, 100 occupied, 255 free.  The ONE statement of the cell rule:
// the published map (k_occ_update) and the ray cast's cell plane (raycast.hip) both apply it.
__device__ __forceinline__ uint8_t occ_cell_state(uint32_t pc, uint32_t hc) {
  uint8_t v = 0;  // GridStates_Unknown
  if (pc > 2u) v = ((double)hc / (double)pc > 0.1) ? 100 : 255;
  return v;
}

// RayTrace (Karto.h:5907-5942) of one beam by one wave (`lane` = 0..63), cells (x0, y0) -> (x1, y1).
// Grid<T>::TraceLine (Karto.h:4680-4745) in closed form: with deltaY <= deltaX the error recurrence
// "error += deltaY; if (2*error >= deltaX) { y += ystep; error -= deltaX; }" has taken
// q(k) = floor((2*k*deltaY + deltaX) / (2*deltaX)) minor steps before point k (k = 0..deltaX).
// Cells with x < done_w and y < done_h are left alone (0, 0: none): a grid that has grown on its max sides re-traces the
// scans it already holds for the margin only -- what the old bounds clipped and the new ones do not.
__device__ __forceinline__ void occ_trace_beam(int lane, int x0, int y0, int x1, int y1, bool end_valid, const OccGeom& g,
                                               uint32_t* __restrict__ pass, uint32_t* __restrict__ hit, int done_w = 0,
                                               int done_h = 0) {
  const int tx = x1, ty = y1;
  const bool steep = abs(y1 - y0) > abs(x1 - x0);
  if (steep) { int t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; }
  if (x0 > x1) { int t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
  const int dX = x1 - x0, dY = abs(y1 - y0), ystep = y0 < y1 ? 1 : -1;
  for (int k = lane; k <= dX; k += 64) {
    const int q = dX > 0 ? (int)((2LL * k * dY + dX) / (2LL * dX)) : 0;
    const int x = x0 + k, y = y0 + ystep * q;
    const int px = steep ? y : x, py = steep ? x : y;
    if (px >= 0 && px < g.w && py >= 0 && py < g.h && !(px < done_w && py < done_h))
      atomicAdd(&pass[px + (size_t)py * g.stride], 1u);
  }
  if (lane == 0 && end_valid && tx >= 0 && tx < g.w && ty >= 0 && ty < g.h && !(tx < done_w && ty < done_h)) {  // :5923-5938
    atomicAdd(&pass[tx + (size_t)ty * g.stride], 1u);
    atomicAdd(&hit[tx + (size_t)ty * g.stride], 1u);
  }
}

// ---- the front-end as the live map sees it (defined in frontend_impl.hpp) ----
struct FrontendView {
  lslam_context* ctx;
  const lslam_laser* laser;
  int n_beams;             // row length of d_ranges
  const double* d_ranges;  // [n_scans][n_beams] resident readings; re-read on every update (growing frees the old rows)
  int n_scans;             // processed scans
  uint64_t generation;     // bumped by lslam_frontend_reset
};
// Waits for whatever the front-end still has in flight that writes its resident rows or poses (a look-ahead match), then
// fills `v`.  Everything else the front-end enqueued is on v->ctx->stream: work put on that stream is ordered behind it.
int frontend_view(lslam_frontend* f, FrontendView* v);
// SENSOR poses of scans [first, first + count) as they stand (derived from the robot poses lslam_frontend_scan_pose
// reports, as the reference's scans derive theirs), 3 doubles each
void frontend_sensor_poses(const lslam_frontend* f, int first, int count, double* out);

// ---- what the ray cast keeps in a grid handle (raycast.hip) ----
struct RayCastState;
void raycast_release(lslam_occgrid* og);  // frees og->rc and takes its hook off the context (lslam_occgrid_destroy)

}  // namespace lslam

struct lslam_occgrid {
  lslam_context* ctx = nullptr;
  lslam::OccGeom g{};
  uint32_t* d_pass = nullptr;  // one allocation: pass plane, then the hit plane
  uint32_t* d_hit = nullptr;
  size_t cells = 0;            // stride * h words per plane
  lslam::DevBuf<uint8_t> d_out;
  // Whoever changes the counters, the planes they live in or the geometry says so HERE, and nowhere else: whatever is
  // derived from the counters and kept (the ray cast's cell plane) compares the epoch it was derived at with this one.
  // Writers take the planes from planes_for_write(), which says it for them.
  uint64_t counters_epoch = 1;
  void counters_written() { counters_epoch++; }
  uint32_t* planes_for_write() {
    counters_written();
    return d_pass;
  }
  lslam::RayCastState* rc = nullptr;  // created by the first ray cast
};
