// karto::OccupancyGrid::RayCast (Karto.h:5717-5755) on MI355X (gfx950), batched: the distance from a pose along its
// heading to the first cell that is not free -- the one way the reference QUERIES the map it builds.  One call per
// beam gives the range image a laser would see from a pose.
//
// Reference behaviour reproduced (never copied), fp64 in the reference's expression order (-ffp-contract=off):
//     scale = 1/resolution;  s = sin(theta);  c = cos(theta)
//     xSteps = 1 + fabs((x + maxRange*c) - x) * scale      (ySteps with s)
//     steps = max(xSteps, ySteps);  delta = maxRange / steps;  distance = delta
//     for (uint32 i = 1; i < steps; i++)                   // i is compared with the double
//       g = WorldToGrid(x + distance*c, y + distance*s)    // Round((w - offset) * scale), Karto.h:4237-4252
//       if (IsValidGridIndex(g) && cell(g) == GridStates_Free) distance = (i + 1) * delta; else break
//     return distance < maxRange ? distance : maxRange
// so unknown cells stop a ray like occupied ones, leaving the grid stops it, the start cell is never tested, and the
// sample of iteration i lies at i * delta: `distance` is known in closed form, the samples of a ray are independent, and
// the result is k * delta for the FIRST failing i = k, or N * delta (N = the first i with !(i < steps)) when none fails.
//
//   k_rc_cells   thread per byte of the cell plane: the state of every cell from the two counters by the grid's own rule
//                (occ_cell_state, the one k_occ_update applies), at the reference's row pitch, behind 8 guard bytes
//   k_rc_rays    form (a): n independent (x, y, theta), per-ray or common maxRange
//   k_rc_scans   form (b): n_poses sensor poses x the beams of a laser, heading = pose.heading + minimum_angle + i * res
//                evaluated left to right (Karto.h:5394)
// Both forms are one body (rc_walk): a wave takes 64 rays, every lane sets ONE ray up (sin/cos once per ray), then the
// wave walks the rays kRayGroup lanes to a ray, kRayGroup samples to a step: the stop is the first failing lane of the
// first step that has one, found with a ballot.  A short ray wastes at most one step.
#include <algorithm>
#include <climits>
#include <cmath>

#include "occgrid_impl.hpp"

using namespace lslam;

#ifndef LSLAM_RAYCAST_GROUP
#define LSLAM_RAYCAST_GROUP 8  // lanes per ray (a power of two, 1..64): DESIGN 4.17 holds what the other widths measured
#endif

namespace lslam {

struct RayCastState {
  DevBuf<uint8_t> d_cells;     // 8 guard bytes (unknown), then h rows of `stride` bytes (the bytes past w unknown too)
  uint64_t cells_epoch = 0;    // lslam_occgrid::counters_epoch the plane was derived at (0: never)
  DevBuf<double> d_in, d_out;  // staging of the host entry points
  unsigned long long* d_samples = nullptr;  // device: samples the reference would have tested, summed over all calls
  unsigned long long* h_unsupported = nullptr;  // PINNED HOST memory: rays refused on the device, summed over all calls
  unsigned long long unsupported_reported = 0;  // of those, how many a call or a synchronise has already reported
  int64_t n_calls = 0, n_rays = 0, n_refreshes = 0;
};

}  // namespace lslam

namespace {

constexpr int kRayGroup = LSLAM_RAYCAST_GROUP;
static_assert(kRayGroup >= 1 && kRayGroup <= 64 && (kRayGroup & (kRayGroup - 1)) == 0, "lanes per ray: a power of two");
constexpr size_t kGuard = 8;  // bytes in front of the first row; byte 0 is where every sample outside the grid reads

__global__ void __launch_bounds__(256)
k_rc_cells(OccGeom g, const uint32_t* __restrict__ pass, const uint32_t* __restrict__ hit, uint8_t* __restrict__ cells) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (blockIdx.x == 0 && y == 0 && threadIdx.x < (int)kGuard) cells[threadIdx.x] = 0;
  if (x >= g.stride || y >= g.h) return;
  const size_t o = x + (size_t)y * g.stride;
  cells[kGuard + o] = x < g.w ? occ_cell_state(pass[o], hit[o]) : (uint8_t)0;
}

struct RayGrid {
  int w, h, stride;
  double scale, ox, oy;
  const uint8_t* cells;
};

// One wave, 64 rays: lane `lane` has set up ITS ray (x, y, heading, maxRange; `have` = it exists).  Returns, in the lanes
// with sub-lane 0 of every group and for every round r, through `emit(slot, value)`: the ray cast of wave slot `slot`.
// tested: samples the reference's loop would have tested, unsupported: rays refused -- both summed by the caller.
template <int G, typename Emit>
__device__ __forceinline__ void rc_walk(int lane, bool have, double x, double y, double heading, double max_range,
                                        const RayGrid& rg, unsigned long long& tested, unsigned int& unsupported,
                                        Emit emit) {
  // ---- per-ray set-up, one lane per ray (Karto.h:5719-5735) ----
  double sn, cs;  // one shared argument reduction; ocml's sincos returns the same values as sin and cos
  sincos(heading, &sn, &cs);
  const double x_stop = x + max_range * cs;
  const double x_steps = 1 + fabs(x_stop - x) * rg.scale;
  const double y_stop = y + max_range * sn;
  const double y_steps = 1 + fabs(y_stop - y) * rg.scale;
  const double steps = x_steps > y_steps ? x_steps : y_steps;  // math::Maximum (Math.h:111-114)
  const double delta = max_range / steps;
  // the reference's counter is a uint32 compared with `steps`: beyond 2^32 - 1 it wraps and never ends.  NaN fails too.
  const bool fits = max_range > 0.0 && max_range <= 1.79769313486231570e308 && steps <= 4294967295.0;
  const double n_end = steps > 1.0 ? ceil(steps) : 1.0;  // the first i >= 1 with !(i < steps)
  const int live = have && fits;
  // ---- the walk: G lanes to a ray, 64 / G rays at a time ----
  constexpr int kRays = 64 / G;
  const int grp = lane / G, sub = lane % G;
  const unsigned long long group_mask = G == 64 ? ~0ull : ((1ull << G) - 1ull) << (grp * G);
#pragma unroll 1
  for (int r = 0; r < G; r++) {
    const int slot = r * kRays + grp;
    const double rx = __shfl(x, slot), ry = __shfl(y, slot), rc = __shfl(cs, slot), rs = __shfl(sn, slot);
    const double rdelta = __shfl(delta, slot), rend = __shfl(n_end, slot), rmax = __shfl(max_range, slot);
    const int rhave = __shfl((int)have, slot);
    bool done = !__shfl(live, slot);
    bool refused = rhave && done;
    double dk = 0.0;  // the index the ray's distance is taken at
    double dbase = 1.0;
    while (__ballot(!done)) {
      const double di = dbase + (double)sub;
      const bool active = !done && di < rend;
      const double distance = di * rdelta;  // iteration 1: delta itself; iteration i > 1: (i - 1 + 1) * delta (Karto.h:5746)
      const double x1 = rx + distance * rc;
      const double y1 = ry + distance * rs;
      const double gxr = kround((x1 - rg.ox) * rg.scale), gyr = kround((y1 - rg.oy) * rg.scale);  // WorldToGrid
      const bool in_i32 = fabs(gxr) < 2147483648.0 && fabs(gyr) < 2147483648.0;  // NaN fails
      const int gx = in_i32 ? (int)gxr : -1, gy = in_i32 ? (int)gyr : -1;
      const bool valid = (unsigned)gx < (unsigned)rg.w && (unsigned)gy < (unsigned)rg.h;  // IsValidGridIndex (Karto.h:4477-4480)
      const size_t at = active && valid ? kGuard + (size_t)gx + (size_t)gy * (size_t)rg.stride : (size_t)0;
      const bool is_free = rg.cells[at] == 255;  // GridStates_Free; the guard byte is unknown
      const unsigned long long stops = __ballot(active && !is_free) & group_mask;
      const unsigned long long overflows = __ballot(active && !in_i32) & group_mask;
      if (!done) {
        if (stops) {
          const int first = __ffsll((long long)stops) - 1;
          dk = dbase + (double)(first - grp * G);
          refused = (overflows >> first) & 1ull;  // the reference would have converted a coordinate that does not fit int32
          done = true;
        } else if (!(dbase + (double)G < rend)) {
          dk = rend;  // ran out: the loop's last assignment was (N - 1 + 1) * delta
          done = true;
        }
      }
      dbase += (double)G;
    }
    if (sub == 0 && rhave) {
      const double distance = dk * rdelta;
      double v = distance < rmax ? distance : rmax;
      if (refused) {
        v = __longlong_as_double(0x7ff8000000000000LL);
        unsupported += 1u;
      } else {
        tested += (unsigned long long)(dk < rend ? dk : rend - 1.0);
      }
      emit(slot, v);
    }
  }
}

__device__ __forceinline__ void rc_account(int lane, unsigned long long tested, unsigned int unsupported,
                                           unsigned long long* __restrict__ samples,
                                           unsigned long long* __restrict__ unsupported_total) {
  for (int o = 32; o > 0; o >>= 1) {
    tested += __shfl_xor(tested, o);
    unsupported += __shfl_xor(unsupported, o);
  }
  if (lane == 0) {
    if (tested) atomicAdd(samples, tested);
    if (unsupported) atomicAdd(unsupported_total, (unsigned long long)unsupported);
  }
}

__global__ void __launch_bounds__(256)
k_rc_rays(int n, const double* __restrict__ poses, const double* __restrict__ max_ranges, double max_range, RayGrid rg,
          double* __restrict__ out, unsigned long long* __restrict__ samples, unsigned long long* __restrict__ unsupported_total) {
  const int lane = threadIdx.x & 63;
  const long long wave_first = ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64;
  const long long t = wave_first + lane;
  const bool have = t < n;
  double x = 0.0, y = 0.0, heading = 0.0, mr = max_range;
  if (have) {
    x = poses[3 * t]; y = poses[3 * t + 1]; heading = poses[3 * t + 2];
    if (max_ranges) mr = max_ranges[t];
  }
  unsigned long long tested = 0;
  unsigned int unsupported = 0;
  rc_walk<kRayGroup>(lane, have, x, y, heading, mr, rg, tested, unsupported,
                     [&](int slot, double v) { out[wave_first + slot] = v; });
  rc_account(lane, tested, unsupported, samples, unsupported_total);
}

__global__ void __launch_bounds__(256)
k_rc_scans(int n_poses, int n_beams, double min_angle, double ang_res, const double* __restrict__ poses, double max_range,
           RayGrid rg, double* __restrict__ out, int out_stride, unsigned long long* __restrict__ samples,
           unsigned long long* __restrict__ unsupported_total) {
  const int lane = threadIdx.x & 63;
  const long long wave_first = ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64;
  const long long t = wave_first + lane;
  const bool have = t < (long long)n_poses * n_beams;
  double x = 0.0, y = 0.0, heading = 0.0;
  if (have) {
    const long long p = t / n_beams;
    const uint32_t b = (uint32_t)(t - p * n_beams);
    x = poses[3 * p]; y = poses[3 * p + 1];
    heading = poses[3 * p + 2] + min_angle + b * ang_res;  // Karto.h:5394
  }
  unsigned long long tested = 0;
  unsigned int unsupported = 0;
  rc_walk<kRayGroup>(lane, have, x, y, heading, max_range, rg, tested, unsupported, [&](int slot, double v) {
    const long long ts = wave_first + slot, p = ts / n_beams;
    out[p * out_stride + (ts - p * n_beams)] = v;
  });
  rc_account(lane, tested, unsupported, samples, unsupported_total);
}

// ---- host side -----------------------------------------------------------------------------------------------------

// what a synchronise (or a host entry point, which has just waited) makes of rays the device refused since the last look
int rc_report(lslam_occgrid* og) {
  RayCastState* st = og->rc;
  if (!st || !st->h_unsupported) return LSLAM_OK;
  const unsigned long long now = __atomic_load_n(st->h_unsupported, __ATOMIC_ACQUIRE);
  if (now == st->unsupported_reported) return LSLAM_OK;
  const unsigned long long fresh = now - st->unsupported_reported;
  st->unsupported_reported = now;
  return og->ctx->fail(LSLAM_ERR_UNSUPPORTED,
                       "ray cast: %llu ray(s) whose step count does not fit the reference's uint32 counter, whose max_range is "
                       "not a positive finite number, or whose stopping sample's grid coordinate does not fit int32 "
                       "(Karto.h:5717-5755); their outputs are NaN", fresh);
}

// the state, and a cell plane that matches the counters as they stand: enqueued on the context stream, no host wait
int rc_prepare(lslam_occgrid* og) {
  lslam_context* ctx = og->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  if (!og->rc) {
    RayCastState* st = new RayCastState();
    hipError_t e = hipMalloc((void**)&st->d_samples, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(st->d_samples, 0, sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) e = hipHostMalloc((void**)&st->h_unsupported, sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) {
      if (st->d_samples) (void)hipFree(st->d_samples);
      delete st;
      return ctx->fail(LSLAM_ERR_HIP, "cannot allocate the ray-cast state: %s", hipGetErrorString(e));
    }
    *st->h_unsupported = 0ull;
    og->rc = st;
    // lslam_synchronize makes a refused ray LOUD once the stream has drained (the _dev entry points cannot)
    ctx->post_sync.emplace_back((void*)og, [](void* p) { return rc_report((lslam_occgrid*)p); });
  }
  RayCastState* st = og->rc;
  if (st->cells_epoch != og->counters_epoch) {
    const OccGeom& g = og->g;
    const size_t bytes = kGuard + (size_t)std::max(g.stride, 0) * std::max(g.h, 0);
    LSLAM_HIP(ctx, st->d_cells.reserve(bytes));
    launch(ctx, "rc_cells", k_rc_cells, dim3((std::max(g.stride, 1) + 255) / 256, std::max(g.h, 1)), dim3(256), 0, g,
           (const uint32_t*)og->d_pass, (const uint32_t*)og->d_hit, st->d_cells.p);
    st->cells_epoch = og->counters_epoch;
    st->n_refreshes++;
  }
  return LSLAM_OK;
}

RayGrid rc_grid(const lslam_occgrid* og) {
  RayGrid rg;
  rg.w = std::max(og->g.w, 0); rg.h = std::max(og->g.h, 0); rg.stride = og->g.stride;
  rg.scale = og->g.scale; rg.ox = og->g.ox; rg.oy = og->g.oy;
  rg.cells = og->rc->d_cells.p;
  return rg;
}

bool rc_range_ok(double max_range) { return max_range > 0.0 && std::isfinite(max_range); }

int rc_rays_dev(lslam_occgrid* og, int n, const double* d_poses, const double* d_max_ranges, double max_range, double* d_out) {
  int rc = rc_prepare(og);
  if (rc) return rc;
  launch(og->ctx, "rc_rays", k_rc_rays, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, n, d_poses, d_max_ranges,
         max_range, rc_grid(og), d_out, og->rc->d_samples, og->rc->h_unsupported);
  og->rc->n_calls++;
  og->rc->n_rays += n;
  return LSLAM_OK;
}

int rc_scans_dev(lslam_occgrid* og, const OccLaser& l, int n_poses, const double* d_poses, double max_range, double* d_out,
                 int out_stride) {
  int rc = rc_prepare(og);
  if (rc) return rc;
  const long long total = (long long)n_poses * l.n_beams;
  launch(og->ctx, "rc_scans", k_rc_scans, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, n_poses, l.n_beams, l.min_angle,
         l.ang_res, d_poses, max_range, rc_grid(og), d_out, out_stride, og->rc->d_samples, og->rc->h_unsupported);
  og->rc->n_calls++;
  og->rc->n_rays += total;
  return LSLAM_OK;
}

// arguments of form (b) that can be judged without a device; *total = rays
int rc_scans_check(lslam_occgrid* og, const lslam_laser* laser, int n_poses, const double* poses, double max_range,
                   const double* out, int out_stride, OccLaser* l, long long* total) {
  if (!og || !laser || n_poses < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  *l = occ_laser(laser);
  *total = (long long)n_poses * std::max(l->n_beams, 0);
  if (*total > 0 && (!poses || !out)) return LSLAM_ERR_INVALID_ARGUMENT;
  if (!rc_range_ok(max_range)) return og->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "max_range must be a positive finite number");
  if (l->n_beams < 0 || (n_poses > 0 && out_stride < l->n_beams))
    return og->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "out_stride %d < num_beams %d", out_stride, l->n_beams);
  if (*total > (long long)INT_MAX) return og->ctx->fail(LSLAM_ERR_UNSUPPORTED, "%lld rays in one call (at most 2^31 - 1)", *total);
  return LSLAM_OK;
}

int rc_rays_check(lslam_occgrid* og, int n, const double* poses, const double* max_ranges, double max_range, const double* out) {
  if (!og || n < 0 || (n > 0 && (!poses || !out))) return LSLAM_ERR_INVALID_ARGUMENT;
  if (!max_ranges && !rc_range_ok(max_range))
    return og->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "max_range must be a positive finite number");
  return LSLAM_OK;
}

}  // namespace

namespace lslam {

void raycast_release(lslam_occgrid* og) {
  RayCastState* st = og->rc;
  if (!st) return;
  auto& hooks = og->ctx->post_sync;
  for (size_t i = 0; i < hooks.size(); i++)
    if (hooks[i].first == (void*)og) {
      hooks.erase(hooks.begin() + (long)i);
      break;
    }
  st->d_cells.release();
  st->d_in.release();
  st->d_out.release();
  if (st->d_samples) (void)hipFree(st->d_samples);
  if (st->h_unsupported) (void)hipHostFree(st->h_unsupported);
  delete st;
  og->rc = nullptr;
}

}  // namespace lslam

extern "C" {

int lslam_occgrid_ray_cast_dev(lslam_occgrid* og, int n_rays, const double* d_poses_xyh, const double* d_max_ranges,
                               double max_range, double* d_out) {
  int rc = rc_rays_check(og, n_rays, d_poses_xyh, d_max_ranges, max_range, d_out);
  if (rc || n_rays == 0) return rc;
  return rc_rays_dev(og, n_rays, d_poses_xyh, d_max_ranges, max_range, d_out);
}

int lslam_occgrid_ray_cast(lslam_occgrid* og, int n_rays, const double* poses_xyh, const double* max_ranges, double max_range,
                           double* out_host) {
  int rc = rc_rays_check(og, n_rays, poses_xyh, max_ranges, max_range, out_host);
  if (rc || n_rays == 0) return rc;
  lslam_context* ctx = og->ctx;
  rc = rc_prepare(og);
  if (rc) return rc;
  RayCastState* st = og->rc;
  const size_t n = (size_t)n_rays;
  LSLAM_HIP(ctx, st->d_in.reserve(4 * n));
  LSLAM_HIP(ctx, st->d_out.reserve(n));
  LSLAM_HIP(ctx, hipMemcpyAsync(st->d_in.p, poses_xyh, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (max_ranges)
    LSLAM_HIP(ctx, hipMemcpyAsync(st->d_in.p + 3 * n, max_ranges, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  rc = rc_rays_dev(og, n_rays, st->d_in.p, max_ranges ? st->d_in.p + 3 * n : nullptr, max_range, st->d_out.p);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(out_host, st->d_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st->d_cells.trim(); st->d_in.trim(); st->d_out.trim();
  return rc_report(og);
}

int lslam_occgrid_ray_cast_scans_dev(lslam_occgrid* og, const lslam_laser* laser, int n_poses, const double* d_sensor_poses,
                                     double max_range, double* d_out_ranges, int out_stride) {
  OccLaser l;
  long long total = 0;
  int rc = rc_scans_check(og, laser, n_poses, d_sensor_poses, max_range, d_out_ranges, out_stride, &l, &total);
  if (rc || total == 0) return rc;
  return rc_scans_dev(og, l, n_poses, d_sensor_poses, max_range, d_out_ranges, out_stride);
}

int lslam_occgrid_ray_cast_scans(lslam_occgrid* og, const lslam_laser* laser, int n_poses, const double* sensor_poses,
                                 double max_range, double* out_ranges_host, int out_stride) {
  OccLaser l;
  long long total = 0;
  int rc = rc_scans_check(og, laser, n_poses, sensor_poses, max_range, out_ranges_host, out_stride, &l, &total);
  if (rc || total == 0) return rc;
  lslam_context* ctx = og->ctx;
  rc = rc_prepare(og);
  if (rc) return rc;
  RayCastState* st = og->rc;
  LSLAM_HIP(ctx, st->d_in.reserve((size_t)n_poses * 3));
  LSLAM_HIP(ctx, st->d_out.reserve((size_t)total));
  LSLAM_HIP(ctx, hipMemcpyAsync(st->d_in.p, sensor_poses, (size_t)n_poses * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  rc = rc_scans_dev(og, l, n_poses, st->d_in.p, max_range, st->d_out.p, l.n_beams);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipMemcpy2DAsync(out_ranges_host, (size_t)out_stride * sizeof(double), st->d_out.p, (size_t)l.n_beams * sizeof(double),
                                  (size_t)l.n_beams * sizeof(double), n_poses, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st->d_cells.trim(); st->d_in.trim(); st->d_out.trim();
  return rc_report(og);
}

int lslam_occgrid_ray_cast_stats(const lslam_occgrid* og, int64_t out[4]) {
  if (!og || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = out[1] = out[2] = out[3] = 0;
  const RayCastState* st = og->rc;
  if (!st) return LSLAM_OK;
  lslam_context* ctx = og->ctx;
  unsigned long long samples = 0;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hipMemcpyAsync(&samples, st->d_samples, sizeof samples, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out[0] = st->n_calls;
  out[1] = st->n_rays;
  out[2] = st->n_refreshes;
  out[3] = (int64_t)samples;
  return LSLAM_OK;
}

}  // extern "C"
