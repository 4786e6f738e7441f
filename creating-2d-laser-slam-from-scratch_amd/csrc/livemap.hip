// Live occupancy map over the streaming front-end's resident scans (gfx950): what SlamKarto::updateMap
// (lesson6/src/karto_slam.cc:507-581) asks of karto::OccupancyGrid::CreateFromScans(GetAllProcessedScans(), resolution)
// (Karto.h:5659-5673) every map_update_interval -- without the caller's copy of the scans, without an upload, and
// without retracing what has been traced.
//
// Why it can be incremental and still equal the from-scratch build bit for bit: the counters are integers (sums in any
// order), the grid geometry depends on the scans only through the union of their boxes (ComputeDimensions,
// Karto.h:5799-5817), and a front-end without a solver never moves a scan an earlier Process call has finished.  So
//   append   the union box is unchanged: trace the new scans into the planes as they stand
//   grow     only a max side moved: same offset, larger w / h -- copy the rows to the new stride, trace the new scans,
//            and re-trace, for the margin only, the old scans whose rays the old bounds clipped (a ray's last cell
//            round((maxx - ox) * scale) == w lies just outside the grid its own scan sized; once the grid has grown it
//            is inside).  Which scans those are is known exactly: every scan's largest traced x and y are kept.
//   rebuild  a min side moved (the offset, hence every round((x - ox) * scale), changes), a traced scan's pose changed,
//            the front-end was reset, or there is no map yet: zero the planes, trace every resident scan
// Rebuilds read the resident rows too: nothing is uploaded but 28 bytes per traced scan (its id and sensor pose).
//
//   k_live_box     block per scan: box of the filtered readings and the sensor position (LocalizedRangeScan::Update,
//                  Karto.h:5362-5428), and the largest x and y any of its rays reaches (AddScan's end points, shortened
//                  to the range threshold), reduced in the block -- kept on the host, the union box is the min/max
//   k_live_trace   wave per 64 beams of the listed scans: each lane classifies one beam and works out its end cell
//                  (AddScan, Karto.h:5851-5885) from the resident reading -- no ends[] / flags[] staging -- then the wave
//                  traces the live beams one after the other (occ_trace_beam: TraceLine in closed form, integer atomics)
//   k_live_regrid  thread per word of the new planes: the old rows at the new stride, zero elsewhere
// Classification is the one-shot grid's k_occ_update: the map is an ordinary lslam_occgrid.
#include <cstring>
#include <vector>

#include "occgrid_impl.hpp"

using namespace lslam;

namespace {

constexpr int kBoxWords = 6;  // per scan: minx, miny, maxx, maxy of its box, then the largest x and y its rays reach

__global__ void __launch_bounds__(256)
k_live_box(const int* __restrict__ ids, const double* __restrict__ poses, const double* __restrict__ ranges, OccLaser l,
           double* __restrict__ boxes /* [scan of the list] minx, miny, maxx, maxy, traced maxx, traced maxy */) {
  __shared__ double sh[4][kBoxWords];
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double sx = poses[3 * (size_t)k], sy = poses[3 * (size_t)k + 1], sh_ = poses[3 * (size_t)k + 2];
  const double* row = ranges + (size_t)ids[k] * l.n_beams;
  double mnx = kBoxBig, mny = kBoxBig, mxx = -kBoxBig, mxy = -kBoxBig;  // BoundingBox2() (Karto.h:2765)
  double tmx = -kBoxBig, tmy = -kBoxBig;
  for (int b = tid; b < l.n_beams; b += 256) {
    const double r = row[b];
    const bool filtered = r >= l.min_range && r <= l.range_threshold;  // Karto.h:5382
    const bool traced = !(r <= l.min_range || r >= l.max_range || isnan(r));  // AddScan (Karto.h:5866-5885)
    if (!filtered && !traced) continue;
    double px, py;
    beam_world_point(sx, sy, sh_, l.min_angle, l.ang_res, (uint32_t)b, r, px, py);
    if (filtered) {  // filtered reading -> scan bounding box (Karto.h:5421-5424)
      mnx = fmin(mnx, px); mxx = fmax(mxx, px);
      mny = fmin(mny, py); mxy = fmax(mxy, py);
    }
    if (traced) {
      if (r >= l.range_threshold) {  // traced up to the range threshold only: the end point k_live_trace computes
        double ratio = l.range_threshold / r;
        double dx = px - sx, dy = py - sy;
        px = sx + ratio * dx;
        py = sy + ratio * dy;
      }
      tmx = fmax(tmx, px); tmy = fmax(tmy, py);
    }
  }
  if (tid == 0) {  // the box also holds the sensor position (Karto.h:5420); every ray starts there
    mnx = fmin(mnx, sx); mxx = fmax(mxx, sx);
    mny = fmin(mny, sy); mxy = fmax(mxy, sy);
    tmx = fmax(tmx, sx); tmy = fmax(tmy, sy);
  }
  for (int o = 32; o > 0; o >>= 1) {  // exact min/max: order of combination is irrelevant
    mnx = fmin(mnx, __shfl_xor(mnx, o)); mny = fmin(mny, __shfl_xor(mny, o));
    mxx = fmax(mxx, __shfl_xor(mxx, o)); mxy = fmax(mxy, __shfl_xor(mxy, o));
    tmx = fmax(tmx, __shfl_xor(tmx, o)); tmy = fmax(tmy, __shfl_xor(tmy, o));
  }
  if (lane == 0) {
    sh[wave][0] = mnx; sh[wave][1] = mny; sh[wave][2] = mxx; sh[wave][3] = mxy; sh[wave][4] = tmx; sh[wave][5] = tmy;
  }
  __syncthreads();
  if (tid < kBoxWords) {
    double v = sh[0][tid];
    for (int w = 1; w < 4; w++) v = tid < 2 ? fmin(v, sh[w][tid]) : fmax(v, sh[w][tid]);
    boxes[kBoxWords * (size_t)k + tid] = v;
  }
}

__global__ void __launch_bounds__(256)
k_live_trace(int K, const int* __restrict__ ids, const double* __restrict__ poses, const double* __restrict__ ranges,
             OccLaser l, OccGeom g, uint32_t* __restrict__ pass, uint32_t* __restrict__ hit, int done_w, int done_h) {
  const int lane = threadIdx.x & 63;
  const long long beam = ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64 + lane;
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0, f = 0;  // f: bit0 = traced, bit1 = end point valid
  if (beam < (long long)K * l.n_beams) {
    const int k = (int)(beam / l.n_beams), b = (int)(beam - (long long)k * l.n_beams);
    const double sx = poses[3 * (size_t)k], sy = poses[3 * (size_t)k + 1], sh_ = poses[3 * (size_t)k + 2];
    const double r = ranges[(size_t)ids[k] * l.n_beams + b];
    // AddScan (Karto.h:5866-5885)
    if (!(r <= l.min_range || r >= l.max_range || isnan(r))) {
      f = 1;
      if (r < (l.range_threshold - kTol)) f |= 2;
      double px, py;
      beam_world_point(sx, sy, sh_, l.min_angle, l.ang_res, (uint32_t)b, r, px, py);
      if (r >= l.range_threshold) {  // trace up to the range threshold only
        double ratio = l.range_threshold / r;
        double dx = px - sx, dy = py - sy;
        px = sx + ratio * dx;
        py = sy + ratio * dy;
      }
      // RayTrace (Karto.h:5907-5942)
      x0 = world_to_grid(sx, g.ox, g.scale); y0 = world_to_grid(sy, g.oy, g.scale);
      x1 = world_to_grid(px, g.ox, g.scale); y1 = world_to_grid(py, g.oy, g.scale);
    }
  }
  // the wave traces its live beams one after the other, all 64 lanes along each ray
  for (unsigned long long live = __ballot(f & 1); live; live &= live - 1) {
    const int j = __ffsll((long long)live) - 1;
    occ_trace_beam(lane, __shfl(x0, j), __shfl(y0, j), __shfl(x1, j), __shfl(y1, j), (__shfl(f, j) & 2) != 0, g, pass, hit,
                   done_w, done_h);
  }
}

// both planes of the new grid: the old rows at the new stride, zero elsewhere (same offset; w and h only ever grow here)
__global__ void __launch_bounds__(256)
k_live_regrid(OccGeom og, const uint32_t* __restrict__ old_pass, const uint32_t* __restrict__ old_hit, OccGeom ng,
              uint32_t* __restrict__ pass, uint32_t* __restrict__ hit) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= ng.stride || y >= ng.h) return;
  const bool in_old = x < og.w && y < og.h;
  const size_t o = x + (size_t)y * og.stride, n = x + (size_t)y * ng.stride;
  pass[n] = in_old ? old_pass[o] : 0u;
  hit[n] = in_old ? old_hit[o] : 0u;
}

}  // namespace

struct lslam_livemap {
  lslam_frontend* f = nullptr;
  lslam_context* ctx = nullptr;
  double resolution = 0.0;
  lslam_occgrid* og = nullptr;   // the map handed out by lslam_livemap_grid; its planes are replaced on grow / rebuild
  size_t cap_words = 0;          // uint32 words og->d_pass was allocated with
  bool have = false;             // og holds the map of `traced`
  uint64_t generation = 0;       // the front-end's when the map was last brought up to date
  double box[4] = {kBoxBig, kBoxBig, -kBoxBig, -kBoxBig};  // union of `boxes`
  std::vector<double> boxes;     // per scan in the map: kBoxWords doubles (k_live_box)
  std::vector<double> traced;    // per scan in the map: the sensor pose it was traced at
  std::vector<double> h_poses;   // staging: current sensor poses of all processed scans
  std::vector<int> h_ids;        // staging: the scan list of the kernels
  std::vector<double> h_list_poses;
  DevBuf<int> d_ids;
  DevBuf<double> d_poses, d_boxes;
  int64_t n_updates = 0, n_appends = 0, n_grows = 0, n_rebuilds = 0, n_traced = 0;
};

namespace {

// the scan list lm->h_ids and those scans' sensor poses onto the device (the caller has synchronised the stream since the
// last list was read)
int live_stage(lslam_livemap* lm) {
  lslam_context* ctx = lm->ctx;
  const size_t K = lm->h_ids.size();
  LSLAM_HIP(ctx, lm->d_ids.reserve(K));
  LSLAM_HIP(ctx, lm->d_poses.reserve(K * 3));
  lm->h_list_poses.resize(K * 3);
  for (size_t k = 0; k < K; k++) memcpy(&lm->h_list_poses[3 * k], &lm->h_poses[3 * (size_t)lm->h_ids[k]], 3 * sizeof(double));
  LSLAM_HIP(ctx, hipMemcpyAsync(lm->d_ids.p, lm->h_ids.data(), K * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(lm->d_poses.p, lm->h_list_poses.data(), K * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return LSLAM_OK;
}
void live_list(lslam_livemap* lm, int first, int N) {
  lm->h_ids.clear();
  for (int s = first; s < N; s++) lm->h_ids.push_back(s);
}

int live_update(lslam_livemap* lm) {
  FrontendView v;
  int rc = frontend_view(lm->f, &v);
  if (rc) return rc;
  lslam_context* ctx = v.ctx;
  if (v.n_scans == 0) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "no processed scans (the reference returns NULL)");
  const OccLaser l = occ_laser(v.laser);
  const int N = v.n_scans, n = l.n_beams;
  if (n != v.n_beams) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "front-end rows hold %d beams, the laser %d", v.n_beams, n);
  lslam_occgrid* og = lm->og;
  const int in_map = (int)(lm->traced.size() / 3);
  lm->h_poses.resize((size_t)N * 3);
  frontend_sensor_poses(lm->f, 0, N, lm->h_poses.data());
  // the map is stale as a whole when scan ids started over or a traced scan is no longer where it was traced
  bool stale = !lm->have || lm->generation != v.generation || N < in_map;
  if (!stale) stale = memcmp(lm->h_poses.data(), lm->traced.data(), (size_t)in_map * 3 * sizeof(double)) != 0;
  int first = stale ? 0 : in_map;
  if (first == N) {  // nothing new: the map is current (and nothing of it is in flight)
    lm->n_updates++;
    return LSLAM_OK;
  }
  lm->have = false;  // until this update has gone through: an error below leaves a map that is rebuilt next time
  // ---- boxes of the scans that have none yet ----
  live_list(lm, first, N);
  rc = live_stage(lm);
  if (rc) return rc;
  LSLAM_HIP(ctx, lm->d_boxes.reserve((size_t)(N - first) * kBoxWords));
  launch(ctx, "live_box", k_live_box, dim3(N - first), dim3(256), 0, (const int*)lm->d_ids.p, (const double*)lm->d_poses.p,
         v.d_ranges, l, lm->d_boxes.p);
  lm->boxes.resize((size_t)N * kBoxWords);
  LSLAM_HIP(ctx, hipMemcpyAsync(lm->boxes.data() + kBoxWords * (size_t)first, lm->d_boxes.p,
                                (size_t)(N - first) * kBoxWords * sizeof(double),
                                hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  lm->d_ids.trim(); lm->d_poses.trim(); lm->d_boxes.trim();
  double box[4] = {kBoxBig, kBoxBig, -kBoxBig, -kBoxBig};
  for (int s = 0; s < N; s++) {
    const double* b = &lm->boxes[kBoxWords * (size_t)s];
    box[0] = std::min(box[0], b[0]); box[1] = std::min(box[1], b[1]);
    box[2] = std::max(box[2], b[2]); box[3] = std::max(box[3], b[3]);
  }
  const OccGeom g = occ_geom(box, lm->resolution);  // ComputeDimensions (Karto.h:5799-5817), as the one-shot build sizes it
  const size_t cells = (size_t)g.stride * std::max(g.h, 0), words = 2 * std::max<size_t>(cells, 1);
  // a moved min side moves the offset, and with it every WorldToGrid of every ray ever traced
  const bool rebuild = stale || box[0] != lm->box[0] || box[1] != lm->box[1];
  const bool grow = !rebuild && (g.w != og->g.w || g.h != og->g.h);
  int margin = 0;  // old scans at the head of the list that are re-traced for the margin of a grown grid
  if (rebuild && first != 0) {
    first = 0;
    live_list(lm, 0, N);
    rc = live_stage(lm);
    if (rc) return rc;
  } else if (grow) {
    lm->h_ids.clear();
    for (int s = 0; s < first; s++) {  // its rays reach a cell the old bounds clipped (WorldToGrid is monotonic)
      const double* b = &lm->boxes[kBoxWords * (size_t)s];
      if (world_to_grid(b[4], g.ox, g.scale) >= og->g.w || world_to_grid(b[5], g.oy, g.scale) >= og->g.h) lm->h_ids.push_back(s);
    }
    margin = (int)lm->h_ids.size();
    for (int s = first; s < N; s++) lm->h_ids.push_back(s);
    rc = live_stage(lm);
    if (rc) return rc;
  }
  const OccGeom old_g = og->g;
  uint32_t* old_planes = nullptr;  // released once nothing on the stream reads them
  if (grow || words > lm->cap_words) {
    uint32_t* fresh = nullptr;
    if (hipMalloc((void**)&fresh, words * sizeof(uint32_t)) != hipSuccess) {
      (void)hipGetLastError();
      return ctx->fail(LSLAM_ERR_HIP, "cannot allocate %d x %d counters", g.w, g.h);
    }
    old_planes = og->d_pass;
    if (grow && cells > 0)
      launch(ctx, "live_regrid", k_live_regrid, dim3((g.stride + 255) / 256, std::max(g.h, 1)), dim3(256), 0, og->g,
             (const uint32_t*)og->d_pass, (const uint32_t*)og->d_hit, g, fresh, fresh + std::max<size_t>(cells, 1));
    og->d_pass = fresh;
    lm->cap_words = words;
  }
  og->d_hit = og->d_pass + std::max<size_t>(cells, 1);
  og->cells = cells;
  og->g = g;
  og->counters_written();  // new planes, a new geometry or new traces: every path below this line changes the map
  if (rebuild) LSLAM_HIP(ctx, hipMemsetAsync(og->d_pass, 0, words * sizeof(uint32_t), ctx->stream));
  const int K = N - first;
  if (n > 0 && cells > 0) {
    if (margin > 0)
      launch(ctx, "live_trace_margin", k_live_trace, dim3((unsigned)(((long long)margin * n + 255) / 256)), dim3(256), 0, margin,
             (const int*)lm->d_ids.p, (const double*)lm->d_poses.p, v.d_ranges, l, g, og->d_pass, og->d_hit, old_g.w, old_g.h);
    launch(ctx, "live_trace", k_live_trace, dim3((unsigned)(((long long)K * n + 255) / 256)), dim3(256), 0, K,
           (const int*)lm->d_ids.p + margin, (const double*)lm->d_poses.p + 3 * (size_t)margin, v.d_ranges, l, g, og->d_pass,
           og->d_hit, 0, 0);
  }
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (old_planes) (void)hipFree(old_planes);
  lm->d_ids.trim(); lm->d_poses.trim();
  if (e != hipSuccess) return ctx->fail(LSLAM_ERR_HIP, "trace failed: %s", hipGetErrorString(e));
  lm->traced.assign(lm->h_poses.begin(), lm->h_poses.end());
  for (int i = 0; i < 4; i++) lm->box[i] = box[i];
  lm->generation = v.generation;
  lm->have = true;
  lm->n_updates++;
  (rebuild ? lm->n_rebuilds : grow ? lm->n_grows : lm->n_appends)++;
  lm->n_traced += K + margin;
  return LSLAM_OK;
}

}  // namespace

extern "C" {

int lslam_frontend_livemap_create(lslam_frontend* f, double resolution, lslam_livemap** out) {
  if (!f || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  FrontendView v;
  int rc = frontend_view(f, &v);
  if (rc) return rc;
  if (resolution == 0.0 || (resolution > -kTol && resolution < kTol))
    return v.ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "Resolution cannot be 0");  // Karto.h:5627-5630
  lslam_livemap* lm = new lslam_livemap();
  lm->f = f;
  lm->ctx = v.ctx;
  lm->resolution = resolution;
  lm->og = new lslam_occgrid();
  lm->og->ctx = v.ctx;
  lm->og->g.scale = 1.0 / resolution;
  *out = lm;
  return LSLAM_OK;
}

void lslam_livemap_destroy(lslam_livemap* lm) {
  if (!lm) return;
  (void)hipSetDevice(lm->ctx->device);
  lslam_occgrid_destroy(lm->og);  // waits for the stream, frees the planes
  lm->d_ids.release();
  lm->d_poses.release();
  lm->d_boxes.release();
  delete lm;
}

int lslam_livemap_update(lslam_livemap* lm) {
  if (!lm) return LSLAM_ERR_INVALID_ARGUMENT;
  return live_update(lm);
}

lslam_occgrid* lslam_livemap_grid(lslam_livemap* lm) { return lm && lm->have ? lm->og : nullptr; }

int lslam_livemap_stats(const lslam_livemap* lm, int64_t out[6]) {
  if (!lm || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = lm->n_updates;
  out[1] = lm->n_appends;
  out[2] = lm->n_grows;
  out[3] = lm->n_rebuilds;
  out[4] = lm->n_traced;
  out[5] = lm->have ? (int64_t)(lm->traced.size() / 3) : 0;
  return LSLAM_OK;
}

}  // extern "C"
