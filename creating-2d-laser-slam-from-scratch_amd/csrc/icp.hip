// lesson2 point-to-point ICP pair matching on the device: ConvertScan2PointCloud and ScanMatchWithICP
// (lesson2/src/scan_match_icp.cc:89-164), and the NaN cloud of lesson2/src/scan_to_pointclod2_converter.cc.
// PARITY UNPINNED: the reference's arithmetic lives in PCL (IterativeClosestPoint, FLANN, Eigen), which is neither vendored nor
// pinned.  What the results are DEFINED by is this project's own fp64 restatement of PCL 1.8's computeTransformation with
// DefaultConvergenceCriteria, `icp` in tools/icp_cpu.py; the five deliberate rules are in include/lslam_gpu.h.
//
// One workgroup of 256 threads per pair, ONE launch per batch, the iterations loop on the device, everything per pair in LDS:
//   1. stage: the source x, y as float32, the target x, y as fp64 (a masked or non-finite target point is staged as NaN: no
//      distance to it is ever `<` the best), a byte per source point that says whether it takes part.
//   2. per iteration, from T = (c, s, tx, ty): every lane owns the source points tid, tid + 256, ...; it transforms up to four
//      of them and walks the target array in ascending index -- every lane reads the same LDS address, a broadcast -- keeping
//      the best (d2, j) in registers under a strict `<`: the lowest index among equals wins.
//   3. the sums, in a fixed order: per-lane partials in ascending i, one shuffle tree per wave, the four waves in order.  Two
//      passes: the means of the accepted pairs (with the count and the sum of d2), then the centred sums.
//   4. the closed form, the composition and the stop rules: every lane does the same fp64 arithmetic on the same sums, so no
//      hand-over; cos / sin / atan2 are the device libm's.
// After the loop one more search gives getFitnessScore().  The loops are bounded by the point count and max_iterations: no
// spins, no hand-overs between blocks, no scratch.
#include <cfloat>
#include <cmath>

#include "common.hpp"

using namespace lslam;

namespace {

constexpr int kIcThreads = 256;
constexpr int kIcWaves = kIcThreads / 64;
constexpr int kIcMax = LSLAM_ICP_MAX_POINTS;
constexpr int kIcSums = 8;
constexpr unsigned short kIcNone = 0xffff;
static_assert(sizeof(lslam_icp_record) == 64, "lslam_icp_record is 64 bytes");
static_assert(sizeof(lslam_icp_params) == 48, "lslam_icp_params is 48 bytes");
static_assert(kIcMax < kIcNone, "correspondences are kept in 16 bits");

struct IcParams {  // what the kernel reads
  double max_d2, tf_eps, fit_eps, abs_mse;
  int max_iter, skip;
};

struct IcShared {                  // 27 bytes per point + the reduction scratch: 54.25 KB, two pairs per CU
  double2 t[kIcMax];               // the target x, y; NaN where the point does not take part
  float2 s[kIcMax];                // the source x, y as stored
  unsigned short corr[kIcMax];     // by source point: the accepted target index, kIcNone: none
  unsigned char sok[kIcMax];       // by source point: takes part
  double red[kIcWaves][kIcSums];
};

struct IcOut {
  double x[3], fitness, mse, inc[3];
  int converged, iterations, ncorr, state;
};

// v[i] <- the block's sum of v[i], the same in every thread and in a fixed order
template <int N>
__device__ __forceinline__ void ic_reduce(IcShared& sh, double (&v)[N]) {
  static_assert(N <= kIcSums, "");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; i++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[i] += __shfl_down(v[i], off);
    if (lane == 0) sh.red[wv][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; i++) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kIcWaves; w++) t += sh.red[w][i];
    v[i] = t;
  }
  __syncthreads();
}

// NP source points of this lane (tiles t0 .. t0 + NP - 1) against every target point.  sums: px, py, qx, qy, d2, count of the
// accepted pairs.  gate: accept iff d2 <= max_d2; without it every point that found a target counts (the fitness score).
template <int NP>
__device__ __forceinline__ void ic_search_tiles(IcShared& sh, int n, int t0, double c, double s, double tx, double ty, bool gate,
                                                double max_d2, double (&sums)[6], int32_t* dbg_corr, double* dbg_d2) {
  const int tid = threadIdx.x;
  double px[NP], py[NP], bd[NP];
  int bj[NP];
  bool any = false;
#pragma unroll
  for (int k = 0; k < NP; k++) {
    const int i = (t0 + k) * kIcThreads + tid;
    const bool ok = i < n && sh.sok[i];
    const double sx = ok ? (double)sh.s[i].x : 0.0, sy = ok ? (double)sh.s[i].y : 0.0;
    px[k] = ok ? (c * sx - s * sy) + tx : __builtin_nan("");
    py[k] = ok ? (s * sx + c * sy) + ty : __builtin_nan("");
    bd[k] = __builtin_inf();
    bj[k] = -1;
    any = any || ok;
  }
  if (__any(any)) {  // (a wave none of whose lanes has a point in these tiles skips the walk: 1081 points leave 57 in the fifth)
#pragma unroll 4
    for (int j = 0; j < n; j++) {
      const double2 q = sh.t[j];
#pragma unroll
      for (int k = 0; k < NP; k++) {
        const double ex = px[k] - q.x, ey = py[k] - q.y;
        const double d = ex * ex + ey * ey;
        if (d < bd[k]) {  // strict: the lowest index among equals; false for a NaN on either side
          bd[k] = d;
          bj[k] = j;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NP; k++) {  // ascending i
    const int i = (t0 + k) * kIcThreads + tid;
    if (i >= n) continue;
    const bool acc = bj[k] >= 0 && (!gate || bd[k] <= max_d2);
    sh.corr[i] = acc ? (unsigned short)bj[k] : kIcNone;
    if (dbg_corr) {
      dbg_corr[i] = acc ? bj[k] : -1;
      dbg_d2[i] = bd[k];
    }
    if (acc) {
      const double2 q = sh.t[bj[k]];
      sums[0] += px[k]; sums[1] += py[k]; sums[2] += q.x; sums[3] += q.y; sums[4] += bd[k]; sums[5] += 1.0;
    }
  }
}

// one search of the whole block: the reduced sums in every thread
__device__ void ic_search(IcShared& sh, int n, double c, double s, double tx, double ty, bool gate, double max_d2,
                          double (&sums)[6], int32_t* dbg_corr, double* dbg_d2) {
#pragma unroll
  for (int i = 0; i < 6; i++) sums[i] = 0.0;
  const int tiles = (n + kIcThreads - 1) / kIcThreads;
  int t = 0;
#pragma unroll 1
  for (; t + 4 <= tiles; t += 4) ic_search_tiles<4>(sh, n, t, c, s, tx, ty, gate, max_d2, sums, dbg_corr, dbg_d2);
#pragma unroll 1
  for (; t + 2 <= tiles; t += 2) ic_search_tiles<2>(sh, n, t, c, s, tx, ty, gate, max_d2, sums, dbg_corr, dbg_d2);
#pragma unroll 1
  for (; t < tiles; t++) ic_search_tiles<1>(sh, n, t, c, s, tx, ty, gate, max_d2, sums, dbg_corr, dbg_d2);
  ic_reduce(sh, sums);
}

// icp(source, target, first guess g) for the whole block; every thread returns the same `out`.  xyz: n x 3 float32; valid: n
// bytes or NULL.  dbg_*: per source point, or NULL.
__device__ void ic_match(IcShared& sh, const IcParams& P, int n, const float* __restrict__ src, const float* __restrict__ tgt,
                         const uint8_t* __restrict__ src_valid, const uint8_t* __restrict__ tgt_valid, double gx, double gy,
                         double gth, IcOut& out, int32_t* dbg_corr, double* dbg_d2) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += kIcThreads) {
    const float sx = src[3 * (size_t)i], sy = src[3 * (size_t)i + 1];
    const float qx = tgt[3 * (size_t)i], qy = tgt[3 * (size_t)i + 1];
    const bool s_ok = isfinite(sx) && isfinite(sy) && !(P.skip && src_valid && !src_valid[i]);
    const bool t_ok = isfinite(qx) && isfinite(qy) && !(P.skip && tgt_valid && !tgt_valid[i]);
    sh.s[i] = make_float2(sx, sy);
    sh.sok[i] = s_ok ? 1 : 0;
    sh.t[i] = t_ok ? make_double2((double)qx, (double)qy) : make_double2(__builtin_nan(""), __builtin_nan(""));
  }
  __syncthreads();
  double c = cos(gth), s = sin(gth), tx = gx, ty = gy, prev = DBL_MAX, mse = 0.0;
  int it = 0, ncorr = 0, state = 0;
  out.inc[0] = out.inc[1] = out.inc[2] = __builtin_nan("");
  double sums[6];
#pragma unroll 1
  while (true) {
    ic_search(sh, n, c, s, tx, ty, true, P.max_d2, sums, dbg_corr, dbg_d2);
    ncorr = (int)sums[5];
    if (ncorr < 3) {
      state = 5;
      break;
    }
    const double cnt = (double)ncorr;
    const double pbx = sums[0] / cnt, pby = sums[1] / cnt, qbx = sums[2] / cnt, qby = sums[3] / cnt;
    double cs[4] = {0.0, 0.0, 0.0, 0.0};  // Sxx, Sxy, Syx, Syy
    for (int i = tid; i < n; i += kIcThreads) {
      const unsigned short j = sh.corr[i];
      if (j == kIcNone) continue;
      const double sx = (double)sh.s[i].x, sy = (double)sh.s[i].y;
      const double ux = ((c * sx - s * sy) + tx) - pbx, uy = ((s * sx + c * sy) + ty) - pby;
      const double2 q = sh.t[j];
      const double vx = q.x - qbx, vy = q.y - qby;
      cs[0] += ux * vx; cs[1] += ux * vy; cs[2] += uy * vx; cs[3] += uy * vy;
    }
    ic_reduce(sh, cs);
    const double th = atan2(cs[1] - cs[2], cs[0] + cs[3]);
    const double ct = cos(th), st = sin(th);
    const double ix = qbx - (ct * pbx - st * pby), iy = qby - (st * pbx + ct * pby);
    // T <- increment o T
    const double nc = ct * c - st * s, ns = st * c + ct * s;
    const double ntx = (ct * tx - st * ty) + ix, nty = (st * tx + ct * ty) + iy;
    c = nc; s = ns; tx = ntx; ty = nty;
    it++;
    mse = sums[4] / cnt;
    out.inc[0] = ix; out.inc[1] = iy; out.inc[2] = th;
    if (it >= P.max_iter) state = 1;
    else if (ct >= 1.0 - P.tf_eps && ix * ix + iy * iy <= P.tf_eps) state = 2;
    else if (fabs(mse - prev) < P.abs_mse) state = 3;
    else if (fabs(mse - prev) / prev < P.fit_eps) state = 4;
    if (state) break;
    prev = mse;
  }
  if (state == 5) out.inc[0] = out.inc[1] = out.inc[2] = __builtin_nan("");
  double fs[6];
  ic_search(sh, n, c, s, tx, ty, false, 0.0, fs, nullptr, nullptr);  // (ends with a barrier: the LDS is quiet)
  out.fitness = fs[5] > 0.0 ? fs[4] / fs[5] : DBL_MAX;
  out.x[0] = tx; out.x[1] = ty; out.x[2] = atan2(s, c);
  out.mse = mse;
  out.converged = (state >= 1 && state <= 4) ? 1 : 0;
  out.iterations = it;
  out.ncorr = ncorr;
  out.state = state;
}

__global__ void __launch_bounds__(kIcThreads)
k_icp_match(IcParams P, int n, const float* __restrict__ xyz, const uint8_t* __restrict__ valid, const int32_t* __restrict__ pair_src,
            const int32_t* __restrict__ pair_tgt, const double* __restrict__ guess, lslam_icp_record* __restrict__ out) {
  __shared__ IcShared sh;
  const size_t b = blockIdx.x;
  const double gx = guess ? guess[3 * b] : 0.0, gy = guess ? guess[3 * b + 1] : 0.0, gth = guess ? guess[3 * b + 2] : 0.0;
  const size_t so = (size_t)pair_src[b] * n, to = (size_t)pair_tgt[b] * n;
  IcOut o;
  ic_match(sh, P, n, xyz + 3 * so, xyz + 3 * to, valid ? valid + so : nullptr, valid ? valid + to : nullptr, gx, gy, gth, o, nullptr,
           nullptr);
  if (threadIdx.x == 0) {
    lslam_icp_record r;
    r.x[0] = o.x[0]; r.x[1] = o.x[1]; r.x[2] = o.x[2];
    r.fitness = o.fitness;
    r.mse = o.mse;
    r.converged = o.converged; r.iterations = o.iterations; r.ncorr = o.ncorr; r.state = o.state;
    r.reserved = 0.0;
    out[b] = r;
  }
}

// one iteration from x_in with the decisions per source point; res = [inc 3 | mse]
__global__ void __launch_bounds__(kIcThreads)
k_icp_debug(IcParams P, int n, const float* __restrict__ src, const float* __restrict__ tgt, const uint8_t* __restrict__ src_valid,
            const uint8_t* __restrict__ tgt_valid, const double* __restrict__ x_in, int32_t* __restrict__ corr,
            double* __restrict__ d2, double* __restrict__ res, int32_t* __restrict__ ncorr) {
  __shared__ IcShared sh;
  IcOut o;
  P.max_iter = 1;
  ic_match(sh, P, n, src, tgt, src_valid, tgt_valid, x_in[0], x_in[1], x_in[2], o, corr, d2);
  if (threadIdx.x == 0) {
    res[0] = o.inc[0]; res[1] = o.inc[1]; res[2] = o.inc[2];
    res[3] = o.mse;
    *ncorr = o.ncorr;
  }
}

// ConvertScan2PointCloud: a tile of 256 beams of one scan per block
__global__ void __launch_bounds__(256)
k_icp_cloud(float angle_min, float angle_inc, float range_min, float range_max, int nan_fill, int n, int tiles, int ranges_stride,
            const float* __restrict__ ranges, float* __restrict__ xyz, uint8_t* __restrict__ valid) {
  const size_t scan = blockIdx.x / (unsigned)tiles;
  const int i = (int)(blockIdx.x % (unsigned)tiles) * 256 + threadIdx.x;
  if (i >= n) return;
  const float r = ranges[scan * ranges_stride + i];
  const bool ok = isfinite(r) && r > range_min && r < range_max;
  const float angle = angle_min + (float)i * angle_inc;  // float32, as the node's (-ffp-contract=off: two roundings)
  const float fill = nan_fill ? __builtin_nanf("") : 0.0f;
  float* p = xyz + 3 * (scan * n + i);
  p[0] = ok ? (float)((double)r * cos((double)angle)) : fill;
  p[1] = ok ? (float)((double)r * sin((double)angle)) : fill;
  p[2] = ok ? 0.0f : fill;
  valid[scan * n + i] = ok ? 1 : 0;
}

IcParams ic_params(const lslam_icp_params& p) {
  IcParams P;
  P.max_d2 = p.max_correspondence_distance * p.max_correspondence_distance;
  P.tf_eps = p.transformation_epsilon;
  P.fit_eps = p.euclidean_fitness_epsilon;
  P.abs_mse = p.absolute_mse;
  P.max_iter = p.max_iterations;
  P.skip = p.skip_invalid ? 1 : 0;
  return P;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// lslam_icp: the batched pair match.  The pair indices go up through a ring of pinned slots (the _dev forms return while their
// launch is still queued); everything else the host forms need belongs to the handle.
// ------------------------------------------------------------------------------------------
struct lslam_icp {
  lslam_context* ctx = nullptr;
  lslam_icp_params params;
  bool laser_set = false;
  float angle_min = 0, angle_inc = 0, range_min = 0, range_max = 0;
  static constexpr int kSlots = 4;
  int32_t* h_pairs = nullptr;  // pinned: kSlots x [source x cap | target x cap]
  size_t pair_cap = 0;
  DevBuf<int32_t> d_pairs[kSlots];
  hipEvent_t slot_done[kSlots] = {};
  bool slot_in_flight[kSlots] = {};
  int next_slot = 0;
  DevBuf<float> d_ranges, d_xyz;
  DevBuf<uint8_t> d_valid;
  DevBuf<double> d_guess;
  DevBuf<lslam_icp_record> d_rec;
  unsigned char* h_io = nullptr;  // pinned: inputs up, results down
  size_t h_io_cap = 0;
  DevBuf<unsigned char> d_dbg;
  int64_t n_pairs = 0, n_launches = 0, n_growths = 0, n_waits = 0;
};

namespace {

template <typename T>
int ic_reserve(lslam_icp* f, DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return LSLAM_OK;
  LSLAM_HIP(f->ctx, b.reserve(n));
  f->n_growths++;
  return LSLAM_OK;
}

int ic_pinned(lslam_icp* f, unsigned char** p, size_t* cap, size_t want) {
  if (want <= *cap) return LSLAM_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t c = want + want / 4 + 256;
  LSLAM_HIP(f->ctx, hipHostMalloc((void**)p, c, hipHostMallocDefault));
  *cap = c;
  f->n_growths++;
  return LSLAM_OK;
}

int ic_wait_slot(lslam_icp* f, int q) {
  if (f->slot_in_flight[q] && hipEventQuery(f->slot_done[q]) != hipSuccess) {
    (void)hipGetLastError();  // hipErrorNotReady is no error
    LSLAM_HIP(f->ctx, hipEventSynchronize(f->slot_done[q]));
    f->n_waits++;
  }
  f->slot_in_flight[q] = false;
  return LSLAM_OK;
}

// cloud: the clouds forms (no laser needed, no stride)
int ic_check(lslam_icp* f, const char* who, bool cloud, int n_scans, int n, const void* in, int ranges_stride, int n_pairs,
             const int32_t* pair_src, const int32_t* pair_tgt, const void* out) {
  if (!f || n_scans < 0 || n < 0 || n_pairs < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (n_pairs == 0) return LSLAM_OK;
  if (!cloud && !f->laser_set) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: lslam_icp_set_laser has not been called", who);
  if (n > LSLAM_ICP_MAX_POINTS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d points per cloud (got %d)", who, LSLAM_ICP_MAX_POINTS, n);
  if (!in || !pair_src || !pair_tgt || !out || (!cloud && ranges_stride < n))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: the input block%s, pair_source, pair_target and out are required", who,
                     cloud ? "" : ", ranges_stride >= n_readings");
  for (int b = 0; b < n_pairs; b++)
    if (pair_src[b] < 0 || pair_src[b] >= n_scans || pair_tgt[b] < 0 || pair_tgt[b] >= n_scans)
      return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: pair %d (%d, %d) is outside the %d clouds", who, b, pair_src[b], pair_tgt[b],
                       n_scans);
  return LSLAM_OK;
}

int ic_convert(lslam_icp* f, int n_scans, int n, const float* d_ranges, int ranges_stride, float* d_xyz, uint8_t* d_valid) {
  if (n_scans == 0 || n == 0) return LSLAM_OK;
  lslam_context* ctx = f->ctx;
  const int tiles = (n + 255) / 256;
  launch(ctx, "icp_cloud", k_icp_cloud, dim3((unsigned)((size_t)tiles * n_scans)), dim3(256), 0, f->angle_min, f->angle_inc, f->range_min,
         f->range_max, f->params.invalid_as_nan ? 1 : 0, n, tiles, ranges_stride, d_ranges, d_xyz, d_valid);
  LSLAM_HIP(ctx, hipGetLastError());
  f->n_launches++;
  return LSLAM_OK;
}

// the pair indices up through the next pinned slot, then ONE launch for the whole batch
int ic_enqueue(lslam_icp* f, int n, const float* d_xyz, const uint8_t* d_valid, int n_pairs, const int32_t* pair_src,
               const int32_t* pair_tgt, const double* d_guess, lslam_icp_record* d_out) {
  lslam_context* ctx = f->ctx;
  int rc;
  if ((size_t)n_pairs > f->pair_cap) {  // every slot grows together: none may be in flight
    for (int q = 0; q < lslam_icp::kSlots; q++)
      if ((rc = ic_wait_slot(f, q))) return rc;
    size_t cap_bytes = f->pair_cap * 2 * sizeof(int32_t) * lslam_icp::kSlots;
    const size_t per = (size_t)n_pairs + (size_t)n_pairs / 4 + 64;
    unsigned char* p = reinterpret_cast<unsigned char*>(f->h_pairs);
    rc = ic_pinned(f, &p, &cap_bytes, per * 2 * sizeof(int32_t) * lslam_icp::kSlots);
    f->h_pairs = reinterpret_cast<int32_t*>(p);
    f->pair_cap = 0;
    if (rc) return rc;
    for (int q = 0; q < lslam_icp::kSlots; q++)
      if ((rc = ic_reserve(f, f->d_pairs[q], 2 * per))) return rc;
    f->pair_cap = per;
  }
  const int q = f->next_slot;
  f->next_slot = (q + 1) % lslam_icp::kSlots;
  if ((rc = ic_wait_slot(f, q))) return rc;
  int32_t* up = f->h_pairs + (size_t)q * 2 * f->pair_cap;
  memcpy(up, pair_src, (size_t)n_pairs * sizeof(int32_t));
  memcpy(up + n_pairs, pair_tgt, (size_t)n_pairs * sizeof(int32_t));
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_pairs[q].p, up, 2 * (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  launch(ctx, "icp_match", k_icp_match, dim3((unsigned)n_pairs), dim3(kIcThreads), 0, ic_params(f->params), n, d_xyz, d_valid,
         (const int32_t*)f->d_pairs[q].p, (const int32_t*)(f->d_pairs[q].p + n_pairs), d_guess, d_out);
  LSLAM_HIP(ctx, hipGetLastError());
  LSLAM_HIP(ctx, hipEventRecord(f->slot_done[q], ctx->stream));
  f->slot_in_flight[q] = true;
  f->n_launches++;
  f->n_pairs += n_pairs;
  return LSLAM_OK;
}

// the end of a host form: the records down, ONE wait
int ic_finish(lslam_icp* f, int n_pairs, lslam_icp_record* out) {
  lslam_context* ctx = f->ctx;
  const size_t rec_bytes = (size_t)n_pairs * sizeof(lslam_icp_record);
  LSLAM_HIP(ctx, hipMemcpyAsync(f->h_io, f->d_rec.p, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  for (int q = 0; q < lslam_icp::kSlots; q++) f->slot_in_flight[q] = false;  // the stream has drained
  memcpy(out, f->h_io, rec_bytes);
  return LSLAM_OK;
}

}  // namespace

extern "C" {

void lslam_icp_params_defaults(lslam_icp_params* p) {
  if (!p) return;
  p->max_correspondence_distance = std::sqrt(DBL_MAX);
  p->transformation_epsilon = 0.0;
  p->euclidean_fitness_epsilon = -DBL_MAX;
  p->absolute_mse = 1e-12;
  p->max_iterations = 10;
  p->skip_invalid = 0;
  p->invalid_as_nan = 0;
  p->reserved = 0;
}

int lslam_icp_create(lslam_context* ctx, const lslam_icp_params* params, lslam_icp** out) {
  if (!ctx || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!params) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_icp_create: params are required");
  if (params->max_iterations < 1) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_icp_create: max_iterations must be >= 1");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_icp* f = new lslam_icp();
  f->ctx = ctx;
  f->params = *params;
  for (int q = 0; q < lslam_icp::kSlots; q++) {
    hipError_t e = hipEventCreateWithFlags(&f->slot_done[q], hipEventDisableTiming);
    if (e != hipSuccess) {
      for (int k = 0; k < q; k++) (void)hipEventDestroy(f->slot_done[k]);
      delete f;
      return ctx->fail(LSLAM_ERR_HIP, "lslam_icp_create: hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
    }
  }
  *out = f;
  return LSLAM_OK;
}

void lslam_icp_destroy(lslam_icp* f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  for (int q = 0; q < lslam_icp::kSlots; q++) {
    (void)hipEventDestroy(f->slot_done[q]);
    f->d_pairs[q].release();
  }
  if (f->h_pairs) (void)hipHostFree(f->h_pairs);
  if (f->h_io) (void)hipHostFree(f->h_io);
  f->d_ranges.release();
  f->d_xyz.release();
  f->d_valid.release();
  f->d_guess.release();
  f->d_rec.release();
  f->d_dbg.release();
  delete f;
}

int lslam_icp_set_laser(lslam_icp* f, double angle_min, double angle_increment, double range_min, double range_max) {
  if (!f) return LSLAM_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(angle_min) || !std::isfinite(angle_increment) || !((float)range_min < (float)range_max))
    return f->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_icp_set_laser: finite angles and range_min < range_max are required");
  f->angle_min = (float)angle_min;
  f->angle_inc = (float)angle_increment;
  f->range_min = (float)range_min;
  f->range_max = (float)range_max;
  f->laser_set = true;
  return LSLAM_OK;
}

int lslam_icp_stats(const lslam_icp* f, int64_t out[4]) {
  if (!f || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = f->n_pairs; out[1] = f->n_launches; out[2] = f->n_growths; out[3] = f->n_waits;
  return LSLAM_OK;
}

int lslam_icp_convert_batch_dev(lslam_icp* f, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride,
                                float* out_xyz_dev, uint8_t* out_valid_dev) {
  if (!f || n_scans < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (!f->laser_set) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_icp_convert_batch_dev: lslam_icp_set_laser has not been called");
  if (n_scans == 0 || n_readings == 0) return LSLAM_OK;
  if (!ranges_dev || !out_xyz_dev || !out_valid_dev || ranges_stride < n_readings)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_icp_convert_batch_dev: ranges, ranges_stride >= n_readings, out_xyz and out_valid are required");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  return ic_convert(f, n_scans, n_readings, ranges_dev, ranges_stride, out_xyz_dev, out_valid_dev);
}

int lslam_icp_convert_batch(lslam_icp* f, int n_scans, int n_readings, const float* ranges, int ranges_stride, float* out_xyz,
                            uint8_t* out_valid) {
  if (!f || n_scans < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (!f->laser_set) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_icp_convert_batch: lslam_icp_set_laser has not been called");
  if (n_scans == 0 || n_readings == 0) return LSLAM_OK;
  if (!ranges || !out_xyz || !out_valid || ranges_stride < n_readings)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_icp_convert_batch: ranges, ranges_stride >= n_readings, out_xyz and out_valid are required");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t pts = (size_t)n_scans * n_readings, plane = pts * sizeof(float), xyz_bytes = 3 * plane;
  int rc;
  // pinned: [xyz | ranges | valid]
  if ((rc = ic_pinned(f, &f->h_io, &f->h_io_cap, xyz_bytes + plane + pts)) || (rc = ic_reserve(f, f->d_ranges, pts)) ||
      (rc = ic_reserve(f, f->d_xyz, 3 * pts)) || (rc = ic_reserve(f, f->d_valid, pts)))
    return rc;
  float* const h_r = reinterpret_cast<float*>(f->h_io + xyz_bytes);
  for (int k = 0; k < n_scans; k++)
    memcpy(h_r + (size_t)k * n_readings, ranges + (size_t)k * ranges_stride, (size_t)n_readings * sizeof(float));
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_ranges.p, h_r, plane, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = ic_convert(f, n_scans, n_readings, f->d_ranges.p, n_readings, f->d_xyz.p, f->d_valid.p))) return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(f->h_io, f->d_xyz.p, xyz_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(f->h_io + xyz_bytes + plane, f->d_valid.p, pts, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  for (int q = 0; q < lslam_icp::kSlots; q++) f->slot_in_flight[q] = false;
  memcpy(out_xyz, f->h_io, xyz_bytes);
  memcpy(out_valid, f->h_io + xyz_bytes + plane, pts);
  return LSLAM_OK;
}

int lslam_icp_match_batch_dev(lslam_icp* f, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride, int n_pairs,
                              const int32_t* pair_source, const int32_t* pair_target, const double* first_guess_dev,
                              lslam_icp_record* out_dev) {
  int rc = ic_check(f, "lslam_icp_match_batch_dev", false, n_scans, n_readings, ranges_dev, ranges_stride, n_pairs, pair_source,
                    pair_target, out_dev);
  if (rc || n_pairs == 0) return rc;
  LSLAM_HIP(f->ctx, hipSetDevice(f->ctx->device));
  const size_t pts = (size_t)n_scans * n_readings;
  if ((rc = ic_reserve(f, f->d_xyz, 3 * pts)) || (rc = ic_reserve(f, f->d_valid, pts)) ||
      (rc = ic_convert(f, n_scans, n_readings, ranges_dev, ranges_stride, f->d_xyz.p, f->d_valid.p)))
    return rc;
  return ic_enqueue(f, n_readings, f->d_xyz.p, f->d_valid.p, n_pairs, pair_source, pair_target, first_guess_dev, out_dev);
}

int lslam_icp_match_batch(lslam_icp* f, int n_scans, int n_readings, const float* ranges, int ranges_stride, int n_pairs,
                          const int32_t* pair_source, const int32_t* pair_target, const double* first_guess, lslam_icp_record* out) {
  int rc = ic_check(f, "lslam_icp_match_batch", false, n_scans, n_readings, ranges, ranges_stride, n_pairs, pair_source, pair_target,
                    out);
  if (rc || n_pairs == 0) return rc;
  lslam_context* ctx = f->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t pts = (size_t)n_scans * n_readings, plane = pts * sizeof(float);
  const size_t guess_bytes = first_guess ? (size_t)n_pairs * 3 * sizeof(double) : 0;
  const size_t rec_bytes = (size_t)n_pairs * sizeof(lslam_icp_record);
  // pinned: [records | guesses | ranges] (every call ends with a wait: nothing in flight reads this buffer at the next call)
  if ((rc = ic_pinned(f, &f->h_io, &f->h_io_cap, rec_bytes + guess_bytes + plane)) || (rc = ic_reserve(f, f->d_ranges, pts)) ||
      (rc = ic_reserve(f, f->d_xyz, 3 * pts)) || (rc = ic_reserve(f, f->d_valid, pts)) ||
      (rc = ic_reserve(f, f->d_rec, (size_t)n_pairs)) || (first_guess && (rc = ic_reserve(f, f->d_guess, (size_t)n_pairs * 3))))
    return rc;
  double* const h_guess = reinterpret_cast<double*>(f->h_io + rec_bytes);
  float* const h_r = reinterpret_cast<float*>(f->h_io + rec_bytes + guess_bytes);
  if (n_readings > 0) {
    for (int k = 0; k < n_scans; k++)
      memcpy(h_r + (size_t)k * n_readings, ranges + (size_t)k * ranges_stride, (size_t)n_readings * sizeof(float));
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_ranges.p, h_r, plane, hipMemcpyHostToDevice, ctx->stream));
  }
  if (first_guess) {
    memcpy(h_guess, first_guess, guess_bytes);
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_guess.p, h_guess, guess_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  if ((rc = ic_convert(f, n_scans, n_readings, f->d_ranges.p, n_readings, f->d_xyz.p, f->d_valid.p)) ||
      (rc = ic_enqueue(f, n_readings, f->d_xyz.p, f->d_valid.p, n_pairs, pair_source, pair_target,
                       first_guess ? f->d_guess.p : nullptr, f->d_rec.p)))
    return rc;
  return ic_finish(f, n_pairs, out);
}

int lslam_icp_match_clouds_dev(lslam_icp* f, int n_clouds, int n_points, const float* xyz_dev, const uint8_t* valid_dev, int n_pairs,
                               const int32_t* pair_source, const int32_t* pair_target, const double* first_guess_dev,
                               lslam_icp_record* out_dev) {
  int rc = ic_check(f, "lslam_icp_match_clouds_dev", true, n_clouds, n_points, xyz_dev, 0, n_pairs, pair_source, pair_target, out_dev);
  if (rc || n_pairs == 0) return rc;
  LSLAM_HIP(f->ctx, hipSetDevice(f->ctx->device));
  return ic_enqueue(f, n_points, xyz_dev, valid_dev, n_pairs, pair_source, pair_target, first_guess_dev, out_dev);
}

int lslam_icp_match_clouds(lslam_icp* f, int n_clouds, int n_points, const float* xyz, const uint8_t* valid, int n_pairs,
                           const int32_t* pair_source, const int32_t* pair_target, const double* first_guess, lslam_icp_record* out) {
  int rc = ic_check(f, "lslam_icp_match_clouds", true, n_clouds, n_points, xyz, 0, n_pairs, pair_source, pair_target, out);
  if (rc || n_pairs == 0) return rc;
  lslam_context* ctx = f->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t pts = (size_t)n_clouds * n_points, xyz_bytes = 3 * pts * sizeof(float), valid_bytes = valid ? pts : 0;
  const size_t guess_bytes = first_guess ? (size_t)n_pairs * 3 * sizeof(double) : 0;
  const size_t rec_bytes = (size_t)n_pairs * sizeof(lslam_icp_record);
  // pinned: [records | guesses | xyz | valid]
  if ((rc = ic_pinned(f, &f->h_io, &f->h_io_cap, rec_bytes + guess_bytes + xyz_bytes + valid_bytes)) ||
      (rc = ic_reserve(f, f->d_xyz, 3 * pts)) || (valid && (rc = ic_reserve(f, f->d_valid, pts))) ||
      (rc = ic_reserve(f, f->d_rec, (size_t)n_pairs)) || (first_guess && (rc = ic_reserve(f, f->d_guess, (size_t)n_pairs * 3))))
    return rc;
  unsigned char* const h_guess = f->h_io + rec_bytes;
  unsigned char* const h_xyz = h_guess + guess_bytes;
  unsigned char* const h_valid = h_xyz + xyz_bytes;
  if (pts > 0) {
    memcpy(h_xyz, xyz, xyz_bytes);
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_xyz.p, h_xyz, xyz_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (valid) {
      memcpy(h_valid, valid, valid_bytes);
      LSLAM_HIP(ctx, hipMemcpyAsync(f->d_valid.p, h_valid, valid_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
  }
  if (first_guess) {
    memcpy(h_guess, first_guess, guess_bytes);
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_guess.p, h_guess, guess_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  if ((rc = ic_enqueue(f, n_points, f->d_xyz.p, valid ? f->d_valid.p : nullptr, n_pairs, pair_source, pair_target,
                       first_guess ? f->d_guess.p : nullptr, f->d_rec.p)))
    return rc;
  return ic_finish(f, n_pairs, out);
}

int lslam_icp_debug_iteration(lslam_icp* f, const float* src_xyz, const float* tgt_xyz, const uint8_t* src_valid,
                              const uint8_t* tgt_valid, int n, const double x_in[3], int32_t* corr, double* d2, double inc[3],
                              double* mse, int32_t* ncorr) {
  if (!f) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (!src_xyz || !tgt_xyz || !x_in || !corr || !d2 || !inc || !mse || !ncorr || n < 0)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_icp_debug_iteration: every pointer but the valid bytes is required");
  if (n > LSLAM_ICP_MAX_POINTS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_icp_debug_iteration: at most %d points per cloud (got %d)", LSLAM_ICP_MAX_POINTS, n);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  // device block: [x_in 3 | inc 3 | mse | pad] doubles, d2 doubles, source and target xyz floats, corr int32, ncorr, valid bytes
  const size_t N = (size_t)n, o_d2 = 8 * sizeof(double), o_src = o_d2 + N * 8, o_tgt = o_src + N * 12, o_corr = o_tgt + N * 12,
               o_nc = o_corr + N * 4, o_sv = o_nc + 4, o_tv = o_sv + N, bytes = o_tv + N;
  int rc;
  if ((rc = ic_reserve(f, f->d_dbg, bytes)) || (rc = ic_pinned(f, &f->h_io, &f->h_io_cap, bytes))) return rc;
  memset(f->h_io, 0, bytes);
  memcpy(f->h_io, x_in, 3 * sizeof(double));
  if (n) {
    memcpy(f->h_io + o_src, src_xyz, N * 12);
    memcpy(f->h_io + o_tgt, tgt_xyz, N * 12);
    if (src_valid) memcpy(f->h_io + o_sv, src_valid, N);
    if (tgt_valid) memcpy(f->h_io + o_tv, tgt_valid, N);
  }
  unsigned char* d = f->d_dbg.p;
  LSLAM_HIP(ctx, hipMemcpyAsync(d, f->h_io, bytes, hipMemcpyHostToDevice, ctx->stream));
  launch(ctx, "icp_debug", k_icp_debug, dim3(1), dim3(kIcThreads), 0, ic_params(f->params), n, (const float*)(d + o_src),
         (const float*)(d + o_tgt), src_valid ? (const uint8_t*)(d + o_sv) : nullptr, tgt_valid ? (const uint8_t*)(d + o_tv) : nullptr,
         (const double*)d, (int32_t*)(d + o_corr), (double*)(d + o_d2), (double*)(d + 3 * sizeof(double)), (int32_t*)(d + o_nc));
  LSLAM_HIP(ctx, hipGetLastError());
  f->n_launches++;
  LSLAM_HIP(ctx, hipMemcpyAsync(f->h_io, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  memcpy(inc, f->h_io + 3 * sizeof(double), 3 * sizeof(double));
  memcpy(mse, f->h_io + 6 * sizeof(double), sizeof(double));
  memcpy(ncorr, f->h_io + o_nc, 4);
  if (n) {
    memcpy(corr, f->h_io + o_corr, N * 4);
    memcpy(d2, f->h_io + o_d2, N * 8);
  }
  return LSLAM_OK;
}

}  // extern "C"
