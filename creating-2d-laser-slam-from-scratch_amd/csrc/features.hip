// lesson1 curvature corner extraction on the device: LaserScan::ScanCallback (lesson1/src/feature_detection.cc:77-179), the
// LIO-SAM-style extractor that sits in front of a matcher.  One workgroup per scan, ONE launch per batch, everything per
// scan in LDS, nothing back to the host in between:
//   1. compaction (:93-106): the finite ranges, in order -> v[0..count), map[] = their original beam index
//   2. curvature (:112-124): 5 <= i < count-5, float32, left to right, no contraction:
//        d = v[i-5]+v[i-4]+v[i-3]+v[i-2]+v[i-1] - v[i]*10 + v[i+1]+v[i+2]+v[i+3]+v[i+4]+v[i+5],  c[i] = d*d;  0 elsewhere
//   3. six sectors (:139-146): s = count*j/6, e = count*(j+1)/6 - 1; a sector with s >= e is skipped whole
//   4. selection (:149-170): the reference sorts [s, e) -- WITHOUT e -- and walks k = e .. s, so element e is looked at
//      first and is picked, whatever its value, when c[e] > threshold; the other slots of the 20 go to the largest
//      c > threshold of [s, e), descending
//   5. output (:163): the range of every pick at its original beam, +0.0f elsewhere
// Selection is by RANK, not by sorting.  The candidates (c > thr) of [s, e) are compacted, in any order, into a list of
// 64-bit keys (float bits of c) << 32 | compacted index -- c is positive there, so its bits order as its value does -- and a
// candidate's rank is the number of keys above its own: a larger c, or an EQUAL c and a HIGHER compacted index (the tie rule
// of this library; the reference's order among equal curvatures is whatever its std::sort leaves).  rank < 20 - [c[e] > thr]
// is a pick and the rank is its output slot, so the order the list was filled in does not show.  The loops are bounded by
// the sector size (at most 250): no spins, no hand-overs between blocks, no scratch memory.
#include <cmath>

#include "common.hpp"

using namespace lslam;

namespace {

constexpr int kFeatThreads = 256;
constexpr int kFeatWaves = kFeatThreads / 64;
constexpr int kFeatMax = LSLAM_FEATURE_MAX_READINGS;
constexpr int kFeatTiles = (kFeatMax + kFeatThreads - 1) / kFeatThreads;  // beams per thread: 6
constexpr int kFeatIndex = LSLAM_FEATURE_SECTORS * LSLAM_FEATURE_PICKS;   // out_index slots per scan: 120
static_assert(kFeatIndex <= kFeatThreads, "one thread per out_index slot");
static_assert(sizeof(lslam_feature_record) == 32, "lslam_feature_record is 32 bytes");
static_assert((kFeatMax + LSLAM_FEATURE_SECTORS - 1) / LSLAM_FEATURE_SECTORS <= kFeatThreads, "a sector is one element per thread");

struct FeatShared {                    // 22.6 KB at any n (the arrays are sized for max_scan_count)
  union {
    float v[kFeatMax];                 // the compacted ranges (new_scan), until the curvature is done;
    unsigned long long keys[kFeatMax]; // then sector j's candidate keys, from keys[s] on
  };
  float c[kFeatMax];                   // the curvature by compacted index (scan_curvature_ / scan_smoothness_[].value)
  unsigned short map[kFeatMax];        // compacted index -> original beam (map_index)
  unsigned char picked[kFeatMax];      // by compacted index
  int wave_cnt[kFeatTiles * kFeatWaves];
  int n_cand[LSLAM_FEATURE_SECTORS];   // candidates (c > thr) of [s, e)
};

__device__ __forceinline__ float curvature_at(const float* v, int i) {  // :114-121, every sum and the product rounded
#pragma clang fp contract(off)
  const float d = v[i - 5] + v[i - 4] + v[i - 3] + v[i - 2] + v[i - 1] - v[i] * 10.0f + v[i + 1] + v[i + 2] + v[i + 3] +
                  v[i + 4] + v[i + 5];
  return d * d;
}

__global__ void __launch_bounds__(kFeatThreads)
k_features(int n, int ranges_stride, float thr, const float* __restrict__ ranges, float* __restrict__ out_ranges,
           int32_t* __restrict__ out_index, lslam_feature_record* __restrict__ out_rec, float* __restrict__ out_curvature) {
  __shared__ FeatShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t k = blockIdx.x;
  const float* __restrict__ r = ranges + k * (size_t)ranges_stride;
  // ---- 1. compaction: beam t*256 + tid is this thread's in tile t; one ballot per tile, one barrier for all of them
  float val[kFeatTiles];
  unsigned long long bal[kFeatTiles];
#pragma unroll
  for (int t = 0; t < kFeatTiles; t++) {
    const int i = t * kFeatThreads + tid;
    val[t] = i < n ? r[i] : 0.f;
    bal[t] = __ballot(i < n && isfinite(val[t]));
    if (lane == 0) sh.wave_cnt[t * kFeatWaves + wv] = __popcll(bal[t]);
  }
  for (int i = tid; i < kFeatMax; i += kFeatThreads) sh.picked[i] = 0;
  if (tid < LSLAM_FEATURE_SECTORS) sh.n_cand[tid] = 0;
  __syncthreads();
  int pos[kFeatTiles];  // the compacted index of this thread's beam of tile t, -1 for a dropped one
  int count = 0;
#pragma unroll
  for (int t = 0; t < kFeatTiles; t++)
#pragma unroll
    for (int w = 0; w < kFeatWaves; w++) {
      if (w == wv) pos[t] = count;
      count += sh.wave_cnt[t * kFeatWaves + w];
    }
#pragma unroll
  for (int t = 0; t < kFeatTiles; t++) {
    const int i = t * kFeatThreads + tid;
    if (i < n && ((bal[t] >> lane) & 1ull)) {
      pos[t] += __popcll(bal[t] & ((1ull << lane) - 1ull));  // pos <= i < kFeatMax
      sh.v[pos[t]] = val[t];
      sh.map[pos[t]] = (unsigned short)i;
    } else {
      pos[t] = -1;
    }
  }
  __syncthreads();
  // ---- 2. curvature
  for (int i = tid; i < count; i += kFeatThreads) sh.c[i] = (i >= 5 && i < count - 5) ? curvature_at(sh.v, i) : 0.f;
  __syncthreads();  // (v is dead from here on)
  // ---- 3. sectors: the candidates of [s, e) into keys[s ..]; element s + tid is this thread's
#pragma unroll 1
  for (int j = 0; j < LSLAM_FEATURE_SECTORS; j++) {
    const int s = count * j / 6, e = count * (j + 1) / 6 - 1;
    if (s >= e) continue;  // (block-uniform)
    const int i = s + tid;
    const float mine = i < e ? sh.c[i] : 0.f;
    const bool cand = i < e && mine > thr;
    const unsigned long long cb = __ballot(cand);
    if (cb) {  // (wave-uniform)
      int first = 0;
      if (lane == 0) first = atomicAdd(&sh.n_cand[j], __popcll(cb));
      first = __shfl(first, 0);
      if (cand)  // fewer than e - s candidates: the slot is inside [s, e)
        sh.keys[s + first + __popcll(cb & ((1ull << lane) - 1ull))] = ((unsigned long long)__float_as_uint(mine) << 32) | (unsigned)i;
    }
  }
  __syncthreads();
  // ---- 4. selection: candidate q of sector j is thread 64 * (j % 4) + q's (the usual few dozen candidates of six sectors
  //         spread over the four waves)
  int32_t* __restrict__ idx = out_index + k * (size_t)kFeatIndex;
#pragma unroll 1
  for (int j = 0; j < LSLAM_FEATURE_SECTORS; j++) {
    const int s = count * j / 6, e = count * (j + 1) / 6 - 1;
    if (s >= e) continue;  // (block-uniform)
    const int end_picked = sh.c[e] > thr ? 1 : 0;
    const int nc = sh.n_cand[j];
    const int q = (tid + kFeatThreads - 64 * (j & 3)) & (kFeatThreads - 1);
    if (__ballot(q < nc)) {  // (wave-uniform)
      const unsigned long long mine = q < nc ? sh.keys[s + q] : ~0ull;
      int rank = 0;
      for (int m = 0; m < nc; m++) rank += sh.keys[s + m] > mine ? 1 : 0;  // every lane reads the same key: an LDS broadcast
      if (q < nc && rank < LSLAM_FEATURE_PICKS - end_picked) {
        const unsigned i = (unsigned)mine;
        idx[LSLAM_FEATURE_PICKS * j + rank + end_picked] = sh.map[i];
        sh.picked[i] = 1;
      }
    }
    if (tid == kFeatThreads - 1 && end_picked) {
      idx[LSLAM_FEATURE_PICKS * j] = sh.map[e];
      sh.picked[e] = 1;
    }
  }
  __syncthreads();
  // ---- 5. the unused slots, the record, the image and the curvature plane (each output word is written once)
  auto picks_of = [&](int j) {  // what sector j published: its candidates up to the cut-off, and element e
    const int s = count * j / 6, e = count * (j + 1) / 6 - 1;
    if (s >= e) return 0;
    const int ep = sh.c[e] > thr ? 1 : 0;
    return min(sh.n_cand[j], LSLAM_FEATURE_PICKS - ep) + ep;
  };
  if (tid < kFeatIndex && tid % LSLAM_FEATURE_PICKS >= picks_of(tid / LSLAM_FEATURE_PICKS)) idx[tid] = -1;
  if (tid == 0) {
    lslam_feature_record rec;
    rec.n_valid = count;
    rec.n_corners = 0;
    for (int j = 0; j < LSLAM_FEATURE_SECTORS; j++) rec.n_corners += rec.per_sector[j] = picks_of(j);
    out_rec[k] = rec;
  }
#pragma unroll
  for (int t = 0; t < kFeatTiles; t++) {
    const int i = t * kFeatThreads + tid;
    if (i < n) {
      if (out_ranges) out_ranges[k * (size_t)n + i] = (pos[t] >= 0 && sh.picked[pos[t]]) ? val[t] : 0.f;
      if (out_curvature) out_curvature[k * (size_t)n + i] = pos[t] >= 0 ? sh.c[pos[t]] : 0.f;
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// lslam_features: the handle.  The kernel takes everything it needs as arguments, so the _dev form enqueues one launch and
// nothing else; the host form's HBM and pinned buffers belong to the handle and a shape seen once allocates nothing.
// ------------------------------------------------------------------------------------------
struct lslam_features {
  lslam_context* ctx = nullptr;
  float threshold = 1.0f;  // edge_threshold_ (:69)
  // host form
  DevBuf<float> d_ranges, d_image, d_curv;
  DevBuf<int32_t> d_index;
  DevBuf<lslam_feature_record> d_rec;
  unsigned char* h_io = nullptr;  // pinned: ranges up; image, curvature, index, records down
  size_t h_io_cap = 0;
  int64_t n_scans = 0, n_launches = 0, n_growths = 0, n_waits = 0;
};

namespace {

template <typename T>
int feat_reserve(lslam_features* f, DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return LSLAM_OK;
  LSLAM_HIP(f->ctx, b.reserve(n));
  f->n_growths++;
  return LSLAM_OK;
}

int feat_check(lslam_features* f, const char* who, int n_scans, int n_readings, const void* ranges, int ranges_stride,
               const void* out_index, const void* out_rec) {
  if (!f || n_scans < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_scans == 0) return LSLAM_OK;
  lslam_context* ctx = f->ctx;
  if (n_readings > LSLAM_FEATURE_MAX_READINGS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d readings per scan (got %d)", who, LSLAM_FEATURE_MAX_READINGS, n_readings);
  if (n_scans > 65535) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most 65535 scans per call (got %d)", who, n_scans);
  if (!out_index || !out_rec) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: out_index and out_rec are required", who);
  if (n_readings > 0 && (!ranges || ranges_stride < n_readings))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: ranges and ranges_stride >= n_readings are required", who);
  return LSLAM_OK;
}

// ONE launch for the whole batch (n_readings == 0 launches too: every scan's slots become -1 and its record zero)
void feat_enqueue(lslam_features* f, int n_scans, int n_readings, const float* d_ranges, int ranges_stride, float* d_image,
                  int32_t* d_index, lslam_feature_record* d_rec, float* d_curv) {
  launch(f->ctx, "features", k_features, dim3((unsigned)n_scans), dim3(kFeatThreads), 0, n_readings, ranges_stride, f->threshold,
         d_ranges, d_image, d_index, d_rec, d_curv);
  f->n_launches++;
  f->n_scans += n_scans;
}

}  // namespace

extern "C" {

int lslam_features_create(lslam_context* ctx, lslam_features** out) {
  if (!ctx || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_features* f = new lslam_features();
  f->ctx = ctx;
  *out = f;
  return LSLAM_OK;
}

void lslam_features_destroy(lslam_features* f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  if (f->h_io) (void)hipHostFree(f->h_io);
  f->d_ranges.release();
  f->d_image.release();
  f->d_curv.release();
  f->d_index.release();
  f->d_rec.release();
  delete f;
}

int lslam_features_set_threshold(lslam_features* f, float edge_threshold) {
  if (!f) return LSLAM_ERR_INVALID_ARGUMENT;
  // (a NaN or negative threshold would make the reference pick its value-initialised entries)
  if (!(edge_threshold >= 0.0f))
    return f->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_features_set_threshold: the threshold must be a number >= 0");
  f->threshold = edge_threshold;
  return LSLAM_OK;
}

int lslam_features_stats(const lslam_features* f, int64_t out[4]) {
  if (!f || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = f->n_scans; out[1] = f->n_launches; out[2] = f->n_growths; out[3] = f->n_waits;
  return LSLAM_OK;
}

int lslam_features_batch_dev(lslam_features* f, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride,
                             float* out_ranges_dev, int32_t* out_index_dev, lslam_feature_record* out_rec_dev,
                             float* out_curvature_dev) {
  int rc = feat_check(f, "lslam_features_batch_dev", n_scans, n_readings, ranges_dev, ranges_stride, out_index_dev, out_rec_dev);
  if (rc || n_scans == 0) return rc;
  lslam_context* ctx = f->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  feat_enqueue(f, n_scans, n_readings, ranges_dev, ranges_stride, out_ranges_dev, out_index_dev, out_rec_dev, out_curvature_dev);
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}

int lslam_features_batch(lslam_features* f, int n_scans, int n_readings, const float* ranges, int ranges_stride,
                         float* out_ranges, int32_t* out_index, lslam_feature_record* out_rec, float* out_curvature) {
  int rc = feat_check(f, "lslam_features_batch", n_scans, n_readings, ranges, ranges_stride, out_index, out_rec);
  if (rc || n_scans == 0) return rc;
  lslam_context* ctx = f->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t total = (size_t)n_scans * (size_t)n_readings;
  const size_t plane = total * sizeof(float);
  const size_t index_bytes = (size_t)n_scans * kFeatIndex * sizeof(int32_t), rec_bytes = (size_t)n_scans * sizeof(lslam_feature_record);
  // pinned: [image | curvature | index | records]; the ranges go up through the image part (every call ends with a wait, so
  // nothing in flight reads this buffer when the next call fills it)
  const size_t want = 2 * plane + index_bytes + rec_bytes;
  if (want > f->h_io_cap) {
    if (f->h_io) (void)hipHostFree(f->h_io);
    f->h_io = nullptr;
    f->h_io_cap = 0;
    const size_t cap = want + want / 4 + 256;
    LSLAM_HIP(ctx, hipHostMalloc((void**)&f->h_io, cap, hipHostMallocDefault));
    f->h_io_cap = cap;
    f->n_growths++;
  }
  if ((rc = feat_reserve(f, f->d_ranges, total)) || (rc = feat_reserve(f, f->d_index, (size_t)n_scans * kFeatIndex)) ||
      (rc = feat_reserve(f, f->d_rec, (size_t)n_scans)))
    return rc;
  if (out_ranges && (rc = feat_reserve(f, f->d_image, total))) return rc;
  if (out_curvature && (rc = feat_reserve(f, f->d_curv, total))) return rc;
  unsigned char* const h_image = f->h_io;
  unsigned char* const h_curv = f->h_io + plane;
  unsigned char* const h_index = f->h_io + 2 * plane;
  unsigned char* const h_rec = h_index + index_bytes;
  if (total) {
    float* h_r = reinterpret_cast<float*>(h_image);
    for (int k = 0; k < n_scans; k++)
      memcpy(h_r + (size_t)k * n_readings, ranges + (size_t)k * ranges_stride, (size_t)n_readings * sizeof(float));
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_ranges.p, h_r, plane, hipMemcpyHostToDevice, ctx->stream));
  }
  feat_enqueue(f, n_scans, n_readings, f->d_ranges.p, n_readings, out_ranges ? f->d_image.p : nullptr, f->d_index.p, f->d_rec.p,
               out_curvature ? f->d_curv.p : nullptr);
  LSLAM_HIP(ctx, hipGetLastError());
  if (out_ranges && total) LSLAM_HIP(ctx, hipMemcpyAsync(h_image, f->d_image.p, plane, hipMemcpyDeviceToHost, ctx->stream));
  if (out_curvature && total) LSLAM_HIP(ctx, hipMemcpyAsync(h_curv, f->d_curv.p, plane, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(h_index, f->d_index.p, index_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(h_rec, f->d_rec.p, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  if (out_ranges && total) memcpy(out_ranges, h_image, plane);
  if (out_curvature && total) memcpy(out_curvature, h_curv, plane);
  memcpy(out_index, h_index, index_bytes);
  memcpy(out_rec, h_rec, rec_bytes);
  return LSLAM_OK;
}

}  // extern "C"
