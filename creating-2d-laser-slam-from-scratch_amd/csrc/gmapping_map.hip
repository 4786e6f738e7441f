// lesson4 GMapping hit/visit count map on the device: GMapping::ComputeMap / PublishMap (lesson4/src/gmapping/gmapping.cc:
// 127-242) over a ScanMatcherMap = Map<PointAccumulator, HierarchicalArray2D<PointAccumulator>> (lesson4/include/lesson4/
// gmapping/grid/map.h, harray2d.h), traced with GridLineTraversal::gridLine (gridlinetraversal.h).  DESIGN.md §4.11.
//
// Planes (row-major y * size_x + x, SoA): visits i32, n i32, acc_x f32, acc_y f32, plus one byte per 32x32 patch (the
// reference's active area).  One integrate of S scans x B beams is five kernel kinds on the context stream:
//   k_gm_endpoint  thread per (scan, beam): filter, clamp, endpoint, p0 / p1, a hit record (key = cell, value = seq)
//   k_gm_trace     wave per beam: gridLine cells in closed form, u32 atomic visits++ (integer sums are order-free)
//   k_gm_hist / k_gm_scan / k_gm_scatter   stable LSD radix sort of the hit records by cell (8-bit digits)
//   k_gm_fold      thread per run of equal cells: ONE owner adds the hits of its cell in seq order -- acc is a float sum, and
//                  only this store-then-ordered-sum form reproduces PointAccumulator::update's `acc.x += (float)p.x` bit for bit
// plus k_gm_reset (clears the marked patches only) and k_gm_classify (the published int8 grid).
#include <climits>
#include <cmath>

#include "common.hpp"

using namespace lslam;

namespace {

constexpr int kPatchMag = 5;                 // HierarchicalArray2D's default patchMagnitude (harray2d.h:36, 75-80)
constexpr int kSortTile = 4096;              // records per radix-sort tile: 256 threads x 16 rounds
constexpr int kSortRounds = kSortTile / 256;
constexpr int kMaxLineCells = 1 << 20;       // bound on max(min(maxRange, maxUrange) / delta): lines stay short
constexpr double kMaxCellCoord = 1073741824.0;  // |(p - center) / delta| of a pose: beyond it (int) would not be defined
// cells per axis: mapSize^2 < 2^32 keeps every cell index AND the no-hit key (= mapSize^2) inside the u32 sort keys
constexpr double kMaxAxisCells = 65504.0;
// readings per integrate call: every thread index of every launch stays inside int (endpoint / fold: n + 255)
constexpr long long kMaxReadings = 1ll << 28;
constexpr int kTraceBlocks = 1 << 16;          // the trace kernel's grid strides over the beams beyond 4 * kTraceBlocks

struct GmCfg {
  int n_beams, size_x, size_y, patches_x;
  int sizeX2, sizeY2;
  unsigned n_cells;  // size_x * size_y; also the key of "no hit record"
  double cx, cy, delta, max_range, max_use_range;
};

// Map::world2map (map.h:171-174): (int)round((p - center) / delta) + sizeX2.  Poses are checked on the host to keep the
// rounded value inside int; an endpoint is at most min(maxRange, maxUrange) = kMaxLineCells cells further.
__device__ __forceinline__ int w2m(double p, double c, double delta, int half) { return (int)round((p - c) / delta) + half; }

// the stats counters: one wave ballot per counter, the wave totals summed in LDS, one global atomic per block (a global
// atomic per thread on three addresses held a 4096-scan batch's endpoint pass at 44 ms)
__device__ __forceinline__ void count_block(unsigned* s_cnt, bool used, bool hit, bool drop) {
  const bool flags[3] = {used, hit, drop};
  for (int i = 0; i < 3; i++) {
    const unsigned long long b = __ballot(flags[i]);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_cnt[i], (unsigned)__popcll(b));
  }
}

__global__ void __launch_bounds__(256)
k_gm_endpoint(GmCfg c, int n_rec, const float* __restrict__ ranges, const double* __restrict__ poses,
              const double* __restrict__ cs, int4* __restrict__ lines, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
              float* __restrict__ hx, float* __restrict__ hy, uint8_t* __restrict__ mask, unsigned long long* __restrict__ stats) {
  __shared__ unsigned s_cnt[3];
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  bool used = false, hit = false, drop = false;
  if (t < n_rec) {
    const int scan = t / c.n_beams, beam = t - scan * c.n_beams;
    uint32_t key = c.n_cells;
    vals[t] = (uint32_t)t;  // the sequence number scan * n_beams + beam: the order of this cell's acc sum
    double d = (double)ranges[t];
    used = !(d > c.max_range || d == 0.0 || !isfinite(d));  // gmapping.cc:190-191
    if (!used) {
      lines[t] = make_int4(INT_MIN, 0, 0, 0);
    } else {
      if (d > c.max_use_range) d = c.max_use_range;  // :192-193
      double x = 0.0, y = 0.0, co = 1.0, si = 0.0;
      if (poses) {
        const double* p = poses + 4 * (size_t)scan;
        x = p[0]; y = p[1]; co = p[2]; si = p[3];
      }
      const double ca = cs[beam], sa = cs[c.n_beams + beam];
      // :196-199 with lp = (x, y, theta): phit = lp + d * R(theta) (cos_i, sin_i).  At pose 0, co = 1 and si = 0 make the
      // rotation exact (1 * a - 0 * b == a), so this is the reference's `phit.x += d * a_cos_[i]` bit for bit
      const double phx = x + d * (co * ca - si * sa);
      const double phy = y + d * (si * ca + co * sa);
      const int p0x = w2m(x, c.cx, c.delta, c.sizeX2), p0y = w2m(y, c.cy, c.delta, c.sizeY2);
      const int p1x = w2m(phx, c.cx, c.delta, c.sizeX2), p1y = w2m(phy, c.cy, c.delta, c.sizeY2);
      lines[t] = make_int4(p0x, p0y, p1x, p1y);
      if (d < c.max_use_range) {  // :214-219, 237-241: a hit only below maxUrange
        if (p1x >= 0 && p1y >= 0 && p1x < c.size_x && p1y < c.size_y) {
          key = (uint32_t)p1y * (uint32_t)c.size_x + (uint32_t)p1x;
          hx[t] = (float)phx;  // PointAccumulator::update: acc.x += static_cast<float>(p.x) (map.h:37-48)
          hy[t] = (float)phy;
          uint8_t* m = mask + (p1y >> kPatchMag) * c.patches_x + (p1x >> kPatchMag);
          if (!*m) *m = 1;
          hit = true;
        } else {
          drop = true;
        }
      }
    }
    keys[t] = key;
  }
  count_block(s_cnt, used, hit, drop);
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&stats[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// GridLineTraversal::gridLine(p0, p1) (gridlinetraversal.h:27-207).  gridLineCore walks from the endpoint with the smaller
// MAJOR coordinate (p0 on a tie) one major step at a time, with the decision variable d = 2 dmin - dmaj, d += 2 dmin while
// d < 0, else a minor step and d += 2 (dmin - dmaj); gridLine then reverses the list if it did not start at p0.  The minor
// offset after k major steps is floor((2 dmin k + dmaj) / (2 dmaj)) (induction on the update: it is the largest m with
// 2 dmin k - 2 dmaj m + dmaj >= 0 ... the same d >= 0 test), so each lane computes its cells without the walk.
// Free cells are every point of the line but the last, which is p1 (gmapping.cc:208-211, 230-233): walk index dmaj if the walk began at p0,
// index 0 if it began at p1.  One wave per beam (grid-stride over the beams): the cells of a line are distinct, so no two
// lanes of a wave add to the same counter.  Lines up to 32767 cells (the node's are <= 500) take the minor offset by a
// 32-bit unsigned division (2 dmin k + dmaj < 2^31); longer ones, up to kMaxLineCells, by a 64-bit one.
__device__ __forceinline__ void trace_line(const GmCfg& c, int4 l, int lane, int* __restrict__ visits,
                                           uint8_t* __restrict__ mask, unsigned& dropped) {
  const int dx = abs(l.z - l.x), dy = abs(l.w - l.y);
  const bool xmaj = dy <= dx;
  const int dmaj = xmaj ? dx : dy, dmin = xmaj ? dy : dx;
  // start S of the walk: p1 when p0 has the larger major coordinate
  const bool from_p1 = xmaj ? (l.x > l.z) : (l.y > l.w);
  const int sx = from_p1 ? l.z : l.x, sy = from_p1 ? l.w : l.y;
  const int ex = from_p1 ? l.x : l.z, ey = from_p1 ? l.y : l.w;
  const int smin = xmaj ? (ey >= sy ? 1 : -1) : (ex >= sx ? 1 : -1);
  const int k_excl = from_p1 ? 0 : dmaj;
  const bool short_line = dmaj <= 32767;
  for (int k = lane; k <= dmaj; k += 64) {
    if (k == k_excl) continue;
    int m = 0;
    if (dmaj)
      m = short_line ? (int)((2u * (unsigned)dmin * (unsigned)k + (unsigned)dmaj) / (2u * (unsigned)dmaj))
                     : (int)(((long long)2 * dmin * k + dmaj) / ((long long)2 * dmaj));
    const int x = xmaj ? sx + k : sx + smin * m;
    const int y = xmaj ? sy + smin * m : sy + k;
    if (x < 0 || y < 0 || x >= c.size_x || y >= c.size_y) {  // our contract: outside the storage is skipped and counted
      dropped++;
      continue;
    }
    atomicAdd(&visits[(size_t)y * c.size_x + x], 1);
    uint8_t* pm = mask + (y >> kPatchMag) * c.patches_x + (x >> kPatchMag);
    if (!*pm) *pm = 1;
  }
}

__global__ void __launch_bounds__(256)
k_gm_trace(GmCfg c, int n_rec, const int4* __restrict__ lines, int* __restrict__ visits, uint8_t* __restrict__ mask,
           unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  unsigned dropped = 0;
  for (int rec = blockIdx.x * 4 + (threadIdx.x >> 6); rec < n_rec; rec += gridDim.x * 4) {
    const int4 l = lines[rec];
    if (l.x != INT_MIN) trace_line(c, l, lane, visits, mask, dropped);
  }
  if (dropped) atomicAdd(&stats[2], (unsigned long long)dropped);
}

// ---- stable LSD radix sort of (key, value) by 8-bit digits --------------------------------------------------------------
// hist[d * n_tiles + tile] = how many records of the tile have digit d; its exclusive scan is each (digit, tile)'s first
// output slot, and the scatter ranks the records of a digit inside a tile in index order: stable.
__global__ void __launch_bounds__(256)
k_gm_hist(const uint32_t* __restrict__ keys, int n, int shift, int n_tiles, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * kSortTile;
  for (int r = 0; r < kSortRounds; r++) {
    const int i = base + r * 256 + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of n words in place by one block: each thread sums a contiguous chunk, the 1024 chunk sums are scanned in
// LDS, then each thread rewrites its chunk.  n = 256 * tiles (some 10^5 words for a batch of 4 M records).
__global__ void __launch_bounds__(1024) k_gm_scan(uint32_t* __restrict__ a, int n) {
  __shared__ uint32_t s[1024];
  const int chunk = (n + 1023) / 1024;
  const int b = threadIdx.x * chunk, e = min(n, b + chunk);
  uint32_t sum = 0;
  for (int i = b; i < e; i++) sum += a[i];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const uint32_t v = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0u;
    __syncthreads();
    s[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = s[threadIdx.x] - sum;
  for (int i = b; i < e; i++) {
    const uint32_t v = a[i];
    a[i] = run;
    run += v;
  }
}

__global__ void __launch_bounds__(256)
k_gm_scatter(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin, uint32_t* __restrict__ kout,
             uint32_t* __restrict__ vout, int n, int shift, int n_tiles, const uint32_t* __restrict__ offs) {
  __shared__ uint32_t run[256];
  __shared__ uint32_t wcnt[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  run[threadIdx.x] = offs[(size_t)threadIdx.x * n_tiles + blockIdx.x];
  const int base = blockIdx.x * kSortTile;
  for (int r = 0; r < kSortRounds; r++) {
    const int i = base + r * 256 + threadIdx.x;
    const bool ok = i < n;
    const uint32_t key = ok ? kin[i] : 0u;
    const uint32_t dig = (key >> shift) & 255u;
    for (int w = 0; w < 4; w++) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    // the lanes of this wave with the same digit: one ballot per digit bit
    unsigned long long same = __ballot(ok);
    for (int bit = 0; bit < 8; bit++) {
      const bool b = (dig >> bit) & 1u;
      const unsigned long long v = __ballot(b);
      same &= b ? v : ~v;
    }
    const uint32_t rank = (uint32_t)__popcll(same & lt);
    if (ok && rank + 1 == (uint32_t)__popcll(same)) wcnt[wave][dig] = rank + 1;  // the last lane of the group reports
    __syncthreads();
    if (ok) {
      uint32_t pos = run[dig] + rank;
      for (int w = 0; w < wave; w++) pos += wcnt[w][dig];
      kout[pos] = key;
      vout[pos] = vin[i];
    }
    __syncthreads();
    run[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
    // the next round's clear of wcnt comes after this read: the clear is behind the __syncthreads above the next ballot,
    // and this thread is the only reader of column threadIdx.x
  }
}

// One owner per cell hit in this batch (the first record of its run in the sorted keys): acc += hits in seq order, then n
// and visits by plain read-add-store (the trace kernel's atomics are complete: same stream).
__global__ void __launch_bounds__(256)
k_gm_fold(int n, uint32_t n_cells, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
          const float* __restrict__ hx, const float* __restrict__ hy, int* __restrict__ visits, int* __restrict__ hits,
          float* __restrict__ ax, float* __restrict__ ay) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t k = keys[t];
  if (k >= n_cells || (t > 0 && keys[t - 1] == k)) return;
  float sx = ax[k], sy = ay[k];
  int cnt = 0;
  for (int j = t; j < n && keys[j] == k; j++) {
    const uint32_t v = vals[j];
    sx += hx[v];
    sy += hy[v];
    cnt++;
  }
  ax[k] = sx;
  ay[k] = sy;
  hits[k] += cnt;
  visits[k] += cnt;
}

// block per 32x32 patch: zero the four planes of a marked patch, then its mark
__global__ void __launch_bounds__(256)
k_gm_reset(int size_x, int patches_x, uint8_t* __restrict__ mask, int* __restrict__ visits, int* __restrict__ hits,
           float* __restrict__ ax, float* __restrict__ ay) {
  const int p = blockIdx.x;
  if (!mask[p]) return;
  const int px = p % patches_x, py = p / patches_x;
  for (int j = threadIdx.x; j < 1024; j += 256) {
    const size_t idx = (size_t)((py << kPatchMag) + (j >> kPatchMag)) * size_x + (px << kPatchMag) + (j & 31);
    visits[idx] = 0;
    hits[idx] = 0;
    ax[idx] = 0.f;
    ay[idx] = 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) mask[p] = 0;
}

// PublishMap (gmapping.cc:141-159): cell (x, y) of the storage -> data[width * y + x] = -1 (visits == 0), 100 ((double)n /
// visits > occ_thresh), else 0; published cells beyond the storage keep the 0 of data.resize (:80)
__global__ void __launch_bounds__(256)
k_gm_classify(int size_x, int size_y, int width, int height, double occ_thresh, const int* __restrict__ visits,
              const int* __restrict__ hits, int8_t* __restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)width * height) return;
  const int y = (int)(t / width), x = (int)(t - (long long)y * width);
  int8_t v = 0;
  if (x < size_x && y < size_y) {
    const size_t i = (size_t)y * size_x + x;
    const int vis = visits[i];
    v = vis == 0 ? (int8_t)-1 : ((double)hits[i] * 1 / (double)vis > occ_thresh ? (int8_t)100 : (int8_t)0);  // map.h:27
  }
  out[t] = v;
}

}  // namespace

struct lslam_gmap {
  lslam_context* ctx = nullptr;
  double xmin = 0, ymin = 0, xmax = 0, ymax = 0;
  GmCfg c{};
  int size_y = 0, patches_y = 0, width = 0, height = 0;
  bool have_laser = false;
  int64_t scans = 0;
  // planes: one allocation, visits | n | acc_x | acc_y, then the patch mask; stats: beams used, hits, dropped cells
  void* d_planes = nullptr;
  unsigned long long* d_stats = nullptr;
  DevBuf<double> d_cs, d_poses;
  DevBuf<float> d_ranges, d_hx, d_hy;
  DevBuf<int4> d_lines;
  DevBuf<uint32_t> d_keys[2], d_vals[2], d_hist;
  DevBuf<int8_t> d_out;
  std::vector<double> h_poses;

  size_t cells() const { return (size_t)c.n_cells; }
  int* visits() const { return (int*)d_planes; }
  int* hits() const { return (int*)d_planes + cells(); }
  float* ax() const { return (float*)d_planes + 2 * cells(); }
  float* ay() const { return (float*)d_planes + 3 * cells(); }
  uint8_t* mask() const { return (uint8_t*)((float*)d_planes + 4 * cells()); }
  int n_patches() const { return c.patches_x * patches_y; }

  void release() {
    if (d_planes) (void)hipFree(d_planes);
    if (d_stats) (void)hipFree(d_stats);
    d_planes = nullptr;
    d_stats = nullptr;
    d_cs.release(); d_poses.release(); d_ranges.release(); d_hx.release(); d_hy.release(); d_lines.release();
    for (int i = 0; i < 2; i++) { d_keys[i].release(); d_vals[i].release(); }
    d_hist.release(); d_out.release();
  }

  // a refused launch leaves nothing on the stream, so a synchronise alone would not see it: clear the thread's last error
  // before the launches, read it after them
  int launch_error(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LSLAM_OK : ctx->fail(LSLAM_ERR_HIP, "%s: kernel launch failed: %s", what, hipGetErrorString(e));
  }

  int enqueue_reset() {
    (void)hipGetLastError();
    launch(ctx, "gm_reset", k_gm_reset, dim3(n_patches()), dim3(256), 0, c.size_x, c.patches_x, mask(), visits(), hits(), ax(),
           ay());
    return launch_error("lslam_gmap_reset");
  }

  // the batch's ranges are in d_ranges, its poses (x, y, cos, sin) in d_poses or absent
  int enqueue_integrate(int n_scans, bool with_poses) {
    const int n = n_scans * c.n_beams;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
      e = d_keys[i].reserve(n);
      if (e == hipSuccess) e = d_vals[i].reserve(n);
    }
    const int n_tiles = (n + kSortTile - 1) / kSortTile;
    if (e == hipSuccess) e = d_lines.reserve(n);
    if (e == hipSuccess) e = d_hx.reserve(n);
    if (e == hipSuccess) e = d_hy.reserve(n);
    if (e == hipSuccess) e = d_hist.reserve((size_t)256 * n_tiles);
    if (e != hipSuccess) return ctx->fail(LSLAM_ERR_HIP, "lslam_gmap_integrate: out of device memory");
    const int blocks = (n + 255) / 256;
    (void)hipGetLastError();
    launch(ctx, "gm_endpoint", k_gm_endpoint, dim3(blocks), dim3(256), 0, c, n, (const float*)d_ranges.p,
           (const double*)(with_poses ? d_poses.p : nullptr), (const double*)d_cs.p, d_lines.p, d_keys[0].p, d_vals[0].p, d_hx.p,
           d_hy.p, mask(), d_stats);
    launch(ctx, "gm_trace", k_gm_trace, dim3(std::min((n + 3) / 4, kTraceBlocks)), dim3(256), 0, c, n, (const int4*)d_lines.p, visits(), mask(),
           d_stats);
    // the sort needs the bits of n_cells (the no-hit key sorts last)
    int bits = 0;
    while (bits < 32 && (c.n_cells >> bits) != 0u) bits++;
    int cur = 0;
    for (int shift = 0; shift < bits; shift += 8) {
      launch(ctx, "gm_hist", k_gm_hist, dim3(n_tiles), dim3(256), 0, (const uint32_t*)d_keys[cur].p, n, shift, n_tiles,
             d_hist.p);
      launch(ctx, "gm_scan", k_gm_scan, dim3(1), dim3(1024), 0, d_hist.p, 256 * n_tiles);
      launch(ctx, "gm_scatter", k_gm_scatter, dim3(n_tiles), dim3(256), 0, (const uint32_t*)d_keys[cur].p,
             (const uint32_t*)d_vals[cur].p, d_keys[cur ^ 1].p, d_vals[cur ^ 1].p, n, shift, n_tiles, (const uint32_t*)d_hist.p);
      cur ^= 1;
    }
    launch(ctx, "gm_fold", k_gm_fold, dim3(blocks), dim3(256), 0, n, c.n_cells, (const uint32_t*)d_keys[cur].p,
           (const uint32_t*)d_vals[cur].p, (const float*)d_hx.p, (const float*)d_hy.p, visits(), hits(), ax(), ay());
    const int rc = launch_error("lslam_gmap_integrate");
    if (rc == LSLAM_OK) scans += n_scans;
    return rc;
  }

  int upload_scans(int n_scans, const float* ranges, const double* poses) {
    const size_t n = (size_t)n_scans * c.n_beams;
    LSLAM_HIP(ctx, d_ranges.reserve(n));
    LSLAM_HIP(ctx, hipMemcpyAsync(d_ranges.p, ranges, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (poses) {
      h_poses.resize(4 * (size_t)n_scans);
      for (int s = 0; s < n_scans; s++) {  // cos / sin of the heading from the host libm's sincos, like the angle cache
        h_poses[4 * s] = poses[3 * s];
        h_poses[4 * s + 1] = poses[3 * s + 1];
        ::sincos(poses[3 * s + 2], &h_poses[4 * s + 3], &h_poses[4 * s + 2]);
      }
      LSLAM_HIP(ctx, d_poses.reserve(h_poses.size()));
      // the pageable copy is staged before the call returns, so h_poses may be reused by the next call
      LSLAM_HIP(ctx, hipMemcpyAsync(d_poses.p, h_poses.data(), h_poses.size() * sizeof(double), hipMemcpyHostToDevice,
                                    ctx->stream));
    }
    return LSLAM_OK;
  }

  int finish(const char* what) {
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ctx->fail(LSLAM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    d_ranges.trim(); d_poses.trim(); d_hx.trim(); d_hy.trim(); d_lines.trim(); d_hist.trim(); d_out.trim();
    for (int i = 0; i < 2; i++) { d_keys[i].trim(); d_vals[i].trim(); }
    return LSLAM_OK;
  }
};

namespace {

int check_scans(lslam_gmap* m, int n_scans, const float* ranges, const double* poses, const char* what) {
  if (!m->have_laser) return m->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: no laser set (lslam_gmap_set_laser)", what);
  if (n_scans < 0 || (n_scans > 0 && !ranges)) return m->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: bad scans", what);
  if ((long long)n_scans * m->c.n_beams > kMaxReadings)
    return m->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: more than 2^28 readings in one call", what);
  for (int s = 0; poses && s < n_scans; s++) {
    const double* p = poses + 3 * (size_t)s;
    if (!std::isfinite(p[2]) || !(std::fabs((p[0] - m->c.cx) / m->c.delta) < kMaxCellCoord) ||
        !(std::fabs((p[1] - m->c.cy) / m->c.delta) < kMaxCellCoord))
      return m->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: pose %d is not finite or too far from the map", what, s);
  }
  return LSLAM_OK;
}

}  // namespace

extern "C" {

int lslam_gmap_create(lslam_context* ctx, double xmin, double ymin, double xmax, double ymax, double delta, lslam_gmap** out) {
  if (!ctx || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!(delta > 0.0) || !std::isfinite(delta) || !std::isfinite(xmin) || !std::isfinite(ymin) || !std::isfinite(xmax) ||
      !std::isfinite(ymax) || !(xmax > xmin) || !(ymax > ymin))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_gmap_create: need delta > 0 and xmax > xmin, ymax > ymin");
  const double wx = (xmax - xmin) / delta, wy = (ymax - ymin) / delta;
  if (!(wx >= 32.0) || !(wy >= 32.0))  // < 32 cells on an axis: HierarchicalArray2D has no patch (harray2d.h:75-80)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_gmap_create: fewer than 32 cells on an axis");
  if (wx > kMaxAxisCells || wy > kMaxAxisCells)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_gmap_create: more than 65504 cells on an axis");
  auto* m = new lslam_gmap();
  m->ctx = ctx;
  m->xmin = xmin; m->ymin = ymin; m->xmax = xmax; m->ymax = ymax;
  // Map(center, xmin, ymin, xmax, ymax, delta) (map.h:133-143) with the node's center (gmapping.cc:130-135)
  const int sx_cells = (int)std::ceil(wx), sy_cells = (int)std::ceil(wy);
  m->c.patches_x = sx_cells >> kPatchMag;
  m->patches_y = sy_cells >> kPatchMag;
  m->c.size_x = m->c.patches_x << kPatchMag;
  m->size_y = m->c.size_y = m->patches_y << kPatchMag;
  m->c.cx = (xmin + xmax) / 2.0;
  m->c.cy = (ymin + ymax) / 2.0;
  m->c.delta = delta;
  m->c.sizeX2 = (int)std::round((m->c.cx - xmin) / delta);
  m->c.sizeY2 = (int)std::round((m->c.cy - ymin) / delta);
  m->c.n_cells = (unsigned)m->c.size_x * (unsigned)m->c.size_y;
  // the published grid (gmapping.cc:72-73): info.width = (uint32)((xmax - xmin) / delta)
  m->width = (int)wx;
  m->height = (int)wy;
  if (m->width < m->c.size_x || m->height < m->c.size_y) {
    delete m;  // the node would index data[width * y + x] past its rows and past its end
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_gmap_create: published grid %.0f x %.0f is narrower than the %d x %d storage",
                     std::floor(wx), std::floor(wy), sx_cells >> kPatchMag << kPatchMag, sy_cells >> kPatchMag << kPatchMag);
  }
  hipError_t e = hipSetDevice(ctx->device);
  const size_t bytes = 4 * m->cells() * sizeof(float) + (size_t)m->n_patches();
  if (e == hipSuccess) e = hipMalloc(&m->d_planes, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&m->d_stats, 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemsetAsync(m->d_planes, 0, bytes, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(m->d_stats, 0, 4 * sizeof(unsigned long long), ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    m->release();
    delete m;
    return ctx->fail(LSLAM_ERR_HIP, "lslam_gmap_create: %s", hipGetErrorString(e));
  }
  *out = m;
  return LSLAM_OK;
}

void lslam_gmap_destroy(lslam_gmap* map) {
  if (!map) return;
  (void)hipSetDevice(map->ctx->device);
  (void)hipStreamSynchronize(map->ctx->stream);
  map->release();
  delete map;
}

int lslam_gmap_info(const lslam_gmap* map, lslam_gmap_geometry* out) {
  if (!map || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out->map_size_x = map->c.size_x;
  out->map_size_y = map->c.size_y;
  out->width = map->width;
  out->height = map->height;
  out->size_x2 = map->c.sizeX2;
  out->size_y2 = map->c.sizeY2;
  out->patches_x = map->c.patches_x;
  out->patches_y = map->patches_y;
  out->center_x = map->c.cx;
  out->center_y = map->c.cy;
  out->delta = map->c.delta;
  return LSLAM_OK;
}

int lslam_gmap_set_laser(lslam_gmap* map, int n_beams, float angle_min, float angle_increment, double max_range,
                         double max_use_range) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  if (n_beams < 1 || !(max_range > 0.0) || !(max_use_range > 0.0) || !std::isfinite(angle_min) ||
      !std::isfinite(angle_increment))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_gmap_set_laser: need n_beams >= 1, max_range > 0, max_use_range > 0");
  if (!(std::fmin(max_range, max_use_range) / map->c.delta <= (double)kMaxLineCells))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_gmap_set_laser: lines longer than %d cells", kMaxLineCells);
  // CreateCache (gmapping.cc:112-124): angle = angle_min + i * angle_increment on the message's float32 fields with an
  // unsigned i, i.e. evaluated in float; cos / sin in double from the host libm.  The node's loop takes cos and sin of the
  // same angle, which g++ -O2 turns into ONE sincos call, and glibc's sincos can differ from its cos in the last bit: the
  // library calls sincos itself rather than leave it to the compiler
  std::vector<double> cs(2 * (size_t)n_beams);
  for (unsigned i = 0; i < (unsigned)n_beams; i++) {
    const float af = angle_min + (float)i * angle_increment;
    ::sincos((double)af, &cs[n_beams + i], &cs[i]);
  }
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a running integrate may still read the old cache
  map->d_cs.trim();
  LSLAM_HIP(ctx, map->d_cs.reserve(cs.size()));
  LSLAM_HIP(ctx, hipMemcpy(map->d_cs.p, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice));
  map->c.n_beams = n_beams;
  map->c.max_range = max_range;
  map->c.max_use_range = max_use_range;
  map->have_laser = true;
  return LSLAM_OK;
}

int lslam_gmap_angle_cache(const lslam_gmap* map, double* cos_out, double* sin_out) {
  if (!map || !map->have_laser || !cos_out || !sin_out) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  const size_t nb = (size_t)map->c.n_beams;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LSLAM_HIP(ctx, hipMemcpy(cos_out, map->d_cs.p, nb * sizeof(double), hipMemcpyDeviceToHost));
  LSLAM_HIP(ctx, hipMemcpy(sin_out, map->d_cs.p + nb, nb * sizeof(double), hipMemcpyDeviceToHost));
  return LSLAM_OK;
}

int lslam_gmap_reset(lslam_gmap* map) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = map->enqueue_reset();
  if (rc != LSLAM_OK) {
    (void)map->finish("lslam_gmap_reset");
    return rc;
  }
  LSLAM_HIP(ctx, hipMemsetAsync(map->d_stats, 0, 4 * sizeof(unsigned long long), ctx->stream));
  map->scans = 0;
  return map->finish("lslam_gmap_reset");
}

int lslam_gmap_integrate(lslam_gmap* map, int n_scans, const float* ranges, const double* poses) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  int rc = check_scans(map, n_scans, ranges, poses, "lslam_gmap_integrate");
  if (rc != LSLAM_OK) return rc;
  if (n_scans == 0) return LSLAM_OK;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = map->upload_scans(n_scans, ranges, poses);
  if (rc == LSLAM_OK) rc = map->enqueue_integrate(n_scans, poses != nullptr);
  const int rs = map->finish("lslam_gmap_integrate");
  return rc != LSLAM_OK ? rc : rs;
}

int lslam_gmap_read_ros_i8(lslam_gmap* map, double occ_thresh, int8_t* out) {
  if (!map || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  const size_t n = (size_t)map->width * map->height;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, map->d_out.reserve(n));
  (void)hipGetLastError();
  launch(ctx, "gm_classify", k_gm_classify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, map->c.size_x, map->c.size_y,
         map->width, map->height, occ_thresh, (const int*)map->visits(), (const int*)map->hits(), map->d_out.p);
  const int rc = map->launch_error("lslam_gmap_read_ros_i8");
  if (rc != LSLAM_OK) {
    (void)map->finish("lslam_gmap_read_ros_i8");
    return rc;
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(out, map->d_out.p, n, hipMemcpyDeviceToHost, ctx->stream));
  return map->finish("lslam_gmap_read_ros_i8");
}

int lslam_gmap_compute_map(lslam_gmap* map, const float* ranges, double occ_thresh, int8_t* out) {
  if (!map || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  int rc = check_scans(map, 1, ranges, nullptr, "lslam_gmap_compute_map");
  if (rc != LSLAM_OK) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = map->enqueue_reset();
  if (rc != LSLAM_OK) {
    (void)map->finish("lslam_gmap_compute_map");
    return rc;
  }
  LSLAM_HIP(ctx, hipMemsetAsync(map->d_stats, 0, 4 * sizeof(unsigned long long), ctx->stream));
  map->scans = 0;
  rc = map->upload_scans(1, ranges, nullptr);
  if (rc == LSLAM_OK) rc = map->enqueue_integrate(1, false);
  if (rc != LSLAM_OK) {
    (void)map->finish("lslam_gmap_compute_map");
    return rc;
  }
  return lslam_gmap_read_ros_i8(map, occ_thresh, out);
}

int lslam_gmap_read_counters(lslam_gmap* map, int32_t* visits, int32_t* n, float* acc_xy) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  const size_t cells = map->cells();
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  if (visits) LSLAM_HIP(ctx, hipMemcpyAsync(visits, map->visits(), cells * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (n) LSLAM_HIP(ctx, hipMemcpyAsync(n, map->hits(), cells * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (acc_xy) LSLAM_HIP(ctx, hipMemcpyAsync(acc_xy, map->ax(), 2 * cells * 4, hipMemcpyDeviceToHost, ctx->stream));
  return map->finish("lslam_gmap_read_counters");
}

int lslam_gmap_read_patch_mask(lslam_gmap* map, uint8_t* out) {
  if (!map || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hipMemcpyAsync(out, map->mask(), (size_t)map->n_patches(), hipMemcpyDeviceToHost, ctx->stream));
  return map->finish("lslam_gmap_read_patch_mask");
}

int lslam_gmap_stats(lslam_gmap* map, int64_t out[4]) {
  if (!map || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  unsigned long long s[4] = {0, 0, 0, 0};
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hipMemcpyAsync(s, map->d_stats, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  const int rc = map->finish("lslam_gmap_stats");
  if (rc != LSLAM_OK) return rc;
  out[0] = map->scans;
  out[1] = (int64_t)s[0];
  out[2] = (int64_t)s[1];
  out[3] = (int64_t)s[2];
  return LSLAM_OK;
}

}  // extern "C"
