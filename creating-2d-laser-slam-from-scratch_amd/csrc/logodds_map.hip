// Hector-style Bresenham ray-casting log-odds occupancy grid update on MI355X (gfx950).
//
// Reference behaviour reproduced (never copied): hectorslam::OccGridMapBase::updateByScan and
// friends (lesson4/include/lesson4/hector_mapping/map/OccGridMapBase.h:118-330), LogOddsCell /
// GridMapLogOddsFunctions (.../map/GridMapLogOdds.h:37-161), GridMapBase::setMapTransformation
// (.../map/GridMapBase.h:270-286), MapRepMultiMap pyramid (.../slam_main/MapRepMultiMap.h:57-93,
// 174-191).  H/ below = lesson4/include/lesson4/hector_mapping/.
//
// The reference walks the beams one after another and uses a per-cell updateIndex so that, per
// scan, every traversed cell gets logOddsFree ONCE and every hit cell gets logOddsOccupied ONCE,
// un-doing a free mark made earlier in the same scan (H/map/OccGridMapBase.h:302-330).  The only
// order-dependent bit is whether (v + free) - free is applied to a hit cell, i.e. whether some
// beam with a smaller index crossed the cell before the first beam that ends in it.
// Device formulation (one WAVE per beam, closed-form Bresenham cells, two kernels, no atomics on
// the float plane):
//   k_logodds_mark   walks the Bresenham line; atomicMax(free_key[cell]) along the ray and
//                    atomicMax(occ_key[end]) where key = epoch<<16 | (65535-beam): for the current
//                    epoch the max key is the SMALLEST beam index that touched the cell.
//   k_logodds_apply  walks again; the owner of a cell (min beam ending in it, else min beam crossing
//                    it) applies exactly the float operations the sequential reference applies.
// HBM-bound integer/byte work: coalescing comes from neighbouring beams crossing neighbouring
// cells; nothing here is GEMM-shaped.
#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "deskew_impl.hpp"  // msync_context, msync_check_scans, msync_stream_drained

using namespace lslam;

namespace {

constexpr int kBeamBits = 16;  // 65536 points per container; the epoch keeps 16 bits (marks cleared every 65535 scans)
constexpr int kMaxBeams = 1 << kBeamBits;
constexpr uint32_t kBeamMask = kMaxBeams - 1;
constexpr uint32_t kMaxEpoch = (1u << (32 - kBeamBits)) - 1;

struct LevelGeom {
  int sx, sy;
  float c, s, tx, ty;      // pose transform: Translation(tx,ty) * Rotation (H/map/OccGridMapBase.h:127-129)
  float factor;            // DataPointContainer::setFrom factor of this level
  float ox, oy;            // origo (level-0 units)
  float lo_free, lo_occ;
  uint32_t epoch;
  int just_once;           // updateByScanJustOnce end-point rule
  int bx, by;              // begin cell
  double metres_per_cell;
};

struct Line {
  int x0, y0, x1, y1;
  bool valid;
};

// end cell of beam i and the in-map test of updateLineBresenhami (H/map/OccGridMapBase.h:143-161,
// 220-238)
__device__ __forceinline__ Line beam_line(const LevelGeom& g, const float* __restrict__ pts, int i) {
  Line l;
  l.x0 = g.bx; l.y0 = g.by;
  bool representable;
  float px = pts[2 * i], py = pts[2 * i + 1];
  if (g.just_once) {
    // scanBeginMapi + (int)round(p / 0.05) with p in metres (:202-203); float / double -> double
    const double rx = round((double)px / g.metres_per_cell), ry = round((double)py / g.metres_per_cell);
    // x86 cvttsd2si yields INT_MIN for NaN / Inf / out-of-range and the in-map test then drops the beam; the
    // gfx950 conversion saturates instead (NaN -> 0), so reject those end points explicitly
    representable = fabs(rx) < 2147483648.0 && fabs(ry) < 2147483648.0;
    l.x1 = g.bx + (int)rx;
    l.y1 = g.by + (int)ry;
  } else {
    px = px * g.factor;  // setFrom (H/scan/DataPointContainer.h:54-57); factor 1 on level 0 is exact
    py = py * g.factor;
    float ex = (g.c * px + (-g.s) * py) + g.tx;
    float ey = (g.s * px + g.c * py) + g.ty;
    ex += 0.5f;
    ey += 0.5f;
    representable = fabsf(ex) < 2147483648.0f && fabsf(ey) < 2147483648.0f;  // false for NaN / Inf too
    l.x1 = (int)ex;
    l.y1 = (int)ey;
  }
  l.valid = representable && !(l.x0 == l.x1 && l.y0 == l.y1) && l.x0 >= 0 && l.x0 < g.sx && l.y0 >= 0 && l.y0 < g.sy &&
            l.x1 >= 0 && l.x1 < g.sx && l.y1 >= 0 && l.y1 < g.sy;
  return l;
}

// Bresenham traversal of H/map/OccGridMapBase.h:240-299 in CLOSED FORM.  The reference loop adds
// abs_db to an error term that starts at abs_da/2 and takes a minor-axis step whenever it reaches
// abs_da; since abs_db <= abs_da that is at most one minor step per major step, so after i major
// steps exactly q(i) = floor((abs_da/2 + i*abs_db) / abs_da) minor steps were taken.  Cell i of the
// ray (i = 0 .. abs_da-1, end point excluded) is therefore start + i*offset_a + q(i)*offset_b --
// independent of the other cells, so a whole wave walks ONE ray, 64 cells at a time, instead of one
// thread crawling it cell by cell with a dependent atomic per step.
struct Ray {
  unsigned start, abs_da, abs_db;
  int offset_a, offset_b;
};
__device__ __forceinline__ Ray ray_of(const Line& l, int sx) {
  int dx = l.x1 - l.x0, dy = l.y1 - l.y0;
  unsigned abs_dx = (unsigned)abs(dx), abs_dy = (unsigned)abs(dy);
  int offset_dx = dx > 0 ? 1 : -1;  // util::sign: sign(0) = -1
  int offset_dy = (dy > 0 ? 1 : -1) * sx;
  Ray r;
  r.start = (unsigned)(l.y0 * sx + l.x0);
  if (abs_dx >= abs_dy) {
    r.abs_da = abs_dx; r.abs_db = abs_dy; r.offset_a = offset_dx; r.offset_b = offset_dy;
  } else {
    r.abs_da = abs_dy; r.abs_db = abs_dx; r.offset_a = offset_dy; r.offset_b = offset_dx;
  }
  return r;
}
__device__ __forceinline__ unsigned ray_minor(const Ray& r, unsigned i) {  // minor-axis steps taken after i major steps
  return (unsigned)(((unsigned long long)(r.abs_da / 2) + (unsigned long long)i * r.abs_db) / r.abs_da);
}
__device__ __forceinline__ unsigned ray_cell(const Ray& r, unsigned i) {
  return r.start + (unsigned)((int)i * r.offset_a) + (unsigned)((int)ray_minor(r, i) * r.offset_b);
}

// "does the traversal of beam P (same origin) visit the cell at signed offset (ox, oy) from the origin?"  The visited
// cells of a ray are exactly { A major steps, q_P(A) minor steps : 0 <= A < abs_da } (end point excluded), so membership
// is one closed-form test.  Used by the mark pass: a beam whose PREDECESSOR also crosses a cell cannot be the smallest
// beam index crossing it, so its atomicMax on that cell cannot change the result and is skipped.  Near the sensor every
// cell is crossed by hundreds of beams; without this the same-address atomics of those cells serialise in L2 and set the
// duration of the whole pass.
struct RayShape {
  unsigned abs_da, abs_db;
  int sgn_x, sgn_y;  // util::sign: sign(0) = -1
  bool x_major, valid;
};
__device__ __forceinline__ RayShape shape_of(const Line& l) {
  RayShape p;
  const int dx = l.x1 - l.x0, dy = l.y1 - l.y0;
  const unsigned adx = (unsigned)abs(dx), ady = (unsigned)abs(dy);
  p.sgn_x = dx > 0 ? 1 : -1;
  p.sgn_y = dy > 0 ? 1 : -1;
  p.x_major = adx >= ady;
  p.abs_da = p.x_major ? adx : ady;
  p.abs_db = p.x_major ? ady : adx;
  p.valid = l.valid;
  return p;
}
__device__ __forceinline__ bool ray_visits(const RayShape& p, int ox, int oy) {
  const int A = p.x_major ? ox * p.sgn_x : oy * p.sgn_y;
  const int M = p.x_major ? oy * p.sgn_y : ox * p.sgn_x;
  if (A < 0 || (unsigned)A >= p.abs_da || M < 0) return false;
  // A < abs_da <= 2^16 on any map this library allocates, so the product stays below 2^32
  return (unsigned)M == (p.abs_da / 2u + (unsigned)A * p.abs_db) / p.abs_da;
}

// one wave per beam; `wave` = index of this wave among the kernel's mark (resp. apply) waves
__device__ __forceinline__ void logodds_mark_wave(const LevelGeom& g, const float* __restrict__ pts, int n, int wave, int lane,
                                                  uint32_t* __restrict__ free_key, uint32_t* __restrict__ occ_key,
                                                  float* __restrict__ pts_copy) {
  const int i = wave;
  if (i >= n) return;
  if (pts_copy && lane < 2) pts_copy[2 * i + lane] = pts[2 * i + lane];  // kept for the deferred apply (pipelined path)
  Line l = beam_line(g, pts, i);
  if (!l.valid) return;
  const uint32_t key = (g.epoch << kBeamBits) | (kBeamMask - (uint32_t)i);
  const Ray r = ray_of(l, g.sx);
  const RayShape me = shape_of(l);
  RayShape prev;
  prev.valid = false;
  if (i > 0 && me.abs_da < 65536u) prev = shape_of(beam_line(g, pts, i - 1));
  prev.valid = prev.valid && prev.abs_da < 65536u;
  for (unsigned c = lane; c < r.abs_da; c += 64) {
    const unsigned q = ray_minor(r, c);
    if (prev.valid) {
      const int ox = me.x_major ? (int)c * me.sgn_x : (int)q * me.sgn_x;
      const int oy = me.x_major ? (int)q * me.sgn_y : (int)c * me.sgn_y;
      if (ray_visits(prev, ox, oy)) continue;  // beam i-1 marks this cell with a larger key
    }
    atomicMax(&free_key[r.start + (unsigned)((int)c * r.offset_a) + (unsigned)((int)q * r.offset_b)], key);
  }
  if (lane == 0) atomicMax(&occ_key[(unsigned)(l.y1 * g.sx + l.x1)], key);
}

__device__ __forceinline__ void logodds_apply_wave(const LevelGeom& g, const float* __restrict__ pts, int n, int wave, int lane,
                                                   const uint32_t* __restrict__ free_key, const uint32_t* __restrict__ occ_key,
                                                   float* __restrict__ logodds) {
  const int i = wave;
  if (i >= n) return;
  Line l = beam_line(g, pts, i);
  if (!l.valid) return;
  const uint32_t me = kBeamMask - (uint32_t)i;
  const uint32_t ep = g.epoch;
  const Ray r = ray_of(l, g.sx);
  // crossed cells: free once per scan unless some beam ends here (bresenhamCellFree, :302-313).
  // Four cells per lane and pass, their three reads issued together: the kernel is a chain of dependent
  // L2 round trips, not bandwidth, so the reads of non-owners are the cheaper evil.
  constexpr int kIlp = 4;
  for (unsigned c0 = lane; c0 < r.abs_da; c0 += 64 * kIlp) {
    unsigned off[kIlp];
    uint32_t fk[kIlp], ok[kIlp];
    float lo[kIlp];
#pragma unroll
    for (int u = 0; u < kIlp; u++) {
      const unsigned c = c0 + 64u * u;
      off[u] = ray_cell(r, c < r.abs_da ? c : c0);
    }
#pragma unroll
    for (int u = 0; u < kIlp; u++) {
      fk[u] = free_key[off[u]];
      ok[u] = occ_key[off[u]];
      lo[u] = logodds[off[u]];
    }
#pragma unroll
    for (int u = 0; u < kIlp; u++) {
      if (c0 + 64u * u >= r.abs_da) continue;
      if ((fk[u] & kBeamMask) != me) continue;       // not the first beam crossing this cell
      if ((ok[u] >> kBeamBits) == ep) continue;      // a hit cell: handled by its occ owner
      logodds[off[u]] = lo[u] + g.lo_free;           // the owner is the only writer of this cell in this kernel
    }
  }
  // end cell (bresenhamCellOcc, :316-330)
  if (lane == 0) {
    unsigned eoff = (unsigned)(l.y1 * g.sx + l.x1);
    uint32_t ok = occ_key[eoff];
    if ((ok & kBeamMask) == me) {  // first beam ending here
      float v = logodds[eoff];
      uint32_t fk = free_key[eoff];
      if ((fk >> kBeamBits) == ep && (fk & kBeamMask) > me) {  // crossed by an EARLIER beam: free then unset
        v += g.lo_free;
        v -= g.lo_free;
      }
      if (v < 50.0f) v += g.lo_occ;  // updateSetOccupied (H/map/GridMapLogOdds.h:108-114)
      logodds[eoff] = v;
    }
  }
}

__global__ void __launch_bounds__(256)
k_logodds_mark(LevelGeom g, const float* __restrict__ pts, int n, uint32_t* __restrict__ free_key,
               uint32_t* __restrict__ occ_key) {
  logodds_mark_wave(g, pts, n, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), threadIdx.x & 63, free_key, occ_key, nullptr);
}

__global__ void __launch_bounds__(256)
k_logodds_apply(LevelGeom g, const float* __restrict__ pts, int n, const uint32_t* __restrict__ free_key,
                const uint32_t* __restrict__ occ_key, float* __restrict__ logodds) {
  logodds_apply_wave(g, pts, n, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), threadIdx.x & 63, free_key, occ_key, logodds);
}

// PIPELINED single-scan update: ONE launch per scan in steady state.  The two kernels above are two dependent ~10 us
// launches whose only link is "apply needs every mark of its scan".  But the apply of scan t-1 and the mark of scan t are
// independent once the two scans keep their keys in different planes: the mark of scan t goes into key-plane set t & 1,
// while the apply of scan t-1 reads set (t-1) & 1 and is the launch's only writer of the float plane.  So each call
// launches [apply blocks of the previous scan | mark blocks of this scan] together and leaves this scan's apply pending;
// a reader (lslam_map_read_*, matchData, a batched update, lslam_synchronize, ...) first flushes the pending apply with the
// stand-alone kernel.  Per cell the float operations and their order are exactly those of the sequential reference:
// apply(t-1) completes in the launch before apply(t) starts (stream order).  The mark blocks also copy their points
// aside (the caller's buffer may be reused before the deferred apply runs).
// As ONE launch for EVERY pyramid level (round 4; a kernel per level until then): a 3-level MapRepMultiMap update was three pipe launches (and,
// when a reader follows every scan -- matchData in lesson4's loop -- three more stand-alone applies), each a ~8 us
// dependent step of a latency-bound chain.  A job = the apply of a level's pending scan or the mark of its new one; the
// blocks of all jobs share the grid, a block finds its job by its index (a uniform select chain over the kernel
// arguments: no dynamic indexing, no table in memory to keep alive behind an asynchronous call).  Within a level the
// invariants of k_logodds_pipe hold unchanged; levels are independent planes.
struct PipeJob {
  LevelGeom g;
  const float* pts;
  int n, first_block, apply;
  const uint32_t* free_r;
  const uint32_t* occ_r;
  uint32_t* free_w;
  uint32_t* occ_w;
  float* logodds;
  float* pts_copy;
};
constexpr int kPipeMaxJobs = 12;
struct PipeJobs {
  int n_jobs;
  PipeJob j[kPipeMaxJobs];
};
__global__ void __launch_bounds__(256)
k_logodds_pipe_ml(PipeJobs J) {
  const int b = (int)blockIdx.x;
  PipeJob cur = J.j[0];
#pragma unroll
  for (int k = 1; k < kPipeMaxJobs; k++)
    if (k < J.n_jobs && b >= J.j[k].first_block) cur = J.j[k];
  // Workgroups go to the eight XCDs round robin (block b -> XCD b % 8) and every XCD has its OWN L2: with beams dealt
  // out in block order, each XCD walked every eighth group of four beams -- all eight of them touched nearly every cell of
  // the scan's fan and fetched its lines separately (measured 4.3x the algorithmic bytes at 1000^2, 5.8x at 4000^2).  A
  // job's blocks are a multiple of 8 and start at a multiple of 8, so block (r, q) = (lb % 8, lb / 8) runs on XCD r:
  // XCD r takes the r-th CONTIGUOUS eighth of the beams -- one 34-degree sector of the fan per L2.
  const int lb = b - cur.first_block, per_xcd = ((cur.n + 3) / 4 + 7) / 8;
  const int lane = threadIdx.x & 63, wave = ((lb & 7) * per_xcd + (lb >> 3)) * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
  if (cur.apply)
    logodds_apply_wave(cur.g, cur.pts, cur.n, wave, lane, cur.free_r, cur.occ_r, cur.logodds);
  else
    logodds_mark_wave(cur.g, cur.pts, cur.n, wave, lane, cur.free_w, cur.occ_w, cur.pts_copy);
}

// ------------------------------------------------------------------------------------------
// BATCHED update: K scans, each with its own pose, applied to the map exactly as K successive
// updateByScan calls would (the float operations of a cell are applied in scan order; cells are
// independent of each other).  The single-scan path above is bound by two dependent ~10 us kernels
// per scan; here the K scans are MARKED in parallel and APPLIED by one pass over the touched tiles:
//   k_lo_batch_hits    thread per (scan, beam): end cell -> byte plane[s][cell] = HIT, and the cell is
//                      entered in scan s's small hash with atomicMin(first beam ending there);
//   k_lo_batch_rays    wave per (scan, beam), closed-form Bresenham cells: a crossed cell whose byte is not
//                      HIT gets plane[s][cell] = CROSSED (plain byte store, every writer writes the same
//                      value); a crossed HIT cell records atomicMin(first beam crossing it) in the hash;
//   k_lo_batch_resolve thread per hash entry: a hit cell crossed by an earlier beam of its scan -> byte HIT_UNDO;
//   k_lo_batch_apply   wave per 8x8-cell tile: reads the tile's 64 "touched by scan s" flags in one load, then
//                      walks ONLY the planes that touched the tile, in scan order, and applies
//                      +free / [(v+free)-free] +occ-if-<50, the float sequence of the sequential reference
//                      (H/map/OccGridMapBase.h:302-330).
// Layout: the byte planes are TILED and WINDOWED.  A tile is 8x8 cells = one 64-byte line, so 64 consecutive cells of a
// ray lie in ~8 lines whichever way the ray runs (instead of 1 line for an x-major and 64 for a y-major ray in a
// row-major plane).  Scan s does not own a plane of the whole map but a WINDOW of tiles -- the square of tiles its rays
// can reach from its begin cell (host: begin cell +- the scan's longest point, ScanHdr::tx0 / ty0 / tw / th) -- stored
// densely in a slot pool: cell (x, y) of scan s is byte
//     pool[(base_s + (y>>3 - ty0_s) * tw_s + (x>>3 - tx0_s)) * 64 + (y&7)*8 + (x&7)].
// A 1081-beam scan with 20 m of range on a 0.025 m map owns 202 x 202 tiles = 2.6 MB whatever the size of the map (a
// plane of a 4000 x 4000 map is 16 MB, of an 8000 x 8000 map 64 MB); a window clipped by a small map IS the plane.
// The scans of a call are cut into ROUNDS whose windows fit the scratch budget (LSLAM_MAP_OPT_BATCH_SCRATCH_MB,
// default 192 MB): normally one.  flags[tile][s] (64 bytes per tile) is what lets the apply pass skip the ~90 % of
// (tile, scan) pairs no ray went through.  Pool and flag bytes carry a 6-bit round epoch, so they are cleared once per
// 63 rounds, not per batch.  HBM-bound byte work; no atomics on the traversal path.
// ------------------------------------------------------------------------------------------
struct ScanHdr {     // one scan of a batch on one pyramid level (host-computed like LevelGeom)
  float c, s, tx, ty;
  int bx, by;        // begin cell
  int n, pts_off;    // points of this scan: pts[2*(pts_off + i)]
  // the scan's window of tiles (clipped to the map; tw = 0: nothing of it is inside) and its first tile slot in the pool:
  // one aligned 16-byte record at offset 32, which k_lo_batch_apply reads with one vector load (lane = scan)
  int tx0, ty0, tw;
  uint32_t base;     // < 2^26: byte offsets into the pool stay below 2^32
  int th, pad[3];
};
static_assert(sizeof(ScanHdr) == 64, "ScanHdr: 64 bytes, window record at offset 32");
struct BatchGeom {
  int sx, sy, K;
  int tiles_x, n_tiles;
  float factor, lo_free, lo_occ;
  uint32_t tag;      // epoch << 2
  uint32_t hash_mask;  // slots per scan - 1 (power of two >= 2 * max points per scan)
};
constexpr uint32_t kCodeCrossed = 1u, kCodeHit = 2u, kCodeHitUndo = 3u;
constexpr uint32_t kHashEmpty = 0xFFFFFFFFu;
constexpr int kBatchSlots = 64;  // scans per batch = flag bytes per tile
#if !defined(LSLAM_TUNE_APPLY_CHUNK)
#define LSLAM_TUNE_APPLY_CHUNK 8
#endif
constexpr int kApplyChunk = LSLAM_TUNE_APPLY_CHUNK;  // planes whose bytes k_lo_batch_apply has in flight at a time (A/B, round 6:
                                                     // 8 / 16 / 32 / 64 -> 0.271 / 0.261 / 0.292 / 0.327 ms per 1000 scans: the tiles every
                                                     // scan touches are NOT what the launch waits for; the unrolled slot bookkeeping is)

__device__ __forceinline__ Line batch_line(const BatchGeom& g, const ScanHdr& h, const float* __restrict__ pts, int i) {
  LevelGeom lg;
  lg.sx = g.sx; lg.sy = g.sy; lg.c = h.c; lg.s = h.s; lg.tx = h.tx; lg.ty = h.ty; lg.factor = g.factor;
  lg.just_once = 0; lg.bx = h.bx; lg.by = h.by; lg.metres_per_cell = 0.0;
  return beam_line(lg, pts + 2 * (size_t)h.pts_off, i);
}
__device__ __forceinline__ uint32_t hash_slot0(uint32_t cell, uint32_t mask) { return (cell * 2654435761u) >> 7 & mask; }
__device__ __forceinline__ uint32_t tile_of(const BatchGeom& g, int x, int y) { return (uint32_t)((y >> 3) * g.tiles_x + (x >> 3)); }
__device__ __forceinline__ uint32_t in_tile(int x, int y) { return (uint32_t)(((y & 7) << 3) | (x & 7)); }
// byte offset of cell (x, y) in the window of scan h; false when the cell lies outside it (a point farther from the
// begin cell than the radius the host was given: counted in `misses`, never written -- nothing outside a window exists)
__device__ __forceinline__ bool window_off(const ScanHdr& h, int x, int y, uint32_t& off) {
  const unsigned wx = (unsigned)((x >> 3) - h.tx0), wy = (unsigned)((y >> 3) - h.ty0);
  off = ((h.base + wy * (unsigned)h.tw + wx) << 6) + in_tile(x, y);  // 32-bit: the host keeps a round below 2^26 slots
  return wx < (unsigned)h.tw && wy < (unsigned)h.th;
}

__global__ void __launch_bounds__(256)
k_lo_batch_hits(BatchGeom g, const ScanHdr* __restrict__ hdr, const float* __restrict__ pts, uint8_t* __restrict__ pool,
                uint8_t* __restrict__ flags, uint32_t* __restrict__ hkey, uint32_t* __restrict__ hhit,
                unsigned long long* __restrict__ misses) {
  const int sidx = blockIdx.y;
  const ScanHdr h = hdr[sidx];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h.n) return;
  const Line l = batch_line(g, h, pts, i);
  if (!l.valid) return;
  const uint32_t cell = (uint32_t)(l.y1 * g.sx + l.x1);
  const uint32_t t = tile_of(g, l.x1, l.y1);
  uint32_t off;
  if (!window_off(h, l.x1, l.y1, off)) {
    atomicAdd(misses, 1ull);
    return;
  }
  pool[off] = (uint8_t)(g.tag | kCodeHit);
  flags[(size_t)t * kBatchSlots + sidx] = (uint8_t)(g.tag | 1u);
  const size_t hb = (size_t)sidx * (g.hash_mask + 1);
  uint32_t slot = hash_slot0(cell, g.hash_mask);
  for (;;) {
    const uint32_t old = atomicCAS(&hkey[hb + slot], kHashEmpty, cell);
    if (old == kHashEmpty || old == cell) break;
    slot = (slot + 1) & g.hash_mask;
  }
  atomicMin(&hhit[hb + slot], (uint32_t)i);
}

// The same marking with the scan's hash built in LDS: one block per scan.  The compare-and-swap that claims a slot
// returns a value, and a returning device-scope atomic is executed at the memory side -- a microsecond-class round trip
// per probe; in LDS it is a few dozen cycles.  The finished table is written out with plain stores for k_lo_batch_rays.
__global__ void __launch_bounds__(1024)
k_lo_batch_hits_lds(BatchGeom g, const ScanHdr* __restrict__ hdr, const float* __restrict__ pts, uint8_t* __restrict__ pool,
                    uint8_t* __restrict__ flags, uint32_t* __restrict__ hkey, uint32_t* __restrict__ hhit,
                    unsigned long long* __restrict__ misses) {
  extern __shared__ uint32_t sh_hash[];
  const uint32_t slots = g.hash_mask + 1;
  uint32_t* key = sh_hash;
  uint32_t* first = sh_hash + slots;
  const int sidx = blockIdx.x, tid = threadIdx.x;
  const ScanHdr h = hdr[sidx];
  for (uint32_t i = tid; i < 2 * slots; i += 1024) sh_hash[i] = kHashEmpty;
  __syncthreads();
  for (int i = tid; i < h.n; i += 1024) {
    const Line l = batch_line(g, h, pts, i);
    if (!l.valid) continue;
    const uint32_t cell = (uint32_t)(l.y1 * g.sx + l.x1);
    const uint32_t t = tile_of(g, l.x1, l.y1);
    uint32_t off;
    if (!window_off(h, l.x1, l.y1, off)) {
      atomicAdd(misses, 1ull);
      continue;
    }
    pool[off] = (uint8_t)(g.tag | kCodeHit);
    flags[(size_t)t * kBatchSlots + sidx] = (uint8_t)(g.tag | 1u);
    uint32_t slot = hash_slot0(cell, g.hash_mask);
    for (;;) {
      const uint32_t old = atomicCAS(&key[slot], kHashEmpty, cell);
      if (old == kHashEmpty || old == cell) break;
      slot = (slot + 1) & g.hash_mask;
    }
    atomicMin(&first[slot], (uint32_t)i);
  }
  __syncthreads();
  const size_t hb = (size_t)sidx * slots;
  for (uint32_t i = tid; i < slots; i += 1024) {
    hkey[hb + i] = key[i];
    hhit[hb + i] = first[i];
  }
}

#if !defined(LSLAM_TUNE_RAY_BEAMS)
#define LSLAM_TUNE_RAY_BEAMS 4
#endif
LSLAM_STAMP_TABLE(g_map_stamps)  // kernel 0 = k_lo_batch_rays: 0 header, 1 beam line, 2 cell addresses, 3 plane bytes back, 4 marks issued
constexpr int kRayBeamsPerWave = LSLAM_TUNE_RAY_BEAMS;  // consecutive beams one wave walks: fewer, longer waves (dispatch-rate bound otherwise)
__global__ void __launch_bounds__(256)
k_lo_batch_rays(BatchGeom g, const ScanHdr* __restrict__ hdr, const float* __restrict__ pts, uint8_t* __restrict__ pool,
                uint8_t* __restrict__ flags, const uint32_t* __restrict__ hkey, uint32_t* __restrict__ hcross, int groups_per_scan) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // wave index = scan * groups_per_scan + beam group
  const int sidx = w / groups_per_scan, grp = w - sidx * groups_per_scan;
  if (sidx >= g.K) return;
  LSLAM_PHASE_CLOCK(pck);
  const ScanHdr h = hdr[sidx];
  const uint32_t crossed = g.tag | kCodeCrossed, hit = g.tag | kCodeHit;
  const size_t hb = (size_t)sidx * (g.hash_mask + 1);
  LSLAM_PHASE_MARK(pck, 0);
  // The wave's points in ONE load (lane j = beam j of the group), handed out by v_readlane: the per-beam point load was a
  // round trip of its own in front of every beam's cells -- 1 850 of a beam's ~5 400 cycles (tools/phase_stamps.py rays,
  // profiles/r06/phase_stamps_rays.json).  The line itself is evaluated per beam from the broadcast point, bit for bit as before.
  const int i_first = grp * kRayBeamsPerWave, i_end = min(h.n, (grp + 1) * kRayBeamsPerWave);
  float2 my_pt = make_float2(0.f, 0.f);
  if (lane < kRayBeamsPerWave && i_first + lane < i_end) my_pt = ((const float2*)pts)[(size_t)h.pts_off + i_first + lane];
  for (int i = i_first; i < i_end; i++) {
    const float bpt[2] = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_pt.x), i - i_first)),
                          __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_pt.y), i - i_first))};
    LevelGeom lg;
    lg.sx = g.sx; lg.sy = g.sy; lg.c = h.c; lg.s = h.s; lg.tx = h.tx; lg.ty = h.ty; lg.factor = g.factor;
    lg.just_once = 0; lg.bx = h.bx; lg.by = h.by; lg.metres_per_cell = 0.0;
    const Line l = beam_line(lg, bpt, 0);  // (batch_line with the point already in registers)
    LSLAM_PHASE_MARK(pck, 1);
    if (!l.valid) continue;
    // the reference's traversal (H/map/OccGridMapBase.h:240-299) in closed form, here as (x, y): cell c of the ray is c
    // major steps and q(c) = floor((abs_da/2 + c*abs_db) / abs_da) minor steps from the begin cell (see ray_cell)
    const int dx = l.x1 - l.x0, dy = l.y1 - l.y0;
    const unsigned abs_dx = (unsigned)abs(dx), abs_dy = (unsigned)abs(dy);
    const int sgx = dx > 0 ? 1 : -1, sgy = dy > 0 ? 1 : -1;  // util::sign: sign(0) = -1
    const bool xmajor = abs_dx >= abs_dy;
    const unsigned abs_da = xmajor ? abs_dx : abs_dy, abs_db = xmajor ? abs_dy : abs_dx;
    // q(c): the numerator stays below 2^31 (map sides <= 32768) and the quotient below 2^16, so a float estimate is
    // within +-1 of it and two integer corrections make it exact (a 64-bit integer division per cell otherwise)
    const float rcp_da = 1.0f / (float)abs_da;
    for (unsigned c = lane; c < abs_da; c += 64) {
      LSLAM_PHASE_MARK(pck, 2);
      const unsigned num = abs_da / 2 + c * abs_db;
      unsigned q = (unsigned)((float)num * rcp_da);
      int rem = (int)(num - q * abs_da);
      if (rem < 0) { q -= 1; rem += (int)abs_da; }
      if (rem < 0) { q -= 1; rem += (int)abs_da; }
      if (rem >= (int)abs_da) { q += 1; rem -= (int)abs_da; }
      if (rem >= (int)abs_da) { q += 1; }
      const int x = l.x0 + (xmajor ? (int)c * sgx : (int)q * sgx);
      const int y = l.y0 + (xmajor ? (int)q * sgy : (int)c * sgy);
      const uint32_t t = tile_of(g, x, y);
      uint32_t off;
      if (!window_off(h, x, y, off)) {  // (the end cell of this beam is outside too: k_lo_batch_hits counted it)
        continue;
      }
      uint8_t* plane = pool;  // (the window's bytes: `off` is an offset into the pool)
      const uint32_t b = plane[off];
      LSLAM_PHASE_MARK(pck, 3);
      if (b == hit) {  // some beam of this scan ends here: remember the first beam that crosses it
        const uint32_t cell = (uint32_t)(y * g.sx + x);
        uint32_t slot = hash_slot0(cell, g.hash_mask);
        while (hkey[hb + slot] != cell) slot = (slot + 1) & g.hash_mask;  // entered by k_lo_batch_hits
        atomicMin(&hcross[hb + slot], (uint32_t)i);
      } else if (b != crossed) {
        plane[off] = (uint8_t)crossed;
        flags[(size_t)t * kBatchSlots + sidx] = (uint8_t)(g.tag | 1u);
      }
      LSLAM_PHASE_MARK(pck, 4);
    }
  }
  LSLAM_PHASE_FLUSH(pck, g_map_stamps, 0, (unsigned)w, lane == 0);
}

// hash entry -> plane byte: a hit cell that an EARLIER beam of the same scan crossed becomes HIT_UNDO, so the apply
// pass needs nothing but the plane bytes (per-cell hash look-ups there were serialised dependent loads on the
// wall cells: 160 us per batch)
__global__ void __launch_bounds__(256)
k_lo_batch_resolve(BatchGeom g, const ScanHdr* __restrict__ hdr, const uint32_t* __restrict__ hkey,
                   const uint32_t* __restrict__ hhit, const uint32_t* __restrict__ hcross, uint8_t* __restrict__ pool) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t slots = (size_t)g.hash_mask + 1;
  if (idx >= slots * g.K) return;
  const uint32_t cell = hkey[idx];
  if (cell == kHashEmpty) return;
  if (hcross[idx] < hhit[idx]) {
    const int x = (int)(cell % (uint32_t)g.sx), y = (int)(cell / (uint32_t)g.sx);
    uint32_t off;
    if (window_off(hdr[idx / slots], x, y, off)) pool[off] = (uint8_t)(g.tag | kCodeHitUndo);  // (entered only from inside)
  }
}

// one wave per tile: lane = plane slot when reading the flags, lane = cell of the tile when applying
__global__ void __launch_bounds__(256)
k_lo_batch_apply(BatchGeom g, const ScanHdr* __restrict__ hdr, const uint8_t* __restrict__ pool,
                 const uint8_t* __restrict__ flags, float* __restrict__ logodds) {
  const int lane = threadIdx.x & 63;
  const uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (t >= (uint32_t)g.n_tiles) return;
  const uint32_t f = flags[(size_t)t * kBatchSlots + lane];
  unsigned long long touched = __ballot(lane < g.K && (f & 0xFCu) == g.tag && (f & 3u) != 0u);  // wave-uniform
  if (!touched) return;
  const int x = (int)(t % (uint32_t)g.tiles_x) * 8 + (lane & 7), y = (int)(t / (uint32_t)g.tiles_x) * 8 + (lane >> 3);
  const bool in_map = x < g.sx && y < g.sy;
  float v = in_map ? logodds[(size_t)y * g.sx + x] : 0.f;
  bool dirty = false;
  // lane s: where THIS tile sits in the window of scan s (one 16-byte load per lane; read back per touched scan by
  // v_readlane with a uniform index)
  const int ttx = (int)(t % (uint32_t)g.tiles_x), tty = (int)(t / (uint32_t)g.tiles_x);
  uint32_t my_off = 0u;
  if (lane < g.K) {
    const int4 w = *(const int4*)((const char*)(hdr + lane) + 32);  // tx0, ty0, tw, base
    my_off = (((uint32_t)w.w + (uint32_t)(tty - w.y) * (uint32_t)w.z + (uint32_t)(ttx - w.x)) << 6);
  }
  // ascending slot = scan order; kApplyChunk planes' bytes in flight at a time (the mask is wave-uniform)
  while (touched) {
    int sl[kApplyChunk];
#pragma unroll
    for (int u = 0; u < kApplyChunk; u++) {
      sl[u] = touched ? __ffsll((long long)touched) - 1 : -1;
      touched &= touched - 1;  // 0 stays 0
    }
    uint32_t bv[kApplyChunk];
#pragma unroll
    for (int u = 0; u < kApplyChunk; u++) {
      bv[u] = 0u;
      if (sl[u] >= 0) {  // wave-uniform; a flagged tile lies inside the window of the scan that flagged it
        const uint32_t tile_off = (uint32_t)__builtin_amdgcn_readlane((int)my_off, sl[u]);
        bv[u] = (uint32_t)pool[tile_off + (uint32_t)lane];
      }
    }
#pragma unroll
    for (int u = 0; u < kApplyChunk; u++) {
      const uint32_t b = bv[u];
      if ((b & 0xFCu) != g.tag) continue;  // also the empty slots (tags start at 1 << 2)
      const uint32_t code = b & 3u;
      if (code == kCodeCrossed) {
        v += g.lo_free;  // bresenhamCellFree, once per scan (:302-313)
        dirty = true;
      } else if (code != 0u) {  // bresenhamCellOcc (:316-330)
        if (code == kCodeHitUndo) {  // crossed by an EARLIER beam: marked free, then un-marked
          v += g.lo_free;
          v -= g.lo_free;
        }
        if (v < 50.0f) v += g.lo_occ;  // updateSetOccupied (H/map/GridMapLogOdds.h:108-114)
        dirty = true;
      }
    }
  }
  if (dirty && in_map) logodds[(size_t)y * g.sx + x] = v;
}

// ------------------------------------------------------------------------------------------
// LaserScan -> Hector DataContainer on the device: what HectorMappingRos::scanCallback does
// before the map sees a scan -- laser_geometry's projectLaser(scan, cloud, 30.0) (hector_slam.cc:193) and
// rosPointCloudToDataContainer (hector_slam.cc:320-362).  One block; order-preserving compaction (the container
// keeps the beams' order, which the once-per-scan cell rule depends on).
//   projection   p = (double)r * (cos, sin)(angle_min + i * angle_increment), cast to float32 -- the cos/sin table is
//                built on the HOST once per scan geometry and cached, exactly as laser_geometry caches its
//                co_sine_map_: the device multiplies, it never evaluates a trigonometric function here
//   filters      r < cutoff && r >= range_min;  min_dist^2 < d2 < max_dist^2;  !(x < 0 && d2 < 0.5);
//                d2 <= use_max^2;  z window of the laser frame (hector_slam.cc:336-354)
//   transform    base_link <- laser (planar: yaw + translation), tf's double arithmetic, then float32 * scaleToMap
// ------------------------------------------------------------------------------------------
struct ProjectCfg {
  int n;
  float range_min, cutoff, sqr_min, sqr_max;
  double use_max_sq;
  float z_min, z_max;
  double cy, sy, tx, ty, tz;  // base_link -> laser transform: rotation about z (host cos/sin) + origin
  float scale_to_map;
};

// Order-preserving compaction of one block of 1024: keep(i, ox, oy) says whether beam i enters and what it becomes.  Rounds
// of 1024 beams; the count stays on the device.
template <class Keep>
__device__ __forceinline__ void hector_compact(int n, float* __restrict__ out_xy, int* __restrict__ out_n, Keep keep_fn) {
  __shared__ int s_wave[16];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + tid;
    float ox = 0.f, oy = 0.f;
    const bool keep = i < n && keep_fn(i, ox, oy);
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int before = s_base;
    for (int w = 0; w < wv; w++) before += s_wave[w];
    if (keep) {
      const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
      out_xy[2 * pos] = ox;
      out_xy[2 * pos + 1] = oy;
    }
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int w = 0; w < 16; w++) tot += s_wave[w];
      s_base += tot;
    }
    __syncthreads();
  }
  if (tid == 0) *out_n = s_base;
}

// rosPointCloudToDataContainer's loop body (hector_slam.cc:333-358) for one point of the cloud
__device__ __forceinline__ bool hector_cloud_point(const ProjectCfg& c, float x, float y, float z, float& ox, float& oy) {
  const float d2 = x * x + y * y;  // :335
  if (!(d2 > c.sqr_min && d2 < c.sqr_max && !(x < 0.0f && d2 < 0.50f) && !((double)d2 > c.use_max_sq))) return false;
  // tf::Transform * tf::Vector3 in double (:348): row . v, then + origin
  const double bx = (c.cy * (double)x + (-c.sy) * (double)y + 0.0 * (double)z) + c.tx;
  const double by = (c.sy * (double)x + c.cy * (double)y + 0.0 * (double)z) + c.ty;
  const double bz = (0.0 * (double)x + 0.0 * (double)y + 1.0 * (double)z) + c.tz;
  const float zl = (float)(bz - c.tz);  // pointPosLaserFrameZ (:351)
  if (!(zl > c.z_min && zl < c.z_max)) return false;
  ox = (float)bx * c.scale_to_map;  // Eigen::Vector2f(x, y) * scaleToMap (:356)
  oy = (float)by * c.scale_to_map;
  return true;
}

// one LaserScan -> DataContainer, one block of 1024 (k_hector_project, and k_hf_project with a member's configuration)
__device__ __forceinline__ void hector_project_body(const ProjectCfg& c, const float* __restrict__ ranges,
                                                    const double2* __restrict__ cossin, float* __restrict__ out_xy,
                                                    int* __restrict__ out_n) {
  hector_compact(c.n, out_xy, out_n, [&](int i, float& ox, float& oy) {
    const float r = ranges[i];
    if (!(r < c.cutoff && r >= c.range_min)) return false;  // laser_geometry::projectLaser_ (NaN fails both)
    const double2 cs = cossin[i];
    const float x = (float)((double)r * cs.x), y = (float)((double)r * cs.y);  // sensor_msgs/PointCloud: float32
    return hector_cloud_point(c, x, y, 0.0f, ox, oy);                          // (projectLaser's cloud has z = 0)
  });
}

__global__ void __launch_bounds__(1024)
k_hector_project(ProjectCfg c, const float* __restrict__ ranges, const double2* __restrict__ cossin,
                 float* __restrict__ out_xy, int* __restrict__ out_n) {
  hector_project_body(c, ranges, cossin, out_xy, out_n);
}

// A de-skewed cloud (lslam_deskew_*: xyz + valid per beam) -> DataContainer: rosPointCloudToDataContainer applied to the
// beams with valid = 1, in beam order.  ProjectCfg's range_min / cutoff are not read.
__global__ void __launch_bounds__(1024)
k_hector_cloud_container(ProjectCfg c, const float* __restrict__ xyz, const uint8_t* __restrict__ valid,
                         float* __restrict__ out_xy, int* __restrict__ out_n) {
  hector_compact(c.n, out_xy, out_n, [&](int i, float& ox, float& oy) {
    if (!valid[i]) return false;
    return hector_cloud_point(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ox, oy);
  });
}

__global__ void k_occupancy_i8(const float* __restrict__ v, int8_t* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x = v[i];
  out[i] = x < 0.0f ? (int8_t)0 : (x > 0.0f ? (int8_t)100 : (int8_t)-1);  // hector_slam.cc:287-304
}

// ------------------------------------------------------------------------------------------
// Hector Gauss-Newton scan-to-map matcher (next-row #2): MapRepMultiMap::matchData
// (H/slam_main/MapRepMultiMap.h:144-167) -> ScanMatcher::matchData / estimateTransformationLogLh
// (H/matcher/ScanMatcher.h:60-139) -> OccGridMapUtil::getCompleteHessianDerivs /
// interpMapValueWithDerivatives (H/map/OccGridMapUtil.h:77-228).  One block per scan walks all
// pyramid levels and iterations: every thread evaluates the bilinear map value + gradient of its
// points and their 9 Hessian/gradient terms in fp32 (parallel), ONE thread then adds the terms in
// point order -- the reference accumulates H and dTr sequentially in fp32, so the order is part of
// the result -- and solves the 3x3 system.  The probability cache of the reference
// (GridMapCacheArray) is a pure memoisation and has no device counterpart.
// ------------------------------------------------------------------------------------------
constexpr int kGnMaxLevels = 8;
struct GnLevels {
  int n_levels;
  int sx[kGnMaxLevels], sy[kGnMaxLevels];
  float scale[kGnMaxLevels], t_x[kGnMaxLevels], t_y[kGnMaxLevels];
  const float* logodds[kGnMaxLevels];
};

// A pointer that a kernel reads from a table in memory is a generic one to the compiler, which then addresses through it with
// flat instructions and a 64-bit address in vector registers; a kernel argument it knows to point into device memory (global
// instructions: scalar base + 32-bit offset).  This says so for the former and changes nothing for the latter.
template <class T>
__device__ __forceinline__ T* in_device_memory(T* p) {
  typedef T __attribute__((address_space(1))) * Global;
  return (T*)(Global)(uintptr_t)p;  // (by way of the integer: a cast there and straight back folds away)
}

__device__ __forceinline__ float gn_prob(const float* lo, int index) {  // getGridProbability (GridMapLogOdds.h:123-127)
  float odds = (float)exp((double)lo[index]);
  return odds / (odds + 1.0f);
}

__device__ __forceinline__ float gn_cof3(const float* m, int i, int j) {
  int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
}

// ---- the statements every form of the matcher shares: ONE copy each, plain inlined functions on values.  The library is
// built with -ffp-contract=off, so a result's bits follow from the order of these expressions and from nothing else.

// The solve + pose update after the nine sums (estimateTransformationLogLh, ScanMatcher.h:113-133); H is the Hessian as summed
__device__ __forceinline__ void gn_solve_step(const float* sum, float* H, float& e0, float& e1, float& e2) {
  const float d0 = sum[0], d1 = sum[1], d2 = sum[2], h00 = sum[3], h11 = sum[4], h22 = sum[5], h01 = sum[6], h02 = sum[7],
              h12 = sum[8];
  H[0] = h00; H[1] = h01; H[2] = h02; H[3] = h01; H[4] = h11; H[5] = h12; H[6] = h02; H[7] = h12; H[8] = h22;
  if (h00 != 0.0f && h11 != 0.0f) {
    const float c0 = gn_cof3(H, 0, 0), c1 = gn_cof3(H, 1, 0), c2 = gn_cof3(H, 2, 0);
    const float det = c0 * H[0] + (c1 * H[3] + c2 * H[6]);
    const float invdet = 1.0f / det;
    const float Hi[9] = {c0 * invdet, c1 * invdet, c2 * invdet,
                         gn_cof3(H, 0, 1) * invdet, gn_cof3(H, 1, 1) * invdet, gn_cof3(H, 2, 1) * invdet,
                         gn_cof3(H, 0, 2) * invdet, gn_cof3(H, 1, 2) * invdet, gn_cof3(H, 2, 2) * invdet};
    float sd[3];
    // H.inverse() * dTr: Eigen's coefficient-based product sums a 3-term row as a0 + (a1 + a2) (Core/Redux.h)
    for (int r = 0; r < 3; r++) sd[r] = Hi[3 * r] * d0 + (Hi[3 * r + 1] * d1 + Hi[3 * r + 2] * d2);
    if (sd[2] > 0.2f) sd[2] = 0.2f; else if (sd[2] < -0.2f) sd[2] = -0.2f;
    e0 += sd[0]; e1 += sd[1]; e2 += sd[2];
  }
}

// level prologue: the world estimate on a level's raster, getMapCoordsPose (GridMapBase.h:238-242)
__device__ __forceinline__ void gn_level_begin(float sc, float t_x, float t_y, float tmp0, float tmp1, float tmp2, float& e0,
                                               float& e1, float& e2) {
  e0 = (sc * tmp0 + 0.0f * tmp1) + t_x;
  e1 = (0.0f * tmp0 + sc * tmp1) + t_y;
  e2 = tmp2;
}

// level epilogue: the level's estimate back in the world, heading normalised
__device__ __forceinline__ void gn_level_end(float sc, float t_x, float t_y, float e0, float e1, float e2, float& tmp0,
                                             float& tmp1, float& tmp2) {
  // util::normalize_angle (UtilFunctions.h:36-48), double arithmetic with M_PI
  const double two_pi = 2.0f * 3.14159265358979323846;
  float a = (float)fmod(fmod((double)e2, two_pi) + two_pi, two_pi);
  if ((double)a > 3.14159265358979323846) a = (float)((double)a - two_pi);
  // getWorldCoordsPose: worldTmap = mapTworld.inverse() (GridMapBase.h:229-233, 285)
  const float invdet = 1.0f / (sc * sc - 0.0f * 0.0f);
  const float l00 = sc * invdet, l01 = -0.0f * invdet, l10 = -0.0f * invdet, l11 = sc * invdet;
  const float wt0 = -(l00 * t_x + l01 * t_y), wt1 = -(l10 * t_x + l11 * t_y);
  tmp0 = (l00 * e0 + l01 * e1) + wt0;
  tmp1 = (l10 * e0 + l11 * e1) + wt1;
  tmp2 = a;
}

// bilinear map value and gradient {v, gxv, gyv} from the four cell probabilities (interpMapValueWithDerivatives,
// OccGridMapUtil.h:77-139); `in_map` false: all three are 0 (the straight-line forms read cell 0 for such a point and mask it
// here).  The mask and the array result are deliberate: with three float& results and the callers masking afterwards hipcc split
// gn_chunk's loads into two dependent groups (k_gn_match_reg<512,3>: its six 8-byte loads as 2 + 4 with a wait in between) and
// a match took 36.63 / 36.90 / 36.65 us against 34.59 / 34.61 / 34.49 with the statements written out (MI355X, three
// alternating runs; DESIGN.md 4.14 "One matcher body" has the table of the form below, which keeps every kernel's load groups).
__device__ __forceinline__ void gn_interp(float i0, float i1, float i2, float i3, float fx, float fy, bool in_map, float* out) {
  const float dx1 = i0 - i1, dx2 = i2 - i3, dy1 = i0 - i2, dy2 = i1 - i3;
  const float xi = 1.0f - fx, yi = 1.0f - fy;
  const float v = in_map ? ((i0 * xi + i1 * fx) * (yi)) + ((i2 * xi + i3 * fx) * (fy)) : 0.0f;
  const float gxv = in_map ? -((dx1 * yi) + (dx2 * fy)) : 0.0f;
  const float gyv = in_map ? -((dy1 * xi) + (dy2 * fx)) : 0.0f;
  out[0] = v; out[1] = gxv; out[2] = gyv;
}

// one point's nine products (getCompleteHessianDerivs, OccGridMapUtil.h:141-183): dTr[0..2], then H's 00 11 22 01 02 12
template <bool ADD>
__device__ __forceinline__ void gn_terms9(float gxv, float gyv, float funVal, float rotDeriv, float* t) {
  const float p[9] = {gxv * funVal, gyv * funVal, rotDeriv * funVal, gxv * gxv, gyv * gyv, rotDeriv * rotDeriv,
                      gxv * gyv, gxv * rotDeriv, gyv * rotDeriv};
#pragma unroll
  for (int q = 0; q < 9; q++) t[q] = ADD ? t[q] + p[q] : p[q];
}

// (the body of k_gn_match; k_gn_match_batch_ordered runs the same statements with one block per entry of a batch)
__device__ __forceinline__ void gn_match_ordered(const GnLevels& lv, const float* __restrict__ pts, int n, float bx, float by,
                                                 float bth, float* __restrict__ out_pose /* [3] */,
                                                 float* __restrict__ out_H /* [9], may be null */) {
  extern __shared__ float terms[];  // [n][9]
  __shared__ float s_est[3], s_sum[9];
  const int tid = threadIdx.x, nt = blockDim.x;
  float tmp0 = bx, tmp1 = by, tmp2 = bth;
  float Hlast[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int L = lv.n_levels - 1; L >= 0; --L) {
    if (n == 0) continue;
    const float* lo = lv.logodds[L];
    const int sx = lv.sx[L], sy = lv.sy[L];
    const float sc = lv.scale[L];
    const float factor = L == 0 ? 1.0f : (float)(1.0 / pow(2.0, (double)L));
    const int iters = 1 + (L == 0 ? 5 : 3);
    if (tid == 0) gn_level_begin(sc, lv.t_x[L], lv.t_y[L], tmp0, tmp1, tmp2, s_est[0], s_est[1], s_est[2]);
    __syncthreads();
    for (int it = 0; it < iters; it++) {
      const float e0 = s_est[0], e1 = s_est[1], e2 = s_est[2];
      const float c = (float)cos((double)e2), s = (float)sin((double)e2);  // Rotation2Df + sinRot/cosRot (:85-88)
      const float lim_x = (float)sx - 2.0f, lim_y = (float)sy - 2.0f;     // MapDimensionProperties.h:66-70
      for (int i = tid; i < n; i += nt) {
        const float px = pts[2 * i] * factor, py = pts[2 * i + 1] * factor;
        const float cx = (c * px + (-s) * py) + e0;
        const float cy = (s * px + c * py) + e1;
        float v = 0.0f, gxv = 0.0f, gyv = 0.0f;
        if (!(cx < 0.0f || cx > lim_x || cy < 0.0f || cy > lim_y)) {  // pointOutOfMapBounds (:60-63)
          const int ix = (int)cx, iy = (int)cy;
          const int index = iy * sx + ix;
          float o[3];
          gn_interp(gn_prob(lo, index), gn_prob(lo, index + 1), gn_prob(lo, index + sx), gn_prob(lo, index + sx + 1),
                    cx - (float)ix, cy - (float)iy, true, o);
          v = o[0]; gxv = o[1]; gyv = o[2];
        }
        const float funVal = 1.0f - v;
        const float rotDeriv = ((-s * px - c * py) * gxv + (c * px - s * py) * gyv);
        gn_terms9<false>(gxv, gyv, funVal, rotDeriv, terms + 9 * i);
      }
      __syncthreads();
      // sequential fp32 accumulation in point order (:94-126): the nine sums are independent chains, so
      // nine lanes walk the points, one chain each -- same order, same roundings, a ninth of the latency
      if (tid < 9) {
        float acc = 0.0f;
#pragma unroll 8
        for (int i = 0; i < n; i++) acc += terms[9 * i + tid];
        s_sum[tid] = acc;
      }
      __syncthreads();
      if (tid == 0) gn_solve_step(s_sum, Hlast, s_est[0], s_est[1], s_est[2]);
      __syncthreads();
    }
    if (tid == 0) gn_level_end(sc, lv.t_x[L], lv.t_y[L], s_est[0], s_est[1], s_est[2], tmp0, tmp1, tmp2);
    __syncthreads();
  }
  if (tid == 0) {
    out_pose[0] = tmp0; out_pose[1] = tmp1; out_pose[2] = tmp2;
    if (out_H)
      for (int q = 0; q < 9; q++) out_H[q] = Hlast[q];
  }
}

__global__ void __launch_bounds__(1024)
k_gn_match(GnLevels lv, const float* __restrict__ pts, int n, float bx, float by, float bth,
           float* __restrict__ out /* pose[3] + H[9] */) {
  gn_match_ordered(lv, pts, n, bx, by, bth, out, out + 3);
}

// ------------------------------------------------------------------------------------------
// k_gn_match_fast -- the same Gauss-Newton matcher, summed in PARALLEL (round 4; the default).
// k_gn_match above adds the nine H / dTr sums in point order on nine lanes so that they round like the reference's
// sequential fp32 loop (it equals the CPU restatement bit for bit): 1081 dependent LDS adds per iteration, fourteen
// iterations, on one CU.  The north star grants 1e-4 m / 1e-4 rad for floating point, device libm already differs from
// glibc in the last bit, and a tree sum is -- if anything -- the more accurate one.  Here every thread keeps nine
// partial sums of ITS points in registers, a wave adds them with DPP row operations (no LDS round trip), the waves'
// partials meet in LDS and EVERY thread adds them up and solves the 3x3 system itself (same inputs, same operations:
// bitwise the same estimate in every thread), so an iteration has ONE barrier and no single-thread phase.  exp / sin /
// cos are the float32 ocml functions (<= 1 ulp; the ordered kernel evaluates them in double like the reference's host
// code).  Points are staged once in LDS; the kernel also writes the cached container (MapRepMultiMap.h:161) when the
// points come from pinned host memory, and its result lands in pinned host memory: no copy operation on the stream.
// LSLAM_MAP_OPT_ORDERED_SUMS selects the ordered kernel (the bit comparison with the restatement).
// The matcher itself is gn_match_fast_body / gn_match_reg_body, which hand pose[3] and H[9] back in every thread: the
// single-call kernels here write them out with the ticket, the streamed k_hs_match_* go on to the update decision.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float gn_row16_sum(float v) {  // every lane of a 16-lane row ends up with the row's sum
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));  // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true));  // row_mirror
  return v;
}
__device__ __forceinline__ float gn_wave_sum(float v) {
  v = gn_row16_sum(v);
  const int b = __float_as_int(v);
  return (__int_as_float(__builtin_amdgcn_readlane(b, 0)) + __int_as_float(__builtin_amdgcn_readlane(b, 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(b, 32)) + __int_as_float(__builtin_amdgcn_readlane(b, 48)));
}
// getGridProbability (GridMapLogOdds.h:123-127) on the hardware's exp2 / reciprocal units (v_exp_f32, v_rcp_f32: ~1e-7
// relative, far inside the 1e-4 the matcher's result is held to).  Log-odds stay below ~52 (the occupied clamp,
// GridMapLogOdds.h:110), so odds + 1 neither overflows nor leaves __fdividef's range; -inf gives 0.
__device__ __forceinline__ float gn_prob_f(float lo) {
  const float odds = __expf(lo);
  return odds * __builtin_amdgcn_rcpf(odds + 1.0f);  // (__fdividef compiles to the full IEEE division sequence here)
}
// Nine wave sums at once: the four row steps of all nine values interleaved (no DPP read-after-write stalls), then the two
// cross-row broadcasts of GFX9's wave64 DPP; the totals are valid in LANE 63 only.
__device__ __forceinline__ void gn_wave_sums9(float* v) {
#define LSLAM_DPP_STEP(CTRL)                                                                                            \
  _Pragma("unroll") for (int q = 0; q < 9; q++)                                                                         \
      v[q] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v[q]), CTRL, 0xF, 0xF, true));
  LSLAM_DPP_STEP(0xB1)   // quad_perm [1,0,3,2]
  LSLAM_DPP_STEP(0x4E)   // quad_perm [2,3,0,1]
  LSLAM_DPP_STEP(0x141)  // row_half_mirror
  LSLAM_DPP_STEP(0x140)  // row_mirror: every lane of a 16-lane row holds the row's sum
#undef LSLAM_DPP_STEP
#pragma unroll
  for (int q = 0; q < 9; q++)  // row_bcast:15 into rows 1 and 3: row 1 = rows 0+1, row 3 = rows 2+3
    v[q] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[q]), 0x142, 0xA, 0xF, false));
#pragma unroll
  for (int q = 0; q < 9; q++)  // row_bcast:31 into rows 2 and 3: row 3 = all four rows
    v[q] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[q]), 0x143, 0xC, 0xF, false));
}
// sin / cos of the pose heading: |x| stays within a few radians (a normalised start estimate plus steps clamped to 0.2),
// so the quadrant reduction is two fused steps of x - k * pi/2 with pi/2 split in two floats (exact to ~1e-8 for |k| <= 8)
// and the rest the classic degree-7 / degree-8 kernels on [-pi/4, pi/4] (~1 ulp).  ocml's sincosf carries the
// large-argument path along: four times the instructions, every thread, every iteration.
__device__ __forceinline__ void gn_sincos(float x, float* sn, float* cs) {
  const float k = rintf(x * 0.636619772367581343f);
  const int q = (int)k;
  float r = fmaf(-k, 1.57079601287841796875f, x);   // pi/2 hi (24 bits)
  r = fmaf(-k, 3.1391647326017846e-7f, r);            // pi/2 lo
  const float r2 = r * r;
  float ps = fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f);
  ps = fmaf(ps, r2, -1.6666654611e-1f);
  ps = fmaf(ps * r2, r, r);                           // sin r
  float pc = fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f);
  pc = fmaf(pc, r2, 4.166664568298827e-2f);
  pc = fmaf(pc, r2, -0.5f);
  pc = fmaf(pc, r2, 1.0f);                            // cos r
  const float s0 = (q & 1) ? pc : ps, c0 = (q & 1) ? ps : pc;
  *sn = (q & 2) ? -s0 : s0;
  *cs = ((q + 1) & 2) ? -c0 : c0;
}

// The waves' nine totals meet in LDS: lane q < 9 of every wave adds the NW partials of sum q (NW LDS reads instead of 9 NW per
// lane) and readlane hands the nine block sums to all lanes.  Two buffers: the next iteration writes the other one, so an
// iteration has ONE barrier.  wave_total(q) is this wave's total of sum q, valid in the lanes where `writer` holds; it is
// evaluated right in front of its store, so a total that comes out of readlanes (gn_wave_sum) does not wait in scalar
// registers for the other eight.  That is why it is a callable and not nine values: with all nine totals computed first the
// compiler reports 106 SGPRs instead of 86 for k_hs_match_fast<NT> (97 instead of 74 for k_gn_match_fast<NT>), and
// k_hs_match_fast<256> drops from 8 waves per SIMD to 7.
template <int NW, class WaveTotal>
__device__ __forceinline__ void gn_block_sums9(WaveTotal wave_total, bool writer, int wv, int lane, int& flip, float* sum) {
  __shared__ float s_part[2][NW][12];
#pragma unroll
  for (int q = 0; q < 9; q++) {
    const float t = wave_total(q);
    if (writer) s_part[flip][wv][q] = t;
  }
  __syncthreads();
  float mine = 0.0f;
  if (lane < 9) {
    mine = s_part[flip][0][lane];
#pragma unroll
    for (int w = 1; w < NW; w++) mine += s_part[flip][w][lane];
  }
#pragma unroll
  for (int q = 0; q < 9; q++) sum[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), q));
  flip ^= 1;
}

// the staged-points form: a container of any length, its points in LDS (pts_in_lds) or read back from memory
template <int NT>
__device__ __forceinline__ void gn_match_fast_body(const GnLevels& lv, const float* __restrict__ pts, float* __restrict__ cache_dst,
                                                   int n, int pts_in_lds, float bx, float by, float bth, float* pose, float* H) {
  extern __shared__ float s_pts[];  // [2n] when pts_in_lds
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < 2 * n; i += NT) {
    const float v = pts[i];
    if (pts_in_lds) s_pts[i] = v;
    if (cache_dst) cache_dst[i] = v;
  }
  const float* P = pts_in_lds ? s_pts : (cache_dst ? cache_dst : pts);
  __syncthreads();  // (a thread reads points other threads staged; cache_dst is only re-read by its own writers' block)
  float tmp0 = bx, tmp1 = by, tmp2 = bth;
#pragma unroll
  for (int q = 0; q < 9; q++) H[q] = 0.0f;
  int flip = 0;
  for (int L = lv.n_levels - 1; L >= 0; --L) {
    if (n == 0) continue;
    const float* lo = in_device_memory(lv.logodds[L]);
    const int sx = lv.sx[L], sy = lv.sy[L];
    const float sc = lv.scale[L];
    const float factor = L == 0 ? 1.0f : 1.0f / (float)(1 << L);
    const int iters = 1 + (L == 0 ? 5 : 3);
    float e0, e1, e2;
    gn_level_begin(sc, lv.t_x[L], lv.t_y[L], tmp0, tmp1, tmp2, e0, e1, e2);
    const float lim_x = (float)sx - 2.0f, lim_y = (float)sy - 2.0f;  // MapDimensionProperties.h:66-70
    for (int it = 0; it < iters; it++) {
      float s, c;
      sincosf(e2, &s, &c);
      float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
      for (int i = tid; i < n; i += NT) {
        const float px = P[2 * i] * factor, py = P[2 * i + 1] * factor;
        const float cx = (c * px + (-s) * py) + e0;
        const float cy = (s * px + c * py) + e1;
        float v = 0.0f, gxv = 0.0f, gyv = 0.0f;
        if (!(cx < 0.0f || cx > lim_x || cy < 0.0f || cy > lim_y)) {  // pointOutOfMapBounds (:60-63)
          const int ix = (int)cx, iy = (int)cy;
          const int index = iy * sx + ix;
          const float l0 = lo[index], l1 = lo[index + 1], l2 = lo[index + sx], l3 = lo[index + sx + 1];
          float o[3];
          gn_interp(gn_prob_f(l0), gn_prob_f(l1), gn_prob_f(l2), gn_prob_f(l3), cx - (float)ix, cy - (float)iy, true, o);
          v = o[0]; gxv = o[1]; gyv = o[2];
        }
        const float funVal = 1.0f - v;
        const float rotDeriv = ((-s * px - c * py) * gxv + (c * px - s * py) * gyv);
        gn_terms9<true>(gxv, gyv, funVal, rotDeriv, acc);
      }
      float sum[9];
      gn_block_sums9<NT / 64>([&](int q) { return gn_wave_sum(acc[q]); }, lane == 0, wv, lane, flip, sum);
      gn_solve_step(sum, H, e0, e1, e2);
    }
    gn_level_end(sc, lv.t_x[L], lv.t_y[L], e0, e1, e2, tmp0, tmp1, tmp2);
  }
  pose[0] = tmp0; pose[1] = tmp1; pose[2] = tmp2;
}

// A single call's result, one thread: `out` is pinned host memory -- a system-scope fence, then the caller's ticket; the host
// spins on it instead of waiting for the stream (the completion signal + wake-up cost several microseconds of a 34 us match)
__device__ __forceinline__ void gn_write_result(float* __restrict__ out, const float* pose, const float* H, int ticket) {
  out[0] = pose[0]; out[1] = pose[1]; out[2] = pose[2];
  for (int q = 0; q < 9; q++) out[3 + q] = H[q];
  __threadfence_system();
  ((volatile int*)out)[15] = ticket;
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_gn_match_fast(GnLevels lv, const float* __restrict__ pts, float* __restrict__ cache_dst, int n, int pts_in_lds, float bx,
                float by, float bth, float* __restrict__ out /* pose[3] + H[9], [15] = ticket */, int ticket) {
  float pose[3], H[9];
  gn_match_fast_body<NT>(lv, pts, cache_dst, n, pts_in_lds, bx, by, bth, pose, H);
  if (threadIdx.x == 0) gn_write_result(out, pose, H, ticket);
}

// One straight-line pass over CH points per lane, the pattern of the register-points form and of the batch kernel: all cell
// addresses first -- an out-of-map point reads cell 0 and is masked afterwards, so no load sits behind a branch --, then the
// 4 * CH loads back to back, then the arithmetic.  One L2 round trip per pass instead of CH.  have[p] false: no point (its
// funVal is 0 as well, so it adds nothing to any sum).
template <int CH>
__device__ __forceinline__ void gn_chunk(const float* __restrict__ lo, int sx, float lim_x, float lim_y, float s, float c, float e0,
                                         float e1, const float* px, const float* py, const bool* have, float* acc) {
  int idx[CH];
  float fx[CH], fy[CH];
  bool inb[CH];
#pragma unroll
  for (int p = 0; p < CH; p++) {
    const float cx = (c * px[p] + (-s) * py[p]) + e0;
    const float cy = (s * px[p] + c * py[p]) + e1;
    inb[p] = have[p] && !(cx < 0.0f || cx > lim_x || cy < 0.0f || cy > lim_y);  // pointOutOfMapBounds (:60-63)
    const int ix = inb[p] ? (int)cx : 0, iy = inb[p] ? (int)cy : 0;
    fx[p] = cx - (float)ix;
    fy[p] = cy - (float)iy;
    idx[p] = iy * sx + ix;
  }
  float l0[CH], l1[CH], l2[CH], l3[CH];
#pragma unroll
  for (int p = 0; p < CH; p++) {
    l0[p] = lo[idx[p]];
    l1[p] = lo[idx[p] + 1];
    l2[p] = lo[idx[p] + sx];
    l3[p] = lo[idx[p] + sx + 1];
  }
#pragma unroll
  for (int p = 0; p < CH; p++) {
    float o[3];
    gn_interp(gn_prob_f(l0[p]), gn_prob_f(l1[p]), gn_prob_f(l2[p]), gn_prob_f(l3[p]), fx[p], fy[p], inb[p], o);
    const float v = o[0], gxv = o[1], gyv = o[2];
    const float funVal = have[p] ? 1.0f - v : 0.0f;
    const float rotDeriv = ((-s * px[p] - c * py[p]) * gxv + (c * px[p] - s * py[p]) * gyv);
    gn_terms9<true>(gxv, gyv, funVal, rotDeriv, acc);
  }
}

// The register-points form: gn_match_fast_body for scans of at most NT * PMAX points (every real LaserScan: 1081 beams =
// 512 x 3), the form that runs.  The staged form walks its points one after the other, and each costs a dependent LDS read,
// then a dependent round trip to L2 for the four map cells: ~3.4 us per Gauss-Newton iteration of mostly waiting.  Here a
// thread's <= PMAX points live in REGISTERS for the whole match (no LDS, no barrier in front of the first iteration), and an
// iteration is one gn_chunk<PMAX>.
template <int NT, int PMAX>
__device__ __forceinline__ void gn_match_reg_body(const GnLevels& lv, const float* __restrict__ pts, float* __restrict__ cache_dst,
                                                  int n, float bx, float by, float bth, float* pose, float* H) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float px0[PMAX], py0[PMAX];
  bool have[PMAX];
#pragma unroll
  for (int p = 0; p < PMAX; p++) {
    const int i = tid + p * NT;
    have[p] = i < n;
    float2 v = make_float2(0.0f, 0.0f);
    if (have[p]) {
      v = reinterpret_cast<const float2*>(pts)[i];
      if (cache_dst) reinterpret_cast<float2*>(cache_dst)[i] = v;
    }
    px0[p] = v.x;
    py0[p] = v.y;
  }
  float tmp0 = bx, tmp1 = by, tmp2 = bth;
#pragma unroll
  for (int q = 0; q < 9; q++) H[q] = 0.0f;
  int flip = 0;
  for (int L = lv.n_levels - 1; L >= 0; --L) {
    if (n == 0) continue;
    const float* __restrict__ lo = in_device_memory(lv.logodds[L]);
    const int sx = lv.sx[L], sy = lv.sy[L];
    const float sc = lv.scale[L];
    const float factor = L == 0 ? 1.0f : 1.0f / (float)(1 << L);
    const int iters = 1 + (L == 0 ? 5 : 3);
    float e0, e1, e2;
    gn_level_begin(sc, lv.t_x[L], lv.t_y[L], tmp0, tmp1, tmp2, e0, e1, e2);
    const float lim_x = (float)sx - 2.0f, lim_y = (float)sy - 2.0f;  // MapDimensionProperties.h:66-70
    float px[PMAX], py[PMAX];
#pragma unroll
    for (int p = 0; p < PMAX; p++) {
      px[p] = px0[p] * factor;
      py[p] = py0[p] * factor;
    }
    for (int it = 0; it < iters; it++) {
      float s, c;
      gn_sincos(e2, &s, &c);
      float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      gn_chunk<PMAX>(lo, sx, lim_x, lim_y, s, c, e0, e1, px, py, have, acc);
      gn_wave_sums9(acc);  // totals in lane 63
      float sum[9];
      gn_block_sums9<NT / 64>([&](int q) { return acc[q]; }, lane == 63, wv, lane, flip, sum);
      gn_solve_step(sum, H, e0, e1, e2);
    }
    gn_level_end(sc, lv.t_x[L], lv.t_y[L], e0, e1, e2, tmp0, tmp1, tmp2);
  }
  pose[0] = tmp0; pose[1] = tmp1; pose[2] = tmp2;
}

template <int NT, int PMAX>
__global__ void __launch_bounds__(NT)
k_gn_match_reg(GnLevels lv, const float* __restrict__ pts, float* __restrict__ cache_dst, int n, float bx, float by, float bth,
               float* __restrict__ out /* pose[3] + H[9], [15] = ticket */, int ticket) {
  float pose[3], H[9];
  gn_match_reg_body<NT, PMAX>(lv, pts, cache_dst, n, bx, by, bth, pose, H);
  if (threadIdx.x == 0) gn_write_result(out, pose, H, ticket);
}

// ------------------------------------------------------------------------------------------
// k_gn_match_batch -- MANY matchData calls against the same pyramid in one launch (lslam_map_match_batch*): entry e is
// (container ent[e].x .. + ent[e].y of the packed points, start pose begin[e]).  Built for throughput, not latency: ONE
// WAVE per entry, four entries per 256-thread block.  A wave needs nobody else: its nine sums meet by DPP
// (gn_wave_sums9) and every lane solves on the broadcast totals, so there is no LDS, no barrier and no atomic, and an
// entry's result is a function of its container, its start pose and the map only -- wherever it stands in the batch.
// A wave walks its container from memory every iteration, kGnBatchChunk points per lane at a time (point i belongs to lane
// i % 64; the reads are coalesced float2 and stay in L1 / L2 -- 8.6 KB for a 1081-beam scan), whatever the container's size:
// ONE form, no switch point.  Holding a 1081-point scan in registers instead (17 points per lane, fully unrolled) was
// tried and dropped: under the 128-VGPR cap hipcc spilled ~700 bytes per lane to scratch at every chunk size.  Each pass is
// one gn_chunk.  <= 128 VGPRs: four waves per SIMD stay resident and cover one another's L2 round trips, which is what bounds
// the single-match kernel.
// ------------------------------------------------------------------------------------------
constexpr int kGnBatchWaves = 4;                        // entries per block
constexpr int kGnBatchChunk = 6;  // points per lane whose four cell loads each are in flight together (384 per wave and pass)

__global__ void __launch_bounds__(64 * kGnBatchWaves) __attribute__((amdgpu_waves_per_eu(4)))
k_gn_match_batch(GnLevels lv, const float* __restrict__ pts, const int2* __restrict__ ent /* [n_entries]: first point, points */,
                 const float* __restrict__ begin /* [n_entries][3] */, int n_entries, float* __restrict__ out_pose /* [n_entries][3] */,
                 float* __restrict__ out_cov /* [n_entries][9], may be null */) {
  constexpr int CH = kGnBatchChunk;
  const int lane = threadIdx.x & 63;
  const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kGnBatchWaves + (threadIdx.x >> 6)));
  if (e >= n_entries) return;  // (whole waves: nothing below waits for another wave)
  const int2 en = ent[e];
  const int first = __builtin_amdgcn_readfirstlane(en.x), n = __builtin_amdgcn_readfirstlane(en.y);
  const float2* __restrict__ P = reinterpret_cast<const float2*>(pts) + first;
  float tmp0 = begin[3 * e], tmp1 = begin[3 * e + 1], tmp2 = begin[3 * e + 2];
  float H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int L = lv.n_levels - 1; L >= 0; --L) {
    if (n == 0) continue;  // ScanMatcher.h:96: an empty container returns beginEstimateWorld as it came
    const float* __restrict__ lo = lv.logodds[L];
    const int sx = lv.sx[L], sy = lv.sy[L];
    const float sc = lv.scale[L];
    const float factor = L == 0 ? 1.0f : 1.0f / (float)(1 << L);
    const int iters = 1 + (L == 0 ? 5 : 3);
    float e0, e1, e2;
    gn_level_begin(sc, lv.t_x[L], lv.t_y[L], tmp0, tmp1, tmp2, e0, e1, e2);
    const float lim_x = (float)sx - 2.0f, lim_y = (float)sy - 2.0f;  // MapDimensionProperties.h:66-70
    for (int it = 0; it < iters; it++) {
      float s, c;
      gn_sincos(e2, &s, &c);
      float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int base = 0; base < n; base += 64 * CH) {  // (n is wave-uniform: no lane leaves the loop early)
        float px[CH], py[CH];
        bool have[CH];
#pragma unroll
        for (int j = 0; j < CH; j++) {
          const int i = base + 64 * j + lane;
          have[j] = i < n;
          float2 v = make_float2(0.0f, 0.0f);
          if (have[j]) v = P[i];
          px[j] = v.x * factor;
          py[j] = v.y * factor;
        }
        gn_chunk<CH>(lo, sx, lim_x, lim_y, s, c, e0, e1, px, py, have, acc);
      }
      gn_wave_sums9(acc);  // totals in lane 63
      float sum[9];
#pragma unroll
      for (int q = 0; q < 9; q++) sum[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc[q]), 63));
      gn_solve_step(sum, H, e0, e1, e2);
    }
    gn_level_end(sc, lv.t_x[L], lv.t_y[L], e0, e1, e2, tmp0, tmp1, tmp2);
  }
  if (lane == 0) {
    out_pose[3 * e] = tmp0; out_pose[3 * e + 1] = tmp1; out_pose[3 * e + 2] = tmp2;
    if (out_cov)
      for (int q = 0; q < 9; q++) out_cov[9 * e + q] = H[q];
  }
}

// ordered sums: the single call's kernel body, one block per entry (bit-identical to lslam_map_match_data in that mode)
__global__ void __launch_bounds__(1024)
k_gn_match_batch_ordered(GnLevels lv, const float* __restrict__ pts, const int2* __restrict__ ent, const float* __restrict__ begin,
                         float* __restrict__ out_pose, float* __restrict__ out_cov) {
  const int e = blockIdx.x;
  const int2 en = ent[e];
  gn_match_ordered(lv, pts + 2 * (size_t)en.x, en.y, begin[3 * e], begin[3 * e + 1], begin[3 * e + 2], out_pose + 3 * (size_t)e,
                   out_cov ? out_cov + 9 * (size_t)e : (float*)nullptr);
}

// ------------------------------------------------------------------------------------------
// POSE SCORING (lslam_map_score_batch / lslam_map_pose_covariance_batch / lslam_map_score_lattice): how well a container
// fits one level of the map at a pose -- OccGridMapUtil::getResidualForState / getLikelihoodForState / getCovarianceForPose
// / getCovMatrixWorldCoords (H/map/OccGridMapUtil.h:249-374) with interpMapValue (:379-434).  A STATE is (container, pose
// on the level's raster, level); its residual is the sum over the container of 1 - interpMapValue(T(pose) * p * 2^-level),
// its likelihood 1 - residual / n.  Three forms feed ONE scoring kernel, which asks ms_state for the pose of state `st`:
//   batch     state e is entry e's world pose
//   cov       state 7 e + k is sigma point k of entry e (getCovarianceForPose's order); k_ms_cov, enqueued behind the scoring
//             launch, turns the seven likelihoods into the weighted covariance -- no host round trip in between
//   lattice   state (k * ny + j) * nx + i is the centre pose plus (i - nx/2, j - ny/2, k - nt/2) steps, evaluated on the
//             device (no pose array goes up); k_ms_best then finds the best state
// and ms_point is the one statement of a point's term (value only: no gradient, no nine products).
// Default mode, k_ms_score: ONE WAVE per state, kMsWaves states per block, as k_gn_match_batch -- no LDS, no barrier.  Lane l
// adds the terms of points l, l + 64, l + 128 ... in that order and gn_wave_sum adds the 64 partials, so a state's result is
// a function of its container, its pose and the map: not of the batch, the block, the form or the chunk size CH (the
// number of points per lane whose cell loads are in flight together).  Hardware exp / rcp (gn_prob_f), ocml sincosf (one
// call per state; a scoring caller's heading is not bounded the way gn_sincos asks).
// Ordered mode, k_ms_score_ordered: one block per state; the threads evaluate the terms of a chunk of points into LDS with the
// ordered matcher's gn_prob and double sin / cos, ONE thread adds them in container order like the reference's loop
// (:366-371).  A float per point and a fixed chunk: any container the map accepts.
// ------------------------------------------------------------------------------------------
constexpr int kMsBatch = 0, kMsCov = 1, kMsLattice = 2;
struct MsJob {
  int mode, n_states;
  const float* lo;      // the level: its plane, size, world -> raster scaling (gn_level_begin), the container's scaling
  int sx, sy;
  float scale, t_x, t_y, factor, cell_length;
  const float* poses;   // batch, cov: [n_entries][3] world poses
  const int2* ent;      // batch, cov: [n_entries] (first point, points)
  int first, n;         // lattice: its one container
  float c0, c1, c2, d0, d1, d2;  // lattice: centre world pose, steps
  int nx, ny, nt;
  float* out_res;       // batch: [n_states], may be null
  float* out_lik;       // [n_states]: batch's likelihoods, cov's [n_entries][7], the lattice's volume
};

// sigma point k of getCovarianceForPose (OccGridMapUtil.h:252-268) around a pose on the level's raster; 6 is the pose itself
__device__ __forceinline__ void ms_sigma_point(int k, float x, float y, float ang, float& e0, float& e1, float& e2) {
  e0 = k == 0 ? x + 1.5f : (k == 1 ? x - 1.5f : x);
  e1 = k == 2 ? y + 1.5f : (k == 3 ? y - 1.5f : y);
  e2 = k == 4 ? ang + 0.05f : (k == 5 ? ang - 0.05f : ang);
}

// state st of a job: its container and its pose on the level's raster
__device__ __forceinline__ void ms_state(const MsJob& J, int st, int2& en, float& e0, float& e1, float& e2) {
  float w0, w1, w2;
  int sigma = 6;
  if (J.mode == kMsLattice) {
    const int i = st % J.nx, j = (st / J.nx) % J.ny, k = st / (J.nx * J.ny);
    w0 = J.c0 + (float)(i - J.nx / 2) * J.d0;
    w1 = J.c1 + (float)(j - J.ny / 2) * J.d1;
    w2 = J.c2 + (float)(k - J.nt / 2) * J.d2;
    en = make_int2(J.first, J.n);
  } else {
    const int e = J.mode == kMsCov ? st / 7 : st;
    if (J.mode == kMsCov) sigma = st - 7 * e;
    w0 = J.poses[3 * (size_t)e]; w1 = J.poses[3 * (size_t)e + 1]; w2 = J.poses[3 * (size_t)e + 2];
    en = J.ent[e];
  }
  float x, y, ang;
  gn_level_begin(J.scale, J.t_x, J.t_y, w0, w1, w2, x, y, ang);
  ms_sigma_point(sigma, x, y, ang, e0, e1, e2);
}

// one point's term of getResidualForState (:369): 1 - interpMapValue(transform * p).  A point outside the map reads cell 0
// and is masked (value 0, :382-385), so no load sits behind a branch.  ORDERED: the ordered matcher's gn_prob (exp in double).
template <bool ORDERED>
__device__ __forceinline__ float ms_point(const float* __restrict__ lo, int sx, float lim_x, float lim_y, float s, float c, float e0,
                                          float e1, float px, float py) {
  const float cx = (c * px + (-s) * py) + e0;
  const float cy = (s * px + c * py) + e1;
  const bool in_map = !(cx < 0.0f || cx > lim_x || cy < 0.0f || cy > lim_y);  // pointOutOfMapBounds (:60-63)
  const int ix = in_map ? (int)cx : 0, iy = in_map ? (int)cy : 0;
  const int index = iy * sx + ix;
  float o[3];
  if (ORDERED) {
    gn_interp(gn_prob(lo, index), gn_prob(lo, index + 1), gn_prob(lo, index + sx), gn_prob(lo, index + sx + 1), cx - (float)ix,
              cy - (float)iy, in_map, o);
  } else {
    const float l0 = lo[index], l1 = lo[index + 1], l2 = lo[index + sx], l3 = lo[index + sx + 1];
    gn_interp(gn_prob_f(l0), gn_prob_f(l1), gn_prob_f(l2), gn_prob_f(l3), cx - (float)ix, cy - (float)iy, in_map, o);
  }
  return 1.0f - o[0];
}

// getLikelihoodForResidual (:349-355); an empty container: 0 / 0
__device__ __forceinline__ void ms_write(const MsJob& J, int st, float residual, int n) {
  if (J.out_res) J.out_res[st] = residual;
  J.out_lik[st] = 1.0f - (residual / (float)n);
}

constexpr int kMsWaves = 4;  // states per block

template <int CH>
__global__ void __launch_bounds__(64 * kMsWaves) __attribute__((amdgpu_waves_per_eu(4)))
k_ms_score(MsJob J, const float* __restrict__ pts) {
  const int lane = threadIdx.x & 63;
  const int st = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kMsWaves + (threadIdx.x >> 6)));
  if (st >= J.n_states) return;  // (whole waves: nothing below waits for another wave)
  int2 en;
  float e0, e1, e2;
  ms_state(J, st, en, e0, e1, e2);
  const int first = __builtin_amdgcn_readfirstlane(en.x), n = __builtin_amdgcn_readfirstlane(en.y);
  const float2* __restrict__ P = reinterpret_cast<const float2*>(pts) + first;
  const float* __restrict__ lo = in_device_memory(J.lo);
  const int sx = J.sx;
  const float lim_x = (float)J.sx - 2.0f, lim_y = (float)J.sy - 2.0f;  // MapDimensionProperties.h:66-70
  const float factor = J.factor;
  float s, c;
  sincosf(e2, &s, &c);
  float acc = 0.0f;
  for (int base = 0; base < n; base += 64 * CH) {  // (n is wave-uniform: no lane leaves the loop early)
    float px[CH], py[CH];
    bool have[CH];
#pragma unroll
    for (int j = 0; j < CH; j++) {
      const int i = base + 64 * j + lane;
      have[j] = i < n;
      float2 v = make_float2(0.0f, 0.0f);
      if (have[j]) v = P[i];
      px[j] = v.x * factor;
      py[j] = v.y * factor;
    }
#pragma unroll
    for (int j = 0; j < CH; j++) {
      const float f = ms_point<false>(lo, sx, lim_x, lim_y, s, c, e0, e1, px[j], py[j]);
      acc += have[j] ? f : 0.0f;
    }
  }
  const float residual = gn_wave_sum(acc);
  if (lane == 0) ms_write(J, st, residual, n);
}

constexpr int kMsOrderedChunk = 4096;  // terms in LDS at a time

__global__ void __launch_bounds__(256)
k_ms_score_ordered(MsJob J, const float* __restrict__ pts) {
  __shared__ float s_term[kMsOrderedChunk];
  const int tid = threadIdx.x, st = blockIdx.x;
  int2 en;
  float e0, e1, e2;
  ms_state(J, st, en, e0, e1, e2);
  const int n = en.y;
  const float2* __restrict__ P = reinterpret_cast<const float2*>(pts) + en.x;
  const float* __restrict__ lo = in_device_memory(J.lo);
  const float lim_x = (float)J.sx - 2.0f, lim_y = (float)J.sy - 2.0f;
  const float c = (float)cos((double)e2), s = (float)sin((double)e2);  // getTransformForState (:437-440)
  float residual = 0.0f;  // thread 0's
  for (int base = 0; base < n; base += kMsOrderedChunk) {
    const int m = min(kMsOrderedChunk, n - base);
    for (int i = tid; i < m; i += 256) {
      const float2 v = P[base + i];
      s_term[i] = ms_point<true>(lo, J.sx, lim_x, lim_y, s, c, e0, e1, v.x * J.factor, v.y * J.factor);
    }
    __syncthreads();
    if (tid == 0) {  // residual += funval, in container order (:366-371)
#pragma unroll 8
      for (int i = 0; i < m; i++) residual += s_term[i];
    }
    __syncthreads();
  }
  if (tid == 0) ms_write(J, st, residual, n);
}

// The lattice's best state: the highest likelihood, the lowest linear index among equals, NaN never; -1 / NaN when there
// is none.  One block: a thread walks its states in rising order, the waves and then the block meet pairwise.
__device__ __forceinline__ void ms_better(float v, int i, float& bv, int& bi) {
  if (i >= 0 && (bi < 0 || v > bv || (v == bv && i < bi))) { bv = v; bi = i; }
}
__global__ void __launch_bounds__(1024)
k_ms_best(const float* __restrict__ vol, int n, int* __restrict__ out_index, float* __restrict__ out_lik) {
  __shared__ float s_v[16];
  __shared__ int s_i[16];
  const int tid = threadIdx.x;
  float bv = 0.0f;
  int bi = -1;
  for (int i = tid; i < n; i += 1024) {
    const float v = vol[i];
    if (v == v) ms_better(v, i, bv, bi);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) ms_better(__shfl_xor(bv, d), __shfl_xor(bi, d), bv, bi);
  if ((tid & 63) == 0) { s_v[tid >> 6] = bv; s_i[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; w++) ms_better(s_v[w], s_i[w], bv, bi);
    if (out_index) *out_index = bi;
    if (out_lik) *out_lik = bi < 0 ? __int_as_float(0x7fc00000) : bv;
  }
}

// getCovarianceForPose's weighted mean and covariance (OccGridMapUtil.h:280-302) from an entry's seven likelihoods, then
// getCovMatrixWorldCoords (:314-339); one thread per entry.  The orders are Eigen's for these fixed sizes: the 7-term sum()
// in halves -- (l0 + (l1 + l2)) + ((l3 + l4) + (l5 + l6)) --, += coefficient by coefficient, the outer product d d^T first and
// the scalar weight in front of it.
__global__ void __launch_bounds__(256)
k_ms_cov(MsJob J, int n_entries, const float* __restrict__ lik /* [n_entries][7] */, float* __restrict__ cov_map,
         float* __restrict__ cov_world) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  float x, y, ang;
  gn_level_begin(J.scale, J.t_x, J.t_y, J.poses[3 * (size_t)e], J.poses[3 * (size_t)e + 1], J.poses[3 * (size_t)e + 2], x, y, ang);
  float sp[7][3], l[7];
#pragma unroll
  for (int k = 0; k < 7; k++) {
    ms_sigma_point(k, x, y, ang, sp[k][0], sp[k][1], sp[k][2]);
    l[k] = lik[7 * (size_t)e + k];
  }
  const float inv = 1.0f / ((l[0] + (l[1] + l[2])) + ((l[3] + l[4]) + (l[5] + l[6])));
  float mean[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 7; k++)
#pragma unroll
    for (int r = 0; r < 3; r++) mean[r] += sp[k][r] * l[k];
#pragma unroll
  for (int r = 0; r < 3; r++) mean[r] *= inv;
  float m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const float d[3] = {sp[k][0] - mean[0], sp[k][1] - mean[1], sp[k][2] - mean[2]};
    const float w = l[k] * inv;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int q = 0; q < 3; q++) m[3 * r + q] += w * (d[r] * d[q]);
  }
  if (cov_map)
    for (int q = 0; q < 9; q++) cov_map[9 * (size_t)e + q] = m[q];
  if (cov_world) {
    const float sc = J.cell_length, sq = sc * sc;
    float* w = cov_world + 9 * (size_t)e;
    w[0] = m[0] * sq; w[4] = m[4] * sq;
    w[3] = m[3] * sq; w[1] = w[3];
    w[6] = m[6] * sc; w[2] = w[6];
    w[7] = m[7] * sc; w[5] = w[7];
    w[8] = m[8];
  }
}


// ------------------------------------------------------------------------------------------
// STREAMED HectorSlamProcessor (lslam_hector_*): HectorSlamProcessor::update (H/slam_main/HectorSlamProcessor.h:81-108) for a
// recorded stretch of scans with the pose chain, the update decision and the update geometry kept on the device.  The
// host-driven loop pays three blocking round trips per scan (the projected count, the matched pose, then cosf / sinf /
// getMapCoordsPose / the begin cell of every level computed from that pose before the update can be enqueued); here a scan
// is [k_hector_project] -> k_hs_match_* -> k_hs_mark -> k_hs_apply on the context's one stream and the host waits once
// per call.  No hand-over words, no spinning kernel, no cooperative launch: stream order is the only ordering.
//   HsState        the processor's three state vectors and covariance, the live and the cached container's counts, the
//                  cached origo, this scan's decision and -- per level -- what update_impl fills into LevelGeom on the host
//   k_hs_match_*   gn_match_reg_body / gn_match_fast_body -- the one matcher lslam_map_match_data runs -- on a count and a
//                  start pose read from the device (same bits as lslam_map_match_data for the same container, start pose,
//                  map and LSLAM_GN_THREADS: tests/test_hector_stream_gpu.py holds it to that); its last phase, one
//                  thread, is the gate (H/util/UtilFunctions.h:72-91) and the geometry of every level
//   k_hs_mark / k_hs_apply   logodds_mark_wave / logodds_apply_wave (the two-kernel, non-deferred update) with geometry,
//                  point pointer and count read from HsState; all levels in one launch each (blockIdx.y = level), the grid
//                  sized for the capacity; a block returns at once when the scan does not update or its beams lie beyond
//                  the count
// Trigonometry of the geometry: the reference evaluates Eigen::Rotation2Df with the host libm.  A scan taken without
// matching has the host's hint as its pose, so the host sends cosf / sinf of it (bit for bit update_impl); a matched pose
// exists on the device only and gets (float)cos((double)theta), (float)sin((double)theta).
// ------------------------------------------------------------------------------------------
struct HsLevelGeom {
  float c, s, tx, ty;
  float ox, oy, factor;
  int bx, by;
  uint32_t epoch;
};
struct HsState {
  // ---- kHsPersistWords words that outlive a call (the host mirrors them: up at the start of a call, down at its end)
  float match_pose[3];    // lastScanMatchPose
  float cov[9];           // lastScanMatchCov
  float update_pose[3];   // lastMapUpdatePose
  int n_live;             // points of the live container (k_hector_project's count, or the caller's)
  int n_cached;           // MapRepMultiMap::dataContainers: size and origo of what the last matchData cached
  float cached_origo[2];
  int updated;            // this scan's decision
  // ---- per scan
  HsLevelGeom lv[kGnMaxLevels];
};
constexpr int kHsPersistWords = 20;
static_assert(offsetof(HsState, lv) == kHsPersistWords * 4, "HsState: the persistent words come first");

struct HsScan {           // what the host knows of one scan (kernel argument)
  float hint[3];          // poseHintWorld; unused when chain
  float hint_c, hint_s;   // host cosf / sinf of hint[2] (host_trig)
  int chain;              // start from HsState::match_pose (hector_slam.cc:200-204)
  int no_match;           // map_without_matching
  int host_trig;
  float origo[2];         // the live container's origo
  float min_dist, min_angle;
  int fabs_gate;
  int capacity;           // points the buffers behind `pts` / the cache hold per scan
  uint32_t epoch[kGnMaxLevels];
};

// util::poseDifferenceLargerThan (H/util/UtilFunctions.h:72-91) in fp32: norm() = sqrt(dx*dx + dy*dy); the heading
// difference wrapped once by +-2 pi in double (M_PI * 2.0f is a double product); then -- the form the reference's toolchain
// compiles -- the unqualified abs(int): the difference truncated toward zero.  fabs_gate: fabsf instead.
__device__ __forceinline__ bool hs_pose_difference_larger_than(const float* p, const float* q, float min_dist, float min_angle,
                                                               int fabs_gate) {
  const float dx = p[0] - q[0], dy = p[1] - q[1];
  if (sqrtf(dx * dx + dy * dy) > min_dist) return true;
  float ad = p[2] - q[2];
  const double pi = 3.14159265358979323846;
  if ((double)ad > pi) ad = (float)((double)ad - pi * 2.0);
  else if ((double)ad < -pi) ad = (float)((double)ad + pi * 2.0);
  if (fabs_gate) return fabsf(ad) > min_angle;
  return (float)abs((int)ad) > min_angle;
}

// last phase of a streamed match, ONE thread: state, record, gate, geometry (HectorSlamProcessor.h:98-107 + update_impl)
__device__ __forceinline__ void hs_finish(const GnLevels& lv, const HsScan& sc, HsState* st,
                                          lslam_hector_record* __restrict__ rec, const float* pose, const float* H, int n) {
  if (!sc.no_match) {
    if (n > 0)  // ScanMatcher.h:96: an empty container leaves covMatrix untouched
      for (int q = 0; q < 9; q++) st->cov[q] = H[q];
    st->n_cached = n;  // dataContainers[..].setFrom (MapRepMultiMap.h:161), also when empty
    st->cached_origo[0] = sc.origo[0];
    st->cached_origo[1] = sc.origo[1];
  }
  st->n_live = n;
  for (int q = 0; q < 3; q++) st->match_pose[q] = pose[q];
  const bool upd = hs_pose_difference_larger_than(pose, st->update_pose, sc.min_dist, sc.min_angle, sc.fabs_gate) || sc.no_match;
  st->updated = upd ? 1 : 0;
  if (upd) {
    for (int q = 0; q < 3; q++) st->update_pose[q] = pose[q];
    float c, s;
    if (sc.host_trig) { c = sc.hint_c; s = sc.hint_s; }
    else { c = (float)cos((double)pose[2]); s = (float)sin((double)pose[2]); }
    const float co0 = st->cached_origo[0], co1 = st->cached_origo[1];
    for (int L = 0; L < lv.n_levels; L++) {
      HsLevelGeom g;
      g.factor = L == 0 ? 1.0f : 1.0f / (float)(1 << L);  // DataPointContainer::setFrom factor (MapRepMultiMap.h:161)
      g.ox = L == 0 ? sc.origo[0] : co0 * g.factor;
      g.oy = L == 0 ? sc.origo[1] : co1 * g.factor;
      g.c = c; g.s = s;
      g.tx = (lv.scale[L] * pose[0] + 0.0f * pose[1]) + lv.t_x[L];  // getMapCoordsPose (GridMapBase.h:238-242)
      g.ty = (0.0f * pose[0] + lv.scale[L] * pose[1]) + lv.t_y[L];
      const float bxf = (c * g.ox + (-s) * g.oy) + g.tx;            // OccGridMapBase.h:132
      const float byf = (s * g.ox + c * g.oy) + g.ty;
      g.bx = (int)(bxf + 0.5f);                                     // :135
      g.by = (int)(byf + 0.5f);
      g.epoch = sc.epoch[L];
      st->lv[L] = g;
    }
  }
  if (rec) {
    for (int q = 0; q < 3; q++) rec->pose[q] = pose[q];
    for (int q = 0; q < 9; q++) rec->cov[q] = st->cov[q];
    rec->updated = upd ? 1 : 0;
    rec->n_points = n;
    rec->pad[0] = rec->pad[1] = 0;
  }
}

// count (clamped to the capacity before any indexing) and start pose of a streamed scan, read by every thread (ranges form:
// n_src points INTO the state block, which is therefore nowhere __restrict__ in these kernels); the barrier
// keeps the one thread that rewrites them in hs_finish behind every reader, also on the paths that run no iteration
__device__ __forceinline__ int hs_begin(const HsScan& sc, const int* n_src, const HsState* st, float* b) {
  int n = *n_src;
  n = n < 0 ? 0 : (n > sc.capacity ? sc.capacity : n);
  for (int q = 0; q < 3; q++) b[q] = sc.chain ? st->match_pose[q] : sc.hint[q];
  __syncthreads();
  return n;
}

// one streamed scan in either form of the matcher: k_hs_match_* take its arguments from the launch, k_hf_match_* from their
// member's entries of the fleet's tables
template <int NT, int PMAX>
__device__ __forceinline__ void hs_scan_reg(const GnLevels& lv, const HsScan& sc, const float* __restrict__ pts, const int* n_src,
                                            float* __restrict__ cache_dst, HsState* st, lslam_hector_record* __restrict__ rec) {
  float b[3], pose[3], H[9];
  const int n = hs_begin(sc, n_src, st, b);
  if (sc.no_match) { pose[0] = b[0]; pose[1] = b[1]; pose[2] = b[2]; }
  else gn_match_reg_body<NT, PMAX>(lv, pts, cache_dst, n, b[0], b[1], b[2], pose, H);
  if (threadIdx.x == 0) hs_finish(lv, sc, st, rec, pose, H, n);
}

template <int NT>
__device__ __forceinline__ void hs_scan_fast(const GnLevels& lv, const HsScan& sc, const float* __restrict__ pts, const int* n_src,
                                             float* __restrict__ cache_dst, int pts_in_lds, HsState* st,
                                             lslam_hector_record* __restrict__ rec) {
  float b[3], pose[3], H[9];
  const int n = hs_begin(sc, n_src, st, b);
  if (sc.no_match) { pose[0] = b[0]; pose[1] = b[1]; pose[2] = b[2]; }
  else gn_match_fast_body<NT>(lv, pts, cache_dst, n, pts_in_lds, b[0], b[1], b[2], pose, H);
  if (threadIdx.x == 0) hs_finish(lv, sc, st, rec, pose, H, n);
}

template <int NT, int PMAX>
__global__ void __launch_bounds__(NT)
k_hs_match_reg(GnLevels lv, HsScan sc, const float* __restrict__ pts, const int* n_src, float* __restrict__ cache_dst,
               HsState* st, lslam_hector_record* __restrict__ rec) {
  hs_scan_reg<NT, PMAX>(lv, sc, pts, n_src, cache_dst, st, rec);
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_hs_match_fast(GnLevels lv, HsScan sc, const float* __restrict__ pts, const int* n_src, float* __restrict__ cache_dst,
                int pts_in_lds, HsState* st, lslam_hector_record* __restrict__ rec) {
  hs_scan_fast<NT>(lv, sc, pts, n_src, cache_dst, pts_in_lds, st, rec);
}

struct HsLevels {  // what does not change from scan to scan
  int n_levels;
  int sx[kGnMaxLevels], sy[kGnMaxLevels];
  float lo_free, lo_occ;
  uint32_t* free_key[kGnMaxLevels];
  uint32_t* occ_key[kGnMaxLevels];
  float* logodds[kGnMaxLevels];
};

__device__ __forceinline__ LevelGeom hs_level_geom(const HsLevels& lv, const HsState* __restrict__ st, int L) {
  const HsLevelGeom h = st->lv[L];
  LevelGeom g;
  g.sx = lv.sx[L]; g.sy = lv.sy[L];
  g.c = h.c; g.s = h.s; g.tx = h.tx; g.ty = h.ty;
  g.factor = h.factor;
  g.ox = h.ox; g.oy = h.oy;
  g.lo_free = lv.lo_free; g.lo_occ = lv.lo_occ;
  g.epoch = h.epoch;
  g.just_once = 0;
  g.bx = h.bx; g.by = h.by;
  g.metres_per_cell = 0.0;
  return g;
}

// level 0 takes the live container, level i > 0 what the last matchData cached (MapRepMultiMap.h:174-191)
__device__ __forceinline__ void hs_mark_block(const HsLevels& lv, const HsState* __restrict__ st, const float* __restrict__ pts_live,
                                              const float* __restrict__ pts_cached, int L) {
  if (!st->updated) return;
  const int n = L == 0 ? st->n_live : st->n_cached;
  const int wave = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (wave >= n) return;
  logodds_mark_wave(hs_level_geom(lv, st, L), L == 0 ? pts_live : pts_cached, n, wave, threadIdx.x & 63,
                    in_device_memory(lv.free_key[L]), in_device_memory(lv.occ_key[L]), nullptr);
}

__device__ __forceinline__ void hs_apply_block(const HsLevels& lv, const HsState* __restrict__ st, const float* __restrict__ pts_live,
                                               const float* __restrict__ pts_cached, int L) {
  if (!st->updated) return;
  const int n = L == 0 ? st->n_live : st->n_cached;
  const int wave = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (wave >= n) return;
  logodds_apply_wave(hs_level_geom(lv, st, L), L == 0 ? pts_live : pts_cached, n, wave, threadIdx.x & 63,
                     in_device_memory(lv.free_key[L]), in_device_memory(lv.occ_key[L]), in_device_memory(lv.logodds[L]));
}

__global__ void __launch_bounds__(256)
k_hs_mark(HsLevels lv, const HsState* __restrict__ st, const float* __restrict__ pts_live, const float* __restrict__ pts_cached) {
  hs_mark_block(lv, st, pts_live, pts_cached, (int)blockIdx.y);
}

__global__ void __launch_bounds__(256)
k_hs_apply(HsLevels lv, const HsState* __restrict__ st, const float* __restrict__ pts_live, const float* __restrict__ pts_cached) {
  hs_apply_block(lv, st, pts_live, pts_cached, (int)blockIdx.y);
}

// ------------------------------------------------------------------------------------------
// GATED streamed chain (lslam_hector_process_many_clouds[_dev], lslam_hector_process_many_synced): whether a scan is taken is
// decided on the device -- lslam_msync_record::status, written by k_msync_walk earlier in the same stream -- so the chain
// k_hg_cloud_container -> k_hg_match_* -> k_hs_mark -> k_hs_apply reads a TAKE word from HBM first: the scan is taken iff
// *take > 0 (LSLAM_MSYNC_CORRECTED is 1, QUEUED 0, every refusal negative); take == nullptr takes every scan.  The host
// hands each launch the address of its scan's word (take + k * stride), so a status field inside an array of records serves
// as it stands.  The arithmetic is hector_compact / hector_cloud_point and hs_scan_*: a taken scan's bits are those of the
// ungated chain.  A scan that is not taken:
//   k_hg_cloud_container   returns before its first store: the live container and its count stay the last taken scan's
//   k_hg_match_*           returns before hs_begin's barrier (the word is uniform over the block); one thread writes the
//                          record of a scan that was not taken (all zero, n_points = -1) and st->updated = 0 -- WITHOUT
//                          that store the state block still holds the previous scan's decision, and
//   k_hs_mark / k_hs_apply (unchanged) would apply the previous scan's update a second time; with it they return at once
// So a refused scan costs four launches of blocks that load one word and leave, and changes nothing of the processor: it is
// NOT a scan with an empty container, which would reset n_live / n_cached and the cached origo (hs_finish).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool hg_taken(const int32_t* take) { return !take || *take > 0; }

// ONE thread: what a scan that was not taken leaves behind
__device__ __forceinline__ void hg_skip(HsState* st, lslam_hector_record* __restrict__ rec) {
  st->updated = 0;
  if (rec) {
    for (int q = 0; q < 3; q++) rec->pose[q] = 0.0f;
    for (int q = 0; q < 9; q++) rec->cov[q] = 0.0f;
    rec->updated = 0;
    rec->n_points = -1;
    rec->pad[0] = rec->pad[1] = 0;
  }
}

// k_hector_cloud_container behind the take word; valid == nullptr: every point is valid
__global__ void __launch_bounds__(1024)
k_hg_cloud_container(ProjectCfg c, const int32_t* __restrict__ take, const float* __restrict__ xyz,
                     const uint8_t* __restrict__ valid, float* __restrict__ out_xy, int* __restrict__ out_n) {
  if (!hg_taken(take)) return;
  hector_compact(c.n, out_xy, out_n, [&](int i, float& ox, float& oy) {
    if (valid && !valid[i]) return false;
    return hector_cloud_point(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ox, oy);
  });
}

template <int NT, int PMAX>
__global__ void __launch_bounds__(NT)
k_hg_match_reg(GnLevels lv, HsScan sc, const int32_t* __restrict__ take, const float* __restrict__ pts, const int* n_src,
               float* __restrict__ cache_dst, HsState* st, lslam_hector_record* __restrict__ rec) {
  if (!hg_taken(take)) {
    if (threadIdx.x == 0) hg_skip(st, rec);
    return;
  }
  hs_scan_reg<NT, PMAX>(lv, sc, pts, n_src, cache_dst, st, rec);
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_hg_match_fast(GnLevels lv, HsScan sc, const int32_t* __restrict__ take, const float* __restrict__ pts, const int* n_src,
                float* __restrict__ cache_dst, int pts_in_lds, HsState* st, lslam_hector_record* __restrict__ rec) {
  if (!hg_taken(take)) {
    if (threadIdx.x == 0) hg_skip(st, rec);
    return;
  }
  hs_scan_fast<NT>(lv, sc, pts, n_src, cache_dst, pts_in_lds, st, rec);
}

// ------------------------------------------------------------------------------------------
// HECTOR FLEET (lslam_hector_fleet_*): R streamed processors, each on its own map, advance one scan each per STEP, and a step
// is the chain of ONE processor -- [k_hf_project] -> k_hf_match_* -> k_hf_mark -> k_hf_apply -- whatever R is.  The members
// are independent SLAM sessions, so nothing orders one against another inside a launch; within a member, stream order is
// the only ordering, exactly as in the single processor's chain.  Every kernel finds its member in the grid (one matcher
// or projection block per member: blockIdx.x; mark / apply: blockIdx.z) and reads two tables by that index:
//   HfMember[R]          what does not change during a call: the pyramid as the matcher and as the update take it, the
//                        projection's configuration, the member's state block and its cached and resident containers
//   HfScan[step][R]      what the host knows of one (step, member): the HsScan the single kernels take as an argument, whether
//                        the member takes part in the step, where its live container, its count and its record are
// The index is uniform over a block, so the tables' words arrive through the scalar cache like kernel arguments do.  The
// arithmetic is hs_scan_* / hs_mark_block / hs_apply_block / hector_project_body: a member's bits are those of its own
// lslam_hector_* call.  A member that sits a step out returns before hs_begin's barrier and before any state is read: its
// state block still holds the `updated` of its last scan.  Members may differ in size and depth: the mark / apply grid
// covers the deepest pyramid and the longest container, and a block beyond its member's levels returns at once.
// ------------------------------------------------------------------------------------------
struct HfMember {
  GnLevels gn;
  HsLevels ul;
  ProjectCfg pc;
  HsState* st;
  float* cached;    // the map's MapRepMultiMap::dataContainers buffer
  float* resident;  // the map's lslam_map_set_scan container: the live container of the ranges form
};
struct HfScan {
  HsScan sc;
  int active;
  const float* pts;     // live container: HfMember::resident, or this scan's points of the call
  const int* n_src;     // its count: &st->n_live, or the call's
  const float* ranges;  // ranges form: this scan's readings
  lslam_hector_record* rec;
  // gated cloud form (k_hfg_*): the scan is taken iff active and (take == nullptr or *take > 0)
  const int32_t* take;
  const float* xyz;
  const uint8_t* valid;  // nullptr: every point is valid
};

// Entry i of a table the host wrote before the launch and no kernel writes: read through the constant address space, so that
// -- i being uniform over the block -- its words come through the scalar cache into scalar registers wherever the kernel
// reads them, also behind its own stores (a plain global load behind a store is a vector load: k_hf_match_fast<256> then
// needs 66 VGPRs where k_hs_match_fast<256> has 62, and drops from 8 waves per SIMD to 7).
template <class T>
__device__ __forceinline__ const T& hf_entry(const T* table, unsigned i) {
  typedef const T __attribute__((address_space(4))) * ConstPtr;
  return *(const T*)(ConstPtr)(uintptr_t)(table + i);  // (by way of the integer, as in_device_memory)
}

__global__ void __launch_bounds__(1024)
k_hf_project(const HfMember* __restrict__ mem, const HfScan* __restrict__ step, const double2* __restrict__ cossin) {
  const HfScan& d = hf_entry(step, blockIdx.x);
  if (!d.active) return;
  const HfMember& m = hf_entry(mem, blockIdx.x);
  hector_project_body(m.pc, in_device_memory(d.ranges), cossin, in_device_memory(m.resident), &in_device_memory(m.st)->n_live);
}

template <int NT, int PMAX>
__global__ void __launch_bounds__(NT)
k_hf_match_reg(const HfMember* __restrict__ mem, const HfScan* __restrict__ step) {
  const HfScan& d = hf_entry(step, blockIdx.x);
  if (!d.active) return;
  const HfMember& m = hf_entry(mem, blockIdx.x);
  hs_scan_reg<NT, PMAX>(m.gn, d.sc, in_device_memory(d.pts), in_device_memory(d.n_src), in_device_memory(m.cached), in_device_memory(m.st), in_device_memory(d.rec));
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_hf_match_fast(const HfMember* __restrict__ mem, const HfScan* __restrict__ step, int pts_in_lds) {
  const HfScan& d = hf_entry(step, blockIdx.x);
  if (!d.active) return;
  const HfMember& m = hf_entry(mem, blockIdx.x);
  hs_scan_fast<NT>(m.gn, d.sc, in_device_memory(d.pts), in_device_memory(d.n_src), in_device_memory(m.cached), pts_in_lds, in_device_memory(m.st), in_device_memory(d.rec));
}

__global__ void __launch_bounds__(256)
k_hf_mark(const HfMember* __restrict__ mem, const HfScan* __restrict__ step) {
  const HfScan& d = hf_entry(step, blockIdx.z);
  if (!d.active) return;
  const HfMember& m = hf_entry(mem, blockIdx.z);
  const int L = (int)blockIdx.y;
  if (L >= m.ul.n_levels) return;
  hs_mark_block(m.ul, in_device_memory(m.st), in_device_memory(d.pts), in_device_memory(m.cached), L);
}

__global__ void __launch_bounds__(256)
k_hf_apply(const HfMember* __restrict__ mem, const HfScan* __restrict__ step) {
  const HfScan& d = hf_entry(step, blockIdx.z);
  if (!d.active) return;
  const HfMember& m = hf_entry(mem, blockIdx.z);
  const int L = (int)blockIdx.y;
  if (L >= m.ul.n_levels) return;
  hs_apply_block(m.ul, in_device_memory(m.st), in_device_memory(d.pts), in_device_memory(m.cached), L);
}

// ------------------------------------------------------------------------------------------
// GATED FLEET chain (lslam_hector_fleet_process_many_clouds[_dev], lslam_hector_fleet_process_many_synced): the gated chain
// above with the member found in the grid.  Entry (step, member) is taken iff the host's `active` is non-zero AND its device
// take word says so (HfScan::take null: `active` alone decides) -- the word of a synced call is the status the fleet's walk
// wrote earlier in the same stream.  k_hfg_cloud_container -> k_hfg_match_* -> k_hf_mark -> k_hf_apply; the last two are the
// ungated fleet's: an entry that is active but refused on the device has its `updated` cleared by k_hfg_match_* (hg_skip), so
// hs_mark_block / hs_apply_block return at once, and an entry that is not active returns on `active` as it always did.  The
// two traps of the single gated chain hold here as well: a skipped match MUST clear `updated`, and a scan that is not taken is
// NOT an empty container.  A host-inactive entry's record is the host's to write, as in the ungated fleet.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool hfg_word_taken(const int32_t* take) { return hg_taken(in_device_memory(take)); }
__device__ __forceinline__ bool hfg_taken(const HfScan& d) { return d.active && hfg_word_taken(d.take); }

__global__ void __launch_bounds__(1024)
k_hfg_cloud_container(const HfMember* __restrict__ mem, const HfScan* __restrict__ step) {
  const HfScan& d = hf_entry(step, blockIdx.x);
  if (!hfg_taken(d)) return;
  const HfMember& m = hf_entry(mem, blockIdx.x);
  const ProjectCfg& c = m.pc;
  const float* __restrict__ xyz = in_device_memory(d.xyz);
  const uint8_t* __restrict__ valid = in_device_memory(d.valid);
  hector_compact(c.n, in_device_memory(m.resident), &in_device_memory(m.st)->n_live, [&](int i, float& ox, float& oy) {
    if (valid && !valid[i]) return false;
    return hector_cloud_point(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ox, oy);
  });
}

template <int NT, int PMAX>
__global__ void __launch_bounds__(NT)
k_hfg_match_reg(const HfMember* __restrict__ mem, const HfScan* __restrict__ step) {
  const HfScan& d = hf_entry(step, blockIdx.x);
  if (!d.active) return;
  const HfMember& m = hf_entry(mem, blockIdx.x);
  if (!hfg_word_taken(d.take)) {
    if (threadIdx.x == 0) hg_skip(in_device_memory(m.st), in_device_memory(d.rec));
    return;
  }
  hs_scan_reg<NT, PMAX>(m.gn, d.sc, in_device_memory(d.pts), in_device_memory(d.n_src), in_device_memory(m.cached), in_device_memory(m.st), in_device_memory(d.rec));
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_hfg_match_fast(const HfMember* __restrict__ mem, const HfScan* __restrict__ step, int pts_in_lds) {
  const HfScan& d = hf_entry(step, blockIdx.x);
  if (!d.active) return;
  const HfMember& m = hf_entry(mem, blockIdx.x);
  if (!hfg_word_taken(d.take)) {
    if (threadIdx.x == 0) hg_skip(in_device_memory(m.st), in_device_memory(d.rec));
    return;
  }
  hs_scan_fast<NT>(m.gn, d.sc, in_device_memory(d.pts), in_device_memory(d.n_src), in_device_memory(m.cached), pts_in_lds, in_device_memory(m.st), in_device_memory(d.rec));
}

float prob_to_logodds(float prob) {  // H/map/GridMapLogOdds.h:151-155 (log() is the double overload)
  float odds = prob / (1.0f - prob);
  return (float)log((double)odds);
}

struct Level {
  int sx = 0, sy = 0;
  float cell_length = 0.f, scale_to_map = 0.f, t_x = 0.f, t_y = 0.f;
  float* d_logodds = nullptr;
  uint32_t* d_free = nullptr;
  uint32_t* d_occ = nullptr;
  uint32_t epoch = 0;
  // pipelined single-scan path: second key-plane set (scans alternate), the points of the scan whose apply is pending
  uint32_t* d_free2 = nullptr;
  uint32_t* d_occ2 = nullptr;
  DevBuf<float> pipe_pts[2];
  bool pending = false;  // marks of scan `pend_g.epoch` are in plane set (epoch & 1); its apply has not been launched
  LevelGeom pend_g;
  int pend_n = 0;
  // batched update (k_lo_batch_*): a pool of 64-byte tile slots holding one window of tiles per scan of a round,
  // allocated on first use and grown on demand (never beyond the scratch budget unless ONE scan's window needs more)
  DevBuf<uint8_t> d_pool;       // [pool_slots][64]
  size_t pool_slots = 0;        // tile slots the epoch bookkeeping below covers (= d_pool.cap / 64 at the last clear)
  uint8_t* d_flags = nullptr;   // [n_tiles][64]: tile touched by the scan in slot s of the round
  int tiles_x = 0, n_tiles = 0;
  uint32_t batch_epoch = 0;     // 6-bit round epoch in the pool / flag bytes
};

}  // namespace

struct lslam_map {
  lslam_context* ctx = nullptr;
  std::vector<Level> levels;
  float off_x = 0.f, off_y = 0.f;
  float lo_free = 0.f, lo_occ = 0.f;
  DevBuf<float> d_pts;
  // MapRepMultiMap::dataContainers (H/slam_main/MapRepMultiMap.h:161,186,220): the points + origo of the LAST
  // matchData call; updateByScan feeds the levels above 0 from these, whatever container it is handed
  DevBuf<float> d_cached;
  int n_cached = 0;
  float cached_origo[2] = {0.f, 0.f};
  DevBuf<float> d_gn_out;
  // lslam_map_match_batch*: the entry table (first point, points), and -- host form -- the start poses in, 12 floats per entry out
  DevBuf<int2> d_gnb_ent;
  DevBuf<float> d_gnb_io;
  // lslam_map_score_* / lslam_map_pose_covariance_batch, host forms: poses in, residuals / likelihoods / covariances / the
  // lattice's volume out (the entry table is d_gnb_ent)
  DevBuf<float> d_score_io;
  int score_chunk = 4;        // LSLAM_SCORE_CHUNK = 2 | 4 | 8: points per lane in flight in k_ms_score (results do not depend on it)
  // matchData, parallel-sum kernel (the default): the container goes up through pinned memory and is read -- and cached in
  // d_cached -- by the kernel itself; its 12 result floats land in pinned memory.  ordered_sums: k_gn_match instead.
  // batched update: scratch budget of the tile-slot pools of ONE level (bytes), rounds used by the last call, cells
  // found outside their scan's window (device counter; must stay 0: see lslam_map_batch_stats)
  size_t batch_budget = (size_t)192 << 20;
  int batch_radius_hint = 0;   // LSLAM_MAP_OPT_BATCH_RADIUS_CELLS: bound for callers whose points the host never sees
  int batch_last_rounds = 0;
  unsigned long long* d_batch_misses = nullptr;  // PINNED HOST memory (device-visible): the kernels' atomicAdd lands where the
                                                 // host can read it after any synchronise, without a copy on the stream
  unsigned long long batch_misses_reported = 0;  // of those, how many a synchronise has already reported as an error
  bool ordered_sums = false;  // lslam_map_set_option(LSLAM_MAP_OPT_ORDERED_SUMS) / LSLAM_GN_ORDERED=1
  int gn_threads = 512;       // LSLAM_GN_THREADS = 256 | 512 | 1024
  float* h_gn_pts = nullptr;
  size_t h_gn_cap = 0;        // floats
  float* h_gn_out = nullptr;  // 12 floats + the ticket word [15] the kernel posts behind them
  int gn_ticket = 0;
  // h_gn_pts[0 .. 2 * gn_host_n) is a host copy of what d_cached holds (the last matchData's container, fed from the
  // host): updateByScan with the SAME points -- HectorSlamProcessor::update always updates with the container it has just
  // matched (HectorSlamProcessor.h:91-105) -- finds them already resident and skips its own staging copy
  int gn_host_n = -1;
  // resident container of lslam_map_set_scan (device-side LaserScan -> DataContainer)
  DevBuf<float> d_scan;         // projected points, then one int: their count
  DevBuf<float> d_scan_ranges;
  DevBuf<double2> d_cossin;     // laser_geometry's co_sine_map_, host-built, cached per scan geometry
  float cs_angle_min = 0.f, cs_angle_inc = 0.f;
  int cs_n = 0;
  int n_scan = 0;
  float scan_origo[2] = {0.f, 0.f};
  DevBuf<uint32_t> d_hash;      // [3][K][slots]: key, first hit beam, first crossing beam
  DevBuf<ScanHdr> d_hdr;
  DevBuf<int8_t> d_i8;
  bool force_two_kernels = false;  // LSLAM_MAP_TWO_KERNELS=1: mark + apply per call, nothing deferred (A/B measurements, tests)
  // host -> device staging of the per-scan points: a ring of pinned slots, so updateByScan only enqueues
  // (copy + two kernels per level) and returns; a slot is reused when its copy has completed
  static constexpr int kStageSlots = 8;
  float* h_stage = nullptr;
  size_t stage_cap = 0;  // floats per slot
  hipEvent_t stage_ev[kStageSlots] = {};
  bool stage_busy[kStageSlots] = {};
  unsigned stage_next = 0;
};

namespace {

int clear_marks(lslam_map* map, Level& L) {
  lslam_context* ctx = map->ctx;
  size_t n = (size_t)L.sx * L.sy;
  LSLAM_HIP(ctx, hipMemsetAsync(L.d_free, 0, n * sizeof(uint32_t), ctx->stream));
  LSLAM_HIP(ctx, hipMemsetAsync(L.d_occ, 0, n * sizeof(uint32_t), ctx->stream));
  if (L.d_free2) {
    LSLAM_HIP(ctx, hipMemsetAsync(L.d_free2, 0, n * sizeof(uint32_t), ctx->stream));
    LSLAM_HIP(ctx, hipMemsetAsync(L.d_occ2, 0, n * sizeof(uint32_t), ctx->stream));
  }
  L.epoch = 0;
  return LSLAM_OK;
}

// blocks of one job of k_logodds_pipe_ml: four beams per block, a multiple of 8 (the kernel's XCD-sector mapping)
inline int pipe_blocks(int n) { return ((n + 3) / 4 + 7) / 8 * 8; }

// apply job of level L's pending scan
PipeJob apply_job(Level& L, int first_block) {
  const int set = (int)(L.pend_g.epoch & 1u);
  PipeJob j{};
  j.g = L.pend_g;
  j.pts = L.pipe_pts[set].p;
  j.n = L.pend_n;
  j.first_block = first_block;
  j.apply = 1;
  j.free_r = set ? L.d_free2 : L.d_free;
  j.occ_r = set ? L.d_occ2 : L.d_occ;
  j.logodds = L.d_logodds;
  return j;
}

// the deferred apply of the pipelined path, as a launch of its own: every reader of the float planes calls this first.
// ONE launch for all levels with a pending scan (k_logodds_pipe_ml); a pyramid deeper than the job table: per level.
int flush_pending(lslam_map* map) {
  lslam_context* ctx = map->ctx;
  PipeJobs J{};
  int blocks = 0;
  for (auto& L : map->levels) {
    if (!L.pending) continue;
    if (J.n_jobs == kPipeMaxJobs) {
      launch(ctx, "logodds_apply", k_logodds_pipe_ml, dim3(blocks), dim3(256), 0, J);
      J = PipeJobs{};
      blocks = 0;
    }
    J.j[J.n_jobs++] = apply_job(L, blocks);
    blocks += pipe_blocks(L.pend_n);
    L.pending = false;
  }
  if (blocks > 0) launch(ctx, "logodds_apply", k_logodds_pipe_ml, dim3(blocks), dim3(256), 0, J);
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}

int update_impl(lslam_map* map, const float* d_pts, int n, const float* origo, const float pose[3],
                int just_once, float begin_x, float begin_y, double metres_per_cell) {
  lslam_context* ctx = map->ctx;
  if (n > kMaxBeams || (!just_once && map->levels.size() > 1 && map->n_cached > kMaxBeams))
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per scan are supported (got %d)", kMaxBeams, n);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const bool pipelined = !just_once && !map->force_two_kernels;
  if (!pipelined) {
    int rc = flush_pending(map);
    if (rc) return rc;
  }
  const int n_levels = just_once ? 1 : (int)map->levels.size();
  const float* const d_pts0 = d_pts;
  const int n0 = n;
  const float origo0[2] = {origo[0], origo[1]};
  // ---- phase 1 (pipelined path): everything that can FAIL -- the second key-plane set, the point buffers of the set this
  // scan will use, the mark reset when an epoch wraps -- for every level, before any epoch is bumped: an error return
  // leaves every level's (epoch, pending) pair as it was
  if (pipelined) {
    for (int li = 0; li < n_levels; li++) {
      Level& L = map->levels[li];
      if (L.epoch >= kMaxEpoch) {
        int rc = flush_pending(map);  // the pending scan's keys are about to be cleared
        if (rc == LSLAM_OK) rc = clear_marks(map, L);
        if (rc) return rc;
      }
      const size_t cells = (size_t)L.sx * L.sy;
      if (!L.d_free2) {  // second key-plane set, on first use of the pipelined path
        if (hipMalloc((void**)&L.d_free2, cells * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void**)&L.d_occ2, cells * sizeof(uint32_t)) != hipSuccess) {
          (void)hipGetLastError();
          if (L.d_free2) (void)hipFree(L.d_free2);
          L.d_free2 = L.d_occ2 = nullptr;
          return ctx->fail(LSLAM_ERR_HIP, "cannot allocate the second key planes of map level %d", li);
        }
        LSLAM_HIP(ctx, hipMemsetAsync(L.d_free2, 0, cells * sizeof(uint32_t), ctx->stream));
        LSLAM_HIP(ctx, hipMemsetAsync(L.d_occ2, 0, cells * sizeof(uint32_t), ctx->stream));
      }
      const int n_li = li == 0 ? n0 : map->n_cached;
      const int set = (int)((L.epoch + 1u) & 1u);
      LSLAM_HIP(ctx, L.pipe_pts[set].reserve((size_t)2 * std::max(n_li, 1)));  // nothing in flight reads THIS set's points
    }
  }
  PipeJobs J{};
  int blocks = 0;
  auto submit = [&]() {
    if (blocks > 0) launch(ctx, "logodds_pipe", k_logodds_pipe_ml, dim3(blocks), dim3(256), 0, J);
    J = PipeJobs{};
    blocks = 0;
  };
  for (int li = 0; li < n_levels; li++) {
    Level& L = map->levels[li];
    // level 0 takes the container it is handed, level i > 0 takes dataContainers[i-1] = what the last matchData
    // cached (H/slam_main/MapRepMultiMap.h:174-191) -- empty until the first matchData
    d_pts = li == 0 ? d_pts0 : map->d_cached.p;
    n = li == 0 ? n0 : map->n_cached;
    origo = li == 0 ? origo0 : map->cached_origo;
    if (!pipelined && L.epoch >= kMaxEpoch) {
      int rc = clear_marks(map, L);  // (nothing is pending on this path)
      if (rc) return rc;
    }
    L.epoch++;
    LevelGeom g;
    g.sx = L.sx; g.sy = L.sy;
    g.lo_free = map->lo_free; g.lo_occ = map->lo_occ;
    g.epoch = L.epoch;
    g.just_once = just_once;
    g.metres_per_cell = metres_per_cell;
    // DataPointContainer::setFrom factor (H/slam_main/MapRepMultiMap.h:161)
    g.factor = li == 0 ? 1.0f : (float)(1.0 / pow(2.0, (double)li));
    float ox = li == 0 ? origo[0] : origo[0] * g.factor;
    float oy = li == 0 ? origo[1] : origo[1] * g.factor;
    g.ox = ox; g.oy = oy;
    float mx, my, ang;
    if (just_once) {
      mx = begin_x; my = begin_y; ang = 0.0f;  // mapPose(800, 800, 0) (H/map/OccGridMapBase.h:182)
    } else {
      // getMapCoordsPose (H/map/GridMapBase.h:238-242), mapTworld = Scale*Translate (:278)
      float s = L.scale_to_map;
      mx = (s * pose[0] + 0.0f * pose[1]) + L.t_x;
      my = (0.0f * pose[0] + s * pose[1]) + L.t_y;
      ang = pose[2];
    }
    // host libm, exactly what the reference's Eigen::Rotation2Df evaluates
    g.c = cosf(ang);
    g.s = sinf(ang);
    g.tx = mx; g.ty = my;
    float bxf = (g.c * ox + (-g.s) * oy) + mx;  // :132
    float byf = (g.s * ox + g.c * oy) + my;
    g.bx = (int)(bxf + 0.5f);                   // :135
    g.by = (int)(byf + 0.5f);
    if (pipelined) {
      // [apply of this level's pending scan | mark of this one], the jobs of ALL levels in one launch
      const int set = (int)(L.epoch & 1u);
      if (J.n_jobs + 2 > kPipeMaxJobs) submit();
      if (L.pending) {
        J.j[J.n_jobs++] = apply_job(L, blocks);
        blocks += pipe_blocks(L.pend_n);
      }
      if (n > 0) {
        PipeJob j{};
        j.g = g;
        j.pts = d_pts;
        j.n = n;
        j.first_block = blocks;
        j.apply = 0;
        j.free_w = set ? L.d_free2 : L.d_free;
        j.occ_w = set ? L.d_occ2 : L.d_occ;
        j.pts_copy = L.pipe_pts[set].p;
        J.j[J.n_jobs++] = j;
        blocks += pipe_blocks(n);
      }
      L.pending = n > 0;
      L.pend_g = g;
      L.pend_n = n;
    } else if (n > 0) {
      dim3 grid((n + 3) / 4), block(256);  // 4 waves per block, one wave per beam
      launch(ctx, "logodds_mark", k_logodds_mark, grid, block, 0, g, d_pts, n, L.d_free, L.d_occ);
      launch(ctx, "logodds_apply", k_logodds_apply, grid, block, 0, g, d_pts, n, (const uint32_t*)L.d_free,
             (const uint32_t*)L.d_occ, L.d_logodds);
    }
  }
  if (pipelined) submit();
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}

}  // namespace

extern "C" {

int lslam_map_create(lslam_context* ctx, int size_x, int size_y, float cell_length, float offset_x,
                     float offset_y, int levels, lslam_map** out) {
  if (!ctx || !out || size_x <= 0 || size_y <= 0 || !(cell_length > 0.f) || levels < 1 || levels > 16)
    return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(LSLAM_ERR_HIP, "hipSetDevice failed");
  lslam_map* map = new lslam_map();
  map->ctx = ctx;
  map->off_x = offset_x;
  map->off_y = offset_y;
  map->lo_free = prob_to_logodds(0.4f);  // GridMapLogOddsFunctions ctor (H/map/GridMapLogOdds.h:98-102)
  map->lo_occ = prob_to_logodds(0.6f);
  int sx = size_x, sy = size_y;
  float cl = cell_length;
  for (int i = 0; i < levels; i++) {
    if (sx <= 0 || sy <= 0) break;
    Level L;
    L.sx = sx; L.sy = sy;
    L.cell_length = cl;
    L.scale_to_map = 1.0f / cl;            // H/map/GridMapBase.h:276
    L.t_x = L.scale_to_map * offset_x;     // Scale * Translate (:278)
    L.t_y = L.scale_to_map * offset_y;
    size_t n = (size_t)sx * sy;
    if (hipMalloc((void**)&L.d_logodds, n * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&L.d_free, n * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void**)&L.d_occ, n * sizeof(uint32_t)) != hipSuccess) {
      map->levels.push_back(std::move(L));
      lslam_map_destroy(map);
      return ctx->fail(LSLAM_ERR_HIP, "cannot allocate map level %d (%dx%d) in HBM", i, sx, sy);
    }
    (void)hipMemsetAsync(L.d_logodds, 0, n * sizeof(float), ctx->stream);
    (void)hipMemsetAsync(L.d_free, 0, n * sizeof(uint32_t), ctx->stream);
    (void)hipMemsetAsync(L.d_occ, 0, n * sizeof(uint32_t), ctx->stream);
    map->levels.push_back(std::move(L));
    sx /= 2;     // resolution /= 2 (H/slam_main/MapRepMultiMap.h:83)
    sy /= 2;
    cl *= 2.0f;  // :84
  }
  {
    const char* e = getenv("LSLAM_MAP_TWO_KERNELS");
    map->force_two_kernels = e && e[0] == '1';
    e = getenv("LSLAM_GN_ORDERED");
    map->ordered_sums = e && e[0] == '1';
    e = getenv("LSLAM_GN_THREADS");
    if (e && atoi(e) >= 256) map->gn_threads = atoi(e);
    e = getenv("LSLAM_SCORE_CHUNK");
    if (e && (atoi(e) == 2 || atoi(e) == 4 || atoi(e) == 8)) map->score_chunk = atoi(e);
  }
  (void)hipStreamSynchronize(ctx->stream);
  ctx->pre_sync.emplace_back((void*)map, [](void* m) { return lslam_map_flush((lslam_map*)m); });  // lslam_synchronize flushes
  // ... and, once the stream has drained, makes a window miss LOUD: cells that LSLAM_MAP_OPT_BATCH_RADIUS_CELLS left outside
  // their scan's window were dropped -- the map no longer equals the reference's -- so the synchronise that learns of it fails
  ctx->post_sync.emplace_back((void*)map, [](void* mp) {
    lslam_map* m = (lslam_map*)mp;
    if (!m->d_batch_misses) return (int)LSLAM_OK;
    const unsigned long long now = __atomic_load_n(m->d_batch_misses, __ATOMIC_ACQUIRE);
    if (now == m->batch_misses_reported) return (int)LSLAM_OK;
    const unsigned long long fresh = now - m->batch_misses_reported;
    m->batch_misses_reported = now;
    return m->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT,
                        "lslam_map_update_batch_dev: %llu hit / free cells lay outside their scan's window and were DROPPED "
                        "(LSLAM_MAP_OPT_BATCH_RADIUS_CELLS understates a scan's reach): the map has diverged from "
                        "updateByScan's (OccGridMapBase.h:118-168); raise the hint or set it to 0 (whole-map windows)", fresh);
  });
  *out = map;
  return LSLAM_OK;
}

void lslam_map_destroy(lslam_map* map) {
  if (!map) return;
  for (size_t i = 0; i < map->ctx->pre_sync.size(); i++)
    if (map->ctx->pre_sync[i].first == (void*)map) {
      map->ctx->pre_sync.erase(map->ctx->pre_sync.begin() + (long)i);
      break;
    }
  for (size_t i = 0; i < map->ctx->post_sync.size(); i++)
    if (map->ctx->post_sync[i].first == (void*)map) {
      map->ctx->post_sync.erase(map->ctx->post_sync.begin() + (long)i);
      break;
    }
  (void)hipSetDevice(map->ctx->device);
  (void)hipStreamSynchronize(map->ctx->stream);
  for (auto& L : map->levels) {
    if (L.d_logodds) (void)hipFree(L.d_logodds);
    if (L.d_free) (void)hipFree(L.d_free);
    if (L.d_occ) (void)hipFree(L.d_occ);
    if (L.d_free2) (void)hipFree(L.d_free2);
    if (L.d_occ2) (void)hipFree(L.d_occ2);
    L.pipe_pts[0].release();
    L.pipe_pts[1].release();
    L.d_pool.release();
    if (L.d_flags) (void)hipFree(L.d_flags);
  }
  if (map->d_batch_misses) (void)hipHostFree(map->d_batch_misses);
  map->d_pts.release();
  map->d_cached.release();
  map->d_gn_out.release();
  map->d_gnb_ent.release();
  map->d_gnb_io.release();
  map->d_score_io.release();
  map->d_hash.release();
  map->d_hdr.release();
  map->d_scan.release();
  map->d_scan_ranges.release();
  map->d_cossin.release();
  map->d_i8.release();
  if (map->h_stage) (void)hipHostFree(map->h_stage);
  if (map->h_gn_pts) (void)hipHostFree(map->h_gn_pts);
  if (map->h_gn_out) (void)hipHostFree(map->h_gn_out);
  for (auto e : map->stage_ev)
    if (e) (void)hipEventDestroy(e);
  delete map;
}

int lslam_map_reset(lslam_map* map) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  for (auto& L : map->levels) {
    L.pending = false;  // a reset map has no use for the deferred apply
    LSLAM_HIP(ctx, hipMemsetAsync(L.d_logodds, 0, (size_t)L.sx * L.sy * sizeof(float), ctx->stream));
    int rc = clear_marks(map, L);
    if (rc) return rc;
  }
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSLAM_OK;
}

int lslam_map_set_update_factor_free(lslam_map* map, float p) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  map->lo_free = prob_to_logodds(p);
  return LSLAM_OK;
}
int lslam_map_set_update_factor_occupied(lslam_map* map, float p) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  map->lo_occ = prob_to_logodds(p);
  return LSLAM_OK;
}
int lslam_map_levels(const lslam_map* map) { return map ? (int)map->levels.size() : LSLAM_ERR_INVALID_ARGUMENT; }
int lslam_map_size(const lslam_map* map, int level, int* sx, int* sy) {
  if (!map || level < 0 || level >= (int)map->levels.size()) return LSLAM_ERR_INVALID_ARGUMENT;
  if (sx) *sx = map->levels[level].sx;
  if (sy) *sy = map->levels[level].sy;
  return LSLAM_OK;
}
float lslam_map_scale_to_map(const lslam_map* map, int level) {
  if (!map || level < 0 || level >= (int)map->levels.size()) return 0.f;
  return map->levels[level].scale_to_map;
}

int lslam_map_update_by_scan_dev(lslam_map* map, const float* pts_dev, int n, const float origo[2],
                                 const float pose[3]) {
  if (!map || n < 0 || (n > 0 && !pts_dev) || !origo || !pose) return LSLAM_ERR_INVALID_ARGUMENT;
  return update_impl(map, pts_dev, n, origo, pose, 0, 0.f, 0.f, 0.0);
}

namespace {
// Copy the caller's points through a pinned ring slot to d_pts on the context stream.  The caller's
// buffer is free again when this returns; the device copy is ordered before the kernels that follow.
int stage_points(lslam_map* map, const float* pts, int n) {
  lslam_context* ctx = map->ctx;
  const size_t floats = (size_t)2 * (n > 0 ? n : 1);
  LSLAM_HIP(ctx, map->d_pts.reserve(floats));
  if (n <= 0) return LSLAM_OK;
  if (floats > map->stage_cap) {  // (re)build the ring; drains whatever is in flight first
    LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (map->h_stage) (void)hipHostFree(map->h_stage);
    map->h_stage = nullptr;
    map->stage_cap = 0;
    const size_t cap = floats + floats / 4 + 64;
    LSLAM_HIP(ctx, hipHostMalloc((void**)&map->h_stage, cap * lslam_map::kStageSlots * sizeof(float), hipHostMallocDefault));
    map->stage_cap = cap;
    for (int i = 0; i < lslam_map::kStageSlots; i++) {
      if (!map->stage_ev[i]) LSLAM_HIP(ctx, hipEventCreateWithFlags(&map->stage_ev[i], hipEventDisableTiming));
      map->stage_busy[i] = false;
    }
  }
  const int slot = (int)(map->stage_next++ % lslam_map::kStageSlots);
  if (map->stage_busy[slot]) LSLAM_HIP(ctx, hipEventSynchronize(map->stage_ev[slot]));
  float* h = map->h_stage + (size_t)slot * map->stage_cap;
  memcpy(h, pts, (size_t)2 * n * sizeof(float));
  LSLAM_HIP(ctx, hipMemcpyAsync(map->d_pts.p, h, (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  LSLAM_HIP(ctx, hipEventRecord(map->stage_ev[slot], ctx->stream));
  map->stage_busy[slot] = true;
  return LSLAM_OK;
}
}  // namespace

// Asynchronous like every device-side mutation of the map: the update is ENQUEUED on the context stream
// when this returns (the caller's `pts` may be reused at once); the readers -- lslam_map_read_*,
// lslam_map_match_data, lslam_synchronize -- are ordered after it.
int lslam_map_update_by_scan(lslam_map* map, const float* pts, int n, const float origo[2], const float pose[3]) {
  if (!map || n < 0 || (n > 0 && !pts) || !origo || !pose) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  if (n > 0 && n == map->gn_host_n && map->levels.size() >= 1 && memcmp(pts, map->h_gn_pts, (size_t)2 * n * sizeof(float)) == 0)
    return update_impl(map, map->d_cached.p, n, origo, pose, 0, 0.f, 0.f, 0.0);  // the container just matched: already in HBM
  int rc = stage_points(map, pts, n);
  if (rc) return rc;
  return update_impl(map, map->d_pts.p, n, origo, pose, 0, 0.f, 0.f, 0.0);
}

namespace {
constexpr int kBatchMaxScans = kBatchSlots;

// The window of tiles of one scan on one level: every cell of a ray lies between the begin cell and the end cell, and the
// end cell is within |p - origo| * factor of the begin cell (a rotation), + 1 for the two roundings, + 1 for float32
// slack.  reach < 0 (or absurdly large) = unknown: the whole map.  out = tx0, ty0, tw, th (tw = 0: nothing reaches the map).
void plan_window(int sx, int sy, int bx, int by, int n, double reach, double factor, int out[4]) {
  long long x0 = 0, y0 = 0, x1 = sx - 1, y1 = sy - 1;
  if (reach >= 0.0 && reach < 1e9) {
    const long long R = (long long)ceil(reach * factor) + 2;
    x0 = std::max<long long>(x0, (long long)bx - R); x1 = std::min<long long>(x1, (long long)bx + R);
    y0 = std::max<long long>(y0, (long long)by - R); y1 = std::min<long long>(y1, (long long)by + R);
  }
  if (n == 0 || x1 < x0 || y1 < y0 || bx < 0 || by < 0 || bx >= sx || by >= sy) {
    out[0] = out[1] = out[2] = out[3] = 0;  // (a begin cell outside the map drops every beam, H/map/OccGridMapBase.h:226-238)
  } else {
    out[0] = (int)(x0 >> 3); out[1] = (int)(y0 >> 3);
    out[2] = (int)(x1 >> 3) - out[0] + 1; out[3] = (int)(y1 >> 3) - out[1] + 1;
  }
}
// Rounds: consecutive scans whose windows fit the budget together; a scan whose window alone exceeds it gets a round
// -- and the memory -- of its own.  base[k] = first tile slot of scan k inside its round; round_of[k] (may be null).
// Returns the number of rounds, or -1 when one window has 2^26 tiles or more (byte offsets into the pool are 32-bit).
int plan_rounds(const int* tw, const int* th, int K, size_t budget_bytes, uint32_t* base, int* round_of, size_t* max_slots) {
  const size_t budget_slots = std::max<size_t>(1, budget_bytes / 64);
  int n_rounds = 0;
  size_t most = 0;
  for (int k0 = 0; k0 < K;) {
    size_t sum = 0;
    int k1 = k0;
    while (k1 < K) {
      const size_t need = (size_t)tw[k1] * (size_t)th[k1];
      if (k1 > k0 && sum + need > budget_slots) break;
      if (sum + need >= ((size_t)1 << 26)) break;
      base[k1] = (uint32_t)sum;
      if (round_of) round_of[k1] = n_rounds;
      sum += need;
      k1++;
    }
    if (k1 == k0) return -1;
    most = std::max(most, sum);
    n_rounds++;
    k0 = k1;
  }
  if (max_slots) *max_slots = most;
  return n_rounds;
}

// K successive MapRepMultiMap::updateByScan calls (every level fed the same scan, i.e. each scan matched first) in
// four launches per level and round.  d_pts: the K containers back to back; counts / origos / poses are host arrays;
// radius (host, may be null): per scan, the distance of its farthest point from its origo in level-0 cells.
int update_batch_impl(lslam_map* map, int K, const float* d_pts, const int32_t* counts, const float* origos,
                      const float* poses, const float* radius, bool use_hint) {
  lslam_context* ctx = map->ctx;
  {
    int rc = flush_pending(map);  // a single-scan update may still owe its apply
    if (rc) return rc;
  }
  int n_max = 0;
  for (int k = 0; k < K; k++) {
    if (counts[k] < 0 || counts[k] > kMaxBeams)
      return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per scan are supported (got %d)", kMaxBeams, counts[k]);
    n_max = std::max(n_max, counts[k]);
  }
  if (n_max == 0) return LSLAM_OK;
  for (const Level& L : map->levels)
    if (L.sx > 32768 || L.sy > 32768)
      return ctx->fail(LSLAM_ERR_UNSUPPORTED, "batched update: map sides up to 32768 cells (k_lo_batch_rays' 32-bit ray arithmetic)");
  uint32_t slots = 64;
  while (slots < 2u * (uint32_t)n_max) slots *= 2;
  LSLAM_HIP(ctx, map->d_hash.reserve((size_t)3 * K * slots));
  LSLAM_HIP(ctx, map->d_hdr.reserve((size_t)K * map->levels.size()));
  if (!map->d_batch_misses) {
    LSLAM_HIP(ctx, hipHostMalloc((void**)&map->d_batch_misses, sizeof(unsigned long long), hipHostMallocDefault));
    *map->d_batch_misses = 0ull;
  }
  std::vector<ScanHdr> hdr((size_t)K * map->levels.size());
  std::vector<int> off(K + 1, 0);
  for (int k = 0; k < K; k++) off[k + 1] = off[k] + counts[k];
  struct Round { int k0, k1; size_t slots; };
  std::vector<std::vector<Round>> rounds(map->levels.size());
  for (size_t li = 0; li < map->levels.size(); li++) {
    Level& L = map->levels[li];
    L.tiles_x = (L.sx + 7) / 8;
    L.n_tiles = L.tiles_x * ((L.sy + 7) / 8);
    const float factor = li == 0 ? 1.0f : (float)(1.0 / pow(2.0, (double)li));
    for (int k = 0; k < K; k++) {
      ScanHdr& h = hdr[li * K + k];
      const float* pose = poses + 3 * k;
      const float ox = li == 0 ? origos[2 * k] : origos[2 * k] * factor;
      const float oy = li == 0 ? origos[2 * k + 1] : origos[2 * k + 1] * factor;
      const float sc = L.scale_to_map;
      const float mx = (sc * pose[0] + 0.0f * pose[1]) + L.t_x;  // getMapCoordsPose (H/map/GridMapBase.h:238-242)
      const float my = (0.0f * pose[0] + sc * pose[1]) + L.t_y;
      h.c = cosf(pose[2]);
      h.s = sinf(pose[2]);
      h.tx = mx; h.ty = my;
      const float bxf = (h.c * ox + (-h.s) * oy) + mx;  // H/map/OccGridMapBase.h:132
      const float byf = (h.s * ox + h.c * oy) + my;
      h.bx = (int)(bxf + 0.5f);                         // :135
      h.by = (int)(byf + 0.5f);
      h.n = counts[k];
      h.pts_off = off[k];
      double reach = -1.0;  // unknown: the whole map
      if (radius) reach = (double)radius[k];
      else if (use_hint && map->batch_radius_hint > 0) reach = (double)map->batch_radius_hint;  // device-resident points only
      int w[4];
      plan_window(L.sx, L.sy, h.bx, h.by, h.n, reach, (double)factor, w);
      h.tx0 = w[0]; h.ty0 = w[1]; h.tw = w[2]; h.th = w[3];
      h.base = 0; h.pad[0] = h.pad[1] = h.pad[2] = 0;
    }
    {
      std::vector<int> tw(K), th(K), round_of(K);
      std::vector<uint32_t> base(K);
      for (int k = 0; k < K; k++) { tw[k] = hdr[li * K + k].tw; th[k] = hdr[li * K + k].th; }
      const int nr = plan_rounds(tw.data(), th.data(), K, map->batch_budget, base.data(), round_of.data(), nullptr);
      if (nr < 0) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "batched update: a scan window of 2^26 tiles or more");
      for (int k = 0; k < K; k++) {
        hdr[li * K + k].base = base[k];
        if (k == 0 || round_of[k] != round_of[k - 1]) rounds[li].push_back(Round{k, k, 0});
        Round& r = rounds[li].back();
        r.k1 = k + 1;
        r.slots = std::max(r.slots, (size_t)base[k] + (size_t)tw[k] * (size_t)th[k]);
      }
    }
  }
  map->batch_last_rounds = (int)rounds[0].size();
  LSLAM_HIP(ctx, hipMemcpyAsync(map->d_hdr.p, hdr.data(), hdr.size() * sizeof(ScanHdr), hipMemcpyHostToDevice, ctx->stream));
  for (size_t li = 0; li < map->levels.size(); li++) {
    Level& L = map->levels[li];
    if (!L.d_flags) {
      if (hipMalloc((void**)&L.d_flags, (size_t)L.n_tiles * kBatchSlots) != hipSuccess) {
        (void)hipGetLastError();
        L.d_flags = nullptr;
        return ctx->fail(LSLAM_ERR_HIP, "cannot allocate the tile flags of the batched update (%zu bytes)", (size_t)L.n_tiles * kBatchSlots);
      }
      L.batch_epoch = 0;
    }
    size_t need_slots = 1;
    for (const Round& r : rounds[li]) need_slots = std::max(need_slots, r.slots);
    if (need_slots * 64 > L.d_pool.cap) {
      // grow to what this call needs, rounded up to 1 MB (rare: the windows of a trajectory have a steady size).  The
      // old pool goes first -- nothing may still read it, so the stream is drained once -- instead of living on beside the new one
      LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
      L.d_pool.release();
      // a sixteenth of headroom: the windows of the next 64 scans are clipped a little differently by the map's edges, and
      // growing again means draining the stream again
      const size_t want = need_slots * 64 + need_slots * 4;
      const size_t bytes = ((want + ((size_t)1 << 20) - 1) >> 20) << 20;
      uint8_t* fresh = nullptr;
      if (hipMalloc((void**)&fresh, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return ctx->fail(LSLAM_ERR_HIP, "cannot allocate %zu bytes of tile slots for the batched update", bytes);
      }
      L.d_pool.p = fresh;
      L.d_pool.cap = bytes;
      L.batch_epoch = 0;  // fresh memory: cleared below
    }
    for (const Round& r : rounds[li]) {
      const int Kr = r.k1 - r.k0;
      if (L.batch_epoch == 0 || L.batch_epoch >= 63) {  // 6-bit epoch in the pool / flag bytes
        LSLAM_HIP(ctx, hipMemsetAsync(L.d_pool.p, 0, L.d_pool.cap, ctx->stream));
        LSLAM_HIP(ctx, hipMemsetAsync(L.d_flags, 0, (size_t)L.n_tiles * kBatchSlots, ctx->stream));
        L.batch_epoch = 0;
      }
      L.batch_epoch++;
      L.pool_slots = L.d_pool.cap / 64;
      const bool lds_hash = (size_t)slots * 8 <= 64 * 1024;  // k_lo_batch_hits_lds writes the key and first-hit tables whole
      if (lds_hash)
        LSLAM_HIP(ctx, hipMemsetAsync(map->d_hash.p + (size_t)2 * Kr * slots, 0xFF, (size_t)Kr * slots * sizeof(uint32_t), ctx->stream));
      else
        LSLAM_HIP(ctx, hipMemsetAsync(map->d_hash.p, 0xFF, (size_t)3 * Kr * slots * sizeof(uint32_t), ctx->stream));
      BatchGeom g;
      g.sx = L.sx; g.sy = L.sy; g.K = Kr;
      g.tiles_x = L.tiles_x; g.n_tiles = L.n_tiles;
      g.factor = li == 0 ? 1.0f : (float)(1.0 / pow(2.0, (double)li));
      g.lo_free = map->lo_free; g.lo_occ = map->lo_occ;
      g.tag = L.batch_epoch << 2;
      g.hash_mask = slots - 1;
      uint32_t* hkey = map->d_hash.p;
      uint32_t* hhit = hkey + (size_t)Kr * slots;
      uint32_t* hcross = hhit + (size_t)Kr * slots;
      const ScanHdr* d_h = map->d_hdr.p + li * K + r.k0;
      int nr_max = 0;
      for (int k = r.k0; k < r.k1; k++) nr_max = std::max(nr_max, counts[k]);
      if (nr_max == 0) continue;
      if (lds_hash)
        launch(ctx, "lo_batch_hits", k_lo_batch_hits_lds, dim3(Kr), dim3(1024), (size_t)slots * 8, g, d_h, d_pts, L.d_pool.p,
               L.d_flags, hkey, hhit, map->d_batch_misses);
      else
        launch(ctx, "lo_batch_hits", k_lo_batch_hits, dim3((nr_max + 255) / 256, Kr), dim3(256), 0, g, d_h, d_pts, L.d_pool.p,
               L.d_flags, hkey, hhit, map->d_batch_misses);
      const int groups = (nr_max + kRayBeamsPerWave - 1) / kRayBeamsPerWave;
      const long long waves = (long long)Kr * groups;
      launch(ctx, "lo_batch_rays", k_lo_batch_rays, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, g, d_h, d_pts, L.d_pool.p,
             L.d_flags, (const uint32_t*)hkey, hcross, groups);
      launch(ctx, "lo_batch_resolve", k_lo_batch_resolve, dim3((unsigned)(((size_t)Kr * slots + 255) / 256)), dim3(256), 0, g,
             d_h, (const uint32_t*)hkey, (const uint32_t*)hhit, (const uint32_t*)hcross, L.d_pool.p);
      launch(ctx, "lo_batch_apply", k_lo_batch_apply, dim3((unsigned)((L.n_tiles + 3) / 4)), dim3(256), 0, g, d_h,
             (const uint8_t*)L.d_pool.p, (const uint8_t*)L.d_flags, L.d_logodds);
    }
  }
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}
}  // namespace

namespace {
// n_scans containers back to back in points_xy; batches larger than 64 scans are cut into groups of 64
int update_batch_dev_impl(lslam_map* map, int n_scans, const float* points_xy_dev, const int32_t* n_points,
                          const float* origos_xy, const float* poses_world, const float* radius, bool use_hint) {
  lslam_context* ctx = map->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  // a call is applied whole or not at all: a scan that a later group of 64 would refuse is refused before the first group runs
  for (int k = 0; k < n_scans; k++)
    if (n_points[k] < 0 || n_points[k] > kMaxBeams)
      return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per scan are supported (got %d)", kMaxBeams, n_points[k]);
  size_t done_pts = 0;
  for (int k0 = 0; k0 < n_scans; k0 += kBatchMaxScans) {
    const int K = std::min(kBatchMaxScans, n_scans - k0);
    int rc = update_batch_impl(map, K, points_xy_dev + 2 * done_pts, n_points + k0, origos_xy + 2 * k0, poses_world + 3 * k0,
                               radius ? radius + k0 : nullptr, use_hint);
    if (rc) return rc;
    for (int k = 0; k < K; k++) done_pts += (size_t)n_points[k0 + k];
  }
  if (n_scans > 0 && map->levels.size() > 1) {  // dataContainers now hold the last scan (as after its matchData)
    const int last = n_scans - 1;
    const int n = n_points[last];
    map->gn_host_n = -1;
    LSLAM_HIP(ctx, map->d_cached.reserve((size_t)2 * (n > 0 ? n : 1)));
    if (n > 0)
      LSLAM_HIP(ctx, hipMemcpyAsync(map->d_cached.p, points_xy_dev + 2 * (done_pts - (size_t)n), (size_t)2 * n * sizeof(float),
                                    hipMemcpyDeviceToDevice, ctx->stream));
    map->n_cached = n;
    map->cached_origo[0] = origos_xy[2 * last];
    map->cached_origo[1] = origos_xy[2 * last + 1];
  }
  return LSLAM_OK;
}
}  // namespace

int lslam_map_update_batch_dev(lslam_map* map, int n_scans, const float* points_xy_dev, const int32_t* n_points,
                               const float* origos_xy, const float* poses_world) {
  if (!map || n_scans < 0 || !n_points || !origos_xy || !poses_world) return LSLAM_ERR_INVALID_ARGUMENT;
  // the host never sees these points: the windows come from LSLAM_MAP_OPT_BATCH_RADIUS_CELLS, or cover the whole map
  return update_batch_dev_impl(map, n_scans, points_xy_dev, n_points, origos_xy, poses_world, nullptr, true);
}

int lslam_map_update_batch(lslam_map* map, int n_scans, const float* points_xy, const int32_t* n_points,
                           const float* origos_xy, const float* poses_world) {
  if (!map || n_scans < 0 || !n_points || !origos_xy || !poses_world) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  size_t total = 0;
  for (int k = 0; k < n_scans; k++) {
    if (n_points[k] < 0) return LSLAM_ERR_INVALID_ARGUMENT;
    total += (size_t)n_points[k];
  }
  if (total > 0 && !points_xy) return LSLAM_ERR_INVALID_ARGUMENT;
  if (total > (size_t)INT32_MAX / 2) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "batch too large");
  // The scans' reach, where it decides anything: on a map whose whole planes fit the budget every window is the map
  // anyway.  One pass over the points the host is about to copy: max |p - origo| per scan, in level-0 cells.
  std::vector<float> radius;
  if (!map->levels.empty()) {
    const Level& L0 = map->levels[0];
    const size_t plane = (size_t)((L0.sx + 7) / 8) * (size_t)((L0.sy + 7) / 8) * 64;
    if (plane * (size_t)std::min(n_scans, kBatchMaxScans) > map->batch_budget) {
      radius.resize((size_t)n_scans);
      size_t at = 0;
      for (int k = 0; k < n_scans; k++) {
        const float ox = origos_xy[2 * k], oy = origos_xy[2 * k + 1];
        float m2 = 0.f;
        bool finite = true;
        for (int i = 0; i < n_points[k]; i++) {
          const float dx = points_xy[2 * (at + i)] - ox, dy = points_xy[2 * (at + i) + 1] - oy;
          const float d2 = dx * dx + dy * dy;
          finite = finite && (d2 == d2) && d2 < 1e18f;
          m2 = d2 > m2 ? d2 : m2;
        }
        at += (size_t)n_points[k];
        radius[k] = finite ? sqrtf(m2) * 1.0001f + 1.0f : 2e9f;  // a non-finite point: no bound (such a beam is dropped anyway)
      }
    }
  }
  int rc = stage_points(map, points_xy, (int)total);
  if (rc) return rc;
  // (the hint is for points the host cannot see; these it has just measured, or their windows are the map anyway)
  return update_batch_dev_impl(map, n_scans, map->d_pts.p, n_points, origos_xy, poses_world, radius.empty() ? nullptr : radius.data(),
                               false);
}

// Host-only: what a batched update of these scans would allocate on a level of sx x sy cells -- the planner
// update_batch_impl itself uses.  No context, no GPU.
int lslam_map_plan_batch_windows(int sx, int sy, int n_scans, const int32_t* begin_cells_xy, const int32_t* n_points,
                                 const double* reach_cells, double level_factor, int64_t budget_bytes, int32_t* windows_out,
                                 uint32_t* base_out, int32_t* round_out, int64_t* pool_bytes_out) {
  if (sx <= 0 || sy <= 0 || n_scans < 0 || budget_bytes < 64 || (n_scans > 0 && (!begin_cells_xy || !n_points || !windows_out || !base_out)))
    return LSLAM_ERR_INVALID_ARGUMENT;
  std::vector<int> tw((size_t)n_scans), th((size_t)n_scans);
  for (int k = 0; k < n_scans; k++) {
    int w[4];
    plan_window(sx, sy, begin_cells_xy[2 * k], begin_cells_xy[2 * k + 1], n_points[k], reach_cells ? reach_cells[k] : -1.0,
                level_factor, w);
    for (int i = 0; i < 4; i++) windows_out[4 * k + i] = w[i];
    tw[k] = w[2]; th[k] = w[3];
  }
  size_t most = 0;
  const int nr = plan_rounds(tw.data(), th.data(), n_scans, (size_t)budget_bytes, base_out, round_out, &most);
  if (nr < 0) return LSLAM_ERR_UNSUPPORTED;
  if (pool_bytes_out) *pool_bytes_out = (int64_t)(most * 64);
  return nr;
}

// out[0] = bytes of scratch the batched update holds right now over all levels (tile-slot pools + tile flags),
// out[1] = rounds level 0 of the last batch needed, out[2] = cells found outside their scan's window since the map was
// created (0 unless LSLAM_MAP_OPT_BATCH_RADIUS_CELLS understated a scan's reach; synchronises), out[3] = the budget
int lslam_map_batch_stats(lslam_map* map, int64_t out[4]) {
  if (!map || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  size_t bytes = 0;
  for (const Level& L : map->levels) bytes += L.d_pool.cap + (L.d_flags ? (size_t)L.n_tiles * kBatchSlots : 0);
  out[0] = (int64_t)bytes;
  out[1] = map->batch_last_rounds;
  out[2] = 0;
  out[3] = (int64_t)map->batch_budget;
  if (map->d_batch_misses) {
    LSLAM_HIP(ctx, hipSetDevice(ctx->device));
    LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out[2] = (int64_t)__atomic_load_n(map->d_batch_misses, __ATOMIC_ACQUIRE);
    map->batch_misses_reported = (unsigned long long)out[2];  // the caller has seen the count: not an error a second time
  }
  return LSLAM_OK;
}

namespace {
// laser_geometry's co_sine_map_ (rebuilt when the scan geometry changes): host libm, like the reference's stack
int ensure_cossin(lslam_map* map, int n, const lslam_hector_scan* sp, bool* rebuilt = nullptr) {
  lslam_context* ctx = map->ctx;
  if (rebuilt) *rebuilt = false;
  if (!(n > map->cs_n || sp->angle_min != map->cs_angle_min || sp->angle_increment != map->cs_angle_inc)) return LSLAM_OK;
  std::vector<double2> cs((size_t)std::max(n, 1));
  for (int i = 0; i < n; i++) {
    const double a = (double)sp->angle_min + (double)i * (double)sp->angle_increment;
    cs[i] = make_double2(cos(a), sin(a));
  }
  LSLAM_HIP(ctx, map->d_cossin.reserve(cs.size()));
  LSLAM_HIP(ctx, hipMemcpyAsync(map->d_cossin.p, cs.data(), cs.size() * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // cs dies with this scope
  map->cs_n = n;
  map->cs_angle_min = sp->angle_min;
  map->cs_angle_inc = sp->angle_increment;
  if (rebuilt) *rebuilt = true;
  return LSLAM_OK;
}

ProjectCfg project_cfg(const lslam_map* map, int n, const lslam_hector_scan* sp) {
  ProjectCfg c;
  c.n = n;
  c.range_min = sp->range_min;
  c.cutoff = sp->range_cutoff < 0.f ? sp->range_max : sp->range_cutoff;  // laser_geometry: cutoff < 0 -> range_max
  c.sqr_min = sp->sqr_laser_min_dist;
  c.sqr_max = sp->sqr_laser_max_dist;
  c.use_max_sq = (double)sp->use_max_scan_range * (double)sp->use_max_scan_range;
  c.z_min = sp->laser_z_min;
  c.z_max = sp->laser_z_max;
  c.cy = cos((double)sp->laser_yaw);
  c.sy = sin((double)sp->laser_yaw);
  c.tx = sp->laser_x; c.ty = sp->laser_y; c.tz = sp->laser_z;
  c.scale_to_map = map->levels[0].scale_to_map;
  return c;
}
}  // namespace

int lslam_map_set_scan(lslam_map* map, const float* ranges, int n, const lslam_hector_scan* sp, int* n_points) {
  if (!map || n < 0 || (n > 0 && !ranges) || !sp) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  if (n > kMaxBeams) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d readings per scan (got %d)", kMaxBeams, n);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, map->d_scan.reserve((size_t)2 * std::max(n, 1) + 4));
  LSLAM_HIP(ctx, map->d_scan_ranges.reserve((size_t)std::max(n, 1)));
  {
    int rc = ensure_cossin(map, n, sp);
    if (rc) return rc;
  }
  if (n > 0)
    LSLAM_HIP(ctx, hipMemcpyAsync(map->d_scan_ranges.p, ranges, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  const ProjectCfg c = project_cfg(map, n, sp);
  int* d_n = reinterpret_cast<int*>(map->d_scan.p + (size_t)2 * std::max(n, 1));
  launch(ctx, "hector_project", k_hector_project, dim3(1), dim3(1024), 0, c, (const float*)map->d_scan_ranges.p,
         (const double2*)map->d_cossin.p, map->d_scan.p, d_n);
  int host_n = 0;
  LSLAM_HIP(ctx, hipMemcpyAsync(&host_n, d_n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  map->n_scan = host_n;
  // dataContainer.setOrigo(Eigen::Vector2f(laserPos.x(), laserPos.y()) * scaleToMap) (hector_slam.cc:331)
  map->scan_origo[0] = (float)(double)sp->laser_x * c.scale_to_map;
  map->scan_origo[1] = (float)(double)sp->laser_y * c.scale_to_map;
  if (n_points) *n_points = host_n;
  return LSLAM_OK;
}

int lslam_map_set_cloud(lslam_map* map, const float* xyz, const uint8_t* valid, int n, const lslam_hector_scan* sp, int* n_points) {
  if (!map || n < 0 || (n > 0 && (!xyz || !valid)) || !sp) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  if (n > kMaxBeams) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per cloud (got %d)", kMaxBeams, n);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, map->d_scan.reserve((size_t)2 * std::max(n, 1) + 4));
  // the cloud's way up shares the ranges' buffer: [xyz: 3 n floats | valid: n bytes]
  LSLAM_HIP(ctx, map->d_scan_ranges.reserve((size_t)3 * std::max(n, 1) + ((size_t)n + 3) / 4));
  float* d_xyz = map->d_scan_ranges.p;
  uint8_t* d_valid = reinterpret_cast<uint8_t*>(map->d_scan_ranges.p + (size_t)3 * std::max(n, 1));
  if (n > 0) {
    LSLAM_HIP(ctx, hipMemcpyAsync(d_xyz, xyz, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    LSLAM_HIP(ctx, hipMemcpyAsync(d_valid, valid, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  }
  const ProjectCfg c = project_cfg(map, n, sp);
  int* d_n = reinterpret_cast<int*>(map->d_scan.p + (size_t)2 * std::max(n, 1));
  launch(ctx, "hector_cloud_container", k_hector_cloud_container, dim3(1), dim3(1024), 0, c, (const float*)d_xyz,
         (const uint8_t*)d_valid, map->d_scan.p, d_n);
  int host_n = 0;
  LSLAM_HIP(ctx, hipMemcpyAsync(&host_n, d_n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  map->n_scan = host_n;
  // dataContainer.setOrigo(Eigen::Vector2f(laserPos.x(), laserPos.y()) * scaleToMap) (hector_slam.cc:329)
  map->scan_origo[0] = (float)(double)sp->laser_x * c.scale_to_map;
  map->scan_origo[1] = (float)(double)sp->laser_y * c.scale_to_map;
  if (n_points) *n_points = host_n;
  return LSLAM_OK;
}

int lslam_map_read_container(lslam_map* map, float* out_xy, int capacity, float origo_xy[2]) {
  if (!map || capacity < 0 || (capacity > 0 && !out_xy)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  const int n = std::min(capacity, map->n_scan);
  if (n > 0) {
    LSLAM_HIP(ctx, hipMemcpyAsync(out_xy, map->d_scan.p, (size_t)2 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (origo_xy) { origo_xy[0] = map->scan_origo[0]; origo_xy[1] = map->scan_origo[1]; }
  return map->n_scan;
}

int lslam_map_update_by_container(lslam_map* map, const float pose_world[3]) {
  if (!map || !pose_world) return LSLAM_ERR_INVALID_ARGUMENT;
  LSLAM_HIP(map->ctx, hipSetDevice(map->ctx->device));
  return update_impl(map, map->d_scan.p, map->n_scan, map->scan_origo, pose_world, 0, 0.f, 0.f, 0.0);
}

int lslam_map_update_just_once(lslam_map* map, const float* pts, int n, const float origo[2], float begin_x,
                               float begin_y, double metres_per_cell) {
  if (!map || n < 0 || (n > 0 && !pts) || !origo || !(metres_per_cell > 0)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  int rc = stage_points(map, pts, n);
  if (rc) return rc;
  const float pose[3] = {0.f, 0.f, 0.f};
  return update_impl(map, map->d_pts.p, n, origo, pose, 1, begin_x, begin_y, metres_per_cell);
}

namespace {
GnLevels gn_levels_of(const lslam_map* map) {  // the pyramid as the matcher's kernels take it
  GnLevels lv;
  lv.n_levels = (int)map->levels.size();
  for (int i = 0; i < lv.n_levels; i++) {
    const Level& L = map->levels[i];
    lv.sx[i] = L.sx; lv.sy[i] = L.sy; lv.scale[i] = L.scale_to_map; lv.t_x[i] = L.t_x; lv.t_y[i] = L.t_y;
    lv.logodds[i] = L.d_logodds;
  }
  return lv;
}

// The form a parallel-sums match of up to `n` points is launched in: threads per block from LSLAM_GN_THREADS; the points of
// the scan in registers when they fit (3 per thread at 512 threads: a 1081-beam scan), else staged in LDS, else read from memory
struct GnForm {
  int nt;      // 256 | 512 | 1024
  bool reg;    // k_*_match_reg<nt, points per thread>; else k_*_match_fast<nt>
  int in_lds;  // staged form: the points fit in LDS
  size_t lds;  // staged form: dynamic LDS bytes (0 for the register form)
};
GnForm gn_form_of(const lslam_map* map, int n) {
  GnForm f;
  f.nt = map->gn_threads >= 1024 ? 1024 : (map->gn_threads >= 512 ? 512 : 256);
  f.reg = n <= (f.nt == 1024 ? 1024 * 2 : (f.nt == 512 ? 512 * 3 : 256 * 5));
  f.in_lds = (size_t)2 * n * sizeof(float) <= 56 * 1024;
  f.lds = !f.reg && f.in_lds ? (size_t)2 * std::max(n, 1) * sizeof(float) : 0;
  return f;
}
// the one ladder over the forms: REG(NT, PMAX) / FAST(NT) are the caller's launch statements
#define LSLAM_GN_DISPATCH(F, REG, FAST)                                                                                    \
  do {                                                                                                                     \
    if ((F).reg) {                                                                                                         \
      if ((F).nt == 1024) REG(1024, 2); else if ((F).nt == 512) REG(512, 3); else REG(256, 5);                             \
    } else {                                                                                                               \
      if ((F).nt == 1024) FAST(1024); else if ((F).nt == 512) FAST(512); else FAST(256);                                   \
    }                                                                                                                      \
  } while (0)

int match_data_impl(lslam_map* map, const float* pts, int n, bool pts_on_device, const float origo[2],
                    const float begin_world[3], float out_pose[3], float out_cov[9]) {
  lslam_context* ctx = map->ctx;
  if ((int)map->levels.size() > kGnMaxLevels)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d pyramid levels", kGnMaxLevels);
  if (map->ordered_sums && (size_t)n * 9 * sizeof(float) > 150 * 1024)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per scan in matchData", (int)(150 * 1024 / 36));
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  {
    int rc = flush_pending(map);  // the matcher reads the float planes
    if (rc) return rc;
  }
  LSLAM_HIP(ctx, map->d_cached.reserve((size_t)2 * (n > 0 ? n : 1)));
  LSLAM_HIP(ctx, map->d_gn_out.reserve(16));
  float* d_out = map->d_gn_out.p;
  map->gn_host_n = -1;  // d_cached is about to be rewritten; the fast host-fed path below re-validates its host copy
  if (map->levels.size() > 1) {
    map->n_cached = n;
    map->cached_origo[0] = origo ? origo[0] : 0.f;
    map->cached_origo[1] = origo ? origo[1] : 0.f;
  }
  const GnLevels lv = gn_levels_of(map);
  if (!map->ordered_sums) {
    // ---- parallel sums (default): one launch, no copy operation on the stream --------------------------------------------
    if (!map->h_gn_out && hipHostMalloc((void**)&map->h_gn_out, 16 * sizeof(float), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return ctx->fail(LSLAM_ERR_HIP, "cannot allocate the pinned result of matchData");
    }
    if (map->gn_ticket == 0) ((int*)map->h_gn_out)[15] = 0;  // fresh allocation: no stale word may look like ticket 1
    const float* src = pts;
    if (!pts_on_device && n > 0) {
      if ((size_t)2 * n > map->h_gn_cap) {
        if (map->h_gn_pts) (void)hipHostFree(map->h_gn_pts);
        map->h_gn_pts = nullptr;
        map->h_gn_cap = 0;
        const size_t want = (size_t)2 * n + 256;
        if (hipHostMalloc((void**)&map->h_gn_pts, want * sizeof(float), hipHostMallocDefault) != hipSuccess) {
          (void)hipGetLastError();
          return ctx->fail(LSLAM_ERR_HIP, "cannot allocate the pinned staging of matchData");
        }
        map->h_gn_cap = want;
      }
      memcpy(map->h_gn_pts, pts, (size_t)2 * n * sizeof(float));
      src = map->h_gn_pts;
      map->gn_host_n = n;
    }
    const GnForm form = gn_form_of(map, n);
    float* cache_dst = n > 0 ? map->d_cached.p : (float*)nullptr;
    const int ticket = ++map->gn_ticket;
#define LSLAM_GN_FAST(NT)                                                                                                  \
  launch(ctx, "gn_match", k_gn_match_fast<NT>, dim3(1), dim3(NT), form.lds, lv, src, cache_dst, n, form.in_lds,            \
         begin_world[0], begin_world[1], begin_world[2], map->h_gn_out, ticket)
#define LSLAM_GN_REG(NT, PMAX)                                                                                             \
  launch(ctx, "gn_match", k_gn_match_reg<NT, PMAX>, dim3(1), dim3(NT), form.lds, lv, src, cache_dst, n, begin_world[0],    \
         begin_world[1], begin_world[2], map->h_gn_out, ticket)
    LSLAM_GN_DISPATCH(form, LSLAM_GN_REG, LSLAM_GN_FAST);
#undef LSLAM_GN_REG
#undef LSLAM_GN_FAST
    LSLAM_HIP(ctx, hipGetLastError());
    // bounded spin on the ticket (acquire); the stream itself if it does not show up (a failed launch, a device fault)
    if (!spin_for_ticket((const int*)map->h_gn_out + 15, ticket)) LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 3; i++) out_pose[i] = map->h_gn_out[i];
    if (out_cov) for (int i = 0; i < 9; i++) out_cov[i] = map->h_gn_out[3 + i];
    return LSLAM_OK;
  }
  // ---- ordered sums: the reference's sequential fp32 accumulation, bit for bit -----------------------------------------
  // dataContainers[index-1].setFrom(dataContainer, ...) (MapRepMultiMap.h:161): the container is cached for the
  // next updateByScan -- also when it is empty
  if (n > 0)
    LSLAM_HIP(ctx, hipMemcpyAsync(map->d_cached.p, pts, (size_t)2 * n * sizeof(float),
                                  pts_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  const size_t lds = (size_t)std::max(n, 1) * 9 * sizeof(float);
  if (lds > 64 * 1024)
    LSLAM_HIP(ctx, hipFuncSetAttribute((const void*)k_gn_match, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  launch(ctx, "gn_match", k_gn_match, dim3(1), dim3(n > 512 ? 1024 : 256), lds, lv, (const float*)map->d_cached.p, n,
         begin_world[0], begin_world[1], begin_world[2], d_out);
  float host[12];
  LSLAM_HIP(ctx, hipMemcpyAsync(host, d_out, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 3; i++) out_pose[i] = host[i];
  if (out_cov) for (int i = 0; i < 9; i++) out_cov[i] = host[3 + i];
  return LSLAM_OK;
}
}  // namespace

int lslam_map_match_data(lslam_map* map, const float* pts, int n, const float origo[2], const float begin_world[3],
                         float out_pose[3], float out_cov[9]) {
  if (!map || n < 0 || (n > 0 && !pts) || !begin_world || !out_pose) return LSLAM_ERR_INVALID_ARGUMENT;
  return match_data_impl(map, pts, n, false, origo, begin_world, out_pose, out_cov);
}

// matchData on the resident container of lslam_map_set_scan (the container is cached like any other)
int lslam_map_match_container(lslam_map* map, const float begin_world[3], float out_pose[3], float out_cov[9]) {
  if (!map || !begin_world || !out_pose) return LSLAM_ERR_INVALID_ARGUMENT;
  return match_data_impl(map, map->d_scan.p, map->n_scan, true, map->scan_origo, begin_world, out_pose, out_cov);
}

namespace {
// Many matchData calls in one launch.  Everything that can be refused is refused before anything is enqueued.  A pure
// query: neither d_cached / n_cached (the container the next updateByScan feeds to the levels above 0) nor a plane changes.
// d_pts: the containers back to back in HBM; begin / out_pose / out_cov (may be null) in HBM; counts / entry_container host.
int match_batch_check(lslam_map* map, const char* who, int n_entries, int n_containers, const void* points_xy,
                      const int32_t* n_points, const int32_t* entry_container, const void* begin_world, const void* out_poses,
                      size_t* total_out) {
  lslam_context* ctx = map->ctx;
  if (n_entries < 0 || n_containers < 0)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: negative count (n_entries %d, n_containers %d)", who, n_entries, n_containers);
  *total_out = 0;
  if (n_entries == 0) return LSLAM_OK;
  if (!begin_world || !out_poses) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: begin_world and out_poses are required", who);
  if (n_containers > 0 && !n_points) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: n_points is required", who);
  if (!entry_container && n_containers != n_entries)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: without entry_container entry i uses container i, so n_containers (%d) must equal n_entries (%d)",
                     who, n_containers, n_entries);
  if ((int)map->levels.size() > kGnMaxLevels) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d pyramid levels", kGnMaxLevels);
  size_t total = 0;
  for (int k = 0; k < n_containers; k++) {
    const int n = n_points[k];
    if (n < 0) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: container %d has a negative point count (%d)", who, k, n);
    if (n > kMaxBeams) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per scan are supported (got %d)", kMaxBeams, n);
    if (map->ordered_sums && (size_t)n * 9 * sizeof(float) > 150 * 1024)
      return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per scan in matchData", (int)(150 * 1024 / 36));
    total += (size_t)n;
  }
  if (total > (size_t)INT32_MAX / 2) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "batch too large");
  if (total > 0 && !points_xy) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: points_xy is required", who);
  if (entry_container)
    for (int e = 0; e < n_entries; e++)
      if (entry_container[e] < 0 || entry_container[e] >= n_containers)
        return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: entry %d names container %d of %d", who, e, entry_container[e], n_containers);
  *total_out = total;
  return LSLAM_OK;
}

int match_batch_launch(lslam_map* map, int n_entries, int n_containers, const float* d_pts, const int32_t* n_points,
                       const int32_t* entry_container, const float* d_begin, float* d_pose, float* d_cov) {
  lslam_context* ctx = map->ctx;
  {
    int rc = flush_pending(map);  // the matcher reads the float planes
    if (rc) return rc;
  }
  std::vector<int> first((size_t)n_containers + 1, 0);
  int n_max = 0;
  for (int k = 0; k < n_containers; k++) {
    first[k + 1] = first[k] + n_points[k];
    n_max = std::max(n_max, n_points[k]);
  }
  std::vector<int2> ent((size_t)n_entries);
  for (int e = 0; e < n_entries; e++) {
    const int k = entry_container ? entry_container[e] : e;
    ent[e] = make_int2(first[k], n_points[k]);
  }
  LSLAM_HIP(ctx, map->d_gnb_ent.reserve((size_t)n_entries));
  // (pageable source: the runtime has staged it when the call returns, like the batched update's scan headers)
  LSLAM_HIP(ctx, hipMemcpyAsync(map->d_gnb_ent.p, ent.data(), ent.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
  const GnLevels lv = gn_levels_of(map);
  const int2* d_ent = map->d_gnb_ent.p;
  if (map->ordered_sums) {
    const size_t lds = (size_t)std::max(n_max, 1) * 9 * sizeof(float);
    if (lds > 64 * 1024)
      LSLAM_HIP(ctx, hipFuncSetAttribute((const void*)k_gn_match_batch_ordered, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    launch(ctx, "gn_match_batch", k_gn_match_batch_ordered, dim3((unsigned)n_entries), dim3(n_max > 512 ? 1024 : 256), lds, lv,
           d_pts, d_ent, d_begin, d_pose, d_cov);
  } else {
    launch(ctx, "gn_match_batch", k_gn_match_batch, dim3((unsigned)((n_entries + kGnBatchWaves - 1) / kGnBatchWaves)),
           dim3(64 * kGnBatchWaves), 0, lv, d_pts, d_ent, d_begin, n_entries, d_pose, d_cov);
  }
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}
}  // namespace

int lslam_map_match_batch_dev(lslam_map* map, int n_entries, int n_containers, const float* points_xy_dev, const int32_t* n_points,
                              const int32_t* entry_container, const float* begin_world_dev, float* out_poses_dev,
                              float* out_covs_dev) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  size_t total = 0;
  int rc = match_batch_check(map, "lslam_map_match_batch_dev", n_entries, n_containers, points_xy_dev, n_points, entry_container,
                             begin_world_dev, out_poses_dev, &total);
  if (rc || n_entries == 0) return rc;
  LSLAM_HIP(map->ctx, hipSetDevice(map->ctx->device));
  return match_batch_launch(map, n_entries, n_containers, points_xy_dev, n_points, entry_container, begin_world_dev, out_poses_dev,
                            out_covs_dev);
}

int lslam_map_match_batch(lslam_map* map, int n_entries, int n_containers, const float* points_xy, const int32_t* n_points,
                          const int32_t* entry_container, const float* begin_world, float* out_poses, float* out_covs) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  size_t total = 0;
  int rc = match_batch_check(map, "lslam_map_match_batch", n_entries, n_containers, points_xy, n_points, entry_container, begin_world,
                             out_poses, &total);
  if (rc || n_entries == 0) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = stage_points(map, points_xy, (int)total);  // -> d_pts (a staging buffer of the updates; not the cached container)
  if (rc) return rc;
  const size_t B = (size_t)n_entries;
  LSLAM_HIP(ctx, map->d_gnb_io.reserve(15 * B));
  float* d_begin = map->d_gnb_io.p;
  float* d_pose = d_begin + 3 * B;
  float* d_cov = d_pose + 3 * B;
  LSLAM_HIP(ctx, hipMemcpyAsync(d_begin, begin_world, 3 * B * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  rc = match_batch_launch(map, n_entries, n_containers, map->d_pts.p, n_points, entry_container, d_begin, d_pose,
                          out_covs ? d_cov : (float*)nullptr);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(out_poses, d_pose, 3 * B * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (out_covs) LSLAM_HIP(ctx, hipMemcpyAsync(out_covs, d_cov, 9 * B * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // one wait for the whole batch
  return LSLAM_OK;
}

namespace {
// ---- pose scoring (k_ms_*).  Like the batched match: everything that can be refused is refused before anything is enqueued
// or written, and nothing here touches a plane, d_cached or n_cached.
constexpr int kMsMaxStates = 1 << 24;  // per call (the lattice's volume, 7 x the covariance entries)

int score_level_check(lslam_map* map, const char* who, int level) {
  lslam_context* ctx = map->ctx;
  if (level < 0 || level >= (int)map->levels.size())
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: level %d is outside the pyramid (%d levels)", who, level, (int)map->levels.size());
  if (map->levels[level].sx < 2 || map->levels[level].sy < 2)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: level %d is smaller than 2 x 2 cells", who, level);
  return LSLAM_OK;
}

int score_check(lslam_map* map, const char* who, int n_entries, int states_per_entry, int n_containers, const void* points_xy,
                const int32_t* n_points, const int32_t* entry_container, const void* poses_world, const void* out, int level,
                size_t* total_out) {
  lslam_context* ctx = map->ctx;
  if (n_entries < 0 || n_containers < 0)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: negative count (n_entries %d, n_containers %d)", who, n_entries, n_containers);
  *total_out = 0;
  if (n_entries == 0) return LSLAM_OK;
  if (!poses_world || !out) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: poses_world and the likelihood output are required", who);
  if (n_containers > 0 && !n_points) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: n_points is required", who);
  if (!entry_container && n_containers != n_entries)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: without entry_container entry i uses container i, so n_containers (%d) must equal n_entries (%d)",
                     who, n_containers, n_entries);
  {
    int rc = score_level_check(map, who, level);
    if (rc) return rc;
  }
  if (n_entries > kMsMaxStates / states_per_entry)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d entries per call", who, kMsMaxStates / states_per_entry);
  size_t total = 0;
  for (int k = 0; k < n_containers; k++) {
    const int n = n_points[k];
    if (n < 0) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: container %d has a negative point count (%d)", who, k, n);
    if (n > kMaxBeams) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per scan are supported (got %d)", kMaxBeams, n);
    total += (size_t)n;
  }
  if (total > (size_t)INT32_MAX / 2) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "batch too large");
  if (total > 0 && !points_xy) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: points_xy is required", who);
  if (entry_container)
    for (int e = 0; e < n_entries; e++)
      if (entry_container[e] < 0 || entry_container[e] >= n_containers)
        return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: entry %d names container %d of %d", who, e, entry_container[e], n_containers);
  *total_out = total;
  return LSLAM_OK;
}

MsJob score_job(const lslam_map* map, int level, int mode, int n_states) {
  const Level& L = map->levels[level];
  MsJob J{};
  J.mode = mode; J.n_states = n_states;
  J.lo = L.d_logodds; J.sx = L.sx; J.sy = L.sy;
  J.scale = L.scale_to_map; J.t_x = L.t_x; J.t_y = L.t_y; J.cell_length = L.cell_length;
  J.factor = level == 0 ? 1.0f : 1.0f / (float)(1 << level);  // DataContainer::setFrom (MapRepMultiMap.h:161), as the matcher
  return J;
}

// the entry table (first point, points) of a batch -> d_gnb_ent
int score_entries(lslam_map* map, int n_entries, int n_containers, const int32_t* n_points, const int32_t* entry_container) {
  lslam_context* ctx = map->ctx;
  std::vector<int> first((size_t)n_containers + 1, 0);
  for (int k = 0; k < n_containers; k++) first[k + 1] = first[k] + n_points[k];
  std::vector<int2> ent((size_t)n_entries);
  for (int e = 0; e < n_entries; e++) {
    const int k = entry_container ? entry_container[e] : e;
    ent[e] = make_int2(first[k], n_points[k]);
  }
  LSLAM_HIP(ctx, map->d_gnb_ent.reserve((size_t)n_entries));
  LSLAM_HIP(ctx, hipMemcpyAsync(map->d_gnb_ent.p, ent.data(), ent.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
  return LSLAM_OK;
}

int score_launch(lslam_map* map, const MsJob& J, const float* d_pts) {
  lslam_context* ctx = map->ctx;
  if (map->ordered_sums) {
    launch(ctx, "ms_score", k_ms_score_ordered, dim3((unsigned)J.n_states), dim3(256), 0, J, d_pts);
  } else {
    const dim3 grid((unsigned)((J.n_states + kMsWaves - 1) / kMsWaves)), block(64 * kMsWaves);
    if (map->score_chunk == 2) launch(ctx, "ms_score", k_ms_score<2>, grid, block, 0, J, d_pts);
    else if (map->score_chunk == 8) launch(ctx, "ms_score", k_ms_score<8>, grid, block, 0, J, d_pts);
    else launch(ctx, "ms_score", k_ms_score<4>, grid, block, 0, J, d_pts);
  }
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}

int score_batch_launch(lslam_map* map, int n_entries, int n_containers, const float* d_pts, const int32_t* n_points,
                       const int32_t* entry_container, const float* d_poses, int level, float* d_res, float* d_lik) {
  int rc = flush_pending(map);  // the kernels read the float planes
  if (rc) return rc;
  rc = score_entries(map, n_entries, n_containers, n_points, entry_container);
  if (rc) return rc;
  MsJob J = score_job(map, level, kMsBatch, n_entries);
  J.poses = d_poses; J.ent = map->d_gnb_ent.p; J.out_res = d_res; J.out_lik = d_lik;
  return score_launch(map, J, d_pts);
}

int score_cov_launch(lslam_map* map, int n_entries, int n_containers, const float* d_pts, const int32_t* n_points,
                     const int32_t* entry_container, const float* d_poses, int level, float* d_lik, float* d_cov_map,
                     float* d_cov_world) {
  lslam_context* ctx = map->ctx;
  int rc = flush_pending(map);
  if (rc) return rc;
  rc = score_entries(map, n_entries, n_containers, n_points, entry_container);
  if (rc) return rc;
  MsJob J = score_job(map, level, kMsCov, 7 * n_entries);
  J.poses = d_poses; J.ent = map->d_gnb_ent.p; J.out_lik = d_lik;
  rc = score_launch(map, J, d_pts);
  if (rc || (!d_cov_map && !d_cov_world)) return rc;
  launch(ctx, "ms_cov", k_ms_cov, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, J, n_entries, (const float*)d_lik,
         d_cov_map, d_cov_world);
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}

int score_lattice_check(lslam_map* map, const char* who, const void* points_xy, int n, const float* centre_world,
                        const int32_t* counts, const float* steps, int level, const void* out_volume, int* n_states) {
  lslam_context* ctx = map->ctx;
  if (n < 0 || (n > 0 && !points_xy) || !centre_world || !counts || !steps || !out_volume)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: points_xy, centre_world, counts, steps and out_volume are required", who);
  if (counts[0] <= 0 || counts[1] <= 0 || counts[2] <= 0)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: lattice counts must be positive (got %d x %d x %d)", who, counts[0], counts[1], counts[2]);
  int rc = score_level_check(map, who, level);
  if (rc) return rc;
  if (n > kMaxBeams) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "at most %d points per scan are supported (got %d)", kMaxBeams, n);
  const long long states = (long long)counts[0] * counts[1] * counts[2];
  if (counts[0] > kMsMaxStates || counts[1] > kMsMaxStates || (long long)counts[0] * counts[1] > kMsMaxStates || states > kMsMaxStates)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d lattice states per call", who, kMsMaxStates);
  *n_states = (int)states;
  return LSLAM_OK;
}

int score_lattice_launch(lslam_map* map, const float* d_pts, int n, const float* centre_world, const int32_t* counts,
                         const float* steps, int level, int n_states, float* d_volume, int* d_best_index, float* d_best_lik) {
  lslam_context* ctx = map->ctx;
  int rc = flush_pending(map);
  if (rc) return rc;
  MsJob J = score_job(map, level, kMsLattice, n_states);
  J.first = 0; J.n = n;
  J.c0 = centre_world[0]; J.c1 = centre_world[1]; J.c2 = centre_world[2];
  J.d0 = steps[0]; J.d1 = steps[1]; J.d2 = steps[2];
  J.nx = counts[0]; J.ny = counts[1]; J.nt = counts[2];
  J.out_lik = d_volume;
  rc = score_launch(map, J, d_pts);
  if (rc || (!d_best_index && !d_best_lik)) return rc;
  launch(ctx, "ms_best", k_ms_best, dim3(1), dim3(1024), 0, (const float*)d_volume, n_states, d_best_index, d_best_lik);
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}
}  // namespace

int lslam_map_score_batch_dev(lslam_map* map, int n_entries, int n_containers, const float* points_xy_dev, const int32_t* n_points,
                              const int32_t* entry_container, const float* poses_world_dev, int level, float* out_residual_dev,
                              float* out_likelihood_dev) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  size_t total = 0;
  int rc = score_check(map, "lslam_map_score_batch_dev", n_entries, 1, n_containers, points_xy_dev, n_points, entry_container,
                       poses_world_dev, out_likelihood_dev, level, &total);
  if (rc || n_entries == 0) return rc;
  LSLAM_HIP(map->ctx, hipSetDevice(map->ctx->device));
  return score_batch_launch(map, n_entries, n_containers, points_xy_dev, n_points, entry_container, poses_world_dev, level,
                            out_residual_dev, out_likelihood_dev);
}

int lslam_map_score_batch(lslam_map* map, int n_entries, int n_containers, const float* points_xy, const int32_t* n_points,
                          const int32_t* entry_container, const float* poses_world, int level, float* out_residual,
                          float* out_likelihood) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  size_t total = 0;
  int rc = score_check(map, "lslam_map_score_batch", n_entries, 1, n_containers, points_xy, n_points, entry_container, poses_world,
                       out_likelihood, level, &total);
  if (rc || n_entries == 0) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = stage_points(map, points_xy, (int)total);  // -> d_pts (a staging buffer of the updates; not the cached container)
  if (rc) return rc;
  const size_t B = (size_t)n_entries;
  LSLAM_HIP(ctx, map->d_score_io.reserve(5 * B));
  float* d_poses = map->d_score_io.p;
  float* d_res = d_poses + 3 * B;
  float* d_lik = d_res + B;
  LSLAM_HIP(ctx, hipMemcpyAsync(d_poses, poses_world, 3 * B * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  rc = score_batch_launch(map, n_entries, n_containers, map->d_pts.p, n_points, entry_container, d_poses, level, d_res, d_lik);
  if (rc) return rc;
  if (out_residual) LSLAM_HIP(ctx, hipMemcpyAsync(out_residual, d_res, B * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(out_likelihood, d_lik, B * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // one wait for the whole batch
  return LSLAM_OK;
}

int lslam_map_pose_covariance_batch_dev(lslam_map* map, int n_entries, int n_containers, const float* points_xy_dev,
                                        const int32_t* n_points, const int32_t* entry_container, const float* poses_world_dev,
                                        int level, float* out_likelihoods_dev, float* out_cov_map_dev, float* out_cov_world_dev) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  size_t total = 0;
  int rc = score_check(map, "lslam_map_pose_covariance_batch_dev", n_entries, 7, n_containers, points_xy_dev, n_points,
                       entry_container, poses_world_dev, out_likelihoods_dev, level, &total);
  if (rc || n_entries == 0) return rc;
  LSLAM_HIP(map->ctx, hipSetDevice(map->ctx->device));
  return score_cov_launch(map, n_entries, n_containers, points_xy_dev, n_points, entry_container, poses_world_dev, level,
                          out_likelihoods_dev, out_cov_map_dev, out_cov_world_dev);
}

int lslam_map_pose_covariance_batch(lslam_map* map, int n_entries, int n_containers, const float* points_xy, const int32_t* n_points,
                                    const int32_t* entry_container, const float* poses_world, int level, float* out_likelihoods,
                                    float* out_cov_map, float* out_cov_world) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  size_t total = 0;
  int rc = score_check(map, "lslam_map_pose_covariance_batch", n_entries, 7, n_containers, points_xy, n_points, entry_container,
                       poses_world, out_likelihoods, level, &total);
  if (rc || n_entries == 0) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = stage_points(map, points_xy, (int)total);
  if (rc) return rc;
  const size_t B = (size_t)n_entries;
  LSLAM_HIP(ctx, map->d_score_io.reserve(28 * B));
  float* d_poses = map->d_score_io.p;
  float* d_lik = d_poses + 3 * B;
  float* d_cm = d_lik + 7 * B;
  float* d_cw = d_cm + 9 * B;
  LSLAM_HIP(ctx, hipMemcpyAsync(d_poses, poses_world, 3 * B * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  rc = score_cov_launch(map, n_entries, n_containers, map->d_pts.p, n_points, entry_container, d_poses, level, d_lik,
                        out_cov_map ? d_cm : (float*)nullptr, out_cov_world ? d_cw : (float*)nullptr);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(out_likelihoods, d_lik, 7 * B * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (out_cov_map) LSLAM_HIP(ctx, hipMemcpyAsync(out_cov_map, d_cm, 9 * B * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (out_cov_world) LSLAM_HIP(ctx, hipMemcpyAsync(out_cov_world, d_cw, 9 * B * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSLAM_OK;
}

int lslam_map_score_lattice_dev(lslam_map* map, const float* points_xy_dev, int n, const float centre_world[3],
                                const int32_t counts[3], const float steps[3], int level, float* out_volume_dev,
                                int32_t* out_best_index_dev, float* out_best_likelihood_dev) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  int n_states = 0;
  int rc = score_lattice_check(map, "lslam_map_score_lattice_dev", points_xy_dev, n, centre_world, counts, steps, level,
                               out_volume_dev, &n_states);
  if (rc) return rc;
  LSLAM_HIP(map->ctx, hipSetDevice(map->ctx->device));
  return score_lattice_launch(map, points_xy_dev, n, centre_world, counts, steps, level, n_states, out_volume_dev,
                              out_best_index_dev, out_best_likelihood_dev);
}

int lslam_map_score_lattice(lslam_map* map, const float* points_xy, int n, const float centre_world[3], const int32_t counts[3],
                            const float steps[3], int level, float* out_volume, int32_t* out_best_index,
                            float* out_best_likelihood) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  int n_states = 0;
  int rc = score_lattice_check(map, "lslam_map_score_lattice", points_xy, n, centre_world, counts, steps, level, out_volume, &n_states);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = stage_points(map, points_xy, n);
  if (rc) return rc;
  const size_t N = (size_t)n_states;
  LSLAM_HIP(ctx, map->d_score_io.reserve(N + 2));
  float* d_vol = map->d_score_io.p;
  int* d_bi = reinterpret_cast<int*>(d_vol + N);
  float* d_bl = d_vol + N + 1;
  rc = score_lattice_launch(map, map->d_pts.p, n, centre_world, counts, steps, level, n_states, d_vol, d_bi, d_bl);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(out_volume, d_vol, N * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (out_best_index) LSLAM_HIP(ctx, hipMemcpyAsync(out_best_index, d_bi, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (out_best_likelihood) LSLAM_HIP(ctx, hipMemcpyAsync(out_best_likelihood, d_bl, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSLAM_OK;
}

int lslam_map_set_option(lslam_map* map, int option, int value) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  if (option == LSLAM_MAP_OPT_ORDERED_SUMS) {
    map->ordered_sums = value != 0;
    return LSLAM_OK;
  }
  if (option == LSLAM_MAP_OPT_BATCH_SCRATCH_MB) {
    if (value < 1) return map->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "batch scratch budget must be >= 1 MB");
    map->batch_budget = (size_t)value << 20;
    return LSLAM_OK;
  }
  if (option == LSLAM_MAP_OPT_BATCH_RADIUS_CELLS) {
    if (value < 0) return map->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "batch radius hint must be >= 0 (0 = none)");
    map->batch_radius_hint = value;
    return LSLAM_OK;
  }
  return map->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "unknown map option %d", option);
}

int lslam_map_cached_points(const lslam_map* map) { return map ? map->n_cached : LSLAM_ERR_INVALID_ARGUMENT; }

int lslam_map_read_logodds(lslam_map* map, int level, float* out) {
  if (!map || !out || level < 0 || level >= (int)map->levels.size()) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  Level& L = map->levels[level];
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  {
    int rc = flush_pending(map);
    if (rc) return rc;
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(out, L.d_logodds, (size_t)L.sx * L.sy * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSLAM_OK;
}

int lslam_map_read_occupancy_i8(lslam_map* map, int level, int8_t* out) {
  if (!map || !out || level < 0 || level >= (int)map->levels.size()) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  Level& L = map->levels[level];
  size_t n = (size_t)L.sx * L.sy;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  {
    int rc = flush_pending(map);
    if (rc) return rc;
  }
  LSLAM_HIP(ctx, map->d_i8.reserve(n));
  launch(ctx, "occupancy_i8", k_occupancy_i8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
         (const float*)L.d_logodds, map->d_i8.p, n);
  LSLAM_HIP(ctx, hipMemcpyAsync(out, map->d_i8.p, n, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSLAM_OK;
}

void* lslam_map_cells_dev_ptr(lslam_map* map, int level) {
  if (!map || level < 0 || level >= (int)map->levels.size()) return nullptr;
  if (lslam_map_flush(map) != LSLAM_OK) return nullptr;  // a plane that lacks the last scan's apply is not handed out (lslam_last_error says why)
  return map->levels[level].d_logodds;
}

// The inverse of the two readers above.  Only the float plane changes.  The key planes stay: a key is (epoch << 16 | beam) of
// the scan that set it, a scan reads a key as "touched by me" only where its epoch is the scan's own, and the next scan's
// epoch is larger than every epoch in the planes (clear_marks zeroes them where the epochs wrap) -- so after the pending apply
// below has gone out, every cell is untouched for whatever scan comes next, as in the reference's map after a completed
// updateByScan (updateIndex < currMarkFreeIndex everywhere).
int lslam_map_write_logodds(lslam_map* map, int level, const float* src) {
  if (!map || !src || level < 0 || level >= (int)map->levels.size()) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  Level& L = map->levels[level];
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  {
    int rc = flush_pending(map);
    if (rc) return rc;
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(L.d_logodds, src, (size_t)L.sx * L.sy * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // src is the caller's again
  return LSLAM_OK;
}

int lslam_map_write_logodds_dev(lslam_map* map, int level, const float* src_dev) {
  if (!map || !src_dev || level < 0 || level >= (int)map->levels.size()) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  Level& L = map->levels[level];
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, src_dev) != hipSuccess) {  // an address the runtime has never heard of: host memory
    (void)hipGetLastError();
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_map_write_logodds_dev: the source is not device memory");
  }
  if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_map_write_logodds_dev: the source is not device memory");
  if (src_dev == L.d_logodds) return flush_pending(map);  // a plane written onto itself
  {
    int rc = flush_pending(map);
    if (rc) return rc;
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(L.d_logodds, src_dev, (size_t)L.sx * L.sy * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  return LSLAM_OK;
}

// Enqueue whatever a single-scan update still owes the float planes (the deferred apply of the pipelined path).
// lslam_map_read_*, lslam_map_match_*, the batched update and lslam_synchronize do this themselves; a caller that reads
// the plane behind lslam_map_cells_dev_ptr from its OWN stream calls it before recording its event on lslam_stream().
#if defined(LSLAM_PHASE_STAMPS)
// diagnostic builds only: out[kernel][8 cycle sums | 8 visit counts] of this translation unit's stamp table (summed over the
// wave slots); reset != 0 clears it
int lslam_debug_map_stamps(lslam_context* ctx, unsigned long long* out, int reset) {
  if (!ctx || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t n = (size_t)lslam::kStampKernels * lslam::kStampSlots * 16;
  std::vector<unsigned long long> h(n);
  LSLAM_HIP(ctx, hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_map_stamps_slots), n * sizeof(unsigned long long)));
  for (int k = 0; k < lslam::kStampKernels; k++)
    for (int i = 0; i < 16; i++) {
      unsigned long long sum = 0;
      for (int sl = 0; sl < lslam::kStampSlots; sl++) sum += h[((size_t)k * lslam::kStampSlots + sl) * 16 + i];
      out[k * 16 + i] = sum;
    }
  if (reset) {
    std::fill(h.begin(), h.end(), 0ull);
    LSLAM_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_map_stamps_slots), h.data(), n * sizeof(unsigned long long)));
  }
  return LSLAM_OK;
}
#endif

int lslam_map_flush(lslam_map* map) {
  if (!map) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = map->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  return flush_pending(map);
}

}  // extern "C"


// ------------------------------------------------------------------------------------------
// lslam_hector_*: the streamed HectorSlamProcessor (device side: k_hs_* above)
// ------------------------------------------------------------------------------------------
namespace {

// The input of a call on its way up: ONE pinned staging buffer and the device buffers it feeds (hs_stage_* below), owned once
// by a processor and once by a fleet.  Every call ends in a wait, so nothing is in flight when the next call reuses or
// regrows any of them.
struct HsStage {
  float* h_in = nullptr;    // pinned: ranges; or points, then counts; or [xyz | take words | valid bytes]
  size_t h_in_cap = 0;
  DevBuf<float> d_in;       // ranges; the fleet's points (the single processor's land in its map's d_pts)
  DevBuf<float> d_xyz;      // clouds: staged from the host, or what the de-skew in front of the processor wrote
  DevBuf<uint8_t> d_valid;
  DevBuf<int32_t> d_take;
  DevBuf<int> d_counts;
  void release() {
    if (h_in) (void)hipHostFree(h_in);
    h_in = nullptr;
    h_in_cap = 0;
    d_in.release();
    d_xyz.release();
    d_valid.release();
    d_take.release();
    d_counts.release();
  }
};

}  // namespace

struct lslam_hector {
  lslam_map* map = nullptr;
  float min_dist = 0.4f, min_angle = 0.13f;  // HectorSlamProcessor.h:66-67
  int fabs_gate = 0;
  HsState* d_state = nullptr;
  // host mirror of HsState's persistent words, and their pinned way up and down (one copy each per call)
  HsState mirror;
  uint32_t* h_io = nullptr;  // [2][kHsPersistWords]
  lslam_hector_record* h_rec = nullptr;
  size_t h_rec_cap = 0;
  DevBuf<lslam_hector_record> d_rec;
  HsStage in;
  // de-skewed form: the batched lesson5 stage in front (created with the first such call); its cloud goes to in.d_xyz
  lslam_deskew* deskew = nullptr;
  // synced form: the walk's lslam_msync_records with their pinned way down
  DevBuf<lslam_msync_record> d_msrec;
  lslam_msync_record* h_msrec = nullptr;
  size_t h_msrec_cap = 0;
  int64_t n_scans = 0, n_updates = 0, n_calls = 0, n_syncs = 0;
};

namespace {

// HectorSlamProcessor::reset (:111-117): lastMapUpdatePose and lastScanMatchPose; lastScanMatchCov stays what it was
void hs_reset_state(lslam_hector* h) {
  for (int q = 0; q < 3; q++) {
    h->mirror.update_pose[q] = FLT_MAX;
    h->mirror.match_pose[q] = 0.0f;
  }
}

template <typename T>
int hs_pinned_reserve(lslam_context* ctx, T** p, size_t* cap, size_t want) {
  if (want <= *cap) return LSLAM_OK;
  if (*p) (void)hipHostFree(*p);  // (every call ends with a synchronise: nothing in flight reads it)
  *p = nullptr;
  *cap = 0;
  const size_t n = want + want / 4 + 16;
  LSLAM_HIP(ctx, hipHostMalloc((void**)p, n * sizeof(T), hipHostMallocDefault));
  *cap = n;
  return LSLAM_OK;
}

// rows x n_readings ranges, `stride` floats apart at the caller's -> s.d_in, packed
int hs_stage_ranges(lslam_context* ctx, HsStage& s, size_t rows, int n_readings, const float* ranges, size_t stride) {
  const size_t total = rows * (size_t)n_readings;
  LSLAM_HIP(ctx, s.d_in.reserve(std::max(total, (size_t)1)));
  int rc = hs_pinned_reserve(ctx, &s.h_in, &s.h_in_cap, std::max(total, (size_t)1));
  if (rc || total == 0) return rc;
  for (size_t i = 0; i < rows; i++) memcpy(s.h_in + i * n_readings, ranges + i * stride, (size_t)n_readings * sizeof(float));
  LSLAM_HIP(ctx, hipMemcpyAsync(s.d_in.p, s.h_in, total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  return LSLAM_OK;
}

// rows clouds of n_points -> s.d_xyz; their valid bytes (null: none) -> s.d_valid; their take flags (null: none), widened to
// the int32 words the gated chain reads -> s.d_take
int hs_stage_clouds(lslam_context* ctx, HsStage& s, size_t rows, int n_points, const float* xyz, const uint8_t* valid,
                    const uint8_t* take) {
  const size_t total = rows * (size_t)n_points;
  const size_t o_take = 3 * total, o_valid = o_take + rows, words = o_valid + (total + 3) / 4;  // pinned: [xyz | take | valid]
  LSLAM_HIP(ctx, s.d_xyz.reserve(std::max(3 * total, (size_t)1)));
  if (valid) LSLAM_HIP(ctx, s.d_valid.reserve(std::max(total, (size_t)1)));
  if (take) LSLAM_HIP(ctx, s.d_take.reserve(rows));
  int rc = hs_pinned_reserve(ctx, &s.h_in, &s.h_in_cap, words);
  if (rc) return rc;
  if (total > 0) {
    memcpy(s.h_in, xyz, 3 * total * sizeof(float));
    LSLAM_HIP(ctx, hipMemcpyAsync(s.d_xyz.p, s.h_in, 3 * total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (valid) {
      memcpy(s.h_in + o_valid, valid, total);
      LSLAM_HIP(ctx, hipMemcpyAsync(s.d_valid.p, s.h_in + o_valid, total, hipMemcpyHostToDevice, ctx->stream));
    }
  }
  if (take) {
    int32_t* t = reinterpret_cast<int32_t*>(s.h_in + o_take);
    for (size_t i = 0; i < rows; i++) t[i] = take[i] ? 1 : 0;
    LSLAM_HIP(ctx, hipMemcpyAsync(s.d_take.p, t, rows * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  return LSLAM_OK;
}

// `total` packed points -> d_pts (the caller's: the map's own buffer, or s.d_in), then their rows counts -> s.d_counts.
// (stage_points' ring waits for a busy slot and drains the stream when it grows; this buffer is never in flight here.)
int hs_stage_points(lslam_context* ctx, HsStage& s, DevBuf<float>& d_pts, size_t rows, const float* points_xy,
                    const int32_t* n_points, size_t total) {
  int rc = hs_pinned_reserve(ctx, &s.h_in, &s.h_in_cap, 2 * total + rows);
  if (rc) return rc;
  LSLAM_HIP(ctx, d_pts.reserve(std::max((size_t)2 * total, (size_t)2)));
  LSLAM_HIP(ctx, s.d_counts.reserve(rows));
  if (total > 0) {
    memcpy(s.h_in, points_xy, 2 * total * sizeof(float));
    LSLAM_HIP(ctx, hipMemcpyAsync(d_pts.p, s.h_in, 2 * total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  memcpy(s.h_in + 2 * total, n_points, rows * sizeof(int32_t));
  LSLAM_HIP(ctx, hipMemcpyAsync(s.d_counts.p, s.h_in + 2 * total, rows * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  return LSLAM_OK;
}

// the de-skew handle in front of a processor or a fleet: made by the first call that needs it
int hs_ensure_deskew(lslam_context* ctx, lslam_deskew** deskew) { return *deskew ? LSLAM_OK : lslam_deskew_create(ctx, deskew); }

// ---- argument checks that several entry points share
bool hs_ranges_given(const lslam_hector_scan* scan, int n_readings, const float* ranges, int ranges_stride) {
  return scan && (n_readings == 0 || (ranges && ranges_stride >= n_readings));
}

int hs_check_stride(lslam_context* ctx, const char* who, int ranges_stride, int n_readings) {
  if (ranges_stride < n_readings) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: ranges_stride >= n_readings is required", who);
  return LSLAM_OK;
}

// the counts of a container-form call -> their sum and the largest; `active` (null: every scan is) is the fleet's
int hs_check_counts(lslam_context* ctx, const char* who, size_t rows, const int32_t* n_points, const uint8_t* active,
                    const float* points_xy, size_t* total, int* cap) {
  *total = 0;
  *cap = 0;
  for (size_t i = 0; i < rows; i++) {
    if (n_points[i] < 0)
      return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: scan %zu has a negative point count (%d)", who, i, n_points[i]);
    if (active && !active[i] && n_points[i] != 0)
      return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: scan %zu is not active but has %d points", who, i, n_points[i]);
    *total += (size_t)n_points[i];
    *cap = std::max(*cap, n_points[i]);
  }
  if (*total > 0 && !points_xy) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: points_xy is required", who);
  return LSLAM_OK;
}

// what every form refuses before anything touches the device
int hs_check(lslam_hector* h, const char* who, int capacity) {
  lslam_map* map = h->map;
  lslam_context* ctx = map->ctx;
  if (map->ordered_sums)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: the streamed processor runs the parallel-sum matcher; LSLAM_MAP_OPT_ORDERED_SUMS "
                     "maps go through lslam_map_match_data / lslam_map_update_by_scan", who);
  if ((int)map->levels.size() > kGnMaxLevels) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d pyramid levels", who, kGnMaxLevels);
  if (capacity > kMaxBeams || map->n_cached > kMaxBeams)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d points per scan are supported (got %d)", who, kMaxBeams,
                     std::max(capacity, map->n_cached));
  return LSLAM_OK;
}

struct HsCall {
  int n_scans = 0, capacity = 0;
  const lslam_hector_scan* scan = nullptr;   // ranges form: project scan k's readings into the map's resident container
  int n_readings = 0;
  struct {                                   // cloud forms (xyz set): scan k's cloud in HBM goes there instead
    const float* xyz = nullptr;
    const uint8_t* valid = nullptr;          //   null: every point is valid
    const int32_t* take = nullptr;           //   gated chain: scan k is taken iff take[k * take_stride] > 0 (null: every scan)
    int take_stride = 0;
  } cloud;
  bool gated = false;                        // the cloud goes through the gated chain (clouds and synced forms)
  lslam_msync* sync = nullptr;               // synced form: the handle whose walk wrote the take words, and where its
  lslam_msync_record* sync_out = nullptr;    //   records (h->d_msrec) go when they come down with the processor's
  const float* d_points = nullptr;           // container form: the packed points in HBM,
  const int32_t* n_points = nullptr;         //   their host counts (offsets) and
  const float* origos = nullptr;             //   origos (may be null)
  const float* hints = nullptr;
  const uint8_t* no_match = nullptr;
  lslam_hector_record* out = nullptr;
};

// the call of every form that fills the map's resident container from n_scans scans of n_readings readings (or points)
HsCall hs_scan_call(const lslam_hector_scan* scan, int n_scans, int n_readings, const float* hints, const uint8_t* no_match,
                    lslam_hector_record* out) {
  HsCall c;
  c.n_scans = n_scans;
  c.capacity = n_readings;
  c.scan = scan;
  c.n_readings = n_readings;
  c.hints = hints;
  c.no_match = no_match;
  c.out = out;
  return c;
}

// the resident container of lslam_map_set_scan, with room for n points
hipError_t hs_reserve_scan(lslam_map* map, int n) { return map->d_scan.reserve((size_t)2 * std::max(n, 1) + 4); }

// ---- what a processor and the host side of its map hand to a call and take back from it, alone (hs_run) or in a fleet (hf_run)

// state up: the processor's vectors are in its mirror; the cached container's count and origo come from the map (a call of
// another handle on it, or a host-driven matchData, may have replaced it since)
void hs_state_up(lslam_hector* h) {
  const lslam_map* map = h->map;
  h->mirror.n_cached = map->n_cached;
  h->mirror.cached_origo[0] = map->cached_origo[0];
  h->mirror.cached_origo[1] = map->cached_origo[1];
  h->mirror.updated = 0;
}

// state down: `words` are the kHsPersistWords that came back; with them, what the host side of the map must know so that
// every lslam_map_* call goes on working on it.  n_taken: the scans of the call that the processor took.  keep_untaken: a
// processor that took none stays as it was (a fleet's member: its block came back as it went up, but for `updated`, which is
// the call's); the single processor always takes its block back.  scan_origo: the origo of the call's projected scans, null
// in the container form; the resident container of lslam_map_set_scan is the last TAKEN scan's.
void hs_state_down(lslam_hector* h, const void* words, int n_taken, bool keep_untaken, const float* scan_origo) {
  if (keep_untaken && n_taken == 0) return;
  lslam_map* map = h->map;
  memcpy(&h->mirror, words, kHsPersistWords * 4);
  if (map->levels.size() > 1) {  // (as match_data_impl: a single-level map keeps no cached container)
    map->n_cached = h->mirror.n_cached;
    map->cached_origo[0] = h->mirror.cached_origo[0];
    map->cached_origo[1] = h->mirror.cached_origo[1];
  }
  map->gn_host_n = -1;  // d_cached was rewritten on the device
  if (scan_origo && n_taken > 0) {
    map->n_scan = h->mirror.n_live;
    map->scan_origo[0] = scan_origo[0];
    map->scan_origo[1] = scan_origo[1];
  }
}

// dataContainer.setOrigo(Eigen::Vector2f(laserPos.x(), laserPos.y()) * scaleToMap) (hector_slam.cc:331)
void hs_scan_origo(const lslam_hector_scan* scan, const ProjectCfg& pc, float origo[2]) {
  origo[0] = (float)(double)scan->laser_x * pc.scale_to_map;
  origo[1] = (float)(double)scan->laser_y * pc.scale_to_map;
}

// one record into its processor's counters -> whether the scan was taken (the gated chain marks the record of one it did not
// take with n_points = -1, and updated = 0)
bool hs_count_record(lslam_hector* h, const lslam_hector_record& r) {
  if (r.n_points < 0) return false;
  h->n_scans++;
  h->n_updates += r.updated != 0;
  return true;
}

// the cached container must survive a growth of its buffer (levels above 0 of a scan taken without matching read it);
// *cache_cap: the points either container of a scan of this call may hold
int hs_reserve_cached(lslam_map* map, int capacity, int* cache_cap) {
  lslam_context* ctx = map->ctx;
  *cache_cap = std::max(std::max(capacity, map->n_cached), 1);
  const float* old = map->d_cached.p;
  LSLAM_HIP(ctx, map->d_cached.reserve((size_t)2 * *cache_cap));
  if (old && old != map->d_cached.p && map->n_cached > 0)
    LSLAM_HIP(ctx, hipMemcpyAsync(map->d_cached.p, old, (size_t)2 * map->n_cached * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  return LSLAM_OK;
}

HsLevels hs_levels_of(const lslam_map* map) {  // the pyramid as the streamed update's kernels take it
  HsLevels ul;
  ul.n_levels = (int)map->levels.size();
  ul.lo_free = map->lo_free;
  ul.lo_occ = map->lo_occ;
  for (int i = 0; i < ul.n_levels; i++) {
    const Level& L = map->levels[i];
    ul.sx[i] = L.sx; ul.sy[i] = L.sy;
    ul.free_key[i] = L.d_free; ul.occ_key[i] = L.d_occ; ul.logodds[i] = L.d_logodds;
  }
  return ul;
}

// what the host knows of one scan, but for its origo and its epochs
HsScan hs_scan_of(const lslam_hector* h, const float* hint, bool no_match, int capacity) {
  HsScan sc{};
  sc.chain = hint ? 0 : 1;
  sc.no_match = no_match ? 1 : 0;
  if (hint) {
    for (int q = 0; q < 3; q++) sc.hint[q] = hint[q];
    sc.hint_c = cosf(sc.hint[2]);  // host libm, exactly what the reference's Eigen::Rotation2Df evaluates
    sc.hint_s = sinf(sc.hint[2]);
    sc.host_trig = sc.no_match;
  }
  sc.min_dist = h->min_dist; sc.min_angle = h->min_angle; sc.fabs_gate = h->fabs_gate;
  sc.capacity = capacity;
  return sc;
}

int hs_run(lslam_hector* h, const HsCall& c) {
  lslam_map* map = h->map;
  lslam_context* ctx = map->ctx;
  const int n_levels = (int)map->levels.size();
  {
    int rc = flush_pending(map);  // the matcher reads the float planes; the streamed update is not deferred
    if (rc) return rc;
  }
  int cache_cap = 1;
  {
    int rc = hs_reserve_cached(map, c.capacity, &cache_cap);
    if (rc) return rc;
  }
  LSLAM_HIP(ctx, h->d_rec.reserve((size_t)c.n_scans));
  {
    int rc = hs_pinned_reserve(ctx, &h->h_rec, &h->h_rec_cap, (size_t)c.n_scans);
    if (rc) return rc;
  }
  hs_state_up(h);
  memcpy(h->h_io, &h->mirror, kHsPersistWords * 4);
  LSLAM_HIP(ctx, hipMemcpyAsync(h->d_state, h->h_io, kHsPersistWords * 4, hipMemcpyHostToDevice, ctx->stream));
  const GnLevels lv = gn_levels_of(map);
  const HsLevels ul = hs_levels_of(map);
  int* const d_n_live = &h->d_state->n_live;
  ProjectCfg pc{};
  float scan_origo[2] = {0.f, 0.f};
  std::vector<size_t> first;
  if (c.scan) {
    pc = project_cfg(map, c.n_readings, c.scan);
    hs_scan_origo(c.scan, pc, scan_origo);
  } else {
    first.assign((size_t)c.n_scans + 1, 0);
    for (int k = 0; k < c.n_scans; k++) first[k + 1] = first[k] + (size_t)c.n_points[k];
  }
  // the matcher's form from the CAPACITY (the live count is the device's): as match_data_impl chooses from n
  const GnForm form = gn_form_of(map, c.capacity);
  const dim3 ugrid((unsigned)((cache_cap + 3) / 4), (unsigned)n_levels), ublock(256);
  for (int k = 0; k < c.n_scans; k++) {
    HsScan sc = hs_scan_of(h, c.hints ? c.hints + 3 * k : nullptr, c.no_match && c.no_match[k], c.capacity);
    // an epoch per scan and level whether or not the device updates (an unused epoch is harmless)
    for (int li = 0; li < n_levels; li++) {
      Level& L = map->levels[li];
      if (L.epoch >= kMaxEpoch) {
        int rc = clear_marks(map, L);  // stream-ordered; nothing is pending
        if (rc) return rc;
      }
      sc.epoch[li] = ++L.epoch;
    }
    const float* pts;
    const int* n_src;
    const int32_t* take = c.cloud.take ? c.cloud.take + (size_t)k * (size_t)c.cloud.take_stride : nullptr;
    if (c.scan) {
      const float* xyz = c.cloud.xyz ? c.cloud.xyz + (size_t)3 * k * c.n_readings : nullptr;
      const uint8_t* valid = c.cloud.valid ? c.cloud.valid + (size_t)k * c.n_readings : nullptr;
      if (c.gated)
        launch(ctx, "hg_cloud_container", k_hg_cloud_container, dim3(1), dim3(1024), 0, pc, take, xyz, valid, map->d_scan.p, d_n_live);
      else if (c.cloud.xyz)
        launch(ctx, "hs_cloud_container", k_hector_cloud_container, dim3(1), dim3(1024), 0, pc, xyz, valid, map->d_scan.p, d_n_live);
      else
        launch(ctx, "hs_project", k_hector_project, dim3(1), dim3(1024), 0, pc, (const float*)(h->in.d_in.p + (size_t)k * c.n_readings),
               (const double2*)map->d_cossin.p, map->d_scan.p, d_n_live);
      pts = map->d_scan.p;
      n_src = d_n_live;
      sc.origo[0] = scan_origo[0]; sc.origo[1] = scan_origo[1];
    } else {
      pts = c.d_points + 2 * first[k];
      n_src = h->in.d_counts.p + k;
      sc.origo[0] = c.origos ? c.origos[2 * k] : 0.f;
      sc.origo[1] = c.origos ? c.origos[2 * k + 1] : 0.f;
    }
    lslam_hector_record* rec = h->d_rec.p + k;
#define LSLAM_HS_REG(NT, PMAX) \
  launch(ctx, "hs_match", k_hs_match_reg<NT, PMAX>, dim3(1), dim3(NT), form.lds, lv, sc, pts, n_src, map->d_cached.p, h->d_state, rec)
#define LSLAM_HS_FAST(NT)                                                                                                    \
  launch(ctx, "hs_match", k_hs_match_fast<NT>, dim3(1), dim3(NT), form.lds, lv, sc, pts, n_src, map->d_cached.p, form.in_lds, \
         h->d_state, rec)
#define LSLAM_HG_REG(NT, PMAX)                                                                                                 \
  launch(ctx, "hg_match", k_hg_match_reg<NT, PMAX>, dim3(1), dim3(NT), form.lds, lv, sc, take, pts, n_src, map->d_cached.p, \
         h->d_state, rec)
#define LSLAM_HG_FAST(NT)                                                                                                      \
  launch(ctx, "hg_match", k_hg_match_fast<NT>, dim3(1), dim3(NT), form.lds, lv, sc, take, pts, n_src, map->d_cached.p, form.in_lds, \
         h->d_state, rec)
    if (c.gated) {
      LSLAM_GN_DISPATCH(form, LSLAM_HG_REG, LSLAM_HG_FAST);
    } else {
      LSLAM_GN_DISPATCH(form, LSLAM_HS_REG, LSLAM_HS_FAST);
    }
#undef LSLAM_HS_REG
#undef LSLAM_HS_FAST
#undef LSLAM_HG_REG
#undef LSLAM_HG_FAST
    launch(ctx, "hs_mark", k_hs_mark, ugrid, ublock, 0, ul, (const HsState*)h->d_state, pts, (const float*)map->d_cached.p);
    launch(ctx, "hs_apply", k_hs_apply, ugrid, ublock, 0, ul, (const HsState*)h->d_state, pts, (const float*)map->d_cached.p);
  }
  LSLAM_HIP(ctx, hipGetLastError());
  // ---- end of the call: the records and the state down, ONE wait
  LSLAM_HIP(ctx, hipMemcpyAsync(h->h_rec, h->d_rec.p, (size_t)c.n_scans * sizeof(lslam_hector_record), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(h->h_io + kHsPersistWords, h->d_state, kHsPersistWords * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (c.sync_out)
    LSLAM_HIP(ctx, hipMemcpyAsync(h->h_msrec, h->d_msrec.p, (size_t)c.n_scans * sizeof(lslam_msync_record), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  h->n_syncs++;
  h->n_calls++;
  int n_taken = 0;
  for (int k = 0; k < c.n_scans; k++) n_taken += hs_count_record(h, h->h_rec[k]);
  if (c.out) memcpy(c.out, h->h_rec, (size_t)c.n_scans * sizeof(lslam_hector_record));
  if (c.sync_out) memcpy(c.sync_out, h->h_msrec, (size_t)c.n_scans * sizeof(lslam_msync_record));
  if (c.sync) msync_stream_drained(c.sync);
  hs_state_down(h, h->h_io + kHsPersistWords, n_taken, false, c.scan ? scan_origo : nullptr);
  return LSLAM_OK;
}

}  // namespace

extern "C" {

int lslam_hector_create(lslam_map* map, lslam_hector** out) {
  if (!map || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  lslam_context* ctx = map->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_hector* h = new lslam_hector();
  h->map = map;
  memset(&h->mirror, 0, sizeof h->mirror);
  hs_reset_state(h);
  if (hipMalloc((void**)&h->d_state, sizeof(HsState)) != hipSuccess ||
      hipHostMalloc((void**)&h->h_io, 2 * kHsPersistWords * 4, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    lslam_hector_destroy(h);
    return ctx->fail(LSLAM_ERR_HIP, "cannot allocate the streamed processor's state block");
  }
  (void)hipMemsetAsync(h->d_state, 0, sizeof(HsState), ctx->stream);
  *out = h;
  return LSLAM_OK;
}

void lslam_hector_destroy(lslam_hector* h) {
  if (!h) return;
  (void)hipSetDevice(h->map->ctx->device);
  (void)hipStreamSynchronize(h->map->ctx->stream);
  if (h->d_state) (void)hipFree(h->d_state);
  if (h->h_io) (void)hipHostFree(h->h_io);
  if (h->h_rec) (void)hipHostFree(h->h_rec);
  if (h->h_msrec) (void)hipHostFree(h->h_msrec);
  h->d_msrec.release();
  h->d_rec.release();
  if (h->deskew) lslam_deskew_destroy(h->deskew);
  h->in.release();
  delete h;
}

int lslam_hector_reset(lslam_hector* h) {
  if (!h) return LSLAM_ERR_INVALID_ARGUMENT;
  hs_reset_state(h);
  return lslam_map_reset(h->map);  // mapRep->reset() (HectorSlamProcessor.h:116)
}

int lslam_hector_set_update_thresholds(lslam_hector* h, float min_dist, float min_angle) {
  if (!h) return LSLAM_ERR_INVALID_ARGUMENT;
  h->min_dist = min_dist;
  h->min_angle = min_angle;
  return LSLAM_OK;
}

int lslam_hector_set_option(lslam_hector* h, int option, int value) {
  if (!h) return LSLAM_ERR_INVALID_ARGUMENT;
  if (option == LSLAM_HECTOR_OPT_FABS_ANGLE_GATE) {
    h->fabs_gate = value != 0;
    return LSLAM_OK;
  }
  return h->map->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "unknown streamed-processor option %d", option);
}

int lslam_hector_process_many(lslam_hector* h, const lslam_hector_scan* scan, int n_scans, int n_readings, const float* ranges,
                              int ranges_stride, const float* pose_hints, const uint8_t* map_without_matching,
                              lslam_hector_record* out) {
  if (!h || n_scans < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_scans == 0) return LSLAM_OK;
  if (!hs_ranges_given(scan, n_readings, ranges, ranges_stride)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_map* map = h->map;
  lslam_context* ctx = map->ctx;
  int rc = hs_check(h, "lslam_hector_process_many", n_readings);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hs_reserve_scan(map, n_readings));
  bool rebuilt = false;
  rc = ensure_cossin(map, n_readings, scan, &rebuilt);  // (waits for its upload when the scan geometry is new)
  if (rc) return rc;
  h->n_syncs += rebuilt;
  rc = hs_stage_ranges(ctx, h->in, (size_t)n_scans, n_readings, ranges, (size_t)ranges_stride);
  if (rc) return rc;
  return hs_run(h, hs_scan_call(scan, n_scans, n_readings, pose_hints, map_without_matching, out));
}

int lslam_hector_process_many_deskewed(lslam_hector* h, const lslam_hector_scan* scan, int n_scans, int n_readings,
                                       const float* ranges, int ranges_stride, const lslam_deskew_params* params,
                                       const int32_t* imu_first, const double* imu_time, const double* imu_rot_x,
                                       const double* imu_rot_y, const double* imu_rot_z, const float* pose_hints,
                                       const uint8_t* map_without_matching, lslam_hector_record* out) {
  if (!h || n_scans < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_scans == 0) return LSLAM_OK;
  if (!params || !imu_first || !hs_ranges_given(scan, n_readings, ranges, ranges_stride)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_map* map = h->map;
  lslam_context* ctx = map->ctx;
  int rc = hs_check(h, "lslam_hector_process_many_deskewed", n_readings);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_ensure_deskew(ctx, &h->deskew);
  if (rc) return rc;
  LSLAM_HIP(ctx, hs_reserve_scan(map, n_readings));
  const size_t total = (size_t)n_scans * (size_t)n_readings;
  LSLAM_HIP(ctx, h->in.d_xyz.reserve(std::max(3 * total, (size_t)1)));
  LSLAM_HIP(ctx, h->in.d_valid.reserve(std::max(total, (size_t)1)));
  rc = hs_stage_ranges(ctx, h->in, (size_t)n_scans, n_readings, ranges, (size_t)ranges_stride);
  if (rc) return rc;
  // ONE de-skew launch for the whole call (it does not depend on the map), asynchronous on the same stream
  rc = lslam_deskew_batch_dev(h->deskew, n_scans, n_readings, h->in.d_in.p, n_readings, params, imu_first, imu_time, imu_rot_x,
                              imu_rot_y, imu_rot_z, h->in.d_xyz.p, h->in.d_valid.p);
  if (rc) return rc;
  HsCall c = hs_scan_call(scan, n_scans, n_readings, pose_hints, map_without_matching, out);
  c.cloud.xyz = h->in.d_xyz.p;
  c.cloud.valid = h->in.d_valid.p;
  return hs_run(h, c);
}

int lslam_hector_process_many_clouds_dev(lslam_hector* h, const lslam_hector_scan* scan, int n_scans, int n_points,
                                         const float* xyz_dev, const uint8_t* valid_dev, const int32_t* take_dev,
                                         int take_stride, const float* pose_hints, const uint8_t* map_without_matching,
                                         lslam_hector_record* out) {
  if (!h || n_scans < 0 || n_points < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_scans == 0) return LSLAM_OK;
  if (!scan || (n_points > 0 && !xyz_dev) || (take_dev && take_stride < 1)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_map* map = h->map;
  lslam_context* ctx = map->ctx;
  int rc = hs_check(h, "lslam_hector_process_many_clouds", n_points);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hs_reserve_scan(map, n_points));
  HsCall c = hs_scan_call(scan, n_scans, n_points, pose_hints, map_without_matching, out);
  c.cloud = {xyz_dev, valid_dev, take_dev, take_stride};
  c.gated = true;
  return hs_run(h, c);
}

int lslam_hector_process_many_clouds(lslam_hector* h, const lslam_hector_scan* scan, int n_scans, int n_points,
                                     const float* xyz, const uint8_t* valid, const uint8_t* take, const float* pose_hints,
                                     const uint8_t* map_without_matching, lslam_hector_record* out) {
  if (!h || n_scans < 0 || n_points < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_scans == 0) return LSLAM_OK;
  if (!scan || (n_points > 0 && !xyz)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = h->map->ctx;
  int rc = hs_check(h, "lslam_hector_process_many_clouds", n_points);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_stage_clouds(ctx, h->in, (size_t)n_scans, n_points, xyz, valid, take);
  if (rc) return rc;
  return lslam_hector_process_many_clouds_dev(h, scan, n_scans, n_points, h->in.d_xyz.p, valid ? h->in.d_valid.p : (const uint8_t*)nullptr,
                                              take ? h->in.d_take.p : (const int32_t*)nullptr, 1, pose_hints, map_without_matching, out);
}

int lslam_hector_process_many_synced(lslam_hector* h, lslam_msync* sync, const lslam_hector_scan* scan,
                                     const lslam_msync_laser* laser, int n_msgs, int n_readings, const float* ranges,
                                     int ranges_stride, const double* stamps, const float* time_increments,
                                     const int64_t* imu_seen, const int64_t* odom_seen, const float* pose_hints,
                                     const uint8_t* map_without_matching, lslam_hector_record* out,
                                     lslam_msync_record* sync_records) {
  if (!h || !sync || n_msgs < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_msgs == 0) return LSLAM_OK;
  if (!scan || !ranges) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_map* map = h->map;
  lslam_context* ctx = map->ctx;
  // ---- everything that can refuse the call, before anything is enqueued or either handle changes
  if (msync_context(sync) != ctx)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_hector_process_many_synced: the lslam_msync handle belongs to another context than the map");
  int rc = hs_check(h, "lslam_hector_process_many_synced", n_readings);
  if (rc) return rc;
  rc = hs_check_stride(ctx, "lslam_hector_process_many_synced", ranges_stride, n_readings);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_ensure_deskew(ctx, &h->deskew);
  if (rc) return rc;
  rc = msync_check_scans(sync, h->deskew, laser, n_msgs, n_readings, stamps, time_increments, imu_seen, odom_seen);
  if (rc) return rc;
  // ---- buffers: ranges up through pinned staging; clouds and the walk's records stay in HBM
  const size_t total = (size_t)n_msgs * (size_t)n_readings;
  LSLAM_HIP(ctx, hs_reserve_scan(map, n_readings));
  LSLAM_HIP(ctx, h->in.d_xyz.reserve(3 * total));
  LSLAM_HIP(ctx, h->in.d_valid.reserve(total));
  LSLAM_HIP(ctx, h->d_msrec.reserve((size_t)n_msgs));
  if (sync_records) {
    rc = hs_pinned_reserve(ctx, &h->h_msrec, &h->h_msrec_cap, (size_t)n_msgs);
    if (rc) return rc;
  }
  rc = hs_stage_ranges(ctx, h->in, (size_t)n_msgs, n_readings, ranges, (size_t)ranges_stride);
  if (rc) return rc;
  // the node's callbacks for the whole call: walk, windows, ONE de-skew launch, blank -- asynchronous, no wait
  rc = lslam_msync_scans_dev(sync, h->deskew, laser, n_msgs, n_readings, h->in.d_in.p, n_readings, stamps, time_increments, imu_seen,
                             odom_seen, h->in.d_xyz.p, h->in.d_valid.p, h->d_msrec.p);
  if (rc) return rc;
  static_assert(offsetof(lslam_msync_record, status) == 0 && sizeof(lslam_msync_record) % sizeof(int32_t) == 0,
                "lslam_msync_record::status is the take word of its callback");
  HsCall c = hs_scan_call(scan, n_msgs, n_readings, pose_hints, map_without_matching, out);
  c.cloud = {h->in.d_xyz.p, h->in.d_valid.p, &h->d_msrec.p->status, (int)(sizeof(lslam_msync_record) / sizeof(int32_t))};
  c.gated = true;
  c.sync = sync;
  c.sync_out = sync_records;
  return hs_run(h, c);
}

int lslam_hector_process_many_points(lslam_hector* h, int n_scans, const float* points_xy, const int32_t* n_points,
                                     const float* origos_xy, const float* pose_hints, const uint8_t* map_without_matching,
                                     lslam_hector_record* out) {
  if (!h || n_scans < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_scans == 0) return LSLAM_OK;
  if (!n_points) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_map* map = h->map;
  lslam_context* ctx = map->ctx;
  const char* who = "lslam_hector_process_many_points";
  size_t total = 0;
  int cap = 0;
  int rc = hs_check_counts(ctx, who, (size_t)n_scans, n_points, nullptr, points_xy, &total, &cap);
  if (!rc) rc = hs_check(h, who, cap);
  if (rc) return rc;
  if (total > (size_t)INT32_MAX / 2) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: call too large", who);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_stage_points(ctx, h->in, map->d_pts, (size_t)n_scans, points_xy, n_points, total);
  if (rc) return rc;
  HsCall c;
  c.n_scans = n_scans;
  c.capacity = cap;
  c.d_points = map->d_pts.p;
  c.n_points = n_points;
  c.origos = origos_xy;
  c.hints = pose_hints;
  c.no_match = map_without_matching;
  c.out = out;
  return hs_run(h, c);
}

int lslam_hector_state(lslam_hector* h, float last_match_pose[3], float last_match_cov[9], float last_update_pose[3]) {
  if (!h) return LSLAM_ERR_INVALID_ARGUMENT;
  if (last_match_pose) memcpy(last_match_pose, h->mirror.match_pose, 3 * sizeof(float));
  if (last_match_cov) memcpy(last_match_cov, h->mirror.cov, 9 * sizeof(float));
  if (last_update_pose) memcpy(last_update_pose, h->mirror.update_pose, 3 * sizeof(float));
  return LSLAM_OK;
}

int lslam_hector_stats(const lslam_hector* h, int64_t out[4]) {
  if (!h || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = h->n_scans; out[1] = h->n_updates; out[2] = h->n_calls; out[3] = h->n_syncs;
  return LSLAM_OK;
}

}  // extern "C"


// ------------------------------------------------------------------------------------------
// lslam_hector_fleet_*: many streamed processors stepped in lockstep launches (device side: k_hf_* above)
// ------------------------------------------------------------------------------------------
struct lslam_hector_fleet {
  lslam_context* ctx = nullptr;
  std::vector<lslam_hector*> members;
  // The device tables, and the members' state blocks of a call side by side: one copy up and one down per call instead of
  // one per member.  What a member IS stays in its own mirror and map: the blocks are filled from them at the start of a
  // call and handed back at its end, as the member's own calls do with its own block.
  HfMember* d_mem = nullptr;
  HsState* d_state = nullptr;
  DevBuf<HfScan> d_step;
  DevBuf<lslam_hector_record> d_rec;
  // pinned staging, the fleet's own
  HfMember* h_mem = nullptr;
  HsState* h_state = nullptr;  // [2][R]: up, down
  HfScan* h_step = nullptr;
  size_t h_step_cap = 0;
  lslam_hector_record* h_rec = nullptr;
  size_t h_rec_cap = 0;
  HsStage in;
  // synced form: the fleet's own de-skew handle and fleet-wide synchronisation, made by the first synced call
  lslam_deskew* deskew = nullptr;
  MsyncFleet* msf = nullptr;
  int64_t n_steps = 0, n_scans = 0, n_updates = 0, n_calls = 0, n_syncs = 0, n_launches = 0;
};

namespace {

constexpr int kHfMaxMembers = 4096;

struct HfCall {
  int n_steps = 0, capacity = 0;
  const lslam_hector_scan* scan = nullptr;  // ranges form
  int n_readings = 0;
  const int32_t* n_points = nullptr;        // container form: host counts (offsets into d_in) and
  const float* origos = nullptr;            //   origos (may be null)
  const float* hints = nullptr;
  const uint8_t* no_match = nullptr;
  const uint8_t* active = nullptr;
  lslam_hector_record* out = nullptr;
  // gated cloud form (with `scan`): per entry i = step * R + member, the device addresses of its cloud, its valid flags (null:
  // all valid) and its take word (null: taken); entries with active == 0 are not read.  take / valid empty: all null
  bool gated = false;
  std::vector<const float*> xyz;
  std::vector<const uint8_t*> valid;
  std::vector<const int32_t*> take;
  // synced form: the fleet-wide synchronisation whose walk wrote the take words; its records and states come down with the
  // processors' and are handed out behind the one wait
  MsyncFleet* msf = nullptr;
  lslam_msync_record* sync_out = nullptr;
};

struct HfWrap { int step, member, level; };  // a key plane whose epochs run out in front of this step

// the call of every form that fills the members' resident containers from n_steps scans each of n_readings readings (or points)
HfCall hf_scan_call(const lslam_hector_scan* scan, int n_steps, int n_readings, const float* hints, const uint8_t* no_match,
                    const uint8_t* active, lslam_hector_record* out) {
  HfCall c;
  c.n_steps = n_steps;
  c.capacity = n_readings;
  c.scan = scan;
  c.n_readings = n_readings;
  c.hints = hints;
  c.no_match = no_match;
  c.active = active;
  c.out = out;
  return c;
}

// what a call refuses before anything is enqueued
int hf_check(lslam_hector_fleet* f, const char* who, int capacity) {
  for (lslam_hector* h : f->members) {
    int rc = hs_check(h, who, capacity);
    if (rc) return rc;
  }
  return LSLAM_OK;
}

// the scans the host offers each member in a call of n_steps (active null: one per step)
std::vector<int> hf_active_counts(const lslam_hector_fleet* f, int n_steps, const uint8_t* active) {
  const size_t R = f->members.size(), total = (size_t)n_steps * R;
  std::vector<int> n_active(R, 0);
  for (size_t i = 0; i < total; i++) n_active[i % R] += !active || active[i];
  return n_active;
}

// Everything of a call that can fail before its first launch: the members' pending updates flushed, and every buffer the call
// needs.  Doing it twice is doing it once, so the synced form runs it in front of the synchronisation's enqueue -- the nodes
// must not walk callbacks that the processors then cannot take -- and hf_run runs it again.  *ucap: the points either
// container of a scan of this call may hold, over all members.
int hf_reserve(lslam_hector_fleet* f, const HfCall& c, int* ucap, int* max_levels) {
  lslam_context* ctx = f->ctx;
  const int R = (int)f->members.size();
  const size_t total = (size_t)c.n_steps * (size_t)R;
  const std::vector<int> n_active = hf_active_counts(f, c.n_steps, c.active);
  *ucap = 1;
  *max_levels = 1;
  for (int m = 0; m < R; m++) {
    lslam_map* map = f->members[m]->map;
    // Growing a resident container drops what it holds: only for a member whose scans may replace it.  In the gated forms
    // the device may refuse every one of them, and then the member must be what it was: the points move along.
    if (c.scan && n_active[m]) {
      const float* old = map->d_scan.p;
      LSLAM_HIP(ctx, hs_reserve_scan(map, c.n_readings));
      if (c.gated && old && old != map->d_scan.p && map->n_scan > 0)
        LSLAM_HIP(ctx, hipMemcpyAsync(map->d_scan.p, old, (size_t)2 * map->n_scan * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    }
    int rc = flush_pending(map);  // the matcher reads the float planes; the streamed update is not deferred
    if (rc) return rc;
    int cache_cap = 1;
    rc = hs_reserve_cached(map, c.capacity, &cache_cap);
    if (rc) return rc;
    *ucap = std::max(*ucap, cache_cap);
    *max_levels = std::max(*max_levels, (int)map->levels.size());
  }
  LSLAM_HIP(ctx, f->d_step.reserve(total));
  LSLAM_HIP(ctx, f->d_rec.reserve(total));
  int rc = hs_pinned_reserve(ctx, &f->h_step, &f->h_step_cap, total);
  if (!rc) rc = hs_pinned_reserve(ctx, &f->h_rec, &f->h_rec_cap, total);
  return rc;
}

int hf_run(lslam_hector_fleet* f, const HfCall& c) {
  lslam_context* ctx = f->ctx;
  const int R = (int)f->members.size();
  const size_t total = (size_t)c.n_steps * (size_t)R;
  const bool ranges_form = c.scan != nullptr;
  int ucap = 1, max_levels = 1;
  {
    int rc = hf_reserve(f, c, &ucap, &max_levels);
    if (rc) return rc;
  }
  // ---- the member table and the state blocks up
  std::vector<float> scan_origo((size_t)2 * R, 0.f);  // ranges form: the origo of member m's projected scans
  for (int m = 0; m < R; m++) {
    lslam_hector* h = f->members[m];
    lslam_map* map = h->map;
    hs_state_up(h);
    memcpy(&f->h_state[m], &h->mirror, sizeof(HsState));
    HfMember& hm = f->h_mem[m];
    hm.gn = gn_levels_of(map);
    hm.ul = hs_levels_of(map);
    hm.pc = ranges_form ? project_cfg(map, c.n_readings, c.scan) : ProjectCfg{};
    if (ranges_form) hs_scan_origo(c.scan, hm.pc, &scan_origo[(size_t)2 * m]);
    hm.st = f->d_state + m;
    hm.cached = map->d_cached.p;
    hm.resident = map->d_scan.p;
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_mem, f->h_mem, (size_t)R * sizeof(HfMember), hipMemcpyHostToDevice, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_state, f->h_state, (size_t)R * sizeof(HsState), hipMemcpyHostToDevice, ctx->stream));
  // ---- the descriptors of the whole call.  An epoch per ACTIVE scan and level whether or not the device updates (an unused
  // epoch is harmless); a plane whose epochs run out is cleared in front of the step that starts them again.
  std::vector<size_t> first;
  if (!ranges_form) {
    first.assign(total + 1, 0);
    for (size_t i = 0; i < total; i++) first[i + 1] = first[i] + (size_t)c.n_points[i];
  }
  std::vector<uint32_t> epoch((size_t)R * kGnMaxLevels, 0);
  for (int m = 0; m < R; m++)
    for (size_t li = 0; li < f->members[m]->map->levels.size(); li++) epoch[(size_t)m * kGnMaxLevels + li] = f->members[m]->map->levels[li].epoch;
  std::vector<HfWrap> wraps;
  for (int k = 0; k < c.n_steps; k++) {
    for (int m = 0; m < R; m++) {
      const size_t i = (size_t)k * R + m;
      lslam_hector* h = f->members[m];
      lslam_map* map = h->map;
      HfScan& d = f->h_step[i];
      d = HfScan{};
      d.active = !c.active || c.active[i] ? 1 : 0;
      if (!d.active) continue;
      d.sc = hs_scan_of(h, c.hints ? c.hints + 3 * i : nullptr, c.no_match && c.no_match[i], c.capacity);
      for (int li = 0; li < (int)map->levels.size(); li++) {
        uint32_t& e = epoch[(size_t)m * kGnMaxLevels + li];
        if (e >= kMaxEpoch) {
          wraps.push_back({k, m, li});
          e = 0;
        }
        d.sc.epoch[li] = ++e;
      }
      if (ranges_form) {
        d.sc.origo[0] = scan_origo[(size_t)2 * m];
        d.sc.origo[1] = scan_origo[(size_t)2 * m + 1];
        d.pts = map->d_scan.p;
        d.n_src = &(f->d_state + m)->n_live;
        if (c.gated) {
          d.xyz = c.xyz[i];
          d.valid = c.valid.empty() ? nullptr : c.valid[i];
          d.take = c.take.empty() ? nullptr : c.take[i];
        } else {
          d.ranges = f->in.d_in.p + i * (size_t)c.n_readings;
        }
      } else {
        d.sc.origo[0] = c.origos ? c.origos[2 * i] : 0.f;
        d.sc.origo[1] = c.origos ? c.origos[2 * i + 1] : 0.f;
        d.pts = f->in.d_in.p + 2 * first[i];
        d.n_src = f->in.d_counts.p + i;
      }
      d.rec = f->d_rec.p + i;
    }
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_step.p, f->h_step, total * sizeof(HfScan), hipMemcpyHostToDevice, ctx->stream));
  // the matcher's form from the call's CAPACITY and the members' common LSLAM_GN_THREADS, as the single processor chooses it
  const GnForm form = gn_form_of(f->members[0]->map, c.capacity);
  const double2* cossin = c.gated ? nullptr : f->members[0]->map->d_cossin.p;  // (the table follows from the scan geometry alone)
  const dim3 ugrid((unsigned)((ucap + 3) / 4), (unsigned)max_levels, (unsigned)R), ublock(256);
  size_t w = 0;
  for (int k = 0; k < c.n_steps; k++) {
    for (; w < wraps.size() && wraps[w].step == k; w++) {
      lslam_map* map = f->members[wraps[w].member]->map;
      int rc = clear_marks(map, map->levels[wraps[w].level]);  // stream-ordered, behind step k-1's apply; nothing is pending
      if (rc) return rc;
    }
    const HfMember* mem = f->d_mem;
    const HfScan* step = f->d_step.p + (size_t)k * R;
    if (c.gated) {
      launch(ctx, "hfg_cloud_container", k_hfg_cloud_container, dim3(R), dim3(1024), 0, mem, step);
      f->n_launches++;
    } else if (ranges_form) {
      launch(ctx, "hf_project", k_hf_project, dim3(R), dim3(1024), 0, mem, step, cossin);
      f->n_launches++;
    }
#define LSLAM_HF_REG(NT, PMAX) launch(ctx, "hf_match", k_hf_match_reg<NT, PMAX>, dim3(R), dim3(NT), form.lds, mem, step)
#define LSLAM_HF_FAST(NT) launch(ctx, "hf_match", k_hf_match_fast<NT>, dim3(R), dim3(NT), form.lds, mem, step, form.in_lds)
#define LSLAM_HFG_REG(NT, PMAX) launch(ctx, "hfg_match", k_hfg_match_reg<NT, PMAX>, dim3(R), dim3(NT), form.lds, mem, step)
#define LSLAM_HFG_FAST(NT) launch(ctx, "hfg_match", k_hfg_match_fast<NT>, dim3(R), dim3(NT), form.lds, mem, step, form.in_lds)
    if (c.gated) {
      LSLAM_GN_DISPATCH(form, LSLAM_HFG_REG, LSLAM_HFG_FAST);
    } else {
      LSLAM_GN_DISPATCH(form, LSLAM_HF_REG, LSLAM_HF_FAST);
    }
#undef LSLAM_HF_REG
#undef LSLAM_HF_FAST
#undef LSLAM_HFG_REG
#undef LSLAM_HFG_FAST
    launch(ctx, "hf_mark", k_hf_mark, ugrid, ublock, 0, mem, step);
    launch(ctx, "hf_apply", k_hf_apply, ugrid, ublock, 0, mem, step);
    f->n_launches += 3;
  }
  for (int m = 0; m < R; m++)
    for (size_t li = 0; li < f->members[m]->map->levels.size(); li++) f->members[m]->map->levels[li].epoch = epoch[(size_t)m * kGnMaxLevels + li];
  LSLAM_HIP(ctx, hipGetLastError());
  // ---- end of the call: the records and the state blocks down, ONE wait
  LSLAM_HIP(ctx, hipMemcpyAsync(f->h_rec, f->d_rec.p, total * sizeof(lslam_hector_record), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(f->h_state + R, f->d_state, (size_t)R * sizeof(HsState), hipMemcpyDeviceToHost, ctx->stream));
  if (c.msf) {
    int rc = msync_fleet_download(c.msf);
    if (rc) return rc;
  }
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_syncs++;
  f->n_calls++;
  f->n_steps += c.n_steps;
  if (c.msf) msync_fleet_finish(c.msf, c.sync_out);
  // the accounting comes from the RECORDS: in the gated forms the device decides whether an active scan is taken
  std::vector<int> n_taken((size_t)R, 0);
  for (size_t i = 0; i < total; i++) {
    lslam_hector_record& r = f->h_rec[i];
    if (!f->h_step[i].active) {  // a scan that was not taken: all zero but the count
      memset(&r, 0, sizeof r);
      r.n_points = -1;
      continue;
    }
    if (!hs_count_record(f->members[i % (size_t)R], r)) continue;  // refused on the device: hg_skip wrote its record
    n_taken[i % (size_t)R]++;
    f->n_scans++;
    f->n_updates += r.updated != 0;
  }
  if (c.out) memcpy(c.out, f->h_rec, total * sizeof(lslam_hector_record));
  for (int m = 0; m < R; m++)
    hs_state_down(f->members[m], &f->h_state[R + m], n_taken[m], true, ranges_form ? &scan_origo[(size_t)2 * m] : nullptr);
  return LSLAM_OK;
}

}  // namespace

extern "C" {

int lslam_hector_fleet_create(lslam_hector* const* members, int n_members, lslam_hector_fleet** out) {
  if (!members || !out || n_members < 1) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  for (int m = 0; m < n_members; m++)
    if (!members[m]) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = members[0]->map->ctx;
  for (int m = 0; m < n_members; m++) {
    if (members[m]->map->ctx != ctx)
      return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_hector_fleet_create: member %d belongs to another context", m);
    for (int q = 0; q < m; q++) {
      if (members[q] == members[m])
        return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_hector_fleet_create: members %d and %d are the same processor", q, m);
      if (members[q]->map == members[m]->map)
        return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_hector_fleet_create: members %d and %d share one map", q, m);
    }
  }
  if (n_members > kHfMaxMembers)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_create: at most %d members (got %d)", kHfMaxMembers, n_members);
  for (int m = 0; m < n_members; m++) {
    const lslam_map* map = members[m]->map;
    if (gn_form_of(map, 0).nt != gn_form_of(members[0]->map, 0).nt)
      return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_create: member %d's map was created under another LSLAM_GN_THREADS "
                       "than member 0's; one launch runs one form of the matcher", m);
    if (map->ordered_sums)
      return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_create: member %d's map is an LSLAM_MAP_OPT_ORDERED_SUMS map; the "
                       "streamed processor runs the parallel-sum matcher", m);
    if ((int)map->levels.size() > kGnMaxLevels)
      return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_create: at most %d pyramid levels (member %d)", kGnMaxLevels, m);
  }
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_hector_fleet* f = new lslam_hector_fleet();
  f->ctx = ctx;
  f->members.assign(members, members + n_members);
  const size_t R = (size_t)n_members;
  if (hipMalloc((void**)&f->d_mem, R * sizeof(HfMember)) != hipSuccess ||
      hipMalloc((void**)&f->d_state, R * sizeof(HsState)) != hipSuccess ||
      hipHostMalloc((void**)&f->h_mem, R * sizeof(HfMember), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&f->h_state, 2 * R * sizeof(HsState), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    lslam_hector_fleet_destroy(f);
    return ctx->fail(LSLAM_ERR_HIP, "cannot allocate the fleet's tables");
  }
  memset(f->h_mem, 0, R * sizeof(HfMember));
  memset(f->h_state, 0, 2 * R * sizeof(HsState));
  *out = f;
  return LSLAM_OK;
}

void lslam_hector_fleet_destroy(lslam_hector_fleet* f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  if (f->d_mem) (void)hipFree(f->d_mem);
  if (f->d_state) (void)hipFree(f->d_state);
  if (f->h_mem) (void)hipHostFree(f->h_mem);
  if (f->h_state) (void)hipHostFree(f->h_state);
  if (f->h_step) (void)hipHostFree(f->h_step);
  if (f->h_rec) (void)hipHostFree(f->h_rec);
  f->d_step.release();
  f->d_rec.release();
  f->in.release();
  if (f->deskew) lslam_deskew_destroy(f->deskew);
  msync_fleet_destroy(f->msf);
  delete f;
}

int lslam_hector_fleet_size(const lslam_hector_fleet* f) { return f ? (int)f->members.size() : LSLAM_ERR_INVALID_ARGUMENT; }

int lslam_hector_fleet_process_many(lslam_hector_fleet* f, const lslam_hector_scan* scan, int n_steps, int n_readings,
                                    const float* ranges, int ranges_stride, const float* pose_hints,
                                    const uint8_t* map_without_matching, const uint8_t* active, lslam_hector_record* out) {
  if (!f || n_steps < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!hs_ranges_given(scan, n_readings, ranges, ranges_stride)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  int rc = hf_check(f, "lslam_hector_fleet_process_many", n_readings);
  if (rc) return rc;
  const size_t rows = (size_t)n_steps * f->members.size();
  if (rows * (size_t)n_readings > (size_t)INT32_MAX / 2)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_process_many: call too large");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  bool rebuilt = false;
  rc = ensure_cossin(f->members[0]->map, n_readings, scan, &rebuilt);  // (waits for its upload when the scan geometry is new)
  if (rc) return rc;
  f->n_syncs += rebuilt;
  rc = hs_stage_ranges(ctx, f->in, rows, n_readings, ranges, (size_t)ranges_stride);
  if (rc) return rc;
  return hf_run(f, hf_scan_call(scan, n_steps, n_readings, pose_hints, map_without_matching, active, out));
}

int lslam_hector_fleet_process_many_points(lslam_hector_fleet* f, int n_steps, const float* points_xy, const int32_t* n_points,
                                           const float* origos_xy, const float* pose_hints,
                                           const uint8_t* map_without_matching, const uint8_t* active, lslam_hector_record* out) {
  if (!f || n_steps < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!n_points) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  const char* who = "lslam_hector_fleet_process_many_points";
  const size_t rows = (size_t)n_steps * f->members.size();
  size_t total = 0;
  int cap = 0;
  int rc = hs_check_counts(ctx, who, rows, n_points, active, points_xy, &total, &cap);
  if (!rc) rc = hf_check(f, who, cap);
  if (rc) return rc;
  if (total > (size_t)INT32_MAX / 2) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: call too large", who);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_stage_points(ctx, f->in, f->in.d_in, rows, points_xy, n_points, total);
  if (rc) return rc;
  HfCall c;
  c.n_steps = n_steps;
  c.capacity = cap;
  c.n_points = n_points;
  c.origos = origos_xy;
  c.hints = pose_hints;
  c.no_match = map_without_matching;
  c.active = active;
  c.out = out;
  return hf_run(f, c);
}

int lslam_hector_fleet_process_many_clouds_dev(lslam_hector_fleet* f, const lslam_hector_scan* scan, int n_steps, int n_points,
                                               const float* const* xyz_dev, const uint8_t* const* valid_dev,
                                               const int32_t* const* take_dev, int take_stride, const float* pose_hints,
                                               const uint8_t* map_without_matching, const uint8_t* active,
                                               lslam_hector_record* out) {
  if (!f || n_steps < 0 || n_points < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!scan || (n_points > 0 && !xyz_dev) || (take_dev && take_stride < 1)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  const size_t R = f->members.size(), total = (size_t)n_steps * R;
  if (n_points > 0) {
    const std::vector<int> n_active = hf_active_counts(f, n_steps, active);
    for (size_t m = 0; m < R; m++)
      if (n_active[m] && !xyz_dev[m])
        return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_hector_fleet_process_many_clouds_dev: member %zu has scans but no cloud block", m);
  }
  int rc = hf_check(f, "lslam_hector_fleet_process_many_clouds", n_points);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  HfCall c = hf_scan_call(scan, n_steps, n_points, pose_hints, map_without_matching, active, out);
  c.gated = true;
  c.xyz.assign(total, nullptr);
  if (valid_dev) c.valid.assign(total, nullptr);
  if (take_dev) c.take.assign(total, nullptr);
  for (size_t i = 0; i < total; i++) {  // member m's row of step k: block m + k rows
    if (active && !active[i]) continue;
    const size_t k = i / R, m = i % R;
    c.xyz[i] = n_points > 0 ? xyz_dev[m] + k * (size_t)n_points * 3 : nullptr;
    if (valid_dev && valid_dev[m]) c.valid[i] = valid_dev[m] + k * (size_t)n_points;
    if (take_dev && take_dev[m]) c.take[i] = take_dev[m] + k * (size_t)take_stride;
  }
  return hf_run(f, c);
}

int lslam_hector_fleet_process_many_clouds(lslam_hector_fleet* f, const lslam_hector_scan* scan, int n_steps, int n_points,
                                           const float* xyz, const uint8_t* valid, const uint8_t* take, const float* pose_hints,
                                           const uint8_t* map_without_matching, const uint8_t* active, lslam_hector_record* out) {
  if (!f || n_steps < 0 || n_points < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!scan || (n_points > 0 && !xyz)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  int rc = hf_check(f, "lslam_hector_fleet_process_many_clouds", n_points);
  if (rc) return rc;
  const size_t R = f->members.size(), rows = (size_t)n_steps * R, total = rows * (size_t)n_points;
  if (total > (size_t)INT32_MAX / 4) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_process_many_clouds: call too large");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_stage_clouds(ctx, f->in, rows, n_points, xyz, valid, take);
  if (rc) return rc;
  HfCall c = hf_scan_call(scan, n_steps, n_points, pose_hints, map_without_matching, active, out);
  c.gated = true;
  c.xyz.assign(rows, nullptr);
  if (valid) c.valid.assign(rows, nullptr);
  if (take) c.take.assign(rows, nullptr);
  for (size_t i = 0; i < rows; i++) {
    c.xyz[i] = f->in.d_xyz.p + 3 * i * (size_t)n_points;
    if (valid) c.valid[i] = f->in.d_valid.p + i * (size_t)n_points;
    if (take) c.take[i] = f->in.d_take.p + i;
  }
  return hf_run(f, c);
}

int lslam_hector_fleet_process_many_synced(lslam_hector_fleet* f, lslam_msync* const* syncs, const lslam_hector_scan* scan,
                                           const lslam_msync_laser* laser, int n_steps, int n_readings, const float* ranges,
                                           int ranges_stride, const double* stamps, const float* time_increments,
                                           const int64_t* imu_seen, const int64_t* odom_seen, const float* pose_hints,
                                           const uint8_t* map_without_matching, const uint8_t* active, lslam_hector_record* out,
                                           lslam_msync_record* sync_records) {
  if (!f || !syncs || n_steps < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!scan || !laser || !ranges || !stamps || !time_increments) return LSLAM_ERR_INVALID_ARGUMENT;
  const int R = (int)f->members.size();
  for (int m = 0; m < R; m++)
    if (!syncs[m]) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  // ---- everything that can refuse the call, before anything is enqueued or any handle changes
  for (int m = 0; m < R; m++) {
    if (msync_context(syncs[m]) != ctx)
      return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_hector_fleet_process_many_synced: member %d's lslam_msync handle belongs to "
                       "another context than the fleet", m);
    for (int q = 0; q < m; q++)
      if (syncs[q] == syncs[m])
        return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_hector_fleet_process_many_synced: members %d and %d share one lslam_msync "
                         "handle; a node belongs to one robot", q, m);
  }
  int rc = hf_check(f, "lslam_hector_fleet_process_many_synced", n_readings);
  if (rc) return rc;
  rc = hs_check_stride(ctx, "lslam_hector_fleet_process_many_synced", ranges_stride, n_readings);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_ensure_deskew(ctx, &f->deskew);
  if (rc) return rc;
  if (!f->msf) f->msf = msync_fleet_create(ctx);
  rc = msync_fleet_plan(f->msf, syncs, R, f->deskew, laser, n_steps, n_readings, stamps, time_increments, imu_seen, odom_seen, active);
  if (rc) return rc;
  HfCall c = hf_scan_call(scan, n_steps, n_readings, pose_hints, map_without_matching, active, out);
  c.gated = true;
  {  // the processors' side of the call is ready before any node walks a callback
    int ucap = 1, max_levels = 1;
    rc = hf_reserve(f, c, &ucap, &max_levels);
    if (rc) return rc;
  }
  // ---- the nodes' callbacks of the whole call: rows, walk, windows, ONE de-skew launch, blank -- asynchronous, no wait
  const float* d_xyz = nullptr;
  const uint8_t* d_valid = nullptr;
  const lslam_msync_record* d_recs = nullptr;
  const int* row_of = nullptr;
  rc = msync_fleet_enqueue(f->msf, f->deskew, laser, ranges, ranges_stride, &d_xyz, &d_valid, &d_recs, &row_of);
  if (rc) return rc;
  static_assert(offsetof(lslam_msync_record, status) == 0, "lslam_msync_record::status is the take word of its callback");
  const size_t total = (size_t)n_steps * (size_t)R;
  c.xyz.assign(total, nullptr);
  c.valid.assign(total, nullptr);
  c.take.assign(total, nullptr);
  for (size_t i = 0; i < total; i++) {
    if (row_of[i] < 0) continue;
    const size_t row = (size_t)row_of[i];
    c.xyz[i] = d_xyz + 3 * row * (size_t)n_readings;
    c.valid[i] = d_valid + row * (size_t)n_readings;
    c.take[i] = &d_recs[row].status;
  }
  c.msf = f->msf;
  c.sync_out = sync_records;
  return hf_run(f, c);
}

int lslam_hector_fleet_sync_stats(const lslam_hector_fleet* f, int64_t out[4]) {
  if (!f || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (f->msf) msync_fleet_stats(f->msf, out);
  return LSLAM_OK;
}

int lslam_hector_fleet_stats(const lslam_hector_fleet* f, int64_t out[6]) {
  if (!f || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = f->n_steps; out[1] = f->n_scans; out[2] = f->n_updates; out[3] = f->n_calls; out[4] = f->n_syncs; out[5] = f->n_launches;
  return LSLAM_OK;
}

}  // extern "C"


#include "hector_loc_impl.hpp"  // lslam_hector_loc_*: R trackers on one borrowed map
