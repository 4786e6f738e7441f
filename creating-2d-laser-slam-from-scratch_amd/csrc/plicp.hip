// lesson3 PL-ICP scan-to-scan matching on the device: ScanMatchPLICP (lesson3/src/scan_match_plicp.cc, plicp_odometry.cc).
// PARITY UNPINNED: the reference's arithmetic lives in the un-vendored third-party `csm` (sm_icp).  What
// the results are DEFINED by is this project's own fp64 restatement of the published algorithm, `sm_icp` in
// tools/plicp_cpu.py; the wrapper logic of the two reference files is followed literally.
//
// One workgroup per pair, ONE launch per batch, the iterations loop on the device, everything per pair in LDS, all fp64:
//   1. LaserScanToLDP (:220-261): a reading is valid iff range_min < r < range_max; the valid points of both scans are
//      compacted in order into LDS (ref: qx, qy, qi; sens: px, py, pi), cos/sin from the handle's table (CreateCache).
//      The cloud forms load points instead (pl_compact_cloud: valid byte and finite x, y; float32 widened; index = position),
//      which is how a de-skewed scan is matched; from there on the two forms are one code.
//   2. per iteration, from x: each lane owns sens points; the nearest valid ref point by an exhaustive search, strict `<` in
//      ascending index (argmin's lowest index wins); j2 = the valid index neighbour of j1 that is closer (d_lo <= d_hi
//      prefers the lower one); the point-to-line distance.
//   3. remove doubles: per ref point a 64-bit minimum over the distances' bits (non-negative doubles order as their bits),
//      then the lowest sens order among the points AT that minimum -- together the (dist, sens order) minimum.  As the
//      restatement's lexsort does, EVERY valid sens point contends, also one whose correspondence was not accepted.
//   4. the survivors' rank = the number of survivors with a smaller distance, or an EQUAL distance and a LOWER sens order
//      (the tie rule of this library).  One ranking serves the trimmed cut (rank < m1) and the adaptive percentile (the
//      distance at rank ridx), because the trimmed list is a prefix of the sorted one.
//   5. the ten sums of A^T A and the four of A^T b, a fixed shuffle tree and a fixed order over the waves, so a pair's
//      record does not depend on the batch it is in; the closed-form solve (every lane does the same arithmetic on the same
//      sums: no hand-over): the 2x2 eigen-decomposition, every real root of the Lagrange quartic in lambda -- bracketed
//      between the quartic's critical points and bisected down to neighbouring doubles -- and the lowest-cost root.
// The loops are bounded by the beam count and by 128 bisection steps: no spins, no hand-overs between blocks, no scratch.
#include <cmath>

#include "common.hpp"

using namespace lslam;

namespace {

constexpr int kPlThreads = 256;
constexpr int kPlWaves = kPlThreads / 64;
constexpr int kPlMax = LSLAM_PLICP_MAX_READINGS;
constexpr int kPlTiles = (kPlMax + kPlThreads - 1) / kPlThreads;  // readings per thread: 8
constexpr int kPlSums = 16;                                       // 10 + 4 sums, padded
static_assert(sizeof(lslam_plicp_record) == 48, "lslam_plicp_record is 48 bytes");
static_assert(sizeof(lslam_plicp_odom_record) == 80, "lslam_plicp_odom_record is 80 bytes");
static_assert(kPlMax <= 65535, "indices are kept in 16 bits");

struct PlParams {  // what sm_icp reads, as the kernel wants it
  double max_d2, max_lin, max_ang, eps_xy, eps_th, max_perc, ad_order, ad_mult, range_min, range_max;
  int max_iter, p2l, doubles, pad;
};

struct PlShared {                       // 127 KB: one workgroup per CU
  double qx[kPlMax], qy[kPlMax];        // the valid ref points, ascending reading index
  double px[kPlMax], py[kPlMax];        // the valid sens points in the sens frame; sens order = this index
  double dist[kPlMax];                  // by sens order
  union {
    unsigned long long best[kPlMax];    // by ref point: the smallest distance (bits) of the sens points on it;
    double cd[kPlMax];                  // then the survivors' distances, compacted in any order
  };
  unsigned int owner[kPlMax];           // by ref point: the lowest sens order at `best`; then the survivors' ranks
  unsigned short cs[kPlMax];            // the survivors' sens order, beside cd
  unsigned short qi[kPlMax], pi[kPlMax];  // compacted index -> reading index
  unsigned short j1[kPlMax];            // by sens order: the ref point (compacted index)
  short j2[kPlMax];                     // the segment's second ref point (compacted index), -1: none
  unsigned char flag[kPlMax];           // bit 1: accepted before outlier rejection, bit 2: kept after it
  double red[kPlWaves][kPlSums];
  double ref_err;
  int wcnt[kPlTiles * kPlWaves];
  int n_surv, n_kept;
};

struct PlOut {
  double x[3], error;
  int valid, iterations, nvalid;
};

// LaserScanToLDP + the points: every thread returns the count.  Order-preserving (ballots per tile, wave counts).
__device__ int pl_compact(PlShared& sh, const float* __restrict__ r, int n, const PlParams& P, const double* __restrict__ tc,
                          const double* __restrict__ ts, double* ox, double* oy, unsigned short* oi) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double val[kPlTiles];
  unsigned long long bal[kPlTiles];
#pragma unroll
  for (int t = 0; t < kPlTiles; t++) {
    const int i = t * kPlThreads + tid;
    val[t] = i < n ? (double)r[i] : 0.0;
    bal[t] = __ballot(i < n && val[t] > P.range_min && val[t] < P.range_max);  // (:231; NaN compares false)
    if (lane == 0) sh.wcnt[t * kPlWaves + wv] = __popcll(bal[t]);
  }
  __syncthreads();
  int count = 0, pos[kPlTiles];
#pragma unroll
  for (int t = 0; t < kPlTiles; t++)
#pragma unroll
    for (int w = 0; w < kPlWaves; w++) {
      if (w == wv) pos[t] = count;
      count += sh.wcnt[t * kPlWaves + w];
    }
#pragma unroll
  for (int t = 0; t < kPlTiles; t++) {
    const int i = t * kPlThreads + tid;
    if ((bal[t] >> lane) & 1ull) {  // (only beams i < n are in the ballot; p <= i < kPlMax)
      const int p = pos[t] + __popcll(bal[t] & ((1ull << lane) - 1ull));
      ox[p] = val[t] * tc[i];
      oy[p] = val[t] * ts[i];
      oi[p] = (unsigned short)i;
    }
  }
  __syncthreads();
  return count;
}

// The cloud form of the loader (cloud_to_ldp in tools/plicp_cpu.py): point i takes part iff its valid byte is set (no bytes:
// every point) and x, y are finite; its coordinates are the float32 x, y widened, z is never read, no range window.  The
// reading index is i.  Same ballots and wave counts as pl_compact.  x, y of point i at p[stride * i], p[stride * i + 1].
__device__ int pl_compact_cloud(PlShared& sh, const float* __restrict__ p, int stride, const uint8_t* __restrict__ valid, int n,
                                double* ox, double* oy, unsigned short* oi) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float vx[kPlTiles], vy[kPlTiles];
  unsigned long long bal[kPlTiles];
#pragma unroll
  for (int t = 0; t < kPlTiles; t++) {
    const int i = t * kPlThreads + tid;
    const bool in = i < n;
    vx[t] = in ? p[(size_t)stride * i] : 0.0f;
    vy[t] = in ? p[(size_t)stride * i + 1] : 0.0f;
    const bool flagged = in && (!valid || valid[i] != 0);
    bal[t] = __ballot(flagged && isfinite(vx[t]) && isfinite(vy[t]));
    if (lane == 0) sh.wcnt[t * kPlWaves + wv] = __popcll(bal[t]);
  }
  __syncthreads();
  int count = 0, pos[kPlTiles];
#pragma unroll
  for (int t = 0; t < kPlTiles; t++)
#pragma unroll
    for (int w = 0; w < kPlWaves; w++) {
      if (w == wv) pos[t] = count;
      count += sh.wcnt[t * kPlWaves + w];
    }
#pragma unroll
  for (int t = 0; t < kPlTiles; t++) {
    const int i = t * kPlThreads + tid;
    if ((bal[t] >> lane) & 1ull) {  // (only points i < n are in the ballot; q <= i < kPlMax)
      const int q = pos[t] + __popcll(bal[t] & ((1ull << lane) - 1ull));
      ox[q] = (double)vx[t];
      oy[q] = (double)vy[t];
      oi[q] = (unsigned short)i;
    }
  }
  __syncthreads();
  return count;
}

// What pl_match loads a scan from: a row of ranges on the handle's beam table, or a cloud.
struct PlRangesSrc {
  const float* r;
  const double *tc, *ts;
  __device__ __forceinline__ int load(PlShared& sh, int n, const PlParams& P, double* ox, double* oy, unsigned short* oi) const {
    return pl_compact(sh, r, n, P, tc, ts, ox, oy, oi);
  }
};
struct PlCloudSrc {
  const float* p;        // x, y of point i at p[stride * i], p[stride * i + 1]
  int stride;            // 3: an xyz cloud; 2: a kept keyframe
  const uint8_t* valid;  // NULL: every point
  __device__ __forceinline__ int load(PlShared& sh, int n, const PlParams&, double* ox, double* oy, unsigned short* oi) const {
    return pl_compact_cloud(sh, p, stride, valid, n, ox, oy, oi);
  }
};

// v[i] <- the block's sum of v[i], the same in every thread and in a fixed order
template <int N>
__device__ __forceinline__ void pl_reduce(PlShared& sh, double (&v)[N]) {
  static_assert(N <= kPlSums, "");
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
    for (int w = 0; w < kPlWaves; w++) t += sh.red[w][i];
    v[i] = t;
  }
  __syncthreads();
}

// The sign change of fn in (lo, hi) by bisection down to neighbouring doubles; fn(lo) > 0 is lo_pos, fn(hi) > 0 is not.
template <typename F>
__device__ __forceinline__ double pl_bisect(F fn, double lo, double hi, bool lo_pos) {
#pragma unroll 1
  for (int i = 0; i < 128; i++) {
    const double mid = 0.5 * (lo + hi);
    if (!(mid > lo && mid < hi)) break;
    if ((fn(mid) > 0.0) == lo_pos) lo = mid; else hi = mid;
  }
  return 0.5 * (lo + hi);
}

// _solve_point_to_line from the sums m = A^T A (upper triangle, row-major: 00 01 02 03 11 12 13 22 23 33) and atb = A^T b
__device__ bool pl_solve(const double* m, const double* atb, double* sol) {
  const double m00 = m[0], m01 = m[1], m02 = m[2], m03 = m[3], m11 = m[4], m12 = m[5], m13 = m[6], m22 = m[7], m23 = m[8],
               m33 = m[9];
  const double g0 = -2.0 * atb[0], g1 = -2.0 * atb[1], g2 = -2.0 * atb[2], g3 = -2.0 * atb[3];
  const double det = m00 * m11 - m01 * m01;
  if (fabs(det) < 1e-12) return false;
  const double i00 = m11 / det, i01 = -m01 / det, i11 = m00 / det;  // ainv
  // w = ainv bb,  bb = [[m02, m03], [m12, m13]]
  const double w00 = i00 * m02 + i01 * m12, w01 = i00 * m03 + i01 * m13;
  const double w10 = i01 * m02 + i11 * m12, w11 = i01 * m03 + i11 * m13;
  // s2 = dd - bb^T w
  const double s00 = m22 - (m02 * w00 + m12 * w10), s01 = m23 - (m02 * w01 + m12 * w11);
  const double s10 = m23 - (m03 * w00 + m13 * w10), s11 = m33 - (m03 * w01 + m13 * w11);
  // h = g[2:] - bb^T ainv g[:2]
  const double ag0 = i00 * g0 + i01 * g1, ag1 = i01 * g0 + i11 * g1;
  const double h0 = g2 - (m02 * ag0 + m12 * ag1), h1 = g3 - (m03 * ag0 + m13 * ag1);
  // eigh of the lower triangle: e0 <= e1, v1 = (c, s), v0 = (-s, c)
  const double th = 0.5 * atan2(2.0 * s10, s00 - s11);
  const double c = cos(th), s = sin(th);
  const double mean = 0.5 * (s00 + s11), rad = hypot(0.5 * (s00 - s11), s10);
  const double e0 = mean - rad, e1 = mean + rad;
  const double hp0 = -s * h0 + c * h1, hp1 = c * h0 + s * h1;
  const double P0 = hp0 * hp0, P1 = hp1 * hp1;
  // The quartic in L is the Lagrange condition of the cost: |u| = 1 with u_i = -hp_i / (2 e_i + 2 L), that is
  //     (2L + 2e0)^2 (2L + 2e1)^2 = hp0^2 (2L + 2e1)^2 + hp1^2 (2L + 2e0)^2.
  // With y = L + mean and over 16:  f(y) = (y^2 - r^2)^2 - (P0 (y + r)^2 + P1 (y - r)^2) / 4, whose derivative is the
  // depressed cubic f'(y) = 4 y^3 - (4 r^2 + (P0 + P1) / 2) y - (P0 - P1) r / 2.
  // The real roots of f lie between its critical points, which lie between the turning points +-k of f'.  The constant term
  // of f' takes either sign, so a lone critical point lies on either side: three of them when f'(-k) > 0 > f'(k); one below
  // -k when f'(k) >= 0 (then f' > 0 from -k on); one above k otherwise (then f' <= 0 up to k).  (|(P0 - P1) r / 2| <= 8 k^3
  // whatever P0, P1 >= 0 and r are, with equality at P = 16 r^2 on one side alone: the lone cases are that tangency and
  // its rounding, on either side.)
  // A root is taken where f changes sign.  A tangent (double) root changes none and is not seen, where np.roots returns it as a
  // pair the helper may accept (|imag| <= 1e-9 max(1, |re|)) and evaluate: on such an input -- none is known -- the device can
  // choose another root than the helper, or none (the zero result).
  const double r2 = rad * rad;
  const double qs = 0.25 * (P0 + P1), qd = 0.5 * (P0 - P1) * rad;
  auto f = [&](double y) {
    const double w = y * y - r2;
    return w * w - 0.25 * (P0 * ((y + rad) * (y + rad)) + P1 * ((y - rad) * (y - rad)));
  };
  auto fd = [&](double y) { return (4.0 * y * y * y - (4.0 * r2 + 2.0 * qs) * y) - qd; };
  // Fujiwara's bound on y^4 + a2 y^2 + a1 y + a0:  a2 = -(2 r^2 + qs), a1 = -qd, a0 = r^4 - qs r^2
  const double R = 2.0 * fmax(fmax(sqrt(2.0 * r2 + qs), cbrt(fabs(qd))), sqrt(sqrt(fabs(r2 * (r2 - qs))))) + 1e-300;
  const double k3 = sqrt((4.0 * r2 + 2.0 * qs) / 12.0);
  // the critical points in ascending order; an absent one repeats its neighbour, which leaves its interval empty
  const bool below = fd(k3) >= 0.0, three = !below && fd(-k3) > 0.0;
  const double c1 = (three || below) ? pl_bisect(fd, -R, -k3, false) : -R;
  const double c2 = three ? pl_bisect(fd, -k3, k3, true) : c1;
  const double c3 = below ? c2 : pl_bisect(fd, k3, R, false);
  const double edge[5] = {-R, c1, c2, c3, R};
  bool have = false;
  double bcost = 0.0, bu0 = 0.0, bu1 = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double lo = edge[k], hi = edge[k + 1];
    const bool flo = f(lo) > 0.0, fhi = f(hi) > 0.0;
    if (flo == fhi) continue;
    const double y = pl_bisect(f, lo, hi, flo);
    const double den0 = 2.0 * (y - rad), den1 = 2.0 * (y + rad);  // 2 e + 2 L
    if (fabs(den0) < 1e-15 || fabs(den1) < 1e-15) continue;
    const double a0 = -hp0 / den0, a1 = -hp1 / den1;
    double u0 = -s * a0 + c * a1, u1 = c * a0 + s * a1;
    const double nu = sqrt(u0 * u0 + u1 * u1);
    if (nu < 1e-12) continue;
    u0 /= nu;
    u1 /= nu;
    const double cost = (u0 * (s00 * u0 + s01 * u1) + u1 * (s10 * u0 + s11 * u1)) + (h0 * u0 + h1 * u1);
    if (!have || cost < bcost) {
      have = true;
      bcost = cost; bu0 = u0; bu1 = u1;
    }
  }
  if (!have) return false;
  // t = -ainv (bb u + 0.5 g[:2])
  const double r0 = (m02 * bu0 + m03 * bu1) + 0.5 * g0, r1 = (m12 * bu0 + m13 * bu1) + 0.5 * g1;
  sol[0] = -(i00 * r0 + i01 * r1);
  sol[1] = -(i01 * r0 + i11 * r1);
  sol[2] = atan2(bu1, bu0);
  return true;
}

// neighbours, acceptance and the distance of sens point s, whose nearest ref point is k at d2 = dmin (sm_icp :150-161)
__device__ __forceinline__ void pl_correspond(PlShared& sh, const PlParams& P, int nr, int s, double wx, double wy, int k,
                                              double dmin) {
  const double inf = __builtin_inf();
  const int rk = sh.qi[k];
  double d_lo = inf, d_hi = inf;
  if (k > 0 && sh.qi[k - 1] == rk - 1) {
    const double dx = wx - sh.qx[k - 1], dy = wy - sh.qy[k - 1];
    d_lo = dx * dx + dy * dy;
  }
  if (k + 1 < nr && sh.qi[k + 1] == rk + 1) {
    const double dx = wx - sh.qx[k + 1], dy = wy - sh.qy[k + 1];
    d_hi = dx * dx + dy * dy;
  }
  const bool lower = d_lo <= d_hi;
  const bool any = fmin(d_lo, d_hi) < inf;
  const int k2 = any ? (lower ? k - 1 : k + 1) : -1;
  bool ok = dmin <= P.max_d2 && any;
  double nx = 0.0, ny = 0.0;
  if (any) {
    const double sx = sh.qx[k2] - sh.qx[k], sy = sh.qy[k2] - sh.qy[k];
    const double len = sqrt(sx * sx + sy * sy);
    ok = ok && len > 1e-12;
    if (ok) {
      nx = -sy / len;
      ny = sx / len;
    }
  }
  const double dx = wx - sh.qx[k], dy = wy - sh.qy[k];
  const double d = P.p2l ? fabs(dx * nx + dy * ny) : sqrt(dmin);
  sh.j1[s] = (unsigned short)k;
  sh.j2[s] = (short)k2;
  sh.dist[s] = d;
  sh.flag[s] = ok ? 2 : 0;
  if (P.doubles) atomicMin(&sh.best[k], (unsigned long long)__double_as_longlong(d));
}

// the unit normal of sens point s's segment (only called for accepted points: j2 >= 0, length > 1e-12)
__device__ __forceinline__ void pl_normal(const PlShared& sh, int s, double* nx, double* ny) {
  const int k = sh.j1[s], k2 = sh.j2[s];
  const double sx = sh.qx[k2] - sh.qx[k], sy = sh.qy[k2] - sh.qy[k];
  const double len = sqrt(sx * sx + sy * sy);
  *nx = -sy / len;
  *ny = sx / len;
}

// sm_icp(ref, sens, first guess g) for the whole block; every thread returns the same `out`.  dbg_*: per READING of the sens
// scan, or all NULL.  Src: PlRangesSrc or PlCloudSrc -- only the loader differs.
template <typename Src>
__device__ void pl_match(PlShared& sh, const PlParams& P, int n, const Src& src_ref, const Src& src_sens, double gx, double gy,
                         double gth, PlOut& out, int32_t* dbg_j1, int32_t* dbg_j2, uint8_t* dbg_flags) {
  const int tid = threadIdx.x, lane = tid & 63;
  out.x[0] = out.x[1] = out.x[2] = 0.0;
  out.error = __builtin_inf();
  out.valid = out.iterations = out.nvalid = 0;
  const int nr = src_ref.load(sh, n, P, sh.qx, sh.qy, sh.qi);
  const int ns = src_sens.load(sh, n, P, sh.px, sh.py, sh.pi);
  if (dbg_flags)
    for (int i = tid; i < n; i += kPlThreads) {
      dbg_j1[i] = -1;
      dbg_j2[i] = -1;
      dbg_flags[i] = 0;
    }
  bool searched = false, failed = nr < 3 || ns < 3;
  double x0 = gx, x1 = gy, x2 = gth, err = __builtin_inf();
  int it = 0, nvalid = 0;
#pragma unroll 1
  while (!failed && it < P.max_iter) {
    it++;
    // ---- correspondences
    for (int k = tid; k < nr; k += kPlThreads) {
      sh.best[k] = ~0ull;
      sh.owner[k] = 0xffffffffu;
    }
    if (tid == 0) sh.n_surv = sh.n_kept = 0;
    __syncthreads();
    const double c = cos(x2), s = sin(x2);
#pragma unroll 1
    for (int s0 = tid; s0 < ns; s0 += 2 * kPlThreads) {
      const bool two = s0 + kPlThreads < ns;
      const int s1 = two ? s0 + kPlThreads : s0;
      const double ax = (sh.px[s0] * c + sh.py[s0] * -s) + x0, ay = (sh.px[s0] * s + sh.py[s0] * c) + x1;
      const double bx = (sh.px[s1] * c + sh.py[s1] * -s) + x0, by = (sh.px[s1] * s + sh.py[s1] * c) + x1;
      double da = __builtin_inf(), db = __builtin_inf();
      int ka = 0, kb = 0;
#pragma unroll 4
      for (int k = 0; k < nr; k++) {
        const double qx = sh.qx[k], qy = sh.qy[k];
        const double ex = ax - qx, ey = ay - qy, fx = bx - qx, fy = by - qy;
        const double d0 = ex * ex + ey * ey, d1 = fx * fx + fy * fy;
        if (d0 < da) { da = d0; ka = k; }
        if (d1 < db) { db = d1; kb = k; }
      }
      pl_correspond(sh, P, nr, s0, ax, ay, ka, da);
      if (two) pl_correspond(sh, P, nr, s1, bx, by, kb, db);
    }
    searched = true;
    __syncthreads();
    // ---- doubles: the lowest sens order among the points at their ref point's minimum
    if (P.doubles) {
      for (int s0 = tid; s0 < ns; s0 += kPlThreads)
        if ((unsigned long long)__double_as_longlong(sh.dist[s0]) == sh.best[sh.j1[s0]]) atomicMin(&sh.owner[sh.j1[s0]], (unsigned)s0);
      __syncthreads();
    }
    // ---- the survivors, compacted in any order (cd lies over best: best is not read any more)
    for (int base = 0; base < ns; base += kPlThreads) {  // (block-uniform trip count: ballots inside)
      const int s0 = base + tid;
      const bool surv = s0 < ns && (sh.flag[s0] & 2) && (!P.doubles || sh.owner[sh.j1[s0]] == (unsigned)s0);
      const unsigned long long b = __ballot(surv);
      if (b) {
        int first = 0;
        if (lane == 0) first = atomicAdd(&sh.n_surv, __popcll(b));
        first = __shfl(first, 0);
        if (surv) {  // at most ns <= kPlMax survivors
          const int e = first + __popcll(b & ((1ull << lane) - 1ull));
          sh.cd[e] = sh.dist[s0];
          sh.cs[e] = (unsigned short)s0;
        }
      }
    }
    __syncthreads();
    const int cnt = sh.n_surv;
    if (cnt < 3) { failed = true; break; }
    // ---- rank, the trimmed cut and the adaptive threshold
    int m1 = (int)floor(P.max_perc * (double)cnt);
    m1 = min(max(3, m1), cnt);
    const int ridx = min(m1 - 1, (int)floor(P.ad_order * (double)m1));
    for (int e = tid; e < cnt; e += kPlThreads) {
      const double d = sh.cd[e];
      const unsigned so = sh.cs[e];
      int rank = 0;
      for (int t = 0; t < cnt; t++) {
        const double dt = sh.cd[t];
        rank += (dt < d || (dt == d && sh.cs[t] < so)) ? 1 : 0;
      }
      sh.owner[e] = (unsigned)rank;
      if (rank == ridx) sh.ref_err = d;
    }
    __syncthreads();
    const double thr = P.ad_mult * sh.ref_err + 1e-12;
    for (int base = 0; base < cnt; base += kPlThreads) {
      const int e = base + tid;
      const bool keep = e < cnt && (int)sh.owner[e] < m1 && sh.cd[e] <= thr;
      if (keep) sh.flag[sh.cs[e]] |= 4;
      const unsigned long long b = __ballot(keep);
      if (b && lane == 0) atomicAdd(&sh.n_kept, __popcll(b));
    }
    __syncthreads();
    const int nk = sh.n_kept;
    if (nk < 3) { failed = true; break; }
    // ---- the sums and the solve
    double sums[14];
#pragma unroll
    for (int i = 0; i < 14; i++) sums[i] = 0.0;
    for (int s0 = tid; s0 < ns; s0 += kPlThreads)
      if (sh.flag[s0] & 4) {
        double nx, ny;
        pl_normal(sh, s0, &nx, &ny);
        const double ppx = sh.px[s0], ppy = sh.py[s0];
        const int k = sh.j1[s0];
        const double a2 = nx * ppx + ny * ppy, a3 = -nx * ppy + ny * ppx, b = nx * sh.qx[k] + ny * sh.qy[k];
        sums[0] += nx * nx; sums[1] += nx * ny; sums[2] += nx * a2; sums[3] += nx * a3;
        sums[4] += ny * ny; sums[5] += ny * a2; sums[6] += ny * a3;
        sums[7] += a2 * a2; sums[8] += a2 * a3; sums[9] += a3 * a3;
        sums[10] += nx * b; sums[11] += ny * b; sums[12] += a2 * b; sums[13] += a3 * b;
      }
    pl_reduce(sh, sums);
    double sol[3];
    if (!pl_solve(sums, sums + 10, sol)) { failed = true; break; }
    nvalid = nk;
    // ---- the error of the solution and the step
    const double cs = cos(sol[2]), sn = sin(sol[2]);
    double e1[1] = {0.0};
    for (int s0 = tid; s0 < ns; s0 += kPlThreads)
      if (sh.flag[s0] & 4) {
        double nx, ny;
        pl_normal(sh, s0, &nx, &ny);
        const int k = sh.j1[s0];
        const double rx = ((sh.px[s0] * cs + sh.py[s0] * -sn) + sol[0]) - sh.qx[k];
        const double ry = ((sh.px[s0] * sn + sh.py[s0] * cs) + sol[1]) - sh.qy[k];
        const double res = rx * nx + ry * ny;
        e1[0] += res * res;
      }
    pl_reduce(sh, e1);
    err = e1[0];
    const double d0 = sol[0] - x0, d1 = sol[1] - x1, d2 = remainder(sol[2] - x2, 6.283185307179586);
    x0 = sol[0]; x1 = sol[1]; x2 = sol[2];
    if (hypot(d0, d1) < P.eps_xy && fabs(d2) < P.eps_th) break;
  }
  if (dbg_flags) {
    __syncthreads();
    for (int s0 = tid; s0 < ns; s0 += kPlThreads) {
      const int i = sh.pi[s0];
      dbg_flags[i] = searched ? (uint8_t)(1 | sh.flag[s0]) : (uint8_t)1;
      if (searched) {
        dbg_j1[i] = sh.qi[sh.j1[s0]];
        dbg_j2[i] = sh.j2[s0] >= 0 ? (int32_t)sh.qi[sh.j2[s0]] : -1;
      }
    }
  }
  __syncthreads();  // the next match of this block starts from a quiet LDS
  if (failed) return;  // sm_icp's early exits return the zero result
  out.x[0] = x0; out.x[1] = x1; out.x[2] = x2;
  out.error = err;
  out.iterations = it;
  out.nvalid = nvalid;
  const bool within = hypot(x0 - gx, x1 - gy) <= P.max_lin && fabs(remainder(x2 - gth, 6.283185307179586)) <= P.max_ang;
  out.valid = (within && nvalid >= 3) ? 1 : 0;
}

__device__ __forceinline__ void pl_store(lslam_plicp_record* rec, const PlOut& o) {
  lslam_plicp_record r;
  r.x[0] = o.x[0]; r.x[1] = o.x[1]; r.x[2] = o.x[2];
  r.error = o.error;
  r.valid = o.valid; r.iterations = o.iterations; r.nvalid = o.nvalid;
  r.reserved = 0;
  *rec = r;
}

__global__ void __launch_bounds__(kPlThreads)
k_plicp_match(PlParams P, int n, int ranges_stride, const float* __restrict__ ranges, const int32_t* __restrict__ pair_ref,
              const int32_t* __restrict__ pair_sens, const double* __restrict__ guess, const double* __restrict__ tc,
              const double* __restrict__ ts, lslam_plicp_record* __restrict__ out) {
  __shared__ PlShared sh;
  const size_t b = blockIdx.x;
  const double gx = guess ? guess[3 * b] : 0.0, gy = guess ? guess[3 * b + 1] : 0.0, gth = guess ? guess[3 * b + 2] : 0.0;
  PlOut o;
  pl_match(sh, P, n, PlRangesSrc{ranges + (size_t)pair_ref[b] * ranges_stride, tc, ts},
           PlRangesSrc{ranges + (size_t)pair_sens[b] * ranges_stride, tc, ts}, gx, gy, gth, o, nullptr, nullptr, nullptr);
  if (threadIdx.x == 0) pl_store(out + b, o);
}

// the same on clouds: cloud c at xyz + c * n * 3, its valid bytes (valid may be NULL) at valid + c * n
__global__ void __launch_bounds__(kPlThreads)
k_plicp_match_clouds(PlParams P, int n, const float* __restrict__ xyz, const uint8_t* __restrict__ valid,
                     const int32_t* __restrict__ pair_ref, const int32_t* __restrict__ pair_sens, const double* __restrict__ guess,
                     lslam_plicp_record* __restrict__ out) {
  __shared__ PlShared sh;
  const size_t b = blockIdx.x;
  const double gx = guess ? guess[3 * b] : 0.0, gy = guess ? guess[3 * b + 1] : 0.0, gth = guess ? guess[3 * b + 2] : 0.0;
  const size_t cr = (size_t)pair_ref[b], cs = (size_t)pair_sens[b];
  PlOut o;
  pl_match(sh, P, n, PlCloudSrc{xyz + cr * n * 3, 3, valid ? valid + cr * n : nullptr},
           PlCloudSrc{xyz + cs * n * 3, 3, valid ? valid + cs * n : nullptr}, gx, gy, gth, o, nullptr, nullptr, nullptr);
  if (threadIdx.x == 0) pl_store(out + b, o);
}

// one iteration from x_in, with the discrete decisions per reading (ranges: [ref | sens], n each)
__global__ void __launch_bounds__(kPlThreads)
k_plicp_debug(PlParams P, int n, const float* __restrict__ ranges, const double* __restrict__ x_in, const double* __restrict__ tc,
              const double* __restrict__ ts, int32_t* __restrict__ j1, int32_t* __restrict__ j2, uint8_t* __restrict__ flags,
              double* __restrict__ x_out) {
  __shared__ PlShared sh;
  PlOut o;
  P.max_iter = 1;
  pl_match(sh, P, n, PlRangesSrc{ranges, tc, ts}, PlRangesSrc{ranges + n, tc, ts}, x_in[0], x_in[1], x_in[2], o, j1, j2, flags);
  const double xs = threadIdx.x == 0 ? o.x[0] : threadIdx.x == 1 ? o.x[1] : o.x[2];
  if (threadIdx.x < 3) x_out[threadIdx.x] = o.iterations == 1 ? xs : __builtin_nan("");
}

// the same on two clouds (xyz: [ref | sens], n x 3 each; valid: [ref | sens] bytes, either may be NULL), per POINT of the sens cloud
__global__ void __launch_bounds__(kPlThreads)
k_plicp_debug_clouds(PlParams P, int n, const float* __restrict__ xyz, const uint8_t* __restrict__ ref_valid,
                     const uint8_t* __restrict__ sens_valid, const double* __restrict__ x_in, int32_t* __restrict__ j1,
                     int32_t* __restrict__ j2, uint8_t* __restrict__ flags, double* __restrict__ x_out) {
  __shared__ PlShared sh;
  PlOut o;
  P.max_iter = 1;
  pl_match(sh, P, n, PlCloudSrc{xyz, 3, ref_valid}, PlCloudSrc{xyz + (size_t)n * 3, 3, sens_valid}, x_in[0], x_in[1], x_in[2], o, j1,
           j2, flags);
  const double xs = threadIdx.x == 0 ? o.x[0] : threadIdx.x == 1 ? o.x[1] : o.x[2];
  if (threadIdx.x < 3) x_out[threadIdx.x] = o.iterations == 1 ? xs : __builtin_nan("");
}

PlParams pl_params(const lslam_plicp_params& p, double range_min, double range_max) {
  PlParams P;
  P.max_d2 = p.max_correspondence_dist * p.max_correspondence_dist;
  P.max_lin = p.max_linear_correction;
  P.max_ang = p.max_angular_correction_deg * (3.141592653589793 / 180.0);  // math.radians
  P.eps_xy = p.epsilon_xy;
  P.eps_th = p.epsilon_theta;
  P.max_perc = p.outliers_maxPerc;
  P.ad_order = p.outliers_adaptive_order;
  P.ad_mult = p.outliers_adaptive_mult;
  P.range_min = range_min;
  P.range_max = range_max;
  P.max_iter = p.max_iterations;
  P.p2l = p.use_point_to_line_distance ? 1 : 0;
  P.doubles = p.outliers_remove_doubles ? 1 : 0;
  P.pad = 0;
  return P;
}

// CreateCache (plicp_odometry.cc:237-252): cos / sin of angle_min + i * angle_increment, once per geometry
struct PlLaser {
  bool set = false;
  double range_min = 0, range_max = 0;
  DevBuf<double> d_table;  // [cos x kPlMax | sin x kPlMax]
  int upload(lslam_context* ctx, double angle_min, double angle_increment, double rmin, double rmax) {
    std::vector<double> t(2 * (size_t)kPlMax);
    for (int i = 0; i < kPlMax; i++) {
      const double a = angle_min + i * angle_increment;
      t[i] = std::cos(a);
      t[kPlMax + i] = std::sin(a);
    }
    LSLAM_HIP(ctx, d_table.reserve(t.size()));
    // (pageable memory: the copy has left `t` when the call returns)
    LSLAM_HIP(ctx, hipMemcpyAsync(d_table.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    range_min = rmin;
    range_max = rmax;
    set = true;
    return LSLAM_OK;
  }
  const double* tc() const { return d_table.p; }
  const double* ts() const { return d_table.p + kPlMax; }
};

}  // namespace

// ------------------------------------------------------------------------------------------
// lslam_plicp: the batched pair match.  The pair indices go up through a ring of pinned slots (the _dev form returns while
// its launch is still queued); everything else the host form needs belongs to the handle.
// ------------------------------------------------------------------------------------------
struct lslam_plicp {
  lslam_context* ctx = nullptr;
  lslam_plicp_params params;
  PlLaser laser;
  static constexpr int kSlots = 4;
  int32_t* h_pairs = nullptr;  // pinned: kSlots x [ref x cap | sens x cap]
  size_t pair_cap = 0;
  DevBuf<int32_t> d_pairs[kSlots];
  hipEvent_t slot_done[kSlots] = {};
  bool slot_in_flight[kSlots] = {};
  int next_slot = 0;
  // host form
  DevBuf<float> d_ranges, d_xyz;
  DevBuf<uint8_t> d_valid;
  DevBuf<double> d_guess;
  DevBuf<lslam_plicp_record> d_rec;
  unsigned char* h_io = nullptr;  // pinned: ranges or clouds and guesses up, records down
  size_t h_io_cap = 0;
  // debug
  DevBuf<unsigned char> d_dbg;
  int64_t n_pairs = 0, n_launches = 0, n_growths = 0, n_waits = 0;
};

namespace {

template <typename T>
int pl_reserve(lslam_plicp* f, DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return LSLAM_OK;
  LSLAM_HIP(f->ctx, b.reserve(n));
  f->n_growths++;
  return LSLAM_OK;
}

int pl_pinned(lslam_plicp* f, unsigned char** p, size_t* cap, size_t want) {
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

int pl_wait_slot(lslam_plicp* f, int q) {
  if (f->slot_in_flight[q] && hipEventQuery(f->slot_done[q]) != hipSuccess) {
    (void)hipGetLastError();  // hipErrorNotReady is no error
    LSLAM_HIP(f->ctx, hipEventSynchronize(f->slot_done[q]));
    f->n_waits++;
  }
  f->slot_in_flight[q] = false;
  return LSLAM_OK;
}

int pl_check(lslam_plicp* f, const char* who, int n_scans, int n_readings, const void* ranges, int ranges_stride, int n_pairs,
             const int32_t* pair_ref, const int32_t* pair_sens, const void* out) {
  if (!f || n_scans < 0 || n_readings < 0 || n_pairs < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (n_pairs == 0) return LSLAM_OK;
  if (!f->laser.set) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: lslam_plicp_set_laser has not been called", who);
  if (n_readings > LSLAM_PLICP_MAX_READINGS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d readings per scan (got %d)", who, LSLAM_PLICP_MAX_READINGS, n_readings);
  if (!ranges || !pair_ref || !pair_sens || !out || ranges_stride < n_readings)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: ranges, ranges_stride >= n_readings, pair_ref, pair_sens and out are required", who);
  for (int b = 0; b < n_pairs; b++)
    if (pair_ref[b] < 0 || pair_ref[b] >= n_scans || pair_sens[b] < 0 || pair_sens[b] >= n_scans)
      return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: pair %d (%d, %d) is outside the %d scans", who, b, pair_ref[b], pair_sens[b],
                       n_scans);
  return LSLAM_OK;
}

int pl_check_clouds(lslam_plicp* f, const char* who, int n_clouds, int n_points, const void* xyz, int n_pairs,
                    const int32_t* pair_ref, const int32_t* pair_sens, const void* out) {
  if (!f || n_clouds < 0 || n_points < 0 || n_pairs < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (n_pairs == 0) return LSLAM_OK;
  if (n_points > LSLAM_PLICP_MAX_READINGS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d points per cloud (got %d)", who, LSLAM_PLICP_MAX_READINGS, n_points);
  if (!xyz || !pair_ref || !pair_sens || !out)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: xyz, pair_ref, pair_sens and out are required", who);
  for (int b = 0; b < n_pairs; b++)
    if (pair_ref[b] < 0 || pair_ref[b] >= n_clouds || pair_sens[b] < 0 || pair_sens[b] >= n_clouds)
      return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: pair %d (%d, %d) is outside the %d clouds", who, b, pair_ref[b], pair_sens[b],
                       n_clouds);
  return LSLAM_OK;
}

// the pair indices up through the next pinned slot, then ONE launch for the whole batch: go(d_pair_ref, d_pair_sens)
template <typename Launch>
int pl_enqueue(lslam_plicp* f, int n_pairs, const int32_t* pair_ref, const int32_t* pair_sens, Launch&& go) {
  lslam_context* ctx = f->ctx;
  int rc;
  if ((size_t)n_pairs > f->pair_cap) {  // every slot grows together: none may be in flight
    for (int q = 0; q < lslam_plicp::kSlots; q++)
      if ((rc = pl_wait_slot(f, q))) return rc;
    size_t cap_bytes = f->pair_cap * 2 * sizeof(int32_t) * lslam_plicp::kSlots;
    const size_t per = (size_t)n_pairs + (size_t)n_pairs / 4 + 64;
    unsigned char* p = reinterpret_cast<unsigned char*>(f->h_pairs);
    rc = pl_pinned(f, &p, &cap_bytes, per * 2 * sizeof(int32_t) * lslam_plicp::kSlots);
    f->h_pairs = reinterpret_cast<int32_t*>(p);
    f->pair_cap = 0;
    if (rc) return rc;
    for (int q = 0; q < lslam_plicp::kSlots; q++)
      if ((rc = pl_reserve(f, f->d_pairs[q], 2 * per))) return rc;
    f->pair_cap = per;
  }
  const int q = f->next_slot;
  f->next_slot = (q + 1) % lslam_plicp::kSlots;
  if ((rc = pl_wait_slot(f, q))) return rc;
  int32_t* up = f->h_pairs + (size_t)q * 2 * f->pair_cap;
  memcpy(up, pair_ref, (size_t)n_pairs * sizeof(int32_t));
  memcpy(up + n_pairs, pair_sens, (size_t)n_pairs * sizeof(int32_t));
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_pairs[q].p, up, 2 * (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  go((const int32_t*)f->d_pairs[q].p, (const int32_t*)(f->d_pairs[q].p + n_pairs));
  LSLAM_HIP(ctx, hipGetLastError());
  LSLAM_HIP(ctx, hipEventRecord(f->slot_done[q], ctx->stream));
  f->slot_in_flight[q] = true;
  f->n_launches++;
  f->n_pairs += n_pairs;
  return LSLAM_OK;
}

int pl_enqueue_ranges(lslam_plicp* f, int n_readings, const float* d_ranges, int ranges_stride, int n_pairs, const int32_t* pair_ref,
                      const int32_t* pair_sens, const double* d_guess, lslam_plicp_record* d_out) {
  return pl_enqueue(f, n_pairs, pair_ref, pair_sens, [&](const int32_t* d_ref, const int32_t* d_sens) {
    launch(f->ctx, "plicp_match", k_plicp_match, dim3((unsigned)n_pairs), dim3(kPlThreads), 0,
           pl_params(f->params, f->laser.range_min, f->laser.range_max), n_readings, ranges_stride, d_ranges, d_ref, d_sens, d_guess,
           f->laser.tc(), f->laser.ts(), d_out);
  });
}

int pl_enqueue_clouds(lslam_plicp* f, int n_points, const float* d_xyz, const uint8_t* d_valid, int n_pairs, const int32_t* pair_ref,
                      const int32_t* pair_sens, const double* d_guess, lslam_plicp_record* d_out) {
  return pl_enqueue(f, n_pairs, pair_ref, pair_sens, [&](const int32_t* d_ref, const int32_t* d_sens) {
    launch(f->ctx, "plicp_match_clouds", k_plicp_match_clouds, dim3((unsigned)n_pairs), dim3(kPlThreads), 0,
           pl_params(f->params, 0.0, 0.0), n_points, d_xyz, d_valid, d_ref, d_sens, d_guess, d_out);
  });
}

}  // namespace

extern "C" {

void lslam_plicp_params_defaults(lslam_plicp_params* p) {
  if (!p) return;
  p->max_angular_correction_deg = 45.0;
  p->max_linear_correction = 1.0;
  p->max_iterations = 10;
  p->epsilon_xy = 0.000001;
  p->epsilon_theta = 0.000001;
  p->max_correspondence_dist = 1.0;
  p->use_point_to_line_distance = 1;
  p->outliers_maxPerc = 0.90;
  p->outliers_adaptive_order = 0.7;
  p->outliers_adaptive_mult = 2.0;
  p->outliers_remove_doubles = 1;
  p->reserved = 0;
}

int lslam_plicp_create(lslam_context* ctx, const lslam_plicp_params* params, lslam_plicp** out) {
  if (!ctx || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!params) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_plicp_create: params are required");
  if (params->max_iterations < 0) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_plicp_create: max_iterations must be >= 0");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_plicp* f = new lslam_plicp();
  f->ctx = ctx;
  f->params = *params;
  for (int q = 0; q < lslam_plicp::kSlots; q++) {
    hipError_t e = hipEventCreateWithFlags(&f->slot_done[q], hipEventDisableTiming);
    if (e != hipSuccess) {
      for (int k = 0; k < q; k++) (void)hipEventDestroy(f->slot_done[k]);
      delete f;
      return ctx->fail(LSLAM_ERR_HIP, "lslam_plicp_create: hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
    }
  }
  *out = f;
  return LSLAM_OK;
}

void lslam_plicp_destroy(lslam_plicp* f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  for (int q = 0; q < lslam_plicp::kSlots; q++) {
    (void)hipEventDestroy(f->slot_done[q]);
    f->d_pairs[q].release();
  }
  if (f->h_pairs) (void)hipHostFree(f->h_pairs);
  if (f->h_io) (void)hipHostFree(f->h_io);
  f->laser.d_table.release();
  f->d_ranges.release();
  f->d_xyz.release();
  f->d_valid.release();
  f->d_guess.release();
  f->d_rec.release();
  f->d_dbg.release();
  delete f;
}

int lslam_plicp_set_laser(lslam_plicp* f, double angle_min, double angle_increment, double range_min, double range_max) {
  if (!f) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (!std::isfinite(angle_min) || !std::isfinite(angle_increment) || !(range_min < range_max))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_plicp_set_laser: finite angles and range_min < range_max are required");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  return f->laser.upload(ctx, angle_min, angle_increment, range_min, range_max);
}

int lslam_plicp_stats(const lslam_plicp* f, int64_t out[4]) {
  if (!f || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = f->n_pairs; out[1] = f->n_launches; out[2] = f->n_growths; out[3] = f->n_waits;
  return LSLAM_OK;
}

int lslam_plicp_match_batch_dev(lslam_plicp* f, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride, int n_pairs,
                                const int32_t* pair_ref, const int32_t* pair_sens, const double* first_guess_dev,
                                lslam_plicp_record* out_dev) {
  int rc = pl_check(f, "lslam_plicp_match_batch_dev", n_scans, n_readings, ranges_dev, ranges_stride, n_pairs, pair_ref, pair_sens,
                    out_dev);
  if (rc || n_pairs == 0) return rc;
  LSLAM_HIP(f->ctx, hipSetDevice(f->ctx->device));
  return pl_enqueue_ranges(f, n_readings, ranges_dev, ranges_stride, n_pairs, pair_ref, pair_sens, first_guess_dev, out_dev);
}

int lslam_plicp_match_batch(lslam_plicp* f, int n_scans, int n_readings, const float* ranges, int ranges_stride, int n_pairs,
                            const int32_t* pair_ref, const int32_t* pair_sens, const double* first_guess, lslam_plicp_record* out) {
  int rc = pl_check(f, "lslam_plicp_match_batch", n_scans, n_readings, ranges, ranges_stride, n_pairs, pair_ref, pair_sens, out);
  if (rc || n_pairs == 0) return rc;
  lslam_context* ctx = f->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const int width = n_readings > 0 ? n_readings : 1;
  const size_t plane = (size_t)n_scans * width * sizeof(float);
  const size_t guess_bytes = first_guess ? (size_t)n_pairs * 3 * sizeof(double) : 0;
  const size_t rec_bytes = (size_t)n_pairs * sizeof(lslam_plicp_record);
  // pinned: [records | guesses | ranges] (every call ends with a wait: nothing in flight reads this buffer at the next call)
  if ((rc = pl_pinned(f, &f->h_io, &f->h_io_cap, rec_bytes + guess_bytes + plane)) ||
      (rc = pl_reserve(f, f->d_ranges, (size_t)n_scans * width)) || (rc = pl_reserve(f, f->d_rec, (size_t)n_pairs)) ||
      (first_guess && (rc = pl_reserve(f, f->d_guess, (size_t)n_pairs * 3))))
    return rc;
  unsigned char* const h_rec = f->h_io;
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
  if ((rc = pl_enqueue_ranges(f, n_readings, f->d_ranges.p, width, n_pairs, pair_ref, pair_sens, first_guess ? f->d_guess.p : nullptr,
                              f->d_rec.p)))
    return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(h_rec, f->d_rec.p, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  for (int q = 0; q < lslam_plicp::kSlots; q++) f->slot_in_flight[q] = false;  // the stream has drained
  memcpy(out, h_rec, rec_bytes);
  return LSLAM_OK;
}

int lslam_plicp_debug_iteration(lslam_plicp* f, const float* ranges_ref, const float* ranges_sens, int n, const double x_in[3],
                                int32_t* j1, int32_t* j2, uint8_t* flags, double x_out[3]) {
  if (!f) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (!ranges_ref || !ranges_sens || !x_in || !j1 || !j2 || !flags || !x_out || n < 0)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_plicp_debug_iteration: every pointer is required");
  if (!f->laser.set) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_plicp_debug_iteration: lslam_plicp_set_laser has not been called");
  if (n > LSLAM_PLICP_MAX_READINGS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_plicp_debug_iteration: at most %d readings per scan (got %d)", LSLAM_PLICP_MAX_READINGS, n);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  // device block: [x_in 3 | x_out 3] doubles, [ref | sens] floats, j1, j2 int32, flags bytes
  const size_t o_r = 6 * sizeof(double), o_j1 = o_r + 2 * (size_t)n * sizeof(float), o_j2 = o_j1 + (size_t)n * 4, o_f = o_j2 + (size_t)n * 4;
  const size_t bytes = o_f + (size_t)n;
  int rc;
  if ((rc = pl_reserve(f, f->d_dbg, bytes)) || (rc = pl_pinned(f, &f->h_io, &f->h_io_cap, bytes))) return rc;
  memcpy(f->h_io, x_in, 3 * sizeof(double));
  memset(f->h_io + 3 * sizeof(double), 0, 3 * sizeof(double));
  if (n) {
    memcpy(f->h_io + o_r, ranges_ref, (size_t)n * sizeof(float));
    memcpy(f->h_io + o_r + (size_t)n * sizeof(float), ranges_sens, (size_t)n * sizeof(float));
  }
  unsigned char* d = f->d_dbg.p;
  LSLAM_HIP(ctx, hipMemcpyAsync(d, f->h_io, o_j1, hipMemcpyHostToDevice, ctx->stream));
  launch(ctx, "plicp_debug", k_plicp_debug, dim3(1), dim3(kPlThreads), 0, pl_params(f->params, f->laser.range_min, f->laser.range_max), n,
         (const float*)(d + o_r), (const double*)d, f->laser.tc(), f->laser.ts(), (int32_t*)(d + o_j1), (int32_t*)(d + o_j2),
         (uint8_t*)(d + o_f), (double*)(d + 3 * sizeof(double)));
  LSLAM_HIP(ctx, hipGetLastError());
  f->n_launches++;
  LSLAM_HIP(ctx, hipMemcpyAsync(f->h_io, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  memcpy(x_out, f->h_io + 3 * sizeof(double), 3 * sizeof(double));
  if (n) {
    memcpy(j1, f->h_io + o_j1, (size_t)n * 4);
    memcpy(j2, f->h_io + o_j2, (size_t)n * 4);
    memcpy(flags, f->h_io + o_f, (size_t)n);
  }
  return LSLAM_OK;
}

int lslam_plicp_match_clouds_dev(lslam_plicp* f, int n_clouds, int n_points, const float* xyz_dev, const uint8_t* valid_dev, int n_pairs,
                                 const int32_t* pair_ref, const int32_t* pair_sens, const double* first_guess_dev,
                                 lslam_plicp_record* out_dev) {
  int rc = pl_check_clouds(f, "lslam_plicp_match_clouds_dev", n_clouds, n_points, xyz_dev, n_pairs, pair_ref, pair_sens, out_dev);
  if (rc || n_pairs == 0) return rc;
  LSLAM_HIP(f->ctx, hipSetDevice(f->ctx->device));
  return pl_enqueue_clouds(f, n_points, xyz_dev, valid_dev, n_pairs, pair_ref, pair_sens, first_guess_dev, out_dev);
}

int lslam_plicp_match_clouds(lslam_plicp* f, int n_clouds, int n_points, const float* xyz, const uint8_t* valid, int n_pairs,
                             const int32_t* pair_ref, const int32_t* pair_sens, const double* first_guess, lslam_plicp_record* out) {
  int rc = pl_check_clouds(f, "lslam_plicp_match_clouds", n_clouds, n_points, xyz, n_pairs, pair_ref, pair_sens, out);
  if (rc || n_pairs == 0) return rc;
  lslam_context* ctx = f->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t pts = (size_t)n_clouds * n_points;
  const size_t plane = pts * 3 * sizeof(float), flag_bytes = valid ? pts : 0;
  const size_t guess_bytes = first_guess ? (size_t)n_pairs * 3 * sizeof(double) : 0;
  const size_t rec_bytes = (size_t)n_pairs * sizeof(lslam_plicp_record);
  // pinned: [records | guesses | xyz | valid] (every call ends with a wait: nothing in flight reads this buffer at the next call)
  if ((rc = pl_pinned(f, &f->h_io, &f->h_io_cap, rec_bytes + guess_bytes + plane + flag_bytes)) ||
      (rc = pl_reserve(f, f->d_xyz, pts * 3 + 1)) || (rc = pl_reserve(f, f->d_rec, (size_t)n_pairs)) ||
      (valid && (rc = pl_reserve(f, f->d_valid, pts + 1))) || (first_guess && (rc = pl_reserve(f, f->d_guess, (size_t)n_pairs * 3))))
    return rc;
  unsigned char* const h_rec = f->h_io;
  double* const h_guess = reinterpret_cast<double*>(f->h_io + rec_bytes);
  unsigned char* const h_xyz = f->h_io + rec_bytes + guess_bytes;
  unsigned char* const h_valid = h_xyz + plane;
  if (pts) {
    memcpy(h_xyz, xyz, plane);
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_xyz.p, h_xyz, plane, hipMemcpyHostToDevice, ctx->stream));
    if (valid) {
      memcpy(h_valid, valid, flag_bytes);
      LSLAM_HIP(ctx, hipMemcpyAsync(f->d_valid.p, h_valid, flag_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
  }
  if (first_guess) {
    memcpy(h_guess, first_guess, guess_bytes);
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_guess.p, h_guess, guess_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  if ((rc = pl_enqueue_clouds(f, n_points, f->d_xyz.p, valid ? f->d_valid.p : nullptr, n_pairs, pair_ref, pair_sens,
                              first_guess ? f->d_guess.p : nullptr, f->d_rec.p)))
    return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(h_rec, f->d_rec.p, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  for (int q = 0; q < lslam_plicp::kSlots; q++) f->slot_in_flight[q] = false;  // the stream has drained
  memcpy(out, h_rec, rec_bytes);
  return LSLAM_OK;
}

int lslam_plicp_debug_iteration_clouds(lslam_plicp* f, const float* ref_xyz, const float* sens_xyz, const uint8_t* ref_valid,
                                       const uint8_t* sens_valid, int n, const double x_in[3], int32_t* j1, int32_t* j2,
                                       uint8_t* flags, double x_out[3]) {
  if (!f) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (!ref_xyz || !sens_xyz || !x_in || !j1 || !j2 || !flags || !x_out || n < 0)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_plicp_debug_iteration_clouds: every pointer but the valid bytes is required");
  if (n > LSLAM_PLICP_MAX_READINGS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_plicp_debug_iteration_clouds: at most %d points per cloud (got %d)",
                     LSLAM_PLICP_MAX_READINGS, n);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  // device block: [x_in 3 | x_out 3] doubles, [ref | sens] xyz floats, j1, j2 int32, [ref | sens] valid bytes, flags bytes
  const size_t o_c = 6 * sizeof(double), o_j1 = o_c + 6 * (size_t)n * sizeof(float), o_j2 = o_j1 + (size_t)n * 4;
  const size_t o_v = o_j2 + (size_t)n * 4, o_f = o_v + 2 * (size_t)n;
  const size_t bytes = o_f + (size_t)n;
  int rc;
  if ((rc = pl_reserve(f, f->d_dbg, bytes)) || (rc = pl_pinned(f, &f->h_io, &f->h_io_cap, bytes))) return rc;
  memset(f->h_io, 0, bytes);
  memcpy(f->h_io, x_in, 3 * sizeof(double));
  if (n) {
    memcpy(f->h_io + o_c, ref_xyz, 3 * (size_t)n * sizeof(float));
    memcpy(f->h_io + o_c + 3 * (size_t)n * sizeof(float), sens_xyz, 3 * (size_t)n * sizeof(float));
    if (ref_valid) memcpy(f->h_io + o_v, ref_valid, (size_t)n);
    if (sens_valid) memcpy(f->h_io + o_v + n, sens_valid, (size_t)n);
  }
  unsigned char* d = f->d_dbg.p;
  LSLAM_HIP(ctx, hipMemcpyAsync(d, f->h_io, bytes, hipMemcpyHostToDevice, ctx->stream));
  launch(ctx, "plicp_debug_clouds", k_plicp_debug_clouds, dim3(1), dim3(kPlThreads), 0, pl_params(f->params, 0.0, 0.0), n,
         (const float*)(d + o_c), (const uint8_t*)(ref_valid ? d + o_v : nullptr), (const uint8_t*)(sens_valid ? d + o_v + n : nullptr),
         (const double*)d, (int32_t*)(d + o_j1), (int32_t*)(d + o_j2), (uint8_t*)(d + o_f), (double*)(d + 3 * sizeof(double)));
  LSLAM_HIP(ctx, hipGetLastError());
  f->n_launches++;
  LSLAM_HIP(ctx, hipMemcpyAsync(f->h_io, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  memcpy(x_out, f->h_io + 3 * sizeof(double), 3 * sizeof(double));
  if (n) {
    memcpy(j1, f->h_io + o_j1, (size_t)n * 4);
    memcpy(j2, f->h_io + o_j2, (size_t)n * 4);
    memcpy(flags, f->h_io + o_f, (size_t)n);
  }
  return LSLAM_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// lslam_plicp_odom: the node of plicp_odometry.cc for R independent tracks.  One launch per call, a workgroup per track
// that walks the track's scans in order through pl_match; SE(2) in double.  The state lives in a device block; the
// keyframe scan is a row of this call's ranges while the call runs and is copied to the handle's HBM row at its end.
// ------------------------------------------------------------------------------------------
namespace {

struct Se2 {
  double x, y, th;
};
__device__ __forceinline__ double se2_yaw(double th) { return atan2(sin(th), cos(th)); }  // tf2::getYaw of the rotation
__device__ __forceinline__ Se2 se2_mul(const Se2& a, const Se2& b) {
  const double c = cos(a.th), s = sin(a.th);
  return Se2{a.x + (c * b.x - s * b.y), a.y + (s * b.x + c * b.y), se2_yaw(a.th + b.th)};
}
__device__ __forceinline__ Se2 se2_inv(const Se2& a) {
  const double c = cos(a.th), s = sin(a.th);
  return Se2{-(c * a.x + s * a.y), -(-s * a.x + c * a.y), se2_yaw(-a.th)};
}

struct PlOdomConsts {
  double kf_lin_sq, kf_ang;
  double b2l[3];
  int kf_count, pad;
};
static_assert(sizeof(lslam_plicp_odom_track) == 80, "lslam_plicp_odom_track is 80 bytes");

struct PlOdomRun {  // a track while its workgroup walks it
  lslam_plicp_odom_track st;
  Se2 base, kf, b2l, l2b;
};

__device__ __forceinline__ PlOdomRun pl_odom_open(const lslam_plicp_odom_track& st, const PlOdomConsts& K) {
  PlOdomRun R;
  R.st = st;
  R.base = Se2{st.base_in_odom[0], st.base_in_odom[1], st.base_in_odom[2]};
  R.kf = Se2{st.keyframe[0], st.keyframe[1], st.keyframe[2]};
  R.b2l = Se2{K.b2l[0], K.b2l[1], K.b2l[2]};
  R.l2b = se2_inv(R.b2l);
  return R;
}

__device__ __forceinline__ void pl_odom_close(PlOdomRun& R, lslam_plicp_odom_track* state) {
  R.st.base_in_odom[0] = R.base.x; R.st.base_in_odom[1] = R.base.y; R.st.base_in_odom[2] = R.base.th;
  R.st.keyframe[0] = R.kf.x; R.st.keyframe[1] = R.kf.y; R.st.keyframe[2] = R.kf.th;
  *state = R.st;
}

// ScanCallback for one scan `cur` of a track whose keyframe scan is `ref`: fills rec (zeroed by the caller) and returns whether
// `cur` is the keyframe scan from now on.  The node's arithmetic, for either kind of scan.
template <typename Src>
__device__ __forceinline__ bool pl_odom_step(PlShared& sh, const PlParams& P, const PlOdomConsts& K, int n, PlOdomRun& R,
                                             const Src& ref, const Src& cur, double stamp, lslam_plicp_odom_record& rec) {
  lslam_plicp_odom_track& st = R.st;
  Se2 &base = R.base, &kf = R.kf;
  const Se2 &b2l = R.b2l, &l2b = R.l2b;
  bool fresh;
  if (!st.initialized) {  // (:196-212)
    st.initialized = 1;
    fresh = true;
    st.last_icp_time = stamp;
    rec.flags = 3;
  } else {
    const double dt = stamp - st.last_icp_time;
    // GetPrediction (:442-456), literally: linear.y and linear.z are never set, a negative speed predicts nothing
    const Se2 pred{st.velocity[0] < 1e-6 ? 0.0 : dt * st.velocity[0], 0.0, 0.0};
    const Se2 pc = se2_mul(pred, se2_mul(base, se2_inv(kf)));                                         // :361
    const Se2 pcl = se2_mul(se2_mul(se2_mul(se2_mul(l2b, se2_inv(base)), pc), base), b2l);            // :366
    PlOut o;
    pl_match(sh, P, n, ref, cur, pcl.x, pcl.y, se2_yaw(pcl.th), o, nullptr, nullptr, nullptr);
    Se2 corr{0.0, 0.0, 0.0};  // an invalid match: the identity (the reference reads an uninitialised transform)
    if (o.valid) {            // :399-413
      corr = se2_mul(se2_mul(b2l, Se2{o.x[0], o.x[1], o.x[2]}), l2b);
      base = se2_mul(kf, corr);
      st.velocity[0] = corr.x / dt;
      st.velocity[1] = se2_yaw(corr.th) / dt;
    }
    // NewKeyframeNeeded (:498-517)
    st.scan_count++;
    if (fabs(se2_yaw(corr.th)) > K.kf_ang) {
      fresh = true;
    } else if (st.scan_count == K.kf_count) {
      st.scan_count = 0;
      fresh = true;
    } else {
      fresh = corr.x * corr.x + corr.y * corr.y > K.kf_lin_sq;
    }
    if (fresh) kf = base;
    st.last_icp_time = stamp;
    rec.x[0] = o.x[0]; rec.x[1] = o.x[1]; rec.x[2] = o.x[2];
    rec.error = o.error;
    rec.valid = o.valid; rec.iterations = o.iterations; rec.nvalid = o.nvalid;
    rec.flags = fresh ? 2 : 0;
  }
  rec.base_in_odom[0] = base.x; rec.base_in_odom[1] = base.y; rec.base_in_odom[2] = base.th;
  return fresh;
}

__global__ void __launch_bounds__(kPlThreads)
k_plicp_odom(PlParams P, PlOdomConsts K, int n_tracks, int n_steps, int n, int ranges_stride, const float* __restrict__ ranges,
             const double* __restrict__ stamps, const uint8_t* __restrict__ active, const double* __restrict__ tc,
             const double* __restrict__ ts, lslam_plicp_odom_track* __restrict__ state, float* __restrict__ kf_scans,
             lslam_plicp_odom_record* __restrict__ out) {
  __shared__ PlShared sh;
  const int tid = threadIdx.x, track = blockIdx.x;
  PlOdomRun R = pl_odom_open(state[track], K);
  float* const kf_row = kf_scans + (size_t)track * kPlMax;
  const float* ref = kf_row;
  int ref_step = -1;
#pragma unroll 1
  for (int step = 0; step < n_steps; step++) {
    const size_t idx = (size_t)step * n_tracks + track;
    lslam_plicp_odom_record rec;
    memset(&rec, 0, sizeof rec);
    if (active && !active[idx]) {
      rec.iterations = -1;
      if (tid == 0) out[idx] = rec;
      continue;
    }
    const float* cur = ranges + idx * (size_t)ranges_stride;
    if (pl_odom_step(sh, P, K, n, R, PlRangesSrc{ref, tc, ts}, PlRangesSrc{cur, tc, ts}, stamps[idx], rec)) {
      ref = cur;
      ref_step = step;
    }
    if (tid == 0) out[idx] = rec;
  }
  if (ref_step >= 0)  // the keyframe scan outlives the call
    for (int i = tid; i < n; i += kPlThreads) kf_row[i] = ref[i];
  if (tid == 0) pl_odom_close(R, state + track);
}

// One track's clouds of a call: step k's cloud at xyz + k * step_rows * n * 3, its valid bytes at valid + k * step_rows * n
// (NULL: every point), its take word at take + k * take_stride (NULL: every step).  step_rows: 1 for a block per track, the
// track count for the host form's step-major block.
struct PlTrackClouds {
  const float* xyz;
  const uint8_t* valid;
  const int32_t* take;
};

// The node on clouds, gated: entry (step, track) is TAKEN iff active says so (NULL: all) and its take word is > 0 (no words:
// all).  An entry that is not taken touches nothing: neither the state nor the keyframe, and its stamp and cloud are not
// read.  The keyframe is kept per track as x, y float32 (kf_xy, two per point) and the valid byte (kf_valid).
__global__ void __launch_bounds__(kPlThreads)
k_plicp_odom_clouds(PlParams P, PlOdomConsts K, int n_tracks, int n_steps, int n, const PlTrackClouds* __restrict__ tracks,
                    int step_rows, int take_stride, const double* __restrict__ stamps, const uint8_t* __restrict__ active,
                    lslam_plicp_odom_track* __restrict__ state, float* __restrict__ kf_xy, uint8_t* __restrict__ kf_valid,
                    lslam_plicp_odom_record* __restrict__ out) {
  __shared__ PlShared sh;
  const int tid = threadIdx.x, track = blockIdx.x;
  PlOdomRun R = pl_odom_open(state[track], K);
  const PlTrackClouds T = tracks[track];
  float* const kf_row = kf_xy + (size_t)track * kPlMax * 2;
  uint8_t* const kf_flag = kf_valid + (size_t)track * kPlMax;
  PlCloudSrc ref{kf_row, 2, kf_flag};
  int ref_step = -1;
#pragma unroll 1
  for (int step = 0; step < n_steps; step++) {
    const size_t idx = (size_t)step * n_tracks + track;
    lslam_plicp_odom_record rec;
    memset(&rec, 0, sizeof rec);
    const bool taken = (!active || active[idx]) && (!T.take || T.take[(size_t)step * take_stride] > 0);
    if (!taken) {
      rec.iterations = -1;
      if (tid == 0) out[idx] = rec;
      continue;
    }
    const size_t row = (size_t)step * step_rows;
    const PlCloudSrc cur{T.xyz + row * n * 3, 3, T.valid ? T.valid + row * n : nullptr};
    if (pl_odom_step(sh, P, K, n, R, ref, cur, stamps[idx], rec)) {
      ref = cur;
      ref_step = step;
    }
    if (tid == 0) out[idx] = rec;
  }
  if (ref_step >= 0)  // the keyframe cloud outlives the call
    for (int i = tid; i < n; i += kPlThreads) {
      kf_row[2 * i] = ref.p[(size_t)3 * i];
      kf_row[2 * i + 1] = ref.p[(size_t)3 * i + 1];
      kf_flag[i] = ref.valid ? ref.valid[i] : (uint8_t)1;
    }
  if (tid == 0) pl_odom_close(R, state + track);
}

}  // namespace

struct lslam_plicp_odom {
  lslam_context* ctx = nullptr;
  lslam_plicp_params params;
  PlLaser laser;
  PlOdomConsts consts;
  int n_tracks = 0, n_readings = -1;  // the beam count of the keyframe scans held (-1: none yet)
  bool clouds = false;                // with n_readings >= 0: the keyframes held are clouds, not range rows
  DevBuf<lslam_plicp_odom_track> d_state;
  DevBuf<float> d_kf, d_ranges;
  DevBuf<float> d_kf_xy, d_xyz;       // cloud calls: the keyframe clouds' x, y; the host form's clouds
  DevBuf<uint8_t> d_kf_valid, d_valid;
  DevBuf<PlTrackClouds> d_tracks;
  DevBuf<double> d_stamps;
  DevBuf<uint8_t> d_active;
  DevBuf<lslam_plicp_odom_record> d_rec;
  unsigned char* h_io = nullptr;
  size_t h_io_cap = 0;
  int64_t n_scans = 0, n_launches = 0, n_growths = 0, n_waits = 0;
};

namespace {

template <typename T>
int plo_reserve(lslam_plicp_odom* f, DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return LSLAM_OK;
  LSLAM_HIP(f->ctx, b.reserve(n));
  f->n_growths++;
  return LSLAM_OK;
}

// Both cloud forms of the node.  Host form: xyz_h (and valid_h, take_h) are step-major host arrays.  Dev form: xyz_h is NULL
// and xyz_dev / valid_dev / take_dev are host tables of one device pointer per track.  Every refusal comes before anything is
// enqueued or reserved.  One launch, one host wait.
int plo_clouds(lslam_plicp_odom* f, const char* who, int n_steps, int n_points, const float* xyz_h, const uint8_t* valid_h,
               const uint8_t* take_h, const float* const* xyz_dev, const uint8_t* const* valid_dev, const int32_t* const* take_dev,
               int take_stride, const double* stamps, const uint8_t* active, lslam_plicp_odom_record* out) {
  lslam_context* ctx = f->ctx;
  const bool host = xyz_h != nullptr;
  const int R = f->n_tracks;
  if (n_points > LSLAM_PLICP_MAX_READINGS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d points per cloud (got %d)", who, LSLAM_PLICP_MAX_READINGS, n_points);
  if (!stamps || !out || (!host && !xyz_dev))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: xyz, stamps and out are required", who);
  if (!host) {
    for (int m = 0; m < R; m++)
      if (!xyz_dev[m]) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: track %d has no cloud block", who, m);
    if (take_dev && take_stride < 1) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: take_stride must be at least 1 word", who);
  }
  if (f->n_readings >= 0 && !f->clouds)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: the keyframes held are range rows, this call brings clouds (reset first)", who);
  if (f->n_readings >= 0 && f->n_readings != n_points)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: the keyframe clouds have %d points, this call %d (reset first)", who, f->n_readings,
                     n_points);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t S = (size_t)n_steps * R, pts = S * n_points;
  const size_t rec_bytes = S * sizeof(lslam_plicp_odom_record), st_bytes = S * sizeof(double);
  const size_t tab_bytes = (size_t)R * sizeof(PlTrackClouds);
  const size_t plane = host ? pts * 3 * sizeof(float) : 0, flag_bytes = host && valid_h ? pts : 0;
  const bool gate = active || (host && take_h);  // the host form's take bytes go up folded into the active bytes
  // pinned: [records | stamps | track table | xyz | valid | active]
  const size_t want = rec_bytes + st_bytes + tab_bytes + plane + flag_bytes + S;
  int rc;
  if (want > f->h_io_cap) {
    if (f->h_io) (void)hipHostFree(f->h_io);
    f->h_io = nullptr;
    f->h_io_cap = 0;
    const size_t cap = want + want / 4 + 256;
    LSLAM_HIP(ctx, hipHostMalloc((void**)&f->h_io, cap, hipHostMallocDefault));
    f->h_io_cap = cap;
    f->n_growths++;
  }
  if ((rc = plo_reserve(f, f->d_kf_xy, (size_t)R * kPlMax * 2)) || (rc = plo_reserve(f, f->d_kf_valid, (size_t)R * kPlMax)) ||
      (rc = plo_reserve(f, f->d_tracks, (size_t)R)) || (rc = plo_reserve(f, f->d_stamps, S)) || (rc = plo_reserve(f, f->d_rec, S)) ||
      (gate && (rc = plo_reserve(f, f->d_active, S))) || (host && (rc = plo_reserve(f, f->d_xyz, pts * 3 + 1))) ||
      (flag_bytes && (rc = plo_reserve(f, f->d_valid, pts))))
    return rc;
  unsigned char* const h_rec = f->h_io;
  double* const h_st = reinterpret_cast<double*>(f->h_io + rec_bytes);
  PlTrackClouds* const h_tab = reinterpret_cast<PlTrackClouds*>(f->h_io + rec_bytes + st_bytes);
  unsigned char* const h_xyz = f->h_io + rec_bytes + st_bytes + tab_bytes;
  unsigned char* const h_valid = h_xyz + plane;
  uint8_t* const h_act = h_valid + flag_bytes;
  for (int m = 0; m < R; m++) {
    if (host)
      h_tab[m] = PlTrackClouds{f->d_xyz.p + (size_t)m * n_points * 3, flag_bytes ? f->d_valid.p + (size_t)m * n_points : nullptr, nullptr};
    else
      h_tab[m] = PlTrackClouds{xyz_dev[m], valid_dev ? valid_dev[m] : nullptr, take_dev ? take_dev[m] : nullptr};
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_tracks.p, h_tab, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
  memcpy(h_st, stamps, st_bytes);
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_stamps.p, h_st, st_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (plane) {
    memcpy(h_xyz, xyz_h, plane);
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_xyz.p, h_xyz, plane, hipMemcpyHostToDevice, ctx->stream));
  }
  if (flag_bytes) {
    memcpy(h_valid, valid_h, flag_bytes);
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_valid.p, h_valid, flag_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  if (gate) {
    for (size_t k = 0; k < S; k++) h_act[k] = ((!active || active[k]) && (!(host && take_h) || take_h[k])) ? 1 : 0;
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_active.p, h_act, S, hipMemcpyHostToDevice, ctx->stream));
  }
  launch(ctx, "plicp_odom_clouds", k_plicp_odom_clouds, dim3((unsigned)R), dim3(kPlThreads), 0, pl_params(f->params, 0.0, 0.0),
         f->consts, R, n_steps, n_points, (const PlTrackClouds*)f->d_tracks.p, host ? R : 1, host ? 1 : take_stride,
         (const double*)f->d_stamps.p, (const uint8_t*)(gate ? f->d_active.p : nullptr), f->d_state.p, f->d_kf_xy.p, f->d_kf_valid.p,
         f->d_rec.p);
  LSLAM_HIP(ctx, hipGetLastError());
  f->n_launches++;
  f->n_readings = n_points;
  f->clouds = true;
  LSLAM_HIP(ctx, hipMemcpyAsync(h_rec, f->d_rec.p, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  memcpy(out, h_rec, rec_bytes);
  for (size_t k = 0; k < S; k++) f->n_scans += out[k].iterations != -1 ? 1 : 0;
  return LSLAM_OK;
}

}  // namespace

extern "C" {

int lslam_plicp_odom_create(lslam_context* ctx, const lslam_plicp_params* params, int n_tracks, double kf_dist_linear,
                            double kf_dist_angular, int kf_scan_count, const double base_to_laser[3], lslam_plicp_odom** out) {
  if (!ctx || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!params || n_tracks < 1 || n_tracks > 65535 || params->max_iterations < 0)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_plicp_odom_create: params and 1 <= n_tracks <= 65535 are required");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_plicp_odom* f = new lslam_plicp_odom();
  f->ctx = ctx;
  f->params = *params;
  f->n_tracks = n_tracks;
  f->consts.kf_lin_sq = kf_dist_linear * kf_dist_linear;  // kf_dist_linear_sq_ (:104)
  f->consts.kf_ang = kf_dist_angular;
  f->consts.kf_count = kf_scan_count;
  f->consts.pad = 0;
  for (int i = 0; i < 3; i++) f->consts.b2l[i] = base_to_laser ? base_to_laser[i] : 0.0;
  hipError_t e = f->d_state.reserve((size_t)n_tracks);
  if (e == hipSuccess) e = f->d_kf.reserve((size_t)n_tracks * kPlMax);
  if (e == hipSuccess) e = hipMemsetAsync(f->d_state.p, 0, (size_t)n_tracks * sizeof(lslam_plicp_odom_track), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->d_kf.p, 0, (size_t)n_tracks * kPlMax * sizeof(float), ctx->stream);
  if (e != hipSuccess) {
    f->d_state.release();
    f->d_kf.release();
    delete f;
    return ctx->fail(LSLAM_ERR_HIP, "lslam_plicp_odom_create: %s", hipGetErrorString(e));
  }
  *out = f;
  return LSLAM_OK;
}

void lslam_plicp_odom_destroy(lslam_plicp_odom* f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  if (f->h_io) (void)hipHostFree(f->h_io);
  f->laser.d_table.release();
  f->d_state.release();
  f->d_kf.release();
  f->d_kf_xy.release();
  f->d_kf_valid.release();
  f->d_xyz.release();
  f->d_valid.release();
  f->d_tracks.release();
  f->d_ranges.release();
  f->d_stamps.release();
  f->d_active.release();
  f->d_rec.release();
  delete f;
}

int lslam_plicp_odom_set_laser(lslam_plicp_odom* f, double angle_min, double angle_increment, double range_min, double range_max) {
  if (!f) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  if (!std::isfinite(angle_min) || !std::isfinite(angle_increment) || !(range_min < range_max))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_plicp_odom_set_laser: finite angles and range_min < range_max are required");
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  return f->laser.upload(ctx, angle_min, angle_increment, range_min, range_max);
}

int lslam_plicp_odom_reset(lslam_plicp_odom* f) {
  if (!f) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hipMemsetAsync(f->d_state.p, 0, (size_t)f->n_tracks * sizeof(lslam_plicp_odom_track), ctx->stream));
  f->n_readings = -1;
  return LSLAM_OK;
}

int lslam_plicp_odom_state(lslam_plicp_odom* f, lslam_plicp_odom_track* out) {
  if (!f || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = f->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hipMemcpyAsync(out, f->d_state.p, (size_t)f->n_tracks * sizeof(lslam_plicp_odom_track), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  return LSLAM_OK;
}

int lslam_plicp_odom_stats(const lslam_plicp_odom* f, int64_t out[4]) {
  if (!f || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = f->n_scans; out[1] = f->n_launches; out[2] = f->n_growths; out[3] = f->n_waits;
  return LSLAM_OK;
}

int lslam_plicp_odom_process_many(lslam_plicp_odom* f, int n_steps, int n_readings, const float* ranges, int ranges_stride,
                                  const double* stamps, const uint8_t* active, lslam_plicp_odom_record* out) {
  if (!f || n_steps < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  lslam_context* ctx = f->ctx;
  const char* who = "lslam_plicp_odom_process_many";
  if (!f->laser.set) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: lslam_plicp_odom_set_laser has not been called", who);
  if (n_readings > LSLAM_PLICP_MAX_READINGS)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d readings per scan (got %d)", who, LSLAM_PLICP_MAX_READINGS, n_readings);
  if (!ranges || !stamps || !out || ranges_stride < n_readings)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: ranges, ranges_stride >= n_readings, stamps and out are required", who);
  if (f->n_readings >= 0 && f->n_readings != n_readings)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: the keyframe scans have %d readings, this call %d (reset first)", who, f->n_readings,
                     n_readings);
  if (f->n_readings >= 0 && f->clouds)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: the keyframes held are clouds, this call brings ranges (reset first)", who);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t S = (size_t)n_steps * f->n_tracks;
  const int width = n_readings > 0 ? n_readings : 1;
  const size_t plane = S * width * sizeof(float), rec_bytes = S * sizeof(lslam_plicp_odom_record), st_bytes = S * sizeof(double);
  // pinned: [records | stamps | ranges | active]
  const size_t want = rec_bytes + st_bytes + plane + S;
  int rc;
  if (want > f->h_io_cap) {
    if (f->h_io) (void)hipHostFree(f->h_io);
    f->h_io = nullptr;
    f->h_io_cap = 0;
    const size_t cap = want + want / 4 + 256;
    LSLAM_HIP(ctx, hipHostMalloc((void**)&f->h_io, cap, hipHostMallocDefault));
    f->h_io_cap = cap;
    f->n_growths++;
  }
  if ((rc = plo_reserve(f, f->d_ranges, S * width)) || (rc = plo_reserve(f, f->d_stamps, S)) || (rc = plo_reserve(f, f->d_rec, S)) ||
      (active && (rc = plo_reserve(f, f->d_active, S))))
    return rc;
  unsigned char* const h_rec = f->h_io;
  double* const h_st = reinterpret_cast<double*>(f->h_io + rec_bytes);
  float* const h_r = reinterpret_cast<float*>(f->h_io + rec_bytes + st_bytes);
  uint8_t* const h_act = f->h_io + rec_bytes + st_bytes + plane;
  memcpy(h_st, stamps, st_bytes);
  LSLAM_HIP(ctx, hipMemcpyAsync(f->d_stamps.p, h_st, st_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n_readings > 0) {
    for (size_t k = 0; k < S; k++)
      memcpy(h_r + k * n_readings, ranges + k * (size_t)ranges_stride, (size_t)n_readings * sizeof(float));
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_ranges.p, h_r, plane, hipMemcpyHostToDevice, ctx->stream));
  }
  if (active) {
    memcpy(h_act, active, S);
    LSLAM_HIP(ctx, hipMemcpyAsync(f->d_active.p, h_act, S, hipMemcpyHostToDevice, ctx->stream));
  }
  launch(ctx, "plicp_odom", k_plicp_odom, dim3((unsigned)f->n_tracks), dim3(kPlThreads), 0,
         pl_params(f->params, f->laser.range_min, f->laser.range_max), f->consts, f->n_tracks, n_steps, n_readings, width,
         (const float*)f->d_ranges.p, (const double*)f->d_stamps.p, (const uint8_t*)(active ? f->d_active.p : nullptr), f->laser.tc(),
         f->laser.ts(), f->d_state.p, f->d_kf.p, f->d_rec.p);
  LSLAM_HIP(ctx, hipGetLastError());
  f->n_launches++;
  f->n_readings = n_readings;
  f->clouds = false;
  LSLAM_HIP(ctx, hipMemcpyAsync(h_rec, f->d_rec.p, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->n_waits++;
  memcpy(out, h_rec, rec_bytes);
  for (size_t k = 0; k < S; k++) f->n_scans += (!active || active[k]) ? 1 : 0;
  return LSLAM_OK;
}

int lslam_plicp_odom_process_many_clouds(lslam_plicp_odom* f, int n_steps, int n_points, const float* xyz, const uint8_t* valid,
                                         const uint8_t* take, const double* stamps, const uint8_t* active,
                                         lslam_plicp_odom_record* out) {
  if (!f || n_steps < 0 || n_points < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  const char* who = "lslam_plicp_odom_process_many_clouds";
  if (!xyz) return f->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "%s: xyz, stamps and out are required", who);
  return plo_clouds(f, who, n_steps, n_points, xyz, valid, take, nullptr, nullptr, nullptr, 1, stamps, active, out);
}

int lslam_plicp_odom_process_many_clouds_dev(lslam_plicp_odom* f, int n_steps, int n_points, const float* const* xyz_dev,
                                             const uint8_t* const* valid_dev, const int32_t* const* take_dev, int take_stride,
                                             const double* stamps, const uint8_t* active, lslam_plicp_odom_record* out) {
  if (!f || n_steps < 0 || n_points < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  return plo_clouds(f, "lslam_plicp_odom_process_many_clouds_dev", n_steps, n_points, nullptr, nullptr, nullptr, xyz_dev, valid_dev,
                    take_dev, take_stride, stamps, active, out);
}

}  // extern "C"
