// lesson5 lidar motion de-skew on the device: LidarUndistortion::CorrectLaserScan with its
// ComputeRotation / ComputePosition helpers (lesson5/src/lidar_undistortion.cc:339-396, 397-447).  Thread per beam:
// time of the beam, IMU rotation interpolated from the integrated gyro samples, odometry translation interpolated over
// the scan, pcl::getTransformation of both (float32 Euler -> affine), the transform of the FIRST valid beam inverted once
// per scan, transBt = transStartInverse * transFinal, point = transBt * (r cos a, r sin a, 1.0) in the reference's mixed
// float/double arithmetic (the z = 1.0 is the reference's).
// The reference's arithmetic goes through PCL (getTransformation) and Eigen (Affine3f inverse and product) inside a ROS node
// class.  This kernel follows the published PCL formula (pcl/common/impl/eigen.hpp) and Eigen 3.3's evaluation orders;
// round 4 pins it against the reference's own source compiled in place behind stand-ins for those libraries
// (tests/test_deskew_pin.py: <= 4e-6 m, the device's float32 cos / sin being the difference).
#include <cmath>

#include "deskew_impl.hpp"  // Aff3, get_transformation, inverse, mul; DeskewScan

using namespace lslam;

namespace {

struct DeskewCfg {
  int n, n_imu_last;  // n_imu_last = current_imu_index_ (index of the last integrated IMU sample)
  float range_min, range_max;
  float angle_min, angle_inc;  // the LaserScan message's float32 fields
  double t0, dt;
  int use_imu, use_odom;
  double odom_t0, odom_t1;
  float odom_dx, odom_dy, odom_dz;
};

__device__ __forceinline__ Aff3 transform_at(const DeskewCfg& c, int i, const double* imu_time, const double* rx,
                                             const double* ry, const double* rz) {
  const double t = c.t0 + i * c.dt;  // :358
  float rotX = 0, rotY = 0, rotZ = 0, posX = 0, posY = 0, posZ = 0;
  if (c.use_imu) {  // ComputeRotation (:397-434): the reference's linear search, whatever the sample times are
    int f = 0;
    while (f < c.n_imu_last) {
      if (t < imu_time[f]) break;
      ++f;
    }
    if (t > imu_time[f] || f == 0) {
      rotX = (float)rx[f]; rotY = (float)ry[f]; rotZ = (float)rz[f];
    } else {
      const int b = f - 1;
      const double rf = (t - imu_time[b]) / (imu_time[f] - imu_time[b]);
      const double rb = (imu_time[f] - t) / (imu_time[f] - imu_time[b]);
      rotX = (float)(rx[f] * rf + rx[b] * rb);
      rotY = (float)(ry[f] * rf + ry[b] * rb);
      rotZ = (float)(rz[f] * rf + rz[b] * rb);
    }
  }
  if (c.use_odom) {  // ComputePosition (:437-447)
    const double rf = (t - c.odom_t0) / (c.odom_t1 - c.odom_t0);
    posX = (float)((double)c.odom_dx * rf);
    posY = (float)((double)c.odom_dy * rf);
    posZ = (float)((double)c.odom_dz * rf);
  }
  return get_transformation(posX, posY, posZ, rotX, rotY, rotZ);
}

// CreateAngleCache (:164-173): the angle is evaluated in FLOAT32 (angle_min + i * angle_increment on the message's float
// fields), then widened for the double cos / sin.  The one statement behind both the per-beam evaluation of the single
// call and the batched call's cached table.
__device__ __forceinline__ double2 beam_cossin(float angle_min, float angle_inc, int i) {
  const float af = angle_min + (float)i * angle_inc;
  const double a = (double)af;
  return make_double2(cos(a), sin(a));
}

constexpr int kDeskewThreads = 256;  // one beam per thread and tile
constexpr int kDeskewLdsImu = 256;   // IMU samples a block stages in LDS (4 doubles each: 8 KiB); more are read from HBM

struct DeskewShared {
  int wave_first[kDeskewThreads / 64];
  Aff3 start_inv;
  double imu[4 * kDeskewLdsImu];
};

// ONE body for lslam_deskew_scan's kernel and the batched kernel: beams [i_begin, i_end) of the scan `c` describes.  Every
// block finds the scan's first valid beam itself (wave ballots from the front of the scan: tile after tile of 256 beams until
// one holds a valid beam), computes transStartInverse once (:377-383) and keeps it in LDS.  TABLE: cos / sin of the beam
// angles come from a table beam_cossin filled, else from beam_cossin here -- the same statement, the same bits.
template <bool TABLE>
__device__ __forceinline__ void deskew_body(const DeskewCfg& c, DeskewShared& sh, const float* __restrict__ ranges,
                                            const double* __restrict__ g_time, const double* __restrict__ g_rx,
                                            const double* __restrict__ g_ry, const double* __restrict__ g_rz,
                                            const double2* __restrict__ table, float* __restrict__ out_xyz,
                                            uint8_t* __restrict__ valid, int i_begin, int i_end) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto is_valid = [&](float r) { return !(!isfinite(r) || r < c.range_min || r > c.range_max); };  // :350-353
  // the scan's integrated IMU samples: into LDS when they fit (every beam walks them from the front)
  const int n_imu = c.use_imu ? c.n_imu_last + 1 : 0;
  const double *imu_time = g_time, *rx = g_rx, *ry = g_ry, *rz = g_rz;
  if (n_imu > 0 && n_imu <= kDeskewLdsImu) {
    for (int j = tid; j < n_imu; j += kDeskewThreads) {
      sh.imu[j] = g_time[j];
      sh.imu[kDeskewLdsImu + j] = g_rx[j];
      sh.imu[2 * kDeskewLdsImu + j] = g_ry[j];
      sh.imu[3 * kDeskewLdsImu + j] = g_rz[j];
    }
    imu_time = sh.imu; rx = sh.imu + kDeskewLdsImu; ry = sh.imu + 2 * kDeskewLdsImu; rz = sh.imu + 3 * kDeskewLdsImu;
  }
  int first = c.n;
  for (int i0 = 0; i0 < c.n; i0 += kDeskewThreads) {  // (block-uniform loop)
    const int i = i0 + tid;
    const bool ok = i < c.n && is_valid(ranges[i]);
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) sh.wave_first[wv] = bal ? i0 + wv * 64 + (__ffsll((long long)bal) - 1) : c.n;
    __syncthreads();  // (also: the staged IMU samples are in place)
    int m = c.n;
    for (int w = 0; w < kDeskewThreads / 64; w++) m = min(m, sh.wave_first[w]);
    __syncthreads();  // wave_first is rewritten by the next tile
    if (m < c.n) {
      first = m;
      break;
    }
  }
  if (first >= c.n) {  // no valid beam in the whole scan: nothing to anchor on, every output is zero
    for (int i = i_begin + tid; i < i_end; i += kDeskewThreads) {
      valid[i] = 0;
      out_xyz[3 * i] = 0.f; out_xyz[3 * i + 1] = 0.f; out_xyz[3 * i + 2] = 0.f;
    }
    return;
  }
  if (tid == 0) sh.start_inv = inverse(transform_at(c, first, imu_time, rx, ry, rz));  // :377-383
  __syncthreads();
  for (int i = i_begin + tid; i < i_end; i += kDeskewThreads) {
    const float r = ranges[i];
    const bool ok = is_valid(r);
    valid[i] = ok ? 1 : 0;
    float x = 0.f, y = 0.f, z = 0.f;
    if (ok) {
      const double2 cs = TABLE ? table[i] : beam_cossin(c.angle_min, c.angle_inc, i);
      const double px = (double)r * cs.x, py = (double)r * cs.y, pz = 1.0;                  // :361-362, :343
      const Aff3 bt = mul(sh.start_inv, transform_at(c, i, imu_time, rx, ry, rz));        // :386-390
      x = (float)((((double)bt.l[0] * px + (double)bt.l[1] * py) + (double)bt.l[2] * pz) + (double)bt.t[0]);  // :394-396
      y = (float)((((double)bt.l[3] * px + (double)bt.l[4] * py) + (double)bt.l[5] * pz) + (double)bt.t[1]);
      z = (float)((((double)bt.l[6] * px + (double)bt.l[7] * py) + (double)bt.l[8] * pz) + (double)bt.t[2]);
    }
    out_xyz[3 * i] = x; out_xyz[3 * i + 1] = y; out_xyz[3 * i + 2] = z;
  }
}

// lslam_deskew_scan: one scan, one block that walks every tile
__global__ void __launch_bounds__(kDeskewThreads)
k_deskew(DeskewCfg c, const float* __restrict__ ranges, const double* __restrict__ imu_time, const double* __restrict__ rx,
         const double* __restrict__ ry, const double* __restrict__ rz, float* __restrict__ out_xyz, uint8_t* __restrict__ valid) {
  __shared__ DeskewShared sh;
  deskew_body<false>(c, sh, ranges, imu_time, rx, ry, rz, nullptr, out_xyz, valid, 0, c.n);
}

struct DeskewGeom {
  int n, ranges_stride;
  float range_min, range_max, angle_min, angle_inc;
};

// lslam_deskew_batch: grid (beam tiles, scans) -- a handful of scans already fills the chip
__global__ void __launch_bounds__(kDeskewThreads)
k_deskew_batch(DeskewGeom g, const DeskewScan* __restrict__ scans, const float* __restrict__ ranges,
               const double* __restrict__ imu, int imu_total, const double2* __restrict__ table, float* __restrict__ out_xyz,
               uint8_t* __restrict__ valid) {
  __shared__ DeskewShared sh;
  const int k = blockIdx.y;
  const DeskewScan s = scans[k];
  DeskewCfg c;
  c.n = g.n; c.n_imu_last = max(s.n_imu, 1) - 1;
  c.range_min = g.range_min; c.range_max = g.range_max;
  c.angle_min = g.angle_min; c.angle_inc = g.angle_inc;
  c.t0 = s.t0; c.dt = s.dt;
  c.use_imu = s.use_imu; c.use_odom = s.use_odom;
  c.odom_t0 = s.odom_t0; c.odom_t1 = s.odom_t1;
  c.odom_dx = s.odom_dx; c.odom_dy = s.odom_dy; c.odom_dz = s.odom_dz;
  const double* it = imu + s.imu_first;
  const int i_begin = blockIdx.x * kDeskewThreads;
  deskew_body<true>(c, sh, ranges + (size_t)k * g.ranges_stride, it, it + imu_total, it + 2 * (size_t)imu_total,
                    it + 3 * (size_t)imu_total, table, out_xyz + (size_t)3 * k * g.n, valid + (size_t)k * g.n, i_begin,
                    min(i_begin + kDeskewThreads, g.n));
}

// the batched call's angle cache: CreateAngleCache on the device, once per scan geometry
__global__ void __launch_bounds__(256)
k_deskew_angles(float angle_min, float angle_inc, int n, double2* __restrict__ table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) table[i] = beam_cossin(angle_min, angle_inc, i);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// lslam_deskew: the batched call's handle.  It owns every buffer a call needs, so a call of a shape it has seen allocates
// nothing: the angle table (per scan geometry), the scan records + IMU samples in HBM and their pinned way up (a small ring,
// because the _dev form returns before the copy has run), and -- host form only -- ranges / xyz / valid in HBM and pinned.
// ------------------------------------------------------------------------------------------
struct lslam_deskew {
  lslam_context* ctx = nullptr;
  DevBuf<double2> d_table;
  int table_n = 0;
  float table_angle_min = 0.f, table_angle_inc = 0.f;
  DevBuf<unsigned char> d_meta;  // [DeskewScan x n_scans][double x 4 x imu_total]
  // pinned way up of the scan records and IMU samples: ONE allocation cut into kSlots equal slots, so that a shape seen once
  // fits every slot
  static constexpr int kSlots = 4;
  unsigned char* h_meta = nullptr;
  size_t slot_cap = 0;  // bytes per slot
  hipEvent_t slot_done[kSlots] = {};
  bool slot_in_flight[kSlots] = {};
  int next_slot = 0;
  // host form
  DevBuf<float> d_ranges, d_xyz;
  DevBuf<uint8_t> d_valid;
  unsigned char* h_io = nullptr;  // pinned: ranges up, then xyz and valid down
  size_t h_io_cap = 0;
  int64_t n_scans = 0, n_launches = 0, n_growths = 0, n_waits = 0;
};

namespace {

template <typename T>
int dsk_reserve(lslam_deskew* d, DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return LSLAM_OK;
  LSLAM_HIP(d->ctx, b.reserve(n));
  d->n_growths++;
  return LSLAM_OK;
}

int dsk_pinned_reserve(lslam_deskew* d, unsigned char** p, size_t* cap, size_t want) {
  if (want <= *cap) return LSLAM_OK;
  if (*p) (void)hipHostFree(*p);  // (the caller has made sure nothing in flight reads it)
  *p = nullptr;
  *cap = 0;
  const size_t n = want + want / 4 + 256;
  LSLAM_HIP(d->ctx, hipHostMalloc((void**)p, n, hipHostMallocDefault));
  *cap = n;
  d->n_growths++;
  return LSLAM_OK;
}

// what both forms check before anything touches the device
int dsk_check(lslam_deskew* d, int n_scans, int n_readings, const void* ranges, int ranges_stride, const lslam_deskew_params* params,
              const int32_t* imu_first, const double* imu_time, const double* rx, const double* ry, const double* rz,
              const void* out_xyz, const void* out_valid) {
  if (!d || n_scans < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_scans == 0) return LSLAM_OK;
  lslam_context* ctx = d->ctx;
  if (!params || !imu_first) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_deskew_batch: params and imu_first are required");
  if (n_readings > 0 && (!ranges || !out_xyz || !out_valid || ranges_stride < n_readings))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_deskew_batch: ranges, out_xyz, out_valid and ranges_stride >= n_readings are required");
  if (n_scans > 65535) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_deskew_batch: at most 65535 scans per call (got %d)", n_scans);
  if (imu_first[0] < 0) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_deskew_batch: imu_first[0] is negative");
  for (int k = 0; k < n_scans; k++) {
    const lslam_deskew_params& p = params[k];
    // (compared as bits would refuse a NaN header against itself; a NaN geometry is refused either way)
    if (!(p.angle_min == params[0].angle_min && p.angle_increment == params[0].angle_increment &&
          p.range_min == params[0].range_min && p.range_max == params[0].range_max))
      return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_deskew_batch: scan %d has another geometry (angle_min, angle_increment, "
                       "range_min, range_max) than scan 0: one call, one geometry", k);
    const int cnt = imu_first[k + 1] - imu_first[k];
    if (cnt < 0) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_deskew_batch: imu_first decreases at scan %d", k);
    if (p.use_imu && cnt < 1) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_deskew_batch: scan %d uses the IMU and owns no sample", k);
  }
  if (imu_first[n_scans] > 0 && (!imu_time || !rx || !ry || !rz))
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_deskew_batch: the IMU arrays are required");
  return LSLAM_OK;
}

// the device part of both forms: records and samples up through a pinned slot, the angle table if the geometry is new, ONE
// launch.  Everything is enqueued on the context's stream; the only wait is for a slot whose copy of kSlots calls ago has
// not run yet.
int dsk_enqueue(lslam_deskew* d, int n_scans, int n_readings, const float* d_ranges, int ranges_stride,
                const lslam_deskew_params* params, const int32_t* imu_first, const double* imu_time, const double* rx,
                const double* ry, const double* rz, float* d_xyz, uint8_t* d_valid) {
  lslam_context* ctx = d->ctx;
  if (n_scans == 0 || n_readings == 0) return LSLAM_OK;
  const int base = imu_first[0];
  const int imu_total = imu_first[n_scans] - base;
  const size_t rec_bytes = (size_t)n_scans * sizeof(DeskewScan);
  const size_t bytes = rec_bytes + (size_t)4 * imu_total * sizeof(double);
  if (bytes > d->slot_cap) {  // every slot grows together: none may be in flight
    for (int q = 0; q < lslam_deskew::kSlots; q++)
      if (d->slot_in_flight[q]) {
        if (hipEventQuery(d->slot_done[q]) != hipSuccess) {
          (void)hipGetLastError();  // hipErrorNotReady is no error
          LSLAM_HIP(ctx, hipEventSynchronize(d->slot_done[q]));
          d->n_waits++;
        }
        d->slot_in_flight[q] = false;
      }
    size_t cap = d->slot_cap * lslam_deskew::kSlots;
    const size_t per = (bytes + bytes / 4 + 255) / 256 * 256;
    int rc = dsk_pinned_reserve(d, &d->h_meta, &cap, per * lslam_deskew::kSlots);
    d->slot_cap = rc ? 0 : per;
    if (rc) return rc;
  }
  const int q = d->next_slot;
  d->next_slot = (d->next_slot + 1) % lslam_deskew::kSlots;
  if (d->slot_in_flight[q] && hipEventQuery(d->slot_done[q]) != hipSuccess) {
    (void)hipGetLastError();  // hipErrorNotReady is no error
    LSLAM_HIP(ctx, hipEventSynchronize(d->slot_done[q]));
    d->n_waits++;
  }
  d->slot_in_flight[q] = false;
  unsigned char* const up_bytes = d->h_meta + (size_t)q * d->slot_cap;
  int rc = dsk_reserve(d, d->d_meta, bytes);
  if (rc) return rc;
  DeskewScan* recs = reinterpret_cast<DeskewScan*>(up_bytes);
  for (int k = 0; k < n_scans; k++) {
    const lslam_deskew_params& p = params[k];
    DeskewScan& s = recs[k];
    s.t0 = p.scan_time_start; s.dt = p.time_increment;
    s.odom_t0 = p.start_odom_time; s.odom_t1 = p.end_odom_time;
    s.odom_dx = p.odom_incre_x; s.odom_dy = p.odom_incre_y; s.odom_dz = p.odom_incre_z;
    s.use_imu = p.use_imu; s.use_odom = p.use_odom;
    s.imu_first = imu_first[k] - base;
    s.n_imu = imu_first[k + 1] - imu_first[k];
    s.pad = 0;
  }
  if (imu_total > 0) {
    double* up = reinterpret_cast<double*>(up_bytes + rec_bytes);
    const double* src[4] = {imu_time, rx, ry, rz};
    for (int a = 0; a < 4; a++) memcpy(up + (size_t)a * imu_total, src[a] + base, (size_t)imu_total * sizeof(double));
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(d->d_meta.p, up_bytes, bytes, hipMemcpyHostToDevice, ctx->stream));
  LSLAM_HIP(ctx, hipEventRecord(d->slot_done[q], ctx->stream));
  d->slot_in_flight[q] = true;
  const lslam_deskew_params& p0 = params[0];
  const float geom[4] = {p0.angle_min, p0.angle_increment, p0.range_min, p0.range_max};
  return deskew_launch_records(d, n_scans, n_readings, d_ranges, ranges_stride, geom, (const DeskewScan*)d->d_meta.p,
                               (const double*)(d->d_meta.p + rec_bytes), imu_total, d_xyz, d_valid);
}

}  // namespace

int lslam::deskew_launch_records(lslam_deskew* d, int n_scans, int n_readings, const float* d_ranges, int ranges_stride,
                                 const float geom[4], const DeskewScan* d_scans, const double* d_imu, int imu_total,
                                 float* d_xyz, uint8_t* d_valid) {
  lslam_context* ctx = d->ctx;
  int rc;
  // CreateAngleCache: once per geometry (a table of more beams serves a shorter scan of the same angles)
  if (n_readings > d->table_n || geom[0] != d->table_angle_min || geom[1] != d->table_angle_inc) {
    rc = dsk_reserve(d, d->d_table, (size_t)n_readings);
    if (rc) return rc;
    launch(ctx, "deskew_angles", k_deskew_angles, dim3((unsigned)((n_readings + 255) / 256)), dim3(256), 0, geom[0], geom[1],
           n_readings, d->d_table.p);
    d->n_launches++;
    d->table_n = n_readings;
    d->table_angle_min = geom[0];
    d->table_angle_inc = geom[1];
  }
  DeskewGeom g;
  g.n = n_readings; g.ranges_stride = ranges_stride;
  g.range_min = geom[2]; g.range_max = geom[3];
  g.angle_min = geom[0]; g.angle_inc = geom[1];
  const dim3 grid((unsigned)((n_readings + kDeskewThreads - 1) / kDeskewThreads), (unsigned)n_scans);
  launch(ctx, "deskew_batch", k_deskew_batch, grid, dim3(kDeskewThreads), 0, g, d_scans, d_ranges, d_imu, imu_total,
         (const double2*)d->d_table.p, d_xyz, d_valid);
  d->n_launches++;
  d->n_scans += n_scans;
  LSLAM_HIP(ctx, hipGetLastError());
  return LSLAM_OK;
}

lslam_context* lslam::deskew_context(lslam_deskew* d) { return d->ctx; }

extern "C" {

int lslam_deskew_scan(lslam_context* ctx, const float* ranges, int n, const lslam_deskew_params* p, const double* imu_time,
                      const double* imu_rot_x, const double* imu_rot_y, const double* imu_rot_z, int n_imu,
                      float* out_xyz, uint8_t* out_valid) {
  if (!ctx || n < 0 || (n > 0 && (!ranges || !out_xyz || !out_valid)) || !p) return LSLAM_ERR_INVALID_ARGUMENT;
  if (p->use_imu && (n_imu < 1 || !imu_time || !imu_rot_x || !imu_rot_y || !imu_rot_z)) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n == 0) return LSLAM_OK;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const int ni = p->use_imu ? n_imu : 1;
  float* d_r = nullptr;
  double* d_imu = nullptr;
  float* d_out = nullptr;
  uint8_t* d_v = nullptr;
  auto cleanup = [&]() {
    if (d_r) (void)hipFree(d_r);
    if (d_imu) (void)hipFree(d_imu);
    if (d_out) (void)hipFree(d_out);
    if (d_v) (void)hipFree(d_v);
  };
  if (hipMalloc((void**)&d_r, (size_t)n * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&d_imu, (size_t)4 * ni * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&d_out, (size_t)3 * n * sizeof(float)) != hipSuccess || hipMalloc((void**)&d_v, (size_t)n) != hipSuccess) {
    cleanup();
    return ctx->fail(LSLAM_ERR_HIP, "lslam_deskew_scan: out of device memory");
  }
  hipError_t e = hipMemcpyAsync(d_r, ranges, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (p->use_imu) {
    const double* src[4] = {imu_time, imu_rot_x, imu_rot_y, imu_rot_z};
    for (int k = 0; k < 4 && e == hipSuccess; k++)
      e = hipMemcpyAsync(d_imu + (size_t)k * ni, src[k], (size_t)ni * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  }
  DeskewCfg c;
  c.n = n; c.n_imu_last = ni - 1;
  c.range_min = p->range_min; c.range_max = p->range_max;
  c.angle_min = p->angle_min; c.angle_inc = p->angle_increment;
  c.t0 = p->scan_time_start; c.dt = p->time_increment;
  c.use_imu = p->use_imu; c.use_odom = p->use_odom;
  c.odom_t0 = p->start_odom_time; c.odom_t1 = p->end_odom_time;
  c.odom_dx = p->odom_incre_x; c.odom_dy = p->odom_incre_y; c.odom_dz = p->odom_incre_z;
  if (e == hipSuccess) {
    launch(ctx, "deskew", k_deskew, dim3(1), dim3(256), 0, c, (const float*)d_r, (const double*)d_imu, (const double*)(d_imu + ni),
           (const double*)(d_imu + 2 * (size_t)ni), (const double*)(d_imu + 3 * (size_t)ni), d_out, d_v);
    e = hipMemcpyAsync(out_xyz, d_out, (size_t)3 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out_valid, d_v, (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  cleanup();
  if (e != hipSuccess) return ctx->fail(LSLAM_ERR_HIP, "lslam_deskew_scan: %s", hipGetErrorString(e));
  return LSLAM_OK;
}

int lslam_deskew_create(lslam_context* ctx, lslam_deskew** out) {
  if (!ctx || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_deskew* d = new lslam_deskew();
  d->ctx = ctx;
  for (auto& e : d->slot_done)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      lslam_deskew_destroy(d);
      return ctx->fail(LSLAM_ERR_HIP, "lslam_deskew_create: cannot create an event");
    }
  *out = d;
  return LSLAM_OK;
}

void lslam_deskew_destroy(lslam_deskew* d) {
  if (!d) return;
  (void)hipSetDevice(d->ctx->device);
  (void)hipStreamSynchronize(d->ctx->stream);
  for (auto e : d->slot_done)
    if (e) (void)hipEventDestroy(e);
  if (d->h_meta) (void)hipHostFree(d->h_meta);
  if (d->h_io) (void)hipHostFree(d->h_io);
  d->d_table.release();
  d->d_meta.release();
  d->d_ranges.release();
  d->d_xyz.release();
  d->d_valid.release();
  delete d;
}

int lslam_deskew_stats(const lslam_deskew* d, int64_t out[4]) {
  if (!d || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = d->n_scans; out[1] = d->n_launches; out[2] = d->n_growths; out[3] = d->n_waits;
  return LSLAM_OK;
}

int lslam_deskew_batch_dev(lslam_deskew* d, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride,
                           const lslam_deskew_params* params, const int32_t* imu_first, const double* imu_time,
                           const double* imu_rot_x, const double* imu_rot_y, const double* imu_rot_z, float* out_xyz_dev,
                           uint8_t* out_valid_dev) {
  int rc = dsk_check(d, n_scans, n_readings, ranges_dev, ranges_stride, params, imu_first, imu_time, imu_rot_x, imu_rot_y,
                     imu_rot_z, out_xyz_dev, out_valid_dev);
  if (rc || n_scans == 0 || n_readings == 0) return rc;
  LSLAM_HIP(d->ctx, hipSetDevice(d->ctx->device));
  return dsk_enqueue(d, n_scans, n_readings, ranges_dev, ranges_stride, params, imu_first, imu_time, imu_rot_x, imu_rot_y,
                     imu_rot_z, out_xyz_dev, out_valid_dev);
}

int lslam_deskew_batch(lslam_deskew* d, int n_scans, int n_readings, const float* ranges, int ranges_stride,
                       const lslam_deskew_params* params, const int32_t* imu_first, const double* imu_time,
                       const double* imu_rot_x, const double* imu_rot_y, const double* imu_rot_z, float* out_xyz,
                       uint8_t* out_valid) {
  int rc = dsk_check(d, n_scans, n_readings, ranges, ranges_stride, params, imu_first, imu_time, imu_rot_x, imu_rot_y, imu_rot_z,
                     out_xyz, out_valid);
  if (rc || n_scans == 0 || n_readings == 0) return rc;
  lslam_context* ctx = d->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t total = (size_t)n_scans * (size_t)n_readings;
  // pinned: [xyz 12 B per beam | valid 1 B per beam]; the ranges go up through the front of the xyz part (every call ends
  // with a wait, so nothing in flight reads this buffer when the next call fills it)
  rc = dsk_pinned_reserve(d, &d->h_io, &d->h_io_cap, total * 13);
  if (rc) return rc;
  if ((rc = dsk_reserve(d, d->d_ranges, total)) || (rc = dsk_reserve(d, d->d_xyz, 3 * total)) || (rc = dsk_reserve(d, d->d_valid, total)))
    return rc;
  float* h_r = reinterpret_cast<float*>(d->h_io);
  for (int k = 0; k < n_scans; k++)
    memcpy(h_r + (size_t)k * n_readings, ranges + (size_t)k * ranges_stride, (size_t)n_readings * sizeof(float));
  LSLAM_HIP(ctx, hipMemcpyAsync(d->d_ranges.p, h_r, total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  rc = dsk_enqueue(d, n_scans, n_readings, d->d_ranges.p, n_readings, params, imu_first, imu_time, imu_rot_x, imu_rot_y, imu_rot_z,
                   d->d_xyz.p, d->d_valid.p);
  if (rc) return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(d->h_io, d->d_xyz.p, total * 12, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(d->h_io + total * 12, d->d_valid.p, total, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  d->n_waits++;
  memcpy(out_xyz, d->h_io, total * 12);
  memcpy(out_valid, d->h_io + total * 12, total);
  return LSLAM_OK;
}

}  // extern "C"
