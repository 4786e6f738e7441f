// What csrc/deskew.hip shares with csrc/motion_sync.hip: the float32 affine arithmetic of the reference's PCL / Eigen calls
// (one statement of it for CorrectLaserScan and for PruneOdomDeque's increment), the per-scan record k_deskew_batch reads, and
// the host entry that launches k_deskew_batch on records that are already in HBM.
#pragma once

#include "common.hpp"

struct lslam_deskew;

namespace lslam {

struct Aff3 {  // Eigen::Affine3f: linear (row-major here) + translation
  float l[9], t[3];
};

// pcl::getTransformation(x, y, z, roll, pitch, yaw) for float
__device__ __forceinline__ Aff3 get_transformation(float x, float y, float z, float roll, float pitch, float yaw) {
  const float A = cosf(yaw), B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll), F = sinf(roll);
  const float DE = D * E, DF = D * F;
  Aff3 t;
  t.l[0] = A * C;  t.l[1] = A * DF - B * E;  t.l[2] = B * F + A * DE;  t.t[0] = x;
  t.l[3] = B * C;  t.l[4] = A * E + B * DF;  t.l[5] = B * DE - A * F;  t.t[1] = y;
  t.l[6] = -D;     t.l[7] = C * F;           t.l[8] = C * E;           t.t[2] = z;
  return t;
}
__device__ __forceinline__ float cof3(const float* m, int i, int j) {  // Eigen cofactor_3x3<i,j>
  const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
}
// Transform::inverse(Affine): linear by the cofactor inverse (LU/InverseImpl.h), translation = (-Linv) * t
__device__ __forceinline__ Aff3 inverse(const Aff3& a) {
  const float* m = a.l;
  const float c0 = cof3(m, 0, 0), c1 = cof3(m, 1, 0), c2 = cof3(m, 2, 0);
  const float det = c0 * m[0] + (c1 * m[3] + c2 * m[6]);
  const float invdet = 1.0f / det;
  Aff3 r;
  r.l[0] = c0 * invdet; r.l[1] = c1 * invdet; r.l[2] = c2 * invdet;
  r.l[3] = cof3(m, 0, 1) * invdet; r.l[4] = cof3(m, 1, 1) * invdet; r.l[5] = cof3(m, 2, 1) * invdet;
  r.l[6] = cof3(m, 0, 2) * invdet; r.l[7] = cof3(m, 1, 2) * invdet; r.l[8] = cof3(m, 2, 2) * invdet;
  for (int i = 0; i < 3; i++)
    r.t[i] = (-r.l[3 * i]) * a.t[0] + ((-r.l[3 * i + 1]) * a.t[1] + (-r.l[3 * i + 2]) * a.t[2]);
  return r;
}
// Affine * Affine (Geometry/Transform.h): linear = L1 L2, translation = L1 t2 + t1; 3-term sums a0 + (a1 + a2)
__device__ __forceinline__ Aff3 mul(const Aff3& a, const Aff3& b) {
  Aff3 r;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++)
      r.l[3 * i + j] = a.l[3 * i] * b.l[j] + (a.l[3 * i + 1] * b.l[3 + j] + a.l[3 * i + 2] * b.l[6 + j]);
    r.t[i] = (a.l[3 * i] * b.t[0] + (a.l[3 * i + 1] * b.t[1] + a.l[3 * i + 2] * b.t[2])) + a.t[i];
  }
  return r;
}

// what differs from scan to scan of a batch (the geometry -- angles, range window, beam count -- is the call's)
struct DeskewScan {
  double t0, dt, odom_t0, odom_t1;
  float odom_dx, odom_dy, odom_dz;
  int use_imu, use_odom;
  int imu_first, n_imu;  // its samples inside the call's concatenated IMU arrays
  int pad;
};
static_assert(sizeof(DeskewScan) % 8 == 0, "the IMU doubles follow the scan records in one buffer");

// The tail of lslam_deskew_batch_dev for records and samples that are in HBM already: the angle table if the geometry
// {angle_min, angle_increment, range_min, range_max} is new, then ONE launch of k_deskew_batch, on the handle's context
// stream.  imu: four planes (time, rot x, y, z) of imu_total doubles each.  Checks nothing; counts launches and scans.
int deskew_launch_records(lslam_deskew* d, int n_scans, int n_readings, const float* d_ranges, int ranges_stride,
                          const float geom[4], const DeskewScan* d_scans, const double* d_imu, int imu_total, float* d_xyz,
                          uint8_t* d_valid);
lslam_context* deskew_context(lslam_deskew* d);

// csrc/motion_sync.hip for the streamed Hector processor (lslam_hector_process_many_synced), which must refuse a call before
// it enqueues anything: the handle's context, and exactly the checks of lslam_msync_scans_dev on the host arguments (the
// device pointers are the caller's own buffers).  Touches no state and no device.
lslam_context* msync_context(const lslam_msync* h);
int msync_check_scans(lslam_msync* h, lslam_deskew* deskew, const lslam_msync_laser* laser, int n_msgs, int n_readings,
                      const double* stamps, const float* time_increments, const int64_t* imu_seen, const int64_t* odom_seen);
// the caller has waited for the context's stream: the pinned staging area is free again and the state copy has landed
void msync_stream_drained(lslam_msync* h);

// csrc/motion_sync.hip for the Hector fleet (lslam_hector_fleet_process_many_synced): the callbacks of R lslam_msync handles
// in ONE walk, ONE windows, ONE k_deskew_batch and ONE blank launch.  The fleet owns the call's buffers, contiguous over the
// members (member m's c_m callbacks are rows row0_m .. row0_m + c_m - 1 of every one of them); a handle keeps what outlives
// a call.  Per-scan host arrays are indexed i = step * R + member; member m's callbacks are its steps with active[i] != 0.
struct MsyncFleet;
MsyncFleet* msync_fleet_create(lslam_context* ctx);
void msync_fleet_destroy(MsyncFleet* mf);
// Everything that can refuse the call (per member exactly what msync_check_scans refuses; the summed window room; the row
// count), and the call's layout.  Touches no handle and no device.  The handles are non-null, distinct and of mf's context.
int msync_fleet_plan(MsyncFleet* mf, lslam_msync* const* syncs, int R, lslam_deskew* deskew, const lslam_msync_laser* laser,
                     int n_steps, int n_readings, const double* stamps, const float* time_increments, const int64_t* imu_seen,
                     const int64_t* odom_seen, const uint8_t* active);
// The planned call on the context's stream, no wait.  -> the clouds, valid flags and records of all rows, and row_of[i] (the
// row of entry i, -1 where it is not active; valid until the next plan)
int msync_fleet_enqueue(MsyncFleet* mf, lslam_deskew* deskew, const lslam_msync_laser* laser, const float* ranges, int ranges_stride,
                        const float** d_xyz, const uint8_t** d_valid, const lslam_msync_record** d_records, const int** row_of);
int msync_fleet_download(MsyncFleet* mf);  // the records and the R states down, behind everything enqueued (no wait)
// the caller has waited for the stream: every member handle learns its state; records[i] (may be null) are handed out
void msync_fleet_finish(MsyncFleet* mf, lslam_msync_record* records);
void msync_fleet_stats(const MsyncFleet* mf, int64_t out[4]);  // {calls, kernel launches, buffer growths, host waits}

}  // namespace lslam
