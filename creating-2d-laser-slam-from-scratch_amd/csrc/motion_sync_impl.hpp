// What csrc/motion_sync.hip shares with csrc/motion_sync_fleet.hip: the node's state and queues as the kernels see them, and
// the device bodies of the walk and the windows kernel -- ONE copy of every statement group: k_msync_* (one node, arguments
// from the launch) and k_msync_fleet_* (R nodes, arguments from the fleet's member table) call the same bodies.
#pragma once

#include <cmath>

#include "deskew_impl.hpp"

namespace lslam {

constexpr int kQueueLength = LSLAM_MSYNC_QUEUE_LENGTH;

// the node's members that outlive a callback (all message indices are GLOBAL: counted since create / reset)
struct MsyncState {
  long long imu_front, odom_front;  // imu_queue_.front() / odom_queue_.front()
  long long start_odom, end_odom;   // start_odom_msg_ / end_odom_msg_; -1: default-constructed (stamp 0, identity)
  double queued_stamp;              // laser_queue_'s one waiting scan (its ranges are row 0 of the handle's rows)
  float queued_tinc;
  int has_queued;
  long long n_corrected, n_refused;
};

// what the walk leaves for the windows kernel, per callback
struct MsyncWalk {
  long long imu_lo, imu_stop, imu_lead;  // the IMU loop of :207-243 runs over [imu_lo, imu_stop); imu_lead: sample 0 or -1
};

struct MsyncQueues {
  const double* imu;   // planes stamp, wx, wy, wz of imu_cap doubles; entry of message g at g - imu_base
  const double* odom;  // planes stamp, x, y, z, qx, qy, qz, qw of odom_cap doubles
  long long imu_base, odom_base;
  size_t imu_cap, odom_cap;
};

// Pop literally (:191-197, :266-272): advance while stamp[front] < lim, no lower bound.  Wave-uniform.
__device__ __forceinline__ long long pop_front(const double* stamp, long long base, long long front, long long seen, double lim,
                                               int lane) {
  while (front < seen) {
    const long long i = front + lane;
    const bool stop = i < seen && !(stamp[i - base] < lim);
    const unsigned long long b = __ballot(stop);
    if (b) return front + (__ffsll((long long)b) - 1);
    front = min(front + 64, seen);
  }
  return front;
}

// The bodies of the walk and the windows kernel, one copy each: k_msync_* take one node's arguments from the launch,
// k_msync_fleet_* find their node in the grid and take them from the fleet's member table.
__device__ __forceinline__ void msync_walk_body(MsyncState* __restrict__ state, const MsyncQueues& q, int use_imu, int use_odom,
                                                int scan_count, int n_msgs, const double* __restrict__ stamps,
                                                const float* __restrict__ tincs, const long long* __restrict__ imu_seen,
                                                const long long* __restrict__ odom_seen, lslam_msync_record* __restrict__ recs,
                                                MsyncWalk* __restrict__ walks) {
  const int lane = threadIdx.x;
  MsyncState st = *state;  // (every lane holds the same copy)
  const double* it = q.imu;
  const double* ot = q.odom;
  for (int k = 0; k < n_msgs; k++) {
    lslam_msync_record r;
    r.status = LSLAM_MSYNC_QUEUED; r.n_imu = 0;
    r.scan_time_start = 0.0; r.time_increment = 0.0;
    r.start_odom_time = 0.0; r.end_odom_time = 0.0;
    r.odom_incre[0] = r.odom_incre[1] = r.odom_incre[2] = 0.f; r.pad = 0.f;
    MsyncWalk w;
    w.imu_lo = w.imu_stop = 0; w.imu_lead = -1;
    const double new_stamp = stamps[k];
    const float new_tinc = tincs[k];
    if (st.has_queued) {  // CacheLaserScan (:142-156): the scan queued by the previous callback is the current one
      const double start = st.queued_stamp;
      const double tinc = (double)st.queued_tinc;
      const double end = start + tinc * (double)(scan_count - 1);
      r.scan_time_start = start; r.time_increment = tinc;
      int status = LSLAM_MSYNC_CORRECTED;
      if (use_imu) {  // PruneImuDeque
        const long long seen = imu_seen[k];
        long long f = st.imu_front;
        if (f >= seen || it[f - q.imu_base] > start || it[seen - 1 - q.imu_base] < end) {  // :182-188
          status = LSLAM_MSYNC_WAIT_IMU;
        } else {
          f = pop_front(it, q.imu_base, f, seen, start - 0.1, lane);
          st.imu_front = f;
          if (f >= seen) {  // :199-200
            status = LSLAM_MSYNC_WAIT_IMU;
          } else {  // where the loop of :207-243 stops, its sample 0, and how many samples it keeps
            long long lead = -1, first_in = -1, stop = seen;
            int kept_in = 0;
            for (long long c = f; c < seen; c += 64) {
              const long long i = c + lane;
              const bool have = i < seen;
              const double t = have ? it[i - q.imu_base] : 0.0;
              const bool pre = have && t < start;            // :212
              const bool late = have && !pre && t > end;     // :227
              const unsigned long long bl = __ballot(late);
              const unsigned long long before = bl ? ((1ull << (__ffsll((long long)bl) - 1)) - 1ull) : ~0ull;
              const unsigned long long bp = __ballot(pre) & before;
              const unsigned long long bi = __ballot(have && !pre && !late) & before;
              if (lead < 0 && bp) lead = c + (__ffsll((long long)bp) - 1);
              if (first_in < 0 && bi) first_in = c + (__ffsll((long long)bi) - 1);
              kept_in = min(kept_in + __popcll(bi), kQueueLength + 1);
              if (bl) {
                stop = c + (__ffsll((long long)bl) - 1);
                break;
              }
            }
            w.imu_lo = f; w.imu_stop = stop; w.imu_lead = lead;
            const int kept = kept_in + (lead >= 0 ? 1 : 0);
            r.n_imu = kept;
            if (kept_in > 0 && (lead < 0 || first_in < lead)) status = LSLAM_MSYNC_IMU_NO_LEAD_SAMPLE;
            else if (kept > kQueueLength) status = LSLAM_MSYNC_IMU_OVERFLOW;
            if (status != LSLAM_MSYNC_CORRECTED) r.n_imu = 0;
          }
        }
      }
      if (use_odom && status == LSLAM_MSYNC_CORRECTED) {  // PruneOdomDeque
        const long long seen = odom_seen[k];
        long long f = st.odom_front;
        if (f >= seen || ot[f - q.odom_base] > start || ot[seen - 1 - q.odom_base] < end) {  // :257-263
          status = LSLAM_MSYNC_WAIT_ODOM;
        } else {
          f = pop_front(ot, q.odom_base, f, seen, start - 0.1, lane);
          st.odom_front = f;
          if (f >= seen) {  // :274-275
            status = LSLAM_MSYNC_WAIT_ODOM;
          } else {  // :280-296: the last message before the start, the last one up to the end; what finds none stays
            for (long long c = f; c < seen; c += 64) {
              const long long i = c + lane;
              const bool have = i < seen;
              const double t = have ? ot[i - q.odom_base] : 0.0;
              const bool pre = have && t < start;               // :284
              const bool late = have && !pre && !(t <= end);    // :290-295
              const unsigned long long bl = __ballot(late);
              const unsigned long long before = bl ? ((1ull << (__ffsll((long long)bl) - 1)) - 1ull) : ~0ull;
              const unsigned long long bp = __ballot(pre) & before;
              const unsigned long long bi = __ballot(have && !pre && !late) & before;
              if (bp) st.start_odom = c + (63 - __clzll((long long)bp));
              if (bi) st.end_odom = c + (63 - __clzll((long long)bi));
              if (bl) break;
            }
            r.start_odom_time = st.start_odom >= 0 ? ot[st.start_odom - q.odom_base] : 0.0;  // :301-302
            r.end_odom_time = st.end_odom >= 0 ? ot[st.end_odom - q.odom_base] : 0.0;
          }
        }
      }
      if (status != LSLAM_MSYNC_CORRECTED) r.n_imu = 0;
      r.status = status;
      if (status == LSLAM_MSYNC_CORRECTED) st.n_corrected++;
      else st.n_refused++;
    }
    st.has_queued = 1;
    st.queued_stamp = new_stamp;
    st.queued_tinc = new_tinc;
    r.imu_front = st.imu_front; r.odom_front = st.odom_front;
    r.start_odom_index = st.start_odom; r.end_odom_index = st.end_odom;
    if (lane == 0) {
      recs[k] = r;
      walks[k] = w;
    }
  }
  if (lane == 0) *state = st;
}

// tf::Matrix3x3(q).getRPY (setRotation + getEulerYPR, solution 1; LinearMath/Matrix3x3.h), double
__device__ __forceinline__ void quat_rpy(double x, double y, double z, double w, double& roll, double& pitch, double& yaw) {
  const double d = x * x + y * y + z * z + w * w;
  const double s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wx = w * xs, wy = w * ys, wz = w * zs;
  const double xx = x * xs, xy = x * ys, xz = x * zs;
  const double yy = y * ys, yz = y * zs, zz = z * zs;
  const double m00 = 1.0 - (yy + zz), m10 = xy + wz, m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
  if (fabs(m20) >= 1.0) {
    yaw = 0.0;
    roll = atan2(m21, m22);
    pitch = m20 < 0 ? M_PI / 2.0 : -M_PI / 2.0;
  } else {
    pitch = -asin(m20);
    roll = atan2(m21 / cos(pitch), m22 / cos(pitch));
    yaw = atan2(m10 / cos(pitch), m00 / cos(pitch));
  }
}

// pcl::getTransformation of an odometry message's pose (:307-325); g < 0: the default-constructed message
__device__ __forceinline__ Aff3 odom_transform(const MsyncQueues& q, long long g) {
  double p[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  if (g >= 0)
    for (int a = 0; a < 7; a++) p[a] = q.odom[(size_t)(a + 1) * q.odom_cap + (size_t)(g - q.odom_base)];
  double roll, pitch, yaw;
  quat_rpy(p[3], p[4], p[5], p[6], roll, pitch, yaw);
  return get_transformation((float)p[0], (float)p[1], (float)p[2], (float)roll, (float)pitch, (float)yaw);
}

__device__ __forceinline__ void msync_windows_body(const MsyncQueues& q, int use_imu, int use_odom, int k, lslam_msync_record* recs,
                                                   const MsyncWalk* __restrict__ walks, const int* __restrict__ win_first,
                                                   DeskewScan* __restrict__ scans, double* win, int win_plane) {
  const int lane = threadIdx.x;
  const lslam_msync_record r = recs[k];
  const MsyncWalk w = walks[k];
  const int first = win_first[k];
  double* T = win + first;
  DeskewScan s;
  s.t0 = r.scan_time_start; s.dt = r.time_increment;
  s.odom_t0 = 0.0; s.odom_t1 = 0.0;
  s.odom_dx = s.odom_dy = s.odom_dz = 0.f;
  s.use_imu = 0; s.use_odom = 0;
  s.imu_first = first; s.n_imu = 0; s.pad = 0;
  if (r.status != LSLAM_MSYNC_CORRECTED) {  // k_deskew_batch still runs on this row: a record that reads nothing
    if (lane == 0) scans[k] = s;
    return;
  }
  if (use_imu) {
    const double start = r.scan_time_start;
    int pos = 0;
    if (w.imu_lead >= 0) {  // :215-222: the first sample before the start is sample 0, rotation 0
      if (lane == 0) T[0] = q.imu[w.imu_lead - q.imu_base];
      if (lane < 3) T[(size_t)(lane + 1) * win_plane] = 0.0;
      pos = 1;
    }
    for (long long c = w.imu_lo; c < w.imu_stop; c += 64) {  // the kept samples, compacted in order (the rot planes hold
      const long long i = c + lane;                          // the angular velocities until they are integrated below)
      double t = 0.0;
      bool keep = false;
      if (i < w.imu_stop) {
        t = q.imu[i - q.imu_base];
        keep = !(t < start);  // later samples before the start are skipped (:223)
      }
      const unsigned long long b = __ballot(keep);
      if (keep) {
        const int at = pos + __popcll(b & ((1ull << lane) - 1ull));
        T[at] = t;
        for (int a = 1; a < 4; a++) T[(size_t)a * win_plane + at] = q.imu[(size_t)a * q.imu_cap + (size_t)(i - q.imu_base)];
      }
      pos += __popcll(b);
    }
    if (pos == 0) {  // no sample in reach: current_imu_index_ = -1, ComputeRotation reads the reset arrays' entry 0
      if (lane < 4) T[(size_t)lane * win_plane] = 0.0;
    }
    __syncthreads();  // (one wave: the samples the other lanes wrote are visible)
    if (lane < 3 && pos > 1) {  // :237-241, one lane per axis
      double* R = T + (size_t)(lane + 1) * win_plane;
      double rot = 0.0, t_prev = T[0];
      for (int i = 1; i < pos; i++) {
        const double t = T[i];
        const double time_diff = t - t_prev;
        rot = rot + R[i] * time_diff;
        R[i] = rot;
        t_prev = t;
      }
    }
    s.use_imu = 1;
    s.n_imu = max(pos, 1);
  }
  if (use_odom && lane == 0) {  // :304-334
    const Aff3 begin = odom_transform(q, r.start_odom_index);
    const Aff3 end = odom_transform(q, r.end_odom_index);
    const Aff3 bt = mul(inverse(begin), end);
    s.use_odom = 1;
    s.odom_t0 = r.start_odom_time; s.odom_t1 = r.end_odom_time;
    s.odom_dx = bt.t[0]; s.odom_dy = bt.t[1]; s.odom_dz = bt.t[2];
    recs[k].odom_incre[0] = bt.t[0]; recs[k].odom_incre[1] = bt.t[1]; recs[k].odom_incre[2] = bt.t[2];
  }
  if (lane == 0) scans[k] = s;
}

// beam i of row k of the output of a queued or refused callback: zero and not valid (k_deskew_batch cannot skip a scan)
__device__ __forceinline__ void msync_blank_body(const lslam_msync_record* __restrict__ recs, int n, int k, int i,
                                                 float* __restrict__ out_xyz, uint8_t* __restrict__ valid) {
  if (recs[k].status == LSLAM_MSYNC_CORRECTED) return;
  if (i >= n) return;
  float* o = out_xyz + ((size_t)k * n + i) * 3;
  o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
  valid[(size_t)k * n + i] = 0;
}

// ---- the fleet's kernels (csrc/motion_sync_fleet.hip).  A member's entry of the table says where its node lives (the handle's
// own state block, queues and queued scan row) and which rows of the call's buffers -- contiguous over the members -- are its
// callbacks'.
struct MsyncMember {
  MsyncState* state;   // the handle's
  float* queued_row;   // the handle's one queued scan (row 0 of its rows)
  MsyncQueues q;
  int use_imu, use_odom;
  int n_cb;            // its callbacks in this call; 0: it sits the call out and nothing of it is read or written
  int row0;            // its first row in the meta, work, ranges, cloud, valid and record buffers
};
static_assert(sizeof(MsyncMember) % 8 == 0, "the call's double arrays follow the member table in one buffer");

// the three launches, on the context's stream (grids: (n / 256, R); R waves; (max_cb, R) waves)
void msync_fleet_launch_rows(lslam_context* ctx, const MsyncMember* mem, int R, int n, float* rows, const float* tail);
void msync_fleet_launch_walk(lslam_context* ctx, const MsyncMember* mem, int R, int scan_count, const double* stamps, const float* tincs,
                             const long long* imu_seen, const long long* odom_seen, lslam_msync_record* recs, MsyncWalk* walks,
                             MsyncState* states_out);
void msync_fleet_launch_windows(lslam_context* ctx, const MsyncMember* mem, int R, int max_cb, lslam_msync_record* recs,
                                const MsyncWalk* walks, const int* win_first, DeskewScan* scans, double* win, int win_plane);

}  // namespace lslam
