// lesson5's IMU / odometry synchronisation on the device: the FRONT half of LidarUndistortion::ScanCallback
// (lesson5/src/lidar_undistortion.cc:96-125) -- ImuCallback / OdomCallback (the two message queues, :82-93), CacheLaserScan's
// one-scan lag (:127-159), PruneImuDeque (:177-249) and PruneOdomDeque (:252-336) -- chained into csrc/deskew.hip's
// k_deskew_batch, which is the back half (CorrectLaserScan).  Raw messages in, de-skewed clouds out.
//
//   k_msync_walk     ONE wave takes the call's scan callbacks in order: the queue fronts and the sticky start / end odometry
//                    messages are a true dependency from callback to callback.  Every lane takes one queue entry, 64 at a
//                    time; a ballot and its first set bit give where a pop or a window stops.
//   k_msync_windows  one wave per callback, in parallel: compacts the kept IMU samples, integrates them (one lane per axis,
//                    double, the reference's order; the build passes -ffp-contract=off), computes the odometry increment, and
//                    writes the DeskewScan record and the IMU planes exactly as k_deskew_batch reads them.
//   k_msync_blank    zeroes the output rows of queued and refused callbacks (k_deskew_batch cannot skip a scan).
//
// Defined where the reference is not: a sample inside the scan with no sample before the scan's start makes :237 read
// imu_time_[-1] (IMU_NO_LEAD_SAMPLE, refused); more than queueLength = 2000 integrated samples run past imu_time_'s end
// (IMU_OVERFLOW, refused).  Both are refusals of the IMU step: the odometry step does not run, the IMU pops stay made.
#include <cmath>

#include "deskew_impl.hpp"

using namespace lslam;

namespace {

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

__global__ void __launch_bounds__(64)
k_msync_walk(MsyncState* __restrict__ state, MsyncQueues q, int use_imu, int use_odom, int scan_count, int n_msgs,
             const double* __restrict__ stamps, const float* __restrict__ tincs, const long long* __restrict__ imu_seen,
             const long long* __restrict__ odom_seen, lslam_msync_record* __restrict__ recs, MsyncWalk* __restrict__ walks) {
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

__global__ void __launch_bounds__(64)
k_msync_windows(MsyncQueues q, int use_imu, int use_odom, lslam_msync_record* recs, const MsyncWalk* __restrict__ walks,
                const int* __restrict__ win_first, DeskewScan* __restrict__ scans, double* win, int win_plane) {
  const int k = blockIdx.x, lane = threadIdx.x;
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

__global__ void __launch_bounds__(256)
k_msync_blank(const lslam_msync_record* __restrict__ recs, int n, float* __restrict__ out_xyz, uint8_t* __restrict__ valid) {
  const int k = blockIdx.y;
  if (recs[k].status == LSLAM_MSYNC_CORRECTED) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* o = out_xyz + ((size_t)k * n + i) * 3;
  o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
  valid[(size_t)k * n + i] = 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// lslam_msync: the node's state in HBM and every buffer a call needs.
// ------------------------------------------------------------------------------------------
struct lslam_msync {
  lslam_context* ctx = nullptr;
  int use_imu = 1, use_odom = 1;
  // A message queue: `planes` planes of cap doubles, message g at g - base.  Two buffers: when the live one is full, what
  // is still needed moves into the other (which grows if it must), and the popped messages are gone.
  struct Queue {
    int planes = 0;
    DevBuf<double> buf[2];
    int live = 0;
    size_t cap = 0;
    long long base = 0, count = 0;  // global index of entry 0; messages pushed since create / reset
    long long seen = 0;             // the last *_seen a call was given
  };
  Queue imu, odom;
  DevBuf<MsyncState> d_state;
  MsyncState* h_state = nullptr;  // pinned: the state after the last call, copied down behind it
  hipEvent_t state_done = nullptr;
  bool state_in_flight = false;
  MsyncState known = {};  // the newest state the host has seen (what may be discarded is measured against it)
  int scan_count = -1;    // scan_count_: the first scan's n_readings
  DevBuf<float> d_rows;   // (n_msgs + 1) rows of scan_count floats: row 0 the queued scan, row 1 + k message k
  DevBuf<unsigned char> d_meta, d_work;
  DevBuf<double> d_win;
  // pinned staging for everything that goes up: a bump area, rewound once the stream has passed it
  unsigned char* h_stage = nullptr;
  size_t stage_cap = 0, stage_used = 0;
  // host form
  DevBuf<float> d_xyz;
  DevBuf<uint8_t> d_valid;
  unsigned char* h_io = nullptr;
  size_t h_io_cap = 0;
  // the last call, for read_windows
  int last_n = 0, last_win_plane = 0;
  std::vector<int> last_win_first;
  int64_t n_callbacks = 0, n_launches = 0, n_growths = 0, n_waits = 0;
};

namespace {

template <typename T>
int ms_reserve(lslam_msync* h, DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return LSLAM_OK;
  LSLAM_HIP(h->ctx, b.reserve(n));
  h->n_growths++;
  return LSLAM_OK;
}

// `bytes` of pinned staging that stay untouched until the stream has passed what is enqueued next
int ms_stage(lslam_msync* h, size_t bytes, unsigned char** out) {
  lslam_context* ctx = h->ctx;
  bytes = (bytes + 63) / 64 * 64;
  if (h->stage_used + bytes > h->stage_cap) {
    if (h->stage_used > 0) {  // copies out of the area may be in flight
      LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
      h->n_waits++;
      h->stage_used = 0;
    }
    if (bytes > h->stage_cap) {
      if (h->h_stage) (void)hipHostFree(h->h_stage);
      h->h_stage = nullptr;
      h->stage_cap = 0;
      const size_t want = std::max<size_t>(2 * bytes, (size_t)1 << 20);
      LSLAM_HIP(ctx, hipHostMalloc((void**)&h->h_stage, want, hipHostMallocDefault));
      h->stage_cap = want;
      h->n_growths++;
    }
  }
  *out = h->h_stage + h->stage_used;
  h->stage_used += bytes;
  return LSLAM_OK;
}

// the newest state a finished call left, if its copy has arrived (never waits)
void ms_poll_state(lslam_msync* h) {
  if (!h->state_in_flight) return;
  if (hipEventQuery(h->state_done) != hipSuccess) {
    (void)hipGetLastError();  // hipErrorNotReady is no error
    return;
  }
  h->known = *h->h_state;
  h->state_in_flight = false;
}

// room for n more messages; `keep`: the oldest global index a later call can still read
int ms_queue_room(lslam_msync* h, lslam_msync::Queue& q, int n, long long keep) {
  lslam_context* ctx = h->ctx;
  const size_t used = (size_t)(q.count - q.base);
  if (used + (size_t)n <= q.cap) return LSLAM_OK;
  keep = std::max(q.base, std::min(keep, q.count));
  const size_t live = (size_t)(q.count - keep);
  const size_t want = live + (size_t)n;
  DevBuf<double>& from = q.buf[q.live];
  DevBuf<double>& to = q.buf[q.live ^ 1];
  size_t cap = to.cap / q.planes;
  if (want > cap) {
    cap = std::max<size_t>(want + want / 2, 1024);
    int rc = ms_reserve(h, to, cap * q.planes);
    if (rc) return rc;
    cap = to.cap / q.planes;
  }
  if (live > 0)
    LSLAM_HIP(ctx, hipMemcpy2DAsync(to.p, cap * sizeof(double), from.p + (size_t)(keep - q.base), q.cap * sizeof(double),
                                    live * sizeof(double), (size_t)q.planes, hipMemcpyDeviceToDevice, ctx->stream));
  q.live ^= 1;
  q.cap = cap;
  q.base = keep;
  return LSLAM_OK;
}

// n messages of `planes` values each (src[a]: plane a's host array, stride[a] doubles apart) behind the queue's last one
int ms_push(lslam_msync* h, lslam_msync::Queue& q, int n, const double* const* src, const int* stride, long long keep) {
  lslam_context* ctx = h->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ms_queue_room(h, q, n, keep);
  if (rc) return rc;
  unsigned char* up = nullptr;
  if ((rc = ms_stage(h, (size_t)n * q.planes * sizeof(double), &up))) return rc;
  double* u = reinterpret_cast<double*>(up);
  for (int a = 0; a < q.planes; a++)
    for (int j = 0; j < n; j++) u[(size_t)a * n + j] = src[a][(size_t)j * stride[a]];
  LSLAM_HIP(ctx, hipMemcpy2DAsync(q.buf[q.live].p + (size_t)(q.count - q.base), q.cap * sizeof(double), u, (size_t)n * sizeof(double),
                                  (size_t)n * sizeof(double), (size_t)q.planes, hipMemcpyHostToDevice, ctx->stream));
  q.count += n;
  return LSLAM_OK;
}

int ms_check(lslam_msync* h, lslam_deskew* deskew, const lslam_msync_laser* laser, int n_msgs, int n_readings, const void* ranges,
             int ranges_stride, const double* stamps, const float* tincs, const int64_t* imu_seen, const int64_t* odom_seen,
             const void* out_xyz, const void* out_valid) {
  if (!h || !deskew || n_msgs < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = h->ctx;
  if (deskew_context(deskew) != ctx) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_msync_scans: the deskew handle belongs to another context");
  if (n_msgs == 0) return LSLAM_OK;
  if (!laser || !stamps || !tincs) return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_msync_scans: laser, stamps and time_increments are required");
  if (n_readings < 1 || !ranges || !out_xyz || !out_valid || ranges_stride < n_readings)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_msync_scans: n_readings >= 1, ranges, out_xyz, out_valid and ranges_stride >= n_readings are required");
  if (n_msgs > 65535) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_msync_scans: at most 65535 scan callbacks per call (got %d)", n_msgs);
  if (h->scan_count >= 0 && n_readings != h->scan_count)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_msync_scans: %d readings, but the first scan had %d (scan_count_ and the angle cache are the first scan's)",
                     n_readings, h->scan_count);
  const int64_t* seen[2] = {imu_seen, odom_seen};
  const lslam_msync::Queue* qs[2] = {&h->imu, &h->odom};
  for (int a = 0; a < 2; a++) {
    if (!seen[a]) continue;
    long long prev = qs[a]->seen;
    for (int k = 0; k < n_msgs; k++) {
      if (seen[a][k] < prev || seen[a][k] > qs[a]->count)
        return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_msync_scans: %s_seen[%d] = %lld decreases or exceeds the %lld messages pushed",
                         a ? "odom" : "imu", k, (long long)seen[a][k], qs[a]->count);
      prev = seen[a][k];
    }
  }
  return LSLAM_OK;
}

// Everything of a call that runs on the device.  d_rows' rows 1.. hold the call's ranges already.
int ms_enqueue(lslam_msync* h, lslam_deskew* deskew, const lslam_msync_laser* laser, int n_msgs, int n, const double* stamps,
               const float* tincs, const int64_t* imu_seen, const int64_t* odom_seen, float* d_xyz, uint8_t* d_valid,
               lslam_msync_record* d_records_out) {
  lslam_context* ctx = h->ctx;
  ms_poll_state(h);
  // the call's small inputs, one copy: [stamps | imu_seen | odom_seen | win_first (int) | tincs (float)]
  const size_t o_stamps = 0, o_iseen = o_stamps + (size_t)n_msgs * 8, o_oseen = o_iseen + (size_t)n_msgs * 8,
               o_first = o_oseen + (size_t)n_msgs * 8, o_tinc = o_first + (size_t)n_msgs * 4, meta_bytes = o_tinc + (size_t)n_msgs * 4;
  unsigned char* up = nullptr;
  int rc = ms_stage(h, meta_bytes, &up);
  if (rc) return rc;
  memcpy(up + o_stamps, stamps, (size_t)n_msgs * 8);
  long long* u_iseen = reinterpret_cast<long long*>(up + o_iseen);
  long long* u_oseen = reinterpret_cast<long long*>(up + o_oseen);
  int* u_first = reinterpret_cast<int*>(up + o_first);
  memcpy(up + o_tinc, tincs, (size_t)n_msgs * 4);
  // every callback owns room for the most samples its window can hold: the reference's queueLength, or what is in the queue
  long long total = 0;
  for (int k = 0; k < n_msgs; k++) {
    u_iseen[k] = imu_seen ? imu_seen[k] : h->imu.count;
    u_oseen[k] = odom_seen ? odom_seen[k] : h->odom.count;
    u_first[k] = (int)total;
    total += h->use_imu ? std::max<long long>(1, std::min<long long>(kQueueLength, u_iseen[k] - h->imu.base)) : 1;
  }
  const int win_plane = (int)total;
  const size_t o_scans = 0, o_recs = o_scans + (size_t)n_msgs * sizeof(DeskewScan),
               o_walks = o_recs + (size_t)n_msgs * sizeof(lslam_msync_record), work_bytes = o_walks + (size_t)n_msgs * sizeof(MsyncWalk);
  if ((rc = ms_reserve(h, h->d_meta, meta_bytes)) || (rc = ms_reserve(h, h->d_work, work_bytes)) ||
      (rc = ms_reserve(h, h->d_win, (size_t)4 * win_plane)))
    return rc;
  LSLAM_HIP(ctx, hipMemcpyAsync(h->d_meta.p, up, meta_bytes, hipMemcpyHostToDevice, ctx->stream));
  MsyncQueues q;
  q.imu = h->imu.buf[h->imu.live].p; q.odom = h->odom.buf[h->odom.live].p;
  q.imu_base = h->imu.base; q.odom_base = h->odom.base;
  q.imu_cap = h->imu.cap; q.odom_cap = h->odom.cap;
  DeskewScan* d_scans = reinterpret_cast<DeskewScan*>(h->d_work.p + o_scans);
  lslam_msync_record* d_recs = reinterpret_cast<lslam_msync_record*>(h->d_work.p + o_recs);
  MsyncWalk* d_walks = reinterpret_cast<MsyncWalk*>(h->d_work.p + o_walks);
  launch(ctx, "msync_walk", k_msync_walk, dim3(1), dim3(64), 0, h->d_state.p, q, h->use_imu, h->use_odom, n, n_msgs,
         (const double*)(h->d_meta.p + o_stamps), (const float*)(h->d_meta.p + o_tinc), (const long long*)(h->d_meta.p + o_iseen),
         (const long long*)(h->d_meta.p + o_oseen), d_recs, d_walks);
  launch(ctx, "msync_windows", k_msync_windows, dim3((unsigned)n_msgs), dim3(64), 0, q, h->use_imu, h->use_odom, d_recs,
         (const MsyncWalk*)d_walks, (const int*)(h->d_meta.p + o_first), d_scans, h->d_win.p, win_plane);
  const float geom[4] = {laser->angle_min, laser->angle_increment, laser->range_min, laser->range_max};
  rc = deskew_launch_records(deskew, n_msgs, n, h->d_rows.p, n, geom, d_scans, h->d_win.p, win_plane, d_xyz, d_valid);
  if (rc) return rc;
  launch(ctx, "msync_blank", k_msync_blank, dim3((unsigned)((n + 255) / 256), (unsigned)n_msgs), dim3(256), 0,
         (const lslam_msync_record*)d_recs, n, d_xyz, d_valid);
  h->n_launches += 3;
  LSLAM_HIP(ctx, hipGetLastError());
  // the last message is the queued scan of the next call
  LSLAM_HIP(ctx, hipMemcpyAsync(h->d_rows.p, h->d_rows.p + (size_t)n_msgs * n, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  if (d_records_out)
    LSLAM_HIP(ctx, hipMemcpyAsync(d_records_out, d_recs, (size_t)n_msgs * sizeof(lslam_msync_record), hipMemcpyDeviceToDevice, ctx->stream));
  if (h->state_in_flight) {  // one pinned copy of the state: the previous one must have landed before it is overwritten
    if (hipEventQuery(h->state_done) != hipSuccess) {
      (void)hipGetLastError();
      LSLAM_HIP(ctx, hipEventSynchronize(h->state_done));
      h->n_waits++;
    }
    h->known = *h->h_state;
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(h->h_state, h->d_state.p, sizeof(MsyncState), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipEventRecord(h->state_done, ctx->stream));
  h->state_in_flight = true;
  h->scan_count = n;
  h->imu.seen = u_iseen[n_msgs - 1];
  h->odom.seen = u_oseen[n_msgs - 1];
  h->n_callbacks += n_msgs;
  h->last_n = n_msgs;
  h->last_win_plane = win_plane;
  h->last_win_first.assign(u_first, u_first + n_msgs);
  return LSLAM_OK;
}

int ms_reset_state(lslam_msync* h) {
  lslam_context* ctx = h->ctx;
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  h->state_in_flight = false;
  h->stage_used = 0;
  MsyncState fresh = {};
  fresh.start_odom = -1; fresh.end_odom = -1;
  h->known = fresh;
  LSLAM_HIP(ctx, hipMemcpy(h->d_state.p, &fresh, sizeof fresh, hipMemcpyHostToDevice));
  for (lslam_msync::Queue* q : {&h->imu, &h->odom}) {
    q->base = 0; q->count = 0; q->seen = 0;
  }
  h->scan_count = -1;
  h->last_n = 0;
  h->last_win_plane = 0;
  h->last_win_first.clear();
  h->n_callbacks = h->n_launches = 0;
  return LSLAM_OK;
}

}  // namespace

lslam_context* lslam::msync_context(const lslam_msync* h) { return h->ctx; }

int lslam::msync_check_scans(lslam_msync* h, lslam_deskew* deskew, const lslam_msync_laser* laser, int n_msgs, int n_readings,
                             const double* stamps, const float* time_increments, const int64_t* imu_seen, const int64_t* odom_seen) {
  const void* const callers = h;  // stands for the device pointers, which ms_check only compares with NULL
  return ms_check(h, deskew, laser, n_msgs, n_readings, callers, n_readings, stamps, time_increments, imu_seen, odom_seen, callers, callers);
}

void lslam::msync_stream_drained(lslam_msync* h) {
  h->stage_used = 0;
  ms_poll_state(h);
}

extern "C" {

int lslam_msync_create(lslam_context* ctx, int use_imu, int use_odom, lslam_msync** out) {
  if (!ctx || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_msync* h = new lslam_msync();
  h->ctx = ctx;
  h->use_imu = use_imu ? 1 : 0;
  h->use_odom = use_odom ? 1 : 0;
  h->imu.planes = 4;
  h->odom.planes = 8;
  if (h->d_state.reserve(1) != hipSuccess || hipHostMalloc((void**)&h->h_state, sizeof(MsyncState), hipHostMallocDefault) != hipSuccess ||
      hipEventCreateWithFlags(&h->state_done, hipEventDisableTiming) != hipSuccess || ms_reset_state(h) != LSLAM_OK) {
    (void)hipGetLastError();
    lslam_msync_destroy(h);
    return ctx->fail(LSLAM_ERR_HIP, "lslam_msync_create: cannot set up the device state");
  }
  *out = h;
  return LSLAM_OK;
}

void lslam_msync_destroy(lslam_msync* h) {
  if (!h) return;
  (void)hipSetDevice(h->ctx->device);
  (void)hipStreamSynchronize(h->ctx->stream);
  if (h->state_done) (void)hipEventDestroy(h->state_done);
  if (h->h_state) (void)hipHostFree(h->h_state);
  if (h->h_stage) (void)hipHostFree(h->h_stage);
  if (h->h_io) (void)hipHostFree(h->h_io);
  for (lslam_msync::Queue* q : {&h->imu, &h->odom})
    for (auto& b : q->buf) b.release();
  h->d_state.release();
  h->d_rows.release();
  h->d_meta.release();
  h->d_work.release();
  h->d_win.release();
  h->d_xyz.release();
  h->d_valid.release();
  delete h;
}

int lslam_msync_reset(lslam_msync* h) {
  if (!h) return LSLAM_ERR_INVALID_ARGUMENT;
  LSLAM_HIP(h->ctx, hipSetDevice(h->ctx->device));
  h->n_waits++;
  return ms_reset_state(h);
}

int lslam_msync_push_imu(lslam_msync* h, int n, const double* stamps, const double* gyro_xyz) {
  if (!h || n < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n == 0) return LSLAM_OK;
  if (!stamps || !gyro_xyz) return h->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_msync_push_imu: stamps and gyro_xyz are required");
  const double* src[4] = {stamps, gyro_xyz, gyro_xyz + 1, gyro_xyz + 2};
  const int stride[4] = {1, 3, 3, 3};
  ms_poll_state(h);
  return ms_push(h, h->imu, n, src, stride, h->known.imu_front);
}

int lslam_msync_push_odom(lslam_msync* h, int n, const double* stamps, const double* pos_xyz, const double* quat_xyzw) {
  if (!h || n < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n == 0) return LSLAM_OK;
  if (!stamps || !pos_xyz || !quat_xyzw)
    return h->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_msync_push_odom: stamps, pos_xyz and quat_xyzw are required");
  const double* src[8] = {stamps, pos_xyz, pos_xyz + 1, pos_xyz + 2, quat_xyzw, quat_xyzw + 1, quat_xyzw + 2, quat_xyzw + 3};
  const int stride[8] = {1, 3, 3, 3, 4, 4, 4, 4};
  ms_poll_state(h);
  // the sticky start / end messages may be older than the front and are still read
  long long keep = h->known.odom_front;
  if (h->known.start_odom >= 0) keep = std::min(keep, h->known.start_odom);
  if (h->known.end_odom >= 0) keep = std::min(keep, h->known.end_odom);
  return ms_push(h, h->odom, n, src, stride, keep);
}

int lslam_msync_scans_dev(lslam_msync* h, lslam_deskew* deskew, const lslam_msync_laser* laser, int n_msgs, int n_readings,
                          const float* ranges_dev, int ranges_stride, const double* stamps, const float* time_increments,
                          const int64_t* imu_seen, const int64_t* odom_seen, float* out_xyz_dev, uint8_t* out_valid_dev,
                          lslam_msync_record* records_dev) {
  int rc = ms_check(h, deskew, laser, n_msgs, n_readings, ranges_dev, ranges_stride, stamps, time_increments, imu_seen, odom_seen,
                    out_xyz_dev, out_valid_dev);
  if (rc || n_msgs == 0) return rc;
  lslam_context* ctx = h->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)n_readings;
  const bool fresh_rows = h->d_rows.p == nullptr;
  const float* old_rows = h->d_rows.p;
  if ((rc = ms_reserve(h, h->d_rows, ((size_t)n_msgs + 1) * n))) return rc;
  if (fresh_rows) LSLAM_HIP(ctx, hipMemsetAsync(h->d_rows.p, 0, n * sizeof(float), ctx->stream));
  else if (old_rows != h->d_rows.p)  // grown: the queued scan moves along
    LSLAM_HIP(ctx, hipMemcpyAsync(h->d_rows.p, old_rows, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpy2DAsync(h->d_rows.p + n, n * sizeof(float), ranges_dev, (size_t)ranges_stride * sizeof(float), n * sizeof(float),
                                  (size_t)n_msgs, hipMemcpyDeviceToDevice, ctx->stream));
  return ms_enqueue(h, deskew, laser, n_msgs, n_readings, stamps, time_increments, imu_seen, odom_seen, out_xyz_dev, out_valid_dev,
                    records_dev);
}

int lslam_msync_scans(lslam_msync* h, lslam_deskew* deskew, const lslam_msync_laser* laser, int n_msgs, int n_readings,
                      const float* ranges, int ranges_stride, const double* stamps, const float* time_increments,
                      const int64_t* imu_seen, const int64_t* odom_seen, float* out_xyz, uint8_t* out_valid,
                      lslam_msync_record* records) {
  int rc = ms_check(h, deskew, laser, n_msgs, n_readings, ranges, ranges_stride, stamps, time_increments, imu_seen, odom_seen, out_xyz,
                    out_valid);
  if (rc || n_msgs == 0) return rc;
  lslam_context* ctx = h->ctx;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)n_readings, total = (size_t)n_msgs * n;
  const size_t rec_bytes = (size_t)n_msgs * sizeof(lslam_msync_record);
  // pinned: [xyz | valid | records]; the ranges go up through the front of the xyz part (the call ends with a wait)
  const size_t io_bytes = total * 13 + 8 + rec_bytes;
  if (io_bytes > h->h_io_cap) {
    if (h->h_io) (void)hipHostFree(h->h_io);
    h->h_io = nullptr;
    h->h_io_cap = 0;
    const size_t want = io_bytes + io_bytes / 4 + 256;
    LSLAM_HIP(ctx, hipHostMalloc((void**)&h->h_io, want, hipHostMallocDefault));
    h->h_io_cap = want;
    h->n_growths++;
  }
  const bool fresh_rows = h->d_rows.p == nullptr;
  const float* old_rows = h->d_rows.p;
  if ((rc = ms_reserve(h, h->d_rows, ((size_t)n_msgs + 1) * n)) || (rc = ms_reserve(h, h->d_xyz, 3 * total)) ||
      (rc = ms_reserve(h, h->d_valid, total)))
    return rc;
  if (fresh_rows) LSLAM_HIP(ctx, hipMemsetAsync(h->d_rows.p, 0, n * sizeof(float), ctx->stream));
  else if (old_rows != h->d_rows.p)
    LSLAM_HIP(ctx, hipMemcpyAsync(h->d_rows.p, old_rows, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  float* h_r = reinterpret_cast<float*>(h->h_io);
  for (int k = 0; k < n_msgs; k++) memcpy(h_r + (size_t)k * n, ranges + (size_t)k * ranges_stride, n * sizeof(float));
  LSLAM_HIP(ctx, hipMemcpyAsync(h->d_rows.p + n, h_r, total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  rc = ms_enqueue(h, deskew, laser, n_msgs, n_readings, stamps, time_increments, imu_seen, odom_seen, h->d_xyz.p, h->d_valid.p, nullptr);
  if (rc) return rc;
  const size_t o_valid = total * 12, o_recs = (total * 13 + 7) / 8 * 8;
  LSLAM_HIP(ctx, hipMemcpyAsync(h->h_io, h->d_xyz.p, total * 12, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(h->h_io + o_valid, h->d_valid.p, total, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(h->h_io + o_recs, h->d_work.p + (size_t)n_msgs * sizeof(DeskewScan), rec_bytes, hipMemcpyDeviceToHost,
                                ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  h->n_waits++;
  h->stage_used = 0;
  ms_poll_state(h);
  memcpy(out_xyz, h->h_io, total * 12);
  memcpy(out_valid, h->h_io + o_valid, total);
  if (records) memcpy(records, h->h_io + o_recs, rec_bytes);
  return LSLAM_OK;
}

int lslam_msync_read_windows(lslam_msync* h, int32_t* imu_first, double* imu_time, double* imu_rot_xyz, int capacity) {
  if (!h || !imu_first || capacity < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = h->ctx;
  imu_first[0] = 0;
  if (h->last_n == 0) return LSLAM_OK;
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  h->n_waits++;
  const int nm = h->last_n;
  std::vector<lslam_msync_record> recs((size_t)nm);
  LSLAM_HIP(ctx, hipMemcpy(recs.data(), h->d_work.p + (size_t)nm * sizeof(DeskewScan), (size_t)nm * sizeof(lslam_msync_record),
                           hipMemcpyDeviceToHost));
  for (int k = 0; k < nm; k++) imu_first[k + 1] = imu_first[k] + (recs[k].status == LSLAM_MSYNC_CORRECTED ? recs[k].n_imu : 0);
  if (capacity == 0) return LSLAM_OK;
  if (capacity < imu_first[nm] || !imu_time || !imu_rot_xyz)
    return ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "lslam_msync_read_windows: %d samples, capacity %d", imu_first[nm], capacity);
  std::vector<double> win((size_t)4 * h->last_win_plane);
  LSLAM_HIP(ctx, hipMemcpy(win.data(), h->d_win.p, win.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int k = 0; k < nm; k++)
    for (int j = 0; j < imu_first[k + 1] - imu_first[k]; j++) {
      const size_t at = (size_t)h->last_win_first[k] + j, to = (size_t)imu_first[k] + j;
      imu_time[to] = win[at];
      for (int a = 0; a < 3; a++) imu_rot_xyz[3 * to + a] = win[(size_t)(a + 1) * h->last_win_plane + at];
    }
  return LSLAM_OK;
}

int lslam_msync_stats(lslam_msync* h, int64_t out[6]) {
  if (!h || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  if (h->state_in_flight) {
    if (hipEventQuery(h->state_done) != hipSuccess) {
      (void)hipGetLastError();
      LSLAM_HIP(h->ctx, hipEventSynchronize(h->state_done));
      h->n_waits++;
    }
    h->known = *h->h_state;
    h->state_in_flight = false;
  }
  out[0] = h->n_callbacks; out[1] = h->known.n_corrected; out[2] = h->known.n_refused;
  out[3] = h->n_launches; out[4] = h->n_growths; out[5] = h->n_waits;
  return LSLAM_OK;
}

}  // extern "C"
