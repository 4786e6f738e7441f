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
// The walk's and the windows' bodies live in csrc/motion_sync_impl.hpp: csrc/motion_sync_fleet.hip runs them for the nodes of
// a whole Hector fleet in one launch each (MsyncFleet below is its host side).
//
// Defined where the reference is not: a sample inside the scan with no sample before the scan's start makes :237 read
// imu_time_[-1] (IMU_NO_LEAD_SAMPLE, refused); more than queueLength = 2000 integrated samples run past imu_time_'s end
// (IMU_OVERFLOW, refused).  Both are refusals of the IMU step: the odometry step does not run, the IMU pops stay made.
#include <cmath>

#include "motion_sync_impl.hpp"

using namespace lslam;

namespace {

__global__ void __launch_bounds__(64)
k_msync_walk(MsyncState* __restrict__ state, MsyncQueues q, int use_imu, int use_odom, int scan_count, int n_msgs,
             const double* __restrict__ stamps, const float* __restrict__ tincs, const long long* __restrict__ imu_seen,
             const long long* __restrict__ odom_seen, lslam_msync_record* __restrict__ recs, MsyncWalk* __restrict__ walks) {
  msync_walk_body(state, q, use_imu, use_odom, scan_count, n_msgs, stamps, tincs, imu_seen, odom_seen, recs, walks);
}

__global__ void __launch_bounds__(64)
k_msync_windows(MsyncQueues q, int use_imu, int use_odom, lslam_msync_record* recs, const MsyncWalk* __restrict__ walks,
                const int* __restrict__ win_first, DeskewScan* __restrict__ scans, double* win, int win_plane) {
  msync_windows_body(q, use_imu, use_odom, (int)blockIdx.x, recs, walks, win_first, scans, win, win_plane);
}

// (the fleet's records are contiguous over its members: one launch of this kernel over all rows serves it as it stands)
__global__ void __launch_bounds__(256)
k_msync_blank(const lslam_msync_record* __restrict__ recs, int n, float* __restrict__ out_xyz, uint8_t* __restrict__ valid) {
  msync_blank_body(recs, n, (int)blockIdx.y, (int)(blockIdx.x * blockDim.x + threadIdx.x), out_xyz, valid);
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
  bool last_in_fleet = false;  // the last call was a fleet's: its windows live in the fleet's buffer (read_windows refuses)
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
  h->last_in_fleet = false;
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
  h->last_in_fleet = false;
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

// ------------------------------------------------------------------------------------------
// MsyncFleet: the buffers of one fleet call and its plan.  Launches per call: k_msync_fleet_rows / _walk / _windows
// (csrc/motion_sync_fleet.hip), k_deskew_batch, k_msync_blank -- kFleetLaunches, whatever R and the number of steps are (a new scan geometry adds the de-skew's angle table).
// ------------------------------------------------------------------------------------------
struct lslam::MsyncFleet {
  lslam_context* ctx = nullptr;
  DevBuf<unsigned char> d_meta, d_work;  // [member table | stamps | imu_seen | odom_seen | win_first | tincs]; [scans | records | walks]
  DevBuf<double> d_win;
  DevBuf<float> d_rows, d_xyz;           // d_rows: the N rows of the call, then one tail row per member
  DevBuf<uint8_t> d_valid;
  DevBuf<MsyncState> d_states;
  unsigned char* h_up = nullptr;         // pinned, what goes up: the meta block, then the ranges
  unsigned char* h_down = nullptr;       // pinned, what comes down: the records, then the states
  size_t h_up_cap = 0, h_down_cap = 0;
  // the plan of the call
  std::vector<lslam_msync*> syncs;
  int R = 0, n = 0, n_steps = 0, N = 0, max_cb = 0, win_plane = 0;
  std::vector<int> n_cb, row0, row_of, win_first;
  std::vector<double> stamps;
  std::vector<float> tincs;
  std::vector<long long> iseen, oseen;
  int64_t n_calls = 0, n_launches = 0, n_growths = 0, n_waits = 0;
};

namespace {

constexpr int kFleetLaunches = 5;

template <typename T>
int mf_reserve(MsyncFleet* mf, DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return LSLAM_OK;
  LSLAM_HIP(mf->ctx, b.reserve(n));
  mf->n_growths++;
  return LSLAM_OK;
}

int mf_pinned(MsyncFleet* mf, unsigned char** p, size_t* cap, size_t bytes) {  // (every call ends with a wait: never in flight here)
  if (bytes <= *cap) return LSLAM_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = bytes + bytes / 4 + 256;
  LSLAM_HIP(mf->ctx, hipHostMalloc((void**)p, want, hipHostMallocDefault));
  *cap = want;
  mf->n_growths++;
  return LSLAM_OK;
}

}  // namespace

MsyncFleet* lslam::msync_fleet_create(lslam_context* ctx) {
  MsyncFleet* mf = new MsyncFleet();
  mf->ctx = ctx;
  return mf;
}

void lslam::msync_fleet_destroy(MsyncFleet* mf) {
  if (!mf) return;
  if (mf->h_up) (void)hipHostFree(mf->h_up);
  if (mf->h_down) (void)hipHostFree(mf->h_down);
  mf->d_meta.release();
  mf->d_work.release();
  mf->d_win.release();
  mf->d_rows.release();
  mf->d_xyz.release();
  mf->d_valid.release();
  mf->d_states.release();
  delete mf;
}

int lslam::msync_fleet_plan(MsyncFleet* mf, lslam_msync* const* syncs, int R, lslam_deskew* deskew, const lslam_msync_laser* laser,
                            int n_steps, int n_readings, const double* stamps, const float* time_increments,
                            const int64_t* imu_seen, const int64_t* odom_seen, const uint8_t* active) {
  lslam_context* ctx = mf->ctx;
  const size_t total = (size_t)n_steps * (size_t)R;
  mf->syncs.assign(syncs, syncs + R);
  mf->R = R; mf->n = n_readings; mf->n_steps = n_steps;
  mf->n_cb.assign((size_t)R, 0);
  mf->row0.assign((size_t)R, 0);
  mf->row_of.assign(total, -1);
  for (size_t i = 0; i < total; i++) mf->n_cb[i % (size_t)R] += !active || active[i];
  size_t N = 0;
  mf->max_cb = 0;
  for (int m = 0; m < R; m++) {
    mf->row0[m] = (int)N;
    N += (size_t)mf->n_cb[m];
    mf->max_cb = std::max(mf->max_cb, mf->n_cb[m]);
  }
  if (N > 65535)  // k_deskew_batch and k_msync_blank take a scan per grid row
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_process_many_synced: at most 65535 scan callbacks per call over "
                     "all members (got %zu); make shorter calls", N);
  mf->N = (int)N;
  mf->stamps.assign(N, 0.0);
  mf->tincs.assign(N, 0.f);
  mf->iseen.assign(N, 0);
  mf->oseen.assign(N, 0);
  mf->win_first.assign(N, 0);
  std::vector<int64_t> is, os;
  long long room = 0;
  for (int m = 0; m < R; m++) {  // member-major: member m's callbacks in step order
    const int c = mf->n_cb[m];
    if (c == 0) continue;
    lslam_msync* h = syncs[m];
    const int r0 = mf->row0[m];
    is.assign((size_t)c, 0);
    os.assign((size_t)c, 0);
    int j = 0;
    for (int k = 0; k < n_steps; k++) {
      const size_t i = (size_t)k * R + m;
      if (active && !active[i]) continue;
      mf->row_of[i] = r0 + j;
      mf->stamps[r0 + j] = stamps[i];
      mf->tincs[r0 + j] = time_increments[i];
      is[j] = imu_seen ? imu_seen[i] : (int64_t)h->imu.count;
      os[j] = odom_seen ? odom_seen[i] : (int64_t)h->odom.count;
      j++;
    }
    const void* const callers = h;  // stands for the device pointers, which ms_check only compares with NULL
    int rc = ms_check(h, deskew, laser, c, n_readings, callers, n_readings, mf->stamps.data() + r0, mf->tincs.data() + r0, is.data(),
                      os.data(), callers, callers);
    if (rc) return rc;
    for (j = 0; j < c; j++) {  // every callback owns room for the most samples its window can hold, as in ms_enqueue
      mf->iseen[r0 + j] = is[j];
      mf->oseen[r0 + j] = os[j];
      if (room > INT_MAX)
        return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_process_many_synced: the IMU windows of the call need more than "
                         "INT_MAX samples of room; make shorter calls");
      mf->win_first[r0 + j] = (int)room;
      room += h->use_imu ? std::max<long long>(1, std::min<long long>(kQueueLength, is[j] - h->imu.base)) : 1;
    }
  }
  if (room > INT_MAX)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_fleet_process_many_synced: the IMU windows of the call need more than "
                     "INT_MAX samples of room; make shorter calls");
  mf->win_plane = (int)room;
  return LSLAM_OK;
}

int lslam::msync_fleet_enqueue(MsyncFleet* mf, lslam_deskew* deskew, const lslam_msync_laser* laser, const float* ranges,
                               int ranges_stride, const float** d_xyz, const uint8_t** d_valid,
                               const lslam_msync_record** d_records, const int** row_of) {
  lslam_context* ctx = mf->ctx;
  const int R = mf->R, N = mf->N;
  const size_t n = (size_t)mf->n, Nz = (size_t)N;
  *row_of = mf->row_of.data();
  // ---- every buffer first (an allocation may wait for the device, but enqueues nothing)
  const size_t o_mem = 0, o_stamps = o_mem + (size_t)R * sizeof(MsyncMember), o_iseen = o_stamps + Nz * 8, o_oseen = o_iseen + Nz * 8,
               o_first = o_oseen + Nz * 8, o_tinc = o_first + Nz * 4, meta_bytes = (o_tinc + Nz * 4 + 7) / 8 * 8;
  const size_t o_scans = 0, o_recs = o_scans + Nz * sizeof(DeskewScan), o_walks = o_recs + Nz * sizeof(lslam_msync_record),
               work_bytes = o_walks + Nz * sizeof(MsyncWalk);
  const size_t rows = Nz + (size_t)R, rec_bytes = Nz * sizeof(lslam_msync_record);
  int rc;
  if ((rc = mf_reserve(mf, mf->d_meta, meta_bytes)) || (rc = mf_reserve(mf, mf->d_work, std::max<size_t>(work_bytes, 8))) ||
      (rc = mf_reserve(mf, mf->d_win, (size_t)4 * std::max(mf->win_plane, 1))) || (rc = mf_reserve(mf, mf->d_rows, rows * n)) ||
      (rc = mf_reserve(mf, mf->d_xyz, std::max<size_t>(3 * Nz * n, 1))) || (rc = mf_reserve(mf, mf->d_valid, std::max<size_t>(Nz * n, 1))) ||
      (rc = mf_reserve(mf, mf->d_states, (size_t)R)) ||
      (rc = mf_pinned(mf, &mf->h_up, &mf->h_up_cap, meta_bytes + rows * n * sizeof(float))) ||
      (rc = mf_pinned(mf, &mf->h_down, &mf->h_down_cap, rec_bytes + (size_t)R * sizeof(MsyncState))))
    return rc;
  *d_xyz = mf->d_xyz.p;
  *d_valid = mf->d_valid.p;
  *d_records = reinterpret_cast<const lslam_msync_record*>(mf->d_work.p + o_recs);
  // Every member with callbacks owns a queued-scan row of at least n floats, which k_msync_fleet_rows reads and writes in
  // full.  A handle that has a scan queued has rows of this n already (ms_check: n is its scan_count, and every call
  // reserves two rows or more).  One that has none -- its first scan ever, or its first after lslam_msync_reset, which
  // forgets scan_count but keeps the buffers, possibly of a SHORTER scan -- gets a row that is long enough and zero (it is
  // never used: has_queued is 0), as the handle's own calls make it.
  for (int m = 0; m < R; m++) {
    lslam_msync* h = mf->syncs[m];
    if (!mf->n_cb[m] || h->d_rows.cap >= n) continue;
    if ((rc = ms_reserve(h, h->d_rows, 2 * n))) return rc;
    LSLAM_HIP(ctx, hipMemsetAsync(h->d_rows.p, 0, n * sizeof(float), ctx->stream));
  }
  mf->n_calls++;
  if (N == 0) return LSLAM_OK;  // nobody has a callback: nothing to run
  for (int m = 0; m < R; m++)
    if (mf->n_cb[m]) ms_poll_state(mf->syncs[m]);
  // ---- up: the member table and the call's small inputs in one copy, the ranges in another
  unsigned char* up = mf->h_up;
  MsyncMember* u_mem = reinterpret_cast<MsyncMember*>(up + o_mem);
  for (int m = 0; m < R; m++) {
    lslam_msync* h = mf->syncs[m];
    MsyncMember e{};
    e.n_cb = mf->n_cb[m];
    e.row0 = mf->row0[m];
    if (e.n_cb) {
      e.state = h->d_state.p;
      e.queued_row = h->d_rows.p;
      e.q.imu = h->imu.buf[h->imu.live].p; e.q.odom = h->odom.buf[h->odom.live].p;
      e.q.imu_base = h->imu.base; e.q.odom_base = h->odom.base;
      e.q.imu_cap = h->imu.cap; e.q.odom_cap = h->odom.cap;
      e.use_imu = h->use_imu; e.use_odom = h->use_odom;
    }
    u_mem[m] = e;
  }
  memcpy(up + o_stamps, mf->stamps.data(), Nz * 8);
  memcpy(up + o_iseen, mf->iseen.data(), Nz * 8);
  memcpy(up + o_oseen, mf->oseen.data(), Nz * 8);
  memcpy(up + o_first, mf->win_first.data(), Nz * 4);
  memcpy(up + o_tinc, mf->tincs.data(), Nz * 4);
  LSLAM_HIP(ctx, hipMemcpyAsync(mf->d_meta.p, up, meta_bytes, hipMemcpyHostToDevice, ctx->stream));
  // row row0 + j, j >= 1, is member m's message j - 1; its last message is tail row m; row row0 is k_msync_fleet_rows'
  float* u_rows = reinterpret_cast<float*>(up + meta_bytes);
  for (size_t i = 0; i < mf->row_of.size(); i++) {
    const int row = mf->row_of[i];
    if (row < 0) continue;
    const int m = (int)(i % (size_t)R);
    const bool last = row == mf->row0[m] + mf->n_cb[m] - 1;
    memcpy(u_rows + (last ? Nz + (size_t)m : (size_t)row + 1) * n, ranges + i * (size_t)ranges_stride, n * sizeof(float));
  }
  LSLAM_HIP(ctx, hipMemcpyAsync(mf->d_rows.p, u_rows, rows * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  const MsyncMember* d_mem = reinterpret_cast<const MsyncMember*>(mf->d_meta.p + o_mem);
  DeskewScan* d_scans = reinterpret_cast<DeskewScan*>(mf->d_work.p + o_scans);
  lslam_msync_record* d_recs = reinterpret_cast<lslam_msync_record*>(mf->d_work.p + o_recs);
  MsyncWalk* d_walks = reinterpret_cast<MsyncWalk*>(mf->d_work.p + o_walks);
  msync_fleet_launch_rows(ctx, d_mem, R, (int)n, mf->d_rows.p, mf->d_rows.p + Nz * n);
  msync_fleet_launch_walk(ctx, d_mem, R, (int)n, (const double*)(mf->d_meta.p + o_stamps), (const float*)(mf->d_meta.p + o_tinc),
                          (const long long*)(mf->d_meta.p + o_iseen), (const long long*)(mf->d_meta.p + o_oseen), d_recs, d_walks,
                          mf->d_states.p);
  msync_fleet_launch_windows(ctx, d_mem, R, mf->max_cb, d_recs, d_walks, (const int*)(mf->d_meta.p + o_first), d_scans, mf->d_win.p,
                             mf->win_plane);
  const float geom[4] = {laser->angle_min, laser->angle_increment, laser->range_min, laser->range_max};
  rc = deskew_launch_records(deskew, N, (int)n, mf->d_rows.p, (int)n, geom, d_scans, mf->d_win.p, mf->win_plane, mf->d_xyz.p,
                             mf->d_valid.p);
  if (rc) return rc;
  launch(ctx, "msync_blank", k_msync_blank, dim3((unsigned)((n + 255) / 256), (unsigned)N), dim3(256), 0,
         (const lslam_msync_record*)d_recs, (int)n, mf->d_xyz.p, mf->d_valid.p);
  mf->n_launches += kFleetLaunches;
  LSLAM_HIP(ctx, hipGetLastError());
  // what each handle's own bookkeeping must know (its launches do not move: the fleet counts those)
  for (int m = 0; m < R; m++) {
    const int c = mf->n_cb[m];
    if (!c) continue;
    lslam_msync* h = mf->syncs[m];
    const int last = mf->row0[m] + c - 1;
    h->scan_count = (int)n;
    h->imu.seen = mf->iseen[last];
    h->odom.seen = mf->oseen[last];
    h->n_callbacks += c;
    h->last_n = 0;
    h->last_win_plane = 0;
    h->last_win_first.clear();
    h->last_in_fleet = true;
  }
  return LSLAM_OK;
}

int lslam::msync_fleet_download(MsyncFleet* mf) {
  lslam_context* ctx = mf->ctx;
  if (mf->N == 0) return LSLAM_OK;
  const size_t Nz = (size_t)mf->N, rec_bytes = Nz * sizeof(lslam_msync_record);
  LSLAM_HIP(ctx, hipMemcpyAsync(mf->h_down, mf->d_work.p + Nz * sizeof(DeskewScan), rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(mf->h_down + rec_bytes, mf->d_states.p, (size_t)mf->R * sizeof(MsyncState), hipMemcpyDeviceToHost,
                                ctx->stream));
  return LSLAM_OK;
}

void lslam::msync_fleet_finish(MsyncFleet* mf, lslam_msync_record* records) {
  mf->n_waits++;
  const lslam_msync_record* recs = reinterpret_cast<const lslam_msync_record*>(mf->h_down);
  const MsyncState* states = reinterpret_cast<const MsyncState*>(mf->h_down + (size_t)mf->N * sizeof(lslam_msync_record));
  for (int m = 0; m < mf->R; m++) {
    if (!mf->n_cb[m]) continue;
    lslam_msync* h = mf->syncs[m];
    h->known = states[m];  // newer than any copy of the handle's own that was in flight, which has landed too
    h->state_in_flight = false;
    h->stage_used = 0;
  }
  if (!records) return;
  for (size_t i = 0; i < mf->row_of.size(); i++) {
    if (mf->row_of[i] < 0) memset(&records[i], 0, sizeof records[i]);
    else records[i] = recs[mf->row_of[i]];
  }
}

void lslam::msync_fleet_stats(const MsyncFleet* mf, int64_t out[4]) {
  out[0] = mf->n_calls; out[1] = mf->n_launches; out[2] = mf->n_growths; out[3] = mf->n_waits;
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
  if (h->last_in_fleet)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_msync_read_windows: the handle's last call was a fleet's "
                     "(lslam_hector_fleet_process_many_synced), whose windows live in the fleet's buffer; they are readable "
                     "again after the handle's next call of its own");
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
