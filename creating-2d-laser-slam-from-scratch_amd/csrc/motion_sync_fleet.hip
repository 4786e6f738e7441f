// lesson5's IMU / odometry synchronisation for the nodes of a whole Hector fleet (lslam_hector_fleet_process_many_synced): the
// kernels of csrc/motion_sync.hip with the node found in the grid.  The callbacks of one node are a true dependency, the
// nodes are independent, so the walk is one wave per member and the windows are one wave per (callback, member); both call
// the device bodies of k_msync_walk / k_msync_windows (csrc/motion_sync_impl.hpp), so a member's bits are those of its own
// lslam_msync_scans call.  The blanking of the rows of queued and refused callbacks needs no twin: the fleet's records are
// contiguous over its members, so ONE launch of k_msync_blank over all rows is that kernel as it stands.
//
//   k_msync_fleet_rows     in front of the walk: member m's queued scan becomes the ranges row of its first callback, and
//                          the last message of the call becomes its queued scan -- one launch instead of 2 R copies
//   k_msync_fleet_walk     grid R, one wave each; leaves every node's state in the handle's own block AND side by side in
//                          one array, for ONE copy to the host
//   k_msync_fleet_windows  grid (most callbacks of a member, R), one wave each
//
// The host side -- the plan of a call, its buffers, what a handle keeps -- is MsyncFleet in csrc/motion_sync.hip.
#include "motion_sync_impl.hpp"

using namespace lslam;

namespace {

// row row0 + j, j >= 1, of a member is its message j - 1 (uploaded by the host), as in a handle's own rows; row row0 is the
// scan the handle has queued, and tail row m -- the member's last message -- is what it queues for its next call
__global__ void __launch_bounds__(256)
k_msync_fleet_rows(const MsyncMember* __restrict__ mem, int n, float* __restrict__ rows, const float* __restrict__ tail) {
  const MsyncMember e = mem[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (e.n_cb < 1 || i >= n) return;
  rows[(size_t)e.row0 * n + i] = e.queued_row[i];
  e.queued_row[i] = tail[(size_t)blockIdx.y * n + i];
}

__global__ void __launch_bounds__(64)
k_msync_fleet_walk(const MsyncMember* __restrict__ mem, int scan_count, const double* __restrict__ stamps,
                   const float* __restrict__ tincs, const long long* __restrict__ imu_seen, const long long* __restrict__ odom_seen,
                   lslam_msync_record* __restrict__ recs, MsyncWalk* __restrict__ walks, MsyncState* __restrict__ states_out) {
  const MsyncMember e = mem[blockIdx.x];
  if (e.n_cb < 1) return;
  msync_walk_body(e.state, e.q, e.use_imu, e.use_odom, scan_count, e.n_cb, stamps + e.row0, tincs + e.row0, imu_seen + e.row0,
                  odom_seen + e.row0, recs + e.row0, walks + e.row0);
  if (threadIdx.x == 0) states_out[blockIdx.x] = *e.state;
}

__global__ void __launch_bounds__(64)
k_msync_fleet_windows(const MsyncMember* __restrict__ mem, lslam_msync_record* recs, const MsyncWalk* __restrict__ walks,
                      const int* __restrict__ win_first, DeskewScan* __restrict__ scans, double* win, int win_plane) {
  const MsyncMember e = mem[blockIdx.y];
  if ((int)blockIdx.x >= e.n_cb) return;
  msync_windows_body(e.q, e.use_imu, e.use_odom, e.row0 + (int)blockIdx.x, recs, walks, win_first, scans, win, win_plane);
}

}  // namespace

void lslam::msync_fleet_launch_rows(lslam_context* ctx, const MsyncMember* mem, int R, int n, float* rows, const float* tail) {
  launch(ctx, "msync_fleet_rows", k_msync_fleet_rows, dim3((unsigned)((n + 255) / 256), (unsigned)R), dim3(256), 0, mem, n, rows, tail);
}

void lslam::msync_fleet_launch_walk(lslam_context* ctx, const MsyncMember* mem, int R, int scan_count, const double* stamps,
                                    const float* tincs, const long long* imu_seen, const long long* odom_seen,
                                    lslam_msync_record* recs, MsyncWalk* walks, MsyncState* states_out) {
  launch(ctx, "msync_fleet_walk", k_msync_fleet_walk, dim3((unsigned)R), dim3(64), 0, mem, scan_count, stamps, tincs, imu_seen,
         odom_seen, recs, walks, states_out);
}

void lslam::msync_fleet_launch_windows(lslam_context* ctx, const MsyncMember* mem, int R, int max_cb, lslam_msync_record* recs,
                                       const MsyncWalk* walks, const int* win_first, DeskewScan* scans, double* win, int win_plane) {
  launch(ctx, "msync_fleet_windows", k_msync_fleet_windows, dim3((unsigned)max_cb, (unsigned)R), dim3(64), 0, mem, recs, walks, win_first,
         scans, win, win_plane);
}
