// lslam_hector_loc_*: R trackers localising on ONE borrowed, finished map.  Included at the end of logodds_map.hip, whose
// matcher bodies, projection and staging helpers it calls.
//
// A taken entry is HectorSlamProcessor::update (H/slam_main/HectorSlamProcessor.h:81-108) with the gate never firing: matchData
// from the hint or the tracker's own last pose, lastScanMatchPose / lastScanMatchCov set, no updateByScan.  The map does not
// change, so nothing orders one tracker against another, and within a tracker the only dependency is its own pose chain:
//   k_hl_container   one block per ENTRY of the chunk (step * R + tracker): hector_project_body, or hector_compact over
//                    hector_cloud_point as the gated cloud kernels run it, into a block [entry][capacity][2] of the handle's own
//                    plus a count per entry.  Containers do not depend on poses: one parallel launch.  (The container form has
//                    no such launch: the caller's points are read where they were staged.)
//   k_hl_track_*     one block per TRACKER walks its entries of the chunk in step order: take / active word, start pose from the
//                    hint or the state block, gn_match_reg_body / gn_match_fast_body on entry i's container, one thread writes
//                    the state and the record, a block barrier, next step.  The loop is bounded by the host's step count; no
//                    hand-over words, no spinning, no cooperative launch, no ordering between blocks.
// The matcher writes no cached container (cache_dst = nullptr): nothing of the map is stored to.

namespace {

struct HlTracker {
  float pose[3];  // lastScanMatchPose
  float cov[9];   // lastScanMatchCov
};

struct HlCall {             // one chunk; every per-entry pointer is at the chunk's first entry
  int R, n_steps, capacity;
  const uint8_t* active;    // null: all active
  const int32_t* take;      // null: every active entry is taken; else taken iff take[i * take_stride] > 0
  int take_stride;
  const float* hints;       // [i][3]; null: chained
  const float* pts;         // the containers: entry i at first[i] points, or (first null) at i * capacity
  const int* first;
  const int* counts;
  HlTracker* state;         // [R]
  lslam_hector_record* rec;
};

struct HlSource {           // what k_hl_container reads and writes, at the chunk's first entry
  const float* ranges;      // ranges form: [i][pc.n]; null: cloud form
  const double2* cossin;
  const float* xyz;         // [i][pc.n][3]
  const uint8_t* valid;     // [i][pc.n]; null: every point is valid
  float* cont;              // [i][pc.n][2]
  int* counts;
};

__device__ __forceinline__ bool hl_taken(const HlCall& c, size_t i) {
  if (c.active && !c.active[i]) return false;
  return !c.take || c.take[i * (size_t)c.take_stride] > 0;
}

__global__ void __launch_bounds__(1024)
k_hl_container(ProjectCfg pc, HlCall c, HlSource s) {
  const size_t i = blockIdx.x;
  if (!__builtin_amdgcn_readfirstlane((int)hl_taken(c, i))) return;
  float* __restrict__ out = s.cont + 2 * i * (size_t)pc.n;
  int* __restrict__ out_n = s.counts + i;
  if (s.ranges) {
    hector_project_body(pc, s.ranges + i * (size_t)pc.n, s.cossin, out, out_n);
  } else {
    const float* __restrict__ xyz = s.xyz + 3 * i * (size_t)pc.n;
    const uint8_t* __restrict__ valid = s.valid ? s.valid + i * (size_t)pc.n : nullptr;
    hector_compact(pc.n, out, out_n, [&](int p, float& ox, float& oy) {
      if (valid && !valid[p]) return false;
      return hector_cloud_point(pc, xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2], ox, oy);
    });
  }
}

// ONE thread: the record of an entry that was not taken; the tracker's state is not touched
__device__ __forceinline__ void hl_skip(lslam_hector_record* __restrict__ rec) {
  for (int q = 0; q < 3; q++) rec->pose[q] = 0.0f;
  for (int q = 0; q < 9; q++) rec->cov[q] = 0.0f;
  rec->updated = 0;
  rec->n_points = -1;
  rec->pad[0] = rec->pad[1] = 0;
}

// ONE thread: HectorSlamProcessor.h:91-98 -- what hs_finish does of them, and nothing of its gate
__device__ __forceinline__ void hl_finish(HlTracker* st, lslam_hector_record* __restrict__ rec, const float* pose, const float* H,
                                          int n) {
  if (n > 0)  // ScanMatcher.h:96: an empty container leaves covMatrix untouched
    for (int q = 0; q < 9; q++) st->cov[q] = H[q];
  for (int q = 0; q < 3; q++) st->pose[q] = pose[q];
  for (int q = 0; q < 3; q++) rec->pose[q] = pose[q];
  for (int q = 0; q < 9; q++) rec->cov[q] = st->cov[q];
  rec->updated = 0;
  rec->n_points = n;
  rec->pad[0] = rec->pad[1] = 0;
}

// Block t's walk over tracker t's entries.  match(pts, n, b, pose, H) is one of the two matcher bodies.  Two barriers per
// taken step: the first keeps the thread that rewrites the state behind every reader of the start pose also where the body
// runs no iteration (hs_begin's), the second stands between that write -- and the body's last reads of its LDS (the waves'
// partial sums, the staged points) -- and the next step's reads and writes of the same words.
template <class Match>
__device__ __forceinline__ void hl_walk(const HlCall& c, Match match) {
  const unsigned t = blockIdx.x;
  HlTracker* st = c.state + t;
  for (int k = 0; k < c.n_steps; k++) {
    const size_t i = (size_t)k * (size_t)c.R + t;
    lslam_hector_record* rec = c.rec + i;
    if (!__builtin_amdgcn_readfirstlane((int)hl_taken(c, i))) {  // (the words are uniform over the block)
      if (threadIdx.x == 0) hl_skip(rec);
      continue;
    }
    int n = c.counts[i];
    n = n < 0 ? 0 : (n > c.capacity ? c.capacity : n);  // clamped before any indexing
    n = __builtin_amdgcn_readfirstlane(n);
    float b[3], pose[3], H[9];
    for (int q = 0; q < 3; q++) b[q] = c.hints ? c.hints[3 * i + q] : st->pose[q];
    __syncthreads();
    const float* pts = c.pts + 2 * (c.first ? (size_t)c.first[i] : i * (size_t)c.capacity);
    match(pts, n, b, pose, H);
    if (threadIdx.x == 0) hl_finish(st, rec, pose, H, n);
    __syncthreads();
  }
}

template <int NT, int PMAX>
__global__ void __launch_bounds__(NT)
k_hl_track_reg(GnLevels lv, HlCall c) {
  hl_walk(c, [&](const float* pts, int n, const float* b, float* pose, float* H) {
    gn_match_reg_body<NT, PMAX>(lv, pts, nullptr, n, b[0], b[1], b[2], pose, H);
  });
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_hl_track_fast(GnLevels lv, HlCall c, int pts_in_lds) {
  hl_walk(c, [&](const float* pts, int n, const float* b, float* pose, float* H) {
    gn_match_fast_body<NT>(lv, pts, nullptr, n, pts_in_lds, b[0], b[1], b[2], pose, H);
  });
}

constexpr int kHlMaxTrackers = 65535;
constexpr size_t kHlContainerBudget = (size_t)64 << 20;  // bytes of one chunk's container block (default chunking)

}  // namespace

struct lslam_hector_loc {
  lslam_map* map = nullptr;
  int R = 0;
  int max_steps = 0;             // LSLAM_HECTOR_LOC_OPT_MAX_STEPS_PER_LAUNCH; 0: from kHlContainerBudget
  HlTracker* d_state = nullptr;  // [R]
  HlTracker* h_state = nullptr;  // pinned [R]: what the trackers are between calls (up at the start of a call, down at its end)
  HsStage in;
  uint32_t* h_aux = nullptr;     // pinned: [hints 3n floats | first n ints | active n bytes]
  size_t h_aux_cap = 0;
  DevBuf<uint32_t> d_aux;
  DevBuf<float> d_cont;          // one chunk's containers
  DevBuf<int> d_counts;          // their counts, for the whole call
  DevBuf<lslam_hector_record> d_rec;
  lslam_hector_record* h_rec = nullptr;
  size_t h_rec_cap = 0;
  DevBuf<double2> d_cossin;      // laser_geometry's co_sine_map_ of the last ranges-form geometry (the map's own is the map's)
  float cs_angle_min = 0.f, cs_angle_inc = 0.f;
  int cs_n = 0;
  int64_t n_steps = 0, n_matched = 0, n_calls = 0, n_syncs = 0, n_launches = 0, n_track_launches = 0;
};

namespace {

struct HlRun {
  int n_steps = 0, capacity = 0;
  const lslam_hector_scan* scan = nullptr;  // ranges and cloud forms: the projection's configuration
  const float* d_ranges = nullptr;          // ranges form
  const float* d_xyz = nullptr;             // cloud forms
  const uint8_t* d_valid = nullptr;
  const int32_t* d_take = nullptr;
  int take_stride = 0;
  const int32_t* n_points = nullptr;        // container form: the host counts (the points are in l->in.d_in, the counts in
  const float* hints = nullptr;             //   l->in.d_counts)
  const uint8_t* active = nullptr;
  lslam_hector_record* out = nullptr;
};

// what every form refuses before anything touches the device
int hl_check(lslam_hector_loc* l, const char* who, int capacity) {
  lslam_map* map = l->map;
  lslam_context* ctx = map->ctx;
  if (map->ordered_sums)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: the localiser runs the parallel-sum matcher; LSLAM_MAP_OPT_ORDERED_SUMS maps go "
                     "through lslam_map_match_data", who);
  if ((int)map->levels.size() > kGnMaxLevels) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d pyramid levels", who, kGnMaxLevels);
  if (capacity > kMaxBeams)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: at most %d readings or points per scan (got %d)", who, kMaxBeams, capacity);
  return LSLAM_OK;
}

// the handle's own cos/sin table (ensure_cossin keeps the map's, which lslam_map_set_scan may rebuild between calls)
int hl_ensure_cossin(lslam_hector_loc* l, int n, const lslam_hector_scan* sp) {
  lslam_context* ctx = l->map->ctx;
  if (!(n > l->cs_n || sp->angle_min != l->cs_angle_min || sp->angle_increment != l->cs_angle_inc)) return LSLAM_OK;
  std::vector<double2> cs((size_t)std::max(n, 1));
  for (int i = 0; i < n; i++) {
    const double a = (double)sp->angle_min + (double)i * (double)sp->angle_increment;
    cs[i] = make_double2(cos(a), sin(a));
  }
  LSLAM_HIP(ctx, l->d_cossin.reserve(cs.size()));
  LSLAM_HIP(ctx, hipMemcpyAsync(l->d_cossin.p, cs.data(), cs.size() * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));  // cs dies with this scope
  l->n_syncs++;
  l->cs_n = n;
  l->cs_angle_min = sp->angle_min;
  l->cs_angle_inc = sp->angle_increment;
  return LSLAM_OK;
}

int hl_run(lslam_hector_loc* l, const HlRun& c) {
  lslam_map* map = l->map;
  lslam_context* ctx = map->ctx;
  const int R = l->R;
  const size_t total = (size_t)c.n_steps * (size_t)R;
  const bool container_form = c.scan == nullptr;
  {
    int rc = flush_pending(map);  // the matcher reads the float planes
    if (rc) return rc;
  }
  // ---- chunks: steps per launch from the option, else from the container block's budget
  int chunk = c.n_steps;
  if (l->max_steps > 0) chunk = std::min(chunk, l->max_steps);
  else if (!container_form) {
    const size_t per_step = (size_t)R * (size_t)std::max(c.capacity, 1) * 2 * sizeof(float);
    chunk = (int)std::min((size_t)chunk, std::max((size_t)1, kHlContainerBudget / per_step));
  }
  // ---- buffers (a repeated shape allocates nothing)
  LSLAM_HIP(ctx, l->d_rec.reserve(total));
  int rc = hs_pinned_reserve(ctx, &l->h_rec, &l->h_rec_cap, total);
  if (rc) return rc;
  const size_t o_first = 3 * total, o_active = o_first + total, aux_words = o_active + (total + 3) / 4;
  LSLAM_HIP(ctx, l->d_aux.reserve(aux_words));
  rc = hs_pinned_reserve(ctx, &l->h_aux, &l->h_aux_cap, aux_words);
  if (rc) return rc;
  if (!container_form) {
    LSLAM_HIP(ctx, l->d_cont.reserve((size_t)chunk * R * (size_t)std::max(c.capacity, 1) * 2));
    LSLAM_HIP(ctx, l->d_counts.reserve(total));
  }
  // ---- the trackers' state and the per-entry words up
  LSLAM_HIP(ctx, hipMemcpyAsync(l->d_state, l->h_state, (size_t)R * sizeof(HlTracker), hipMemcpyHostToDevice, ctx->stream));
  if (c.hints) memcpy(l->h_aux, c.hints, 3 * total * sizeof(float));
  if (container_form) {
    int32_t* first = reinterpret_cast<int32_t*>(l->h_aux + o_first);
    size_t at = 0;
    for (size_t i = 0; i < total; i++) {
      first[i] = (int32_t)at;
      at += (size_t)c.n_points[i];
    }
  }
  if (c.active) memcpy(l->h_aux + o_active, c.active, total);
  LSLAM_HIP(ctx, hipMemcpyAsync(l->d_aux.p, l->h_aux, aux_words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  const float* d_hints = c.hints ? reinterpret_cast<const float*>(l->d_aux.p) : nullptr;
  const int* d_first = container_form ? reinterpret_cast<const int*>(l->d_aux.p + o_first) : nullptr;
  const uint8_t* d_active = c.active ? reinterpret_cast<const uint8_t*>(l->d_aux.p + o_active) : nullptr;
  const GnLevels lv = gn_levels_of(map);
  // the matcher's form from the CALL's capacity and the map's LSLAM_GN_THREADS, as the streamed processor chooses it
  const GnForm form = gn_form_of(map, c.capacity);
  ProjectCfg pc{};
  if (!container_form) pc = project_cfg(map, c.capacity, c.scan);
  for (int k0 = 0; k0 < c.n_steps; k0 += chunk) {
    const size_t e0 = (size_t)k0 * R;
    HlCall d{};
    d.R = R;
    d.n_steps = std::min(chunk, c.n_steps - k0);
    d.capacity = c.capacity;
    d.active = d_active ? d_active + e0 : nullptr;
    d.take = c.d_take ? c.d_take + e0 * (size_t)c.take_stride : nullptr;
    d.take_stride = c.take_stride;
    d.hints = d_hints ? d_hints + 3 * e0 : nullptr;
    d.pts = container_form ? l->in.d_in.p : l->d_cont.p;
    d.first = d_first ? d_first + e0 : nullptr;
    d.counts = (container_form ? l->in.d_counts.p : l->d_counts.p) + e0;
    d.state = l->d_state;
    d.rec = l->d_rec.p + e0;
    if (!container_form) {
      HlSource s{};
      s.ranges = c.d_ranges ? c.d_ranges + e0 * (size_t)c.capacity : nullptr;
      s.cossin = l->d_cossin.p;
      s.xyz = c.d_xyz ? c.d_xyz + 3 * e0 * (size_t)c.capacity : nullptr;
      s.valid = c.d_valid ? c.d_valid + e0 * (size_t)c.capacity : nullptr;
      s.cont = l->d_cont.p;
      s.counts = l->d_counts.p + e0;
      launch(ctx, "hl_container", k_hl_container, dim3((unsigned)((size_t)d.n_steps * R)), dim3(1024), 0, pc, d, s);
      l->n_launches++;
    }
#define LSLAM_HL_REG(NT, PMAX) launch(ctx, "hl_track", k_hl_track_reg<NT, PMAX>, dim3(R), dim3(NT), form.lds, lv, d)
#define LSLAM_HL_FAST(NT) launch(ctx, "hl_track", k_hl_track_fast<NT>, dim3(R), dim3(NT), form.lds, lv, d, form.in_lds)
    LSLAM_GN_DISPATCH(form, LSLAM_HL_REG, LSLAM_HL_FAST);
#undef LSLAM_HL_REG
#undef LSLAM_HL_FAST
    l->n_launches++;
    l->n_track_launches++;
  }
  LSLAM_HIP(ctx, hipGetLastError());
  // ---- end of the call: the records and the state down, ONE wait
  LSLAM_HIP(ctx, hipMemcpyAsync(l->h_rec, l->d_rec.p, total * sizeof(lslam_hector_record), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipMemcpyAsync(l->h_state, l->d_state, (size_t)R * sizeof(HlTracker), hipMemcpyDeviceToHost, ctx->stream));
  LSLAM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  l->n_syncs++;
  l->n_calls++;
  l->n_steps += c.n_steps;
  for (size_t i = 0; i < total; i++) l->n_matched += l->h_rec[i].n_points >= 0;
  if (c.out) memcpy(c.out, l->h_rec, total * sizeof(lslam_hector_record));
  return LSLAM_OK;
}

}  // namespace

extern "C" {

int lslam_hector_loc_create(lslam_map* map, int n_trackers, lslam_hector_loc** out) {
  if (!map || !out || n_trackers < 1) return LSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  lslam_context* ctx = map->ctx;
  if (n_trackers > kHlMaxTrackers)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_loc_create: at most %d trackers (got %d)", kHlMaxTrackers, n_trackers);
  if (map->ordered_sums)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_loc_create: the localiser runs the parallel-sum matcher; this is an "
                     "LSLAM_MAP_OPT_ORDERED_SUMS map");
  if ((int)map->levels.size() > kGnMaxLevels)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "lslam_hector_loc_create: at most %d pyramid levels", kGnMaxLevels);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  lslam_hector_loc* l = new lslam_hector_loc();
  l->map = map;
  l->R = n_trackers;
  const size_t R = (size_t)n_trackers;
  if (hipMalloc((void**)&l->d_state, R * sizeof(HlTracker)) != hipSuccess ||
      hipHostMalloc((void**)&l->h_state, R * sizeof(HlTracker), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    lslam_hector_loc_destroy(l);
    return ctx->fail(LSLAM_ERR_HIP, "cannot allocate the localiser's state blocks");
  }
  memset(l->h_state, 0, R * sizeof(HlTracker));
  *out = l;
  return LSLAM_OK;
}

void lslam_hector_loc_destroy(lslam_hector_loc* l) {
  if (!l) return;
  (void)hipSetDevice(l->map->ctx->device);
  (void)hipStreamSynchronize(l->map->ctx->stream);
  if (l->d_state) (void)hipFree(l->d_state);
  if (l->h_state) (void)hipHostFree(l->h_state);
  if (l->h_aux) (void)hipHostFree(l->h_aux);
  if (l->h_rec) (void)hipHostFree(l->h_rec);
  l->in.release();
  l->d_aux.release();
  l->d_cont.release();
  l->d_counts.release();
  l->d_rec.release();
  l->d_cossin.release();
  delete l;
}

int lslam_hector_loc_size(const lslam_hector_loc* l) { return l ? l->R : LSLAM_ERR_INVALID_ARGUMENT; }

int lslam_hector_loc_set_poses(lslam_hector_loc* l, int first, int count, const float* poses_xyh) {
  if (!l || first < 0 || count < 0 || first > l->R || count > l->R - first || (count > 0 && !poses_xyh))
    return LSLAM_ERR_INVALID_ARGUMENT;
  for (int t = 0; t < count; t++) memcpy(l->h_state[first + t].pose, poses_xyh + 3 * t, 3 * sizeof(float));
  return LSLAM_OK;
}

int lslam_hector_loc_state(lslam_hector_loc* l, int tracker, float pose[3], float cov[9]) {
  if (!l || tracker < 0 || tracker >= l->R) return LSLAM_ERR_INVALID_ARGUMENT;
  if (pose) memcpy(pose, l->h_state[tracker].pose, 3 * sizeof(float));
  if (cov) memcpy(cov, l->h_state[tracker].cov, 9 * sizeof(float));
  return LSLAM_OK;
}

int lslam_hector_loc_set_option(lslam_hector_loc* l, int option, int value) {
  if (!l) return LSLAM_ERR_INVALID_ARGUMENT;
  if (option == LSLAM_HECTOR_LOC_OPT_MAX_STEPS_PER_LAUNCH) {
    if (value < 0) return l->map->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "steps per launch must be >= 0 (0 = the default)");
    l->max_steps = value;
    return LSLAM_OK;
  }
  return l->map->ctx->fail(LSLAM_ERR_INVALID_ARGUMENT, "unknown localiser option %d", option);
}

int lslam_hector_loc_process_many(lslam_hector_loc* l, const lslam_hector_scan* scan, int n_steps, int n_readings,
                                  const float* ranges, int ranges_stride, const float* pose_hints, const uint8_t* active,
                                  lslam_hector_record* out) {
  if (!l || n_steps < 0 || n_readings < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!scan || n_readings < 1 || !ranges || ranges_stride < n_readings) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = l->map->ctx;
  const char* who = "lslam_hector_loc_process_many";
  int rc = hl_check(l, who, n_readings);
  if (rc) return rc;
  const size_t rows = (size_t)n_steps * (size_t)l->R;
  if (rows * (size_t)n_readings > (size_t)INT32_MAX / 2) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: call too large", who);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hl_ensure_cossin(l, n_readings, scan);  // (waits for its upload when the scan geometry is new)
  if (rc) return rc;
  rc = hs_stage_ranges(ctx, l->in, rows, n_readings, ranges, (size_t)ranges_stride);
  if (rc) return rc;
  HlRun c;
  c.n_steps = n_steps;
  c.capacity = n_readings;
  c.scan = scan;
  c.d_ranges = l->in.d_in.p;
  c.hints = pose_hints;
  c.active = active;
  c.out = out;
  return hl_run(l, c);
}

int lslam_hector_loc_process_many_points(lslam_hector_loc* l, int n_steps, const float* points_xy, const int32_t* n_points,
                                         const float* pose_hints, const uint8_t* active, lslam_hector_record* out) {
  if (!l || n_steps < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!n_points) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = l->map->ctx;
  const char* who = "lslam_hector_loc_process_many_points";
  const size_t rows = (size_t)n_steps * (size_t)l->R;
  size_t total = 0;
  int cap = 0;
  int rc = hs_check_counts(ctx, who, rows, n_points, active, points_xy, &total, &cap);
  if (!rc) rc = hl_check(l, who, cap);
  if (rc) return rc;
  if (total > (size_t)INT32_MAX / 2) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: call too large", who);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_stage_points(ctx, l->in, l->in.d_in, rows, points_xy, n_points, total);
  if (rc) return rc;
  HlRun c;
  c.n_steps = n_steps;
  c.capacity = cap;
  c.n_points = n_points;
  c.hints = pose_hints;
  c.active = active;
  c.out = out;
  return hl_run(l, c);
}

int lslam_hector_loc_process_many_clouds_dev(lslam_hector_loc* l, const lslam_hector_scan* scan, int n_steps, int n_points,
                                             const float* xyz_dev, const uint8_t* valid_dev, const int32_t* take_dev,
                                             int take_stride, const float* pose_hints, const uint8_t* active,
                                             lslam_hector_record* out) {
  if (!l || n_steps < 0 || n_points < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!scan || (n_points > 0 && !xyz_dev) || (take_dev && take_stride < 1)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = l->map->ctx;
  const char* who = "lslam_hector_loc_process_many_clouds";
  int rc = hl_check(l, who, n_points);
  if (rc) return rc;
  if ((size_t)n_steps * (size_t)l->R * (size_t)n_points > (size_t)INT32_MAX / 4)
    return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: call too large", who);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  HlRun c;
  c.n_steps = n_steps;
  c.capacity = n_points;
  c.scan = scan;
  c.d_xyz = xyz_dev;
  c.d_valid = valid_dev;
  c.d_take = take_dev;
  c.take_stride = take_dev ? take_stride : 0;
  c.hints = pose_hints;
  c.active = active;
  c.out = out;
  return hl_run(l, c);
}

int lslam_hector_loc_process_many_clouds(lslam_hector_loc* l, const lslam_hector_scan* scan, int n_steps, int n_points,
                                         const float* xyz, const uint8_t* valid, const uint8_t* take, const float* pose_hints,
                                         const uint8_t* active, lslam_hector_record* out) {
  if (!l || n_steps < 0 || n_points < 0) return LSLAM_ERR_INVALID_ARGUMENT;
  if (n_steps == 0) return LSLAM_OK;
  if (!scan || (n_points > 0 && !xyz)) return LSLAM_ERR_INVALID_ARGUMENT;
  lslam_context* ctx = l->map->ctx;
  const char* who = "lslam_hector_loc_process_many_clouds";
  int rc = hl_check(l, who, n_points);
  if (rc) return rc;
  const size_t rows = (size_t)n_steps * (size_t)l->R;
  if (rows * (size_t)n_points > (size_t)INT32_MAX / 4) return ctx->fail(LSLAM_ERR_UNSUPPORTED, "%s: call too large", who);
  LSLAM_HIP(ctx, hipSetDevice(ctx->device));
  rc = hs_stage_clouds(ctx, l->in, rows, n_points, xyz, valid, take);
  if (rc) return rc;
  return lslam_hector_loc_process_many_clouds_dev(l, scan, n_steps, n_points, l->in.d_xyz.p,
                                                  valid ? l->in.d_valid.p : (const uint8_t*)nullptr,
                                                  take ? l->in.d_take.p : (const int32_t*)nullptr, 1, pose_hints, active, out);
}

int lslam_hector_loc_stats(const lslam_hector_loc* l, int64_t out[6]) {
  if (!l || !out) return LSLAM_ERR_INVALID_ARGUMENT;
  out[0] = l->n_steps; out[1] = l->n_matched; out[2] = l->n_calls; out[3] = l->n_syncs; out[4] = l->n_launches;
  out[5] = l->n_track_launches;
  return LSLAM_OK;
}

}  // extern "C"
