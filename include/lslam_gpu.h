/*
 * lslam_gpu.h -- C ABI of the MI355X-native 2-D laser SLAM front-end hot path
 * (Karto-style correlative scan matcher + Hector-style Bresenham log-odds grid update).
 *
 * This is the drop-in boundary.  The reference (xiangli0608/Creating-2D-laser-slam-from-scratch)
 * has no FFI for this path -- its seams are C++ classes -- so every entry point below names the
 * reference interface it stands in for (file:line relative to the reference repo; short names:
 *   Mapper.h/Karto.h = lesson6/lib/open_karto/include/open_karto/..., Mapper.cpp = .../src/Mapper.cpp,
 *   H/ = lesson4/include/lesson4/hector_mapping/).
 * INTEGRATION.md shows the adapter a maintainer of the reference would add on top of it.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.  Opaque handles.
 *  - Every call returns LSLAM_OK (0) or a negative lslam_status; lslam_last_error() gives text.
 *    No exception ever crosses the boundary (the reference throws karto::Exception /
 *    std::runtime_error, Mapper.cpp:444-447,484-487, Karto.h:4488-4499; those surface as
 *    per-scan `status` in lslam_match_result or as the call's return code).
 *  - Poses are (x [m], y [m], heading [rad]).  Matcher poses are SENSOR poses
 *    (LocalizedRangeScan::GetSensorPose, Karto.h:5280); lslam_sensor_pose_from_robot /
 *    lslam_robot_pose_from_sensor convert (Karto.h:5289-5313).
 *  - "host" entry points take host pointers and are synchronous.  "_dev" entry points take
 *    device (HBM) pointers, only enqueue work on the context's HIP stream and return; use
 *    lslam_synchronize() or your own event on lslam_stream().
 *  - A context is bound to one GPU and is not thread-safe, like the reference's matcher
 *    (one grid + one lookup per ScanMatcher instance, Mapper.h:1273-1278).
 *  - There is NO CPU fallback: without a usable gfx950 device lslam_create fails.
 */
#ifndef LSLAM_GPU_H
#define LSLAM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSLAM_ABI_VERSION 5

typedef enum lslam_status {
  LSLAM_OK = 0,
  LSLAM_ERR_INVALID_ARGUMENT = -1, /* ScanMatcher::Create returning NULL (Mapper.cpp:130-145) */
  LSLAM_ERR_NO_DEVICE = -2,
  LSLAM_ERR_INDEX_OUT_OF_RANGE = -3,  /* karto::Exception from Grid::GridIndex (Karto.h:4488-4499) */
  LSLAM_ERR_PROBABILITY_SEARCH = -4,  /* "Index out of range in probability search" (Mapper.cpp:444-447) */
  LSLAM_ERR_NO_BEST_POSE = -5,        /* "Unable to find best position" (Mapper.cpp:484-487) */
  LSLAM_ERR_HIP = -6,
  LSLAM_ERR_SMEAR_DEVIATION = -7,     /* CalculateKernel range check (Mapper.h:1041-1053) */
  LSLAM_ERR_UNSUPPORTED = -8,
  LSLAM_ERR_NO_DATA = -9              /* a diagnostic was read before anything had been collected for it */
} lslam_status;

typedef struct lslam_context lslam_context;
typedef struct lslam_matcher lslam_matcher;
typedef struct lslam_map lslam_map;

/* ---------------------------------------------------------------------------------------- */
/* context                                                                                  */
/* ---------------------------------------------------------------------------------------- */
int lslam_abi_version(void);
/* device = HIP device ordinal.  Fails (LSLAM_ERR_NO_DEVICE) if no GPU is visible. */
int lslam_create(int device, lslam_context** out);
void lslam_destroy(lslam_context* ctx);
const char* lslam_last_error(const lslam_context* ctx); /* ctx may be NULL: last global error */
int lslam_synchronize(lslam_context* ctx);
void* lslam_stream(lslam_context* ctx); /* the hipStream_t all work of this context runs on */
/* device memory helpers for callers without their own allocator (bench / tests) */
int lslam_dev_alloc(lslam_context* ctx, size_t bytes, void** out);
int lslam_dev_free(lslam_context* ctx, void* p);
int lslam_dev_upload(lslam_context* ctx, void* dst_dev, const void* src_host, size_t bytes);
int lslam_dev_download(lslam_context* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* per-kernel HIP-event timing of subsequent calls (bench.py's roofline numbers).
 * lslam_profile_read returns the number of records written: name (<=31 chars), launches, total ms */
typedef struct lslam_kernel_time {
  char name[32];
  int64_t launches;
  double total_ms;
} lslam_kernel_time;
/* Diagnostics: 256 samples {where + 1, shader-clock ticks (s_memtime), 100 MHz ticks (s_memrealtime)} from 256 single-wave
 * blocks; `where` = XCD << 16 | shader engine / array / CU bits of HW_ID; 0 = that block did not report.  Two calls around a timed
 * region give the clock it ran at -- (t1 - t0) / ((r1 - r0) / 1e8), taken per CU present in both samples, so that nothing depends
 * on whether the counters of different CUs agree.  Synchronises the context stream.  (bench.py prices cycles with it.) */
int lslam_clock_sample(lslam_context* ctx, uint64_t out[768]);
int lslam_profile_enable(lslam_context* ctx, int on);
/* restrict the timing to kernels launched under this name (NULL or "" = every kernel): two events per
 * launch cost ~3 us of stream time, which matters when a batch is five kernels */
int lslam_profile_only(lslam_context* ctx, const char* kernel_name);
int lslam_profile_reset(lslam_context* ctx);
int lslam_profile_read(lslam_context* ctx, lslam_kernel_time* out, int capacity);

/* ---------------------------------------------------------------------------------------- */
/* Karto correlative scan matcher  (replaces karto::ScanMatcher, Mapper.h:1127-1279)        */
/* ---------------------------------------------------------------------------------------- */
typedef struct lslam_matcher_config {
  double search_size;                /* ScanMatcher::Create searchSize   (Mapper.h:1139-1143) */
  double resolution;                 /*                      resolution                        */
  double smear_deviation;            /*                      smearDeviation                    */
  double range_threshold;            /*                      rangeThreshold                    */
  /* the Mapper parameters the matcher reads through friend access (Mapper.cpp:206,238-256,
   * 279-280,405-411).  The two variance penalties are VARIANCES: Mapper::setParam*VariancePenalty
   * squares what the ROS node passes (Mapper.cpp:1919-1927). */
  double coarse_search_angle_offset; /* m_pCoarseSearchAngleOffset */
  double coarse_angle_resolution;    /* m_pCoarseAngleResolution   */
  double fine_search_angle_offset;   /* m_pFineSearchAngleOffset   */
  double distance_variance_penalty;  /* m_pDistanceVariancePenalty */
  double angle_variance_penalty;     /* m_pAngleVariancePenalty    */
  double minimum_distance_penalty;   /* m_pMinimumDistancePenalty  */
  double minimum_angle_penalty;      /* m_pMinimumAnglePenalty     */
  int32_t use_response_expansion;    /* m_pUseResponseExpansion    */
  int32_t reserved;
} lslam_matcher_config;

/* karto::LaserRangeFinder parameters the hot path reads (Karto.h:4127-4137, karto_slam.cc:384-395) */
typedef struct lslam_laser {
  double minimum_angle, maximum_angle, angular_resolution;
  double minimum_range, maximum_range, range_threshold;
  double offset_x, offset_y, offset_heading; /* Sensor::SetOffsetPose (karto_slam.cc:387-389) */
} lslam_laser;

/* Pose2 mean + response + Matrix3 covariance of one match (Mapper.h:1155-1159): 104 B padded to 112 */
typedef struct lslam_match_result {
  double pose[3];       /* rMean: best SENSOR pose */
  double response;      /* return value of MatchScan, in [0,1] */
  double covariance[9]; /* rCovariance, row-major 3x3 */
  int32_t status;       /* LSLAM_OK or the lslam_status the reference would have thrown */
  int32_t flags;        /* bit0: response expansion was used */
} lslam_match_result;

/* default parameters of the library (Mapper.cpp:1572-1647) */
void lslam_matcher_config_defaults(lslam_matcher_config* cfg);

/* ScanMatcher::Create (Mapper.h:1139-1143, Mapper.cpp:126-172): allocates the correlation grid,
 * smear kernel and workspaces in HBM.  Invalid parameters -> LSLAM_ERR_INVALID_ARGUMENT (the
 * reference returns NULL) / LSLAM_ERR_SMEAR_DEVIATION (the reference throws). */
int lslam_matcher_create(lslam_context* ctx, const lslam_matcher_config* cfg,
                         const lslam_laser* laser, lslam_matcher** out);
void lslam_matcher_destroy(lslam_matcher* m); /* ~ScanMatcher (Mapper.cpp:119-124) */

/* LaserRangeFinder::GetNumberOfRangeReadings (Karto.h:4152-4161): round((max-min)/res), no +1 */
int lslam_matcher_num_beams(const lslam_matcher* m);
/* GetCorrelationGrid() geometry (Mapper.h:1226): out[8] = width,height,widthStep,roi_x,roi_y,
 * roi_w,roi_h,kernel_size ; offset_xy = CoordinateConverter offset of the current grid */
int lslam_matcher_grid_info(const lslam_matcher* m, int32_t out[8], double offset_xy[2]);
/* GetCorrelationGrid()->GetDataPointer() contents: height*widthStep bytes */
int lslam_matcher_get_grid_u8(lslam_matcher* m, uint8_t* out_host);
int lslam_matcher_get_kernel_u8(lslam_matcher* m, uint8_t* out_host);
/* shared-grid mode: install a prebuilt correlation grid (same geometry) + its offset */
int lslam_matcher_set_grid_u8(lslam_matcher* m, const uint8_t* grid_host, const double offset_xy[2]);
/* same, from a device buffer (used to replicate one rank's grid after an RCCL broadcast) */
int lslam_matcher_set_grid_u8_dev(lslam_matcher* m, const uint8_t* grid_dev, const double offset_xy[2]);
/* device address of the grid bytes (height*widthStep), e.g. as an RCCL broadcast buffer */
void* lslam_matcher_grid_dev_ptr(lslam_matcher* m);

/* Tuning / diagnostics switches; none of them changes a result.
 *  LSLAM_OPT_ROW_OCCUPANCY (default 1): exact zero-row pruning of the coarse pass.  0 = every in-range lattice row
 *    of every beam is gathered -- the worst case over world sparsity (bench.py reports both step times).
 *  LSLAM_OPT_COLLECT_STATS (default 0): 1 clears the counters and routes coarse passes through an instrumented twin of
 *    the hot kernel (slower: for an untimed diagnostic launch); lslam_matcher_read_stats then returns, summed over
 *    the passes since: [0] lattice rows inside the reference's index range (Mapper.cpp:841-845), [1] rows still live
 *    after pruning, [2] readable beam x angle pairs, [3] those with at least one live row.  The kernel takes a lattice in
 *    blocks of 11 rows (lattice rows of up to 12 positions) or 8 rows (13..16 positions) and visits every beam once per
 *    block: on a lattice with more rows than one block holds, [2] and [3] count beam x angle x row-block triples
 *    (16 x 16 x 21: every readable pair twice in [2]; in [3] once per block in which it has a live row). */
/*  LSLAM_OPT_LDS_STAGED (default 0): 1 routes the coarse pass of chip-filling batches through the LDS-staged variant of
 *    the hot kernel (phase B reads its rows from per-drain patches of the parity planes staged in LDS): an experiment that
 *    was measured and dropped (DESIGN_HISTORY.md B, "LDS-staged experiment"), kept selectable so the measurement can be repeated. */
/*  LSLAM_OPT_PIPELINE_DEPTH (default 1; 1..4): with depth D > 1 consecutive lslam_matcher_match_batch_dev_* calls become
 *    PIPELINED STEPS: they take turns on D internal HIP streams, each with its own set of per-step workspaces, so that
 *    D steps share the chip: their response kernels fill each other's tails and their latency-bound prep / reduce
 *    kernels run side by side instead of one step after the other (what small per-GPU batches of a sharded run need:
 *    512 scans/step 0.118 -> 0.086 ms on one MI355X; DESIGN.md 6 has the timeline).  Same kernels, same arguments, byte-identical
 *    records.  A step is ordered behind everything the CONTEXT stream held when the call was made (inputs, grid
 *    changes) but not behind the steps before it; the context stream falls in behind all steps at the next
 *    lslam_synchronize / lslam_matcher_flush or any matcher entry point that touches the grid.  The caller's side of
 *    the contract: up to D steps are in flight at once, so D consecutive calls must not share an output buffer whose
 *    earlier contents are still wanted, and results are read after lslam_synchronize (or lslam_matcher_flush + work on
 *    the context stream).  lslam_matcher_match_batch (host arrays) splits its batch into up to D sub-batches of >= 256
 *    scans and pipelines those, uploads included; it returns with everything done, as before.  The reference has no
 *    counterpart: karto::ScanMatcher is one grid, one lookup table, one caller (Mapper.h:1273-1278). */
/*  LSLAM_OPT_CHECK_OUTPUT_REUSE (default 0; debug): with 1 a pipelined step whose result buffer overlaps the buffer of a
 *    step that may still be in flight returns LSLAM_ERR_INVALID_ARGUMENT instead of letting two steps write the same
 *    records (the caller's side of the LSLAM_OPT_PIPELINE_DEPTH contract, checked on the host: no device cost). */
/*  LSLAM_OPT_ROWS_WAVES (1, 2, 4 or 8; default 1): waves per block of the coarse response kernel of chip-filling batches.
 *    With W > 1 the W waves of a block take W consecutive candidate angles of ONE scan (k_resp_rows_mw), so they run on one
 *    CU and share its L1 (points, occupancy words, lines of the tiled planes); 1 = one wave per block (k_resp_rows).  Same
 *    numerators either way. */
/*  LSLAM_OPT_STEP_KERNEL (0, 3 or 4): ONE launch per batched match instead of five.  With 3 or 4 a workgroup of that
 *    many wave64s takes one scan through scan_prep -> coarse responses -> coarse reduce -> fine responses -> fine reduce
 *    (k_match_step: the same device functions in the same order, byte-identical records); the int32 response numerators
 *    stay in LDS and the latency-bound phases of one scan run under the gathers of the scans resident beside it.  Applies
 *    to batches of at least LSLAM_OPT_STEP_MIN_SCANS scans (default 64) whose configuration takes the tiled production
 *    kernels: no response expansion, refinement on, coarse lattice rows of 5..16 positions, the 3 x 3 fine lattice;
 *    everything else keeps the five-kernel path (value 0 = always).  lslam_matcher_step_kernel_launches counts the
 *    launches that did go out as one kernel.  The reference has no counterpart (Mapper.cpp:184-291 is one scan at a time). */
/*  LSLAM_OPT_LONE_KERNEL (0, 4, 8 or 16; default 0): the match of ONE scan (lslam_matcher_match_scan, the streaming
 *    front-end, a batch of one) as ONE launch instead of four: k_match_lone keeps the width of the chain -- one (angle, beam
 *    slice) task per wave, blocks of that many wave64s -- and replaces the launches between coarse responses, coarse reduce,
 *    fine responses and fine reduce by counters in device memory (the last block to arrive runs the reduce; the others wait,
 *    bounded, on one word).  Same device functions, same atomically accumulated integers: byte-identical records.  A hand-over
 *    that does not arrive within ~40 ms makes the record's status LSLAM_ERR_HIP; nothing hangs.  Measured: 3 us per scan SLOWER
 *    than the four launches (profiles/r06/experiments/README.md section 6), hence off by default; value + 100 = one task wave
 *    per block (the A/B form).  lslam_matcher_lone_kernel_launches counts the matches that did go out as one kernel.  The
 *    reference has no counterpart. */
/*  LSLAM_OPT_ROWS_MFMA (default 1): the coarse response kernel (k_resp_rows / k_resp_rows_mw, lattice rows of 5..16
 *    positions, the instrumented twins included) sums the bytes of its queued rows with v_mfma_i32_16x16x64_i8 -- the
 *    lane's 16 candidate bytes against a one-hot operand, int32 accumulators -- instead of packed 16-bit fields on the
 *    VALU.  The instruction reads the bytes SIGNED, so the form is taken only while every byte of the grid is <= 127:
 *    always for a grid the library builds (<= 100), after lslam_matcher_set_grid_u8 if its host copy says so, never after
 *    lslam_matcher_set_grid_u8_dev (bytes the host has not seen); any other grid, and value 0, runs the packed form.  Same
 *    numerators either way; the launches are counted under the same form names, and lslam_matcher_rows_mfma_launches
 *    counts those that took the MFMA accumulate.  The one-launch kernels (LSLAM_OPT_STEP_KERNEL / LSLAM_OPT_LONE_KERNEL),
 *    the LDS-staged experiment and rows of up to 4 positions keep the packed form. */
/*  LSLAM_OPT_FINE_MFMA (default 1): the fine response kernel on the 4x4 blocks (k_resp_tile3, batches whose fine pass fills
 *    the chip) sums the bytes of each beam's 3x3 patch with v_mfma_i32_16x16x64_i8 -- the three patch rows, shifted to the
 *    patch's column, against the same one-hot operand, one int32x4 accumulator per angle -- instead of v_perm_b32 selections
 *    into packed 16-bit fields and a DPP + v_readlane reduction per candidate.  A group's angles beyond the last fine angle
 *    cost nothing in this form.  Signed bytes again: taken under exactly the conditions of LSLAM_OPT_ROWS_MFMA (every byte of
 *    the grid <= 127 as far as the host knows), the packed form otherwise and for value 0.  Same numerators either way; the
 *    launches stay under the form name fine_tile3 and the profile name resp_tile_fine, and
 *    lslam_matcher_fine_mfma_launches counts those that summed on the matrix pipe.  The one-launch kernels keep the packed
 *    form. */
enum { LSLAM_OPT_ROW_OCCUPANCY = 1, LSLAM_OPT_COLLECT_STATS = 2, LSLAM_OPT_LDS_STAGED = 3, LSLAM_OPT_PIPELINE_DEPTH = 4,
       LSLAM_OPT_STEP_KERNEL = 5, LSLAM_OPT_STEP_MIN_SCANS = 6, LSLAM_OPT_ROWS_WAVES = 7, LSLAM_OPT_CHECK_OUTPUT_REUSE = 8, LSLAM_OPT_LONE_KERNEL = 9,
       LSLAM_OPT_ROWS_MFMA = 10, LSLAM_OPT_FINE_MFMA = 11 };
/* current value of an option (negative: error code) */
int lslam_matcher_get_option(const lslam_matcher* m, int option);
/* Order the context stream behind every pipelined step in flight (no host wait).  No-op at depth 1. */
int lslam_matcher_flush(lslam_matcher* m);
/* diagnostics: pipelined steps enqueued so far (0 while LSLAM_OPT_PIPELINE_DEPTH is 1) */
int64_t lslam_matcher_pipelined_steps(const lslam_matcher* m);
/* diagnostics: batched matches that went out as ONE launch (LSLAM_OPT_STEP_KERNEL) so far */
int64_t lslam_matcher_step_kernel_launches(const lslam_matcher* m);
/* diagnostics: single-scan matches that went out as ONE launch (LSLAM_OPT_LONE_KERNEL) so far */
int64_t lslam_matcher_lone_kernel_launches(const lslam_matcher* m);
/* diagnostics: k_resp_rows / k_resp_rows_mw launches that took the MFMA accumulate (LSLAM_OPT_ROWS_MFMA) so far */
int64_t lslam_matcher_rows_mfma_launches(const lslam_matcher* m);
/* diagnostics: k_resp_tile3 launches that summed on the matrix pipe (LSLAM_OPT_FINE_MFMA) so far */
int64_t lslam_matcher_fine_mfma_launches(const lslam_matcher* m);
/* diagnostics: which FORM of the response kernel took the passes of the matches so far.  Every coarse form goes out under
 * the same profile name (resp_rows_coarse), and the dispatch falls back silently (a batch below the tiled planes' threshold,
 * more than 2048 beams, planes that could not be allocated ...): a test or an A/B run that selects a form with
 * lslam_matcher_set_option reads here whether that form really ran.  One count per launch, kept on the host (no device cost);
 * matches that went out as ONE kernel (LSLAM_OPT_STEP_KERNEL / LSLAM_OPT_LONE_KERNEL) are counted by the two functions above
 * instead.  Coarse passes (expansion passes included):
 *   GENERIC                k_resp_generic: a lattice outside the packed kernels, or forced (either pass)
 *   ROWS_LINEAR            k_resp_rows on the linear parity planes (small batches: beam slices)
 *   ROWS_TILED             k_resp_rows on the tiled parity planes (chip-filling batches; the hot kernel)
 *   ROWS_MULTIWAVE         k_resp_rows_mw (LSLAM_OPT_ROWS_WAVES 2 / 4 / 8)
 *   ROWS_LDS_STAGED        k_resp_rows, phase B through LDS patches of the linear planes (LSLAM_OPT_LDS_STAGED)
 *   ROWS_STATS_LINEAR / ROWS_STATS_TILED / ROWS_STATS_LDS_STAGED   the instrumented twins (LSLAM_OPT_COLLECT_STATS) of the three
 *   BIG                    k_resp_dense (loop-closure-size lattices)
 * and the fine pass: FINE_ROWS (k_resp_rows on the grid itself), FINE_TILE3 (k_resp_tile3 on the 4x4 blocks). */
enum { LSLAM_FORM_GENERIC = 0, LSLAM_FORM_ROWS_LINEAR = 1, LSLAM_FORM_ROWS_TILED = 2, LSLAM_FORM_ROWS_MULTIWAVE = 3,
       LSLAM_FORM_ROWS_LDS_STAGED = 4, LSLAM_FORM_ROWS_STATS_LINEAR = 5, LSLAM_FORM_ROWS_STATS_TILED = 6,
       LSLAM_FORM_ROWS_STATS_LDS_STAGED = 7, LSLAM_FORM_BIG = 8, LSLAM_FORM_FINE_ROWS = 9, LSLAM_FORM_FINE_TILE3 = 10,
       LSLAM_FORM_COUNT = 11 };
int lslam_matcher_coarse_form_launches(const lslam_matcher* m, int64_t out[LSLAM_FORM_COUNT]);
/* diagnostics: k_match_lone's hand-over words, 16 slots x 8 words {coarse tickets, coarse done, fine ready, fine tickets,
 * fine done, timeouts, 0, 0}; LSLAM_ERR_NO_DATA before the first such launch */
int lslam_debug_lone_sync(lslam_matcher* m, unsigned* out128);
/* diagnostics, no device needed: the dynamic LDS bytes one block of the coarse reduce (k_reduce_coarse_lds) is launched with
 * for this configuration's coarse lattice, in its 128-, 256- or 1024-thread form; dims (optional) = the lattice {nX, nY, nA}.
 * Together with the kernel's static LDS this is what decides how many blocks a CU holds.  -1 for anything else. */
int lslam_debug_reduce_lds_bytes(const lslam_matcher_config* cfg, int threads, int dims[3]);
int lslam_matcher_set_option(lslam_matcher* m, int option, int value);
int lslam_matcher_read_stats(lslam_matcher* m, uint64_t out[4]);
/* after an instrumented pass: out[0] = readable (scan, beam) pairs of that batch, out[1] = those with a live lattice row in
 * AT LEAST ONE of the scan's coarse angles (a beam outside out[1] contributes nothing to any candidate of its scan);
 * out[2], out[3] = with LSLAM_OPT_LDS_STAGED: drains of 64 queued beams whose patches fit LDS / that took the global path */
int lslam_matcher_read_beam_stats(lslam_matcher* m, uint64_t out[4]);

/* LocalizedRangeScan::GetSensorAt / SetSensorPose (Karto.h:5280-5313), host-side, double */
void lslam_sensor_pose_from_robot(const lslam_laser* laser, const double robot[3], double sensor[3]);
void lslam_robot_pose_from_sensor(const lslam_laser* laser, const double sensor[3], double robot[3]);

/* MatchScan steps 1-4 + AddScans (Mapper.cpp:212-225,699-748): recentre the grid on
 * center_pose, clear it, rasterise + smear the valid points (FindValidPoints, :756-811, viewpoint =
 * center position) of n_scans base scans.  ranges: n_scans rows of `ranges_stride` doubles
 * (>= num_beams used), sensor_poses: n_scans*3. */
int lslam_matcher_set_base_scans(lslam_matcher* m, int n_scans, const double* ranges,
                                 int ranges_stride, const double* sensor_poses,
                                 const double center_pose[3]);

/* ScanMatcher::MatchScan (Mapper.h:1155-1159, Mapper.cpp:184-291), complete: rebuild the grid
 * from the base scans around the query's sensor pose, coarse + (expansion) + fine search. */
int lslam_matcher_match_scan(lslam_matcher* m, int n_base, const double* base_ranges,
                             int ranges_stride, const double* base_sensor_poses,
                             const double* query_ranges, const double query_sensor_pose[3],
                             int do_penalize, int do_refine, lslam_match_result* out);

/* The search part of MatchScan (Mapper.cpp:227-290 = CorrelateScan coarse/expansion/fine,
 * Mapper.h:1177-1186) for n_scans INDEPENDENT scans against the CURRENT grid (batched
 * many-scan mode; n_scans = 1 is the single-scan case).  Host pointers, synchronous. */
int lslam_matcher_match_batch(lslam_matcher* m, int n_scans, const double* ranges,
                              int ranges_stride, const double* sensor_poses, int do_penalize,
                              int do_refine, lslam_match_result* out);
/* Same with everything resident in HBM: float32 ranges exactly as a sensor_msgs/LaserScan
 * carries them (widened to double on the device like karto_slam.cc:428-433), results written
 * to out_dev.  Asynchronous on the context stream. */
int lslam_matcher_match_batch_dev_f32(lslam_matcher* m, int n_scans, const float* ranges_dev,
                                      int ranges_stride, const double* sensor_poses_dev,
                                      int do_penalize, int do_refine,
                                      lslam_match_result* out_dev);
int lslam_matcher_match_batch_dev_f64(lslam_matcher* m, int n_scans, const double* ranges_dev,
                                      int ranges_stride, const double* sensor_poses_dev,
                                      int do_penalize, int do_refine,
                                      lslam_match_result* out_dev);

/* ---- device-side scan cache behind seam B1 -------------------------------------------------------------------------
 * karto::ScanMatcher::MatchScan (Mapper.h:1155-1159) is handed its base scans as a LocalizedRangeScanVector on every
 * call: the running window (Mapper.cpp:2040), near chains (:942, :1140), loop chains (:991, :1015).  A scan's readings
 * never change and its pose changes about once in its life (when its own match is accepted, Mapper.cpp:2040-2044, or a
 * closed loop re-poses it), so re-sending ~70 x 8.6 KB per call -- what lslam_matcher_match_scan's literal signature
 * costs -- is avoidable: the cache keeps a scan's readings, its world points and the anchor chain of FindValidPoints
 * (Mapper.cpp:756-811) resident in HBM under an id the CALLER chooses (integration/karto_scan_matcher_gpu.cpp numbers the
 * LocalizedRangeScan objects it meets).  One cache serves every matcher of its context that was created for the same
 * laser (the sequential and the loop matcher of one Mapper).  Not thread-safe, like the matcher. */
typedef struct lslam_scan_cache lslam_scan_cache;
int lslam_scan_cache_create(lslam_context* ctx, const lslam_laser* laser, lslam_scan_cache** out);
void lslam_scan_cache_destroy(lslam_scan_cache* cache);
/* readings of scan `scan_id` (>= 0; num_beams doubles, LocalizedRangeScan::GetRangeReadings) into HBM; an id that is
 * already cached is overwritten.  The caller's buffer is free again on return. */
int lslam_scan_cache_put(lslam_scan_cache* cache, int64_t scan_id, const double* ranges);
int lslam_scan_cache_contains(const lslam_scan_cache* cache, int64_t scan_id); /* 1 / 0 */
int lslam_scan_cache_forget(lslam_scan_cache* cache, int64_t scan_id);         /* scan_id < 0: every scan */
int lslam_scan_cache_size(const lslam_scan_cache* cache);
/* World points + FindValidPoints anchors of cached scan `scan_id` at `sensor_pose`, ENQUEUED on the context stream (returns
 * at once): for a caller that knows -- or can guess -- the pose a scan will have when it is next named as a base scan
 * (integration/karto_scan_matcher_gpu.cpp: the pose AddEdges gives the scan Mapper::Process has just matched, Mapper.cpp:
 * 930-973), so that the preparation runs beside the caller's host code instead of in front of its next match.  A guess
 * that turns out wrong costs nothing but the refresh it would have saved. */
int lslam_scan_cache_prepare(lslam_scan_cache* cache, int64_t scan_id, const double sensor_pose[3]);
/* out[5] = matches served, scans uploaded, (scan, pose) refreshes (world points + anchors recomputed because the pose
 * differed bitwise from the cached one), speculative refreshes (below), bytes of HBM held */
int lslam_scan_cache_counters(const lslam_scan_cache* cache, int64_t out[5]);
/* flags of lslam_matcher_match_scan_cached */
enum {
  LSLAM_MATCH_PENALIZE = 1, /* doPenalize */
  LSLAM_MATCH_REFINE = 2,   /* doRefineMatch */
  /* The caller will give the query scan the returned mean as its sensor pose (Mapper::Process: SetSensorPose(bestPose),
   * Mapper.cpp:2040-2044): its world points + anchors at that pose are computed BEHIND the match on the stream, and the
   * call returns as soon as the result record is on the host.  Purely a hint: a pose that turns out different is
   * refreshed again when the scan is next named as a base scan. */
  LSLAM_MATCH_QUERY_TAKES_RESULT_POSE = 4
};
/* ScanMatcher::MatchScan, complete (= lslam_matcher_match_scan, identical results), with the base scans named by id.
 * base_sensor_poses: n_base*3, the scans' CURRENT sensor poses (24 bytes per scan are all that cross the bus).
 * query_id >= 0 and cached: query_ranges may be NULL.  query_id >= 0 and not cached: query_ranges are uploaded INTO the
 * cache under that id (the scan the caller is about to add to its running window).  query_id < 0: anonymous query
 * (TryCloseLoop's temporary scan, Mapper.cpp:1008-1015), nothing is kept.  An unknown base id -> LSLAM_ERR_INVALID_ARGUMENT. */
int lslam_matcher_match_scan_cached(lslam_matcher* m, lslam_scan_cache* cache, int n_base, const int64_t* base_ids,
                                    const double* base_sensor_poses, int64_t query_id, const double* query_ranges,
                                    const double query_sensor_pose[3], int flags, lslam_match_result* out);

/* ---- inspection hooks used by the parity tests (intermediate state of the reference) ---- */
/* GridIndexLookup::ComputeOffsets (Karto.h:6409-6501) for one scan: out = n_angles*num_beams
 * int32 (INT_MAX = INVALID_SCAN); returns n_angles in *n_angles_out */
int lslam_matcher_debug_lookup_table(lslam_matcher* m, const double* ranges,
                                     const double sensor_pose[3], double angle_center,
                                     double angle_offset, double angle_resolution,
                                     int32_t* out_host, int* n_angles_out);
/* integer numerators of GetResponse (Mapper.cpp:819-856) over the COARSE lattice of one scan
 * against the current grid, order y,x,angle; returns counts through nx,ny,na */
int lslam_matcher_debug_coarse_sums(lslam_matcher* m, const double* ranges,
                                    const double sensor_pose[3], int32_t* out_host, int* nx,
                                    int* ny, int* na, int force_generic_kernel);
/* the same for a BATCH: the n_scans scans go through exactly the launches a coarse-only match of that batch takes (so the
 * variant of the response kernel the batch size selects -- beam slices, linear or tiled planes, fp64 or estimate-first table
 * cells -- is the one whose numerators come back); out: n_scans * ny * nx * na int32, each scan in the order y, x, angle */
int lslam_matcher_debug_coarse_sums_batch(lslam_matcher* m, int n_scans, const double* ranges, int ranges_stride,
                                          const double* sensor_poses, int32_t* out);
/* ... and of the FINE pass (Mapper.cpp:276-281: 3 x 3 positions x 11 angles around the coarse pass's mean) of every scan of a
 * batch, through the launches a complete match of that batch takes; centers_out: n_scans * 3, the mean each fine pass was
 * centred on (NaN where the coarse pass failed); out: n_scans * ny * nx * na int32, order y, x, angle.  With out == NULL
 * only the counts are returned. */
int lslam_matcher_debug_fine_sums_batch(lslam_matcher* m, int n_scans, const double* ranges, int ranges_stride,
                                        const double* sensor_poses, double* centers_out, int32_t* out, int* nx, int* ny,
                                        int* na);
/* FindValidPoints mask (Mapper.cpp:756-811) of one scan: out[num_beams] bytes, 1 = kept */
int lslam_matcher_debug_valid_mask(lslam_matcher* m, const double* ranges,
                                   const double sensor_pose[3], const double viewpoint[2],
                                   uint8_t* out_host);

/* ---------------------------------------------------------------------------------------- */
/* Batched many-scan mode across the GPUs of one node, one host process:     */
/* one context + matcher per device, the shared grid replicated device-to-device over xGMI,   */
/* scans [r*B/W, (r+1)*B/W) matched on device r, results in scan order.  No collective: the   */
/* units are independent.  (bench.py is the one-process-per-GPU form with RCCL.)              */
/* ---------------------------------------------------------------------------------------- */
typedef struct lslam_pool lslam_pool;
/* n_devices = 0: every visible GPU; more than are visible -> LSLAM_ERR_INVALID_ARGUMENT */
int lslam_pool_create(int n_devices, const lslam_matcher_config* cfg, const lslam_laser* laser, lslam_pool** out);
/* explicit device ordinals (repeats allowed: several contexts on one GPU, which is how the 1-GPU tests shard) */
int lslam_pool_create_on(const int* devices, int n_devices, const lslam_matcher_config* cfg, const lslam_laser* laser,
                         lslam_pool** out);
void lslam_pool_destroy(lslam_pool* pool);
int lslam_pool_devices(const lslam_pool* pool);
lslam_matcher* lslam_pool_matcher(lslam_pool* pool, int i); /* borrowed */
const char* lslam_pool_last_error(const lslam_pool* pool);
/* lslam_matcher_set_base_scans on the first device, then the 4 MB grid goes to the others by hipMemcpyPeerAsync
 * (replicate_by_rebuild = 0) or every device rasterises the same base scans itself (!= 0) */
int lslam_pool_set_base_scans(lslam_pool* pool, int n_scans, const double* ranges, int ranges_stride,
                              const double* sensor_poses, const double center_pose[3], int replicate_by_rebuild);
/* lslam_matcher_match_batch over the whole pool; out[n_scans] in scan order */
int lslam_pool_match_batch(lslam_pool* pool, int n_scans, const double* ranges, int ranges_stride,
                           const double* sensor_poses, int do_penalize, int do_refine, lslam_match_result* out);

/* ---------------------------------------------------------------------------------------- */
/* Streaming front-end: karto::Mapper::Process (Mapper.cpp:1999-2079) with every processed scan  */
/* resident in HBM (replaces Mapper::Process as karto_slam.cc:444 calls it; the pose graph's    */
/* matches run on the device, its bookkeeping on the host, the optional solver stays outside)   */
/* ---------------------------------------------------------------------------------------- */
typedef struct lslam_frontend lslam_frontend;
/* The Mapper parameters Mapper::Process and MapperGraph read (Mapper.cpp:1457-1604; defaults = the library's).
 * Variances are VARIANCES (the node's setters square their inputs, Mapper.cpp:1919-1927, 1873-1876). */
typedef struct lslam_frontend_config {
  int32_t scan_buffer_size;                  /* ScanBufferSize */
  int32_t use_scan_barycenter;               /* UseScanBarycenter: reference pose of a scan = barycentre of its readings */
  int32_t do_loop_closing;                   /* DoLoopClosing: TryCloseLoop after every processed scan */
  int32_t loop_match_minimum_chain_size;     /* LoopMatchMinimumChainSize (also the minimum near-chain size) */
  double scan_buffer_maximum_scan_distance;  /* ScanBufferMaximumScanDistance */
  double minimum_travel_distance;            /* MinimumTravelDistance */
  double minimum_travel_heading;             /* MinimumTravelHeading [rad] */
  double minimum_time_interval;              /* MinimumTimeInterval [s] */
  double link_match_minimum_response_fine;   /* LinkMatchMinimumResponseFine */
  double link_scan_maximum_distance;         /* LinkScanMaximumDistance */
  double loop_search_maximum_distance;       /* LoopSearchMaximumDistance */
  double loop_match_maximum_variance_coarse; /* LoopMatchMaximumVarianceCoarse */
  double loop_match_minimum_response_coarse; /* LoopMatchMinimumResponseCoarse */
  double loop_match_minimum_response_fine;   /* LoopMatchMinimumResponseFine */
  double loop_search_space_dimension;        /* LoopSearchSpaceDimension: the loop matcher's search_size */
  double loop_search_space_resolution;       /* LoopSearchSpaceResolution */
  double loop_search_space_smear_deviation;  /* LoopSearchSpaceSmearDeviation */
} lslam_frontend_config;
void lslam_frontend_config_defaults(lslam_frontend_config* cfg);
/* Mapper::Process with its pose graph (Mapper.cpp:1999-2079, 862-1390): every processed scan stays resident in HBM;
 * AddEdges' LinkNearChains matches (Mapper.cpp:1124-1149) and TryCloseLoop's coarse (loop matcher, created here from
 * the sequential matcher's parameters + the three loop_search_space_* values, Mapper.cpp:862-871) and fine matches
 * (Mapper.cpp:976-1051) run on the device, the graph walk (breadth-first FindNearLinkedScans, FindNearChains,
 * FindPossibleLoopClosure) on the host.  No ScanSolver: CorrectPoses() is a no-op exactly as in karto::Mapper without
 * an optimizer (the solvers are third-party back-ends).  The matcher must outlive the front-end. */
int lslam_frontend_create_ex(lslam_matcher* m, const lslam_frontend_config* cfg, lslam_frontend** out);
/* round-1 spelling: library defaults for everything not named here, loop closing OFF.
 * scan_buffer_size / scan_buffer_max_distance: ScanBufferSize, ScanBufferMaximumScanDistance
 * (Mapper.cpp:1501-1515); min_travel_*: MinimumTravelDistance / MinimumTravelHeading (:1480-1499). */
int lslam_frontend_create(lslam_matcher* m, int scan_buffer_size, double scan_buffer_max_distance,
                          double min_travel_distance, double min_travel_heading, lslam_frontend** out);
void lslam_frontend_destroy(lslam_frontend* f);
int lslam_frontend_reset(lslam_frontend* f);
/* One LaserScan in (ranges widened to double, odometric ROBOT pose), corrected ROBOT pose out.
 * *processed = 0 when HasMovedEnough rejects the scan (Mapper.cpp:2028-2031): corrected_pose is then the odometric
 * pose carried through the last correction, covariance the identity and response 0.  covariance/response may be NULL.
 * lslam_frontend_process = time 0 (the MinimumTimeInterval test of HasMovedEnough never fires). */
int lslam_frontend_process(lslam_frontend* f, const double* ranges, int n_ranges, const double odom_pose[3],
                           int* processed, double corrected_pose[3], double covariance[9], double* response);
int lslam_frontend_process_stamped(lslam_frontend* f, const double* ranges, int n_ranges, const double odom_pose[3],
                                   double time_s, int* processed, double corrected_pose[3], double covariance[9],
                                   double* response);
/* Mapper::Process for n_scans scans the caller ALREADY HOLDS (offline / batch use: a recorded trajectory), one after the
 * other, with one scan of look-ahead: while the loop search of scan t -- a chain of lone, latency-bound matches on the
 * loop matchers, 98 % of which close nothing -- is in flight, the running-window match of scan t + 1 is enqueued on the
 * sequential matcher; Process(t + 1) finds it done.  A loop that does close re-poses scan t: the look-ahead match is
 * dropped and redone, so scan for scan the poses, the edges and the graph are those of n_scans calls of
 * lslam_frontend_process_stamped.  ranges: n_scans rows of ranges_stride doubles; odom_poses n_scans*3; times_s n_scans or
 * NULL (= 0); processed n_scans; corrected_poses n_scans*3; covariances n_scans*9 or NULL; responses n_scans or NULL.
 * The reference has no counterpart (Mapper::Process takes one scan: Mapper.cpp:1999-2079). */
int lslam_frontend_process_many(lslam_frontend* f, int n_scans, const double* ranges, int ranges_stride,
                                const double* odom_poses, const double* times_s, int32_t* processed,
                                double* corrected_poses, double* covariances, double* responses);
/* diagnostics of the speculative anchor chains (the newest scan's FindValidPoints anchors are worked out beside its own
 * match, on the points at the pose the match starts from, and taken over at the final pose when that is provably the same
 * chain): out[0] = world-point refreshes that were handed one, out[1] = of those, the ones that worked the chain out again. */
int lslam_frontend_spec_chain_stats(lslam_frontend* f, int64_t out[2]);
/* diagnostics: FindValidPoints' anchors (Mapper.cpp:774-787) of resident scan scan_id at its current pose: out[0] = count,
 * out[1..count] = beam indices in order; out holds num_beams + 1 ints */
int lslam_debug_frontend_anchor_row(lslam_frontend* f, int scan_id, int32_t* out);
/* out[3] = look-ahead matches started, accepted, discarded */
int lslam_frontend_lookahead_stats(const lslam_frontend* f, int64_t out[3]);
/* GetAllProcessedScans().size(); corrected ROBOT pose of processed scan `scan_id` as it stands now (a closed loop
 * re-poses the closing scan); out[6] = scans, graph edges, near-chain matches, loop coarse matches, loop fine
 * matches, loops closed */
int lslam_frontend_num_scans(const lslam_frontend* f);
int lslam_frontend_scan_pose(const lslam_frontend* f, int scan_id, double robot_pose[3]);
int lslam_frontend_stats(const lslam_frontend* f, int64_t out[6]);
int lslam_frontend_running_scans(const lslam_frontend* f); /* ScanManager::GetRunningScans().size() */

/* ---------------------------------------------------------------------------------------- */
/* Karto hit/pass-counter occupancy grid (replaces karto::OccupancyGrid::CreateFromScans,     */
/* Karto.h:5659-5673, as SlamKarto::updateMap calls it, karto_slam.cc:507-581)                */
/* ---------------------------------------------------------------------------------------- */
typedef struct lslam_occgrid lslam_occgrid;
/* n_scans scans (rows of `ranges_stride` doubles) at SENSOR poses; the grid is sized by
 * ComputeDimensions (Karto.h:5799-5817).  No scans -> LSLAM_ERR_INVALID_ARGUMENT (reference: NULL). */
int lslam_occgrid_create_from_scans(lslam_context* ctx, const lslam_laser* laser, int n_scans, const double* ranges,
                                    int ranges_stride, const double* sensor_poses, double resolution,
                                    lslam_occgrid** out);
void lslam_occgrid_destroy(lslam_occgrid* og);
/* GetWidth/GetHeight, CoordinateConverter offset, resolution */
int lslam_occgrid_info(const lslam_occgrid* og, int32_t dims[2], double offset_xy[2], double* resolution);
/* GetValue(x,y): 0 unknown, 100 occupied, 255 free (GridStates, Karto.h:4193-4198); row-major y*w+x */
int lslam_occgrid_read_u8(lslam_occgrid* og, uint8_t* out_host);
/* nav_msgs/OccupancyGrid data as karto_slam.cc:546-569 fills it: -1 unknown, 100 occupied, 0 free */
int lslam_occgrid_read_ros_i8(lslam_occgrid* og, int8_t* out_host);

/* Sharded build over several GPUs / ranks (SURVEY 8(e) "offline map build from known poses").  The reference's
 * result depends on the scans only through (i) the union of their bounding boxes (ComputeDimensions, Karto.h:
 * 5799-5817: min/max) and (ii) per-cell hit/pass counts (AddScan/RayTrace, Karto.h:5851-5942: integer sums), so
 * disjoint scan subsets combine exactly, in any order:
 *   1. every rank: lslam_occgrid_scan_bounds over ITS scans -> box = {minx, miny, maxx, maxy}
 *      (n_scans == 0 is allowed: the identity box {+big, +big, -big, -big});
 *   2. all-reduce the boxes (min on [0..1], max on [2..3]);
 *   3. every rank: lslam_occgrid_create_partial with the merged box -> the counters of its scans on the common grid;
 *   4. all-reduce(sum) the counter buffers: lslam_occgrid_export_counters -> collective -> lslam_occgrid_import_
 *      counters (accumulate = 0).  The buffer is lslam_occgrid_counter_words 32-bit words: the pass plane
 *      (stride*height, stride = width rounded up to 8) followed by the hit plane, so ONE collective moves both.
 *      on_device = 1: `buf` is a device pointer on the grid's device (RCCL works on it in place), 0: host memory.
 *      accumulate = 1 adds a peer's exported buffer instead (one-process / tree merges).
 *   5. every rank (or only the one that publishes) reads the cells: lslam_occgrid_read_u8 / _read_ros_i8.
 * An empty merged box (no scans anywhere) -> LSLAM_ERR_INVALID_ARGUMENT, the reference's NULL. */
int lslam_occgrid_scan_bounds(lslam_context* ctx, const lslam_laser* laser, int n_scans, const double* ranges,
                              int ranges_stride, const double* sensor_poses, double box[4]);
int lslam_occgrid_create_partial(lslam_context* ctx, const lslam_laser* laser, int n_scans, const double* ranges,
                                 int ranges_stride, const double* sensor_poses, double resolution, const double box[4],
                                 lslam_occgrid** out);
int lslam_occgrid_counter_words(const lslam_occgrid* og, size_t* words);
/* device address of the counter buffer (pass plane, then hit plane; lslam_occgrid_counter_words uint32 words): a caller
 * with its own RCCL communicator all-reduces it in place.  Handing it out counts as a write of the counters: a caller
 * that writes through it again later asks for it again before the next ray cast. */
void* lslam_occgrid_counters_dev_ptr(lslam_occgrid* og);
int lslam_occgrid_export_counters(lslam_occgrid* og, uint32_t* buf, int on_device);
int lslam_occgrid_import_counters(lslam_occgrid* og, const uint32_t* buf, int on_device, int accumulate);

/* Steps 1-4 above as ONE call per rank, with RCCL called directly from this library (librccl is dlopen'ed on first use;
 * LSLAM_ERR_UNSUPPORTED if it cannot be loaded).  nccl_comm: the caller's ncclComm_t for ctx's device (one process per
 * GPU: ncclCommInitRank; one process, one thread per device: ncclCommInitAll).  n_scans = 0 is a valid shard.  Two
 * collectives on the context stream: all-reduce(max) of (-minx, -miny, maxx, maxy), then ONE all-reduce(sum, uint32)
 * over both counter planes in place in HBM (32 MB at 2005^2 cells).  *out holds the grid of ALL ranks' scans. */
int lslam_occgrid_create_sharded(lslam_context* ctx, const lslam_laser* laser, int n_scans, const double* ranges,
                                 int ranges_stride, const double* sensor_poses, double resolution, void* nccl_comm,
                                 lslam_occgrid** out);
/* The same over the devices of an lslam_pool in ONE process (scans [r*n/W, (r+1)*n/W) to device r, one host thread per
 * device, communicators from ncclCommInitAll); the grid is returned on the pool's first device.  A pool that names one
 * GPU more than once cannot form an RCCL clique: its partial grids are then merged by counter addition instead. */
int lslam_pool_occgrid_from_scans(lslam_pool* pool, const lslam_laser* laser, int n_scans, const double* ranges,
                                  int ranges_stride, const double* sensor_poses, double resolution, lslam_occgrid** out);

/* Live map over a front-end's resident scans: what SlamKarto::updateMap (karto_slam.cc:507-581) publishes every
 * map_update_interval, OccupancyGrid::CreateFromScans(mapper_->GetAllProcessedScans(), resolution_) (Karto.h:5659-5673),
 * maintained incrementally.  The scans and their poses are already on the device / in the front-end: no host copy of the
 * scans, no upload, and only the scans processed since the last update are traced unless the grid has to move (a min side
 * of the union bounding box changed: new offset, ComputeDimensions Karto.h:5799-5817), a traced scan's pose changed, or
 * the front-end was reset -- then all resident scans are retraced, still without an upload.  After every update the map
 * equals CreateFromScans over all processed scans at their current poses bit for bit (integer counters).
 * resolution 0 -> LSLAM_ERR_INVALID_ARGUMENT (Karto.h:5627-5630).  The front-end must outlive the live map. */
typedef struct lslam_livemap lslam_livemap;
int lslam_frontend_livemap_create(lslam_frontend* f, double resolution, lslam_livemap** out);
void lslam_livemap_destroy(lslam_livemap* lm);
/* SlamKarto::updateMap's CreateFromScans (karto_slam.cc:511-512).  No processed scan -> LSLAM_ERR_INVALID_ARGUMENT (the
 * reference returns NULL, Karto.h:5661-5664); the handle stays usable.  Returns with the context stream synchronised. */
int lslam_livemap_update(lslam_livemap* lm);
/* the map as an ordinary lslam_occgrid (lslam_occgrid_info / _read_u8 / _read_ros_i8 / _counter_words / _export_counters /
 * _counters_dev_ptr; karto_slam.cc:527-569 reads width, height, offset and the cells).  Borrowed: owned by the live map,
 * valid until the next update or destroy, never to be passed to lslam_occgrid_destroy.  NULL before the first update. */
lslam_occgrid* lslam_livemap_grid(lslam_livemap* lm);
/* out[6] = updates, of those appends (box unchanged: new scans traced), grows (a max side moved: rows copied to the new
 * stride, new scans traced, old scans re-traced for the cells the old bounds clipped), rebuilds (everything retraced); scans traced summed over all updates; scans in the map */
int lslam_livemap_stats(const lslam_livemap* lm, int64_t out[6]);

/* Ray cast: karto::OccupancyGrid::RayCast(const Pose2&, kt_double maxRange) (Karto.h:5717-5755), batched -- the distance
 * from a pose along its heading to the first cell that is not FREE, in the reference's fp64 expression order:
 *     steps = max(1 + |maxRange cos h| / res, 1 + |maxRange sin h| / res), delta = maxRange / steps; sample i = 1, 2, ...
 *     (while i < steps) lies i * delta away; the first sample outside the grid or on a cell that is not free (unknown
 *     cells stop a ray like occupied ones) ends the ray at i * delta; a ray that runs out returns maxRange.  The start
 *     cell itself is never tested.
 * Rays read the cell states lslam_occgrid_read_u8 reports; the grid keeps them as a byte plane in HBM that is derived
 * again only when the counters have changed since the last cast (create, import_counters, a live-map update, handing
 * out lslam_occgrid_counters_dev_ptr).  Every entry point works on the borrowed grid of lslam_livemap_grid.
 *   lslam_occgrid_ray_cast        n_rays poses (x, y, heading), 3 doubles each; max_ranges[n_rays], or NULL: the common
 *                                 max_range for every ray; out[n_rays].  (Karto.h:5717-5755)
 *   lslam_occgrid_ray_cast_scans  n_poses SENSOR poses x the beams of `laser` (its beam count as everywhere else in this
 *                                 library): beam i has heading pose.heading + minimum_angle + i * angular_resolution,
 *                                 evaluated left to right (Karto.h:5394), and is cast as above (Karto.h:5717-5755).
 *                                 out_ranges[n_poses][out_stride], out_stride >= beams: the layout lslam_matcher_match_batch
 *                                 and the front-end take as `ranges`.  Bit-identical to lslam_occgrid_ray_cast fed those
 *                                 headings.
 * The host entry points are synchronous.  The _dev ones take device pointers, enqueue on the context stream and do
 * not wait; nothing is allocated for a repeated shape.  (Karto.h:5717-5755)
 * LSLAM_ERR_INVALID_ARGUMENT: NULL pointers, negative counts, out_stride below the beam count, a common max_range that
 * is not a positive finite number (all without a device).  LSLAM_ERR_UNSUPPORTED: a ray the reference itself cannot
 * finish -- its `steps` does not fit the reference's uint32 counter, its stopping sample's grid coordinate does not fit
 * int32, or its per-ray max_range is not a positive finite number.  That is found on the device: such a ray's output
 * is NaN, every other ray's is valid, and the error is returned by the host entry point, or by the next
 * lslam_synchronize after a _dev one. */
int lslam_occgrid_ray_cast(lslam_occgrid* og, int n_rays, const double* poses_xyh, const double* max_ranges /* NULL: common */,
                           double max_range, double* out_host);
int lslam_occgrid_ray_cast_dev(lslam_occgrid* og, int n_rays, const double* d_poses_xyh, const double* d_max_ranges,
                               double max_range, double* d_out);
int lslam_occgrid_ray_cast_scans(lslam_occgrid* og, const lslam_laser* laser, int n_poses, const double* sensor_poses,
                                 double max_range, double* out_ranges_host, int out_stride);
int lslam_occgrid_ray_cast_scans_dev(lslam_occgrid* og, const lslam_laser* laser, int n_poses, const double* d_sensor_poses,
                                     double max_range, double* d_out_ranges, int out_stride);
/* out[4] = calls, rays, cell-plane refreshes, samples tested (what the loop of Karto.h:5717-5755 would have tested: the
 * stopping index of a stopped ray, every sample of one that ran out).  Waits for the context stream. */
int lslam_occgrid_ray_cast_stats(const lslam_occgrid* og, int64_t out[4]);

/* ---------------------------------------------------------------------------------------- */
/* Hector log-odds occupancy grid  (replaces hectorslam::OccGridMapBase<LogOddsCell,...>,    */
/* H/map/OccGridMapBase.h, H/map/GridMapLogOdds.h, H/map/GridMapBase.h)                      */
/* ---------------------------------------------------------------------------------------- */
/* GridMapBase ctor (H/map/GridMapBase.h:54-67) x MapRepMultiMap pyramid (H/slam_main/
 * MapRepMultiMap.h:50-93): level i has size>>i cells of cell_length*2^i.
 * top-left offset as in H/map/GridMapBase.h:270-286. */
int lslam_map_create(lslam_context* ctx, int size_x, int size_y, float cell_length,
                     float offset_x, float offset_y, int levels, lslam_map** out);
void lslam_map_destroy(lslam_map* map);
int lslam_map_reset(lslam_map* map);                         /* GridMapBase::reset (:95-110) */
int lslam_map_set_update_factor_free(lslam_map* map, float p);     /* H/map/OccGridMapBase.h:103-106 */
int lslam_map_set_update_factor_occupied(lslam_map* map, float p); /* :108-111 */
int lslam_map_levels(const lslam_map* map);
int lslam_map_size(const lslam_map* map, int level, int* size_x, int* size_y);
float lslam_map_scale_to_map(const lslam_map* map, int level); /* getScaleToMap (:292-295) */
/* MapRepMultiMap::updateByScan (H/slam_main/MapRepMultiMap.h:174-191): OccGridMapBase::updateByScan
 * (H/map/OccGridMapBase.h:118-168) on every pyramid level.  Level 0 takes (points_xy, origo_xy); level
 * i > 0 takes -- exactly like the reference's dataContainers[i-1] -- the container CACHED BY THE LAST
 * lslam_map_match_data CALL, scaled by 1/2^i (DataPointContainer::setFrom, H/scan/DataPointContainer.h:
 * 46-58): empty until the first matchData, stale if the caller updates with a different scan than it
 * matched.  HectorSlamProcessor::update always matches first (HectorSlamProcessor.h:84-110), so in the
 * reference's own flow all levels see the same scan.  A single-level map has no such coupling.
 * points_xy: n points in LEVEL-0 MAP-CELL units, robot frame (hector_slam.cc:320-362);
 * origo_xy: DataContainer origo; pose_world: (x[m], y[m], heading).
 * Points whose end cell is not representable (NaN/Inf or beyond the int32 range) are dropped, as on
 * the reference's x86 build, where the float->int cast yields INT_MIN and the in-map test rejects it.
 * At most 65536 points per container (LSLAM_ERR_UNSUPPORTED beyond; the reference has no limit).
 * ASYNCHRONOUS and pipelined: when the call returns points_xy has been copied and may be reused at once, this scan's
 * marks are enqueued on the context stream and its apply rides in the NEXT update's launch (or in the flush any reader
 * issues: lslam_map_read_*, lslam_map_match_data, lslam_synchronize ... are ordered after the complete update). */
int lslam_map_update_by_scan(lslam_map* map, const float* points_xy, int n,
                             const float origo_xy[2], const float pose_world[3]);
int lslam_map_update_by_scan_dev(lslam_map* map, const float* points_xy_dev, int n,
                                 const float origo_xy[2], const float pose_world[3]);
/* BATCHED update: n_scans containers, each with its own origo and robot pose, applied exactly as n_scans successive
 * [matchData-cached] updateByScan calls in this order would (bit-identical log-odds planes: the float operations of
 * every cell are applied in scan order), but marked in parallel and applied by one pass over the map -- three
 * launches per pyramid level per 64 scans instead of two dependent launches per scan and level.  For callers that know
 * several poses before the map is needed again: an offline map build from known poses, or a front-end whose matcher does
 * not read this map (the Karto front-end of BASELINE config 5).
 * points_xy: the containers back to back (sum of n_points[] points, level-0 map-cell units); n_points[n_scans];
 * origos_xy[n_scans][2]; poses_world[n_scans][3].  Every level is fed the same scan (each scan counts as matched
 * first); afterwards the cached container is the last scan's. */
int lslam_map_update_batch(lslam_map* map, int n_scans, const float* points_xy, const int32_t* n_points,
                           const float* origos_xy, const float* poses_world);
/* same with the points already in HBM (n_points / origos / poses stay host arrays: a few bytes per scan) */
int lslam_map_update_batch_dev(lslam_map* map, int n_scans, const float* points_xy_dev, const int32_t* n_points,
                               const float* origos_xy, const float* poses_world);
/* OccGridMapBase::updateByScanJustOnce (H/map/OccGridMapBase.h:175-217): the lesson4
 * make_hector_map demo variant -- points in METRES, begin cell and 1/0.05 scale hard-coded by
 * the reference (we take them as parameters; pass 800,800,0.05 for the literal behaviour). */
int lslam_map_update_just_once(lslam_map* map, const float* points_xy, int n,
                               const float origo_xy[2], float begin_x, float begin_y,
                               double metres_per_cell);
/* MapRepresentationInterface::matchData (H/slam_main/MapRepresentationInterface.h:58-60) =
 * MapRepMultiMap::matchData (H/slam_main/MapRepMultiMap.h:144-167): coarse-to-fine Gauss-Newton
 * scan-to-map matching on the pyramid.  points_xy / origo_xy = the DataContainer (level-0 map-cell
 * units; origo_xy may be NULL = (0,0); the matcher itself never reads the origo, but the container is
 * cached for the next updateByScan, see above); begin_world = beginEstimateWorld; out_cov = covMatrix
 * (the last Hessian, ScanMatcher.h:82-86).  n = 0 returns begin_world unchanged (ScanMatcher.h:96). */
int lslam_map_match_data(lslam_map* map, const float* points_xy, int n, const float origo_xy[2],
                         const float begin_world[3], float out_pose[3], float out_cov[9]);
/* BATCHED matchData: n_entries matches against the map as it is, in ONE launch and with one wait for all of them.  Entry e
 * returns exactly what lslam_map_match_data returns for (container entry_container[e], begin_world[e]): coarse to fine over
 * all levels, 3+1 / 5+1 iterations, the +-0.2 heading step clamp, normalize_angle, the last Hessian as covariance.  For
 * callers with many matches against the same pyramid: one scan from K candidate start poses (re-localisation), a particle
 * front-end, a log replayed against a finished map, a recorded trajectory being scored.
 * points_xy: the n_containers containers back to back (sum of n_points[] points, level-0 map-cell units, as for
 * lslam_map_update_batch); n_points[n_containers]; entry_container[n_entries] names each entry's container -- one container
 * may serve any number of entries (K hypotheses of one scan upload it once) --, or NULL: entry i uses container i (then
 * n_containers == n_entries); begin_world[n_entries][3]; out_poses[n_entries][3]; out_covs[n_entries][9], may be NULL.
 * An entry whose container is empty returns its begin_world bit for bit; n_entries == 0 is LSLAM_OK and launches nothing.
 * A PURE QUERY: unlike lslam_map_match_data it does not replace the cached container the next updateByScan feeds to the
 * levels above 0 (lslam_map_cached_points is unchanged) and it changes no plane; like every reader it enqueues a pending
 * pipelined apply first.  An entry's result depends on its container, its start pose and the map only, not on the batch
 * around it.  LSLAM_MAP_OPT_ORDERED_SUMS = 1: one block per entry of the ordered kernel, bit-identical to the single
 * ordered call (and bound by its 4266 points per container).
 * The host form returns with the results in the caller's arrays.  The _dev form takes points_xy, begin_world, out_poses and
 * out_covs in HBM (n_points / entry_container stay host arrays and have been copied when it returns) and is ASYNCHRONOUS
 * on lslam_stream(): the results are valid after lslam_synchronize or the caller's own event. */
int lslam_map_match_batch(lslam_map* map, int n_entries, int n_containers, const float* points_xy, const int32_t* n_points,
                          const int32_t* entry_container, const float* begin_world, float* out_poses, float* out_covs);
int lslam_map_match_batch_dev(lslam_map* map, int n_entries, int n_containers, const float* points_xy_dev,
                              const int32_t* n_points, const int32_t* entry_container, const float* begin_world_dev,
                              float* out_poses_dev, float* out_covs_dev);
/* matchData adds its nine Hessian / gradient sums over the points in PARALLEL (tree sums in fp32, float32 exp / sin / cos):
 * within 1e-5 of the reference's poses on the test sequences, tolerance 1e-4 m / 1e-4 rad.  LSLAM_MAP_OPT_ORDERED_SUMS = 1
 * selects the kernel that adds them in point order like the reference's sequential loop (H/matcher/ScanMatcher.h:94-126)
 * and evaluates the libm calls in double like its host code: bit-equal to the CPU restatement, ~4x slower. */
/* POSE SCORING: how well does a container fit ONE level of the map at a pose?  The half of OccGridMapUtil the matcher does
 * not use (H/map/OccGridMapUtil.h): what tells the K answers of lslam_map_match_batch apart, and -- as a lattice -- what
 * finds the start pose the local Gauss-Newton matcher needs.
 * Common to the three calls: containers as for lslam_map_match_batch (points_xy back to back in level-0 map-cell units,
 * n_points[n_containers], entry_container[n_entries] or NULL, at most 65536 points each, in BOTH sum modes); poses are WORLD
 * poses and go to the level's raster as the matcher's do (getMapCoordsPose, GridMapBase.h:238-242), points are scaled by
 * 2^-level (DataContainer::setFrom, MapRepMultiMap.h:161); `level` is per call.  A point outside pointOutOfMapBounds
 * contributes the value 0; an empty container has residual 0 and likelihood 0 / 0 = NaN, as the reference's arithmetic gives.
 * Default: fp32 tree sums, hardware exp / rcp; a state's result depends on its container, its pose and the map only -- not on
 * the batch around it or on the call it came through.  LSLAM_MAP_OPT_ORDERED_SUMS = 1: the residual is added in container
 * order with exp / sin / cos in double, bit for bit the reference's result.  (LSLAM_SCORE_CHUNK = 2 | 4 | 8 in the environment
 * when a map is created: points per lane in flight in the default kernel, for measurements; results do not depend on it.)
 * PURE QUERIES: no plane, no cached container, no lslam_map_cached_points changes; like every reader they enqueue a pending
 * pipelined apply first.  n_entries == 0 is LSLAM_OK and launches nothing.  LSLAM_ERR_INVALID_ARGUMENT, outputs untouched: a
 * level outside the pyramid, a container index out of range, a lattice with a non-positive count, missing arrays.
 * The host forms return with the results in the caller's arrays; the _dev forms take points, poses and outputs in HBM
 * (n_points / entry_container / centre / counts / steps stay host arrays) and are ASYNCHRONOUS on lslam_stream().
 *
 * lslam_map_score_batch: getResidualForState (:357-374, interpMapValue :379-434) and getLikelihoodForState /
 * getLikelihoodForResidual (:342-355) for n_entries (container, pose) pairs -> out_residual[n_entries] (may be NULL),
 * out_likelihood[n_entries] = 1 - residual / n. */
int lslam_map_score_batch(lslam_map* map, int n_entries, int n_containers, const float* points_xy, const int32_t* n_points,
                          const int32_t* entry_container, const float* poses_world, int level, float* out_residual,
                          float* out_likelihood);
int lslam_map_score_batch_dev(lslam_map* map, int n_entries, int n_containers, const float* points_xy_dev, const int32_t* n_points,
                              const int32_t* entry_container, const float* poses_world_dev, int level, float* out_residual_dev,
                              float* out_likelihood_dev);
/* getCovarianceForPose (:249-306) and getCovMatrixWorldCoords (:314-339) per entry: the likelihoods of the seven sigma points
 * (+-1.5 cells in x, +-1.5 cells in y, +-0.05 rad, then the pose itself, on the level's raster) ->
 * out_likelihoods[n_entries][7]; their likelihood-weighted covariance -> out_cov_map[n_entries][9] (row-major 3 x 3, level
 * cells / rad) and, scaled with the level's cell length, out_cov_world[n_entries][9] (m / rad); either cov array may be NULL.
 * The covariance is computed on the device behind the scoring launch, in fp32 and in Eigen's expression order. */
int lslam_map_pose_covariance_batch(lslam_map* map, int n_entries, int n_containers, const float* points_xy, const int32_t* n_points,
                                    const int32_t* entry_container, const float* poses_world, int level, float* out_likelihoods,
                                    float* out_cov_map, float* out_cov_world);
int lslam_map_pose_covariance_batch_dev(lslam_map* map, int n_entries, int n_containers, const float* points_xy_dev,
                                        const int32_t* n_points, const int32_t* entry_container, const float* poses_world_dev,
                                        int level, float* out_likelihoods_dev, float* out_cov_map_dev, float* out_cov_world_dev);
/* getLikelihoodForState (:342-347) over a lattice of poses around centre_world, for one container of n points: state (i, j, k),
 * i < counts[0] = nx, j < counts[1] = ny, k < counts[2] = nt, has the world pose
 *   (c.x + (float)(i - nx/2) * steps[0],  c.y + (float)(j - ny/2) * steps[1],  c.theta + (float)(k - nt/2) * steps[2])
 * (integer division, fp32, product and sum rounded separately), evaluated on the device: no pose array goes up.
 * out_volume[nt][ny][nx]: the likelihoods, bit-identical to lslam_map_score_batch called with these poses.
 * out_best_index / out_best_likelihood (each may be NULL): the state with the highest likelihood, the lowest linear index
 * (k * ny + j) * nx + i among equals; -1 and NaN when every likelihood is NaN.  At most 2^24 states per call. */
int lslam_map_score_lattice(lslam_map* map, const float* points_xy, int n, const float centre_world[3], const int32_t counts[3],
                            const float steps[3], int level, float* out_volume, int32_t* out_best_index,
                            float* out_best_likelihood);
int lslam_map_score_lattice_dev(lslam_map* map, const float* points_xy_dev, int n, const float centre_world[3],
                                const int32_t counts[3], const float steps[3], int level, float* out_volume_dev,
                                int32_t* out_best_index_dev, float* out_best_likelihood_dev);
/* The batched update's scratch (lslam_map_update_batch*): every scan of a batch owns a WINDOW of 8x8-cell tiles -- the
 * square its rays can reach from its begin cell -- in a pool of 64-byte tile slots, not a byte plane of the whole map
 * (a 1081-beam scan with 20 m of range on a 0.025 m map: 2.6 MB, whatever the map's size).
 *  LSLAM_MAP_OPT_BATCH_SCRATCH_MB (default 192): budget of one pyramid level's pool; the scans of a call are applied in
 *    rounds whose windows fit it (one round normally; a single scan whose window is larger gets a round -- and the
 *    memory -- of its own).  Results do not depend on it.
 *  LSLAM_MAP_OPT_BATCH_RADIUS_CELLS (default 0 = none): for lslam_map_update_batch_dev, whose points the host never
 *    sees: an upper bound, in level-0 cells, on |point - origo| of every scan handed in.  Without it such scans get
 *    windows the size of the map (the rounds still keep the scratch inside the budget, there are just more of them).
 *    A bound that is too small loses cells: lslam_map_batch_stats counts them, and must read 0. */
enum { LSLAM_MAP_OPT_ORDERED_SUMS = 1, LSLAM_MAP_OPT_BATCH_SCRATCH_MB = 2, LSLAM_MAP_OPT_BATCH_RADIUS_CELLS = 3 };
int lslam_map_set_option(lslam_map* map, int option, int value);
/* out[0] = bytes of batched-update scratch held over all levels (tile-slot pools + tile flags), out[1] = rounds level 0
 * of the last batch took, out[2] = cells found outside their scan's window so far (synchronises), out[3] = budget, bytes */
int lslam_map_batch_stats(lslam_map* map, int64_t out[4]);
/* Host-only planner (no context, no GPU): the windows and rounds a batched update of n_scans scans would use on a level of
 * sx x sy cells.  begin_cells_xy: the scans' begin cells on that level; reach_cells: per scan the distance of its farthest
 * point from its origo in LEVEL-0 cells (NULL or < 0: unknown = the whole map); level_factor: 1, 0.5, 0.25 ... for levels
 * 0, 1, 2.  windows_out[4k..] = first tile x, first tile y, tiles wide, tiles high (8x8-cell tiles; 0 wide = nothing
 * of the scan reaches the map); base_out[k] = first tile slot inside its round; round_out[k] (may be NULL);
 * *pool_bytes_out = bytes the largest round needs.  Returns the number of rounds (>= 0) or a negative lslam_status. */
int lslam_map_plan_batch_windows(int sx, int sy, int n_scans, const int32_t* begin_cells_xy, const int32_t* n_points,
                                 const double* reach_cells, double level_factor, int64_t budget_bytes,
                                 int32_t* windows_out, uint32_t* base_out, int32_t* round_out, int64_t* pool_bytes_out);
/* LaserScan -> DataContainer ON THE DEVICE: HectorMappingRos::scanCallback's pre-processing (hector_slam.cc:186-205):
 * laser_geometry's projectLaser(scan, cloud, 30.0) and rosPointCloudToDataContainer (hector_slam.cc:320-362).  The
 * container stays resident in HBM; lslam_map_match_container / lslam_map_update_by_container are matchData /
 * updateByScan on it (no per-scan point list crosses PCIe, only the float32 ranges).  The cos/sin table of the beam
 * angles is built on the host once per scan geometry and cached (laser_geometry's co_sine_map_), so the projected
 * float32 points are bit-identical to a host evaluation.  The base_link -> laser transform is planar (yaw +
 * translation); a tilted laser needs the host path. */
typedef struct lslam_hector_scan {
  float angle_min, angle_increment, range_min, range_max; /* sensor_msgs/LaserScan header */
  float range_cutoff;         /* projectLaser's range_cutoff (hector_slam.cc:193 passes 30.0); < 0 = range_max */
  float sqr_laser_min_dist;   /* p_sqr_laser_min_dist_ */
  float sqr_laser_max_dist;   /* p_sqr_laser_max_dist_ */
  float use_max_scan_range;   /* p_use_max_scan_range_ */
  float laser_z_min, laser_z_max; /* p_laser_z_min_value_, p_laser_z_max_value_ */
  float laser_x, laser_y, laser_z, laser_yaw; /* laserTransform_: base_link -> laser */
} lslam_hector_scan;
int lslam_map_set_scan(lslam_map* map, const float* ranges, int n, const lslam_hector_scan* scan, int* n_points);
/* A de-skewed cloud -> DataContainer ON THE DEVICE: rosPointCloudToDataContainer (hector_slam.cc:320-362) applied to what
 * lslam_deskew_scan / lslam_deskew_batch return (xyz: n x 3 float32, valid: n), the counterpart of lslam_map_set_scan for
 * lesson5's output.  Only beams with valid = 1 enter, in beam order; d2 = x*x + y*y in float32 and the filters of :336-345;
 * the transform is tf's double row . v + origin (planar: yaw + translation) and INCLUDES the point's z:
 * pointPosLaserFrameZ = (float)(bz - tz) is tested against the z window (:351-353); the point becomes ((float)bx, (float)by)
 * * scaleToMap.  Of `scan` the filter fields (sqr_laser_*_dist, use_max_scan_range, laser_z_min / laser_z_max) and the
 * laser transform are read; angle_min, angle_increment, range_min, range_max and range_cutoff are IGNORED (the de-skew
 * has applied the scan's own range window).  The container is left resident like lslam_map_set_scan's:
 * lslam_map_match_container / lslam_map_update_by_container work on it.
 * A consequence of composing the two lessons literally: lesson5 transforms (x, y, 1.0), so its cloud's z is ~ 1 (exactly 1
 * for a planar robot: no roll or pitch rate, no odometry z), and the Hector node's default z window (-1, 1) -- both ends
 * exclusive -- DROPS EVERY such POINT.  A caller who wants points passes a window that contains 1 (e.g. laser_z_max = 2). */
int lslam_map_set_cloud(lslam_map* map, const float* xyz, const uint8_t* valid, int n, const lslam_hector_scan* scan,
                        int* n_points);
/* copies up to `capacity` points of the resident container (+ its origo) to the host; returns the container size */
int lslam_map_read_container(lslam_map* map, float* out_xy, int capacity, float origo_xy[2]);
int lslam_map_match_container(lslam_map* map, const float begin_world[3], float out_pose[3], float out_cov[9]);
int lslam_map_update_by_container(lslam_map* map, const float pose_world[3]);
/* size of the cached containers (dataContainers[i].getSize()); 0 before the first matchData */
int lslam_map_cached_points(const lslam_map* map);
/* LogOddsCell::logOddsVal of every cell, row-major y*size_x+x (H/map/GridMapLogOdds.h:85) */
int lslam_map_read_logodds(lslam_map* map, int level, float* out_host);
/* nav_msgs/OccupancyGrid data as hector_slam.cc:287-304 / hector_mapping.cc:186-200 publish
 * it: free(<0) -> 0, occupied(>0) -> 100, else -1 */
int lslam_map_read_occupancy_i8(lslam_map* map, int level, int8_t* out_host);
void* lslam_map_cells_dev_ptr(lslam_map* map, int level); /* float log-odds plane in HBM (flushes, see below) */
/* lslam_map_update_by_scan[_dev] / _by_container are PIPELINED: a call launches [apply of the previous scan | mark of
 * this scan] as ONE kernel and leaves this scan's apply pending (one launch per scan in steady state instead of two
 * dependent ones; bit-identical planes).  Every reader in this library -- lslam_map_read_*, lslam_map_match_* (lslam_map_match_batch* included), the batched
 * update, lslam_map_cells_dev_ptr, lslam_synchronize -- enqueues the pending apply first.  A caller that consumes the raw
 * plane from its OWN stream calls lslam_map_flush before recording its event on lslam_stream(). */
int lslam_map_flush(lslam_map* map);

/* ---------------------------------------------------------------------------------------- */
/* Streamed HectorSlamProcessor (H/slam_main/HectorSlamProcessor.h:57-117): many scans per     */
/* call, the pose chain, the update decision and the update geometry kept on the device.       */
/* ---------------------------------------------------------------------------------------- */
/* Per scan (HectorSlamProcessor::update, :81-108):
 *   newPose = map_without_matching ? hint : matchData(hint, container, lastScanMatchCov)          (:88-96)
 *   lastScanMatchPose = newPose                                                                   (:98)
 *   if (poseDifferenceLargerThan(newPose, lastMapUpdatePose, minDist, minAngle) || map_without_matching)
 *     updateByScan(container, newPose) on every level; lastMapUpdatePose = newPose                (:101-107)
 * Level 0 takes the container it is handed, level i > 0 what the last matchData cached, scaled (H/slam_main/
 * MapRepMultiMap.h:161,174-191).  Every scan is one short chain of launches on lslam_stream() -- [projection], match (the
 * arithmetic of lslam_map_match_data's parallel-sum kernel: the same bits for the same container, start pose, map and
 * LSLAM_GN_THREADS, the register or LDS form chosen from the readings / points per scan of the CALL), mark, apply -- whose
 * count, start pose, decision and per-level update geometry stay in a device state block; a call makes ONE host
 * synchronisation, at its end, whatever n_scans is.  A scan k+1 sees the map as scan k left it.
 * The map is BORROWED: every lslam_map_* call keeps working on it between calls (the cached container, its origo and --
 * ranges form -- the resident container of lslam_map_set_scan are the last streamed scan's).
 * The gate is H/util/UtilFunctions.h:72-91 in fp32: sqrt(dx*dx + dy*dy) > minDist, or the heading difference, wrapped once by
 * +-2 pi, beyond minAngle.  The reference's unqualified abs() there resolves to abs(int) with its toolchain, so the
 * wrapped difference is truncated toward zero before the comparison: that is the default here;
 * LSLAM_HECTOR_OPT_FABS_ANGLE_GATE = 1 compares fabsf of it.
 * Update geometry: for a scan taken without matching the rotation is the host's cosf / sinf of the hint (bit for bit
 * lslam_map_update_by_scan at that pose); for a matched scan the device evaluates (float)cos((double)theta) and
 * (float)sin((double)theta), which may differ from the host libm's float functions in the last bit. */
typedef struct lslam_hector lslam_hector;
typedef struct lslam_hector_record { /* 64 bytes */
  float pose[3];     /* lastScanMatchPose after this scan (:98) */
  float cov[9];      /* lastScanMatchCov after this scan (:91; an empty or unmatched scan leaves it as it was) */
  int32_t updated;   /* the map was updated with this scan (:101-107) */
  int32_t n_points;  /* size of the scan's container */
  int32_t pad[2];
} lslam_hector_record;
enum { LSLAM_HECTOR_OPT_FABS_ANGLE_GATE = 1 };
/* HectorSlamProcessor ctor (:57-68) on an existing map, which it borrows (destroy the processor first): state as after
 * reset(), thresholds 0.4 / 0.13 (:66-67) */
int lslam_hector_create(lslam_map* map, lslam_hector** out);
void lslam_hector_destroy(lslam_hector* h);
/* HectorSlamProcessor::reset (:111-117): lastMapUpdatePose = FLT_MAX, lastScanMatchPose = 0, lslam_map_reset;
 * lastScanMatchCov stays what it was, as in the reference */
int lslam_hector_reset(lslam_hector* h);
/* setMapUpdateMinDistDiff / setMapUpdateMinAngleDiff (:66-67) */
int lslam_hector_set_update_thresholds(lslam_hector* h, float min_dist, float min_angle);
int lslam_hector_set_option(lslam_hector* h, int option, int value);
/* update() (:81-108) for n_scans LaserScans of n_readings float32 readings each (row k at ranges + k * ranges_stride): the
 * projection of lslam_map_set_scan on the device, its count never read back.  pose_hints: n_scans x 3, or NULL = chain: scan
 * 0 starts from lastScanMatchPose and scan k from scan k-1's result (hector_slam.cc:200-204).  map_without_matching:
 * n_scans flags, NULL = all 0.  out: n_scans records, may be NULL.  n_scans == 0 is LSLAM_OK and does nothing.
 * LSLAM_ERR_UNSUPPORTED (with a message) for LSLAM_MAP_OPT_ORDERED_SUMS maps, pyramids deeper than 8 levels and more than
 * 65536 readings per scan. */
int lslam_hector_process_many(lslam_hector* h, const lslam_hector_scan* scan, int n_scans, int n_readings, const float* ranges,
                              int ranges_stride, const float* pose_hints, const uint8_t* map_without_matching,
                              lslam_hector_record* out);
/* the same for DataContainers: points_xy = the containers back to back in level-0 map-cell units (as lslam_map_match_batch
 * takes them), n_points[n_scans], origos_xy n_scans x 2 or NULL = (0, 0) */
int lslam_hector_process_many_points(lslam_hector* h, int n_scans, const float* points_xy, const int32_t* n_points,
                                     const float* origos_xy, const float* pose_hints, const uint8_t* map_without_matching,
                                     lslam_hector_record* out);
/* the same for RAW scans that lesson5 de-skews first: ranges + params + IMU samples exactly as lslam_deskew_batch takes them
 * (one geometry per call) go through ONE batched de-skew launch for the whole call, then every scan's cloud goes through
 * rosPointCloudToDataContainer on the device (lslam_map_set_cloud's kernel; `scan` as there, origo as in the ranges form),
 * match, mark and apply.  Nothing comes back before the end of the call: still one host synchronisation.  Afterwards the
 * map's resident and cached containers are the last scan's.  Mind the z window (lslam_map_set_cloud).  The same
 * LSLAM_ERR_UNSUPPORTED cases as lslam_hector_process_many; what lslam_deskew_batch refuses is refused here. */
struct lslam_deskew_params;
int lslam_hector_process_many_deskewed(lslam_hector* h, const lslam_hector_scan* scan, int n_scans, int n_readings,
                                       const float* ranges, int ranges_stride, const struct lslam_deskew_params* params,
                                       const int32_t* imu_first, const double* imu_time, const double* imu_rot_x,
                                       const double* imu_rot_y, const double* imu_rot_z, const float* pose_hints,
                                       const uint8_t* map_without_matching, lslam_hector_record* out);
/* GATED forms: clouds that are de-skewed already, and lesson5's whole node in front of update().  Whether a scan reaches
 * HectorSlamProcessor::update (HectorSlamProcessor.h:81-108) is decided by a per-scan TAKE word the kernels read from HBM:
 * the reference's node publishes nothing for a scan PruneImuDeque / PruneOdomDeque refuse (lidar_undistortion.cc:96-125), so
 * rosPointCloudToDataContainer (hector_slam.cc:320-362) and update() never run for it.  A scan that is NOT TAKEN changes
 * nothing of the processor: the three state vectors, the covariance, the live (resident) and the cached container with their
 * counts and origo and every plane stay as they were; its record is all zero except n_points = -1 (the fleet's convention
 * for active[i] == 0).  It is NOT an empty container, which update() would process (and which would empty the cached
 * container the next update of levels > 0 reads).  `scans` of lslam_hector_stats advances by the taken scans only; the map's
 * resident container is the last TAKEN scan's and is untouched when none was taken.  pose_hints NULL chains from
 * lastScanMatchPose, and a scan that is not taken does not break the chain; hints and flags of such a scan are not read.
 * A scan is the chain container, match, mark, apply -- 4 launches, taken or not: a scan that is not taken costs four launches
 * of blocks that load one word and return.  All three make ONE host synchronisation, at the end of the call, whatever the
 * count; inputs go up through pinned staging.  What lslam_hector_process_many refuses is refused here, before anything is
 * enqueued; NULL handles are LSLAM_ERR_INVALID_ARGUMENT without a device.
 *
 * update() for n_scans clouds of n_points beams in the de-skew's layout: xyz[n_scans][n_points][3] float32,
 * valid[n_scans][n_points] (NULL: every point valid), through rosPointCloudToDataContainer on the device.
 * take[n_scans] (NULL: all): a scan with take == 0 is not taken (see above). */
int lslam_hector_process_many_clouds(lslam_hector* h, const lslam_hector_scan* scan, int n_scans, int n_points,
                                     const float* xyz, const uint8_t* valid, const uint8_t* take,
                                     const float* pose_hints, const uint8_t* map_without_matching, lslam_hector_record* out);
/* the same on clouds already in HBM (Deskewer.batch_dev, MotionSync.scans_dev, IcpMatcher.convert_dev): nothing but
 * hints and flags goes up; taken iff take_dev[k * take_stride] > 0 (NULL: all).  take_stride counts int32 words:
 * &records_dev[0].status of lslam_msync_record with sizeof(lslam_msync_record) / 4 (22) serves as it stands --
 * LSLAM_MSYNC_CORRECTED is 1, QUEUED 0, every refusal negative. */
int lslam_hector_process_many_clouds_dev(lslam_hector* h, const lslam_hector_scan* scan, int n_scans, int n_points,
                                         const float* xyz_dev, const uint8_t* valid_dev, const int32_t* take_dev,
                                         int take_stride, const float* pose_hints, const uint8_t* map_without_matching,
                                         lslam_hector_record* out);
/* n_msgs ScanCallbacks of lesson5's node chained into update(): lslam_msync_scans_dev on buffers the processor owns
 * (its lazily created lslam_deskew, as _deskewed uses), then the gated chain per callback on the status the walk wrote.
 * Record k of both outputs belongs to callback k, which corrects message k - 1 (CacheLaserScan's one-scan lag,
 * lidar_undistortion.cc:142-156; row 0: the scan the previous call left queued).  sync_records may be NULL.  The arguments
 * from `laser` to `odom_seen` are lslam_msync_scans'.  Refused, with neither handle changed: what lslam_msync_scans_dev
 * refuses (LSLAM_ERR_INVALID_ARGUMENT: another n_readings than the handle's first scan's, *_seen that decrease or exceed the
 * pushed count; LSLAM_ERR_UNSUPPORTED: more than 65535 callbacks) and a `sync` whose context is not the map's
 * (LSLAM_ERR_INVALID_ARGUMENT). */
struct lslam_msync;
struct lslam_msync_laser;
struct lslam_msync_record;
int lslam_hector_process_many_synced(lslam_hector* h, struct lslam_msync* sync, const lslam_hector_scan* scan,
                                     const struct lslam_msync_laser* laser, int n_msgs, int n_readings, const float* ranges,
                                     int ranges_stride, const double* stamps, const float* time_increments,
                                     const int64_t* imu_seen, const int64_t* odom_seen, const float* pose_hints,
                                     const uint8_t* map_without_matching, lslam_hector_record* out,
                                     struct lslam_msync_record* sync_records);
/* getLastScanMatchPose / getLastScanMatchCovariance (:120-122) and lastMapUpdatePose; any pointer may be NULL.  Host only. */
int lslam_hector_state(lslam_hector* h, float last_match_pose[3], float last_match_cov[9], float last_update_pose[3]);
/* out = {scans processed, map updates made, calls that processed scans, waits for the stream those calls made}.  The last is
 * counted where the library waits: once per call, at its end, plus once in a ranges-form call that meets a new scan geometry
 * (it uploads the cos / sin table and waits for it).  Inputs go up through pinned memory, so no copy blocks on the way.  NOT
 * counted: what the runtime does inside an allocation -- a call that has to grow a staging or device buffer (the first call, or
 * one longer than any before it) goes through hipHostMalloc / hipHostFree / hipMalloc, which may wait for the device. */
int lslam_hector_stats(const lslam_hector* h, int64_t out[4]);

/* ---------------------------------------------------------------------------------------- */
/* Hector fleet: many streamed processors, each on its own map, stepped in lockstep launches.  */
/* ---------------------------------------------------------------------------------------- */
/* Within one processor a scan's chain of launches is a true dependency; across processors it is not.  A fleet BORROWS
 * R = n_members existing lslam_hector processors (destroy the fleet first) and advances every one of them by one scan per
 * STEP with the launches of ONE chain: [projection], match, mark, apply -- 4 per step in the ranges form, 3 in the container
 * form, whatever R is.  It keeps no SLAM state of its own: thresholds, the gate option, the three state vectors, the
 * covariance and the map are the member's, read at the start of a call and handed back at its end, so every member stays
 * usable through lslam_hector_* and its map through lslam_map_* between fleet calls.
 * Every per-scan array of a call is indexed i = step * R + member: ranges row i at ranges + i * ranges_stride; n_points[i]
 * with the containers back to back in that order; origos_xy[i][2], pose_hints[i][3], map_without_matching[i], active[i],
 * out[i].  pose_hints NULL: every member chains from its own lastScanMatchPose.  active NULL: all 1.  A scan with
 * active[i] == 0 is not taken: nothing of that member changes (state, planes, cached and resident container, counters), its
 * record is all zero except n_points = -1, and in the container form its n_points[i] must be 0 -- ragged logs and robots
 * with different scan rates.
 * Equivalence: after a call each member's records, lslam_hector_state, planes on every level, cached and resident
 * container are the bits lslam_hector_process_many[_points] gives on that member alone over its active scans in step
 * order, whenever both launch the same form of the matcher.  The form follows the call's capacity (n_readings; in the
 * container form the longest container of the whole call) and the members' common LSLAM_GN_THREADS.  A member's `scans` and
 * `map_updates` counters advance by its active scans; its `calls` and `host_syncs` do not move: the fleet counts those.
 * One host synchronisation per call, plus one in a ranges-form call that meets a new scan geometry (the cos / sin table,
 * kept with member 0's map).  Inputs go up through pinned staging of the fleet's own.
 * Members may differ in map size, cell length, offset and number of levels.
 * LSLAM_ERR_INVALID_ARGUMENT: NULL pointers, n_members < 1, negative counts (without a device); the same processor twice, two
 * members on one map, members of different contexts; active[i] == 0 with n_points[i] != 0.  LSLAM_ERR_UNSUPPORTED (with a
 * message): more than 4096 members, maps created under different LSLAM_GN_THREADS, an LSLAM_MAP_OPT_ORDERED_SUMS map, more
 * than 8 levels, more than 65536 readings or points per scan.  Nothing is enqueued by a refused call. */
typedef struct lslam_hector_fleet lslam_hector_fleet;
int lslam_hector_fleet_create(lslam_hector* const* members, int n_members, lslam_hector_fleet** out);
void lslam_hector_fleet_destroy(lslam_hector_fleet* f);
int lslam_hector_fleet_size(const lslam_hector_fleet* f);
int lslam_hector_fleet_process_many(lslam_hector_fleet* f, const lslam_hector_scan* scan, int n_steps, int n_readings,
                                    const float* ranges, int ranges_stride, const float* pose_hints,
                                    const uint8_t* map_without_matching, const uint8_t* active, lslam_hector_record* out);
int lslam_hector_fleet_process_many_points(lslam_hector_fleet* f, int n_steps, const float* points_xy, const int32_t* n_points,
                                           const float* origos_xy, const float* pose_hints,
                                           const uint8_t* map_without_matching, const uint8_t* active, lslam_hector_record* out);
/* out = {steps, member-scans processed, map updates made, calls that processed steps, waits for the stream, launches of the
 * fleet's four kernels (copies and the clearing of an exhausted key plane are not launches of them)} */
int lslam_hector_fleet_stats(const lslam_hector_fleet* f, int64_t out[6]);

/* The fleet's GATED forms: the clouds of lslam_hector_process_many_clouds[_dev] and the raw messages of
 * lslam_hector_process_many_synced, for R robots per launch.  Entry i = step * R + member is TAKEN iff active[i] != 0 (NULL:
 * all) and its take word says so (none: `active` alone decides); an entry that is not taken -- masked by the host or refused
 * on the device -- changes nothing of its member and gives the record that is all zero except n_points = -1.  A member of
 * which nothing is taken in a call is unchanged: state, cached and resident container, counters, every plane (a resident
 * container that a longer scan makes grow is moved, not dropped: the single processor's gated forms drop it).  A step is the
 * chain cloud -> container, match, mark, apply: 4 launches whatever R is; lslam_hector_fleet_stats counts them like the
 * ungated ones.  One host synchronisation per call.  A member's `scans` / `map_updates` and the fleet's advance by the taken
 * scans.  Equivalence: after the call member m is bit for bit what lslam_hector_process_many_clouds[_dev] /
 * lslam_hector_process_many_synced leaves when run on it alone over its active entries in step order; either route may
 * continue after the other.  Refused before anything is enqueued, with no processor changed: what
 * lslam_hector_fleet_process_many refuses.
 *
 * Host form: xyz[n_steps * R][n_points][3], valid[n_steps * R][n_points] (NULL: every point), take[n_steps * R] (NULL: all).
 * Rows of entries with active[i] == 0 are not used. */
int lslam_hector_fleet_process_many_clouds(lslam_hector_fleet* f, const lslam_hector_scan* scan, int n_steps, int n_points,
                                           const float* xyz, const uint8_t* valid, const uint8_t* take, const float* pose_hints,
                                           const uint8_t* map_without_matching, const uint8_t* active, lslam_hector_record* out);
/* Clouds in HBM: xyz_dev, valid_dev and take_dev are HOST arrays of R device pointers, one block per member -- R separate
 * lslam_msync_scans_dev outputs or slices of one block.  Member m's cloud of step k is at xyz_dev[m] + k * n_points * 3, its
 * valid flags at valid_dev[m] + k * n_points, its take word (taken iff > 0) at take_dev[m] + k * take_stride, take_stride in
 * int32 words (22 on &records[0].status of lslam_msync_record).  valid_dev or single entries of it may be NULL (every point
 * valid); take_dev or single entries of it may be NULL (every scan taken).  Pointers of entries with active[i] == 0 are not
 * read.  Only hints, flags and `active` go up. */
int lslam_hector_fleet_process_many_clouds_dev(lslam_hector_fleet* f, const lslam_hector_scan* scan, int n_steps, int n_points,
                                               const float* const* xyz_dev, const uint8_t* const* valid_dev,
                                               const int32_t* const* take_dev, int take_stride, const float* pose_hints,
                                               const uint8_t* map_without_matching, const uint8_t* active,
                                               lslam_hector_record* out);
/* Raw messages in: syncs[R] are the members' lesson5 nodes (IMU and odometry pushed into each before).  Member m's
 * callbacks of the call are its steps with active[i] != 0, in step order; ranges row i, stamps[i], time_increments[i],
 * imu_seen[i], odom_seen[i] (NULL: every message pushed to that member's handle so far) are read for those only.  Entries with
 * active[i] == 0 give the not-taken out[i] and an all-zero sync_records[i] (may be NULL).  One laser header and one
 * n_readings for the whole fleet.  The synchronisation runs for all members at once: S = 5 launches per call (queued rows,
 * walk, windows, ONE k_deskew_batch, blank) whatever R and n_steps are, plus the angle table when the scan geometry is new;
 * the buffers of the call and a lazily created lslam_deskew are the fleet's, a handle keeps what outlives a call (queues,
 * state, queued scan, scan_count, the *_seen counters).  A member handle's n_callbacks and corrected / refused counts advance;
 * its `launches` do not move (lslam_hector_fleet_sync_stats counts them).  After a fleet call lslam_msync_read_windows on a
 * member handle is LSLAM_ERR_UNSUPPORTED until that handle's next call of its own (the windows live in the fleet's buffer).
 * Refused before anything is enqueued, with no processor and no lslam_msync handle changed (the *_seen counters included):
 * LSLAM_ERR_INVALID_ARGUMENT -- NULL handles or arrays (without a device), the same lslam_msync twice or one of another
 * context, and for any member what lslam_msync_scans_dev refuses (another n_readings than that handle's first scan's, *_seen
 * that decrease or exceed the pushed count); LSLAM_ERR_UNSUPPORTED -- what lslam_hector_fleet_process_many refuses, more than
 * 65535 callbacks over all members in one call (k_deskew_batch takes a scan per grid row: make shorter calls), IMU windows
 * whose summed room exceeds INT_MAX samples.  The processors' side of the call -- pending map updates flushed, every buffer
 * reserved -- is made ready before the nodes walk a callback, so an allocation failure leaves the nodes where they were too.
 * NOT atomic: a HIP error once launches are under way (LSLAM_ERR_HIP, e.g. from the clearing of an exhausted key plane
 * between two steps); the nodes have then walked the call's callbacks, as after such an error in
 * lslam_hector_process_many_synced.  A handle that was reset (lslam_msync_reset keeps its buffers) may continue with scans of
 * any length. */
int lslam_hector_fleet_process_many_synced(lslam_hector_fleet* f, struct lslam_msync* const* syncs, const lslam_hector_scan* scan,
                                           const struct lslam_msync_laser* laser, int n_steps, int n_readings, const float* ranges,
                                           int ranges_stride, const double* stamps, const float* time_increments,
                                           const int64_t* imu_seen, const int64_t* odom_seen, const float* pose_hints,
                                           const uint8_t* map_without_matching, const uint8_t* active, lslam_hector_record* out,
                                           struct lslam_msync_record* sync_records);
/* out = {synced calls, launches of the fleet's synchronisation kernels and its k_deskew_batch (5 per call that has a
 * callback), growths of the synchronisation's buffers, host waits (one per call)} */
int lslam_hector_fleet_sync_stats(const lslam_hector_fleet* f, int64_t out[4]);

/* ---------------------------------------------------------------------------------------- */
/* Hector localisation: write a pyramid level; track R robots on ONE finished map per launch   */
/* ---------------------------------------------------------------------------------------- */
/* The inverse of lslam_map_read_logodds / lslam_map_cells_dev_ptr: sx*sy floats, row-major y*size_x+x, copied bit for bit (NaN,
 * +-inf and -0.0 included).  Like every reader the call first enqueues a pending pipelined apply; the cached and resident
 * containers, the update factors and every counter stay as they were.  The per-cell "touched by this scan" marks need no
 * reset: they carry the epoch of the scan that made them, and every later scan compares against a larger one.
 * The host form returns when the plane is written; the _dev form is asynchronous on lslam_stream(), and another map's
 * lslam_map_cells_dev_ptr of the same context and level size is a legal source (the device-to-device snapshot).
 * LSLAM_ERR_INVALID_ARGUMENT, map unchanged: a NULL pointer, a level out of range, a _dev source the runtime knows not to be
 * device memory. */
int lslam_map_write_logodds(lslam_map* map, int level, const float* src_host);
int lslam_map_write_logodds_dev(lslam_map* map, int level, const float* src_dev);

/* R trackers on one BORROWED map (destroy the localiser first).  A taken entry is HectorSlamProcessor::update (:81-108) with the
 * gate never firing: newPose = matchData(hint or lastScanMatchPose, container); lastScanMatchPose / lastScanMatchCov set; no
 * updateByScan -- bit for bit the records and state of a lslam_hector processor on the same map with both thresholds +inf, run
 * alone over the tracker's taken entries, whenever both launch the same form of the matcher (the form follows the capacity of
 * the CALL and the map's LSLAM_GN_THREADS, as the streamed processor's).  The map is only read: every plane, the cached and
 * resident containers, their origo and lslam_map_cached_points are what they were; between calls the map may change through
 * any lslam_map_* / lslam_hector_* call, and the next call sees it as it then is.
 * Indexing is the fleet's: entry i = step * R + tracker for the ranges rows, the containers (back to back), pose_hints[i][3],
 * active[i], out[i] and the take words.  pose_hints NULL: every tracker chains from its own last pose; active NULL: all
 * active.  An entry is taken iff it is active and -- cloud forms -- its take flag / word is > 0 (lslam_msync_record::status
 * with take_stride = sizeof(lslam_msync_record) / 4 serves as it stands).  An entry that is not taken changes nothing of its
 * tracker; its record is all zero with n_points = -1.  `updated` is always 0.  An empty container returns the start pose and
 * leaves the covariance as it was (ScanMatcher.h:96).
 * A call is cut into chunks of LSLAM_HECTOR_LOC_OPT_MAX_STEPS_PER_LAUNCH steps (0 = the default: as many as keep the chunk's
 * container block within 64 MiB, at least 1); a chunk is 2 launches (containers of every entry; one block per tracker walking
 * its entries in step order), 1 in the container form, whatever R and the steps are, and chunking changes no bit.  ONE host
 * synchronisation per call, plus one in a ranges-form call that meets a new scan geometry.
 * LSLAM_ERR_INVALID_ARGUMENT (no device needed): NULL handles or required arrays, n_trackers < 1, negative counts, first /
 * count out of range, n_readings < 1 in the ranges form, a container-form entry with active == 0 and n_points != 0.
 * LSLAM_ERR_UNSUPPORTED: LSLAM_MAP_OPT_ORDERED_SUMS maps, more than 8 levels, more than 65536 readings or points per scan,
 * more than 65535 trackers.  n_steps == 0 is LSLAM_OK and does nothing. */
typedef struct lslam_hector_loc lslam_hector_loc;
enum { LSLAM_HECTOR_LOC_OPT_MAX_STEPS_PER_LAUNCH = 1 };
int lslam_hector_loc_create(lslam_map* map, int n_trackers, lslam_hector_loc** out);
void lslam_hector_loc_destroy(lslam_hector_loc* l);
int lslam_hector_loc_size(const lslam_hector_loc* l);
/* lastScanMatchPose of trackers first .. first+count-1 (after create: 0, 0, 0; lastScanMatchCov: zero) */
int lslam_hector_loc_set_poses(lslam_hector_loc* l, int first, int count, const float* poses_xyh);
int lslam_hector_loc_state(lslam_hector_loc* l, int tracker, float pose[3], float cov[9]);
int lslam_hector_loc_set_option(lslam_hector_loc* l, int option, int value);
int lslam_hector_loc_process_many(lslam_hector_loc* l, const lslam_hector_scan* scan, int n_steps, int n_readings,
                                  const float* ranges, int ranges_stride, const float* pose_hints, const uint8_t* active,
                                  lslam_hector_record* out);
int lslam_hector_loc_process_many_points(lslam_hector_loc* l, int n_steps, const float* points_xy, const int32_t* n_points,
                                         const float* pose_hints, const uint8_t* active, lslam_hector_record* out);
int lslam_hector_loc_process_many_clouds(lslam_hector_loc* l, const lslam_hector_scan* scan, int n_steps, int n_points,
                                         const float* xyz, const uint8_t* valid, const uint8_t* take, const float* pose_hints,
                                         const uint8_t* active, lslam_hector_record* out);
/* clouds in HBM: xyz_dev [n_steps * R][n_points][3], valid_dev [n_steps * R][n_points] or NULL, take_dev int32 words
 * take_stride apart or NULL */
int lslam_hector_loc_process_many_clouds_dev(lslam_hector_loc* l, const lslam_hector_scan* scan, int n_steps, int n_points,
                                             const float* xyz_dev, const uint8_t* valid_dev, const int32_t* take_dev,
                                             int take_stride, const float* pose_hints, const uint8_t* active,
                                             lslam_hector_record* out);
/* out = {steps, tracker-scans matched, calls, waits for the stream, kernel launches, launches of the tracking kernel} */
int lslam_hector_loc_stats(const lslam_hector_loc* l, int64_t out[6]);

/* ---------------------------------------------------------------------------------------- */
/* lesson5 lidar motion de-skew (LidarUndistortion::CorrectLaserScan, lesson5/src/            */
/* lidar_undistortion.cc:339-447) -- SURVEY 8(f) #4.  Pinned (round 4) against the reference's */
/* own source compiled in place behind ROS / tf / PCL / Eigen stand-ins (oracle/shim, which    */
/* define PCL's getTransformation formula and Eigen 3.3's evaluation orders; tests/            */
/* test_deskew_pin.py): <= 4e-6 m (float32 cos / sin of the Euler angles from the device libm).*/
/* ---------------------------------------------------------------------------------------- */
typedef struct lslam_deskew_params {
  float angle_min, angle_increment, range_min, range_max; /* sensor_msgs/LaserScan header */
  double scan_time_start, time_increment;                 /* header.stamp, time_increment (:154-155) */
  int32_t use_imu, use_odom;
  double start_odom_time, end_odom_time;                  /* :300-301 */
  float odom_incre_x, odom_incre_y, odom_incre_z, pad;    /* :331-334 */
} lslam_deskew_params;
/* imu_time / imu_rot_*: the integrated gyro samples of this scan (imu_time_[0..current_imu_index_], :205-243),
 * n_imu = current_imu_index_ + 1.  out_xyz: n x 3 float32 (zeros for the beams the reference skips), out_valid: n */
int lslam_deskew_scan(lslam_context* ctx, const float* ranges, int n, const lslam_deskew_params* params,
                      const double* imu_time, const double* imu_rot_x, const double* imu_rot_y, const double* imu_rot_z,
                      int n_imu, float* out_xyz, uint8_t* out_valid);
/* BATCHED de-skew: n_scans scans of one geometry per launch, grid (tiles of 256 beams x scans).  Every scan's output is
 * bit for bit what lslam_deskew_scan returns for that scan alone (both kernels run one __device__ body).  The handle owns
 * every device and pinned buffer a call needs -- a call of a shape it has seen allocates nothing -- and the double cos / sin
 * table of the beam angles (CreateAngleCache, :162-173), computed on the device once per (angle_min, angle_increment,
 * n_readings) and kept until another geometry arrives (a table of more beams serves a shorter scan of the same angles).
 * ranges: row k at ranges + k * ranges_stride.  params[n_scans]: angle_min, angle_increment, range_min and range_max must
 * be equal across one call (LSLAM_ERR_INVALID_ARGUMENT otherwise).  imu_first[n_scans + 1]: scan k owns the integrated
 * samples [imu_first[k], imu_first[k+1]) of imu_time / imu_rot_* -- the state PruneImuDeque leaves, as for
 * lslam_deskew_scan; a scan with use_imu = 0 may own none, one with use_imu = 1 must own at least one.
 * out_xyz: n_scans x n_readings x 3 float32, out_valid: n_scans x n_readings.  n_scans == 0 is LSLAM_OK and launches
 * nothing.  At most 65535 scans per call.
 * The _dev form takes ranges, out_xyz and out_valid in HBM (params, imu_first and the IMU arrays stay host arrays and have
 * been copied when it returns), is ASYNCHRONOUS on lslam_stream() and makes no host wait: its small inputs go up through a
 * ring of 4 pinned slots, and only a caller more than 4 unfinished calls ahead of the device waits for one (counted). */
typedef struct lslam_deskew lslam_deskew;
int lslam_deskew_create(lslam_context* ctx, lslam_deskew** out);
void lslam_deskew_destroy(lslam_deskew* d);
int lslam_deskew_batch(lslam_deskew* d, int n_scans, int n_readings, const float* ranges, int ranges_stride,
                       const lslam_deskew_params* params, const int32_t* imu_first, const double* imu_time,
                       const double* imu_rot_x, const double* imu_rot_y, const double* imu_rot_z, float* out_xyz,
                       uint8_t* out_valid);
int lslam_deskew_batch_dev(lslam_deskew* d, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride,
                           const lslam_deskew_params* params, const int32_t* imu_first, const double* imu_time,
                           const double* imu_rot_x, const double* imu_rot_y, const double* imu_rot_z, float* out_xyz_dev,
                           uint8_t* out_valid_dev);
/* out = {scans de-skewed, kernel launches (the angle table's included), buffer growths (device or pinned), host waits}.  A
 * second call of a shape already seen reports no new growth; the host form waits once per call, at its end. */
int lslam_deskew_stats(const lslam_deskew* d, int64_t out[4]);

/* ---------------------------------------------------------------------------------------- */
/* lesson5 IMU / odometry synchronisation: the FRONT half of LidarUndistortion::ScanCallback  */
/* (lesson5/src/lidar_undistortion.cc:96-125) on the device, chained into the de-skew launch  */
/* above.  Raw sensor_msgs/Imu, nav_msgs/Odometry and LaserScan messages go in, de-skewed      */
/* clouds come out; the host stages no per-scan motion data.  The handle owns the node's state */
/* in HBM: imu_queue_ and odom_queue_ (doubles), their fronts, start_odom_msg_ / end_odom_msg_ */
/* as global message indices (-1: the default-constructed message, stamp 0, identity pose),    */
/* the one LaserScan CacheLaserScan keeps queued, and scan_count_.                             */
/* ---------------------------------------------------------------------------------------- */
#define LSLAM_MSYNC_QUEUED 0              /* the first scan ever: only queued (:145-146) */
#define LSLAM_MSYNC_CORRECTED 1
#define LSLAM_MSYNC_WAIT_IMU (-1)         /* PruneImuDeque refused (:182-188, :199-200) */
#define LSLAM_MSYNC_WAIT_ODOM (-2)        /* PruneOdomDeque refused (:257-263, :274-275) */
#define LSLAM_MSYNC_IMU_NO_LEAD_SAMPLE (-3) /* a sample inside the scan and none before its start: :237 reads imu_time_[-1] */
#define LSLAM_MSYNC_IMU_OVERFLOW (-4)     /* more than LSLAM_MSYNC_QUEUE_LENGTH integrated samples: past imu_time_'s end */
#define LSLAM_MSYNC_QUEUE_LENGTH 2000     /* queueLength (:20) */
/* One record per scan callback.  Callback k corrects the scan of callback k - 1 (CacheLaserScan's one-scan lag, :142-156);
 * a scan that a Prune* step refuses has left laser_queue_ and is dropped, not retried, and IMU pops made before an odometry
 * refusal stay made. */
typedef struct lslam_msync_record {
  int32_t status;                          /* LSLAM_MSYNC_* */
  int32_t n_imu;                           /* current_imu_index_ + 1 (0: no sample in reach, corrected with zero rotation) */
  double scan_time_start, time_increment;  /* of the scan this callback took off the queue (:154-155); 0 when QUEUED */
  double start_odom_time, end_odom_time;   /* :301-302 */
  float odom_incre[3], pad;                /* :332-334 */
  int64_t imu_front, odom_front;           /* messages popped so far, after this callback (:191-197, :266-272) */
  int64_t start_odom_index, end_odom_index;/* start_odom_msg_ / end_odom_msg_ after this callback, -1: the default message */
} lslam_msync_record;
typedef struct lslam_msync_laser {         /* the LaserScan header of the scans one call corrects */
  float angle_min, angle_increment, range_min, range_max;
} lslam_msync_laser;
typedef struct lslam_msync lslam_msync;
/* the node's constructor with its use_imu / use_odom parameters (:27-28); _reset brings the handle back to a fresh node
 * (it waits for the stream; the buffers, and with them the growth and wait counts, are kept) */
int lslam_msync_create(lslam_context* ctx, int use_imu, int use_odom, lslam_msync** out);
void lslam_msync_destroy(lslam_msync* h);
int lslam_msync_reset(lslam_msync* h);
/* n ImuCallbacks (:82-86) / OdomCallbacks (:89-93): stamps[n], gyro_xyz[n][3] (angular_velocity), pos_xyz[n][3],
 * quat_xyzw[n][4].  The messages are appended to the device queue by an asynchronous copy on lslam_stream(): no kernel, and
 * no host wait unless the pinned staging area is still in flight (counted).  Messages a finished call has popped are
 * discarded when room is needed; the buffers grow when they must (counted). */
int lslam_msync_push_imu(lslam_msync* h, int n, const double* stamps, const double* gyro_xyz);
int lslam_msync_push_odom(lslam_msync* h, int n, const double* stamps, const double* pos_xyz, const double* quat_xyzw);
/* n_msgs ScanCallbacks (:96-125) in order.  ranges: row k at ranges + k * ranges_stride, stamps[k] = header.stamp,
 * time_increments[k] the message's float32 field.  imu_seen[k] / odom_seen[k]: how many IMU / odometry messages, counted
 * since create or reset, had arrived when callback k ran -- the interleaving of the callbacks; non-decreasing, also across
 * calls, and at most what has been pushed; NULL = every message pushed so far.  laser: the header of the corrected scans
 * (the angle cache is the first scan's, :129-137, so one geometry).  n_readings must equal the handle's first scan's, which
 * fixes scan_count_.
 * out_xyz[n_msgs][n_readings][3], out_valid[n_msgs][n_readings]: row k is the cloud of the scan callback k corrected, that
 * is message k - 1, row 0 the scan the previous call left queued; rows of queued or refused callbacks are zeros with
 * valid 0.  records[n_msgs] (may be NULL).
 * Per call: k_msync_walk (one wave, the callbacks in order), k_msync_windows (one wave per callback: PruneImuDeque's
 * integration, bit for bit imu_time_ / imu_rot_*, and PruneOdomDeque's increment), lslam_deskew's own k_deskew_batch on
 * the records they wrote, and k_msync_blank.  The host form waits once, at its end.  The _dev form takes ranges, out_xyz,
 * out_valid and records in HBM, is asynchronous on lslam_stream() and makes no host wait (stamps, time_increments and the
 * *_seen arrays stay host arrays and have been copied when it returns).
 * Refused with LSLAM_ERR_INVALID_ARGUMENT, nothing enqueued and no state changed: what lslam_deskew_batch refuses, a deskew
 * handle of another context, another n_readings than the first scan's, *_seen that decrease or exceed the pushed count.
 * LSLAM_ERR_UNSUPPORTED: more than 65535 callbacks per call. */
int lslam_msync_scans(lslam_msync* h, lslam_deskew* deskew, const lslam_msync_laser* laser, int n_msgs, int n_readings,
                      const float* ranges, int ranges_stride, const double* stamps, const float* time_increments,
                      const int64_t* imu_seen, const int64_t* odom_seen, float* out_xyz, uint8_t* out_valid,
                      lslam_msync_record* records);
int lslam_msync_scans_dev(lslam_msync* h, lslam_deskew* deskew, const lslam_msync_laser* laser, int n_msgs, int n_readings,
                          const float* ranges_dev, int ranges_stride, const double* stamps, const float* time_increments,
                          const int64_t* imu_seen, const int64_t* odom_seen, float* out_xyz_dev, uint8_t* out_valid_dev,
                          lslam_msync_record* records_dev);
/* Debug read-back of the LAST call's integrated samples (imu_time_ / imu_rot_* of :207-243), for the parity tests: callback k
 * owns [imu_first[k], imu_first[k + 1]) of imu_time[] and imu_rot_xyz[][3]; imu_first has n_msgs + 1 entries.  With
 * capacity 0 only imu_first is filled (to size the arrays); a capacity below imu_first[n_msgs] is refused.  Waits. */
int lslam_msync_read_windows(lslam_msync* h, int32_t* imu_first, double* imu_time, double* imu_rot_xyz, int capacity);
/* out = {scan callbacks, scans corrected, scans refused, launches of the three msync kernels, buffer growths (device or
 * pinned), host waits}.  The two scan counts come from the device and wait for the calls enqueued so far. */
int lslam_msync_stats(lslam_msync* h, int64_t out[6]);

/* ---------------------------------------------------------------------------------------- */
/* lesson4 GMapping hit/visit count map (lesson4_gmapping_node: GMapping::ComputeMap /        */
/* PublishMap, lesson4/src/gmapping/gmapping.cc:127-242, over ScanMatcherMap = G/map.h +      */
/* G/harray2d.h, traced by GridLineTraversal::gridLine, G/gridlinetraversal.h; short name     */
/* G/ = lesson4/include/lesson4/gmapping/grid/).  Storage is mapSize = (ceil(W/delta)>>5)<<5  */
/* cells per axis in 32x32 patches; per cell visits, n (hits) and the float hit-position sum  */
/* acc.  Pinned bit for bit (tests/test_gmapping_pin.py, tests/test_gmapping_gpu.py) against  */
/* the reference's header classes driven through the node's callback sequence.               */
/*  - The node publishes info.width = (uint32)((xmax - xmin) / resolution) with the float32   */
/*    MapMetaData.resolution: 1599 for its own +-40 m / 0.05 box, one column short of the      */
/*    1600-cell storage, and its PublishMap loop then writes data[width*y + x] past the end.  */
/*    Here the width is taken with the double delta, (uint32)((xmax - xmin) / delta): 1600.   */
/*  - Accumulation at poses (GMapping's registerScan use) is our contract: pose (x, y, theta) */
/*    with c, s = sincos(theta) from the host libm, endpoint                                    */
/*      phit.x = x + d*(c*cos_i - s*sin_i),  phit.y = y + d*(s*cos_i + c*sin_i)               */
/*    in fp64 without contraction, p0 = world2map(x, y).  At pose (0,0,0) this IS the node's  */
/*    phit = lp + d*(cos_i, sin_i) bit for bit (1*a - 0*b == a).  Scans apply in order: the   */
/*    hits of scan k come before those of scan k+1 in every cell's acc sum.  Cells outside    */
/*    [0, mapSize) are skipped and counted (the reference indexes patch (-1,-1) there).       */
/* ---------------------------------------------------------------------------------------- */
typedef struct lslam_gmap lslam_gmap;
typedef struct lslam_gmap_geometry {
  int32_t map_size_x, map_size_y; /* storage: getMapSizeX/Y (G/map.h:79-80)  */
  int32_t width, height;          /* published nav_msgs/OccupancyGrid (see above) */
  int32_t size_x2, size_y2;       /* m_sizeX2 = round((center - xmin)/delta) (G/map.h:141-142) */
  int32_t patches_x, patches_y;   /* 32x32 patches (HierarchicalArray2D, G/harray2d.h:75-80) */
  double center_x, center_y, delta;
} lslam_gmap_geometry;
/* ScanMatcherMap gmapping_map_(center, xmin, ymin, xmax, ymax, delta) (gmapping.cc:130-135; G/map.h:133-143).
 * LSLAM_ERR_INVALID_ARGUMENT for delta <= 0, xmax <= xmin, ymax <= ymin or fewer than 32 cells on an axis (no patch);
 * LSLAM_ERR_UNSUPPORTED when the published grid is narrower or lower than the storage (the node would write out of
 * bounds) or an axis has more than 65504 cells (mapSize^2 must stay below 2^32).  All counters start at zero. */
int lslam_gmap_create(lslam_context* ctx, double xmin, double ymin, double xmax, double ymax, double delta, lslam_gmap** out);
void lslam_gmap_destroy(lslam_gmap* map);
int lslam_gmap_info(const lslam_gmap* map, lslam_gmap_geometry* out);
/* GMapping::CreateCache (gmapping.cc:112-124) + the InitParams maxRange / maxUrange (:46-49): angle_i = angle_min +
 * i * angle_increment in FLOAT (the message's float32 fields, unsigned i), cos / sin in double by the host libm's sincos
 * (what g++ -O2 makes of the node's cos / sin pair; glibc's sincos can differ from its cos in the last bit).  The
 * node takes the cache from its first scan only; calling this again replaces it.  Integrating before it is
 * LSLAM_ERR_INVALID_ARGUMENT. */
int lslam_gmap_set_laser(lslam_gmap* map, int n_beams, float angle_min, float angle_increment, double max_range,
                         double max_use_range);
/* the cached cos_i / sin_i (n_beams each) */
int lslam_gmap_angle_cache(const lslam_gmap* map, double* cos_out, double* sin_out);
/* every counter, the patch mask and the stats back to zero (clears the marked patches only) */
int lslam_gmap_reset(lslam_gmap* map);
/* n_scans x n_beams float32 ranges, scan-major; poses n_scans x (x, y, theta) or NULL = all at (0, 0, 0).  Per beam
 * (ComputeMap, gmapping.cc:171-242): skip d > maxRange, d == 0, non-finite; clamp d to maxUrange; visits++ on every
 * gridLine(p0, p1) point but the last; if d < maxUrange a hit at p1: n++, visits++, acc += (float)phit.  Free updates of
 * a batch come before its hits (integer counts do not care); hits add in (scan, beam) order.  At most 2^28 readings
 * (n_scans * n_beams) per call: LSLAM_ERR_INVALID_ARGUMENT beyond; a map takes any number of calls. */
int lslam_gmap_integrate(lslam_gmap* map, int n_scans, const float* ranges, const double* poses);
/* GMapping::ScanCallback's map work in one call: reset + integrate one scan at the origin + read_ros_i8.
 * out: width x height int8, row-major y * width + x. */
int lslam_gmap_compute_map(lslam_gmap* map, const float* ranges, double occ_thresh, int8_t* out);
/* PublishMap (gmapping.cc:141-159): storage cells -1 (visits == 0), 100 ((double)n / visits > occ_thresh), 0 otherwise;
 * published cells beyond the storage 0 (data.resize, :80).  out: width x height int8. */
int lslam_gmap_read_ros_i8(lslam_gmap* map, double occ_thresh, int8_t* out);
/* map_size_x * map_size_y counters, row-major y * map_size_x + x; acc_xy = all acc.x, then all acc.y (2 x cells).
 * Any pointer may be NULL. */
int lslam_gmap_read_counters(lslam_gmap* map, int32_t* visits, int32_t* n, float* acc_xy);
/* patches_y x patches_x bytes, 1 = active: the patch holds a free point of a line or a hit cell (setActiveArea,
 * gmapping.cc:207-224) of any scan since the last reset */
int lslam_gmap_read_patch_mask(lslam_gmap* map, uint8_t* out);
/* since the last reset: scans, beams used (past the range filter), hits applied, cell updates dropped outside */
int lslam_gmap_stats(lslam_gmap* map, int64_t out[4]);

/* ---------------------------------------------------------------------------------------- */
/* lesson1 curvature corner extraction (LaserScan::ScanCallback, lesson1/src/                */
/* feature_detection.cc:77-179): compact the finite ranges, an 11-point range curvature, the  */
/* 20 sharpest points of each sixth of the scan.  Pinned BIT FOR BIT against the reference's  */
/* own source (tests/golden/features_golden.npz, tests/test_features_gpu.py).                 */
/*  1. Beams with a non-finite range (NaN, +-inf) are dropped; zero and negative ranges stay.  */
/*     v[0..count) are the rest in order, map[i] their original beam index.                    */
/*  2. For 5 <= i < count-5, in float32, left to right, every operation rounded:               */
/*       d = v[i-5]+v[i-4]+v[i-3]+v[i-2]+v[i-1] - v[i]*10 + v[i+1]+v[i+2]+v[i+3]+v[i+4]+v[i+5] */
/*       c[i] = d*d;  c = 0 at every other compacted index.                                    */
/*  3. Sector j = 0..5 is [s, e] with s = count*j/6, e = count*(j+1)/6 - 1 (integers); a sector */
/*     with s >= e is skipped whole.                                                           */
/*  4. The reference sorts [s, e) -- without e -- and walks from e down: element e is picked   */
/*     whenever c[e] > threshold, whatever its value, and uses one of the sector's 20 slots;   */
/*     the other slots go to the largest c > threshold of [s, e), in descending order.         */
/*  5. TIE RULE (this library's; the reference's order among equal curvatures is whatever its   */
/*     unstable std::sort leaves): among equal curvatures the HIGHER compacted index ranks      */
/*     first.  Where no equal curvatures straddle a sector's cut-off the picks are the          */
/*     reference's; the number of picks per sector is the reference's everywhere.               */
/* ---------------------------------------------------------------------------------------- */
#define LSLAM_FEATURE_SECTORS 6
#define LSLAM_FEATURE_PICKS 20          /* per sector */
#define LSLAM_FEATURE_MAX_READINGS 1500 /* max_scan_count, feature_detection.cc:23 */
typedef struct lslam_feature_record {
  int32_t n_valid;       /* count: the finite beams */
  int32_t n_corners;     /* the sum of per_sector */
  int32_t per_sector[6]; /* picks of each sector, 0..20 */
} lslam_feature_record;  /* 32 bytes */
typedef struct lslam_features lslam_features;
int lslam_features_create(lslam_context* ctx, lslam_features** out);
void lslam_features_destroy(lslam_features* f);
/* edge_threshold_ (:69), 1.0f by default.  NaN or below 0 -> LSLAM_ERR_INVALID_ARGUMENT (there the reference would pick
 * its value-initialised entries). */
int lslam_features_set_threshold(lslam_features* f, float edge_threshold);
/* n_scans scans of n_readings beams in ONE launch (a workgroup per scan, everything per scan in LDS); row k of ranges at
 * ranges + k * ranges_stride -- the block layout lslam_matcher_match_batch_dev_f32 and lslam_deskew_batch_dev take.
 *  out_ranges    n_scans x n_readings float32, may be NULL: the reference's published corner_scan.ranges (its first
 *                n_readings entries): the range of every pick at its beam, +0.0f elsewhere
 *  out_index     n_scans x 120 int32: ORIGINAL beam indices; sector j owns slots [20j, 20j+20): element e first if it was
 *                picked, then descending curvature (ties by the rule above); unused slots are -1
 *  out_rec       n_scans records
 *  out_curvature n_scans x n_readings float32, may be NULL: c scattered to the original beam index, 0 elsewhere
 * n_scans == 0 is LSLAM_OK and launches nothing; n_readings == 0 is LSLAM_OK and leaves every scan empty (all slots -1, a
 * zero record).  At most 65535 scans per call and LSLAM_FEATURE_MAX_READINGS beams per scan (LSLAM_ERR_UNSUPPORTED beyond:
 * the reference's stack arrays end there).  The handle owns every buffer the host form needs: a repeated shape allocates
 * nothing, and the call waits once, at its end.  The _dev form takes ranges and every out_* in HBM, is ASYNCHRONOUS on
 * lslam_stream() and makes no host wait; every scan of a batch is bit for bit the same scan run alone. */
int lslam_features_batch(lslam_features* f, int n_scans, int n_readings, const float* ranges, int ranges_stride,
                         float* out_ranges, int32_t* out_index, lslam_feature_record* out_rec, float* out_curvature);
int lslam_features_batch_dev(lslam_features* f, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride,
                             float* out_ranges_dev, int32_t* out_index_dev, lslam_feature_record* out_rec_dev,
                             float* out_curvature_dev);
/* out = {scans extracted, kernel launches, buffer growths (device or pinned), host waits} */
int lslam_features_stats(const lslam_features* f, int64_t out[4]);

/* ---------------------------------------------------------------------------------------- */
/* lesson3 PL-ICP scan-to-scan matching (ScanMatchPLICP: lesson3/src/scan_match_plicp.cc and  */
/* lesson3/src/plicp_odometry.cc, "O/" below), many pairs per launch, and the node's keyframe */
/* odometry for many tracks per launch.                                                       */
/* STANDING: PARITY WITH THE REFERENCE IS UNPINNED.  Its arithmetic lives in the un-vendored   */
/* third-party library csm (sm_icp).  The results are DEFINED by this          */
/* project's own fp64 restatement of the published algorithm (A. Censi, ICRA 2008): `sm_icp`   */
/* in tools/plicp_cpu.py -- exhaustive nearest-neighbour search, duplicate / trimmed /         */
/* adaptive outlier rejection, closed-form point-to-line minimiser.  The wrapper logic of the  */
/* two reference files is followed literally.  All device arithmetic is fp64.                  */
/* Three deliberate rules, and a fourth fact about the definition:                            */
/*  1. RANK TIES: the trimmed cut and the adaptive percentile go by rank; among EQUAL          */
/*     distances the LOWER sens order ranks first (sens order = the reading's position among   */
/*     the valid readings of the sens scan).  The same (distance, sens order) order decides    */
/*     which of two sens points on one ref point survives "remove doubles".                    */
/*  2. INVALID MATCH: where sm_icp reports valid = 0 the reference reads an uninitialised      */
/*     corr_ch (O/:397-423).  Here corr_ch is the IDENTITY and the pose and velocity are left   */
/*     untouched; NewKeyframeNeeded still counts the scan.                                     */
/*  3. LITERAL PREDICTION: GetPrediction (O/:442-456) reads linear.y and linear.z, which        */
/*     nothing ever sets, so the prediction is (v.linear.x < 1e-6 ? 0 : dt * v.linear.x, 0, 0): */
/*     no angular prediction, and a negative speed predicts nothing.                           */
/*  4. THE QUARTIC IS THE LAGRANGE CONDITION of the stated cost: with t eliminated the cost is     */
/*     u^T S u + h^T u on |u| = 1, and in S's eigenbasis (2L+2e0)^2 (2L+2e1)^2 =                  */
/*     hp0^2 (2L+2e1)^2 + hp1^2 (2L+2e0)^2.  All its real roots are tried and the lowest-cost    */
/*     one taken: the solve is the minimum of sum_k (n_k . (R(theta) p_k + t - q_k))^2, held to   */
/*     an independent search of that cost by the tests.  It has no unique answer for 3 or 4      */
/*     correspondences or a scene of exactly two lines.                         */
/* ---------------------------------------------------------------------------------------- */
#define LSLAM_PLICP_MAX_READINGS 2048
/* the sm_params sm_icp reads; defaults = ScanMatchPLICP::InitParams (scan_match_plicp.cc:43-156) */
typedef struct lslam_plicp_params {
  double max_angular_correction_deg; /* 45.0 */
  double max_linear_correction;      /* 1.0 */
  double epsilon_xy;                 /* 0.000001 */
  double epsilon_theta;              /* 0.000001 */
  double max_correspondence_dist;    /* 1.0 */
  double outliers_maxPerc;           /* 0.90 */
  double outliers_adaptive_order;    /* 0.7 */
  double outliers_adaptive_mult;     /* 2.0 */
  int32_t max_iterations;            /* 10 */
  int32_t use_point_to_line_distance; /* 1 */
  int32_t outliers_remove_doubles;   /* 1 */
  int32_t reserved;
} lslam_plicp_params;
void lslam_plicp_params_defaults(lslam_plicp_params* p);
/* sm_result's fields the node reads (scan_match_plicp.cc:285-300).  sm_icp's early exits (fewer than 3 valid readings on a
 * side, fewer than 3 correspondences after either rejection step, a singular solve) give the zero record with error = +inf;
 * a result beyond max_linear_correction / max_angular_correction_deg of the first guess has valid = 0 with x still reported. */
typedef struct lslam_plicp_record {
  double x[3];        /* the pose of the sens scan in the ref scan's frame */
  double error;       /* the sum of squared point-to-line residuals of the last iteration */
  int32_t valid;
  int32_t iterations;
  int32_t nvalid;     /* correspondences of the last iteration */
  int32_t reserved;
} lslam_plicp_record; /* 48 bytes */
typedef struct lslam_plicp lslam_plicp;
int lslam_plicp_create(lslam_context* ctx, const lslam_plicp_params* params, lslam_plicp** out);
void lslam_plicp_destroy(lslam_plicp* h);
/* LaserScanToLDP's header fields (scan_match_plicp.cc:220-261): a reading is valid iff range_min < r < range_max (NaN is
 * invalid), theta_i = angle_min + i * angle_increment in double.  The cos / sin table is built once per geometry, as
 * CreateCache (O/:237-252) does, and kept by the handle. */
int lslam_plicp_set_laser(lslam_plicp* h, double angle_min, double angle_increment, double range_min, double range_max);
/* ScanMatchWithPLICP (scan_match_plicp.cc:266-300) for n_pairs pairs in ONE launch (a workgroup per pair, the iterations loop
 * on the device).  ranges: n_scans rows of n_readings float32, row k at ranges + k * ranges_stride (the matcher's and the
 * de-skew's block layout); pair b matches scan pair_sens[b] against scan pair_ref[b], so a log uploads each scan once.
 * first_guess: n_pairs x 3 doubles, NULL = zeros (as :266-300).  out: n_pairs records.  pair_ref / pair_sens are HOST arrays
 * in both forms.  The host form owns its buffers (a repeated shape allocates nothing) and waits once, at its end.  The _dev
 * form takes ranges, first_guess and out in HBM, is ASYNCHRONOUS on lslam_stream() and makes no host wait -- with one
 * back-pressure: the pair indices go up through a ring of 4 pinned slots, so a call that would reuse a slot whose launch has
 * not finished (the fifth of five queued calls), or that brings more pairs than any call before it (every slot grows), waits
 * for that launch first; such waits are counted in the stats.  A pair's record is
 * byte for byte the same alone and in any batch.  n_pairs == 0 is LSLAM_OK and launches nothing.
 * LSLAM_ERR_INVALID_ARGUMENT, outputs untouched: NULL pointers, a pair index outside [0, n_scans), no laser set.
 * LSLAM_ERR_UNSUPPORTED: more than LSLAM_PLICP_MAX_READINGS readings. */
int lslam_plicp_match_batch(lslam_plicp* h, int n_scans, int n_readings, const float* ranges, int ranges_stride, int n_pairs,
                            const int32_t* pair_ref, const int32_t* pair_sens, const double* first_guess, lslam_plicp_record* out);
int lslam_plicp_match_batch_dev(lslam_plicp* h, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride, int n_pairs,
                                const int32_t* pair_ref, const int32_t* pair_sens, const double* first_guess_dev,
                                lslam_plicp_record* out_dev);
/* ONE iteration of sm_icp from x_in, by the same device code as the batch kernel (host pointers; one launch, one wait).
 * Per reading of the sens scan: j1, j2 = the ref READING indices of the segment (-1 where none), flags bit 0 = valid reading,
 * bit 1 = correspondence accepted before outlier rejection, bit 2 = kept after doubles / trimmed / adaptive rejection.
 * x_out = the solved pose, NaN where the iteration took one of sm_icp's early exits. */
int lslam_plicp_debug_iteration(lslam_plicp* h, const float* ranges_ref, const float* ranges_sens, int n, const double x_in[3],
                                int32_t* j1, int32_t* j2, uint8_t* flags, double x_out[3]);
/* The CLOUD forms: ScanMatchWithPLICP (scan_match_plicp.cc:220-300) on point clouds in the de-skew's layout (what
 * lslam_deskew_batch, lslam_msync_scans[_dev] and lslam_icp_convert_batch write): xyz = n_clouds x n_points x 3 float32, valid =
 * n_clouds x n_points bytes or NULL (every point).  A de-skewed scan's points no longer lie on the nominal beam angles, so it has
 * no ranges form; csm's laser_data carries a theta per reading and sm_icp works on the points alone (cloud_to_ldp in
 * tools/plicp_cpu.py is the definition).  The rules:
 *   - point i takes part iff (valid == NULL or valid[i] != 0) and x[i], y[i] are finite;
 *   - its coordinates are (double)x[i], (double)y[i]: the float32 values widened, no trigonometry; z is ignored, NaN included;
 *   - no range window is applied and no laser is needed: the producer's valid byte already says what the node's
 *     range_min < r < range_max (:231) would;
 *   - the reading index is i: the j1 +- 1 adjacency, "remove doubles" and the (distance, sens order) tie rule go by it exactly as
 *     in the ranges form, so neighbours are scan-order neighbours even where a de-skewed scan's bearings are not monotone.
 * Everything else -- the layout of pair_ref / pair_sens (HOST arrays), first_guess, out, the ring of 4 pinned slots, one launch,
 * the host form waits once and the _dev form (xyz, valid, first_guess, out in HBM) makes no host wait, n_pairs == 0 -- is as
 * lslam_plicp_match_batch[_dev] above.  A pair's record is byte for byte the same alone and in any batch.
 * LSLAM_ERR_INVALID_ARGUMENT, outputs untouched: NULL pointers (valid and first_guess may be NULL), a pair index outside
 * [0, n_clouds).  LSLAM_ERR_UNSUPPORTED: n_points > LSLAM_PLICP_MAX_READINGS. */
int lslam_plicp_match_clouds(lslam_plicp* h, int n_clouds, int n_points, const float* xyz, const uint8_t* valid, int n_pairs,
                             const int32_t* pair_ref, const int32_t* pair_sens, const double* first_guess, lslam_plicp_record* out);
int lslam_plicp_match_clouds_dev(lslam_plicp* h, int n_clouds, int n_points, const float* xyz_dev, const uint8_t* valid_dev, int n_pairs,
                                 const int32_t* pair_ref, const int32_t* pair_sens, const double* first_guess_dev,
                                 lslam_plicp_record* out_dev);
/* lslam_plicp_debug_iteration on two clouds of n points (n x 3 float32 each; the valid bytes may be NULL), under the rules
 * above; j1, j2 and flags are per POINT of the sens cloud.  Host pointers; one launch, one wait. */
int lslam_plicp_debug_iteration_clouds(lslam_plicp* h, const float* ref_xyz, const float* sens_xyz, const uint8_t* ref_valid,
                                       const uint8_t* sens_valid, int n, const double x_in[3], int32_t* j1, int32_t* j2,
                                       uint8_t* flags, double x_out[3]);
/* out = {pairs matched, kernel launches, buffer growths (device or pinned), host waits} */
int lslam_plicp_stats(const lslam_plicp* h, int64_t out[4]);

/* The node of O/ (ScanCallback :191-232, ScanMatchWithPLICP :327-436, NewKeyframeNeeded :498-517) for n_tracks independent
 * tracks (robots or logs): ONE launch per call, a workgroup per track walking its scans in order; the state stays on the
 * device, the keyframe scan in HBM; one host wait per call.  kf_dist_linear 0.1, kf_dist_angular 5 deg * pi / 180,
 * kf_scan_count 10 (O/:64-67); base_to_laser: the planar base <- laser transform (x, y, yaw), NULL = identity. */
typedef struct lslam_plicp_odom_record {
  double x[3];        /* sm_icp's result against the keyframe scan, as lslam_plicp_record */
  double error;
  int32_t valid;
  int32_t iterations; /* -1: an inactive scan (every other field zero) */
  int32_t nvalid;
  int32_t flags;      /* bit 0: the first scan of the track, no match made; bit 1: this scan became the keyframe */
  double base_in_odom[3];
  double reserved;
} lslam_plicp_odom_record; /* 80 bytes */
typedef struct lslam_plicp_odom_track {
  double base_in_odom[3];
  double keyframe[3];  /* base_in_odom_keyframe_ */
  double velocity[2];  /* latest_velocity_.linear.x, .angular.z */
  double last_icp_time;
  int32_t scan_count;
  int32_t initialized;
} lslam_plicp_odom_track; /* 80 bytes */
typedef struct lslam_plicp_odom lslam_plicp_odom;
int lslam_plicp_odom_create(lslam_context* ctx, const lslam_plicp_params* params, int n_tracks, double kf_dist_linear,
                            double kf_dist_angular, int kf_scan_count, const double base_to_laser[3], lslam_plicp_odom** out);
void lslam_plicp_odom_destroy(lslam_plicp_odom* h);
int lslam_plicp_odom_set_laser(lslam_plicp_odom* h, double angle_min, double angle_increment, double range_min, double range_max);
/* every track back to its state after create (asynchronous) */
int lslam_plicp_odom_reset(lslam_plicp_odom* h);
/* out: n_tracks states (one host wait) */
int lslam_plicp_odom_state(lslam_plicp_odom* h, lslam_plicp_odom_track* out);
/* n_steps scans per track; every per-scan array is indexed step * n_tracks + track: ranges rows (float32, ranges_stride
 * apart), stamps (seconds), active (NULL = all 1; an inactive scan changes nothing of its track), out.  Host pointers.  Every
 * call of one handle between resets takes the same n_readings. */
int lslam_plicp_odom_process_many(lslam_plicp_odom* h, int n_steps, int n_readings, const float* ranges, int ranges_stride,
                                  const double* stamps, const uint8_t* active, lslam_plicp_odom_record* out);
/* The node of O/ (plicp_odometry.cc) on CLOUDS under the rules of lslam_plicp_match_clouds (scan_match_plicp.cc:220-300 read on
 * points: valid byte and finite x, y; float32 x, y widened; z ignored; no range window; the reading index is i), with a take
 * gate, so that lslam_msync_scans_dev output (xyz, valid, records[].status) feeds R tracks with nothing but stamps and flags
 * crossing the bus.  No laser is needed.  Entry i = step * n_tracks + track.
 *   Host form: xyz[n_steps * R][n_points][3], valid[n_steps * R][n_points] or NULL, take[n_steps * R] bytes or NULL.
 *   _dev form: xyz_dev, valid_dev, take_dev are HOST arrays of R device pointers, one block per track: track m's cloud of step k
 *   is at xyz_dev[m] + k * n_points * 3, its flags at valid_dev[m] + k * n_points, its take word at take_dev[m] + k * take_stride;
 *   the entry is taken iff the word is > 0.  take_stride counts int32 words: 22 on &records[0].status of lslam_msync_record
 *   serves as it stands.  valid_dev, take_dev, or single entries of them may be NULL (every point / every step).
 * stamps, active and out are HOST arrays in both forms; one launch and one host wait per call; in the _dev form only the stamps,
 * the active bytes and the R-entry pointer table go up.
 * Entry i is TAKEN iff active[i] != 0 (NULL: all) and its take word says so.  An entry that is not taken changes nothing of its
 * track -- the state (initialized, scan_count, last_icp_time, velocity), the pose, the keyframe pose and the keyframe cloud stay
 * as they were; its stamp and its cloud are not read; its record is all zero with iterations = -1.  A track whose first callbacks
 * are refused is initialised by its first taken scan.  The keyframe is kept per track as a cloud (x, y float32 and the valid byte)
 * in a buffer of the handle's and outlives the call.  The node's arithmetic -- the prediction, corr_ch, NewKeyframeNeeded and
 * the three rules above -- is that of the ranges form, unchanged.
 * Between resets a handle runs EITHER range calls or cloud calls, with one n_points: the other kind, or another length, is
 * LSLAM_ERR_INVALID_ARGUMENT with nothing enqueued and nothing changed; lslam_plicp_odom_reset frees the choice.
 * LSLAM_ERR_UNSUPPORTED: n_points > LSLAM_PLICP_MAX_READINGS. */
int lslam_plicp_odom_process_many_clouds(lslam_plicp_odom* h, int n_steps, int n_points, const float* xyz, const uint8_t* valid,
                                         const uint8_t* take, const double* stamps, const uint8_t* active,
                                         lslam_plicp_odom_record* out);
int lslam_plicp_odom_process_many_clouds_dev(lslam_plicp_odom* h, int n_steps, int n_points, const float* const* xyz_dev,
                                             const uint8_t* const* valid_dev, const int32_t* const* take_dev, int take_stride,
                                             const double* stamps, const uint8_t* active, lslam_plicp_odom_record* out);
/* out = {scans processed, kernel launches, buffer growths, host waits} */
int lslam_plicp_odom_stats(const lslam_plicp_odom* h, int64_t out[4]);

/* ---------------------------------------------------------------------------------------- */
/* lesson2 point-to-point ICP pair matching (ScanMatchICP: lesson2/src/scan_match_icp.cc, and */
/* the cloud of lesson2/src/scan_to_pointclod2_converter.cc, "C/" below), many pairs per      */
/* launch.                                                                                    */
/* STANDING: PARITY WITH THE REFERENCE IS UNPINNED.  Its arithmetic lives in PCL              */
/* (IterativeClosestPoint, with FLANN and Eigen under it), which is neither vendored nor       */
/* pinned.  The results are DEFINED by this project's own fp64 restatement of PCL 1.8's        */
/* computeTransformation with DefaultConvergenceCriteria: `icp` in tools/icp_cpu.py.  All      */
/* device arithmetic is fp64 on the stored float32 x, y; z is ignored.                         */
/* Five deliberate rules:                                                                     */
/*  1. LOWEST INDEX: among equal distances the lowest target index wins (FLANN's order among   */
/*     equals is unspecified).                                                                */
/*  2. FP64 ON THE ORIGINAL POINTS: every iteration transforms the original source points by   */
/*     the accumulated transform, where PCL re-transforms a float cloud in place.              */
/*  3. 2-D CLOSED FORM: theta = atan2(Sxy - Syx, Sxx + Syy), t = qbar - R(theta) pbar from the  */
/*     means and then the centred sums of the accepted pairs, where PCL runs a 3-D SVD.        */
/*  4. LITERAL ORIGIN POINTS: an invalid reading stays in the cloud as the point (0, 0, 0), as */
/*     the node leaves it (scan_match_icp.cc:96-123), and is matched like any other point.     */
/*  5. skip_invalid = 1 is the opt-in that removes the invalid readings from both clouds.  A   */
/*     point whose x or y is not finite (C/'s NaN point) never takes part, in either mode.     */
/* And a fact about the definition: THE ORDER OF THE SUMS is part of it -- 256 partial sums     */
/* over the points l, l + 256, ... in ascending index, a binary tree per 64 partials, the four  */
/* groups in order (tools/icp_cpu.py block_sum).  With transformation_epsilon = 0 rule 2 below  */
/* fires only on an increment that is exactly the identity, which at a fixed point is decided  */
/* by the last bit of these sums.                                             */
/* ---------------------------------------------------------------------------------------- */
#define LSLAM_ICP_MAX_POINTS 2048
/* defaults = what lesson2 leaves in place, PCL's own */
typedef struct lslam_icp_params {
  double max_correspondence_distance; /* sqrt(DBL_MAX); a correspondence is accepted iff d2 <= its square */
  double transformation_epsilon;      /* 0 */
  double euclidean_fitness_epsilon;   /* -DBL_MAX */
  double absolute_mse;                /* 1e-12 */
  int32_t max_iterations;             /* 10; at least 1 */
  int32_t skip_invalid;               /* 0 */
  int32_t invalid_as_nan;             /* 0; 1: the conversion writes C/'s invalid_point_ (NaN, NaN, NaN) for an invalid reading */
  int32_t reserved;
} lslam_icp_params; /* 48 bytes */
void lslam_icp_params_defaults(lslam_icp_params* p);
/* state: the stop rule that fired -- 1 iterations >= max_iterations, 2 cos(theta) >= 1 - transformation_epsilon and |t|^2 <=
 * transformation_epsilon, 3 |mse - previous mse| < absolute_mse, 4 |mse - previous| / previous < euclidean_fitness_epsilon
 * (converged = 1 for all four), 5 fewer than 3 correspondences were accepted (converged = 0, x = the pose accumulated so far). */
typedef struct lslam_icp_record {
  double x[3];        /* (tx, ty, atan2(s, c)) of the final transformation: source (pair_source) into target (pair_target) */
  double fitness;     /* getFitnessScore(): mean over the source points of the squared distance from the finally transformed
                         point to its nearest target point; DBL_MAX where no source point has one */
  double mse;         /* mean accepted d2 of the last iteration's search, i.e. before its increment was applied */
  int32_t converged;
  int32_t iterations;
  int32_t ncorr;      /* correspondences accepted by the last search */
  int32_t state;
  double reserved;
} lslam_icp_record; /* 64 bytes */
typedef struct lslam_icp lslam_icp;
int lslam_icp_create(lslam_context* ctx, const lslam_icp_params* params, lslam_icp** out);
void lslam_icp_destroy(lslam_icp* h);
/* The LaserScan header fields, kept as float32 as the message keeps them: a reading is valid iff it is finite and
 * range_min < r < range_max compared in float32; angle_i = angle_min + i * angle_increment evaluated in float32. */
int lslam_icp_set_laser(lslam_icp* h, double angle_min, double angle_increment, double range_min, double range_max);
/* ConvertScan2PointCloud (scan_match_icp.cc:89-130) for n_scans scans in one launch.  ranges: n_scans rows of n_readings float32,
 * row k at ranges + k * ranges_stride.  out_xyz: n_scans x n_readings x 3 float32, x = (float)((double)r * cos((double)angle)),
 * y with sin, z = 0; an invalid reading gives (0, 0, 0), or (NaN, NaN, NaN) with invalid_as_nan.  out_valid: n_scans x n_readings
 * bytes, produced in both modes.  This is the layout lslam_deskew_batch writes and lslam_map_set_cloud reads.  The _dev form
 * takes all three in HBM and makes no host wait. */
int lslam_icp_convert_batch(lslam_icp* h, int n_scans, int n_readings, const float* ranges, int ranges_stride, float* out_xyz,
                            uint8_t* out_valid);
int lslam_icp_convert_batch_dev(lslam_icp* h, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride,
                                float* out_xyz_dev, uint8_t* out_valid_dev);
/* ScanMatchWithICP (scan_match_icp.cc:135-164) for n_pairs pairs: one conversion launch and ONE match launch (a workgroup per
 * pair, the iterations loop on the device).  Pair b aligns the cloud of scan pair_source[b] to the cloud of scan pair_target[b]
 * (the node: source = last, target = current).  first_guess: n_pairs x 3 doubles (x, y, yaw), NULL = zeros.  pair_source /
 * pair_target are HOST arrays in both forms.  The host form owns its buffers (a repeated shape allocates nothing) and waits
 * once, at its end.  The _dev form takes ranges, first_guess and out in HBM, is asynchronous on lslam_stream() and makes no host
 * wait, with the back-pressure of lslam_plicp_match_batch_dev: the pair indices go up through a ring of 4 pinned slots.
 * A pair's record is byte for byte the same alone and in any batch.  n_pairs == 0 is LSLAM_OK and launches nothing.
 * LSLAM_ERR_INVALID_ARGUMENT, outputs untouched: NULL pointers, a pair index outside [0, n_scans), no laser set.
 * LSLAM_ERR_UNSUPPORTED: more than LSLAM_ICP_MAX_POINTS readings. */
int lslam_icp_match_batch(lslam_icp* h, int n_scans, int n_readings, const float* ranges, int ranges_stride, int n_pairs,
                          const int32_t* pair_source, const int32_t* pair_target, const double* first_guess, lslam_icp_record* out);
int lslam_icp_match_batch_dev(lslam_icp* h, int n_scans, int n_readings, const float* ranges_dev, int ranges_stride, int n_pairs,
                              const int32_t* pair_source, const int32_t* pair_target, const double* first_guess_dev,
                              lslam_icp_record* out_dev);
/* The same on clouds: xyz = n_clouds x n_points x 3 float32, valid = n_clouds x n_points bytes or NULL (all valid; read only with
 * skip_invalid) -- a converter's or the de-skew's output.  ONE launch; needs no laser. */
int lslam_icp_match_clouds(lslam_icp* h, int n_clouds, int n_points, const float* xyz, const uint8_t* valid, int n_pairs,
                           const int32_t* pair_source, const int32_t* pair_target, const double* first_guess, lslam_icp_record* out);
int lslam_icp_match_clouds_dev(lslam_icp* h, int n_clouds, int n_points, const float* xyz_dev, const uint8_t* valid_dev, int n_pairs,
                               const int32_t* pair_source, const int32_t* pair_target, const double* first_guess_dev,
                               lslam_icp_record* out_dev);
/* ONE iteration from x_in = (x, y, yaw), by the same device code as the batch kernel (host pointers; one launch, one wait).
 * Per source point: corr = the target index, -1 where the correspondence was rejected or the point is masked; d2 = the best
 * squared distance (+inf where there is none).  inc = the solved increment (tx, ty, theta), NaN where fewer than 3 were accepted;
 * mse and ncorr of this search.  src_valid / tgt_valid may be NULL. */
int lslam_icp_debug_iteration(lslam_icp* h, const float* src_xyz, const float* tgt_xyz, const uint8_t* src_valid,
                              const uint8_t* tgt_valid, int n, const double x_in[3], int32_t* corr, double* d2, double inc[3],
                              double* mse, int32_t* ncorr);
/* out = {pairs matched, kernel launches, buffer growths (device or pinned), host waits} */
int lslam_icp_stats(const lslam_icp* h, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* LSLAM_GPU_H */
