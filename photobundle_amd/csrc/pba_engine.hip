// pba_engine.hip -- C-ABI (include/pba.h) of the MI355X photometric bundle-adjustment engine.
//
// Owns all device memory, one HIP stream per engine; every pass is stream-ordered and the host synchronises
// once per step attempt (pba_step) to read a 32-double scalar block.  There is no CPU fallback: pba_create
// fails with PBA_ERR_NO_DEVICE when no GPU is visible.
#include "../../include/pba.h"
#include "pba_comm.h"
#include "pba_handle.h"
#include "pba_internal.h"
#include "pba_mode_rules.h"
#include "pba_kernels.h"
#include "pba_frontend.h"
#include "pba_resident.h"
#include "pba_wide.h"
#include "pba_batch.h"
#include "pba_pose.h"
#include "pba_points.h"
#include "pba_cov.h"
#include "pba_prior.h"
#include "pba_cull.h"
#include "pba_admit.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace pba;

// Event times of the N kernels of one off-loop call (pba_covariance, pba_marginalize) under event profiling (pba_set_profiling(e, 1)):
// one begin / end pair of events per kernel, created on first use; ms[k] of the last call, -1: kernel k did not run or profiling was off
template <int N>
struct KernelTimes {
  hipEvent_t ev[2 * N] = {};
  double ms[N] = {};
  bool on = false, ran[N] = {};
  int start(pba::Handle* h, bool timed) {
    on = timed;
    for (bool& r : ran) r = false;
    if (timed && !ev[0])
      for (hipEvent_t& x : ev) { const int rc = handle_event(h, &x); if (rc) return rc; }
    return PBA_OK;
  }
  void begin(const pba::Handle* h, int k) { if (on) { (void)hipEventRecord(ev[2 * k], h->stream); ran[k] = true; } }
  void end(const pba::Handle* h, int k) { if (on) (void)hipEventRecord(ev[2 * k + 1], h->stream); }
  void collect() {
    for (int k = 0; k < N; ++k) {
      float t = 0.0f;
      ms[k] = (on && ran[k] && hipEventElapsedTime(&t, ev[2 * k], ev[2 * k + 1]) == hipSuccess) ? (double)t : -1.0;
    }
  }
  void copy_to(double* out) const { for (int k = 0; k < N; ++k) out[k] = ms[k]; }
};

struct pba_engine : pba::Handle {      // (device, stream, err, mem, events)
  pba_config cfg{};

  // frames
  uint32_t* d_frames = nullptr;     // [max_frames][rows*cols] packed texels
  float* d_frames_mc = nullptr;     // channels > 1: [max_frames][channels][rows*cols] channel VALUES (gradients are formed at use)
  int channels = 1;
  uint8_t* d_img_stage = nullptr;   // [rows*cols]
  bool img_stage_valid = false;     // d_img_stage holds the u8 image of the frame uploaded last (set by the u8 / descriptor / pyr_down
                                    // setters, cleared by the float setters): what the device front-end's ZNCC reads
  uint8_t* h_img_stage = nullptr;   // pinned host copy of the frame being uploaded
  double* h_state_stage = nullptr;  // pinned, host-mapped landing buffer of pba_get_state (grown on demand)
  double* h_state_dev = nullptr;    // its device address
  hipEvent_t ev_img_stage = nullptr;
  bool img_stage_busy = false;
  hipEvent_t ev_xdep = nullptr;     // orders another engine's stream against this one (pba_set_frame_pyr_down)
  uint8_t* d_u8_work[2] = {nullptr, nullptr};   // device-side descriptor producers: smoothed frame, census image (on first use)
  // device front-end (pba_frontend_*), everything on first use
  uint8_t* d_fe_mask = nullptr;     // [rows*cols] selection mask (1 = free)
  uint8_t* d_fe_flag = nullptr;     // [rows*cols] candidate flags
  float* d_fe_smap = nullptr;       // [rows*cols] saliency
  float* d_fe_depth = nullptr;      // [rows*cols]
  int32_t* d_fe_rows = nullptr;     // [2 rows + 1] per-row counts | offsets
  pba_candidate* d_fe_cand = nullptr;   // [rows*cols]
  char* d_fe_io = nullptr;          // grow-only device scratch of the visibility / descriptor calls
  char* h_fe_io = nullptr;          // pinned staging (grow-only)
  bool fe_mask_valid = false;       // pba_frontend_visibility ran for the current frame
  int fe_n_cand = 0;
  std::vector<uint8_t> frame_set;
  uint32_t slot_mask = 0;           // window slots referenced by the observation list

  // problem
  int n_points = 0, n_obs = 0, n_frames = 0, n_free = 0;
  uint32_t anchor_mask = 0;         // constant slots (pba_set_cameras_anchored; pba_slot_rule.h turns it into free indices)
  bool have_problem = false, have_cams = false, have_lin = false;
  bool lin_valid[2] = {false, false};   // rec[k] holds a Jacobian pass of point k
  bool speculate = true;            // candidate pass = Jacobian pass (skips the re-linearisation after an accept)
  int cur = 0;                      // ping-pong index of the current point
  double* d_xyz[2] = {nullptr, nullptr};
  double* d_cams[2] = {nullptr, nullptr};
  CamGeom* d_geom[2] = {nullptr, nullptr};
  float* d_desc = nullptr;
  double* d_w2 = nullptr;
  double* d_rays = nullptr;         // inverse-depth variant: [n_points][6] fixed world rays (null pointer passed otherwise)
  bool inverse_depth = false;
  std::vector<double> h_rays;       // host copy for pba_get_points_world
  int32_t* d_obs_point = nullptr;
  uint8_t* d_obs_slot = nullptr;
  int32_t* d_pt_begin = nullptr;
  int4* d_tile_info = nullptr;
  int2* d_lane_rec = nullptr;       // [n_tiles][kTile] per tile lane: point, slot | first lane << 8 | observations of the point << 16
  int n_tiles = 0;
  // linearisation + solve scratch
  int64_t rec_stride = 0;
  double* d_rec[2] = {nullptr, nullptr};   // [6][rec_stride] per point parity
  double* d_sp = nullptr;           // [n_points][3]
  double* d_ptrec = nullptr;        // [n_points][12]
  double* d_sc = nullptr;           // [2][6 * max(kMaxFrames, max_frames)]: Jacobi scales | live flags (the [1] part starts at 6 n_free)
  double* d_delta_c = nullptr;      // [max(kMaxFrames, max_frames)][6]
  double* d_partial = nullptr;      // [schur_grid][part_stride]
  double* d_red = nullptr;          // [kChunks][part_stride]
  double* d_packed = nullptr;       // [part_stride] (the tri layout of pba_solve.h needs packed_stride(n) < part_stride of them)
  uint32_t* d_solve_tab = nullptr;  // window-shape index tables of the reduced solve (solve_tables), rebuilt when n_free changes
  int solve_tab_nf = -1;
  double* d_S = nullptr;            // [n*n] debug copy
  double* d_rhs = nullptr;          // [n]
  double* d_block_cost[2] = {nullptr, nullptr};   // [sample_grid] block costs of the last pass at point parity k
  int32_t* d_block_fail[2] = {nullptr, nullptr};
  int cost_blocks[2] = {0, 0};      // valid entries in d_block_cost[k] (grid of the pass that wrote them)
  double* d_bs_out = nullptr;       // [backsub_grid][3]
  double* d_scal = nullptr;         // [kNumScal]
  double* d_xchg = nullptr;         // [kSumBCount + kMaxCount * world] multi-rank exchange buffer
  double* h_scal = nullptr;         // pinned + mapped: [kNumScal] doubles then one u64 sequence number
  double* h_scal_dev = nullptr;     // device view of h_scal
  unsigned long long seq = 0;
  int64_t jac_passes = 0, cost_passes = 0;
  int schur_grid = 0, sample_grid = 0, backsub_grid = 0, sample_waves = 4, fused_grid = 0;
  bool unit_weights = false;        // all patch weights are exactly 1 (MakePatchWeights without the Gaussian)
  bool fuse = true;                 // back-substitution + finalisation fused into the candidate pass (radius <= 3)
  unsigned int* d_ticket = nullptr;
  unsigned int* d_ticket_solve = nullptr;   // arrival counter of k_reduce_solve
  unsigned long long* d_stamp = nullptr;    // [kStampMaxIters + 1][kStampRecord] device time stamps of the pipelined iterations (pba_set_profiling(e, 2))
  bool stamps = false;
  int stamp_iter = 0;                       // record of the iteration being enqueued (0: the first linearisation)
  int solve_kind = 0;               // PBA_SOLVE: 0 blocked workgroup L D L^T (fused with the reduction at one rank), 1 k_solve_generic (diagnostics)
  // asynchronous driver (device-side trust-region decisions)
  LmState* d_lm = nullptr;          // device state
  LmState* h_lm = nullptr;          // host-mapped mirror, written at every publish
  LmState* h_lm_dev = nullptr;
  pba_iteration_summary* h_log = nullptr;      // host-mapped iteration log
  pba_iteration_summary* h_log_dev = nullptr;
  pba_iteration_summary* d_log = nullptr;      // device iteration log of the asynchronous driver (flushed at the end)
  static constexpr int kMaxLog = 1024;
  int async_cur = 0;                // parity assumed at enqueue time
  bool use_async = true;            // PBA_ASYNC=0 disables
  // resident solve (pba_resident.h): one cooperative launch per pba_solve when the window fits one resident round of workgroups
  bool use_resident = true;         // PBA_RESIDENT=0 disables
  unsigned* d_res_sync = nullptr;   // flag block (kResSyncBytes), zeroed once: epochs grow from launch to launch
  static constexpr unsigned kResEpochLimit = 0xF0000000u;      // the epochs restart (flag block zeroed) before a launch would count beyond this
  unsigned res_epoch = 1;           // first epoch of the next resident launch
  unsigned res_epoch_launch = 1;    // ... of the one in flight / last finished
  int res_groups_max[2][2] = {{-1, -1}, {-1, -1}};   // [radius - 1][unit weights]: co-resident workgroups of k_resident (-1: not asked yet, 0: none)
  int res_groups_n[2][2] = {{-1, -1}, {-1, -1}};     // ... the reduced-system size that answer was given for
  int n_cus = 0, coop_launch = 0;
  int lds_max = 0;                  // LDS bytes a workgroup may ask for (read once at pba_create; 0: unknown, nothing is refused on it)
  int64_t res_launches = 0;
  int last_driver = 0;              // 0 none, 1 resident, 2 pipelined, 3 host-stepped, 4 batched (pba_solve_driver)
  double wait_timeout_s = 120.0;    // PBA_WAIT_TIMEOUT_S: watchdog of the publication waits
  double tick_hz = 1e8;             // rate of s_memrealtime (hipDeviceAttributeWallClockRate; 100 MHz on gfx950): device-side time-outs
  bool poisoned = false;            // a publication wait timed out: the stream still holds the stalled work, every later
                                    // call fails fast and pba_destroy neither waits for the stream nor for the collective
  unsigned long long* d_dbg = nullptr;   // PBA_SCHUR_TIMING diagnostics, on first use
  static constexpr size_t kDbgWords = 8 * (1024 + 4096);
  int dbg_left = 0;
  int n_pairs = 0, part_stride = 0;
  static constexpr int kChunks = 32;
  // wide windows (more than kMaxFrames slots, or kWideMinFree..kMaxFramesWide free cameras; pba_wide.h): chosen by pba_set_cameras_anchored
  // from the window shape
  bool wide = false;
  bool wide_ready = false;          // the co-observation lists below match the current problem and camera set
  std::vector<int32_t> h_pt_begin;  // host copies of the observation structure
  std::vector<uint8_t> h_obs_slot;
  double* d_wfac = nullptr;         // [n_obs][kWideFac] observation factors
  double* d_wpt_part = nullptr;     // [point blocks][3]
  int2* d_went = nullptr;           // co-observations, pair-major
  int4* d_wchunk = nullptr;         // [wide_chunks] {first entry, end, diagonal, pair}
  int32_t* d_wpair_chunk = nullptr; // [n_pairs + 1]
  double* d_wsums = nullptr;        // [wide_chunks][kWideVals]
  int wide_chunks = 0, wide_pt_blocks = 0;

  // pose-only solves (pba_set_points_constant, pba_pose.h): everything on first use
  bool points_const = false;
  bool pose_xyz_synced = false;     // both point parities hold the same (constant) points
  int pose_sums_cur = -1;           // parity whose linearisation d_pose_sums was reduced from, -1 none
  int pose_grid = 0;                // workgroups of the last k_pose_system launch (rows of d_pose_partial)
  double* d_pose_partial = nullptr; // [kPoseMaxGrid][n_frames * kPoseVals]
  double* d_pose_sums = nullptr;    // [n_frames * kPoseVals + 2]

  // structure-only solves (pba_set_cameras_constant, pba_points.h): everything on first use
  bool cams_const = false;
  bool pts_cams_synced = false;     // both camera parities hold the same (constant) cameras and geometry
  int pts_sys_cur = -1;             // parity whose linearisation d_pts_sys was built from, -1 none
  bool pts_dbg_valid = false;       // d_pts_V / d_pts_rhs hold the blocks of a step in the mode
  double* d_pts_sys = nullptr;      // [kPointsSys][n_points]
  double* d_pts_part = nullptr;     // [waves of k_points_solve][kPointsRow]
  double* d_pts_V = nullptr;        // [n_points][9] test hook (pba_config.flags bit 0)
  double* d_pts_rhs = nullptr;      // [n_points][3]

  // the point elimination of pba_covariance and pba_marginalize (pba_elim.h): everything on first use, nothing shared with the LM; a
  // call writes every buffer it reads, so the two calls use one set
  double* d_elim_X = nullptr;       // [n_points][6] triangular factor of V^-1 (marginalisation: zero outside the marginalised points)
  double* d_elim_part = nullptr;    // [point blocks][kCovPart or kMargPart]
  double* d_elim_S = nullptr;       // [n][n] undamped, unscaled reduced camera matrix (marginalisation: of the marginalised points)
  double* d_elim_info = nullptr;    // [3] (k_cov_invert: 2, k_marg_eliminate: 3)
  // covariance output (pba_covariance, pba_cov.h)
  double* d_cov_P = nullptr;        // [n_points][6] V^-1
  double* d_cov_C = nullptr;        // [n][n] the inverse of S
  double* d_cov_pp = nullptr;       // [n_points][9]
  KernelTimes<4> cov_times;         // k_cov_point, k_elim_pair, k_cov_invert, k_cov_points

  // camera prior (pba_set_camera_prior, pba_prior.h): one extra residual block on the camera blocks prior_slots, in information form
  bool prior_on = false;
  int prior_k = 0;
  double prior_c = 0.0;
  int32_t prior_slots[kMaxFrames] = {};
  double* d_prior = nullptr;        // x0 [6 k] | eta [6 k] | Lambda [6 k][6 k]
  double* d_prior_out = nullptr;    // [6 k + 1] gradient | E of the last evaluation that asked for them
  // point prior (pba_set_point_prior, pba_point_prior.h): one extra residual block on every point, in information form
  bool pp_on = false;
  double* d_pp_x0 = nullptr;        // [n_points][3]
  double* d_pp_L6 = nullptr;        // [n_points][6] upper triangle of Lambda_i row by row
  double* d_pp_part = nullptr;      // [kPointPriorMaxGrid] workgroup partials of k_point_prior_cost
  double* d_pp_E = nullptr;         // [1] E_pts of the last evaluation that asked for it (pba_linearize's cost)
  unsigned int* d_pp_ticket = nullptr;   // zero between launches
  double* d_cull_pp_x0 = nullptr;   // the fresh buffers an applied cull gathers the surviving rows into (exchanged with the two above)
  double* d_cull_pp_L6 = nullptr;
  // marginalisation (pba_marginalize): everything on first use, nothing shared with the LM
  double* d_marg_z = nullptr;       // [n_points][3]
  double* d_marg_r = nullptr;       // [n] gradient of the reduced system d_elim_S
  double* d_marg_L = nullptr;       // [nk][nk] the output
  double* d_marg_eta = nullptr;     // [nk]
  KernelTimes<5> marg_times;        // k_marg_point, k_elim_pair, k_marg_grad, k_prior, k_marg_eliminate

  // outlier culling (pba_cull, pba_cull.h): everything on first use, nothing shared with the LM
  uint32_t* d_cull_hist = nullptr;  // [kCullPasses][kCullBins] radix-select tables
  uint64_t* d_cull_sel = nullptr;   // [kCullSelWords] (k_cull_finish)
  int32_t* d_cull_pt_cnt = nullptr; // [n_points] surviving blocks per point
  int4* d_cull_part = nullptr;      // [point blocks] workgroup sums
  int2* d_cull_off = nullptr;       // [point blocks] their exclusive scan
  int32_t* d_cull_tot = nullptr;    // [kCullTotals]
  int32_t* d_cull_map = nullptr;    // [n_points] new index or -1
  int32_t* d_cull_dst = nullptr;    // [n_obs] new index or -1
  uint8_t* d_cull_keep = nullptr;   // [n_obs]
  double* d_cull_xyz = nullptr;     // the fresh buffers the survivors are gathered into; an applied cull exchanges them with
  float* d_cull_desc = nullptr;     // d_xyz[cur], d_desc, d_rays, d_obs_point, d_obs_slot
  double* d_cull_rays = nullptr;
  int32_t* d_cull_obs_point = nullptr;
  uint8_t* d_cull_obs_slot = nullptr;

  // re-observation (pba_admit, pba_admit.h): everything on first use, nothing shared with the LM or with pba_cull
  uint32_t* d_admit_hist = nullptr;       // [kCullPasses][kCullBins] radix-select tables
  uint64_t* d_admit_sel = nullptr;        // [kCullSelWords]
  uint32_t* d_admit_cand_mask = nullptr;  // [n_points] candidate slots
  uint32_t* d_admit_take_mask = nullptr;  // [n_points] taken slots
  int32_t* d_admit_cand_begin = nullptr;  // [n_points]
  uint2* d_admit_part = nullptr;          // [point blocks] workgroup sums
  uint2* d_admit_off = nullptr;           // [point blocks] their exclusive scan
  int32_t* d_admit_tot = nullptr;         // [kAdmitTotals]
  int32_t* d_admit_cand_point = nullptr;  // [n_cand] the candidate list: an observation list of its own
  uint8_t* d_admit_cand_slot = nullptr;
  uint8_t* d_admit_cand_take = nullptr;
  double* d_admit_rec = nullptr;          // [6][stride] the candidates' records (row 5: their costs)
  double* d_admit_block_cost = nullptr;   // [workgroups of the candidates' pass]
  int32_t* d_admit_block_fail = nullptr;
  int32_t* d_admit_obs_point = nullptr;   // the fresh buffers the merged lists are written into; an applied admission exchanges them with
  uint8_t* d_admit_obs_slot = nullptr;    // d_obs_point, d_obs_slot
  int32_t* d_admit_pt_begin = nullptr;    // [n_points + 1] of the merged list

  // batched solves (pba_solve_batch, pba_batch.h): the window table lives with the batch's FIRST engine (grow-only), whose stream
  // carries the batch; while a batch runs every engine's `stream` names that stream and `stream_own` keeps its own
  BatchWindow* d_batch = nullptr;
  BatchWindow* h_batch = nullptr;   // pinned staging of the table
  hipStream_t stream_own = nullptr;
  int batch_init2 = 0;              // init_scale of this window's final pass (max_num_iterations <= 0)

  Comm comm;
  unsigned int* h_comm_err = nullptr;      // host-mapped: a peer-exchange wait timed out (k_peer_allreduce)
  unsigned int* h_comm_err_dev = nullptr;

  // counters
  bool profile = false;
  static constexpr int kEvPairs = 7;     // Jacobian pass, cost pass, Schur, reduction, solve, exchange A, exchange B
  hipEvent_t ev[2 * kEvPairs] = {};
  bool ev_used[kEvPairs] = {};
  pba_counters ctr{};
};

namespace {

double wall_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#define HIP_TRY(e, call) PBA_HIP_TRY(e, call)

// A timed-out publication wait leaves the stream stalled: every later call returns at once instead of hanging on it.
#define PBA_NOT_POISONED(e) \
  do { if ((e)->poisoned) return fail((e), PBA_ERR_STATE, "the engine is unusable after a timed-out step (stalled stream / collective); destroy it"); } while (0)
// ... and every call that touches the device selects the engine's first
#define PBA_ENTER(e) \
  do { PBA_NOT_POISONED(e); HIP_TRY(e, hipSetDevice((e)->cfg.device)); } while (0)

// A peer-exchange wait that timed out on the device (k_peer_allreduce / the solve's prologue) reports through a host-mapped
// word.  The report is STICKY: the sums of that step were poisoned (NaN) on the device, the exchange sequence numbers may no
// longer match the peers', so the engine is unusable from then on -- every later call fails with PBA_ERR_COMM / PBA_ERR_STATE.
int comm_failed(pba_engine* e) {
  if (!e->h_comm_err) return PBA_OK;
  const unsigned int w = *reinterpret_cast<volatile unsigned int*>(e->h_comm_err);
  if (!w) return PBA_OK;
  e->poisoned = true;
  return fail(e, PBA_ERR_COMM, "peer exchange timed out after %.0f s waiting for rank %u", 0.5 * e->wait_timeout_s, w - 1);
}

// Grow-only buffers (Allocations::reserve): a sliding-window caller re-submits a problem of similar size for every frame, and a free +
// allocate pair per buffer per frame is pure overhead.  Contents are undefined after the call (every user overwrites or uploads the
// whole buffer).  The call is all a buffer needs besides its field: pba_destroy releases whatever the registry holds.
template <class T>
int dev_alloc(pba_engine* e, T** p, size_t n) {
  HIP_TRY(e, (hipError_t)e->mem.reserve(p, MemKind::device, n));
  return PBA_OK;
}
// ... of pinned host memory; dev_view: host-mapped, *dev_view its device address
template <class T>
int host_alloc(pba_engine* e, T** p, size_t n, T** dev_view = nullptr) {
  HIP_TRY(e, (hipError_t)e->mem.reserve(p, dev_view ? MemKind::mapped : MemKind::pinned, n, dev_view));
  return PBA_OK;
}

// the engine is in the full mode (cameras and points free) with every slot anchored: no camera column is left
bool full_mode_all_anchored(const pba_engine* e) { return e->have_cams && e->n_free == 0 && !e->points_const && !e->cams_const; }

// pba_config.flags: bit 0 keeps the reduced system for the test hooks, bits 1-2 pick a precision-sweep sampler mode (0: exact); the
// fixed world rays of the inverse-depth variant as the kernels take them (null outside it)
bool keep_system(const pba_engine* e) { return (e->cfg.flags & 1) != 0; }
int sweep_mode(const pba_engine* e) { return (e->cfg.flags >> 1) & 3; }
const double* rays_or_null(const pba_engine* e) { return e->inverse_depth ? e->d_rays : nullptr; }
// `need` bytes of LDS against what a workgroup of this device may ask for: "[prefix]<count> <what> need ... of LDS for <use>, ..."
int check_lds(pba_engine* e, size_t need, const char* prefix, int count, const char* what, const char* use) {
  if (e->lds_max <= 0 || need <= (size_t)e->lds_max) return PBA_OK;
  return fail(e, PBA_ERR_INVALID, "%s%d %s need %zu bytes of LDS for %s, the device offers %d per workgroup", prefix, count, what, need, use, e->lds_max);
}

// ---- shared by the two off-loop calls that eliminate the points (pba_covariance, pba_marginalize) ---------------------------------------
// The workgroup rows of a point kernel (pba_elim.h: smallest pivot | first failing point | n_sums sums, the cost first), read back
// behind whatever the caller queued, the stream drained, and reduced in block order.
struct PointPartials { double min_pivot = 1.0, sums[2] = {0.0, 0.0}; int32_t failed = -1; };
int read_point_partials(pba_engine* e, int pt_blocks, int n_sums, PointPartials* out) {
  const int width = elim_part_width(n_sums);
  std::vector<double> part((size_t)width * pt_blocks);
  HIP_TRY(e, hipMemcpyAsync(part.data(), e->d_elim_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  double bad = kElimNone;
  for (int k = 0; k < pt_blocks; ++k) {      // block order
    const double* row = part.data() + (size_t)width * k;
    out->min_pivot = std::min(out->min_pivot, row[0]);
    bad = std::min(bad, row[1]);
    for (int i = 0; i < n_sums; ++i) out->sums[i] += row[2 + i];
  }
  if (bad < kElimNone) out->failed = (int32_t)bad;
  return PBA_OK;
}
// a failing point block: the info fields and the PBA_ERR_NUMERIC report of `call`
template <class Info>
int point_block_failed(pba_engine* e, const char* call, const char* tail, int32_t point, Info& inf, Info* info) {
  inf.failed_is_point = 1; inf.failed_index = point; inf.min_point_pivot = 0.0;
  if (info) *info = inf;
  return fail(e, PBA_ERR_NUMERIC, "%s: the block of point %d is not positive definite (non-positive or non-finite pivot)%s", call, point, tail);
}
// what the kernels of both calls read of the engine's current point
template <class Params>
void elim_inputs(const pba_engine* e, Params& p) {
  const int cur = e->cur;
  p.xyz = e->d_xyz[cur]; p.geom = e->d_geom[cur]; p.rec = e->d_rec[cur]; p.pt_begin = e->d_pt_begin; p.obs_slot = e->d_obs_slot;
  p.rec_stride = e->rec_stride; p.n_points = e->n_points; p.fx = e->cfg.fx; p.fy = e->cfg.fy;
}

// ---- what is derived from what: a setter names the inputs it changed, invalidate() drops the caches derived from them; no setter
// assigns a validity flag itself ------------------------------------------------------------------------------------------------------
enum Input : unsigned { kInProblem = 1, kInCameras = 2, kInPointParams = 4, kInPointsConst = 8, kInCamsConst = 16, kInFrame = 32, kInPrior = 64, kInPointPrior = 128 };
// rec[k] no longer holds a Jacobian pass of point k (an input changed, or it is being overwritten): the sums reduced from it go too
void drop_lin(pba_engine* e, int k) {
  e->lin_valid[k] = false;
  if (e->pose_sums_cur == k) e->pose_sums_cur = -1;
  if (e->pts_sys_cur == k) e->pts_sys_cur = -1;
}
void invalidate(pba_engine* e, unsigned changed) {
  if (changed) { drop_lin(e, 0); drop_lin(e, 1); e->have_lin = false; }      // the linearisation: every input (the sampler reads the frames)
  if (changed & (kInProblem | kInCameras)) e->wide_ready = false;                                       // co-observation lists (wide_prepare)
  if (changed & (kInProblem | kInPointParams | kInPointsConst)) e->pose_xyz_synced = false;             // constant points in both parities
  if (changed & (kInProblem | kInCameras | kInCamsConst)) e->pts_cams_synced = false;                   // constant cameras in both parities
  if (changed & (kInProblem | kInCameras | kInPointParams | kInCamsConst)) e->pts_dbg_valid = false;    // d_pts_V / d_pts_rhs
}

// The end of every pba_set_frame_*: the slot holds a frame, the sampler has a new input.  u8: d_img_stage holds the frame's u8 image (what
// the device front-end's ZNCC reads); else there is none behind this frame
int frame_uploaded(pba_engine* e, int slot, bool u8) {
  e->img_stage_valid = u8;
  e->frame_set[slot] = 1;
  invalidate(e, kInFrame);
  return PBA_OK;
}

// The features the engine has switched on, for mode_conflict (pba_mode_rules.h); `multi`: the caller's reading of multi-rank
unsigned modes_present(const pba_engine* e, bool multi) {
  return (multi ? kModeMulti : 0u) | (e->inverse_depth ? kModeInverseDepth : 0u) | (sweep_mode(e) ? kModeSweep : 0u) |
         (e->have_cams && e->wide ? kModeWide : 0u) | (e->points_const ? kModePointsConst : 0u) | (e->cams_const ? kModeCamsConst : 0u) |
         (e->have_cams && e->n_frames - e->n_free >= 2 ? kModeAnchors : 0u) | (e->prior_on ? kModePrior : 0u) | (e->pp_on ? kModePointPrior : 0u);
}

// Call-order / consistency check before any pass touches the device (include/pba.h: PBA_ERR_STATE).
int check_ready(pba_engine* e, const char* who) {
  if (e->poisoned) return fail(e, PBA_ERR_STATE, "%s: the engine is unusable after a timed-out step (stalled stream / collective); destroy it", who);
  if (!e->have_problem || !e->have_cams)
    return fail(e, PBA_ERR_STATE, "call order violated: %s before set_problem/set_cameras", who);
  if (full_mode_all_anchored(e))      // (pba_set_problem switched a constant mode off under a mask that was legal in it)
    return fail(e, PBA_ERR_STATE, "%s: the anchor mask covers all %d slots and no constant mode is on; set the cameras again", who, e->n_frames);
  for (int s = 0; s < kMaxFramesWide; ++s) {
    if (!((e->slot_mask >> s) & 1u)) continue;
    if (s >= e->n_frames) return fail(e, PBA_ERR_STATE, "call order violated: an observation uses slot %d but only %d cameras are set", s, e->n_frames);
    if (!e->frame_set[s]) return fail(e, PBA_ERR_STATE, "call order violated: an observation uses slot %d but no frame was uploaded to it", s);
  }
  return PBA_OK;
}

constexpr int kSampleWaves = 4;    // 256-thread workgroups at every patch radius (two 128-observation tiles when fused)
static_assert(kBatchSampleWaves == kSampleWaves && kMaxBatch == PBA_MAX_BATCH, "the batched launches run the solo workgroups");

// MF: camera-table length of the sampling kernels -- kMaxFrames, or kMaxFramesWide on wide windows (unfused, exact precision only:
// pba_set_cameras refuses the sweep modes there)
template <int R, bool JAC, bool FUSED, int MF>
void launch_sample_r(pba_engine* e, const SampleParams& sp) {
  const int grid = FUSED ? e->fused_grid : e->sample_grid;
  const dim3 block(kSampleWaves * 64);
  if constexpr (FUSED) {
    // the reduced-precision sweep modes never take the fused path (fused_capable)
    if (e->unit_weights) hipLaunchKernelGGL((k_sample<R, JAC, kSampleWaves, true, true, false>), dim3(grid), block, 0, e->stream, sp);
    else hipLaunchKernelGGL((k_sample<R, JAC, kSampleWaves, true, false, false>), dim3(grid), block, 0, e->stream, sp);
  } else if constexpr (MF != kMaxFrames) {
    if (e->unit_weights) hipLaunchKernelGGL((k_sample<R, JAC, kSampleWaves, false, true, false, MF>), dim3(grid), block, 0, e->stream, sp);
    else hipLaunchKernelGGL((k_sample<R, JAC, kSampleWaves, false, false, false, MF>), dim3(grid), block, 0, e->stream, sp);
  } else {
    if (e->unit_weights && sp.prec != 0) hipLaunchKernelGGL((k_sample<R, JAC, kSampleWaves, false, true, true>), dim3(grid), block, 0, e->stream, sp);
    else if (e->unit_weights) hipLaunchKernelGGL((k_sample<R, JAC, kSampleWaves, false, true, false>), dim3(grid), block, 0, e->stream, sp);
    else hipLaunchKernelGGL((k_sample<R, JAC, kSampleWaves, false, false, false>), dim3(grid), block, 0, e->stream, sp);
  }
}
template <int R, bool JAC, bool FUSED, int MF>
void launch_sample_mc_r(pba_engine* e, const SampleParams& sp) {
  const dim3 grid(FUSED ? e->fused_grid : e->sample_grid), block(kSampleWaves * 64);
  if (e->unit_weights) hipLaunchKernelGGL((k_sample_mc<R, JAC, kSampleWaves, FUSED, true, MF>), grid, block, 0, e->stream, sp, (const float*)e->d_frames_mc, e->channels);
  else hipLaunchKernelGGL((k_sample_mc<R, JAC, kSampleWaves, FUSED, false, MF>), grid, block, 0, e->stream, sp, (const float*)e->d_frames_mc, e->channels);
}
template <bool JAC, bool FUSED, int MF>
void launch_sample_mf(pba_engine* e, const SampleParams& sp) {
  if (e->channels > 1) {
    switch (e->cfg.radius) {
      case 1: launch_sample_mc_r<1, JAC, FUSED, MF>(e, sp); break;
      case 2: launch_sample_mc_r<2, JAC, FUSED, MF>(e, sp); break;
      case 3: launch_sample_mc_r<3, JAC, FUSED, MF>(e, sp); break;
      case 4: launch_sample_mc_r<4, JAC, FUSED, MF>(e, sp); break;
      default: launch_sample_mc_r<5, JAC, FUSED, MF>(e, sp); break;
    }
    return;
  }
  switch (e->cfg.radius) {
    case 1: launch_sample_r<1, JAC, FUSED, MF>(e, sp); break;
    case 2: launch_sample_r<2, JAC, FUSED, MF>(e, sp); break;
    case 3: launch_sample_r<3, JAC, FUSED, MF>(e, sp); break;
    case 4: launch_sample_r<4, JAC, FUSED, MF>(e, sp); break;
    default: launch_sample_r<5, JAC, FUSED, MF>(e, sp); break;
  }
}
template <bool JAC, bool FUSED = false>
void launch_sample(pba_engine* e, const SampleParams& sp) {
  if constexpr (!FUSED) {
    if (e->wide) { launch_sample_mf<JAC, false, kMaxFramesWide>(e, sp); return; }
  }
  launch_sample_mf<JAC, FUSED, kMaxFrames>(e, sp);
}
// one kernel for back-substitution + candidate pass + step finalisation, at every patch radius; the opt-in
// reduced-precision sampler modes (pba_config.flags bits 1-2) keep the unfused kernels
// (wide windows run the unfused chain: the fused kernels stage kMaxFrames-entry tables)
// The Schur elimination runs the wide chain (pba_wide.h): on a wide window, and at every window shape while a point prior is set (its
// addend to V_i and g_i lives in k_wide_point<true>; k_schur is not touched).  `wide` alone keeps meaning the window's shape.
bool eliminates_wide(const pba_engine* e) { return e->wide || e->pp_on; }
bool fused_capable(const pba_engine* e) { return e->fuse && sweep_mode(e) == 0 && !eliminates_wide(e); }
int sample_waves_for_radius(int) { return kSampleWaves; }

__global__ void k_noop() {}
// initial trust-region state of a solve, passed by value (a device-to-device hipMemcpyAsync of the host-mapped mirror goes through
// the copy engine: its hand-over sat in front of the first kernel of every solve)
#ifndef PBA_LM_INIT_KERNEL
#define PBA_LM_INIT_KERNEL 0
#endif
__global__ void k_lm_init(LmState* dst, LmState st) { if (threadIdx.x == 0) *dst = st; }
// device -> host-mapped pinned memory (8-byte words, grid-stride); visible to the host once the stream has drained
__global__ void k_to_host(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
// A timing bracket that starts on an idle stream would charge the kernel with the host's launch latency (the begin
// event is stamped at once, the kernel arrives microseconds later): a no-op kernel in front absorbs it.
void ev_begin(pba_engine* e, int k) {
  if (e->profile) {
    hipLaunchKernelGGL(k_noop, dim3(1), dim3(1), 0, e->stream);
    (void)hipEventRecord(e->ev[2 * k], e->stream);
  }
}
void ev_end(pba_engine* e, int k) { if (e->profile) { (void)hipEventRecord(e->ev[2 * k + 1], e->stream); e->ev_used[k] = true; } }
void ev_collect(pba_engine* e) {
  if (!e->profile) return;
  double* acc[pba_engine::kEvPairs] = {&e->ctr.linearize_ms, &e->ctr.cost_ms, &e->ctr.schur_ms, &e->ctr.solve_ms, &e->ctr.solve_ms,
                                       &e->ctr.exchange_ms, &e->ctr.exchange_ms};
  int64_t* cnt[pba_engine::kEvPairs] = {&e->ctr.linearize_launches, &e->ctr.cost_launches, &e->ctr.schur_launches, &e->ctr.solve_launches,
                                        nullptr, &e->ctr.exchange_launches, nullptr};
  for (int k = 0; k < pba_engine::kEvPairs; ++k) {
    if (!e->ev_used[k]) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->ev[2 * k], e->ev[2 * k + 1]) == hipSuccess) { *acc[k] += ms; if (cnt[k]) *cnt[k] += 1; }
    e->ev_used[k] = false;
  }
}

void launch_solve(pba_engine* e, const SolveParams& so, int n) {
  if (e->solve_kind == 0) {
    if (e->n_free > kSolveNarrowFree) hipLaunchKernelGGL((k_solve_blocked<kSolveWideThreads>), dim3(1), dim3(kSolveWideThreads), solve_blocked_smem_bytes(n), e->stream, so);
    else hipLaunchKernelGGL((k_solve_blocked<kSolveBlockedThreads>), dim3(1), dim3(kSolveBlockedThreads), solve_blocked_smem_bytes(n), e->stream, so);
    return;
  }
  const size_t solve_smem = sizeof(double) * ((size_t)n * (n + 1) + 5 * n);
  hipLaunchKernelGGL(k_solve_generic, dim3(1), dim3(kSolveThreads), solve_smem, e->stream, so);
}

// record of the iteration being enqueued in the device time-stamp log (null: stamps off / beyond the log)
unsigned long long* stamp_record(pba_engine* e) {
  if (!e->stamps || !e->d_stamp || e->stamp_iter > kStampMaxIters) return nullptr;
  return e->d_stamp + (size_t)e->stamp_iter * kStampRecord;
}

// ---- peer exchange (pba_comm.h): kind 0 = packed reduced system, 1 = step scalars -------------------------------------
PeerParams peer_params(const pba_engine* e) {
  PeerParams pp{};
  for (int q = 0; q < Comm::kMaxPeers; ++q) pp.mb[q] = e->comm.mb_peer[q];
  pp.own = e->comm.mb_own; pp.world = e->comm.world; pp.rank = e->comm.rank;
  return pp;
}
// where the producer of the NEXT exchange of `kind` writes this rank's contribution
double* peer_slot(pba_engine* e, int kind) {
  const unsigned long long x = (kind == 0 ? e->comm.seq_a : e->comm.seq_b) + 1;
  return e->comm.mb_own + Comm::data_offset(kind, x);
}
// the exchange itself: flags + rank-ordered sum of n doubles into `out` (device memory of this rank)
int peer_allreduce(pba_engine* e, int kind, int n, double* out) {
  const unsigned long long x = ++(kind == 0 ? e->comm.seq_a : e->comm.seq_b);
  // device-side wait: half the host watchdog (100 MHz s_memrealtime), so that the recoverable PBA_ERR_COMM wins the race
  const unsigned long long ticks = (unsigned long long)(0.5 * e->wait_timeout_s * e->tick_hz);
  const int grid = std::max(1, std::min(32, (n + 255) / 256));
  hipLaunchKernelGGL(k_peer_allreduce, dim3(grid), dim3(256), 0, e->stream, peer_params(e), (int)Comm::flag_index(kind, x),
                     (unsigned long long)Comm::data_offset(kind, x), n, x, out, ticks, e->h_comm_err_dev);
  HIP_TRY(e, hipGetLastError());
  return PBA_OK;
}

// Reduction of the Schur partials + reduced solve.  One launch (k_reduce_solve) at a single rank; with more ranks the
// exchange of the packed sums sits between the two, so they stay separate kernels.  With the peer exchange there is no
// exchange kernel: the reduction's last workgroup raises this rank's mailbox flag, the solve's prologue waits for every
// rank's flag and sums the mailbox slots in rank order (pba_solve.h).
int reduce_grid(const pba_engine* e) { return (e->part_stride + kReduceEntries - 1) / kReduceEntries + 1; }
ReduceParams reduce_params(pba_engine* e, int cur, int n_cost_blocks) {
  ReduceParams rp{};
  rp.partial = e->d_partial; rp.n_blocks = e->schur_grid; rp.stride = e->part_stride; rp.n_free = e->n_free; rp.n_pairs = e->n_pairs;
  rp.block_cost = e->d_block_cost[cur]; rp.block_fail = e->d_block_fail[cur]; rp.n_cost_blocks = n_cost_blocks;
  rp.packed = e->d_packed; rp.scal = e->d_scal;
  return rp;
}
// parameters of the single-rank k_reduce_solve (the solo launch below and the batched one, pba_batch.h)
ReduceSolveParams reduce_solve_params(pba_engine* e, SolveParams so, int n, int cur, int cand, const LmState* lm, int final_pass, int n_cost_blocks,
                                      const ReduceSolveParams::Fin* fin) {
  // The gradient-only pass neither forms nor reduces the pair blocks and the right-hand side: the reduced-system test hook
  // (pba_get_reduced_system) keeps the system of the last FULL step instead of being overwritten with entries nobody computed
  if (final_pass && !so.init_scale) { so.S_dbg = nullptr; so.rhs_dbg = nullptr; }
  ReduceSolveParams rsp{};
  rsp.rp = reduce_params(e, cur, n_cost_blocks);
  rsp.block_cost_alt = e->d_block_cost[cand]; rsp.block_fail_alt = e->d_block_fail[cand];
  rsp.ticket = e->d_ticket_solve; rsp.so = so;
  if (fin) {
    rsp.fin = *fin;
    // gradient-only: the pair blocks and the right-hand side of the partials are not consumed
    if (final_pass && !so.init_scale) rsp.rp.first_entry = 36 * e->n_pairs + n;
  }
  rsp.stamp = (lm && !final_pass) ? stamp_record(e) : nullptr;
  return rsp;
}

// The camera prior evaluated at `cams` (pba_prior.h): the caller names the destinations.  col: the reduced program's camera column of
// every prior slot (its free index, -1 for an anchored slot, which takes part in d but has no column)
PriorParams prior_params(const pba_engine* e, const double* cams) {
  PriorParams pp{};
  const int m = 6 * e->prior_k;
  pp.x0 = e->d_prior; pp.eta = e->d_prior + m; pp.Lambda = e->d_prior + 2 * m; pp.cams = cams;
  pp.c = e->prior_c; pp.k = e->prior_k; pp.n_free = e->n_free;
  for (int i = 0; i < e->prior_k; ++i) {
    pp.slot[i] = (uint8_t)e->prior_slots[i];
    pp.col[i] = (int8_t)slot_free_index(e->anchor_mask, e->prior_slots[i]);
  }
  return pp;
}
void launch_prior(pba_engine* e, const PriorParams& pp) { hipLaunchKernelGGL(k_prior, dim3(1), dim3(kPriorThreads), 0, e->stream, pp); }

int launch_reduce_and_solve(pba_engine* e, SolveParams so, int n, int cur, int cand, const LmState* lm, int final_pass, int n_cost_blocks,
                            const ReduceSolveParams::Fin* fin = nullptr) {
  const bool multi = e->comm.multi();
  const int grid = reduce_grid(e);
  const int pstride = packed_stride(n);
  const ReduceParams rp = reduce_params(e, cur, n_cost_blocks);
  // with a camera prior the reduction and the solve stay separate launches: the prior's addend goes in between
  if (!multi && e->solve_kind == 0 && !e->prior_on && !(PBA_PHASE_TIMING && getenv("PBA_SPLIT_SOLVE"))) {
    const ReduceSolveParams rsp = reduce_solve_params(e, so, n, cur, cand, lm, final_pass, n_cost_blocks, fin);
    ev_begin(e, 3);
    hipLaunchKernelGGL(k_reduce_solve, dim3(grid), dim3(kReduceThreads), solve_blocked_smem_bytes(n), e->stream, rsp);
    ev_end(e, 3);
    HIP_TRY(e, hipGetLastError());
    return PBA_OK;
  }
  if (final_pass && !so.init_scale) { so.S_dbg = nullptr; so.rhs_dbg = nullptr; }      // (as reduce_solve_params does)
  const bool peer = multi && e->comm.peer;
  if (peer && (size_t)pstride > Comm::kCapA) return fail(e, PBA_ERR_COMM, "reduced system of %d doubles exceeds the peer mailbox", pstride);
  ReduceFinalParams fp{};
  fp.rp = rp; fp.lm = lm; fp.enq_cur = cur; fp.final_pass = final_pass;
  fp.block_cost_alt = e->d_block_cost[cand]; fp.block_fail_alt = e->d_block_fail[cand];
  fp.sys_stores = peer ? 1 : 0; fp.ticket = e->d_ticket_solve; fp.peer_flag = -1;
  if (peer) {
    const unsigned long long x = ++e->comm.seq_a;
    fp.rp.packed = e->comm.mb_own + Comm::data_offset(0, x);
    fp.peer_own = e->comm.mb_own; fp.peer_flag = (int)Comm::flag_index(0, x); fp.peer_seq = x;
    so.peer = peer_params(e); so.peer_world = e->comm.world; so.peer_flag = (int)Comm::flag_index(0, x);
    so.peer_off = (unsigned long long)Comm::data_offset(0, x); so.peer_seq = x;
    so.peer_timeout = (unsigned long long)(0.5 * e->wait_timeout_s * e->tick_hz);      // device-side wait: half the host watchdog, so that the recoverable error wins
    so.peer_err = e->h_comm_err_dev;
  }
  ev_begin(e, 3);
  hipLaunchKernelGGL(k_reduce_final, dim3(grid), dim3(kReduceThreads), 0, e->stream, fp);
  ev_end(e, 3);
  HIP_TRY(e, hipGetLastError());
  if (multi && !peer) {
    ev_begin(e, 5);
    if (e->comm.allreduce_device(e->d_packed, (size_t)pstride, 0, e->stream))
      return fail(e, PBA_ERR_COMM, "allreduce(reduced system) failed: %s", e->comm.err.c_str());
    ev_end(e, 5);
  }
  ev_begin(e, 4);
  if (e->prior_on) {      // (single rank: pba_set_camera_prior refuses the transports)
    PriorParams pp = prior_params(e, so.cams);
    pp.packed = e->d_packed;
    launch_prior(e, pp);
  }
  launch_solve(e, so, n);
  ev_end(e, 4);
  HIP_TRY(e, hipGetLastError());
  return PBA_OK;
}

void launch_schur(pba_engine* e, const SchurParams& sp) {
  hipLaunchKernelGGL(k_schur, dim3(e->schur_grid), dim3(kTile), 0, e->stream, sp);
}

// E_pts of the point prior at the points `xyz` (pba_point_prior.h): added to *add_to and / or stored to *out, in stream order
void launch_point_prior_cost(pba_engine* e, const double* xyz, double* add_to, double* out) {
  PointPriorCostParams cp{};
  cp.xyz = xyz; cp.x0 = e->d_pp_x0; cp.L6 = e->d_pp_L6; cp.part = e->d_pp_part; cp.ticket = e->d_pp_ticket; cp.add_to = add_to; cp.out = out;
  cp.n_points = e->n_points;
  const int grid = std::max(1, std::min(kPointPriorMaxGrid, (e->n_points + kPointPriorThreads - 1) / kPointPriorThreads));
  hipLaunchKernelGGL(k_point_prior_cost, dim3(grid), dim3(kPointPriorThreads), 0, e->stream, cp);
}

// ---- wide windows (pba_wide.h) ------------------------------------------------------------------------------------
// Co-observation lists, built on the host once per problem and camera set: for every pair of free cameras a <= b (enumerated
// row by row, as the packed pair blocks) the (observation of a, observation of b) of every point both observe, in point order,
// cut into chunks of kWideChunk.  A causal window is banded: pairs of cameras far apart share few points or none.
int wide_prepare(pba_engine* e) {
  if (e->wide_ready) return PBA_OK;
  const int nf = e->n_free, n_pairs = e->n_pairs;
  auto free_of = [&](int s) { return slot_free_index(e->anchor_mask, s); };
  auto pair_of = [&](int a, int b) { return a * nf - a * (a - 1) / 2 + (b - a); };
  std::vector<int64_t> off((size_t)n_pairs + 1, 0);
  int fa[kMaxFramesWide], lo[kMaxFramesWide];
  auto point_obs = [&](int p) {     // free-camera observations of point p (slots ascending, so free indices ascending)
    int k = 0;
    for (int o = e->h_pt_begin[p]; o < e->h_pt_begin[p + 1]; ++o) {
      const int f = free_of(e->h_obs_slot[o]);
      if (f >= 0) { fa[k] = f; lo[k] = o; ++k; }
    }
    return k;
  };
  for (int p = 0; p < e->n_points; ++p) {
    const int k = point_obs(p);
    for (int i = 0; i < k; ++i)
      for (int j = i; j < k; ++j) off[(size_t)pair_of(fa[i], fa[j]) + 1]++;
  }
  for (int q = 0; q < n_pairs; ++q) off[q + 1] += off[q];
  const int64_t n_ent = off[n_pairs];
  if (n_ent >= (1ll << 31) - kWideChunk)
    return fail(e, PBA_ERR_INVALID, "wide window: %lld co-observations exceed the int32 range of the pair lists", (long long)n_ent);
  std::vector<int2> ent((size_t)std::max<int64_t>(n_ent, 1));
  {
    std::vector<int64_t> fill(off.begin(), off.end() - 1);
    for (int p = 0; p < e->n_points; ++p) {
      const int k = point_obs(p);
      for (int i = 0; i < k; ++i)
        for (int j = i; j < k; ++j) ent[(size_t)fill[pair_of(fa[i], fa[j])]++] = make_int2(lo[i], lo[j]);
    }
  }
  std::vector<int4> chunks;
  std::vector<int32_t> pair_chunk((size_t)n_pairs + 1, 0);
  for (int q = 0, a = 0, b = 0; q < n_pairs; ++q) {
    pair_chunk[q] = (int32_t)chunks.size();
    for (int64_t c = off[q]; c < off[q + 1]; c += kWideChunk)
      chunks.push_back(make_int4((int)c, (int)std::min<int64_t>(c + kWideChunk, off[q + 1]), a == b ? 1 : 0, q));
    if (++b == nf) { ++a; b = a; }
  }
  pair_chunk[n_pairs] = (int32_t)chunks.size();
  e->wide_chunks = (int)chunks.size();
  e->wide_pt_blocks = (e->n_points + kWideThreads - 1) / kWideThreads;
  int rc;
  if ((rc = dev_alloc(e, &e->d_went, ent.size()))) return rc;
  if ((rc = dev_alloc(e, &e->d_wchunk, std::max<size_t>(chunks.size(), 1)))) return rc;
  if ((rc = dev_alloc(e, &e->d_wpair_chunk, pair_chunk.size()))) return rc;
  if ((rc = dev_alloc(e, &e->d_wsums, std::max<size_t>(chunks.size(), 1) * kWideVals))) return rc;
  if ((rc = dev_alloc(e, &e->d_wfac, (size_t)e->n_obs * kWideFac))) return rc;
  if ((rc = dev_alloc(e, &e->d_wpt_part, (size_t)3 * e->wide_pt_blocks))) return rc;
  HIP_TRY(e, hipMemcpyAsync(e->d_went, ent.data(), sizeof(int2) * ent.size(), hipMemcpyHostToDevice, e->stream));
  if (!chunks.empty()) HIP_TRY(e, hipMemcpyAsync(e->d_wchunk, chunks.data(), sizeof(int4) * chunks.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_wpair_chunk, pair_chunk.data(), sizeof(int32_t) * pair_chunk.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));      // (the host vectors go out of scope)
  e->wide_ready = true;
  return PBA_OK;
}

// Schur elimination of a wide window: point stage, pair stage, assembly into the packed reduced system (profiling: the Schur share)
int wide_eliminate(pba_engine* e, int cur, int init_scale, const pba_solver_options* o, double radius) {
  { const int rc = wide_prepare(e); if (rc) return rc; }
  WidePointParams wp{};
  wp.xyz = e->d_xyz[cur]; wp.geom = e->d_geom[cur]; wp.rec = e->d_rec[cur]; wp.pt_begin = e->d_pt_begin; wp.obs_slot = e->d_obs_slot;
  wp.sp = e->d_sp; wp.ptrec = e->d_ptrec; wp.fac = e->d_wfac; wp.part = e->d_wpt_part; wp.rec_stride = e->rec_stride;
  wp.n_points = e->n_points; wp.n_frames = e->n_frames; wp.init_scale = init_scale; wp.jacobi = o->jacobi_scaling;
  wp.fx = e->cfg.fx; wp.fy = e->cfg.fy; wp.inv_radius = 1.0 / radius; wp.min_diag = o->min_lm_diagonal; wp.max_diag = o->max_lm_diagonal;
  wp.prior_x0 = e->d_pp_x0; wp.prior_L6 = e->d_pp_L6;
  WidePairParams pp{};
  pp.fac = e->d_wfac; pp.ent = e->d_went; pp.chunk = e->d_wchunk; pp.out = e->d_wsums;
  WideAssembleParams ap{};
  ap.chunk_sums = e->d_wsums; ap.pair_chunk = e->d_wpair_chunk; ap.pt_part = e->d_wpt_part; ap.n_pt_blocks = e->wide_pt_blocks;
  ap.block_cost = e->d_block_cost[cur]; ap.block_fail = e->d_block_fail[cur]; ap.n_cost_blocks = e->cost_blocks[cur];
  ap.packed = e->d_packed; ap.scal = e->d_scal; ap.n_free = e->n_free; ap.n_pairs = e->n_pairs;
  ev_begin(e, 2);
  if (e->pp_on) hipLaunchKernelGGL(k_wide_point<true>, dim3(e->wide_pt_blocks), dim3(kWideThreads), 0, e->stream, wp);
  else hipLaunchKernelGGL(k_wide_point<false>, dim3(e->wide_pt_blocks), dim3(kWideThreads), 0, e->stream, wp);
  if (e->wide_chunks > 0) hipLaunchKernelGGL(k_wide_pairs, dim3(e->wide_chunks), dim3(kWideThreads), 0, e->stream, pp);
  hipLaunchKernelGGL(k_wide_assemble, dim3(e->n_pairs + 1), dim3(128), 0, e->stream, ap);
  // the point prior at the linearisation point joins the cost of the packed tail, last, after the photometric sum
  if (e->pp_on) launch_point_prior_cost(e, e->d_xyz[cur], e->d_packed + tri_index(6 * e->n_free + 1) + 2 * 6 * e->n_free, nullptr);
  ev_end(e, 2);
  HIP_TRY(e, hipGetLastError());
  return PBA_OK;
}

SampleParams make_sample_params(pba_engine* e, int which_point) {
  const int which_out = which_point;
  SampleParams sp{};
  sp.prec = sweep_mode(e);
  sp.frames = e->d_frames;
  sp.geom = e->d_geom[which_point];
  sp.xyz = e->d_xyz[which_point];
  sp.rays = rays_or_null(e);
  sp.desc = e->d_desc;
  sp.w2 = e->d_w2;
  sp.obs_point = e->d_obs_point;
  sp.obs_slot = e->d_obs_slot;
  sp.rec = e->d_rec[which_point];
  sp.block_cost = e->d_block_cost[which_out];
  sp.block_fail = e->d_block_fail[which_out];
  sp.rec_stride = e->rec_stride;
  sp.n_obs = e->n_obs;
  sp.n_frames = e->n_frames;
  sp.rows = e->cfg.rows;
  sp.cols = e->cfg.cols;
  sp.fx = e->cfg.fx; sp.fy = e->cfg.fy; sp.cx = e->cfg.cx; sp.cy = e->cfg.cy;
  sp.huber = e->cfg.huber;
  return sp;
}

// ONE sum all-reduce for the step scalars of all ranks (sum group + rank-slotted max group, see k_xchg_pack)
int ensure_xchg(pba_engine* e) {
  // grow-only and cheap when large enough: a transport re-initialised with a larger world must not overrun the buffer
  return dev_alloc(e, &e->d_xchg, (size_t)kSumBCount + (size_t)kMaxCount * e->comm.world);
}

// packed == true: the fused sampling kernel's last workgroup already filled the exchange buffer
int exchange_step_scalars(pba_engine* e, bool packed) {
  const int world = e->comm.world;
  const size_t n = (size_t)kSumBCount + (size_t)kMaxCount * world;
  int rc = ensure_xchg(e);
  if (rc) return rc;
  if (!packed) {
    hipLaunchKernelGGL(k_xchg_pack, dim3(1), dim3(64), 0, e->stream, e->d_scal, e->comm.peer ? peer_slot(e, 1) : e->d_xchg, e->comm.rank, world,
                       e->comm.peer ? 1 : 0);
    HIP_TRY(e, hipGetLastError());
  }
  ev_begin(e, 6);
  if (e->comm.peer) {
    const int rcp = peer_allreduce(e, 1, (int)n, e->d_xchg);
    if (rcp) return rcp;
  } else if (e->comm.allreduce_device(e->d_xchg, n, 0, e->stream)) {
    return fail(e, PBA_ERR_COMM, "allreduce(step scalars) failed: %s", e->comm.err.c_str());
  }
  ev_end(e, 6);
  return PBA_OK;
}

// the sequence number behind the scalars of the host mirror, at its device-visible address
unsigned long long* host_seq_dev(const pba_engine* e) { return reinterpret_cast<unsigned long long*>(e->h_scal_dev + kNumScal); }

// k_schur at the engine's buffers of parity `cur`: everything but what the device decides (async_schur_params adds that)
SchurParams schur_params(pba_engine* e, int cur, int init_scale, const pba_solver_options* o, double radius) {
  SchurParams sc{};
  sc.xyz = e->d_xyz[cur]; sc.rays = rays_or_null(e); sc.geom = e->d_geom[cur]; sc.rec = e->d_rec[cur]; sc.obs_point = e->d_obs_point;
  sc.obs_slot = e->d_obs_slot; sc.tile_info = e->d_tile_info; sc.lane_rec = e->d_lane_rec; sc.sp = e->d_sp;
  sc.ptrec = e->d_ptrec; sc.partial = e->d_partial; sc.rec_stride = e->rec_stride; sc.n_tiles = e->n_tiles; sc.n_frames = e->n_frames;
  sc.n_free = e->n_free; sc.n_pairs = e->n_pairs; sc.part_stride = e->part_stride; sc.init_scale = init_scale;
  sc.jacobi = o->jacobi_scaling; sc.fx = e->cfg.fx; sc.fy = e->cfg.fy; sc.radius = radius; sc.inv_radius = 1.0 / radius;
  sc.min_diag = o->min_lm_diagonal; sc.max_diag = o->max_lm_diagonal;
  return sc;
}
// the reduced solve at parity `cur`, likewise (with_cand: it also forms the candidate cameras' geometry for the fused sampling pass)
SolveParams solve_params(pba_engine* e, int cur, int init_scale, const pba_solver_options* o, double radius, bool with_cand) {
  const int cand = 1 - cur;
  SolveParams so{};
  so.packed = e->d_packed; so.cams = e->d_cams[cur]; so.cams_cand = e->d_cams[cand]; so.delta_c = e->d_delta_c;
  so.sc = e->d_sc; so.S_dbg = keep_system(e) ? e->d_S : nullptr; so.rhs_dbg = e->d_rhs; so.scal = e->d_scal; so.geom = e->d_geom[cur];
  so.n_frames = e->n_frames; so.n_free = e->n_free; so.n_pairs = e->n_pairs; so.stride = e->part_stride; so.anchor_mask = e->anchor_mask; so.tab = e->d_solve_tab;
  so.geom_cand = with_cand ? e->d_geom[cand] : nullptr;
  so.init_scale = init_scale; so.jacobi = o->jacobi_scaling; so.radius = radius; so.min_diag = o->min_lm_diagonal; so.max_diag = o->max_lm_diagonal;
  return so;
}
// multi-rank: the fused sampling kernel's last workgroup packs the step scalars into the exchange buffer (the peer mailbox slot, or d_xchg)
int set_sample_exchange(pba_engine* e, SampleParams& sp) {
  const int rc = ensure_xchg(e);
  if (rc) return rc;
  sp.xchg = e->comm.peer ? peer_slot(e, 1) : e->d_xchg; sp.xchg_sys = e->comm.peer ? 1 : 0;
  sp.xchg_rank = e->comm.rank; sp.xchg_world = e->comm.world;
  return PBA_OK;
}

// ---- phase-timing dumps of the host-stepped driver (PBA_SCHUR_TIMING with a TIMING=1 build) -----------------------------------------
void dump_schur_phase_cycles(pba_engine* e) {
  std::vector<unsigned long long> h(8 * (size_t)e->schur_grid);
  (void)hipMemcpyAsync(h.data(), e->d_dbg, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, e->stream);
  (void)hipStreamSynchronize(e->stream);
  double avg[8] = {0};
  for (int b = 0; b < e->schur_grid; ++b) for (int k = 0; k < 8; ++k) avg[k] += (double)h[8 * b + k] / e->schur_grid;
  std::fprintf(stderr, "k_schur phase cycles/block (stage, P1, point totals, P + camera record, camera sums, W|Y write, pair blocks): %.0f %.0f %.0f %.0f %.0f %.0f %.0f  tiles/block %.2f\n",
               avg[0], avg[1], avg[2], avg[3], avg[4], avg[5], avg[6], (double)e->n_tiles / e->schur_grid);
  {
    const int rem = e->n_tiles % e->schur_grid;   // blocks [0, rem) run one tile more than the others
    double d_long = 0, d_short = 0, d_max = 0; int n_long = 0, n_short = 0;
    for (int b = 0; b < e->schur_grid; ++b) {
      const double d = 0.01 * (double)h[8 * b + 7];
      d_max = std::max(d_max, d);
      if (b < rem) { d_long += d; ++n_long; } else { d_short += d; ++n_short; }
    }
    std::fprintf(stderr, "  k_schur tile loop: %d blocks with the extra tile %.2f us, %d others %.2f us, max %.2f us\n", n_long,
                 n_long ? d_long / n_long : 0.0, n_short, n_short ? d_short / n_short : 0.0, d_max);
  }
}
void dump_fused_sample_timeline(pba_engine* e, const unsigned long long* dbg) {
  const int fl = e->fused_grid;
  std::vector<unsigned long long> h(8 * (size_t)fl + 8);
  (void)hipMemcpyAsync(h.data(), dbg, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, e->stream);
  (void)hipStreamSynchronize(e->stream);
  double avg[8] = {0};
  for (int b = 0; b < fl; ++b) for (int k = 0; k < 6; ++k) avg[k] += (double)(h[8 * b + k] & 0xffffffffffffffull) / fl;
  // per-XCD timeline (the counters of different XCDs are not assumed to be synchronised)
  {
    unsigned long long g0 = ~0ull, g1 = 0;
    for (int b = 0; b < fl; ++b) { g0 = std::min(g0, h[8 * b + 6]); g1 = std::max(g1, h[8 * b + 7]); }
    double mean_dur = 0.0;
    for (int b = 0; b < fl; ++b) mean_dur += 0.01 * (double)(h[8 * b + 7] - h[8 * b + 6]) / fl;
    std::fprintf(stderr, "k_sample(fused) timeline: first start -> last end %.2f us, mean block duration %.2f us\n",
                 0.01 * (double)(g1 - g0), mean_dur);
    int hist[16] = {0};
    for (int b = 0; b < fl; ++b) { int k = (int)((h[8 * b + 6] - g0) / 400); hist[k > 15 ? 15 : k]++; }
    const unsigned long long* hf = &h[8 * (size_t)fl];
    std::fprintf(stderr, "  last workgroup: own work %.2f us, finalisation %.2f us (loads %.2f, reduce %.2f, decide %.2f)\n",
                 0.01 * (double)hf[1], 0.01 * (double)hf[0], 0.01 * (double)hf[2], 0.01 * (double)hf[3], 0.01 * (double)hf[4]);
    std::fprintf(stderr, "  block starts per 4 us bin:");
    for (int k = 0; k < 16; ++k) std::fprintf(stderr, " %d", hist[k]);
    std::fprintf(stderr, "\n");
  }
  for (int x = 0; x < 8; ++x) {
    unsigned long long t0 = ~0ull, t1 = 0; int n = 0; int late = 0;
    int mism = 0;
    for (int b = 0; b < fl; ++b) {
      if ((int)(h[8 * b] >> 56) != x) continue;
      t0 = std::min(t0, h[8 * b + 6]); t1 = std::max(t1, h[8 * b + 7]); ++n;
      if ((b & 7) != x) ++mism;
    }
    unsigned long long first_end = ~0ull;
    for (int b = 0; b < fl; ++b) if ((int)(h[8 * b] >> 56) == x) first_end = std::min(first_end, h[8 * b + 7]);
    for (int b = 0; b < fl; ++b) if ((int)(h[8 * b] >> 56) == x && h[8 * b + 6] >= first_end) ++late;
    (void)mism;
    std::fprintf(stderr, "  xcd %d: %d blocks, span %.2f us, first block done after %.2f us, %d blocks started later than that\n",
                 x, n, 0.01 * (double)(t1 - t0), 0.01 * (double)(first_end - t0), late);
  }
  std::fprintf(stderr, "k_sample(fused) phase cycles/block: geom-stage %.0f  backsub %.0f  geometry+base %.0f  staging %.0f  walk %.0f  loss+reduce %.0f\n",
               avg[0], avg[1], avg[2], avg[3], avg[4], avg[5]);
}

}  // namespace

extern "C" {

const char* pba_status_string(int s) {
  switch (s) {
    case PBA_OK: return "ok";
    case PBA_ERR_INVALID: return "invalid argument";
    case PBA_ERR_HIP: return "HIP runtime error";
    case PBA_ERR_NO_DEVICE: return "no HIP device (the engine has no CPU fallback)";
    case PBA_ERR_STATE: return "call order violated";
    case PBA_ERR_COMM: return "collective transport error";
    case PBA_ERR_NUMERIC: return "non-finite evaluation";
    default: return "unknown";
  }
}

const char* pba_last_error(const pba_engine* e) { return e ? e->err.c_str() : ""; }

void pba_default_solver_options(pba_solver_options* o) {
  o->max_num_iterations = 500;              // reference photobundle.cc:751
  o->max_num_consecutive_invalid_steps = 5;
  o->function_tolerance = 1e-6;             // :756
  o->gradient_tolerance = 1e-6;             // :757
  o->parameter_tolerance = 1e-6;            // :758
  o->initial_trust_region_radius = 1e4;     // Ceres defaults
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->jacobi_scaling = 1;
  o->verbose = 0;
}

int pba_create(const pba_config* cfg, pba_engine** out) {
  if (!cfg || !out) return PBA_ERR_INVALID;
  *out = nullptr;
  if (cfg->rows < 8 || cfg->cols < 8 || cfg->max_frames < 2 || cfg->max_frames > kMaxFramesWide || cfg->radius < 1 ||
      cfg->radius > kMaxRadius || (int64_t)cfg->rows * cfg->cols * cfg->max_frames >= (1ll << 31))
    return PBA_ERR_INVALID;
  if (cfg->channels < 0 || cfg->channels > PBA_MAX_CHANNELS ||
      (int64_t)cfg->rows * cfg->cols * cfg->max_frames * std::max(1, cfg->channels) >= (1ll << 31))
    return PBA_ERR_INVALID;
  if (cfg->channels > 1 && ((cfg->flags >> 1) & 3) != 0) return PBA_ERR_INVALID;   // the sweep modes are single-channel
  if (!device_exists(cfg->device)) return PBA_ERR_NO_DEVICE;
  pba_engine* e = new pba_engine();
  e->cfg = *cfg;
  int rc = PBA_OK;
  auto bail = [&](int code) { pba_destroy(e); return code; };
  if ((rc = handle_open(e, cfg->device))) return bail(rc);
  e->comm.stream = e->stream;
  const size_t npix = (size_t)cfg->rows * cfg->cols;
  if ((rc = dev_alloc(e, &e->d_frames, npix * cfg->max_frames))) return bail(rc);
  if ((rc = dev_alloc(e, &e->d_img_stage, npix))) return bail(rc);
  if ((rc = host_alloc(e, &e->h_img_stage, npix))) return bail(rc);
  if ((rc = handle_event(e, &e->ev_img_stage, hipEventDisableTiming))) return bail(rc);
  if (hipMemsetAsync(e->d_frames, 0, npix * cfg->max_frames * sizeof(uint32_t), e->stream) != hipSuccess) return bail(PBA_ERR_HIP);
  e->channels = std::max(1, cfg->channels);
  if (e->channels > 1) {
    if ((rc = dev_alloc(e, &e->d_frames_mc, npix * cfg->max_frames * e->channels))) return bail(rc);
    if (hipMemsetAsync(e->d_frames_mc, 0, npix * cfg->max_frames * e->channels * sizeof(float), e->stream) != hipSuccess) return bail(PBA_ERR_HIP);
  }
  e->frame_set.assign(cfg->max_frames, 0);
  // per-camera buffers: kMaxFrames slots as ever, more for an engine that may see a wide window
  const int mf = std::max(kMaxFrames, cfg->max_frames);
  for (int k = 0; k < 2; ++k) {
    if ((rc = dev_alloc(e, &e->d_cams[k], 6 * mf))) return bail(rc);
    if ((rc = dev_alloc(e, &e->d_geom[k], mf))) return bail(rc);
  }
  if ((rc = dev_alloc(e, &e->d_sc, 2 * 6 * mf))) return bail(rc);
  if ((rc = dev_alloc(e, &e->d_delta_c, 6 * mf))) return bail(rc);
  if ((rc = dev_alloc(e, &e->d_scal, (size_t)kNumScal))) return bail(rc);
  if ((rc = dev_alloc(e, &e->d_S, (size_t)36 * mf * mf))) return bail(rc);
  if ((rc = dev_alloc(e, &e->d_rhs, (size_t)6 * mf))) return bail(rc);
  if (hipMemsetAsync(e->d_scal, 0, kNumScal * sizeof(double), e->stream) != hipSuccess) return bail(PBA_ERR_HIP);
  if ((rc = host_alloc(e, &e->h_scal, (size_t)kNumScal + 1, &e->h_scal_dev))) return bail(rc);
  std::memset(e->h_scal, 0, (kNumScal + 1) * sizeof(double));
  if (const char* sv = getenv("PBA_SPECULATE")) e->speculate = atoi(sv) != 0;
  if (const char* sv = getenv("PBA_FUSE")) e->fuse = atoi(sv) != 0;
  if (const char* sv = getenv("PBA_ASYNC")) e->use_async = atoi(sv) != 0;
  if (const char* sv = getenv("PBA_RESIDENT")) e->use_resident = atoi(sv) != 0;
  if (const char* sv = getenv("PBA_RES_EPOCH0")) e->res_epoch = e->res_epoch_launch = (unsigned)strtoul(sv, nullptr, 0);      // test aid: start next to the restart of the epochs
  (void)hipDeviceGetAttribute(&e->n_cus, hipDeviceAttributeMultiprocessorCount, cfg->device);
  (void)hipDeviceGetAttribute(&e->coop_launch, hipDeviceAttributeCooperativeLaunch, cfg->device);
  if (hipDeviceGetAttribute(&e->lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device) != hipSuccess) e->lds_max = 0;
  if ((rc = dev_alloc(e, &e->d_res_sync, kResSyncBytes / sizeof(unsigned)))) return bail(rc);
  if (hipMemsetAsync(e->d_res_sync, 0, kResSyncBytes, e->stream) != hipSuccess) return bail(PBA_ERR_HIP);
  if (const char* sv = getenv("PBA_WAIT_TIMEOUT_S")) { const double v = atof(sv); if (v > 0.0) e->wait_timeout_s = v; }
  { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, cfg->device) == hipSuccess && khz > 0) e->tick_hz = 1e3 * khz; }
  if ((rc = dev_alloc(e, &e->d_lm, (size_t)1))) return bail(rc);
  if ((rc = host_alloc(e, &e->h_lm, (size_t)1, &e->h_lm_dev))) return bail(rc);
  if ((rc = host_alloc(e, &e->h_log, (size_t)pba_engine::kMaxLog, &e->h_log_dev))) return bail(rc);
  if ((rc = dev_alloc(e, &e->d_log, (size_t)pba_engine::kMaxLog))) return bail(rc);
  if (const char* sv = getenv("PBA_SCHUR_TIMING")) {
    if (PBA_PHASE_TIMING) e->dbg_left = atoi(sv);
    else std::fprintf(stderr, "PBA_SCHUR_TIMING ignored: libpba_hip.so was built without the phase stamps (make TIMING=1)\n");
  }
  if ((rc = dev_alloc(e, &e->d_ticket, (size_t)1))) return bail(rc);
  if (hipMemsetAsync(e->d_ticket, 0, sizeof(unsigned int), e->stream) != hipSuccess) return bail(PBA_ERR_HIP);
  if ((rc = host_alloc(e, &e->h_comm_err, (size_t)1, &e->h_comm_err_dev))) return bail(rc);
  *e->h_comm_err = 0;
  if ((rc = dev_alloc(e, &e->d_ticket_solve, (size_t)1))) return bail(rc);
  if (hipMemsetAsync(e->d_ticket_solve, 0, sizeof(unsigned int), e->stream) != hipSuccess) return bail(PBA_ERR_HIP);
  if (const char* sv = getenv("PBA_SOLVE")) e->solve_kind = atoi(sv);
  for (int k = 0; k < 2 * pba_engine::kEvPairs; ++k)
    if ((rc = handle_event(e, &e->ev[k]))) return bail(rc);
  if ((rc = handle_event(e, &e->ev_xdep, hipEventDisableTiming))) return bail(rc);
  e->sample_waves = sample_waves_for_radius(cfg->radius);
  if ((rc = host_alloc(e, &e->h_state_stage, (size_t)6 * mf + 3 * 65536, &e->h_state_dev))) return bail(rc);   // grown on demand beyond 64k points
  // The first frame-sized host -> device DMA of a process costs ~8 ms (seen in the drop-in class: first
  // pba_set_frame_u8): paid here, from the engine's own pinned buffer
  if (hipMemcpyAsync(e->d_img_stage, e->h_img_stage, npix, hipMemcpyHostToDevice, e->stream) != hipSuccess) return bail(PBA_ERR_HIP);
  // loads this library's code object now rather than at the first frame (10+ ms in a process that has not touched it yet)
  hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, e->stream);
  if (hipGetLastError() != hipSuccess) return bail(PBA_ERR_HIP);
  // (The first COOPERATIVE launch of a process -- the resident solve's kind -- sets up a queue of its own, ~10 ms.  It is NOT paid here:
  // a cooperative queue is exclusive on the device, so two processes that share one GPU -- two ranks on one device in the tests -- then
  // time-slice at ~20 ms per LM step (measured: 139 us -> 22.5 ms), and rocprofv3 crashes in its exit handlers once a process has made
  // a cooperative launch (its output files are complete by then).  The first resident solve pays it; multi-rank engines never make one.)
  if (hipStreamSynchronize(e->stream) != hipSuccess) return bail(PBA_ERR_HIP);
  *out = e;
  return PBA_OK;
}

void pba_destroy(pba_engine* e) {
  if (!e) return;
  if (e->poisoned) {
    // the stream holds work that will never finish (pba_step / pba_solve timed out): waiting for it, freeing memory it
    // may still touch or destroying its stream would hang or fault; abort the communicator and leak the device side
    (void)hipSetDevice(e->cfg.device);
    e->mem.abandon();
    e->comm.shutdown(true);
    delete e;
    return;
  }
  handle_drain(e);
  e->comm.shutdown();
  handle_close(e);
  delete e;
}

int pba_set_frame_channels_f32(pba_engine* e, int slot, int32_t n_channels, const float* channels) {
  if (!e || !channels || slot < 0 || slot >= e->cfg.max_frames) return PBA_ERR_INVALID;
  if (e->channels <= 1 || n_channels != e->channels)
    return fail(e, PBA_ERR_INVALID, "pba_set_frame_channels_f32: the engine was created for %d channel(s), got %d", e->channels, n_channels);
  PBA_ENTER(e);
  const size_t npix = (size_t)e->cfg.rows * e->cfg.cols;
  // the slot keeps the channel VALUES as they come ([C][rows*cols], the layout of the argument): one copy, no kernel; the
  // caller's buffer is only borrowed for the call
  HIP_TRY(e, hipMemcpyAsync(e->d_frames_mc + (size_t)slot * n_channels * npix, channels, (size_t)n_channels * npix * sizeof(float),
                            hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return frame_uploaded(e, slot, false);
}

int pba_set_frame_u8(pba_engine* e, int slot, const uint8_t* image) {
  if (!e || !image || slot < 0 || slot >= e->cfg.max_frames) return PBA_ERR_INVALID;
  if (e->channels > 1) return fail(e, PBA_ERR_INVALID, "pba_set_frame_u8: the engine was created for %d channels (pba_set_frame_channels_f32)", e->channels);
  PBA_ENTER(e);
  const size_t npix = (size_t)e->cfg.rows * e->cfg.cols;
  // The caller's buffer is only borrowed for the call: it is copied into a pinned staging buffer here, and the upload +
  // packing run asynchronously behind the return (a pageable hipMemcpy plus a stream sync cost ~1.2 ms per frame).
  // The previous use of the staging buffers is awaited first; it normally finished long ago.
  if (e->img_stage_busy) { HIP_TRY(e, hipEventSynchronize(e->ev_img_stage)); e->img_stage_busy = false; }
  std::memcpy(e->h_img_stage, image, npix);
  HIP_TRY(e, hipMemcpyAsync(e->d_img_stage, e->h_img_stage, npix, hipMemcpyHostToDevice, e->stream));
  dim3 grid((e->cfg.cols + 255) / 256, e->cfg.rows);
  hipLaunchKernelGGL(k_pack_frame, grid, dim3(256), 0, e->stream, e->d_img_stage, e->d_frames + npix * slot,
                     e->cfg.rows, e->cfg.cols);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev_img_stage, e->stream));
  e->img_stage_busy = true;
  return frame_uploaded(e, slot, true);
}

int pba_get_frame_planes(pba_engine* e, int slot, float* I, float* Gx, float* Gy) {
  if (!e || slot < 0 || slot >= e->cfg.max_frames || !I || !Gx || !Gy) return PBA_ERR_INVALID;
  if (e->channels > 1) return fail(e, PBA_ERR_INVALID, "pba_get_frame_planes reads the single-channel planes");
  PBA_ENTER(e);
  const size_t npix = (size_t)e->cfg.rows * e->cfg.cols;
  DeviceTemp<float> tmp;
  HIP_TRY(e, tmp.alloc(3 * npix));
  float* d = tmp.p;
  hipLaunchKernelGGL(k_unpack_frame, dim3((npix + 255) / 256), dim3(256), 0, e->stream, e->d_frames + npix * slot, d,
                     d + npix, d + 2 * npix, (int)npix);
  HIP_TRY(e, hipMemcpyAsync(I, d, npix * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(Gx, d + npix, npix * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(Gy, d + 2 * npix, npix * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_get_frame_channel(pba_engine* e, int slot, int32_t channel, float* I, float* Gx, float* Gy) {
  if (!e || slot < 0 || slot >= e->cfg.max_frames || !I || !Gx || !Gy) return PBA_ERR_INVALID;
  if (e->channels <= 1 || channel < 0 || channel >= e->channels)
    return fail(e, PBA_ERR_INVALID, "pba_get_frame_channel: channel %d of an engine with %d channel(s)", channel, e->channels);
  PBA_ENTER(e);
  const size_t npix = (size_t)e->cfg.rows * e->cfg.cols;
  DeviceTemp<float> tmp;
  HIP_TRY(e, tmp.alloc(3 * npix));
  float* d = tmp.p;
  hipLaunchKernelGGL(k_unpack_channel, dim3((e->cfg.cols + 255) / 256, e->cfg.rows), dim3(256), 0, e->stream,
                     (const float*)e->d_frames_mc + ((size_t)slot * e->channels + channel) * npix, e->cfg.rows, e->cfg.cols, d, d + npix, d + 2 * npix);
  HIP_TRY(e, hipMemcpyAsync(I, d, npix * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(Gx, d + npix, npix * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(Gy, d + 2 * npix, npix * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_get_frame_channels_f32(pba_engine* e, int slot, float* channels) {
  if (!e || slot < 0 || slot >= e->cfg.max_frames || !channels) return PBA_ERR_INVALID;
  if (e->channels <= 1) return fail(e, PBA_ERR_INVALID, "pba_get_frame_channels_f32: single-channel engine");
  if (!e->frame_set[slot]) return fail(e, PBA_ERR_STATE, "pba_get_frame_channels_f32: slot %d holds no frame", slot);
  PBA_ENTER(e);
  const size_t n = (size_t)e->channels * e->cfg.rows * e->cfg.cols;
  HIP_TRY(e, hipMemcpyAsync(channels, e->d_frames_mc + (size_t)slot * n, n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_sample_frame(pba_engine* e, int slot, int32_t channel, int32_t n, const float* y, const float* x, float* out3) {
  if (!e || slot < 0 || slot >= e->cfg.max_frames || n <= 0 || !y || !x || !out3 || channel < 0 || channel >= e->channels) return PBA_ERR_INVALID;
  if (!e->frame_set[slot]) return fail(e, PBA_ERR_STATE, "pba_sample_frame: slot %d holds no frame", slot);
  PBA_ENTER(e);
  const size_t npix = (size_t)e->cfg.rows * e->cfg.cols;
  DeviceTemp<float> tmp;
  HIP_TRY(e, tmp.alloc((size_t)5 * n));
  float* d = tmp.p;
  HIP_TRY(e, hipMemcpyAsync(d, y, (size_t)n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(d + n, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  if (e->channels > 1)
    hipLaunchKernelGGL(k_sample_probe_mc, dim3((n + 255) / 256), dim3(256), 0, e->stream,
                       (const float*)e->d_frames_mc + ((size_t)slot * e->channels + channel) * npix, e->cfg.rows, e->cfg.cols, n,
                       (const float*)d, (const float*)(d + n), d + 2 * (size_t)n);
  else
    hipLaunchKernelGGL(k_sample_probe, dim3((n + 255) / 256), dim3(256), 0, e->stream, (const uint32_t*)(e->d_frames + npix * slot),
                       e->cfg.rows, e->cfg.cols, n, (const float*)d, (const float*)(d + n), d + 2 * (size_t)n);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(out3, d + 2 * (size_t)n, (size_t)3 * n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

// cv::getGaussianKernel(n, sigma > 0, CV_32F) as host/imgproc.h gaussianKernel restates it
static void gaussian_kernel_f32(int n, double sigma, float* k) {
  const double scale2x = -0.5 / (sigma * sigma);
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    k[i] = (float)std::exp(scale2x * x * x);
    sum += k[i];
  }
  sum = 1.0 / sum;
  for (int i = 0; i < n; ++i) k[i] = (float)(k[i] * sum);
}

int pba_set_frame_descriptor_u8(pba_engine* e, int slot, const uint8_t* image, int32_t descriptor, float sigma_ct, float sigma_bp) {
  if (!e || !image || slot < 0 || slot >= e->cfg.max_frames) return PBA_ERR_INVALID;
  if (descriptor == PBA_DESCRIPTOR_INTENSITY) return pba_set_frame_u8(e, slot, image);
  const int want = descriptor == PBA_DESCRIPTOR_INTENSITY_AND_GRADIENT ? 3 : descriptor == PBA_DESCRIPTOR_BITPLANES ? 8 : 0;
  if (!want) return fail(e, PBA_ERR_INVALID, "pba_set_frame_descriptor_u8: unknown descriptor %d", descriptor);
  if (e->channels != want)
    return fail(e, PBA_ERR_INVALID, "pba_set_frame_descriptor_u8: descriptor %d has %d channels, the engine was created for %d", descriptor, want, e->channels);
  PBA_ENTER(e);
  const int rows = e->cfg.rows, cols = e->cfg.cols;
  const size_t npix = (size_t)rows * cols;
  int rc;
  if (descriptor == PBA_DESCRIPTOR_BITPLANES)
    for (int k = 0; k < 2; ++k)
      if (!e->d_u8_work[k] && (rc = dev_alloc(e, &e->d_u8_work[k], npix))) return rc;
  // same borrowed-buffer protocol as pba_set_frame_u8: pinned copy, everything else asynchronous behind the return
  if (e->img_stage_busy) { HIP_TRY(e, hipEventSynchronize(e->ev_img_stage)); e->img_stage_busy = false; }
  std::memcpy(e->h_img_stage, image, npix);
  HIP_TRY(e, hipMemcpyAsync(e->d_img_stage, e->h_img_stage, npix, hipMemcpyHostToDevice, e->stream));
  const dim3 grid((cols + 255) / 256, rows), block(256);
  float* planes = e->d_frames_mc + (size_t)slot * want * npix;      // the slot's channel planes: produced in place
  if (descriptor == PBA_DESCRIPTOR_INTENSITY_AND_GRADIENT) {
    hipLaunchKernelGGL(k_channels_intensity_gradient, grid, block, 0, e->stream, (const uint8_t*)e->d_img_stage, planes, rows, cols);
  } else {
    const uint8_t* src = e->d_img_stage;
    if (sigma_ct > 0.0f) {
      float kf[3];
      gaussian_kernel_f32(3, (double)sigma_ct, kf);
      int ki[3];
      for (int i = 0; i < 3; ++i) ki[i] = (int)std::nearbyint((double)kf[i] * 256.0);
      hipLaunchKernelGGL(k_blur3_u8, grid, block, 0, e->stream, src, e->d_u8_work[0], rows, cols, ki[0], ki[1], ki[2]);
      src = e->d_u8_work[0];
    }
    hipLaunchKernelGGL(k_census, grid, block, 0, e->stream, src, e->d_u8_work[1], rows, cols);
    float k5[5] = {0.f, 0.f, 1.f, 0.f, 0.f};
    if (sigma_bp > 0.0f) gaussian_kernel_f32(5, (double)sigma_bp, k5);
    hipLaunchKernelGGL(k_bitplanes, grid, block, 0, e->stream, (const uint8_t*)e->d_u8_work[1], planes, rows, cols,
                       sigma_bp > 0.0f ? 1 : 0, k5[0], k5[1], k5[2]);
  }
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev_img_stage, e->stream));
  e->img_stage_busy = true;
  return frame_uploaded(e, slot, true);
}

int pba_set_frame_pyr_down(pba_engine* e, int slot, pba_engine* finer, int finer_slot, uint8_t* image_out) {
  if (!e || !finer || e == finer || slot < 0 || slot >= e->cfg.max_frames || finer_slot < 0 || finer_slot >= finer->cfg.max_frames)
    return PBA_ERR_INVALID;
  if (e->channels > 1 || finer->channels > 1) return fail(e, PBA_ERR_INVALID, "pba_set_frame_pyr_down: single-channel engines only");
  if (e->cfg.device != finer->cfg.device) return fail(e, PBA_ERR_INVALID, "pba_set_frame_pyr_down: the two engines live on devices %d and %d", e->cfg.device, finer->cfg.device);
  const int rows = finer->cfg.rows, cols = finer->cfg.cols, drows = (rows + 1) / 2, dcols = (cols + 1) / 2;
  if (e->cfg.rows != drows || e->cfg.cols != dcols)
    return fail(e, PBA_ERR_INVALID, "pba_set_frame_pyr_down: %dx%d is not the next level of %dx%d (%dx%d)", e->cfg.rows, e->cfg.cols, rows, cols, drows, dcols);
  if (!finer->frame_set[finer_slot]) return fail(e, PBA_ERR_STATE, "pba_set_frame_pyr_down: slot %d of the finer level holds no frame", finer_slot);
  PBA_NOT_POISONED(e);
  PBA_NOT_POISONED(finer);
  HIP_TRY(e, hipSetDevice(e->cfg.device));
  // the finer frame is produced on the other engine's stream
  HIP_TRY(e, hipEventRecord(finer->ev_xdep, finer->stream));
  HIP_TRY(e, hipStreamWaitEvent(e->stream, finer->ev_xdep, 0));
  const dim3 grid((dcols + 255) / 256, drows), block(256);
  hipLaunchKernelGGL(k_pyr_down<uint32_t>, grid, block, 0, e->stream, (const uint32_t*)(finer->d_frames + (size_t)rows * cols * finer_slot),
                     e->d_img_stage, rows, cols, drows, dcols);
  // ... and must not be overwritten there before it has been read here
  HIP_TRY(e, hipEventRecord(e->ev_xdep, e->stream));
  HIP_TRY(e, hipStreamWaitEvent(finer->stream, e->ev_xdep, 0));
  hipLaunchKernelGGL(k_pack_frame, grid, block, 0, e->stream, (const uint8_t*)e->d_img_stage, e->d_frames + (size_t)drows * dcols * slot, drows, dcols);
  HIP_TRY(e, hipGetLastError());
  if (image_out) {
    HIP_TRY(e, hipMemcpyAsync(image_out, e->d_img_stage, (size_t)drows * dcols, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
  }
  return frame_uploaded(e, slot, true);
}

// ---- device front-end ---------------------------------------------------------------------------------------------------
static int fe_stage(pba_engine* e, size_t bytes) { return host_alloc(e, &e->h_fe_io, bytes); }      // pinned staging buffer of the front-end calls

int pba_frontend_visibility(pba_engine* e, int32_t n, const double* uv, const int32_t* rc, const float* patches26, double min_score,
                            int32_t mask_radius, uint8_t* hit) {
  if (!e || n < 0 || mask_radius < 0 || (n > 0 && (!uv || !rc || !patches26 || !hit))) return PBA_ERR_INVALID;
  PBA_NOT_POISONED(e);
  if (n > 0 && !e->img_stage_valid)
    return fail(e, PBA_ERR_STATE, "pba_frontend_visibility: no u8 frame behind the ZNCC (upload one with pba_set_frame_u8 / _descriptor_u8 / _pyr_down first)");
  HIP_TRY(e, hipSetDevice(e->cfg.device));
  const int rows = e->cfg.rows, cols = e->cfg.cols;
  const size_t npix = (size_t)rows * cols;
  int rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_mask, npix))) return rcode;
  HIP_TRY(e, hipMemsetAsync(e->d_fe_mask, 1, npix, e->stream));
  e->fe_mask_valid = true;
  if (n == 0) return PBA_OK;
  for (int i = 0; i < n; ++i)
    if (rc[2 * i] < mask_radius || rc[2 * i] >= rows - mask_radius || rc[2 * i + 1] < mask_radius || rc[2 * i + 1] >= cols - mask_radius)
      return fail(e, PBA_ERR_INVALID, "pba_frontend_visibility: point %d at (row %d, col %d) is closer than the mask radius to the border", i, rc[2 * i], rc[2 * i + 1]);
  // one upload: uv (16 B) | patches (104 B) | rc (8 B) per point; hits come back through the same pinned buffer
  const size_t o_uv = 0, o_pt = o_uv + (size_t)n * 16, o_rc = o_pt + (size_t)n * 104, o_hit = o_rc + (size_t)n * 8, total = o_hit + (size_t)n;
  if ((rcode = fe_stage(e, total))) return rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_io, total + total / 4))) return rcode;
  std::memcpy(e->h_fe_io + o_uv, uv, (size_t)n * 16);
  std::memcpy(e->h_fe_io + o_pt, patches26, (size_t)n * 104);
  std::memcpy(e->h_fe_io + o_rc, rc, (size_t)n * 8);
  HIP_TRY(e, hipMemcpyAsync(e->d_fe_io, e->h_fe_io, o_hit, hipMemcpyHostToDevice, e->stream));
  uint8_t* d_hit = reinterpret_cast<uint8_t*>(e->d_fe_io + o_hit);
  hipLaunchKernelGGL(k_fe_visibility, dim3((n + 127) / 128), dim3(128), 0, e->stream, (const uint8_t*)e->d_img_stage, rows, cols, n,
                     reinterpret_cast<const double*>(e->d_fe_io + o_uv), reinterpret_cast<const float*>(e->d_fe_io + o_pt), min_score, d_hit, (float*)nullptr);
  hipLaunchKernelGGL(k_fe_mask_stamp, dim3((n + 255) / 256), dim3(256), 0, e->stream, n, reinterpret_cast<const int2*>(e->d_fe_io + o_rc),
                     (const uint8_t*)d_hit, mask_radius, e->d_fe_mask, cols);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(e->h_fe_io + o_hit, d_hit, (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  std::memcpy(hit, e->h_fe_io + o_hit, (size_t)n);
  return PBA_OK;
}

int pba_frontend_zncc_probe(pba_engine* e, int32_t n, const double* uv, const float* patches26, float* out27) {
  if (!e || n <= 0 || !uv || !patches26 || !out27) return PBA_ERR_INVALID;
  PBA_NOT_POISONED(e);
  if (!e->img_stage_valid)
    return fail(e, PBA_ERR_STATE, "pba_frontend_zncc_probe: no u8 frame behind the ZNCC (upload one with pba_set_frame_u8 / _descriptor_u8 / _pyr_down first)");
  HIP_TRY(e, hipSetDevice(e->cfg.device));
  const size_t o_pt = (size_t)n * 16, o_out = o_pt + (size_t)n * 104, total = o_out + (size_t)n * 108;
  int rcode;
  if ((rcode = fe_stage(e, total))) return rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_io, total + total / 4))) return rcode;
  std::memcpy(e->h_fe_io, uv, (size_t)n * 16);
  std::memcpy(e->h_fe_io + o_pt, patches26, (size_t)n * 104);
  HIP_TRY(e, hipMemcpyAsync(e->d_fe_io, e->h_fe_io, o_out, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_fe_visibility, dim3((n + 127) / 128), dim3(128), 0, e->stream, (const uint8_t*)e->d_img_stage, e->cfg.rows, e->cfg.cols, n,
                     reinterpret_cast<const double*>(e->d_fe_io), reinterpret_cast<const float*>(e->d_fe_io + o_pt), 0.0, (uint8_t*)nullptr,
                     reinterpret_cast<float*>(e->d_fe_io + o_out));
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(e->h_fe_io + o_out, e->d_fe_io + o_out, (size_t)n * 108, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  std::memcpy(out27, e->h_fe_io + o_out, (size_t)n * 108);
  return PBA_OK;
}

int pba_frontend_candidates(pba_engine* e, int32_t slot, const float* depth, double min_depth, double max_depth, int32_t nms_radius,
                            int32_t border, int32_t* n_out) {
  if (!e || !depth || !n_out || slot < 0 || slot >= e->cfg.max_frames || border < 0) return PBA_ERR_INVALID;
  if (!e->frame_set[slot]) return fail(e, PBA_ERR_STATE, "pba_frontend_candidates: slot %d holds no frame", slot);
  if (nms_radius > border) return fail(e, PBA_ERR_INVALID, "pba_frontend_candidates: nms radius %d reaches over the border %d", nms_radius, border);
  if (2 * border >= e->cfg.rows || 2 * border >= e->cfg.cols)
    return fail(e, PBA_ERR_INVALID, "pba_frontend_candidates: border %d leaves no interior in a %d x %d image", border, e->cfg.rows, e->cfg.cols);
  PBA_ENTER(e);
  const int rows = e->cfg.rows, cols = e->cfg.cols;
  const size_t npix = (size_t)rows * cols;
  int rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_mask, npix))) return rcode;
  if (!e->fe_mask_valid) HIP_TRY(e, hipMemsetAsync(e->d_fe_mask, 1, npix, e->stream));      // no visibility call for this frame: nothing is masked
  e->fe_mask_valid = false;       // (consumed: the next frame starts from a fresh mask)
  if ((rcode = dev_alloc(e, &e->d_fe_flag, npix))) return rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_smap, npix))) return rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_depth, npix))) return rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_rows, (size_t)2 * rows + 1))) return rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_cand, npix))) return rcode;
  if ((rcode = fe_stage(e, npix * sizeof(float)))) return rcode;
  std::memcpy(e->h_fe_io, depth, npix * sizeof(float));
  HIP_TRY(e, hipMemcpyAsync(e->d_fe_depth, e->h_fe_io, npix * sizeof(float), hipMemcpyHostToDevice, e->stream));
  const dim3 grid((cols + 255) / 256, rows), block(256);
  const bool mc = e->channels > 1;
  hipLaunchKernelGGL(k_fe_saliency, grid, block, 0, e->stream, (const uint32_t*)(e->d_frames + npix * slot),
                     mc ? (const float*)(e->d_frames_mc + (size_t)slot * e->channels * npix) : (const float*)nullptr, e->channels, rows, cols, e->d_fe_smap);
  CandParams cp{};
  cp.smap = e->d_fe_smap; cp.depth = e->d_fe_depth; cp.mask = e->d_fe_mask; cp.rows = rows; cp.cols = cols; cp.border = border; cp.nms = nms_radius;
  cp.min_depth = min_depth; cp.max_depth = max_depth; cp.flag = e->d_fe_flag; cp.row_count = e->d_fe_rows; cp.row_offset = e->d_fe_rows + rows;
  cp.out = e->d_fe_cand;
  hipLaunchKernelGGL(k_fe_cand_flags, dim3(rows), dim3(256), 0, e->stream, cp);
  hipLaunchKernelGGL(k_fe_scan_rows, dim3(1), dim3(256), 0, e->stream, (const int32_t*)cp.row_count, cp.row_offset, rows);
  hipLaunchKernelGGL(k_fe_cand_write, dim3(rows), dim3(256), 0, e->stream, cp);
  HIP_TRY(e, hipGetLastError());
  int32_t* h_n = reinterpret_cast<int32_t*>(e->h_fe_io);
  HIP_TRY(e, hipMemcpyAsync(h_n, cp.row_offset + rows, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  e->fe_n_cand = *h_n;
  *n_out = e->fe_n_cand;
  return PBA_OK;
}

int pba_frontend_get_candidates(pba_engine* e, pba_candidate* out, int32_t n) {
  if (!e || n < 0 || (n > 0 && !out)) return PBA_ERR_INVALID;
  if (n > e->fe_n_cand) return fail(e, PBA_ERR_STATE, "pba_frontend_get_candidates: %d requested, the last scan found %d", n, e->fe_n_cand);
  if (n == 0) return PBA_OK;
  PBA_ENTER(e);
  { const int rcode = fe_stage(e, (size_t)n * sizeof(pba_candidate)); if (rcode) return rcode; }
  HIP_TRY(e, hipMemcpyAsync(e->h_fe_io, e->d_fe_cand, (size_t)n * sizeof(pba_candidate), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  std::memcpy(out, e->h_fe_io, (size_t)n * sizeof(pba_candidate));
  return PBA_OK;
}

int pba_frontend_descriptors(pba_engine* e, int32_t slot, int32_t n, const int32_t* xy, float* desc) {
  if (!e || n < 0 || slot < 0 || slot >= e->cfg.max_frames || (n > 0 && (!xy || !desc))) return PBA_ERR_INVALID;
  if (!e->frame_set[slot]) return fail(e, PBA_ERR_STATE, "pba_frontend_descriptors: slot %d holds no frame", slot);
  if (n == 0) return PBA_OK;
  PBA_ENTER(e);
  const int rows = e->cfg.rows, cols = e->cfg.cols, R = e->cfg.radius, P = (2 * R + 1) * (2 * R + 1);
  const size_t npix = (size_t)rows * cols;
  const size_t b_xy = (size_t)n * 8, b_out = (size_t)n * e->channels * P * sizeof(float);
  int rcode;
  if ((rcode = fe_stage(e, b_xy + b_out))) return rcode;
  if ((rcode = dev_alloc(e, &e->d_fe_io, b_xy + b_out + (b_xy + b_out) / 4))) return rcode;
  std::memcpy(e->h_fe_io, xy, b_xy);
  HIP_TRY(e, hipMemcpyAsync(e->d_fe_io, e->h_fe_io, b_xy, hipMemcpyHostToDevice, e->stream));
  const bool mc = e->channels > 1;
  const size_t total = (size_t)n * e->channels * P;
  hipLaunchKernelGGL(k_fe_descriptors, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, e->stream,
                     (const uint32_t*)(e->d_frames + npix * slot), mc ? (const float*)(e->d_frames_mc + (size_t)slot * e->channels * npix) : (const float*)nullptr,
                     e->channels, rows, cols, R, n, reinterpret_cast<const int2*>(e->d_fe_io), reinterpret_cast<float*>(e->d_fe_io + b_xy));
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(e->h_fe_io + b_xy, e->d_fe_io + b_xy, b_out, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  std::memcpy(desc, e->h_fe_io + b_xy, b_out);
  return PBA_OK;
}

// The part of a problem that follows from its observation lists alone, shared by pba_set_problem and an applied pba_cull.
struct ProblemLayout {
  std::vector<int32_t> pt_begin;
  std::vector<uint8_t> slot8;
  std::vector<int4> tinfo;
  std::vector<int2> lane_rec;
};
// validate + CSR + tiles (whole points per tile of <= kTile observations); sets n_tiles, n_points, n_obs
static int problem_layout(pba_engine* e, int32_t n_points, int32_t n_obs, const int32_t* obs_point, const int32_t* obs_slot, ProblemLayout* L) {
  std::vector<int32_t>& pt_begin = L->pt_begin;
  std::vector<uint8_t>& slot8 = L->slot8;
  pt_begin.assign((size_t)n_points + 1, 0);
  slot8.resize(n_obs);
  for (int o = 0; o < n_obs; ++o) {
    const int p = obs_point[o], s = obs_slot[o];
    if (p < 0 || p >= n_points || s < 0 || s >= e->cfg.max_frames) return fail(e, PBA_ERR_INVALID, "observation %d out of range", o);
    if (o > 0 && p < obs_point[o - 1]) return fail(e, PBA_ERR_INVALID, "observations must be grouped by point");
    if (o > 0 && p == obs_point[o - 1] && s <= obs_slot[o - 1]) return fail(e, PBA_ERR_INVALID, "duplicate / unsorted slot for point %d", p);
    pt_begin[p + 1]++;
    slot8[o] = (uint8_t)s;
  }
  for (int p = 0; p < n_points; ++p) {
    if (pt_begin[p + 1] == 0) return fail(e, PBA_ERR_INVALID, "point %d has no observation", p);
    pt_begin[p + 1] += pt_begin[p];
  }
  std::vector<int32_t> tiles(1, 0);
  {
    int begin = 0;
    for (int p = 0; p < n_points; ++p) {
      if (pt_begin[p + 1] - begin > kTile) { tiles.push_back(pt_begin[p]); begin = pt_begin[p]; }
    }
    tiles.push_back(n_obs);
  }
  e->n_tiles = (int)tiles.size() - 1;
  L->tinfo.resize(e->n_tiles);
  L->lane_rec.assign((size_t)e->n_tiles * kTile, make_int2(0, 0));
  for (int t = 0; t < e->n_tiles; ++t) {
    const int o0 = tiles[t], o1 = tiles[t + 1];
    L->tinfo[t] = make_int4(o0, o1 - o0, obs_point[o0], obs_point[o1 - 1] - obs_point[o0] + 1);
    for (int o = o0; o < o1; ++o) {
      const int p = obs_point[o];
      L->lane_rec[(size_t)t * kTile + (o - o0)] = make_int2(p, (int)slot8[o] | ((pt_begin[p] - o0) << 8) | ((pt_begin[p + 1] - pt_begin[p]) << 16));
    }
  }
  e->n_points = n_points;
  e->n_obs = n_obs;
  e->ctr.n_obs = n_obs; e->ctr.n_points = n_points;
  return PBA_OK;
}
// every buffer and launch shape sized by n_points / n_obs / n_tiles (PD: descriptor entries per point)
static int problem_reserve(pba_engine* e, const ProblemLayout& L, int PD) {
  const int n_points = e->n_points, n_obs = e->n_obs;
  int rc;
  for (int k = 0; k < 2; ++k) if ((rc = dev_alloc(e, &e->d_xyz[k], (size_t)3 * n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_desc, (size_t)n_points * PD))) return rc;
  if ((rc = dev_alloc(e, &e->d_obs_point, (size_t)n_obs))) return rc;
  if ((rc = dev_alloc(e, &e->d_obs_slot, (size_t)n_obs))) return rc;
  if ((rc = dev_alloc(e, &e->d_pt_begin, (size_t)n_points + 1))) return rc;
  if ((rc = dev_alloc(e, &e->d_tile_info, L.tinfo.size()))) return rc;
  if ((rc = dev_alloc(e, &e->d_lane_rec, L.lane_rec.size()))) return rc;
  e->rec_stride = ((int64_t)n_obs + 255) / 256 * 256;
  for (int k = 0; k < 2; ++k) if ((rc = dev_alloc(e, &e->d_rec[k], (size_t)6 * e->rec_stride))) return rc;
  if ((rc = dev_alloc(e, &e->d_sp, (size_t)3 * n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_ptrec, (size_t)12 * n_points))) return rc;
  e->sample_grid = (n_obs + e->sample_waves * 64 - 1) / (e->sample_waves * 64);
  {
    const int tiles_per_block = std::max(1, e->sample_waves * 64 / kTile);
    e->fused_grid = (e->n_tiles + tiles_per_block - 1) / tiles_per_block;
  }
  const int cost_blocks = std::max(e->sample_grid, e->fused_grid);
  for (int k = 0; k < 2; ++k) {
    if ((rc = dev_alloc(e, &e->d_block_cost[k], (size_t)cost_blocks))) return rc;
    if ((rc = dev_alloc(e, &e->d_block_fail[k], (size_t)cost_blocks))) return rc;
    e->cost_blocks[k] = 0;
  }
  e->backsub_grid = (n_points + 255) / 256;
  if ((rc = dev_alloc(e, &e->d_bs_out, (size_t)3 * std::max(e->backsub_grid, e->fused_grid)))) return rc;
  e->schur_grid = std::min(e->n_tiles, 256 * 4);
  // (experiment switch: workgroups of the persistent k_schur launch; the partial buffers are sized for <= 1024)
  if (const char* sv = getenv("PBA_SCHUR_GRID")) { const int g = atoi(sv); if (g >= 1 && g <= 1024) e->schur_grid = std::min(e->n_tiles, g); }
  return PBA_OK;
}
// the index tables the host built, enqueued (the caller synchronises before L goes out of scope)
static int problem_upload_tables(pba_engine* e, const ProblemLayout& L) {
  HIP_TRY(e, hipMemcpyAsync(e->d_pt_begin, L.pt_begin.data(), sizeof(int32_t) * (e->n_points + 1), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_tile_info, L.tinfo.data(), sizeof(int4) * L.tinfo.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_lane_rec, L.lane_rec.data(), sizeof(int2) * L.lane_rec.size(), hipMemcpyHostToDevice, e->stream));
  return PBA_OK;
}
// after the synchronisation: the slot mask and the host copies of the observation structure (the caller invalidates with kInProblem)
static void problem_installed(pba_engine* e, ProblemLayout* L) {
  e->slot_mask = 0;
  for (int o = 0; o < e->n_obs; ++o) e->slot_mask |= 1u << L->slot8[o];
  e->h_pt_begin = std::move(L->pt_begin);      // (wide_prepare; moved, not copied)
  e->h_obs_slot = std::move(L->slot8);
  e->have_problem = true;
}

int pba_set_problem(pba_engine* e, int32_t n_points, const double* xyz, const double* desc, int32_t n_obs,
                    const int32_t* obs_point, const int32_t* obs_slot, const double* weights) {
  if (!e || n_points <= 0 || n_obs <= 0 || !xyz || !desc || !obs_point || !obs_slot || !weights) return PBA_ERR_INVALID;
  PBA_ENTER(e);
  const int P = (2 * e->cfg.radius + 1) * (2 * e->cfg.radius + 1);     // pixels of one patch (weights)
  const int PD = P * e->channels;                                       // descriptor entries per point
  ProblemLayout L;
  int rc;
  if ((rc = problem_layout(e, n_points, n_obs, obs_point, obs_slot, &L))) return rc;

  std::vector<float> descf((size_t)n_points * PD);
  for (size_t i = 0; i < descf.size(); ++i) descf[i] = (float)desc[i];
  std::vector<double> w2(P);
  e->unit_weights = true;
  for (int i = 0; i < P; ++i) { w2[i] = weights[i] * weights[i]; if (weights[i] != 1.0) e->unit_weights = false; }

  if ((rc = dev_alloc(e, &e->d_w2, (size_t)P))) return rc;
  if ((rc = problem_reserve(e, L, PD))) return rc;

  // the points go to the CURRENT parity: the cameras of an earlier pba_set_cameras live there too, so the two calls may
  // come in either order
  HIP_TRY(e, hipMemcpyAsync(e->d_xyz[e->cur], xyz, sizeof(double) * 3 * n_points, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_desc, descf.data(), sizeof(float) * descf.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_w2, w2.data(), sizeof(double) * P, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_obs_point, obs_point, sizeof(int32_t) * n_obs, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_obs_slot, L.slot8.data(), n_obs, hipMemcpyHostToDevice, e->stream));
  if ((rc = problem_upload_tables(e, L))) return rc;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  problem_installed(e, &L);
  e->inverse_depth = false;         // back to the reference's free world points until pba_set_inverse_depth says otherwise
  e->points_const = false;          // ... and to free points until pba_set_points_constant says otherwise
  e->cams_const = false;            // ... and to free cameras until pba_set_cameras_constant says otherwise
  e->pp_on = false;                 // a point prior belongs to one set of points
  invalidate(e, kInProblem | kInPointPrior);
  return PBA_OK;
}

int pba_set_cameras(pba_engine* e, const double* cams6, int32_t n_frames, int32_t fixed_slot) {
  if (!e || !cams6 || n_frames < 2 || n_frames > e->cfg.max_frames || fixed_slot >= n_frames) return PBA_ERR_INVALID;
  return pba_set_cameras_anchored(e, cams6, n_frames, slot_mask_of_fixed(fixed_slot));
}

int pba_set_cameras_anchored(pba_engine* e, const double* cams6, int32_t n_frames, uint32_t anchor_mask) {
  if (!e || !cams6 || n_frames < 2 || n_frames > e->cfg.max_frames || n_frames > kMaxFramesWide) return PBA_ERR_INVALID;
  if (n_frames < 32 && (anchor_mask >> n_frames))
    return fail(e, PBA_ERR_INVALID, "pba_set_cameras_anchored: anchor_mask 0x%x has bits at or above n_frames = %d", anchor_mask, n_frames);
  const int nf = slot_count_free(anchor_mask, n_frames);
  if (nf == 0 && !e->points_const && !e->cams_const)
    return fail(e, PBA_ERR_INVALID, "pba_set_cameras_anchored: anchor_mask covers all %d slots: no camera is left to solve for; hold every "
                                    "camera constant with pba_set_cameras_constant", n_frames);
  const unsigned present = modes_present(e, e->comm.multi()) & ~(unsigned)kModePrior;      // (the call clears the prior: it is in nothing's way)
  if (const char* why = n_frames - nf >= 2 ? mode_conflict(present, kModeAnchors) : nullptr)
    return fail(e, PBA_ERR_INVALID, "pba_set_cameras_anchored: %d constant slots: %s", n_frames - nf, why);
  PBA_ENTER(e);
  // the window shape picks the path: the narrow kernels stage kMaxFrames-slot camera tables and hold up to kWideMinFree - 1 free
  // cameras; a window with more slots or more free cameras runs the wide chain
  const bool wide = n_frames > kMaxFrames || nf >= kWideMinFree;
  int rc;
  if (wide) {
    const char* why = mode_conflict(present, kModeWide);
    if (why && nf >= kWideMinFree)
      return fail(e, PBA_ERR_INVALID, "pba_set_cameras: %d free cameras: %s (at most %d free cameras there)", nf, why, kWideMinFree - 1);
    if (why) return fail(e, PBA_ERR_INVALID, "pba_set_cameras: %d slots: %s (at most %d slots there)", n_frames, why, kMaxFrames);
    if ((rc = check_lds(e, solve_wide_smem_bytes(6 * nf) + 1024, "", nf, "free cameras", "the reduced solve"))) return rc;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_solve_wide), hipFuncAttributeMaxDynamicSharedMemorySize, (int)solve_wide_smem_bytes(6 * nf));
    (void)hipGetLastError();
  }
  e->n_frames = n_frames;
  e->anchor_mask = anchor_mask;
  e->n_free = nf;
  e->n_pairs = e->n_free * (e->n_free + 1) / 2;
  e->part_stride = 36 * e->n_pairs + 3 * 6 * e->n_free + 3;
  e->wide = wide;
  e->prior_on = false;      // a prior belongs to one set of cameras
  invalidate(e, kInCameras | kInPrior);
  if (e->wide) {
    if ((rc = dev_alloc(e, &e->d_packed, (size_t)packed_stride(6 * e->n_free)))) return rc;
  } else {
    if (e->n_pairs > kTile) return fail(e, PBA_ERR_INVALID, "too many free cameras for the Schur tile (%d pairs)", e->n_pairs);
    // the reduced solve keeps the whole augmented matrix in LDS (dynamic) next to ~21 KB of static LDS: fits the 160 KB of a
    // gfx950 CU at every supported window; a device with less (gfx90a / gfx942: 64 KB) gets a clear error instead of a failed launch
    if ((rc = check_lds(e, solve_blocked_smem_bytes(6 * e->n_free) + 22 * 1024, "", e->n_free, "free cameras", "the reduced solve"))) return rc;
    if ((rc = dev_alloc(e, &e->d_partial, (size_t)(256 * 4) * (((size_t)e->part_stride + 15) / 16 * 16)))) return rc;      // [entry / 16][workgroup][16]
    if ((rc = dev_alloc(e, &e->d_red, (size_t)pba_engine::kChunks * e->part_stride))) return rc;
    if ((rc = dev_alloc(e, &e->d_packed, (size_t)e->part_stride))) return rc;
  }
  if (e->solve_tab_nf != e->n_free) {
    std::vector<uint32_t> tab((size_t)solve_table_words(e->n_free));
    solve_tables(e->n_free, tab.data());
    if ((rc = dev_alloc(e, &e->d_solve_tab, tab.size()))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->d_solve_tab, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));      // (the host vector goes out of scope)
    e->solve_tab_nf = e->n_free;
  }
  HIP_TRY(e, hipMemcpyAsync(e->d_cams[e->cur], cams6, sizeof(double) * 6 * n_frames, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_cam_geom, dim3(1), dim3(64), 0, e->stream, e->d_cams[e->cur], e->d_geom[e->cur], n_frames, e->anchor_mask);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  e->have_cams = true;
  return PBA_OK;
}

static int fetch_state(pba_engine* e, double* cams6, double* xyz) {
  PBA_ENTER(e);
  // through the engine's host-mapped pinned buffer, written by a kernel: the runtime's copy call blocks for 8 ms the
  // first time a process moves a few hundred KB device -> host (seen in the drop-in class, pinned or pageable
  // destination alike); a kernel that stores over PCIe plus a host copy is ~50 us every time
  const size_t nc = (size_t)6 * e->n_frames, nx = (size_t)3 * e->n_points;
  { const int rc = host_alloc(e, &e->h_state_stage, nc + nx, &e->h_state_dev); if (rc) return rc; }
  if (cams6) k_to_host<<<dim3(1), dim3(256), 0, e->stream>>>(e->d_cams[e->cur], e->h_state_dev, nc);
  if (xyz) k_to_host<<<dim3((unsigned)std::min<size_t>((nx + 1023) / 1024, 256)), dim3(256), 0, e->stream>>>(e->d_xyz[e->cur], e->h_state_dev + nc, nx);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (cams6) std::memcpy(cams6, e->h_state_stage, sizeof(double) * nc);
  if (xyz) std::memcpy(xyz, e->h_state_stage + nc, sizeof(double) * nx);
  return PBA_OK;
}

int pba_get_state(pba_engine* e, double* cams6, double* xyz) {
  if (!e) return PBA_ERR_INVALID;
  if (e->poisoned) return fail(e, PBA_ERR_STATE, "pba_get_state: the engine is unusable after a timed-out step; destroy it");
  if (!e->have_problem || !e->have_cams) return fail(e, PBA_ERR_STATE, "call order violated: pba_get_state before set_problem/set_cameras");
  return fetch_state(e, cams6, xyz);
}

int pba_set_inverse_depth(pba_engine* e, const double* rays6, const double* rho) {
  if (!e || !rays6 || !rho) return PBA_ERR_INVALID;
  if (!e->have_problem) return fail(e, PBA_ERR_STATE, "call order violated: pba_set_inverse_depth before pba_set_problem");
  if (const char* why = mode_conflict(modes_present(e, e->comm.multi()), kModeInverseDepth))
    return fail(e, PBA_ERR_INVALID, "pba_set_inverse_depth: %s (%d free cameras)", why, e->n_free);
  PBA_ENTER(e);
  const int n = e->n_points;
  std::vector<double> prm((size_t)3 * n, 0.0);
  for (int i = 0; i < n; ++i) {
    if (!(rho[i] > 0.0) || !std::isfinite(rho[i])) return fail(e, PBA_ERR_INVALID, "inverse depth of point %d is not positive", i);
    prm[3 * (size_t)i] = rho[i];
  }
  int rc = dev_alloc(e, &e->d_rays, (size_t)6 * n);
  if (rc) return rc;
  e->h_rays.assign(rays6, rays6 + (size_t)6 * n);
  HIP_TRY(e, hipMemcpyAsync(e->d_rays, rays6, sizeof(double) * 6 * n, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_xyz[e->cur], prm.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  e->inverse_depth = true;
  invalidate(e, kInPointParams);
  return PBA_OK;
}

// pba_set_points_constant / pba_set_cameras_constant: `mine` is the mode's own switch, `other` the other mode's
static int set_constant_mode(pba_engine* e, int32_t on, const char* who, unsigned feature, bool* mine, bool other, unsigned input) {
  if (!e->have_problem) return fail(e, PBA_ERR_STATE, "call order violated: %s before pba_set_problem", who);
  PBA_NOT_POISONED(e);
  if (const char* why = on ? mode_conflict(modes_present(e, e->comm.multi()), feature) : nullptr) return fail(e, PBA_ERR_INVALID, "%s: %s", who, why);
  if (!on && e->have_cams && e->n_free == 0 && *mine && !other)
    return fail(e, PBA_ERR_INVALID, "%s(0): the anchor mask covers all %d slots (pba_set_cameras_anchored): no camera is left to solve "
                                    "for; set other cameras first, or hold every camera constant with pba_set_cameras_constant", who, e->n_frames);
  *mine = on != 0;
  invalidate(e, input);
  return PBA_OK;
}
int pba_set_points_constant(pba_engine* e, int32_t on) {
  return !e ? PBA_ERR_INVALID : set_constant_mode(e, on, "pba_set_points_constant", kModePointsConst, &e->points_const, e->cams_const, kInPointsConst);
}
int pba_set_cameras_constant(pba_engine* e, int32_t on) {
  return !e ? PBA_ERR_INVALID : set_constant_mode(e, on, "pba_set_cameras_constant", kModeCamsConst, &e->cams_const, e->points_const, kInCamsConst);
}

// The constant blocks live in BOTH parities (the candidate pass reads the candidate parity, pba_accept flips it): device-to-device copies
// of the current points, or cameras and geometry, byte for byte, once per problem.
static int sync_constant_blocks(pba_engine* e) {
  if (e->points_const && !e->pose_xyz_synced) {
    HIP_TRY(e, hipMemcpyAsync(e->d_xyz[1 - e->cur], e->d_xyz[e->cur], sizeof(double) * 3 * e->n_points, hipMemcpyDeviceToDevice, e->stream));
    e->pose_xyz_synced = true;
  }
  if (e->cams_const && !e->pts_cams_synced) {
    HIP_TRY(e, hipMemcpyAsync(e->d_cams[1 - e->cur], e->d_cams[e->cur], sizeof(double) * 6 * e->n_frames, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->d_geom[1 - e->cur], e->d_geom[e->cur], sizeof(CamGeom) * e->n_frames, hipMemcpyDeviceToDevice, e->stream));
    e->pts_cams_synced = true;
  }
  return PBA_OK;
}

int pba_get_points_world(pba_engine* e, double* xyz) {
  if (!e || !xyz) return PBA_ERR_INVALID;
  if (!e->have_problem) return fail(e, PBA_ERR_STATE, "call order violated: pba_get_points_world before pba_set_problem");
  PBA_ENTER(e);
  { const int rc = fetch_state(e, nullptr, xyz); if (rc) return rc; }
  if (e->inverse_depth) {
    for (int i = 0; i < e->n_points; ++i) {
      const double inv = 1.0 / xyz[3 * (size_t)i];
      const double* r = e->h_rays.data() + 6 * (size_t)i;
      for (int k = 0; k < 3; ++k) xyz[3 * (size_t)i + k] = r[k] + r[3 + k] * inv;
    }
  }
  return PBA_OK;
}

// E of the camera prior at the current cameras (k_prior); the gradient over the prior's rows stays in d_prior_out
static int prior_energy(pba_engine* e, double* E) {
  PriorParams pp = prior_params(e, e->d_cams[e->cur]);
  pp.out = e->d_prior_out;
  launch_prior(e, pp);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(E, e->d_prior_out + 6 * e->prior_k, sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_linearize(pba_engine* e, double* cost) {
  if (!e) return PBA_ERR_INVALID;
  { const int rc0 = check_ready(e, "pba_linearize"); if (rc0) return rc0; }
  PBA_ENTER(e);
  { const int rcp = sync_constant_blocks(e); if (rcp) return rcp; }
  if (!e->lin_valid[e->cur]) {      // (whatever dropped it dropped the sums reduced from it: drop_lin)
    SampleParams sp = make_sample_params(e, e->cur);
    ev_begin(e, 0);
    launch_sample<true>(e, sp);
    ev_end(e, 0);
    HIP_TRY(e, hipGetLastError());
    e->cost_blocks[e->cur] = e->sample_grid;
    e->lin_valid[e->cur] = true;
    e->jac_passes++;
  }
  e->have_lin = true;
  if (cost) {
    std::vector<double> bc(e->cost_blocks[e->cur]);
    HIP_TRY(e, hipMemcpyAsync(bc.data(), e->d_block_cost[e->cur], sizeof(double) * bc.size(), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    ev_collect(e);
    double c = 0.0;
    for (double v : bc) c += v;
    if (e->comm.multi()) {
      if (e->comm.allreduce_host(&c, 1, 0)) return fail(e, PBA_ERR_COMM, "allreduce(cost) failed: %s", e->comm.err.c_str());
    }
    if (e->prior_on) {      // E at the current cameras, added last
      double E = 0.0;
      const int rcp = prior_energy(e, &E);
      if (rcp) return rcp;
      c += E;
    }
    if (e->pp_on) {      // E_pts at the current points, added last
      double E = 0.0;
      launch_point_prior_cost(e, e->d_xyz[e->cur], nullptr, e->d_pp_E);
      HIP_TRY(e, hipGetLastError());
      HIP_TRY(e, hipMemcpyAsync(&E, e->d_pp_E, sizeof(double), hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
      c += E;
    }
    *cost = c;
  }
  return PBA_OK;
}

// Spins on the host-mapped sequence number until step `seq` is published.  exact: a synchronous step -- the number must become `seq`
// itself; else a pipelined wait -- any number from `seq` on will do, and a terminated solve (whose remaining kernels are no-ops) may
// drain the stream without ever publishing it.
static int wait_published(pba_engine* e, unsigned long long seq, bool exact) {
  volatile unsigned long long* h_seq = reinterpret_cast<volatile unsigned long long*>(e->h_scal + kNumScal);
  const auto pending = [&] { return exact ? *h_seq != seq : *h_seq < seq; };
  unsigned long spins = 0;
  double t_first = -1.0;
  { const int rcc = comm_failed(e); if (rcc) return rcc; }
  while (pending()) {
    { const int rcc = comm_failed(e); if (rcc) return rcc; }
    // hipStreamQuery is not free for the device (it showed up as a ~6 us bubble in front of the next kernel), so it only
    // serves as a watchdog here: roughly every 50 ms of spinning
    if ((++spins & 0x3ffffff) == 0) {
      const hipError_t q = hipStreamQuery(e->stream);
      if (q != hipSuccess && q != hipErrorNotReady) return fail(e, PBA_ERR_HIP, "stream error while waiting: %s", hipGetErrorString(q));
      if (q == hipSuccess && pending()) {
        if (exact) return fail(e, PBA_ERR_HIP, "step finished without publishing its scalars");
        if (reinterpret_cast<volatile LmState*>(e->h_lm)->done) return PBA_OK;
        return fail(e, PBA_ERR_HIP, "step finished without publishing");
      }
      // a collective that never completes (a peer died, or the ranks disagree on the number of enqueued steps) would
      // otherwise spin forever: bounded by PBA_WAIT_TIMEOUT_S (default 120 s) of wall-clock per awaited step
      const double t = wall_seconds();
      if (t_first < 0.0) t_first = t;
      else if (t - t_first > e->wait_timeout_s) {
        e->poisoned = true;
        const int code = e->comm.multi() ? PBA_ERR_COMM : PBA_ERR_HIP;
        if (exact) return fail(e, code, "timed out after %.0f s waiting for step %llu", e->wait_timeout_s, seq);
        return fail(e, code, "timed out after %.0f s waiting for step %llu (last published %llu)", e->wait_timeout_s, seq,
                    (unsigned long long)*h_seq);
      }
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  // the sequence number may already have been there when the wait was entered (normal with the pipelined driver): the error word is
  // checked on the way out too
  return comm_failed(e);
}

// Waits for the device to publish the scalar block of step `seq` and unpacks it (the end of every pba_step); scal != nullptr also
// gets the raw block (kNumScal doubles, what lm_decide reads).  PBA_ERR_NUMERIC comes with both outputs filled.
static int wait_step_scalars(pba_engine* e, unsigned long long seq, pba_step_info* out, double* scal) {
  { const int rcw = wait_published(e, seq, true); if (rcw) return rcw; }
  if (e->profile) { HIP_TRY(e, hipStreamSynchronize(e->stream)); ev_collect(e); }
  double s[kNumScal];
  for (int k = 0; k < kNumScal; ++k) s[k] = reinterpret_cast<volatile double*>(e->h_scal)[k];
  out->cost = s[kCostLin];
  out->gradient_max_norm = std::max(s[kGmaxPts], s[kGmaxCams]);
  out->gradient_norm = std::sqrt(s[kGnorm2Pts] + s[kGnorm2Cams]);
  out->model_cost_change = s[kMccPts] + s[kMccCams];
  out->step_norm = std::sqrt(s[kStep2Pts] + s[kStep2Cams]);
  out->x_norm = std::sqrt(s[kX2Pts] + s[kX2Cams]);
  out->candidate_cost = s[kCandCost];
  out->linear_solver_ok = (s[kSolveOk] > 0.5 && s[kSchurFail] < 0.5) ? 1 : 0;
  out->eval_ok = (s[kEvalFailCand] < 0.5 && std::isfinite(s[kCandCost])) ? 1 : 0;
  if (scal) std::memcpy(scal, s, sizeof(s));
  if (s[kEvalFailLin] > 0.5) return fail(e, PBA_ERR_NUMERIC, "non-finite residual block at the linearisation point");
  return PBA_OK;
}

// The candidate pass of a host-stepped step: a Jacobian pass when speculating on acceptance (the candidate is then already linearised
// when pba_accept makes it the current point), else a cost pass.  fused: the kernel that also back-substitutes and finalises the step.
static void candidate_pass(pba_engine* e, const SampleParams& sp, int cand, bool fused) {
  const int k = e->speculate ? 0 : 1;
  ev_begin(e, k);
  if (fused) { if (e->speculate) launch_sample<true, true>(e, sp); else launch_sample<false, true>(e, sp); }
  else { if (e->speculate) launch_sample<true>(e, sp); else launch_sample<false>(e, sp); }
  ev_end(e, k);
  ++(e->speculate ? e->jac_passes : e->cost_passes);
  e->cost_blocks[cand] = fused ? e->fused_grid : e->sample_grid;
  drop_lin(e, cand); e->lin_valid[cand] = e->speculate;      // rec[cand] is overwritten: with a Jacobian pass when speculating
}

// pba_step of the pose-only mode (pba_pose.h): per-camera sums of the stored linearisation (once per linearisation), the block-diagonal
// damped solve, the candidate pass at the candidate cameras with the unchanged points, the candidate cost.
static int pose_step(pba_engine* e, double radius, int32_t init_scale, const pba_solver_options* o, pba_step_info* out, double* scal,
                     int grad_only) {
  const int cur = e->cur, cand = 1 - e->cur;
  int rc;
  if ((rc = sync_constant_blocks(e))) return rc;
  if ((rc = dev_alloc(e, &e->d_pose_partial, (size_t)kPoseMaxGrid * kMaxFramesWide * kPoseVals))) return rc;
  if ((rc = dev_alloc(e, &e->d_pose_sums, (size_t)kMaxFramesWide * kPoseVals + 2))) return rc;
  const bool reduce = e->pose_sums_cur != cur;
  if (reduce) {
    PoseSystemParams ps{};
    ps.xyz = e->d_xyz[cur]; ps.rays = rays_or_null(e); ps.geom = e->d_geom[cur]; ps.rec = e->d_rec[cur];
    ps.obs_point = e->d_obs_point; ps.obs_slot = e->d_obs_slot; ps.partial = e->d_pose_partial; ps.rec_stride = e->rec_stride;
    ps.n_obs = e->n_obs; ps.n_frames = e->n_frames; ps.fx = e->cfg.fx; ps.fy = e->cfg.fy;
    e->pose_grid = std::max(1, std::min(kPoseMaxGrid, (e->n_obs + kPoseThreads - 1) / kPoseThreads));
    ev_begin(e, 2);
    hipLaunchKernelGGL(k_pose_system, dim3(e->pose_grid), dim3(kPoseThreads), 0, e->stream, ps);
    ev_end(e, 2);
    HIP_TRY(e, hipGetLastError());
  }
  PoseSolveParams so{};
  so.partial = e->d_pose_partial; so.sums = e->d_pose_sums; so.block_cost = e->d_block_cost[cur]; so.block_fail = e->d_block_fail[cur];
  so.cams = e->d_cams[cur]; so.cams_cand = e->d_cams[cand]; so.delta_c = e->d_delta_c; so.sc = e->d_sc;
  so.S_dbg = keep_system(e) ? e->d_S : nullptr; so.rhs_dbg = e->d_rhs; so.scal = e->d_scal;
  so.geom = e->d_geom[cur]; so.geom_cand = e->d_geom[cand];
  so.n_parts = e->pose_grid; so.n_cost_blocks = e->cost_blocks[cur]; so.reduce = reduce ? 1 : 0;
  so.n_frames = e->n_frames; so.n_free = e->n_free; so.anchor_mask = e->anchor_mask; so.init_scale = init_scale; so.jacobi = o->jacobi_scaling;
  so.grad_only = grad_only; so.radius = radius; so.min_diag = o->min_lm_diagonal; so.max_diag = o->max_lm_diagonal;
  ev_begin(e, 3);
  hipLaunchKernelGGL(k_pose_solve, dim3(1), dim3(kPoseThreads), 0, e->stream, so);
  ev_end(e, 3);
  HIP_TRY(e, hipGetLastError());
  e->pose_sums_cur = cur;
  const unsigned long long seq = ++e->seq;
  unsigned long long* const h_seq_dev = host_seq_dev(e);
  if (!grad_only) {
    // candidate point: Jacobian pass when speculating on acceptance, else cost pass; the points are the current ones
    SampleParams sp = make_sample_params(e, cand);
    candidate_pass(e, sp, cand, false);
    hipLaunchKernelGGL(k_pose_finalize, dim3(1), dim3(kPoseThreads), 0, e->stream, (const double*)e->d_block_cost[cand],
                       (const int32_t*)e->d_block_fail[cand], e->sample_grid, e->d_scal, e->h_scal_dev, h_seq_dev, seq);
  } else {
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, e->stream, e->d_scal, e->h_scal_dev, h_seq_dev, seq, (const double*)nullptr, 1);
  }
  HIP_TRY(e, hipGetLastError());
  return wait_step_scalars(e, seq, out, scal);
}

// pba_step of the structure-only mode (pba_points.h): per-point blocks of the stored linearisation (once per linearisation), the
// block-diagonal damped solve into the candidate points, the candidate pass there with the unchanged cameras, the scalar block.
static int points_step(pba_engine* e, double radius, int32_t init_scale, const pba_solver_options* o, pba_step_info* out, double* scal,
                       int grad_only) {
  const int cur = e->cur, cand = 1 - e->cur;
  const int grid = (e->n_points + kPointsThreads - 1) / kPointsThreads;
  const bool dbg = keep_system(e);
  int rc;
  if ((rc = sync_constant_blocks(e))) return rc;
  if ((rc = dev_alloc(e, &e->d_pts_sys, (size_t)kPointsSys * e->n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_pts_part, (size_t)grid * kPointsWaves * kPointsRow))) return rc;
  if (dbg) {
    if ((rc = dev_alloc(e, &e->d_pts_V, (size_t)9 * e->n_points))) return rc;
    if ((rc = dev_alloc(e, &e->d_pts_rhs, (size_t)3 * e->n_points))) return rc;
  }
  if (e->pts_sys_cur != cur) {
    PointsSystemParams ps{};
    ps.xyz = e->d_xyz[cur]; ps.rays = rays_or_null(e); ps.geom = e->d_geom[cur]; ps.rec = e->d_rec[cur];
    ps.pt_begin = e->d_pt_begin; ps.obs_slot = e->d_obs_slot; ps.sys = e->d_pts_sys; ps.rec_stride = e->rec_stride;
    ps.n_points = e->n_points; ps.n_frames = e->n_frames; ps.fx = e->cfg.fx; ps.fy = e->cfg.fy;
    ps.prior_x0 = e->d_pp_x0; ps.prior_L6 = e->d_pp_L6;
    ev_begin(e, 2);
    if (e->pp_on) hipLaunchKernelGGL(k_points_system<true>, dim3(grid), dim3(kPointsThreads), 0, e->stream, ps);
    else hipLaunchKernelGGL(k_points_system<false>, dim3(grid), dim3(kPointsThreads), 0, e->stream, ps);
    ev_end(e, 2);
    HIP_TRY(e, hipGetLastError());
    e->pts_sys_cur = cur;
  }
  PointsSolveParams so{};
  so.sys = e->d_pts_sys; so.xyz = e->d_xyz[cur]; so.xyz_cand = e->d_xyz[cand]; so.sp = e->d_sp; so.part = e->d_pts_part;
  so.V_dbg = dbg ? e->d_pts_V : nullptr; so.rhs_dbg = dbg ? e->d_pts_rhs : nullptr;
  so.n_points = e->n_points; so.dim = e->inverse_depth ? 1 : 3; so.init_scale = init_scale; so.jacobi = o->jacobi_scaling;
  so.grad_only = grad_only; so.radius = radius; so.min_diag = o->min_lm_diagonal; so.max_diag = o->max_lm_diagonal;
  ev_begin(e, 3);
  hipLaunchKernelGGL(k_points_solve, dim3(grid), dim3(kPointsThreads), 0, e->stream, so);
  ev_end(e, 3);
  HIP_TRY(e, hipGetLastError());
  if (dbg && !(grad_only && !init_scale)) e->pts_dbg_valid = true;
  const unsigned long long seq = ++e->seq;
  PointsFinalizeParams fp{};
  fp.part = e->d_pts_part; fp.n_rows = grid * kPointsWaves; fp.cost_lin = e->d_block_cost[cur]; fp.fail_lin = e->d_block_fail[cur];
  fp.n_lin = e->cost_blocks[cur]; fp.scal = e->d_scal; fp.host_scal = e->h_scal_dev; fp.host_seq = host_seq_dev(e); fp.seq = seq;
  if (!grad_only) {
    // candidate point: Jacobian pass when speculating on acceptance, else cost pass; the cameras are the current ones
    SampleParams sp = make_sample_params(e, cand);
    candidate_pass(e, sp, cand, false);
    fp.cost_cand = e->d_block_cost[cand]; fp.fail_cand = e->d_block_fail[cand]; fp.n_cand = e->sample_grid;
  }
  if (e->pp_on) {
    // the point prior joins both costs, last, after the photometric sums; the block is published behind them
    hipLaunchKernelGGL(k_points_finalize<true>, dim3(1), dim3(kPointsThreads), 0, e->stream, fp);
    launch_point_prior_cost(e, e->d_xyz[cur], e->d_scal + kCostLin, nullptr);
    if (!grad_only) launch_point_prior_cost(e, e->d_xyz[cand], e->d_scal + kCandCost, nullptr);
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, e->stream, e->d_scal, e->h_scal_dev, fp.host_seq, seq, (const double*)nullptr, 1);
  } else {
    hipLaunchKernelGGL(k_points_finalize<false>, dim3(1), dim3(kPointsThreads), 0, e->stream, fp);
  }
  HIP_TRY(e, hipGetLastError());
  rc = wait_step_scalars(e, seq, out, scal);
  if ((rc == PBA_OK || rc == PBA_ERR_NUMERIC) && !grad_only && !out->linear_solver_ok) {
    // a failed block makes the whole step a zero step: the candidate points are the current ones again
    HIP_TRY(e, hipMemcpyAsync(e->d_xyz[cand], e->d_xyz[cur], sizeof(double) * 3 * e->n_points, hipMemcpyDeviceToDevice, e->stream));
    drop_lin(e, cand);
  }
  return rc;
}

int pba_step(pba_engine* e, double radius, int32_t init_scale, const pba_solver_options* o, pba_step_info* out) {
  return pba_internal_step(e, radius, init_scale, o, out, nullptr, 0);
}

// grad_only != 0: stop after the reduced solve (cost / gradient norms of the linearisation point only).  scal: nullptr, or kNumScal
// doubles for the step's raw scalar block.
int pba_internal_step(pba_engine* e, double radius, int32_t init_scale, const pba_solver_options* o, pba_step_info* out, double* scal,
                      int grad_only) {
  if (!e || !o || !out || !(radius > 0.0)) return PBA_ERR_INVALID;
  e->last_driver = 3;
  if (!e->have_lin) return fail(e, PBA_ERR_STATE, "call order violated: pba_step before pba_linearize");
  PBA_ENTER(e);
  if (e->points_const) return pose_step(e, radius, init_scale, o, out, scal, grad_only);
  if (e->cams_const) return points_step(e, radius, init_scale, o, out, scal, grad_only);
  const int cur = e->cur, cand = 1 - e->cur;
  const int n = 6 * e->n_free;
  const bool multi = e->comm.multi();

  SchurParams sc = schur_params(e, cur, init_scale, o, radius);
  if (e->dbg_left > 0 && !eliminates_wide(e)) {
    { const int rcd = dev_alloc(e, &e->d_dbg, pba_engine::kDbgWords); if (rcd) return rcd; }
    sc.dbg = e->d_dbg;
  }
  if (eliminates_wide(e)) {
    const int rcw = wide_eliminate(e, cur, init_scale, o, radius);
    if (rcw) return rcw;
  } else {
    ev_begin(e, 2);
    launch_schur(e, sc);
    ev_end(e, 2);
  }
  if (sc.dbg) { dump_schur_phase_cycles(e); --e->dbg_left; }
  SolveParams so = solve_params(e, cur, init_scale, o, radius, !grad_only && fused_capable(e));
  so.dbg = (e->dbg_left > 0) ? 1 : 0;
  if (eliminates_wide(e)) {
    ev_begin(e, 3);
    hipLaunchKernelGGL(k_solve_wide, dim3(1), dim3(kSolveWideT), solve_wide_smem_bytes(n), e->stream, so);
    ev_end(e, 3);
    HIP_TRY(e, hipGetLastError());
  } else {
    const int rcs = launch_reduce_and_solve(e, so, n, cur, cand, nullptr, 0, e->cost_blocks[cur]);
    if (rcs) return rcs;
  }
  const unsigned long long seq = ++e->seq;
  unsigned long long* const h_seq_dev = host_seq_dev(e);
  bool xchg_packed = false;
  if (!grad_only && fused_capable(e)) {
    // one kernel: back-substitution -> candidate pass (Jacobian pass when speculating) -> step finalisation
    SampleParams sp = make_sample_params(e, cand);
    sp.tile_info = e->d_tile_info; sp.lane_rec = e->d_lane_rec; sp.geom_prev = e->d_geom[cur];
    sp.xyz_prev = e->d_xyz[cur]; sp.rec_prev = e->d_rec[cur]; sp.sp = e->d_sp; sp.ptrec = e->d_ptrec;
    sp.delta_c = e->d_delta_c; sp.block_bs = e->d_bs_out; sp.ticket = e->d_ticket; sp.scal = e->d_scal;
    sp.host_scal = (multi || e->prior_on) ? nullptr : e->h_scal_dev; sp.host_seq = h_seq_dev; sp.seq = seq; sp.n_tiles = e->n_tiles;
    sp.dbg = (e->dbg_left > 0 && e->d_dbg) ? e->d_dbg + 8 * 1024 : nullptr;
    if (multi) {
      const int rcx = set_sample_exchange(e, sp);
      if (rcx) return rcx;
      xchg_packed = true;
    }
    candidate_pass(e, sp, cand, true);
    if (sp.dbg) dump_fused_sample_timeline(e, sp.dbg);
  } else if (!grad_only) {
    BacksubParams bs{};
    bs.xyz = e->d_xyz[cur]; bs.rays = rays_or_null(e); bs.xyz_cand = e->d_xyz[cand]; bs.geom = e->d_geom[cur]; bs.rec = e->d_rec[cur];
    bs.pt_begin = e->d_pt_begin; bs.obs_slot = e->d_obs_slot; bs.sp = e->d_sp; bs.ptrec = e->d_ptrec;
    bs.delta_c = e->d_delta_c; bs.block_out = e->d_bs_out; bs.rec_stride = e->rec_stride; bs.n_points = e->n_points;
    bs.fx = e->cfg.fx; bs.fy = e->cfg.fy;
    bs.cams_cand = e->d_cams[cand]; bs.geom_cand = e->d_geom[cand]; bs.n_frames = e->n_frames; bs.anchor_mask = e->anchor_mask;
    hipLaunchKernelGGL(k_backsub, dim3(e->backsub_grid), dim3(256), 0, e->stream, bs);
    // candidate point: Jacobian pass when speculating on acceptance, else cost pass
    SampleParams sp = make_sample_params(e, cand);
    candidate_pass(e, sp, cand, false);
    hipLaunchKernelGGL(k_finalize_step, dim3(1), dim3(256), 0, e->stream, e->d_bs_out, e->backsub_grid, e->d_block_cost[cand],
                       e->d_block_fail[cand], e->sample_grid, e->d_scal, (multi || e->prior_on || e->pp_on) ? nullptr : e->h_scal_dev, h_seq_dev, seq);
  }
  if (e->prior_on && !grad_only) {
    // the prior at the candidate cameras joins the candidate cost, last, after the photometric sum; the block is published below
    PriorParams pp = prior_params(e, e->d_cams[cand]);
    pp.add_to = e->d_scal + kCandCost;
    launch_prior(e, pp);
  }
  // the point prior at the candidate points, likewise (k_backsub wrote them; single rank: pba_set_point_prior refuses the transports)
  if (e->pp_on && !grad_only) launch_point_prior_cost(e, e->d_xyz[cand], e->d_scal + kCandCost, nullptr);
  HIP_TRY(e, hipGetLastError());
  if (multi) {
    int rc2 = exchange_step_scalars(e, xchg_packed);
    if (rc2) return rc2;
  }
  if (multi || grad_only || e->prior_on || e->pp_on) {
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, e->stream, e->d_scal, e->h_scal_dev, h_seq_dev, seq,
                       (const double*)(multi ? e->d_xchg : nullptr), e->comm.world);
    HIP_TRY(e, hipGetLastError());
  }
  return wait_step_scalars(e, seq, out, scal);
}

int pba_accept(pba_engine* e) {
  if (!e) return PBA_ERR_INVALID;
  if (!e->have_lin) return fail(e, PBA_ERR_STATE, "call order violated: pba_accept before pba_step");
  drop_lin(e, e->cur);      // (the sums were reduced from this parity: pose_step / points_step)
  e->cur = 1 - e->cur;
  e->have_lin = e->lin_valid[e->cur];
  return PBA_OK;
}

int pba_get_point_system(pba_engine* e, double* V9, double* rhs3) {
  if (!e) return PBA_ERR_INVALID;
  if (!keep_system(e)) return fail(e, PBA_ERR_STATE, "call order violated: pba_get_point_system needs pba_config.flags bit 0 (keep reduced system)");
  if (!e->cams_const || !e->pts_dbg_valid)
    return fail(e, PBA_ERR_STATE, "call order violated: pba_get_point_system needs a pba_step in the cameras-constant mode (pba_set_cameras_constant)");
  PBA_ENTER(e);
  if (V9) HIP_TRY(e, hipMemcpyAsync(V9, e->d_pts_V, sizeof(double) * 9 * e->n_points, hipMemcpyDeviceToHost, e->stream));
  if (rhs3) HIP_TRY(e, hipMemcpyAsync(rhs3, e->d_pts_rhs, sizeof(double) * 3 * e->n_points, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_get_reduced_system(pba_engine* e, double* S, double* rhs, int32_t* n_out) {
  if (!e || !n_out) return PBA_ERR_INVALID;
  if (!keep_system(e)) return fail(e, PBA_ERR_STATE, "call order violated: pba_get_reduced_system needs pba_config.flags bit 0 (keep reduced system)");
  if (e->cams_const) return fail(e, PBA_ERR_STATE, "pba_get_reduced_system: the cameras-constant mode (pba_set_cameras_constant) has no reduced camera system; see pba_get_point_system");
  PBA_ENTER(e);
  const int n = 6 * e->n_free;
  *n_out = n;
  if (S) HIP_TRY(e, hipMemcpyAsync(S, e->d_S, sizeof(double) * n * n, hipMemcpyDeviceToHost, e->stream));
  if (rhs) HIP_TRY(e, hipMemcpyAsync(rhs, e->d_rhs, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

// Covariance output (pba_cov.h).  Every refusal comes before the first launch; the Jacobian pass is pba_linearize's; the kernels write
// buffers of the off-loop calls only, and the host copies the results out once every pivot is known to be positive.
int pba_covariance(pba_engine* e, double* cam_cov, double* point_cov, pba_covariance_info* info) {
  if (!e) return PBA_ERR_INVALID;
  pba_covariance_info inf{};
  inf.min_cam_pivot = 1.0; inf.min_point_pivot = 1.0; inf.failed_index = -1;
  if (info) *info = inf;
  const bool pose = e->points_const, structure = e->cams_const;
  const unsigned present = modes_present(e, e->comm.multi()) & ~((pose || structure) ? (unsigned)kModeInverseDepth : 0u);      // (free cameras only)
  if (const char* why = mode_conflict(present, kModeCovariance)) return fail(e, PBA_ERR_INVALID, "pba_covariance: %s", why);
  if (pose && point_cov)
    return fail(e, PBA_ERR_INVALID, "pba_covariance: the points are constant (pba_set_points_constant): point_cov must be NULL");
  if (structure && cam_cov)
    return fail(e, PBA_ERR_INVALID, "pba_covariance: the cameras are constant (pba_set_cameras_constant): cam_cov must be NULL");
  { const int rc0 = check_ready(e, "pba_covariance"); if (rc0) return rc0; }
  // the program's camera columns in ascending slot order
  ElimPairParams cs{};
  CovPointsParams cp{};
  int n_cols = 0;
  uint32_t cost_mask = 0xffffffffu;
  for (int s = 0; s < kMaxFramesWide; ++s) cp.col_of_slot[s] = -1;
  if (!structure) {
    if (pose) cost_mask = 0;
    for (int s = 0; s < e->n_frames; ++s) {
      if (!slot_is_free(e->anchor_mask, s)) continue;
      if (pose) cost_mask |= 1u << s;
      if (!((e->slot_mask >> s) & 1u)) {
        if (pose) continue;      // (Ceres: a parameter block without a residual block is not in the program)
        return fail(e, PBA_ERR_INVALID, "pba_covariance: free camera slot %d has no residual block: its block of the normal matrix is zero; "
                                        "hold it constant (pba_set_cameras_anchored)", s);
      }
      cp.col_of_slot[s] = (int8_t)n_cols;
      cs.slot_of_col[n_cols++] = (uint8_t)s;
    }
    if (n_cols == 0) return fail(e, PBA_ERR_INVALID, "pba_covariance: no free camera has a residual block");
  }
  const int n = 6 * n_cols;
  const int dim = e->inverse_depth ? 1 : 3;
  const int pt_blocks = (e->n_points + kElimThreads - 1) / kElimThreads;
  PBA_ENTER(e);
  int rc;
  if (n > 0 && (rc = check_lds(e, cov_invert_smem_bytes(n) + 64, "pba_covariance: ", n_cols, "camera columns", "the inverse"))) return rc;
  if ((rc = pba_linearize(e, nullptr))) return rc;
  if ((rc = dev_alloc(e, &e->d_elim_part, (size_t)kCovPart * pt_blocks))) return rc;
  if (!pose) {
    if ((rc = dev_alloc(e, &e->d_cov_P, (size_t)6 * e->n_points))) return rc;
    if ((rc = dev_alloc(e, &e->d_elim_X, (size_t)6 * e->n_points))) return rc;
    if ((rc = dev_alloc(e, &e->d_cov_pp, (size_t)9 * e->n_points))) return rc;
  }
  if (n > 0) {
    if ((rc = dev_alloc(e, &e->d_elim_S, (size_t)n * n))) return rc;
    if ((rc = dev_alloc(e, &e->d_cov_C, (size_t)n * n))) return rc;
    if ((rc = dev_alloc(e, &e->d_elim_info, (size_t)3))) return rc;
  }
  const double* rays = rays_or_null(e);
  CovPointParams pp{};
  elim_inputs(e, pp);
  pp.rays = rays; pp.P = pose ? nullptr : e->d_cov_P; pp.X = pose ? nullptr : e->d_elim_X; pp.pp = structure ? e->d_cov_pp : nullptr; pp.part = e->d_elim_part;
  pp.n_frames = e->n_frames; pp.dim = dim; pp.cost_mask = cost_mask;
  pp.prior_x0 = e->d_pp_x0; pp.prior_L6 = e->d_pp_L6;
  // event profiling: read back at the end of the call (pba_internal_covariance_times)
  KernelTimes<4>& times = e->cov_times;
  if ((rc = times.start(e, e->profile))) return rc;
  times.begin(e, 0);
  // (the point prior's Lambda_i joins V_i; pba_set_point_prior refuses the points-constant and the inverse-depth mode)
  if (e->pp_on) hipLaunchKernelGGL(k_cov_point<true>, dim3(pt_blocks), dim3(kElimThreads), 0, e->stream, pp);
  else hipLaunchKernelGGL(k_cov_point<false>, dim3(pt_blocks), dim3(kElimThreads), 0, e->stream, pp);
  times.end(e, 0);
  if (n > 0) {
    elim_inputs(e, cs);
    cs.rays = rays; cs.X = pose ? nullptr : e->d_elim_X; cs.S = e->d_elim_S; cs.n_cols = n_cols;
    // pose-only mode: S = blockdiag(U_a), the zero blocks by a memset and one workgroup per diagonal block
    cs.diag_only = pose ? 1 : 0;
    times.begin(e, 1);
    if (pose) HIP_TRY(e, hipMemsetAsync(e->d_elim_S, 0, sizeof(double) * n * n, e->stream));
    hipLaunchKernelGGL(k_elim_pair<false>, dim3(pose ? n_cols : n_cols * (n_cols + 1) / 2), dim3(kElimThreads), 0, e->stream, cs);
    times.end(e, 1);
    CovInvertParams ci{};
    ci.S = e->d_elim_S; ci.C = e->d_cov_C; ci.info = e->d_elim_info; ci.n = n;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cov_invert), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cov_invert_smem_bytes(n));
    (void)hipGetLastError();
    times.begin(e, 2);
    hipLaunchKernelGGL(k_cov_invert, dim3(1), dim3(kCovInvertT), cov_invert_smem_bytes(n), e->stream, ci);
    times.end(e, 2);
  }
  // the first pass decides: nothing is launched on the inverse of a singular matrix, nothing is copied out
  double cinfo[2] = {1.0, -1.0};
  HIP_TRY(e, hipGetLastError());
  if (n > 0) HIP_TRY(e, hipMemcpyAsync(cinfo, e->d_elim_info, sizeof(cinfo), hipMemcpyDeviceToHost, e->stream));
  PointPartials pts;
  if ((rc = read_point_partials(e, pt_blocks, 1, &pts))) return rc;
  inf.min_point_pivot = pts.min_pivot;
  inf.n_cam = n;
  inf.point_dim = pose ? 0 : dim;
  inf.num_residuals = (int32_t)(pba_internal_program_blocks(e) * pba_internal_patch_len(e));
  inf.num_parameters = n + (pose ? 0 : dim * e->n_points);
  inf.cost = pts.sums[0];
  inf.min_cam_pivot = n > 0 ? cinfo[0] : 1.0;
  if (pts.failed >= 0) {
    times.collect();
    return point_block_failed(e, "pba_covariance", ": the normal matrix is singular", pts.failed, inf, info);
  }
  if (n > 0 && cinfo[1] >= 0.0) {
    times.collect();
    inf.failed_is_point = 0; inf.failed_index = (int32_t)cinfo[1];
    if (info) *info = inf;
    return fail(e, PBA_ERR_NUMERIC, "pba_covariance: non-positive or non-finite pivot at camera column %d (slot %d, parameter %d): the "
                                    "normal matrix is singular; is the gauge fixed?", inf.failed_index, (int)cs.slot_of_col[inf.failed_index / 6], inf.failed_index % 6);
  }
  if (point_cov && !pose && !structure) {
    elim_inputs(e, cp);
    cp.P = e->d_cov_P; cp.C = e->d_cov_C; cp.pp = e->d_cov_pp; cp.n_frames = e->n_frames; cp.n = n;
    times.begin(e, 3);
    hipLaunchKernelGGL(k_cov_points, dim3(pt_blocks), dim3(kElimThreads), 0, e->stream, cp);
    times.end(e, 3);
    HIP_TRY(e, hipGetLastError());
  }
  if (cam_cov) HIP_TRY(e, hipMemcpyAsync(cam_cov, e->d_cov_C, sizeof(double) * n * n, hipMemcpyDeviceToHost, e->stream));
  if (point_cov) HIP_TRY(e, hipMemcpyAsync(point_cov, e->d_cov_pp, sizeof(double) * 9 * e->n_points, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  times.collect();
  if (info) *info = inf;
  return PBA_OK;
}

// Event time [ms] of the four kernels of the LAST pba_covariance (k_cov_point, k_elim_pair with its memset in the pose-only mode,
// k_cov_invert, k_cov_points), -1 for a kernel that did not run or when event profiling (pba_set_profiling(e, 1)) was off.
void pba_internal_covariance_times(const pba_engine* e, double* ms4) { e->cov_times.copy_to(ms4); }

// ---- camera prior (pba_prior.h) ---------------------------------------------------------------------------------------------------
int pba_set_camera_prior(pba_engine* e, int32_t k, const int32_t* slots, const double* x0, const double* Lambda, const double* eta, double c) {
  if (!e) return PBA_ERR_INVALID;
  PBA_NOT_POISONED(e);
  if (!e->have_cams) return fail(e, PBA_ERR_INVALID, "pba_set_camera_prior: the cameras are not set (a prior belongs to one set of cameras)");
  if (k < 0 || k > e->n_frames) return fail(e, PBA_ERR_INVALID, "pba_set_camera_prior: k = %d is outside 0..%d", k, e->n_frames);
  if (k == 0) {
    e->prior_on = false;
    e->prior_k = 0;
    invalidate(e, kInPrior);
    return PBA_OK;
  }
  if (!slots || !x0 || !Lambda || !eta) return fail(e, PBA_ERR_INVALID, "pba_set_camera_prior: null pointer with k = %d", k);
  for (int i = 0; i < k; ++i)
    if (slots[i] < 0 || slots[i] >= e->n_frames || (i > 0 && slots[i] <= slots[i - 1]))
      return fail(e, PBA_ERR_INVALID, "pba_set_camera_prior: slots must ascend and stay below n_frames = %d (slots[%d] = %d)", e->n_frames, i, slots[i]);
  const int m = 6 * k;
  bool finite = std::isfinite(c);
  for (int i = 0; i < m && finite; ++i) finite = std::isfinite(x0[i]) && std::isfinite(eta[i]);
  for (size_t i = 0; i < (size_t)m * m && finite; ++i) finite = std::isfinite(Lambda[i]);
  if (!finite) return fail(e, PBA_ERR_INVALID, "pba_set_camera_prior: non-finite input");
  if (c < 0.0) return fail(e, PBA_ERR_INVALID, "pba_set_camera_prior: c = %g is negative", c);
  if (const char* why = mode_conflict(modes_present(e, e->comm.multi()) & ~(unsigned)kModePrior, kModePrior))
    return fail(e, PBA_ERR_INVALID, "pba_set_camera_prior: %s", why);
  PBA_ENTER(e);
  int rc;
  // (grow-only buffers: a larger prior than the one in use moves them, so nothing of the old one is kept on a failure below -- the
  // stream is idle here: every pass synchronises before it returns)
  if ((rc = dev_alloc(e, &e->d_prior, (size_t)2 * m + (size_t)m * m))) return rc;
  if ((rc = dev_alloc(e, &e->d_prior_out, (size_t)kPriorMaxDim + 1))) return rc;
  HIP_TRY(e, hipMemcpyAsync(e->d_prior, x0, sizeof(double) * m, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_prior + m, eta, sizeof(double) * m, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_prior + 2 * m, Lambda, sizeof(double) * m * m, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  for (int i = 0; i < k; ++i) e->prior_slots[i] = slots[i];
  e->prior_k = k;
  e->prior_c = c;
  e->prior_on = true;
  invalidate(e, kInPrior);
  return PBA_OK;
}

// ---- point prior (pba_point_prior.h) ------------------------------------------------------------------------------------------------
int pba_set_point_prior(pba_engine* e, int32_t n_points, const double* x0, const double* Lambda6) {
  if (!e) return PBA_ERR_INVALID;
  PBA_NOT_POISONED(e);
  if (!e->have_problem) return fail(e, PBA_ERR_INVALID, "pba_set_point_prior: no problem is set (a point prior belongs to one set of points)");
  if (n_points != e->n_points) return fail(e, PBA_ERR_INVALID, "pba_set_point_prior: n_points = %d, the problem has %d", n_points, e->n_points);
  if ((x0 == nullptr) != (Lambda6 == nullptr)) return fail(e, PBA_ERR_INVALID, "pba_set_point_prior: exactly one of x0 and Lambda6 is NULL");
  if (!x0) {
    e->pp_on = false;
    invalidate(e, kInPointPrior);
    return PBA_OK;
  }
  for (size_t i = 0; i < (size_t)n_points; ++i) {
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(x0[3 * i + k])) return fail(e, PBA_ERR_INVALID, "pba_set_point_prior: non-finite x0 of point %zu", i);
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(Lambda6[6 * i + k])) return fail(e, PBA_ERR_INVALID, "pba_set_point_prior: non-finite Lambda of point %zu", i);
    if (Lambda6[6 * i] < 0.0 || Lambda6[6 * i + 3] < 0.0 || Lambda6[6 * i + 5] < 0.0)
      return fail(e, PBA_ERR_INVALID, "pba_set_point_prior: negative diagonal entry of Lambda of point %zu", i);
  }
  if (const char* why = mode_conflict(modes_present(e, e->comm.multi()) & ~(unsigned)kModePointPrior, kModePointPrior))
    return fail(e, PBA_ERR_INVALID, "pba_set_point_prior: %s", why);
  PBA_ENTER(e);
  int rc;
  // From here on the rows of an older prior are overwritten: it is switched off first, so that an upload that fails leaves an engine
  // WITHOUT a prior (and without a linearisation), never one with mixed rows.  (The stream is idle: every pass synchronises before
  // it returns.)
  e->pp_on = false;
  invalidate(e, kInPointPrior);
  if ((rc = dev_alloc(e, &e->d_pp_part, (size_t)kPointPriorMaxGrid))) return rc;
  if ((rc = dev_alloc(e, &e->d_pp_E, (size_t)1))) return rc;
  if (!e->d_pp_ticket) {
    if ((rc = dev_alloc(e, &e->d_pp_ticket, (size_t)1))) return rc;
    HIP_TRY(e, hipMemsetAsync(e->d_pp_ticket, 0, sizeof(unsigned int), e->stream));
  }
  if ((rc = dev_alloc(e, &e->d_pp_x0, (size_t)3 * n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_pp_L6, (size_t)6 * n_points))) return rc;
  HIP_TRY(e, hipMemcpyAsync(e->d_pp_x0, x0, sizeof(double) * 3 * n_points, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemcpyAsync(e->d_pp_L6, Lambda6, sizeof(double) * 6 * n_points, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  e->pp_on = true;
  invalidate(e, kInPointPrior);
  return PBA_OK;
}

// Marginalisation (pba_prior.h).  Every refusal comes before the first launch; the Jacobian pass is pba_linearize's; the kernels write
// buffers of the off-loop calls only (the d_elim_* set is shared with pba_covariance: either call writes all it reads of it), and
// the host copies the results out once every pivot is known to be positive.
int pba_marginalize(pba_engine* e, uint32_t drop_mask, int32_t* slots, double* x0, double* Lambda, double* eta, double* c, pba_marginal_info* info) {
  if (!e) return PBA_ERR_INVALID;
  pba_marginal_info inf{};
  inf.min_point_pivot = 1.0; inf.min_cam_pivot = 1.0; inf.failed_index = -1;
  if (info) *info = inf;
  if (!slots || !x0 || !Lambda || !eta || !c) return fail(e, PBA_ERR_INVALID, "pba_marginalize: null output pointer");
  if (const char* why = mode_conflict(modes_present(e, e->comm.multi()) & ~(unsigned)kModePrior, kModePrior))
    return fail(e, PBA_ERR_INVALID, "pba_marginalize: %s", why);
  { const int rc0 = check_ready(e, "pba_marginalize"); if (rc0) return rc0; }
  if (drop_mask == 0) return fail(e, PBA_ERR_INVALID, "pba_marginalize: drop_mask is empty");
  if (e->n_frames < 32 && (drop_mask >> e->n_frames))
    return fail(e, PBA_ERR_INVALID, "pba_marginalize: drop_mask 0x%x has bits at or above n_frames = %d", drop_mask, e->n_frames);
  // camera columns of the elimination: every free slot in ascending order (the reduced program's columns), split into dropped and kept
  ElimPairParams ms{};
  MargEliminateParams me{};
  int nd_cams = 0, nk_cams = 0;
  int32_t kept_slots[kMaxFrames];
  for (int s = 0; s < e->n_frames; ++s) {
    const int col = slot_free_index(e->anchor_mask, s);
    if (col < 0) continue;
    ms.slot_of_col[col] = (uint8_t)s;
    if ((drop_mask >> s) & 1u) me.col_d[nd_cams++] = (uint8_t)col;
    else { kept_slots[nk_cams] = s; me.col_k[nk_cams++] = (uint8_t)col; }
  }
  if (nk_cams == 0) return fail(e, PBA_ERR_INVALID, "pba_marginalize: no free camera is kept (drop_mask 0x%x, anchor mask 0x%x)", drop_mask, e->anchor_mask);
  const int n_cols = e->n_free, n = 6 * n_cols, nd = 6 * nd_cams, nk = 6 * nk_cams;
  // the marginalised points and their residual blocks
  for (int p = 0; p < e->n_points; ++p) {
    bool in = false;
    for (int o = e->h_pt_begin[p]; o < e->h_pt_begin[p + 1]; ++o) in = in || ((drop_mask >> e->h_obs_slot[o]) & 1u);
    if (in) { ++inf.n_points; inf.n_blocks += e->h_pt_begin[p + 1] - e->h_pt_begin[p]; }
  }
  inf.k = nk_cams;
  const int pt_blocks = (e->n_points + kElimThreads - 1) / kElimThreads;
  PBA_ENTER(e);
  int rc;
  if ((rc = check_lds(e, marg_eliminate_smem_bytes(nd, nk) + 64, "pba_marginalize: ", nd_cams, "dropped free cameras", "their elimination"))) return rc;
  if ((rc = pba_linearize(e, nullptr))) return rc;
  if ((rc = dev_alloc(e, &e->d_elim_X, (size_t)6 * e->n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_marg_z, (size_t)3 * e->n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_elim_part, (size_t)kMargPart * pt_blocks))) return rc;
  if ((rc = dev_alloc(e, &e->d_elim_S, (size_t)n * n))) return rc;
  if ((rc = dev_alloc(e, &e->d_marg_r, (size_t)n))) return rc;
  if ((rc = dev_alloc(e, &e->d_marg_L, (size_t)nk * nk))) return rc;
  if ((rc = dev_alloc(e, &e->d_marg_eta, (size_t)nk))) return rc;
  if ((rc = dev_alloc(e, &e->d_elim_info, (size_t)3))) return rc;
  KernelTimes<5>& times = e->marg_times;
  if ((rc = times.start(e, e->profile))) return rc;
  MargPointParams mp{};
  elim_inputs(e, mp);
  mp.X = e->d_elim_X; mp.z = e->d_marg_z; mp.part = e->d_elim_part; mp.n_frames = e->n_frames; mp.drop_mask = drop_mask;
  times.begin(e, 0);
  hipLaunchKernelGGL(k_marg_point, dim3(pt_blocks), dim3(kElimThreads), 0, e->stream, mp);
  times.end(e, 0);
  elim_inputs(e, ms);
  ms.X = e->d_elim_X; ms.z = e->d_marg_z; ms.S = e->d_elim_S; ms.r = e->d_marg_r; ms.n_cols = n_cols; ms.point_mask = drop_mask;
  times.begin(e, 1);
  hipLaunchKernelGGL(k_elim_pair<true>, dim3(n_cols * (n_cols + 1) / 2), dim3(kElimThreads), 0, e->stream, ms);
  times.end(e, 1);
  times.begin(e, 2);
  hipLaunchKernelGGL(k_marg_grad, dim3(n_cols), dim3(kElimThreads), 0, e->stream, ms);
  times.end(e, 2);
  if (e->prior_on) {
    // the current prior is one more factor: re-expanded at the current cameras (exact: it is quadratic), so priors chain
    PriorParams pp = prior_params(e, e->d_cams[e->cur]);
    pp.S = e->d_elim_S; pp.r = e->d_marg_r; pp.ld = n; pp.out = e->d_prior_out;
    times.begin(e, 3);
    launch_prior(e, pp);
    times.end(e, 3);
  }
  me.S = e->d_elim_S; me.r = e->d_marg_r; me.Lambda = e->d_marg_L; me.eta = e->d_marg_eta; me.info = e->d_elim_info;
  me.n = n; me.nd_cams = nd_cams; me.nk_cams = nk_cams;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_marg_eliminate), hipFuncAttributeMaxDynamicSharedMemorySize, (int)marg_eliminate_smem_bytes(nd, nk));
  (void)hipGetLastError();
  times.begin(e, 4);
  hipLaunchKernelGGL(k_marg_eliminate, dim3(1), dim3(kMargElimThreads), marg_eliminate_smem_bytes(nd, nk), e->stream, me);
  times.end(e, 4);
  HIP_TRY(e, hipGetLastError());
  double einfo[3] = {1.0, -1.0, 0.0}, E_old = 0.0;
  HIP_TRY(e, hipMemcpyAsync(einfo, e->d_elim_info, sizeof(einfo), hipMemcpyDeviceToHost, e->stream));
  if (e->prior_on) HIP_TRY(e, hipMemcpyAsync(&E_old, e->d_prior_out + 6 * e->prior_k, sizeof(double), hipMemcpyDeviceToHost, e->stream));
  PointPartials pts;
  if ((rc = read_point_partials(e, pt_blocks, 2, &pts))) return rc;
  times.collect();
  inf.min_point_pivot = pts.min_pivot;
  inf.cost = pts.sums[0];
  inf.min_cam_pivot = einfo[0];
  if (pts.failed >= 0) return point_block_failed(e, "pba_marginalize", "", pts.failed, inf, info);
  if (einfo[1] >= 0.0) {
    inf.failed_is_point = 0; inf.failed_index = (int32_t)einfo[1];
    if (info) *info = inf;
    return fail(e, PBA_ERR_NUMERIC, "pba_marginalize: non-positive or non-finite pivot at row %d of the dropped cameras' block (slot %d, parameter %d)",
                inf.failed_index, (int)ms.slot_of_col[me.col_d[inf.failed_index / 6]], inf.failed_index % 6);
  }
  // x0: the current cameras of the kept columns, byte for byte
  std::vector<double> cams((size_t)6 * e->n_frames);
  if ((rc = fetch_state(e, cams.data(), nullptr))) return rc;
  HIP_TRY(e, hipMemcpyAsync(Lambda, e->d_marg_L, sizeof(double) * nk * nk, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(eta, e->d_marg_eta, sizeof(double) * nk, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  for (int i = 0; i < nk_cams; ++i) {
    slots[i] = kept_slots[i];
    std::memcpy(x0 + 6 * i, cams.data() + 6 * kept_slots[i], sizeof(double) * 6);
  }
  *c = ((pts.sums[0] - pts.sums[1]) - einfo[2]) + E_old;      // (sums: cost_M | sum over M of |z|^2 / 2)
  if (info) *info = inf;
  return PBA_OK;
}

// Event time [ms] of the five kernels of the LAST pba_marginalize (k_marg_point, k_elim_pair, k_marg_grad, k_prior, k_marg_eliminate),
// -1 for a kernel that did not run or when event profiling (pba_set_profiling(e, 1)) was off.
void pba_internal_marginal_times(const pba_engine* e, double* ms5) { e->marg_times.copy_to(ms5); }

// ---- outlier culling (pba_cull.h) -------------------------------------------------------------------------------------------------
int pba_get_block_costs(pba_engine* e, double* cost) {
  if (!e || !cost) return PBA_ERR_INVALID;
  { const int rc0 = check_ready(e, "pba_get_block_costs"); if (rc0) return rc0; }
  PBA_ENTER(e);
  { const int rc = pba_linearize(e, nullptr); if (rc) return rc; }
  HIP_TRY(e, hipMemcpyAsync(cost, e->d_rec[e->cur] + 5 * e->rec_stride, sizeof(double) * e->n_obs, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

// Test hook: the select kernels of pba_cull on a caller's array; *out = the k-th smallest of v [n] (0-based) in the order of the bit patterns
int pba_internal_select_u64order(pba_engine* e, const double* v, int64_t n, int64_t k, double* out) {
  if (!e || !v || !out || n < 1 || n > INT32_MAX || k < 0 || k >= n) return PBA_ERR_INVALID;
  PBA_ENTER(e);
  int rc;
  if ((rc = dev_alloc(e, &e->d_cull_hist, (size_t)kCullPasses * kCullBins))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_sel, (size_t)kCullSelWords))) return rc;
  DeviceTemp<uint64_t> dv;
  HIP_TRY(e, dv.alloc((size_t)n));
  HIP_TRY(e, hipMemcpyAsync(dv.p, v, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, e->stream));
  cull_enqueue_select(e->stream, dv.p, n, (uint32_t)k, e->d_cull_hist, e->d_cull_sel, 0, 0.0, 0.0);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(out, e->d_cull_sel, sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

// Every refusal that can be known in advance comes before the first launch; the verdict is computed into cull-owned buffers, the host
// reads the keep bytes, the point map and the counts, and only then is anything of the engine's problem replaced.
int pba_cull(pba_engine* e, const pba_cull_options* o, uint8_t* block_keep, int32_t* point_map, pba_cull_info* info) {
  if (!e || !o) return PBA_ERR_INVALID;
  pba_cull_info inf{};
  if (info) *info = inf;
  if (!(o->min_cost >= 0.0) || !std::isfinite(o->min_cost)) return fail(e, PBA_ERR_INVALID, "pba_cull: min_cost = %g must be finite and >= 0", o->min_cost);
  if (!(o->factor >= 0.0) || !std::isfinite(o->factor)) return fail(e, PBA_ERR_INVALID, "pba_cull: factor = %g must be finite and >= 0", o->factor);
  if (!(o->quantile >= 0.0 && o->quantile <= 1.0)) return fail(e, PBA_ERR_INVALID, "pba_cull: quantile = %g must be in [0, 1]", o->quantile);
  if (o->min_observations < 1) return fail(e, PBA_ERR_INVALID, "pba_cull: min_observations = %d must be >= 1", o->min_observations);
  if (const char* why = mode_conflict(modes_present(e, e->comm.multi()), kModeCull)) return fail(e, PBA_ERR_INVALID, "pba_cull: %s", why);
  { const int rc0 = check_ready(e, "pba_cull"); if (rc0) return rc0; }
  PBA_ENTER(e);
  int rc;
  if ((rc = pba_linearize(e, nullptr))) return rc;
  const int n_obs = e->n_obs, n_points = e->n_points, cur = e->cur;
  const int pt_blocks = (n_points + kCullThreads - 1) / kCullThreads, obs_blocks = (n_obs + kCullThreads - 1) / kCullThreads;
  if ((rc = dev_alloc(e, &e->d_cull_hist, (size_t)kCullPasses * kCullBins))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_sel, (size_t)kCullSelWords))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_pt_cnt, (size_t)n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_part, (size_t)pt_blocks))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_off, (size_t)pt_blocks))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_tot, (size_t)kCullTotals))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_map, (size_t)n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_dst, (size_t)n_obs))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_keep, (size_t)n_obs))) return rc;

  const int64_t k = (int64_t)std::floor(o->quantile * (double)(n_obs - 1));
  const double* cost = e->d_rec[cur] + 5 * e->rec_stride;
  cull_enqueue_select(e->stream, reinterpret_cast<const uint64_t*>(cost), n_obs, (uint32_t)k, e->d_cull_hist, e->d_cull_sel, 1, o->min_cost, o->factor);
  CullParams cp{};
  cp.cost = cost; cp.sel = e->d_cull_sel; cp.pt_begin = e->d_pt_begin; cp.obs_point = e->d_obs_point; cp.obs_slot = e->d_obs_slot;
  cp.pt_cnt = e->d_cull_pt_cnt; cp.part = e->d_cull_part; cp.off = e->d_cull_off; cp.tot = e->d_cull_tot; cp.point_map = e->d_cull_map;
  cp.obs_dst = e->d_cull_dst; cp.keep = e->d_cull_keep;
  cp.n_points = n_points; cp.n_obs = n_obs; cp.n_part = pt_blocks; cp.min_observations = o->min_observations;
  hipLaunchKernelGGL(k_cull_verdict, dim3(pt_blocks), dim3(kCullThreads), 0, e->stream, cp);
  hipLaunchKernelGGL(k_cull_offsets, dim3(1), dim3(kCullThreads), 0, e->stream, cp);
  hipLaunchKernelGGL(k_cull_index, dim3(pt_blocks), dim3(kCullThreads), 0, e->stream, cp);
  HIP_TRY(e, hipGetLastError());
  uint64_t sel[kCullSelWords] = {0, 0, 0};
  int32_t tot[kCullTotals] = {0, 0, 0, 0};
  std::vector<uint8_t> keep(n_obs);
  std::vector<int32_t> map(n_points);
  HIP_TRY(e, hipMemcpyAsync(sel, e->d_cull_sel, sizeof(sel), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(tot, e->d_cull_tot, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(keep.data(), e->d_cull_keep, (size_t)n_obs, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(map.data(), e->d_cull_map, sizeof(int32_t) * n_points, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));

  inf.n_blocks_before = inf.n_blocks_after = n_obs;
  inf.n_points_before = inf.n_points_after = n_points;
  std::memcpy(&inf.quantile_cost, &sel[0], sizeof(double));
  std::memcpy(&inf.threshold, &sel[1], sizeof(double));
  if (sel[2]) {
    if (info) *info = inf;
    return fail(e, PBA_ERR_NUMERIC, "pba_cull: factor * quantile_cost = %g * %g is not finite", o->factor, inf.quantile_cost);
  }
  inf.n_points_after = tot[0]; inf.n_blocks_after = tot[1]; inf.n_blocks_over_threshold = tot[2]; inf.n_blocks_by_point_rule = tot[3];
  if (block_keep) std::memcpy(block_keep, keep.data(), keep.size());
  if (point_map) std::memcpy(point_map, map.data(), sizeof(int32_t) * map.size());
  if (info) *info = inf;
  if (!o->apply || inf.n_blocks_after == n_obs) return PBA_OK;
  if (inf.n_points_after == 0)
    return fail(e, PBA_ERR_INVALID, "pba_cull: no point would be left (threshold %g, quantile cost %g, min_observations %d)", inf.threshold,
                inf.quantile_cost, o->min_observations);

  // the survivors, gathered into fresh buffers that then take the place of the engine's
  const int PD = pba_internal_patch_len(e);
  if ((rc = dev_alloc(e, &e->d_cull_xyz, (size_t)3 * n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_desc, (size_t)n_points * PD))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_obs_point, (size_t)n_obs))) return rc;
  if ((rc = dev_alloc(e, &e->d_cull_obs_slot, (size_t)n_obs))) return rc;
  if (e->inverse_depth && (rc = dev_alloc(e, &e->d_cull_rays, (size_t)6 * n_points))) return rc;
  if (e->pp_on) {
    if ((rc = dev_alloc(e, &e->d_cull_pp_x0, (size_t)3 * n_points))) return rc;
    if ((rc = dev_alloc(e, &e->d_cull_pp_L6, (size_t)6 * n_points))) return rc;
  }
  cp.obs_point_new = e->d_cull_obs_point; cp.obs_slot_new = e->d_cull_obs_slot;
  const auto row_grid = [&](int row_len) { return dim3((unsigned)std::min<int64_t>(((int64_t)n_points * row_len + kCullThreads - 1) / kCullThreads, 1 << 16)); };
  hipLaunchKernelGGL(k_cull_gather_obs, dim3(obs_blocks), dim3(kCullThreads), 0, e->stream, cp);
  hipLaunchKernelGGL(k_cull_gather_rows<double>, row_grid(3), dim3(kCullThreads), 0, e->stream, (const double*)e->d_xyz[cur], e->d_cull_xyz,
                     (const int32_t*)e->d_cull_map, n_points, 3);
  hipLaunchKernelGGL(k_cull_gather_rows<float>, row_grid(PD), dim3(kCullThreads), 0, e->stream, (const float*)e->d_desc, e->d_cull_desc,
                     (const int32_t*)e->d_cull_map, n_points, PD);
  if (e->inverse_depth)
    hipLaunchKernelGGL(k_cull_gather_rows<double>, row_grid(6), dim3(kCullThreads), 0, e->stream, (const double*)e->d_rays, e->d_cull_rays,
                       (const int32_t*)e->d_cull_map, n_points, 6);
  if (e->pp_on) {      // the point prior's rows travel with the surviving points
    hipLaunchKernelGGL(k_cull_gather_rows<double>, row_grid(3), dim3(kCullThreads), 0, e->stream, (const double*)e->d_pp_x0, e->d_cull_pp_x0,
                       (const int32_t*)e->d_cull_map, n_points, 3);
    hipLaunchKernelGGL(k_cull_gather_rows<double>, row_grid(6), dim3(kCullThreads), 0, e->stream, (const double*)e->d_pp_L6, e->d_cull_pp_L6,
                       (const int32_t*)e->d_cull_map, n_points, 6);
  }
  HIP_TRY(e, hipGetLastError());
  // the surviving lists on the host, for the tile builder pba_set_problem runs
  std::vector<int32_t> op((size_t)inf.n_blocks_after), os((size_t)inf.n_blocks_after);
  {
    size_t d = 0;
    for (int p = 0; p < n_points; ++p)
      for (int ob = e->h_pt_begin[p]; ob < e->h_pt_begin[p + 1]; ++ob)
        if (keep[ob]) { op[d] = map[p]; os[d] = e->h_obs_slot[ob]; ++d; }
  }
  if (e->inverse_depth) {
    for (int p = 0; p < n_points; ++p)
      if (map[p] >= 0 && map[p] != p) std::memmove(&e->h_rays[6 * (size_t)map[p]], &e->h_rays[6 * (size_t)p], 6 * sizeof(double));
    e->h_rays.resize((size_t)6 * inf.n_points_after);
  }
  ProblemLayout L;
  if ((rc = problem_layout(e, inf.n_points_after, inf.n_blocks_after, op.data(), os.data(), &L))) return rc;
  e->mem.exchange(&e->d_xyz[cur], &e->d_cull_xyz);
  e->mem.exchange(&e->d_desc, &e->d_cull_desc);
  e->mem.exchange(&e->d_obs_point, &e->d_cull_obs_point);
  e->mem.exchange(&e->d_obs_slot, &e->d_cull_obs_slot);
  if (e->inverse_depth) e->mem.exchange(&e->d_rays, &e->d_cull_rays);
  if (e->pp_on) { e->mem.exchange(&e->d_pp_x0, &e->d_cull_pp_x0); e->mem.exchange(&e->d_pp_L6, &e->d_cull_pp_L6); }
  if ((rc = problem_reserve(e, L, PD))) return rc;
  if ((rc = problem_upload_tables(e, L))) return rc;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  problem_installed(e, &L);
  invalidate(e, kInProblem);
  inf.applied = 1;
  if (info) *info = inf;
  return PBA_OK;
}

// ---- re-observation (pba_admit.h) -------------------------------------------------------------------------------------------------
// The Jacobian pass of the current state over ANOTHER observation list of the same points: the kernel, the sampler and the loss of
// pba_linearize, records and block partials into the caller's buffers.  No counter, event or validity flag of the engine moves.
static void admit_sample_list(pba_engine* e, SampleParams sp, int n) {
  const int grid = e->sample_grid;
  e->sample_grid = (n + e->sample_waves * 64 - 1) / (e->sample_waves * 64);
  launch_sample<true>(e, sp);
  e->sample_grid = grid;
}

// Sizing: count, then fill.  k_admit_enum + k_admit_offsets give the number of candidates, the host reads it (one int) and sizes the list,
// the records and the launch of the candidates' pass by it; the same pair (k_admit_count + k_admit_offsets) sizes the merged lists.
int pba_admit(pba_engine* e, const pba_admit_options* o, int32_t capacity, int32_t* cand_point, int32_t* cand_slot, double* cand_cost, uint8_t* cand_take,
              pba_admit_info* info) {
  if (!e || !o) return PBA_ERR_INVALID;
  pba_admit_info inf{};
  if (info) *info = inf;
  if (!(o->min_depth > 0.0) || !std::isfinite(o->min_depth)) return fail(e, PBA_ERR_INVALID, "pba_admit: min_depth = %g must be finite and > 0", o->min_depth);
  if (o->border < 0) return fail(e, PBA_ERR_INVALID, "pba_admit: border = %d must be >= 0", o->border);
  if (!(o->min_cost >= 0.0) || !std::isfinite(o->min_cost)) return fail(e, PBA_ERR_INVALID, "pba_admit: min_cost = %g must be finite and >= 0", o->min_cost);
  if (!(o->factor >= 0.0) || !std::isfinite(o->factor)) return fail(e, PBA_ERR_INVALID, "pba_admit: factor = %g must be finite and >= 0", o->factor);
  if (!(o->quantile >= 0.0 && o->quantile <= 1.0)) return fail(e, PBA_ERR_INVALID, "pba_admit: quantile = %g must be in [0, 1]", o->quantile);
  if (capacity < 0) return fail(e, PBA_ERR_INVALID, "pba_admit: capacity = %d must be >= 0", capacity);
  if (o->slot_mask == 0) return fail(e, PBA_ERR_INVALID, "pba_admit: slot_mask is empty");
  if (const char* why = mode_conflict(modes_present(e, e->comm.multi()), kModeAdmit)) return fail(e, PBA_ERR_INVALID, "pba_admit: %s", why);
  { const int rc0 = check_ready(e, "pba_admit"); if (rc0) return rc0; }
  if (e->n_frames < 32 && (o->slot_mask >> e->n_frames))
    return fail(e, PBA_ERR_INVALID, "pba_admit: slot_mask 0x%x has bits at or above n_frames = %d", o->slot_mask, e->n_frames);
  for (int s = 0; s < e->n_frames; ++s)
    if (((o->slot_mask >> s) & 1u) && !e->frame_set[s]) return fail(e, PBA_ERR_INVALID, "pba_admit: slot %d of slot_mask holds no frame", s);
  PBA_ENTER(e);
  int rc;
  if ((rc = pba_linearize(e, nullptr))) return rc;
  const int n_obs = e->n_obs, n_points = e->n_points, cur = e->cur;
  const int pt_blocks = (n_points + kAdmitThreads - 1) / kAdmitThreads;
  if ((rc = dev_alloc(e, &e->d_admit_hist, (size_t)kCullPasses * kCullBins))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_sel, (size_t)kCullSelWords))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_cand_mask, (size_t)n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_take_mask, (size_t)n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_cand_begin, (size_t)n_points))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_part, (size_t)pt_blocks))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_off, (size_t)pt_blocks))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_tot, (size_t)kAdmitTotals))) return rc;

  AdmitParams ap{};
  ap.xyz = e->d_xyz[cur]; ap.rays = rays_or_null(e); ap.geom = e->d_geom[cur]; ap.pt_begin = e->d_pt_begin; ap.obs_slot = e->d_obs_slot;
  ap.sel = e->d_admit_sel; ap.cand_mask = e->d_admit_cand_mask; ap.take_mask = e->d_admit_take_mask; ap.cand_begin = e->d_admit_cand_begin;
  ap.part = e->d_admit_part; ap.off = e->d_admit_off; ap.tot = e->d_admit_tot;
  ap.fx = e->cfg.fx; ap.fy = e->cfg.fy; ap.cx = e->cfg.cx; ap.cy = e->cfg.cy;
  ap.min_depth = o->min_depth;
  ap.u_lo = (double)o->border; ap.u_hi = (double)(e->cfg.cols - 1 - o->border);
  ap.v_lo = (double)o->border; ap.v_hi = (double)(e->cfg.rows - 1 - o->border);
  ap.slot_mask = o->slot_mask; ap.n_points = n_points; ap.n_frames = e->n_frames; ap.n_part = pt_blocks;

  // the count ...
  int32_t tot[kAdmitTotals] = {0, 0};
  hipLaunchKernelGGL(k_admit_enum, dim3(pt_blocks), dim3(kAdmitThreads), 0, e->stream, ap);
  hipLaunchKernelGGL(k_admit_offsets, dim3(1), dim3(kAdmitThreads), 0, e->stream, ap);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(tot, e->d_admit_tot, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  const int n_cand = tot[0];
  const int cand_blocks = (n_cand + kAdmitThreads - 1) / kAdmitThreads;
  ap.n_cand = n_cand;

  // ... then the fill, and the candidates' costs through the Jacobian pass
  const int64_t cand_stride = ((int64_t)n_cand + 255) / 256 * 256;
  if (n_cand > 0) {
    const int sample_blocks = (n_cand + e->sample_waves * 64 - 1) / (e->sample_waves * 64);
    if ((rc = dev_alloc(e, &e->d_admit_cand_point, (size_t)n_cand))) return rc;
    if ((rc = dev_alloc(e, &e->d_admit_cand_slot, (size_t)n_cand))) return rc;
    if ((rc = dev_alloc(e, &e->d_admit_cand_take, (size_t)n_cand))) return rc;
    if ((rc = dev_alloc(e, &e->d_admit_rec, (size_t)6 * cand_stride))) return rc;
    if ((rc = dev_alloc(e, &e->d_admit_block_cost, (size_t)sample_blocks))) return rc;
    if ((rc = dev_alloc(e, &e->d_admit_block_fail, (size_t)sample_blocks))) return rc;
    ap.cand_point = e->d_admit_cand_point; ap.cand_slot = e->d_admit_cand_slot; ap.cand_take = e->d_admit_cand_take;
    ap.cand_cost = e->d_admit_rec + 5 * cand_stride;
    hipLaunchKernelGGL(k_admit_fill, dim3(pt_blocks), dim3(kAdmitThreads), 0, e->stream, ap);
    SampleParams sp = make_sample_params(e, cur);
    sp.obs_point = e->d_admit_cand_point; sp.obs_slot = e->d_admit_cand_slot; sp.n_obs = n_cand;
    sp.rec = e->d_admit_rec; sp.rec_stride = cand_stride; sp.block_cost = e->d_admit_block_cost; sp.block_fail = e->d_admit_block_fail;
    admit_sample_list(e, sp, n_cand);
  }

  // the verdict: the order statistic over the costs of the problem's own blocks, the threshold, one lane per candidate
  const int64_t k = (int64_t)std::floor(o->quantile * (double)(n_obs - 1));
  const double* cost = e->d_rec[cur] + 5 * e->rec_stride;
  cull_enqueue_select(e->stream, reinterpret_cast<const uint64_t*>(cost), n_obs, (uint32_t)k, e->d_admit_hist, e->d_admit_sel, 1, o->min_cost, o->factor);
  HIP_TRY(e, hipMemsetAsync(e->d_admit_take_mask, 0, sizeof(uint32_t) * n_points, e->stream));
  if (n_cand > 0) hipLaunchKernelGGL(k_admit_verdict, dim3(cand_blocks), dim3(kAdmitThreads), 0, e->stream, ap);
  hipLaunchKernelGGL(k_admit_count, dim3(pt_blocks), dim3(kAdmitThreads), 0, e->stream, ap);
  hipLaunchKernelGGL(k_admit_offsets, dim3(1), dim3(kAdmitThreads), 0, e->stream, ap);
  HIP_TRY(e, hipGetLastError());
  uint64_t sel[kCullSelWords] = {0, 0, 0};
  std::vector<int32_t> h_point(n_cand);
  std::vector<uint8_t> h_slot(n_cand), h_take(n_cand);
  std::vector<double> h_cost(n_cand);
  HIP_TRY(e, hipMemcpyAsync(sel, e->d_admit_sel, sizeof(sel), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(tot, e->d_admit_tot, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
  if (n_cand > 0) {
    HIP_TRY(e, hipMemcpyAsync(h_point.data(), e->d_admit_cand_point, sizeof(int32_t) * n_cand, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(h_slot.data(), e->d_admit_cand_slot, (size_t)n_cand, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(h_take.data(), e->d_admit_cand_take, (size_t)n_cand, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(h_cost.data(), ap.cand_cost, sizeof(double) * n_cand, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));

  inf.n_blocks_before = inf.n_blocks_after = n_obs;
  inf.n_points = n_points;
  inf.n_candidates = n_cand;
  std::memcpy(&inf.quantile_cost, &sel[0], sizeof(double));
  std::memcpy(&inf.threshold, &sel[1], sizeof(double));
  if (sel[2]) {
    if (info) *info = inf;
    return fail(e, PBA_ERR_NUMERIC, "pba_admit: factor * quantile_cost = %g * %g is not finite", o->factor, inf.quantile_cost);
  }
  inf.n_blocks_after = tot[0]; inf.n_admitted = tot[1];
  inf.n_written = std::min(n_cand, capacity);
  for (int i = 0; i < inf.n_written; ++i) {
    if (cand_point) cand_point[i] = h_point[i];
    if (cand_slot) cand_slot[i] = h_slot[i];
    if (cand_cost) cand_cost[i] = h_cost[i];
    if (cand_take) cand_take[i] = h_take[i];
  }
  if (info) *info = inf;
  if (!o->apply || inf.n_admitted == 0) return PBA_OK;
  if (inf.n_blocks_after != n_obs + inf.n_admitted) return fail(e, PBA_ERR_HIP, "pba_admit: the merged count %d is not %d + %d", inf.n_blocks_after, n_obs, inf.n_admitted);

  // the merged lists, written into fresh buffers that then take the place of the engine's
  const int n_after = inf.n_blocks_after;
  if ((rc = dev_alloc(e, &e->d_admit_obs_point, (size_t)n_after))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_obs_slot, (size_t)n_after))) return rc;
  if ((rc = dev_alloc(e, &e->d_admit_pt_begin, (size_t)n_points + 1))) return rc;
  ap.obs_point_new = e->d_admit_obs_point; ap.obs_slot_new = e->d_admit_obs_slot; ap.pt_begin_new = e->d_admit_pt_begin;
  hipLaunchKernelGGL(k_admit_merge, dim3(pt_blocks), dim3(kAdmitThreads), 0, e->stream, ap, (int32_t)n_after);
  HIP_TRY(e, hipGetLastError());
  // ... and on the host, from the candidate list and the take bytes, for the tile builder pba_set_problem runs
  std::vector<int32_t> op((size_t)n_after), os((size_t)n_after);
  {
    size_t d = 0, c = 0;
    for (int p = 0; p < n_points; ++p) {
      int ob = e->h_pt_begin[p];
      const int ob1 = e->h_pt_begin[p + 1];
      while (c < (size_t)n_cand && h_point[c] == p && !h_take[c]) ++c;
      while (ob < ob1 || (c < (size_t)n_cand && h_point[c] == p)) {
        const bool have_new = c < (size_t)n_cand && h_point[c] == p;
        if (ob < ob1 && (!have_new || e->h_obs_slot[ob] < h_slot[c])) { op[d] = p; os[d] = e->h_obs_slot[ob]; ++ob; }
        else { op[d] = p; os[d] = h_slot[c]; ++c; while (c < (size_t)n_cand && h_point[c] == p && !h_take[c]) ++c; }
        ++d;
      }
    }
    if (d != (size_t)n_after) return fail(e, PBA_ERR_HIP, "pba_admit: the host's merged list holds %zu blocks, the device's %d", d, n_after);
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));      // (the merge read d_pt_begin / d_obs_slot: done before they are replaced)
  const int PD = pba_internal_patch_len(e);
  ProblemLayout L;
  if ((rc = problem_layout(e, n_points, n_after, op.data(), os.data(), &L))) return rc;
  e->mem.exchange(&e->d_obs_point, &e->d_admit_obs_point);
  e->mem.exchange(&e->d_obs_slot, &e->d_admit_obs_slot);
  if ((rc = problem_reserve(e, L, PD))) return rc;
  if ((rc = problem_upload_tables(e, L))) return rc;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  problem_installed(e, &L);
  invalidate(e, kInProblem);
  inf.applied = 1;
  if (info) *info = inf;
  return PBA_OK;
}

int pba_get_obs_records(pba_engine* e, double* rec6) {
  if (!e || !rec6) return PBA_ERR_INVALID;
  if (!e->have_problem) return fail(e, PBA_ERR_STATE, "no problem");
  PBA_ENTER(e);
  std::vector<double> tmp((size_t)6 * e->rec_stride);
  HIP_TRY(e, hipMemcpyAsync(tmp.data(), e->d_rec[e->cur], sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  for (int o = 0; o < e->n_obs; ++o)
    for (int k = 0; k < 6; ++k) rec6[(size_t)o * 6 + k] = tmp[(size_t)k * e->rec_stride + o];
  return PBA_OK;
}

int pba_comm_unique_id(void* id128) { return Comm::unique_id(id128) ? PBA_ERR_COMM : PBA_OK; }

// What both pba_comm_init_* ask first: may an engine in this state join `world` ranks?
static int comm_init_refusal(pba_engine* e, int32_t world) {
  unsigned with = 0;
  const char* why = world > 1 ? mode_conflict(modes_present(e, false), kModeMulti, &with) : nullptr;
  if (!why) return PBA_OK;
  if (with == kModeWide) return fail(e, PBA_ERR_INVALID, "pba_comm_init: %s (%d free cameras)", why, e->n_free);
  if (with == kModeAnchors) return fail(e, PBA_ERR_INVALID, "pba_comm_init: %s (pba_set_cameras_anchored holds %d)", why, e->n_frames - e->n_free);
  return fail(e, PBA_ERR_INVALID, "pba_comm_init: %s", why);
}

int pba_comm_init_rccl(pba_engine* e, const void* id128, int32_t rank, int32_t world) {
  if (!e || !id128 || world < 1 || rank < 0 || rank >= world) return PBA_ERR_INVALID;
  if (const int rc = comm_init_refusal(e, world)) return rc;
  PBA_ENTER(e);
  if (e->comm.init_rccl(id128, rank, world)) return fail(e, PBA_ERR_COMM, "%s", e->comm.err.c_str());
  return PBA_OK;
}

int pba_comm_init_callback(pba_engine* e, pba_allreduce_fn fn, void* ctx, int32_t rank, int32_t world) {
  if (!e || !fn || world < 1 || rank < 0 || rank >= world) return PBA_ERR_INVALID;
  if (const int rc = comm_init_refusal(e, world)) return rc;
  PBA_ENTER(e);
  if (e->comm.init_callback(fn, ctx, rank, world)) return fail(e, PBA_ERR_COMM, "%s", e->comm.err.c_str());
  return PBA_OK;
}

int pba_comm_enable_peer_exchange(pba_engine* e) {
  if (!e) return PBA_ERR_INVALID;
  if (e->comm.kind == 0) return fail(e, PBA_ERR_STATE, "call order violated: pba_comm_enable_peer_exchange before pba_comm_init_*");
  PBA_ENTER(e);
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (e->comm.enable_peer()) e->err = e->comm.err;      // not an error: the base transport keeps serving (pba_comm_transport tells)
  return PBA_OK;
}

int pba_comm_rank_count(const pba_engine* e) { return e ? e->comm.rank_count() : 0; }

const char* pba_comm_transport(const pba_engine* e) {
  if (!e || e->comm.kind == 0) return "none";
  if (e->comm.kind == 1) return e->comm.peer ? "rccl+peer" : "rccl";
  return e->comm.peer ? "callback+peer" : "callback";
}

const char* pba_solve_driver(const pba_engine* e) {
  static const char* names[] = {"none", "resident", "pipelined", "host-stepped", "batched"};
  return names[(e && e->last_driver >= 0 && e->last_driver <= 4) ? e->last_driver : 0];
}

int pba_get_counters(pba_engine* e, pba_counters* c) {
  if (!e || !c) return PBA_ERR_INVALID;
  if (e->stamps && e->d_stamp && e->last_driver == 1) {
    // resident solve: phase stamps of the serial workgroup.  The three counters keep their meaning as SHARES OF THE ITERATION: elimination
    // (k_schur's work) | reduction of the partials + reduced solve (k_reduce_solve's) | back-substitution + sampling + decision (k_sample's)
    PBA_ENTER(e);
    const int n_rec = std::min(std::max(e->stamp_iter, 0) + 2, (int)kStampMaxIters);
    std::vector<unsigned long long> st((size_t)n_rec * kResStampRecord);
    HIP_TRY(e, hipMemcpyAsync(st.data(), e->d_stamp, sizeof(unsigned long long) * st.size(), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    double d_sample = 0.0, d_schur = 0.0, d_solve = 0.0;
    int64_t n = 0;
    for (int it = 2; it < n_rec; ++it) {
      const unsigned long long* r = &st[(size_t)it * kResStampRecord];
      const unsigned long long prev = st[(size_t)(it - 1) * kResStampRecord + kResStampDecided];
      if (!prev || r[kResStampSchur] <= prev || r[kResStampSolved] <= r[kResStampSchur] || r[kResStampDecided] <= r[kResStampSolved]) continue;   // a step that did not run
      d_schur += (double)(r[kResStampSchur] - prev); d_solve += (double)(r[kResStampSolved] - r[kResStampSchur]);
      d_sample += (double)(r[kResStampDecided] - r[kResStampSolved]);
      ++n;
    }
    e->ctr.linearize_ms = 1e-5 * d_sample; e->ctr.linearize_launches = n;
    e->ctr.schur_ms = 1e-5 * d_schur; e->ctr.schur_launches = n;
    e->ctr.solve_ms = 1e-5 * d_solve; e->ctr.solve_launches = n;
  } else if (e->stamps && e->d_stamp) {
    // device time stamps of the LAST asynchronous solve (100 MHz ticks): intervals between consecutive kernel ends
    PBA_ENTER(e);
    const int n_rec = std::min(e->stamp_iter, (int)kStampMaxIters) + 1;
    std::vector<unsigned long long> st((size_t)n_rec * kStampRecord);
    HIP_TRY(e, hipMemcpyAsync(st.data(), e->d_stamp, sizeof(unsigned long long) * st.size(), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    double d_sample = 0.0, d_schur = 0.0, d_solve = 0.0;
    int64_t n = 0;
    for (int it = 1; it < n_rec; ++it) {
      const unsigned long long* r = &st[(size_t)it * kStampRecord];
      const unsigned long long prev = st[(size_t)(it - 1) * kStampRecord + kStampEndSample];
      unsigned long long e_schur = 0;
      for (int b = 0; b < kStampSchurBlocks; ++b) e_schur = std::max(e_schur, r[kStampSchur0 + b]);
      if (!prev || e_schur <= prev || r[kStampEndSolve] <= e_schur || r[kStampEndSample] <= r[kStampEndSolve]) continue;   // a step that did not run
      d_schur += (double)(e_schur - prev); d_solve += (double)(r[kStampEndSolve] - e_schur); d_sample += (double)(r[kStampEndSample] - r[kStampEndSolve]);
      ++n;
    }
    e->ctr.linearize_ms = 1e-5 * d_sample; e->ctr.linearize_launches = n;
    e->ctr.schur_ms = 1e-5 * d_schur; e->ctr.schur_launches = n;
    e->ctr.solve_ms = 1e-5 * d_solve; e->ctr.solve_launches = n;
  }
  *c = e->ctr;
  return PBA_OK;
}

int pba_reset_counters(pba_engine* e) {
  if (!e) return PBA_ERR_INVALID;
  const int64_t no = e->ctr.n_obs, np = e->ctr.n_points;
  e->ctr = pba_counters{};
  e->ctr.n_obs = no; e->ctr.n_points = np;
  e->profile = true;   // counters are only collected once asked for
  e->stamps = false;
  return PBA_OK;
}

int pba_set_profiling(pba_engine* e, int32_t mode) {
  if (!e || mode < 0 || mode > 2) return PBA_ERR_INVALID;
  PBA_ENTER(e);
  const int64_t no = e->ctr.n_obs, np = e->ctr.n_points;
  e->ctr = pba_counters{};
  e->ctr.n_obs = no; e->ctr.n_points = np;
  e->profile = (mode == 1);
  e->stamps = (mode == 2);
  e->stamp_iter = 0;
  if (e->stamps) {
    const int rc = dev_alloc(e, &e->d_stamp, (size_t)(kStampMaxIters + 1) * kStampRecord);
    if (rc) return rc;
    HIP_TRY(e, hipMemsetAsync(e->d_stamp, 0, sizeof(unsigned long long) * (kStampMaxIters + 1) * kStampRecord, e->stream));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return PBA_OK;
}

}  // extern "C"

// resident solve (pba_resident.h): kernel and LDS pool of the engine's patch radius / weights
namespace {
template <int R, bool UNITW>
const void* resident_kernel() { return reinterpret_cast<const void*>(&k_resident<R, UNITW>); }
const void* resident_kernel_for(const pba_engine* e) {
  if (e->cfg.radius == 1) return e->unit_weights ? resident_kernel<1, true>() : resident_kernel<1, false>();
  return e->unit_weights ? resident_kernel<2, true>() : resident_kernel<2, false>();
}
size_t resident_pool_for(const pba_engine* e) {
  const int n = 6 * e->n_free;
  return e->cfg.radius == 1 ? resident_pool_bytes<1>(n) : resident_pool_bytes<2>(n);
}
}  // namespace

// engine internals needed by the LM driver (pba_lm.cpp)
extern "C" {
int pba_internal_world(const pba_engine* e) { return e->comm.world; }
int pba_internal_rank(const pba_engine* e) { return e->comm.rank; }
int pba_internal_is_multi(const pba_engine* e) { return e->comm.multi() ? 1 : 0; }
int64_t pba_internal_local_blocks(const pba_engine* e) { return e->n_obs; }
int pba_internal_patch_len(const pba_engine* e) { return e->channels * (2 * e->cfg.radius + 1) * (2 * e->cfg.radius + 1); }
// ---- asynchronous driver ----------------------------------------------------------------------------------------
int pba_internal_async_capable(const pba_engine* e, const pba_solver_options* o) {
  if (e->points_const || e->cams_const) return 0;     // the pose-only and structure-only modes are built on the host-stepped driver
  if (e->prior_on) return 0;                          // the camera prior is an addend between reduction and solve: host-stepped only
  if (e->pp_on) return 0;                             // the point prior eliminates through the wide chain: host-stepped only
  return e->use_async && fused_capable(e) && (e->comm.kind != 2 || e->comm.peer) && o->max_num_iterations < pba_engine::kMaxLog - 2 && !e->profile;
}
int pba_internal_points_constant(const pba_engine* e) { return e->points_const ? 1 : 0; }
// residual blocks of the reduced program: those of the free cameras
int64_t pba_internal_program_blocks(const pba_engine* e) {
  if (!e->points_const || e->anchor_mask == 0) return e->n_obs;
  int64_t n = 0;
  for (uint8_t s : e->h_obs_slot) n += slot_is_free(e->anchor_mask, (int)s);
  return n;
}
// cost of the residual blocks of the constant cameras, as the last pba_step found it (0 outside the mode)
double pba_internal_fixed_cost(const pba_engine* e) {
  return e->points_const ? reinterpret_cast<const volatile double*>(e->h_scal)[kPoseFixedCost] : 0.0;
}
int pba_internal_refuse(pba_engine* e, int code, const char* msg) { return fail(e, code, "%s", msg); }

int pba_internal_ready(pba_engine* e) { return check_ready(e, "pba_solve"); }

// 1: the final (gradient-only) enqueue, kind 2, also flushes to the host mirror -- no kind-3 enqueue behind it (single rank, the
// reduction + solve as one launch)
int pba_internal_final_flushes(const pba_engine* e) {
  static const bool off = [] { const char* sv = getenv("PBA_FUSE_FINAL"); return sv && atoi(sv) == 0; }();
  return (!off && !e->comm.multi() && e->solve_kind == 0 && !PBA_PHASE_TIMING) ? 1 : 0;
}

int pba_internal_async_begin(pba_engine* e, const pba_solver_options* o) {
  { const int rc0 = check_ready(e, "pba_solve"); if (rc0) return rc0; }
  PBA_ENTER(e);
  const LmState st = lm_initial_state(o, e->cur);
  *e->h_lm = st;
  // The device copy of the initial state is made by the first kernel of the solve (workgroup 0 of the kind-0 sampling pass reads the
  // host-mapped mirror: SampleParams::lm_init_*); PBA_LM_INIT_KERNEL=1 keeps the separate launch of rounds 3-4.
  if (PBA_LM_INIT_KERNEL) {
    hipLaunchKernelGGL(k_lm_init, dim3(1), dim3(64), 0, e->stream, e->d_lm, st);
    HIP_TRY(e, hipGetLastError());
  }
  e->async_cur = e->cur;
  e->last_driver = 2;
  return PBA_OK;
}

}  // extern "C"

// ---- parameters of the asynchronous driver's passes (pba_internal_async_enqueue; the batched launches of pba_solve_batch use the same) ----
namespace {
// the fused sampling pass: kind 0 = first linearisation (plain Jacobian pass at the current point), 1 = candidate pass of a full
// iteration (single rank: decide = 1, stamps and the sequence number are the caller's)
SampleParams async_sample_params(pba_engine* e, int kind) {
  const int cur = e->async_cur, cand = 1 - cur;
  const bool skip = kind == 0;
  unsigned long long* const h_seq_dev = host_seq_dev(e);
  SampleParams sp = make_sample_params(e, skip ? cur : cand);
  sp.tile_info = e->d_tile_info; sp.lane_rec = e->d_lane_rec;
  sp.geom_prev = e->d_geom[skip ? cand : cur]; sp.xyz_prev = e->d_xyz[skip ? cand : cur]; sp.rec_prev = e->d_rec[skip ? cand : cur];
  sp.sp = e->d_sp; sp.ptrec = e->d_ptrec; sp.delta_c = e->d_delta_c; sp.block_bs = e->d_bs_out; sp.ticket = e->d_ticket;
  sp.scal = e->d_scal; sp.n_tiles = e->n_tiles; sp.skip_backsub = skip ? 1 : 0;
  sp.block_cost_alt = e->d_block_cost[skip ? cand : cur]; sp.block_fail_alt = e->d_block_fail[skip ? cand : cur];
  sp.host_state = e->h_lm_dev; sp.log = e->d_log; sp.max_log = pba_engine::kMaxLog;
  sp.host_seq = h_seq_dev; sp.enq_cur = cur;
  sp.host_scal = nullptr;     // kind 1: published by the next k_schur (or k_flush): see SchurParams::pub_*
  if (skip) {
    sp.lm = nullptr; sp.seq = 0; sp.decide = 0;
    if (!PBA_LM_INIT_KERNEL) { sp.lm_init_dst = e->d_lm; sp.lm_init_src = e->h_lm_dev; }
  } else {
    sp.lm = e->d_lm; sp.decide = 1;
  }
  return sp;
}
// k_schur of kind 1 (full iteration) / 2 (gradient norms of the final point); pub_seq = the engine's last sequence number, no stamps
SchurParams async_schur_params(pba_engine* e, int kind, int init_scale, const pba_solver_options* o) {
  const int cur = e->async_cur, cand = 1 - cur;
  SchurParams sc = schur_params(e, cur, init_scale, o, 1.0);      // (the radius comes from the device state)
  // the previous enqueue decided on the device (last workgroup of the fused sampling kernel, or k_decide after the
  // multi-rank exchange) without publishing; this kernel does
  sc.pub_state = e->h_lm_dev; sc.pub_scal = e->d_scal; sc.pub_host_scal = e->h_scal_dev;
  sc.pub_host_seq = host_seq_dev(e); sc.pub_seq = e->seq;
  sc.lm = e->d_lm; sc.enq_cur = cur; sc.final_pass = (kind == 2) ? 1 : 0; sc.xyz_alt = e->d_xyz[cand]; sc.geom_alt = e->d_geom[cand]; sc.rec_alt = e->d_rec[cand];
  return sc;
}
SolveParams async_solve_params(pba_engine* e, int kind, int init_scale, const pba_solver_options* o) {
  const int cur = e->async_cur, cand = 1 - cur;
  SolveParams so = solve_params(e, cur, init_scale, o, 1.0, kind == 1);
  so.lm = e->d_lm; so.enq_cur = cur; so.final_pass = (kind == 2) ? 1 : 0; so.cams_alt = e->d_cams[cand]; so.cams_cand_alt = e->d_cams[cur]; so.geom_alt = e->d_geom[cand];
  so.geom_cand_alt = e->d_geom[cur];
  return so;
}
// the end of a single-rank solve folded into its final pass (decision + flush by the last workgroup of k_reduce_solve)
ReduceSolveParams::Fin async_fin(pba_engine* e, unsigned long long seq) {
  ReduceSolveParams::Fin fin{};
  fin.lm = e->d_lm; fin.log = e->d_log; fin.host_log = e->h_log_dev; fin.max_log = (int)pba_engine::kMaxLog; fin.host_state = e->h_lm_dev;
  fin.host_scal = e->h_scal_dev; fin.host_seq = host_seq_dev(e); fin.seq = seq;
  return fin;
}
}  // namespace

extern "C" {
// kind 0: first linearisation; 1: full iteration; 2: gradient norms of the final point; 3: flush (log + state to the
// host).  Returns the sequence number that marks the enqueued work as complete (0 for kind 0).  Single rank: a kind-1
// sequence number is published by the NEXT kind-1 / kind-3 enqueue, so callers end every solve with a flush.
int pba_internal_async_enqueue(pba_engine* e, int kind, int init_scale, const pba_solver_options* o, unsigned long long* seq_out) {
  const int cur = e->async_cur, cand = 1 - cur;
  const int n = 6 * e->n_free;
  const bool multi = e->comm.multi();
  unsigned long long* const h_seq_dev = host_seq_dev(e);
  *seq_out = 0;
  if (kind == 0) {
    // plain Jacobian pass at the current point, on the fused (tile) grid so that both parities share one block count
    SampleParams sp = async_sample_params(e, 0);
    e->stamp_iter = 0;
    sp.stamp = stamp_record(e);
    launch_sample<true, true>(e, sp);
    e->jac_passes++;
    e->cost_blocks[0] = e->cost_blocks[1] = e->fused_grid;
    HIP_TRY(e, hipGetLastError());
    return PBA_OK;
  }
  if (kind == 3) {
    // end of the solve: iteration log, final state and sequence number to the host mirror
    const unsigned long long seq = ++e->seq;
    hipLaunchKernelGGL(k_flush, dim3(1), dim3(256), 0, e->stream, (const LmState*)e->d_lm, e->h_lm_dev, (const double*)e->d_scal,
                       e->h_scal_dev, (const pba_iteration_summary*)e->d_log, e->h_log_dev, (int)pba_engine::kMaxLog, h_seq_dev, seq);
    HIP_TRY(e, hipGetLastError());
    *seq_out = seq;
    return PBA_OK;
  }
  SchurParams sc = async_schur_params(e, kind, init_scale, o);
  if (kind == 1 && e->stamps) e->stamp_iter++;
  sc.stamp = (kind == 1) ? stamp_record(e) : nullptr;
  launch_schur(e, sc);
  SolveParams so = async_solve_params(e, kind, init_scale, o);
  // single rank: the final pass decides and flushes in its own last workgroup (no k_decide, no k_flush behind it)
  const bool fin_fused = kind == 2 && pba_internal_final_flushes(e);
  const unsigned long long seq = ++e->seq;
  const ReduceSolveParams::Fin fin = async_fin(e, seq);
  { const int rcs = launch_reduce_and_solve(e, so, n, cur, cand, e->d_lm, kind == 2 ? 1 : 0, e->fused_grid, fin_fused ? &fin : nullptr); if (rcs) return rcs; }
  if (fin_fused) { HIP_TRY(e, hipGetLastError()); *seq_out = seq; return PBA_OK; }
  unsigned long long fused_x = 0;      // exchange number of the step scalars when k_decide does the exchange itself
  if (kind == 1) {
    SampleParams sp = async_sample_params(e, 1);
    sp.decide = multi ? 0 : 1;
    sp.stamp = stamp_record(e);
    sp.seq = seq;
    if (multi) {
      const int rcx = set_sample_exchange(e, sp);
      if (rcx) return rcx;
      if (e->comm.peer) {
        // the exchange of the step scalars has no kernel of its own: the sampling kernel's last workgroup raises the flag,
        // k_decide waits for every rank's and sums the slots
        fused_x = ++e->comm.seq_b;
        sp.xchg = e->comm.mb_own + Comm::data_offset(1, fused_x);
        sp.xchg_flag = reinterpret_cast<unsigned long long*>(e->comm.mb_own) + Comm::flag_index(1, fused_x);
        sp.xchg_seq = fused_x;
      }
    }
    launch_sample<true, true>(e, sp);
    e->jac_passes++;
    HIP_TRY(e, hipGetLastError());
  }
  if (multi && !fused_x) {
    int rc2 = exchange_step_scalars(e, kind == 1);
    if (rc2) return rc2;
  }
  if (multi || kind == 2) {
    DecideParams dp{};
    if (fused_x) {
      dp.peer = peer_params(e); dp.peer_world = e->comm.world; dp.peer_flag = (int)Comm::flag_index(1, fused_x);
      dp.peer_off = (unsigned long long)Comm::data_offset(1, fused_x); dp.peer_seq = fused_x;
      dp.peer_timeout = (unsigned long long)(0.5 * e->wait_timeout_s * e->tick_hz); dp.peer_err = e->h_comm_err_dev;
    }
    dp.lm = e->d_lm; dp.host_state = e->h_lm_dev; dp.scal = e->d_scal; dp.host_scal = e->h_scal_dev; dp.log = e->d_log;
    dp.xchg = (multi && !fused_x) ? e->d_xchg : nullptr; dp.world = e->comm.world;
    dp.max_log = pba_engine::kMaxLog; dp.grad_only = (kind == 2) ? 1 : 0; dp.seq = seq;
    dp.host_seq = (kind == 1) ? nullptr : h_seq_dev;      // a full step is published by the next k_schur / k_flush
    hipLaunchKernelGGL(k_decide, dim3(1), dim3(64), 0, e->stream, dp);
  }
  HIP_TRY(e, hipGetLastError());
  *seq_out = seq;
  return PBA_OK;
}

int pba_internal_async_wait(pba_engine* e, unsigned long long seq) { return wait_published(e, seq, false); }

// ---- resident solve ------------------------------------------------------------------------------------------------

// A resident launch that left without publishing: one of its device-side waits timed out (a lost hand-over) and raised the abort word, which
// stays raised -- like every timed-out wait, this poisons the engine (later calls fail fast, pba_destroy does not wait for the stream).
void pba_internal_resident_failed(pba_engine* e) {
  e->poisoned = true;
  e->err += " -- the resident solve ended without publishing (a device-side wait timed out); the engine is unusable, destroy it";
}

void pba_internal_resident_done(pba_engine* e, int iterations) {
  e->res_epoch = e->res_epoch_launch + (unsigned)std::max(0, iterations) + 8u;
}

// PBA_RES_TRACE: phase intervals of the serial workgroup (100 MHz stamps), averaged over the steps of the last resident solve
void pba_internal_resident_trace(pba_engine* e, int iterations) {
  static const bool res_trace = getenv("PBA_RES_TRACE") != nullptr;
  if (!res_trace || !e->d_stamp || iterations < 1 || iterations + 2 > kStampMaxIters) return;
  std::vector<unsigned long long> st((size_t)kResStampRecord * (iterations + 2));
  if (hipMemcpyAsync(st.data(), e->d_stamp, sizeof(unsigned long long) * st.size(), hipMemcpyDeviceToHost, e->stream) != hipSuccess) return;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return;
  double d[5] = {0, 0, 0, 0, 0}, x[5] = {0, 0, 0, 0, 0};
  int n = 0;
  for (int r = 1; r <= iterations; ++r) {
    const unsigned long long* c = &st[(size_t)r * kResStampRecord];
    const unsigned long long prev = (r == 1) ? 0ull : st[(size_t)(r - 1) * kResStampRecord + kResStampDecided];
    if (!c[kResStampDecided] || !c[kResStampSchur]) continue;
    if (prev) d[0] += (double)(c[kResStampSchur] - prev);
    d[1] += (double)(c[kResStampReduced] - c[kResStampSchur]); d[2] += (double)(c[kResStampSolved] - c[kResStampReduced]);
    d[3] += (double)(c[kResStampSampled] - c[kResStampSolved]); d[4] += (double)(c[kResStampDecided] - c[kResStampSampled]);
    if (prev) x[0] += (double)(c[kResStampSchurBegin] - prev);
    x[1] += (double)(c[kResStampSchurBody] - c[kResStampSchurBegin]); x[2] += (double)(c[kResStampSchur] - c[kResStampSchurBody]);
    x[3] += (double)(c[kResStampGathered] - c[kResStampSampled]); x[4] += (double)(c[kResStampSampled] - c[kResStampSampleBegin]);
    ++n;
  }
  if (n > 1)
    std::fprintf(stderr, "resident solve, serial workgroup, us per step over %d steps: elimination %.2f | wait partials + reduce + wait reducers %.2f | solve %.2f | "
                         "back-substitution + sampling %.2f | wait cost partials + sum + decide %.2f | first linearisation + launch %.2f\n",
                 n, 0.01 * d[0] / (n - 1), 0.01 * d[1] / n, 0.01 * d[2] / n, 0.01 * d[3] / n, 0.01 * d[4] / n,
                 0.01 * (double)(st[kResStampRecord + kResStampSchur] - st[kResStampStart]));
  if (atoi(getenv("PBA_RES_TRACE")) >= 2 && e->d_dbg) {
    std::vector<unsigned long long> h(16 * (size_t)e->n_tiles);
    (void)hipMemcpyAsync(h.data(), e->d_dbg, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, e->stream);
    (void)hipStreamSynchronize(e->stream);
    double avg[12] = {0};
    for (int b = 0; b < e->n_tiles; ++b) for (int k = 0; k < 12; ++k) avg[k] += (double)h[16 * b + k] / e->n_tiles;
    std::fprintf(stderr, "   schur_body epilogue cycles: combine groups %.0f, camera sums out %.0f, pair blocks out %.0f, statistics %.0f\n", avg[8], avg[9], avg[10], avg[11]);
    std::fprintf(stderr, "   schur_body phase cycles per tile (100 MHz x ?: s_memtime): stage %.0f, P1 %.0f, point totals %.0f, P + camera record %.0f, camera sums %.0f, factors %.0f, pair blocks %.0f; tile loop %.2f us\n",
                 avg[0], avg[1], avg[2], avg[3], avg[4], avg[5], avg[6], 0.01 * avg[7]);
  }
  if (n > 1)
    std::fprintf(stderr, "   detail: decision -> elimination starts %.2f, schur_body %.2f, partial stores drained + flag %.2f | cost partials gathered %.2f | "
                         "sample_wg alone %.2f\n", 0.01 * x[0] / (n - 1), 0.01 * x[1] / n, 0.01 * x[2] / n, 0.01 * x[3] / n, 0.01 * x[4] / n);
}

// The window fits ONE resident round of 256-thread workgroups (two whole-point tiles each) and the solve is one the resident kernel
// covers: single rank, single channel, reference-exact sampler, free world points, patch radius <= 2, <= 8 free cameras.
int pba_internal_resident_capable(pba_engine* e, const pba_solver_options* o) {
  if (!e->use_resident || !e->use_async || !e->coop_launch || e->comm.multi() || e->channels != 1 || !fused_capable(e) || e->inverse_depth) return 0;
  if (e->cfg.radius > 2 || e->n_free < 1 || e->n_free > kSolveNarrowFree || keep_system(e) || e->solve_kind != 0 || e->profile || PBA_PHASE_TIMING) return 0;
  if (o->max_num_iterations >= pba_engine::kMaxLog - 2) return 0;
  const int groups = (e->n_tiles + 1) / 2;
  if (groups > kResMaxGroups || (e->part_stride + kReduceEntries - 1) / kReduceEntries + 1 > kResMaxReduce) return 0;
  int& gmax = e->res_groups_max[e->cfg.radius - 1][e->unit_weights ? 1 : 0];
  int& gn = e->res_groups_n[e->cfg.radius - 1][e->unit_weights ? 1 : 0];
  if (gmax < 0 || gn != e->n_free) {
    gmax = 0; gn = e->n_free;
    if (hipSetDevice(e->cfg.device) != hipSuccess) return 0;
    const void* fn = resident_kernel_for(e);
    const size_t pool = resident_pool_for(e);
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pool);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kResThreads, pool) == hipSuccess && per_cu > 0) gmax = per_cu * e->n_cus;
    (void)hipGetLastError();
  }
  return groups <= gmax ? 1 : 0;
}

int pba_internal_resident_launch(pba_engine* e, const pba_solver_options* o, unsigned long long* seq_out) {
  { const int rc0 = check_ready(e, "pba_solve"); if (rc0) return rc0; }
  PBA_ENTER(e);
  *e->h_lm = lm_initial_state(o, e->cur);
  __atomic_thread_fence(__ATOMIC_RELEASE);
  ResidentParams P{};
  P.frames = e->d_frames; P.desc = e->d_desc; P.w2 = e->d_w2; P.tile_info = e->d_tile_info; P.lane_rec = e->d_lane_rec;
  for (int k = 0; k < 2; ++k) {
    P.xyz[k] = e->d_xyz[k]; P.rec[k] = e->d_rec[k]; P.cams[k] = e->d_cams[k]; P.geom[k] = e->d_geom[k];
    P.block_cost[k] = e->d_block_cost[k]; P.block_fail[k] = e->d_block_fail[k];
  }
  P.sp = e->d_sp; P.ptrec = e->d_ptrec; P.delta_c = e->d_delta_c; P.sc = e->d_sc; P.packed = e->d_packed; P.partial = e->d_partial;
  P.scal = e->d_scal; P.block_bs = e->d_bs_out; P.tab = e->d_solve_tab; P.rec_stride = e->rec_stride;
  P.n_tiles = e->n_tiles; P.n_obs = e->n_obs; P.n_frames = e->n_frames; P.n_free = e->n_free; P.n_pairs = e->n_pairs;
  P.part_stride = e->part_stride; P.anchor_mask = e->anchor_mask; P.rows = e->cfg.rows; P.cols = e->cfg.cols; P.jacobi = o->jacobi_scaling;
  P.cur0 = e->cur; P.max_num_iterations = o->max_num_iterations;
  P.fx = e->cfg.fx; P.fy = e->cfg.fy; P.cx = e->cfg.cx; P.cy = e->cfg.cy; P.huber = e->cfg.huber;
  P.min_diag = o->min_lm_diagonal; P.max_diag = o->max_lm_diagonal; P.radius0 = o->initial_trust_region_radius;
  // epochs: one per step trip; the launch reserves max_num_iterations + 8 of them, pba_internal_resident_done hands back what the solve did not use
  // (the reference's 500-iteration limit against ~30 iterations actually taken: the 32-bit epochs then last ten times longer)
  // (32-bit epochs: a zeroed word would validate at epoch 0 and a stale one 2^32 epochs -- about a day of back-to-back solves -- later, so long
  // before the count wraps the block is zeroed again, stream-ordered behind the previous solve, and the count restarts)
  const unsigned need = (unsigned)std::max(0, o->max_num_iterations) + 8u;
  if (e->res_epoch > pba_engine::kResEpochLimit - need) {
    HIP_TRY(e, hipMemsetAsync(e->d_res_sync, 0, kResSyncBytes, e->stream));
    e->res_epoch = 1;
  }
  P.sync = e->d_res_sync; P.epoch0 = e->res_epoch;
  e->res_epoch_launch = e->res_epoch;
  e->res_epoch += need;
  // every device-side wait is bounded (a lost flag must not hang the GPU): well below the host watchdog and the compute-queue's own
  P.timeout_ticks = (unsigned long long)(std::min(2.0, 0.25 * e->wait_timeout_s) * e->tick_hz);
  P.lm_init = e->h_lm_dev; P.host_state = e->h_lm_dev; P.log = e->d_log; P.host_log = e->h_log_dev; P.max_log = (int)pba_engine::kMaxLog;
  P.host_scal = e->h_scal_dev; P.host_seq = host_seq_dev(e);
  const unsigned long long seq = ++e->seq;
  P.seq = seq;
  P.stamp = nullptr;
  if (const char* sv = getenv("PBA_RES_STOP")) P.debug_stop = atoi(sv);
  static const bool res_trace = getenv("PBA_RES_TRACE") != nullptr;      // dev aid: per-phase stamps of the serial workgroup, printed after the solve
  if (res_trace && o->max_num_iterations + 2 <= kStampMaxIters) {
    const int rcs = dev_alloc(e, &e->d_stamp, (size_t)(kStampMaxIters + 1) * kStampRecord);
    if (rcs) return rcs;
    HIP_TRY(e, hipMemsetAsync(e->d_stamp, 0, sizeof(unsigned long long) * kResStampRecord * (o->max_num_iterations + 2), e->stream));
    P.stamp = e->d_stamp;
    if (atoi(getenv("PBA_RES_TRACE")) >= 2) {
      { const int rcd = dev_alloc(e, &e->d_dbg, pba_engine::kDbgWords); if (rcd) return rcd; }
      P.schur_dbg = e->d_dbg;
    }
  }
  if (!P.stamp && e->stamps && e->d_stamp && o->max_num_iterations + 2 <= kStampMaxIters) {
    // pba_set_profiling(e, 2): the serial workgroup's phase stamps (the block holds kStampMaxIters + 1 records of kStampRecord words)
    static_assert((int)kResStampRecord <= (int)kStampRecord, "resident stamp records fit the block");
    HIP_TRY(e, hipMemsetAsync(e->d_stamp, 0, sizeof(unsigned long long) * kResStampRecord * (o->max_num_iterations + 2), e->stream));
    P.stamp = e->d_stamp;
  }
  const int groups = (e->n_tiles + 1) / 2;
  void* args[] = {&P};
  // A cooperative launch can be REFUSED by the runtime before anything runs (the grid does not fit the co-residency this process is
  // granted on this device: CU masks, partition modes, a queue limit).  That is not an error of the solve: the epochs and the sequence
  // number go back, this engine stays on the pipelined driver from here on and the caller runs the same solve there (same device
  // functions, same bits).  PBA_RES_REFUSE=1 injects the refusal (tests/test_gpu_resident.py).
  const char* inject = getenv("PBA_RES_REFUSE");
  const hipError_t le = (inject && atoi(inject) != 0) ? hipErrorCooperativeLaunchTooLarge
      : hipLaunchCooperativeKernel(resident_kernel_for(e), dim3(groups), dim3(kResThreads), args, (unsigned)resident_pool_for(e), e->stream);
  if (le != hipSuccess) {
    (void)hipGetLastError();
    e->res_epoch = e->res_epoch_launch;
    e->seq = seq - 1;
    e->use_resident = 0;
    std::fprintf(stderr, "[pba] cooperative launch of %d workgroups refused (%s): this engine solves on the pipelined driver from here on\n", groups,
                 hipGetErrorString(le));
    return PBA_INTERNAL_RESIDENT_REFUSED;
  }
  e->res_launches++;
  e->last_driver = 1;
  e->stamp_iter = o->max_num_iterations;
  e->cost_blocks[0] = e->cost_blocks[1] = groups;
  *seq_out = seq;
  return PBA_OK;
}

const void* pba_internal_async_state(const pba_engine* e) { return e->h_lm; }
const pba_iteration_summary* pba_internal_async_log(const pba_engine* e) { return e->h_log; }

// Leaves the engine in the state a synchronous solve would: current parity, valid linearisation.
int pba_internal_async_end(pba_engine* e) {
  // the host mirror was written by the last publishing kernel the caller waited for; kernels enqueued after a
  // termination are no-ops, so nothing behind it touches the state
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  { const int rcc = comm_failed(e); if (rcc) return rcc; }
  const LmState st = *e->h_lm;
  e->cur = st.cur;
  drop_lin(e, 1 - e->cur); e->lin_valid[e->cur] = true;
  e->have_lin = true;
  return PBA_OK;
}

void pba_internal_set_speculate(pba_engine* e, int on) {
  static const bool forced_off = [] { const char* sv = getenv("PBA_SPECULATE"); return sv && atoi(sv) == 0; }();
  e->speculate = on != 0 && !forced_off;
}
void pba_internal_pass_counts(const pba_engine* e, int64_t* jac, int64_t* cost) { *jac = e->jac_passes; *cost = e->cost_passes; }
void pba_internal_reset_pass_counts(pba_engine* e) { e->jac_passes = 0; e->cost_passes = 0; }
int pba_internal_allreduce_host(pba_engine* e, double* v, int n, int op) {
  if (!e->comm.multi()) return 0;
  return e->comm.allreduce_host(v, n, op);
}
}  // extern "C"

// ---- batched solves (pba_solve_batch: pba_lm.cpp drives, pba_batch.h computes) ------------------------------------------
namespace {
int batch_refuse(pba_engine* const* es, int i, int code, const char* fmt, ...) {
  char buf[400];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (es[0]) fail(es[0], code, "pba_solve_batch: engine %d: %s", i, buf);
  if (i >= 0 && es[i]) fail(es[i], code, "pba_solve_batch: engine %d: %s", i, buf);
  return code;
}

template <int R>
void launch_sample_batch_r(const pba_engine* e0, int grid, const BatchLaunch& L, hipStream_t st) {
  const dim3 block(kSampleWaves * 64);
  if (e0->channels > 1) {
    if (e0->unit_weights) hipLaunchKernelGGL((k_sample_mc_batch<R, true>), dim3(grid), block, 0, st, L);
    else hipLaunchKernelGGL((k_sample_mc_batch<R, false>), dim3(grid), block, 0, st, L);
  } else {
    if (e0->unit_weights) hipLaunchKernelGGL((k_sample_batch<R, true>), dim3(grid), block, 0, st, L);
    else hipLaunchKernelGGL((k_sample_batch<R, false>), dim3(grid), block, 0, st, L);
  }
}
void launch_sample_batch(const pba_engine* e0, int grid, const BatchLaunch& L, hipStream_t st) {
  switch (e0->cfg.radius) {
    case 1: launch_sample_batch_r<1>(e0, grid, L, st); break;
    case 2: launch_sample_batch_r<2>(e0, grid, L, st); break;
    case 3: launch_sample_batch_r<3>(e0, grid, L, st); break;
    case 4: launch_sample_batch_r<4>(e0, grid, L, st); break;
    default: launch_sample_batch_r<5>(e0, grid, L, st); break;
  }
}
}  // namespace

extern "C" {
// Every condition of pba_solve_batch (include/pba.h), checked before anything touches a device.
int pba_internal_batch_validate(pba_engine* const* es, int32_t n, const pba_solver_options* o) {
  if (!es || n < 1 || n > PBA_MAX_BATCH) return PBA_ERR_INVALID;
  for (int i = 0; i < n; ++i) if (!es[i]) return batch_refuse(es, i, PBA_ERR_INVALID, "the engine is null");
  const pba_engine* e0 = es[0];
  for (int i = 0; i < n; ++i) {
    pba_engine* e = es[i];
    for (int j = 0; j < i; ++j)
      if (es[j] == e) return batch_refuse(es, i, PBA_ERR_INVALID, "the same engine as index %d (every window appears once)", j);
    if (e->cfg.device != e0->cfg.device) return batch_refuse(es, i, PBA_ERR_INVALID, "on device %d, the batch is on device %d", e->cfg.device, e0->cfg.device);
    if (e->poisoned) return batch_refuse(es, i, PBA_ERR_STATE, "the engine is unusable after a timed-out step; destroy it");
    if (check_ready(e, "pba_solve_batch")) return batch_refuse(es, i, PBA_ERR_STATE, "%s", e->err.c_str());
    static_assert(kWideMinFree <= kMaxFrames, "more free cameras than a batch takes (kMaxFrames - 1) make a wide window");
    unsigned with = 0;      // (an engine with any transport counts as multi-rank here)
    const char* why = mode_conflict(modes_present(e, e->comm.kind != 0 || e->comm.multi()), kModeBatch, &with);
    if (why && with == kModeWide) return batch_refuse(es, i, PBA_ERR_INVALID, "%s (%d free cameras, a batch takes <= %d)", why, e->n_free, kMaxFrames - 1);
    if (why) return batch_refuse(es, i, PBA_ERR_INVALID, "%s", why);
    if (e->profile || e->stamps) return batch_refuse(es, i, PBA_ERR_INVALID, "profiling is on (pba_set_profiling / pba_reset_counters)");
    if (!pba_internal_async_capable(e, &o[i]) || e->solve_kind != 0)
      return batch_refuse(es, i, PBA_ERR_INVALID, "the options or the environment need the host-stepped driver (max_num_iterations %d)", o[i].max_num_iterations);
    if (e->cfg.radius != e0->cfg.radius) return batch_refuse(es, i, PBA_ERR_INVALID, "patch radius %d, engine 0 has %d (one kernel key per batch)", e->cfg.radius, e0->cfg.radius);
    if (e->channels != e0->channels) return batch_refuse(es, i, PBA_ERR_INVALID, "%d channels, engine 0 has %d (one kernel key per batch)", e->channels, e0->channels);
    if (e->unit_weights != e0->unit_weights)
      return batch_refuse(es, i, PBA_ERR_INVALID, "%s patch weights, engine 0 has %s (one kernel key per batch)", e->unit_weights ? "unit" : "Gaussian", e0->unit_weights ? "unit" : "Gaussian");
    if (e->n_tiles < 1 || e->n_free < 1) return batch_refuse(es, i, PBA_ERR_INVALID, "empty window (%d observations, %d free cameras)", e->n_obs, e->n_free);
    if ((double)e->n_obs * pba_internal_patch_len(e) > 2147483647.0)
      return batch_refuse(es, i, PBA_ERR_INVALID, "%d residual blocks x %d residuals exceed the int32 range of the summary", e->n_obs, pba_internal_patch_len(e));
  }
  return PBA_OK;
}

// Orders every engine's own stream in front of the batch stream (engine 0's), lends that stream to every engine, begins every window's
// solve (pba_internal_async_begin) and uploads the window table.
int pba_internal_batch_begin(pba_engine* const* es, int32_t n, const pba_solver_options* o) {
  pba_engine* e0 = es[0];
  HIP_TRY(e0, hipSetDevice(e0->cfg.device));
  hipStream_t bs = e0->stream;
  for (int i = 1; i < n; ++i) {
    HIP_TRY(e0, hipEventRecord(es[i]->ev_xdep, es[i]->stream));
    HIP_TRY(e0, hipStreamWaitEvent(bs, es[i]->ev_xdep, 0));
  }
  for (int i = 0; i < n; ++i) { es[i]->stream_own = es[i]->stream; es[i]->stream = bs; }
  if (const int rc = host_alloc(e0, &e0->h_batch, (size_t)PBA_MAX_BATCH)) return rc;      // the window table and its staging: on the first batch
  if (const int rc = dev_alloc(e0, &e0->d_batch, (size_t)PBA_MAX_BATCH)) return rc;
  for (int i = 0; i < n; ++i) {
    pba_engine* e = es[i];
    const int rc = pba_internal_async_begin(e, &o[i]);
    if (rc) return batch_refuse(es, i, rc, "%s", e->err.c_str());
    const int cur = e->async_cur, cand = 1 - cur, nn = 6 * e->n_free;
    e->batch_init2 = o[i].max_num_iterations <= 0 ? 1 : 0;
    BatchWindow& bw = e0->h_batch[i];
    bw = BatchWindow{};
    bw.sample[0] = async_sample_params(e, 0);
    bw.sample[1] = async_sample_params(e, 1);
    bw.schur[0] = async_schur_params(e, 1, 0, &o[i]);
    bw.schur[1] = async_schur_params(e, 2, e->batch_init2, &o[i]);
    bw.rsolve[0] = reduce_solve_params(e, async_solve_params(e, 1, 0, &o[i]), nn, cur, cand, e->d_lm, 0, e->fused_grid, nullptr);
    const ReduceSolveParams::Fin fin = async_fin(e, 0);      // (the sequence number travels with the launch)
    bw.rsolve[1] = reduce_solve_params(e, async_solve_params(e, 2, e->batch_init2, &o[i]), nn, cur, cand, e->d_lm, 1, e->fused_grid, &fin);
    bw.frames_mc = e->channels > 1 ? e->d_frames_mc : nullptr;
    bw.channels = e->channels;
  }
  HIP_TRY(e0, hipMemcpyAsync(e0->d_batch, e0->h_batch, sizeof(BatchWindow) * n, hipMemcpyHostToDevice, bs));
  return PBA_OK;
}

// One batched pass of `kind` (0: first linearisation; 1: full iteration; 2: the final gradient-only pass, which decides and flushes) over
// the windows sel[0..n_sel) -- indices into es -- in one launch per phase.  seq_out[k]: the sequence number of window sel[k]'s enqueue.
int pba_internal_batch_enqueue(pba_engine* const* es, const int32_t* sel, int32_t n_sel, int kind, int init_scale, unsigned long long* seq_out) {
  pba_engine* e0 = es[0];
  if (n_sel < 1) return PBA_OK;
  hipStream_t bs = e0->stream;
  BatchLaunch L{};
  L.tab = e0->d_batch;
  L.n = n_sel;
  int g_schur = 0, g_red = 0, g_sample = 0;
  size_t lds = 0;
  for (int k = 0; k < n_sel; ++k) {
    pba_engine* e = es[sel[k]];
    L.win[k] = (uint8_t)sel[k];
    const int init = kind == 2 ? e->batch_init2 : init_scale;
    L.mode[k] = (uint8_t)((kind == 2 ? 1 : 0) | (init ? 2 : 0));
    if (kind == 0) { seq_out[k] = 0; e->jac_passes++; e->cost_blocks[0] = e->cost_blocks[1] = e->fused_grid; }
    else { L.seq[k] = seq_out[k] = ++e->seq; if (kind == 1) e->jac_passes++; }
    lds = std::max(lds, solve_blocked_smem_bytes(6 * e->n_free));
  }
  auto grids = [&](auto grid_of) {
    int g = 0;
    for (int k = 0; k < n_sel; ++k) { L.begin[k] = g; g += grid_of(es[sel[k]]); }
    L.begin[n_sel] = g;
    return g;
  };
  if (kind != 0) {
    g_schur = grids([](const pba_engine* e) { return e->schur_grid; });
    hipLaunchKernelGGL(k_schur_batch, dim3(g_schur), dim3(kTile), 0, bs, L);
    g_red = grids([](const pba_engine* e) { return reduce_grid(e); });
    hipLaunchKernelGGL(k_reduce_solve_batch, dim3(g_red), dim3(kReduceThreads), lds, bs, L);
  }
  if (kind != 2) {
    if (kind == 1) for (int k = 0; k < n_sel; ++k) L.mode[k] = 1;     // sampling variant 1: the candidate pass
    g_sample = grids([](const pba_engine* e) { return e->fused_grid; });
    launch_sample_batch(e0, g_sample, L, bs);
  }
  HIP_TRY(e0, hipGetLastError());
  return PBA_OK;
}

// Gives every engine its own stream back, ordered behind the batch; after a timed-out wait (one engine poisoned) every engine of the batch
// is poisoned: they all share the stalled stream.
void pba_internal_batch_end(pba_engine* const* es, int32_t n, int failed) {
  pba_engine* e0 = es[0];
  int bad = -1;
  for (int i = 0; i < n; ++i) if (es[i]->poisoned) bad = i;
  for (int i = 0; i < n; ++i) {
    if (es[i]->stream_own) es[i]->stream = es[i]->stream_own;
    es[i]->stream_own = nullptr;
  }
  if (bad >= 0) {
    for (int i = 0; i < n; ++i) {
      if (!es[i]->poisoned) {
        es[i]->poisoned = true;
        es[i]->err = "pba_solve_batch: a wait of engine " + std::to_string(bad) + " of the batch timed out; the engine is unusable, destroy it";
      }
    }
    return;
  }
  // (a batch that failed part-way drains the stream: the pinned table staging may still be read by its copy)
  if (failed) (void)hipStreamSynchronize(e0->stream);
  (void)hipEventRecord(e0->ev_xdep, e0->stream);
  for (int i = 0; i < n; ++i) {
    if (i > 0) (void)hipStreamWaitEvent(es[i]->stream, e0->ev_xdep, 0);
    if (!failed) es[i]->last_driver = 4;
  }
}
}  // extern "C"
