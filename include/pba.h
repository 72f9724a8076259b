/*
 * pba.h -- C-ABI of the MI355X photometric bundle-adjustment engine (libpba_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path the engine replaces: the inner seam of
 * PhotometricBundleAdjustment::optimize(), reference src/photobundle.cc:784-829, i.e.
 *
 *     ceres::Problem problem;                                            (:784)
 *     problem.AddResidualBlock(DescriptorError::Create(...), loss, camera_ptr, xyz);   (:801-802)
 *     problem.SetParameterBlockConstant(first_camera);                   (:809-813)
 *     ceres::Solve(GetSolverOptions(...), &problem, &summary);           (:829)
 *
 * plus the per-frame plane producer feeding it (DescriptorFrame, :151-257 / imgproc.cc:27-95).
 * Everything is `extern "C"`, plain pointers and sizes, no C++/torch types.  Functions return 0 on
 * success or a negative pba_status; they never throw.  All host buffers are caller-owned and are
 * only read/written during the call; all device memory is engine-owned.  One host thread per handle.
 *
 * Data conventions (identical to what the reference hands to Ceres):
 *   cameras  : 6 doubles per window slot = angle-axis (3) + translation (3) of the WORLD->CAMERA
 *              transform (photobundle.cc:646-656 PoseToParams of the inverted pose, :774-778)
 *   points   : 3 doubles, world XYZ (photobundle.cc:795)
 *   desc     : C (2R+1)^2 doubles per point: the row-major patch of every channel, channel-major (photobundle.cc:466-479,
 *              :597-603); values are float casts of pixels, stored as fp32 on the device
 *   obs      : one residual block per (point, slot) entry, grouped by point (photobundle.cc:791-804)
 *   weights  : (2R+1)^2 doubles (photobundle.cc:617-644)
 */
#ifndef PBA_H
#define PBA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBA_MAX_FRAMES 32
#define PBA_MAX_RADIUS 5
#define PBA_MAX_CHANNELS 8

typedef struct pba_engine pba_engine;

typedef enum pba_status {
  PBA_OK = 0,
  PBA_ERR_INVALID = -1,     /* bad argument */
  PBA_ERR_HIP = -2,         /* HIP runtime error (see pba_last_error) */
  PBA_ERR_NO_DEVICE = -3,   /* no gfx950 device visible: there is NO CPU fallback */
  PBA_ERR_STATE = -4,       /* call order violated (e.g. solve before set_problem) */
  PBA_ERR_COMM = -5,        /* collective transport error */
  PBA_ERR_NUMERIC = -6      /* non-finite evaluation at the initial point; pba_covariance: singular normal matrix */
} pba_status;

/* Replaces the constructor arguments of PhotometricBundleAdjustment (photobundle.h:148) that matter on the
 * hot path: Calibration (calibration.h:19-26), ImageSize (types.h:57-63), Options::patchRadius /
 * slidingWindowSize / robustThreshold (photobundle.h:26-85). */
typedef struct pba_config {
  int32_t rows, cols;        /* image size */
  int32_t max_frames;        /* window slots (Options::slidingWindowSize), 2..PBA_MAX_FRAMES (32) */
  int32_t radius;            /* Options::patchRadius, 1..PBA_MAX_RADIUS */
  double fx, fy, cx, cy;     /* pinhole intrinsics */
  double huber;              /* Options::robustThreshold; <= 0 disables the loss (photobundle.cc:797-798) */
  int32_t device;            /* HIP device ordinal */
  int32_t flags;             /* bit 0: keep a copy of the reduced system for pba_get_reduced_system (test hook);
                              * bits 1-2: sampler precision for the BASELINE configs[4] tolerance sweep: 0 = exact
                              * restatement of sample_eigen.h:82-101 (default, the only mode with reference parity),
                              * 1 = fp32 interpolation and accumulation, 2 = fp32 with bf16-rounded residual/gradient
                              * operands.  Modes 1-2 need unit patch weights. */
  int32_t channels;          /* descriptor channels C (Options::descriptorType, photobundle.cc:229-245): 0 or 1 =
                              * Intensity (frames arrive as u8 through pba_set_frame_u8); 2..PBA_MAX_CHANNELS = float
                              * channel images through pba_set_frame_channels_f32 (IntensityAndGradient: 3, BitPlanes: 8).
                              * Descriptors then hold C patches per point, channel-major (photobundle.cc:597-603). */
  int32_t reserved;
} pba_config;

/* ceres::Solver::Options as configured by GetSolverOptions (photobundle.cc:738-761) + the Ceres defaults
 * that shape the path.  pba_default_solver_options fills the reference's values. */
typedef struct pba_solver_options {
  int32_t max_num_iterations;            /* 500  (photobundle.cc:751) */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  double function_tolerance;             /* 1e-6 (photobundle.cc:756) */
  double gradient_tolerance;             /* 1e-6 (:757) */
  double parameter_tolerance;            /* 1e-6 (:758) */
  double initial_trust_region_radius;    /* 1e4  */
  double max_trust_region_radius;        /* 1e16 */
  double min_trust_region_radius;        /* 1e-32 */
  double min_relative_decrease;          /* 1e-3 */
  double min_lm_diagonal;                /* 1e-6 */
  double max_lm_diagonal;                /* 1e32 */
  int32_t jacobi_scaling;                /* 1 */
  int32_t verbose;                       /* minimizer_progress_to_stdout (photobundle.cc:750) */
} pba_solver_options;

/* ceres::IterationSummary: the 18 fields the reference serialises (ceres_cereal.h:13-30), same names. */
typedef struct pba_iteration_summary {
  int32_t iteration;
  int32_t step_is_valid;
  int32_t step_is_nonmonotonic;
  int32_t step_is_successful;
  double cost;
  double cost_change;
  double gradient_max_norm;
  double gradient_norm;
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
  double eta;
  double step_size;
  int32_t line_search_function_evaluations;
  int32_t line_search_gradient_evaluations;
  int32_t line_search_iterations;
  int32_t linear_solver_iterations;
  double iteration_time_in_seconds;
  double step_solver_time_in_seconds;
  double cumulative_time_in_seconds;
  double model_cost_change;   /* extra (parity debugging) */
  double candidate_cost;      /* extra */
} pba_iteration_summary;

/* ceres::Solver::Summary subset consumed at photobundle.cc:867-874. */
typedef struct pba_solver_summary {
  double initial_cost, final_cost, fixed_cost;
  int32_t num_successful_steps, num_unsuccessful_steps;
  int32_t num_iterations;            /* entries written to the iterations array */
  int32_t num_residuals;             /* global (all ranks) */
  int32_t num_residual_blocks;       /* global (all ranks) */
  int32_t termination_type;          /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE */
  double total_time_in_seconds;
  int64_t num_jacobian_passes;       /* linearisations (residual + Jacobian) */
  int64_t num_cost_passes;           /* candidate (residual-only) evaluations */
  int64_t num_resolve_passes;        /* extra damped Schur solves after rejected / invalid steps.  Driver-dependent: the device
                                      * drivers report num_unsuccessful_steps; the host-stepped driver counts the re-solves it
                                      * actually ran.  The two can differ by one where the solve ends */
  char message[256];
} pba_solver_summary;

/* Output of one trust-region step attempt (pba_step). */
typedef struct pba_step_info {
  double cost;               /* cost at the current linearisation point */
  double gradient_max_norm;  /* |J^T r|_inf at the current point (unscaled) */
  double gradient_norm;
  double model_cost_change;
  double step_norm;          /* |delta| unscaled */
  double x_norm;             /* |x| over the free cameras that have residual blocks and all points, at the current point */
  double candidate_cost;
  int32_t linear_solver_ok;  /* 0: LINEAR_SOLVER_FAILURE (non-PD block / non-finite step) */
  int32_t eval_ok;           /* 0: candidate evaluation non-finite */
} pba_step_info;

/* Device-side accounting for bench.py / rocprof cross-checks. */
typedef struct pba_counters {
  double linearize_ms;       /* sum of HIP-event durations of the Jacobian-pass kernel on the engine stream */
  double cost_ms;            /* ... of the cost-pass kernel */
  double schur_ms;           /* ... of the Schur elimination kernel */
  int64_t linearize_launches, cost_launches, schur_launches;
  int64_t n_obs, n_points;   /* local shard */
  double solve_ms;           /* ... of the reduction of the Schur partials + reduced camera solve (k_reduce_solve, or k_reduce_final
                                + k_solve_blocked at more than one rank, without the exchange between them) */
  double exchange_ms;        /* ... of the two per-step exchanges (all-reduce of the packed reduced system + of the step scalars):
                                RCCL collectives or the peer-exchange kernels; 0 at a single rank */
  int64_t solve_launches, exchange_launches;
} pba_counters;

const char* pba_status_string(int status);
const char* pba_last_error(const pba_engine* e);
void pba_default_solver_options(pba_solver_options* o);

/* ---- lifetime ------------------------------------------------------------------------------------------ */
/* Allocates the device state for cfg->max_frames frames of cfg->rows x cfg->cols, loads the library's code object and
 * runs one frame-sized host -> device transfer, so that the first pba_set_frame_* / pba_solve of a process see the
 * steady-state latency (the runtime's lazy set-up costs ~10 ms each otherwise).  ~30 ms. */
int pba_create(const pba_config* cfg, pba_engine** out);
void pba_destroy(pba_engine* e);

/* ---- frames: replaces DescriptorFrame::Create + ImageGradient::compute (photobundle.cc:225-248, :126-135) --
 * `image` is the dense row-major rows x cols u8 frame addFrame() receives (photobundle.h:160).  The engine
 * builds its device plane (I, Gx, Gy bit-exactly as imgproc.cc:27-95) and keeps it in window slot `slot`.
 * A frame is an input of the linearisation like the problem and the cameras: every pba_set_frame_* call (_u8, _channels_f32,
 * _descriptor_u8, _pyr_down into `e`) drops the engine's linearisation and what was reduced from it.  The next pba_linearize /
 * pba_covariance / pba_solve samples again; pba_step and pba_accept want a pba_linearize first (PBA_ERR_STATE otherwise). */
int pba_set_frame_u8(pba_engine* e, int slot, const uint8_t* image);
/* Multi-channel descriptors (pba_config.channels = C > 1): `channels` holds the C float channel images DescriptorFrame::
 * Create produces (photobundle.cc:225-248), [C][rows*cols] row-major; the engine adds every channel's own gradient
 * images (DescriptorFrame ctor :172-175, imgproc.cc:27-95).  Drops the linearisation, as pba_set_frame_u8 does. */
int pba_set_frame_channels_f32(pba_engine* e, int slot, int32_t n_channels, const float* channels);
/* Debug/test readback of the device planes as float I, Gx, Gy (each rows*cols). */
int pba_get_frame_planes(pba_engine* e, int slot, float* I, float* Gx, float* Gy);
/* ... and of channel `channel` of a multi-channel slot: value, Gx, Gy (each rows*cols). */
int pba_get_frame_channel(pba_engine* e, int slot, int32_t channel, float* I, float* Gx, float* Gy);
/* Debug/test: the engine's sampler (SampleLinear, sample_eigen.h:56-102, in the reference's mixed float/double arithmetic)
 * at n float positions (y[i], x[i]) of channel `channel` (0 on a single-channel engine) of the frame in `slot`;
 * out3[3 i .. 3 i + 2] = value, Gx, Gy. */
int pba_sample_frame(pba_engine* e, int slot, int32_t channel, int32_t n, const float* y, const float* x, float* out3);

/* ---- device-side producers (round 3): the channel images and the pyramid without the host round trip --------------
 * pba_set_frame_descriptor_u8: DescriptorFrame::Create on the device (photobundle.cc:225-248).  `descriptor` selects
 * the channels built from the u8 frame: PBA_DESCRIPTOR_INTENSITY (= pba_set_frame_u8), _INTENSITY_AND_GRADIENT (I, Gx,
 * Gy as float: photobundle.cc:229-235, imgproc.cc:27-95; engine created with channels = 3), _BITPLANES (census of the
 * 3x3-smoothed frame, its eight bit planes smoothed 5x5: imgproc.cc:109-245 with sigma_ct / sigma_bp of imgproc.h:44-46,
 * <= 0 skips the smoothing; channels = 8).  Bit-identical to pba_set_frame_channels_f32 fed with the host's channel images
 * (photobundle_amd/host/imgproc.h), at 1/12 .. 1/32 of the upload.  Drops the linearisation, as pba_set_frame_u8 does. */
enum { PBA_DESCRIPTOR_INTENSITY = 0, PBA_DESCRIPTOR_INTENSITY_AND_GRADIENT = 1, PBA_DESCRIPTOR_BITPLANES = 2 };
int pba_set_frame_descriptor_u8(pba_engine* e, int slot, const uint8_t* image, int32_t descriptor, float sigma_ct, float sigma_bp);
/* The channel images of a multi-channel slot back on the host, [C][rows*cols] (the layout pba_set_frame_channels_f32
 * takes): a front-end that needs them (saliency over all channels, descriptor patches: photobundle.cc:213-221, :466-479)
 * reads the device-produced ones instead of running DescriptorFrame::Create on the CPU as well. */
int pba_get_frame_channels_f32(pba_engine* e, int slot, float* channels);
/* cv::pyrDown of the frame in slot `finer_slot` of engine `finer` into slot `slot` of `e` (photobundle_pyramid.cc:45-52:
 * the next pyramid level; `e` must have been created for ((rows+1)/2, (cols+1)/2) on the same device), device to device.
 * `image_out` (nullable, (rows+1)/2 * (cols+1)/2 bytes) receives the down-sampled frame for the host front-end; the
 * call is asynchronous when it is null.  The depth map never enters the engine (it only initialises points on the host,
 * photobundle.cc:540-560), so cv::resize of the depth (:54-56) stays with the caller.  Drops the linearisation of `e` (not of
 * `finer`), as pba_set_frame_u8 does. */
int pba_set_frame_pyr_down(pba_engine* e, int slot, pba_engine* finer, int finer_slot, uint8_t* image_out);

/* ---- device front-end (round 4): the per-frame work of PhotometricBundleAdjustment::addFrame on the frame that already sits in
 * the engine (reference src/photobundle.cc:505-603), so that neither the float planes nor the channel images travel back:
 *   pba_frontend_visibility   ZNCC test of the tracked points (ZnccPatch_<2, float>, :315-361, :512-542) on the u8 frame MOST
 *                             RECENTLY handed to pba_set_frame_u8 / pba_set_frame_descriptor_u8 (or produced by
 *                             pba_set_frame_pyr_down).  uv [n][2]: projections K (T_c X) of the points the caller already found
 *                             inside the border (:519-523), rc [n][2]: their rounded (row, column), patches [n][26]: the stored
 *                             zero-mean 5x5 patch and its norm.  hit[i] = score > min_score; the (2 mask_radius + 1)^2 block around
 *                             every hit leaves the engine's selection mask (:536-538), which the call first resets.  n may be 0.
 *                             PBA_ERR_STATE when the frame uploaded last left no u8 image behind (pba_set_frame_channels_f32, or no
 *                             upload at all): the ZNCC would otherwise score a stale image.
 *   pba_frontend_candidates   saliency map of the frame in `slot` (sum over the channels of |Ix| + |Iy|, :213-221), then every pixel
 *                             of [border, rows - border - 1) x [border, cols - border - 1) with min_depth <= depth <= max_depth
 *                             that is unmasked and a STRICT local maximum of the saliency over (2 nms_radius + 1)^2 (:555-573,
 *                             src/imgproc.h:176-212; nms_radius <= 0: every valid-depth pixel).  depth: rows * cols floats of the
 *                             caller (borrowed for the call).  *n_out = number of candidates, kept on the device in the row-major
 *                             order of the reference's scan; PBA_ERR_INVALID for nms_radius > border or a border that leaves no
 *                             interior (2 border >= rows or cols);
 *   pba_frontend_get_candidates   copies the first n of them out (the caller selects the maxNumPoints most salient, :578-585);
 *   pba_frontend_descriptors  ExtractPatch (:466-479, :597-603) at n integer pixels xy [n][2] = (x, y): desc [n][C][(2 R + 1)^2]
 *                             channel values as float (exact: the reference stores the same floats widened to double).
 * Same arithmetic, type by type and in the same order, as the host restatement in photobundle_amd/host/photobundle.cc: the
 * class produces byte-identical trajectories with either (PBA_HOST_FRONTEND=1 selects the host one). */
typedef struct pba_candidate { float saliency; int32_t x, y; } pba_candidate;
int pba_frontend_visibility(pba_engine* e, int32_t n, const double* uv, const int32_t* rc, const float* patches26, double min_score,
                            int32_t mask_radius, uint8_t* hit);
int pba_frontend_candidates(pba_engine* e, int32_t slot, const float* depth, double min_depth, double max_depth, int32_t nms_radius,
                            int32_t border, int32_t* n_out);
int pba_frontend_get_candidates(pba_engine* e, pba_candidate* out, int32_t n);
int pba_frontend_descriptors(pba_engine* e, int32_t slot, int32_t n, const int32_t* xy, float* desc);
/* Test hook: what pba_frontend_visibility computes for point i, out27[27 i ..] = the zero-mean patch of the new frame at uv (25),
 * its norm, the score against patches26[i] (-1 when the product of the norms is <= 1e-6).  No mask, no flags. */
int pba_frontend_zncc_probe(pba_engine* e, int32_t n, const double* uv, const float* patches26, float* out27);

/* ---- problem: replaces the AddResidualBlock loop (photobundle.cc:786-806) -------------------------------
 * Call order: pba_set_frame_u8 (every slot the observation list uses), pba_set_problem and pba_set_cameras may come in
 * any order, all three before pba_linearize / pba_solve; a pass that finds one of them missing, an observation whose
 * slot is >= n_frames, or a slot without an uploaded frame returns PBA_ERR_STATE (nothing is launched).
 * Limit: at most 32 slots (n_frames <= max_frames <= PBA_MAX_FRAMES).  The window shape picks the path at pba_set_cameras /
 * pba_set_cameras_anchored: a window of at most 16 slots with at most 15 free cameras runs the narrow kernels and drivers, one
 * with more slots or with 16 to 32 free cameras the wide chain (host-stepped driver).
 * A wide window refuses the multi-rank transports (pba_comm_*), the inverse-depth mode and the precision-sweep flags:
 * PBA_ERR_INVALID with a message in pba_last_error, whichever of the calls comes second.
 * pba_set_points_constant (after pba_set_problem, before or after pba_set_cameras / pba_set_inverse_depth) turns the passes
 * below into the pose-only problem; pba_set_problem switches it off again. */
int pba_set_problem(pba_engine* e, int32_t n_points, const double* xyz, const double* desc,
                    int32_t n_obs, const int32_t* obs_point, const int32_t* obs_slot, const double* weights);
/* cams6: [n_frames][6]; fixed_slot: SetParameterBlockConstant (photobundle.cc:809-813), -1 for none. */
int pba_set_cameras(pba_engine* e, const double* cams6, int32_t n_frames, int32_t fixed_slot);
/* Any set of constant cameras (anchor frames of a local bundle adjustment).  Bit c of anchor_mask set: slot c is constant, the Ceres
 * call SetParameterBlockConstant on that camera block.  pba_set_cameras(e, cams6, n, fixed_slot) IS this call with
 * anchor_mask = fixed_slot < 0 ? 0 : 1u << fixed_slot: same launches, same bits, on every driver.  Semantics are Ceres' for the reduced
 * program.  Full mode: the camera columns are the slots outside the mask in ascending slot order (pba_get_reduced_system returns
 * n = 6 x the number of free slots); every residual block stays, because each depends on a free point, and a constant camera's blocks
 * still feed the point blocks; summary.fixed_cost = 0; gradient norms, step_norm and x_norm run over the free cameras that have
 * residual blocks and over all points.  Anchored cameras are never written: pba_get_state returns them byte for byte as set.
 * Pose-only mode (pba_set_points_constant): the blocks of every anchored camera leave the program, summary.fixed_cost is their
 * loss-corrected cost summed in ascending slot order, the counts are the program's.  Structure-only mode (pba_set_cameras_constant):
 * the mask has no effect.  The inverse-depth mode and pba_solve_batch take anchored narrow windows.
 * PBA_ERR_INVALID with a message in pba_last_error: bits at or above n_frames; in the full mode a mask that covers every slot (use
 * pba_set_cameras_constant), whichever of this call and the switch back from a constant mode comes second -- such a mask is legal
 * while a constant mode is on, and a pba_set_problem that ends the mode under it makes the passes return PBA_ERR_STATE until the
 * cameras are set again; a mask of two or more bits together with a multi-rank transport (pba_comm_*) or the precision-sweep flags,
 * whichever call comes second.  After a refused call the engine holds what it held before. */
int pba_set_cameras_anchored(pba_engine* e, const double* cams6, int32_t n_frames, uint32_t anchor_mask);
/* Inverse-depth variant of the point parameterisation (named by the project's north star; the REFERENCE optimises free
 * world points, photobundle.cc:692/:795, so this mode has no reference counterpart and is outside every parity claim).
 * Call after pba_set_problem: point i then lives on the fixed world ray rays6[i] = {origin (3), direction (3)} with the
 * single free parameter rho[i] > 0, X_i = origin + direction / rho_i.  pba_get_state afterwards returns the parameters
 * (rho, 0, 0) in `xyz`; pba_get_points_world returns world coordinates in either mode.  pba_set_problem switches the
 * mode off again. */
int pba_set_inverse_depth(pba_engine* e, const double* rays6, const double* rho);
int pba_get_points_world(pba_engine* e, double* xyz);
/* Pose-only solves.  Ceres: SetParameterBlockConstant on every point block.  on != 0: pba_linearize / pba_step / pba_accept / pba_solve
 * treat every point as constant; cameras outside the anchor mask (other than fixed_slot) stay free.  Call after pba_set_problem; pba_set_problem switches it off
 * again (as it does for inverse depth).  Semantics are Ceres' for the reduced program: its parameter blocks are the free cameras that
 * have at least one residual block; the residual blocks of the constant cameras leave the program and their loss-corrected cost is
 * summary.fixed_cost (initial_cost and final_cost include it; the per-iteration cost, num_residual_blocks and num_residuals count the
 * program only; pba_linearize's cost stays the sum over ALL residual blocks).  The normal equations are block diagonal, one 6x6 block
 * per free camera solved by an exact Cholesky, at every window shape (2..32 slots); gradient norms, step_norm, x_norm and
 * model_cost_change run over the program's camera columns.  pba_get_state / pba_get_points_world return the points byte for byte as
 * set; pba_get_reduced_system returns the block-diagonal system in the dense n x n layout.  pba_solve runs the host-stepped driver and
 * returns PBA_ERR_INVALID before any launch when no free camera has a residual block.  Refused with PBA_ERR_INVALID and a message,
 * whichever call comes second: the multi-rank transports, the precision-sweep flags, pba_solve_batch with such an engine (and, on
 * windows of 16..32 free cameras, what pba_set_cameras refuses there).  Switched off again the engine solves as a fresh one does. */
int pba_set_points_constant(pba_engine* e, int32_t on);
/* Structure-only solves.  Ceres: SetParameterBlockConstant on every camera block.  on != 0: pba_linearize / pba_step / pba_accept /
 * pba_solve treat every camera as constant and refine the points against them; fixed_slot of pba_set_cameras (the anchor mask) has no effect.  Call
 * order and lifetime are pba_set_points_constant's.  Semantics are Ceres' for the reduced program: its parameter blocks are the points,
 * every residual block stays in it (summary.fixed_cost = 0, num_residual_blocks and num_residuals count every block).  The normal
 * equations are block diagonal, one 3x3 block per point (1x1 in the inverse-depth mode) solved by an exact Cholesky, at every window
 * shape (2..32 slots); a non-positive pivot or a non-finite step in any block gives linear_solver_ok = 0 and a zero step everywhere.
 * Gradient norms, step_norm, x_norm and model_cost_change run over the point columns.  The cameras are never written: pba_get_state
 * returns them byte for byte as set.  pba_solve runs the host-stepped driver.  pba_get_reduced_system returns PBA_ERR_STATE in the mode
 * (there is no reduced camera system).  Refused with PBA_ERR_INVALID and a message, whichever call comes second: both constant modes at
 * once (the program would be empty), the multi-rank transports, the precision-sweep flags, pba_solve_batch with such an engine (and, on
 * windows of 16..32 free cameras, what pba_set_cameras refuses there).  Switched off again the engine solves as a fresh one does. */
int pba_set_cameras_constant(pba_engine* e, int32_t on);
/* Current (best) state; either pointer may be NULL. */
int pba_get_state(pba_engine* e, double* cams6, double* xyz);

/* ---- primitive passes used by the host LM driver (exposed for tests and alternative drivers) ------------- */
/* Jacobian pass at the current point: residuals, analytic per-patch structure tensors, loss correction. */
int pba_linearize(pba_engine* e, double* cost);
/* Damped Schur solve with trust-region `radius` from the stored linearisation, back-substitution, candidate
 * point and its cost (cost pass).  init_scale != 0 (iteration 0) also fixes the Jacobi scaling vector. */
int pba_step(pba_engine* e, double radius, int32_t init_scale, const pba_solver_options* o, pba_step_info* out);
/* Make the candidate the current point (the caller then calls pba_linearize). */
int pba_accept(pba_engine* e);
/* Test hooks: copies of the reduced (global) system of the LAST pba_step (after pba_solve: of the last FULL iteration -- the
 * gradient-only pass that ends a solve at the iteration limit leaves them alone): n = 6 * free cameras.
 * S[n*n] row-major = s_c (U - sum W P W^T) s_c + D_c^2, rhs[n], both in Jacobi-scaled space. */
int pba_get_reduced_system(pba_engine* e, double* S, double* rhs, int32_t* n);
/* Test hook of the cameras-constant mode (needs pba_config.flags bit 0, after a pba_step in the mode): V9 [n_points][9] the scaled and
 * damped point blocks s_p V_p s_p + D_p^2, row-major; rhs3 [n_points][3] the scaled gradient.  In the inverse-depth mode entry 0 of
 * each is set and the rest are zero.  Either pointer may be NULL. */
int pba_get_point_system(pba_engine* e, double* V9, double* rhs3);
/* Test hook: per-observation record of the last linearisation: [n_obs][6] = rho'*M11, M12, M22, rho'*b1, b2, rho/2. */
int pba_get_obs_records(pba_engine* e, double* rec6);

/* ---- the LM loop: replaces ceres::Solve (photobundle.cc:829) --------------------------------------------- */
int pba_solve(pba_engine* e, const pba_solver_options* o, pba_solver_summary* summary,
              pba_iteration_summary* iterations, int32_t max_iterations_out);

/* ---- covariance output: replaces ceres::Covariance::Compute + GetCovarianceBlock after ceres::Solve ------------
 * Blocks of (J^T J)^-1 of the reduced program of the mode that is on, J the loss-corrected Jacobian (sqrt(rho') row scaling) at the
 * current (best) state, the one pba_get_state returns.  No damping, no Jacobi scaling, unit residual variance: the caller scales by
 * its own sigma^2 (num_residuals, num_parameters and cost are there for 2 cost / (m - n)).  Camera blocks are in the engine's camera
 * parameters: angle-axis and translation of the WORLD->CAMERA transform.
 *   cam_cov    dense n_cam x n_cam, row-major, symmetric bit for bit.  Columns: the program's camera columns in ascending slot order --
 *              full mode: the slots outside the anchor mask (the layout of pba_get_reduced_system); pose-only mode: the free cameras
 *              that have a residual block.
 *   point_cov  [n_points][9] row-major 3x3; in the inverse-depth mode entry 0 is set and the rest are zero (the convention of
 *              pba_get_point_system).  Camera x point cross blocks are not computed.
 * Full mode (any anchor mask, 2..32 slots), H = [U W; W^T V]: Sigma_cc = S^-1 with S = U - sum_p W_p V_p^-1 W_p^T;
 * Sigma_pp(i) = V_i^-1 + (V_i^-1 W_i^T) Sigma_cc (W_i V_i^-1), W_i over the free cameras that observe point i (a point seen by
 * anchored cameras only: V_i^-1).  Pose-only mode: blockdiag(U_a^-1), point_cov must be NULL.  Structure-only mode: V_i^-1 (1x1 with
 * inverse depths), cam_cov must be NULL.  Either output pointer and info may be NULL.
 * Every block (S, every V_i) is factorised in its UNIT-DIAGONAL form D^-1/2 A D^-1/2, D = diag A, and the inverse is unscaled again,
 * so the reported pivots are scale-free numbers in (0, 1]; a pivot is the diagonal entry the Cholesky takes the root of.  The library
 * applies no threshold of its own: a gauge-open window (one constant frame) can pass by rounding with a pivot near 1e-12 and a
 * meaningless inverse -- min_cam_pivot and min_point_pivot are the caller's to judge.  Every sum has a fixed order: two fresh engines
 * give the same bits.
 * The call runs pba_linearize (the engine then holds a valid linearisation at the current point) and moves nothing else of the LM
 * state: scales, radius bookkeeping, candidate parity, pba_solve_driver.  It writes device buffers of its own.  The one counter that
 * can move is the one pba_linearize moves: when the current point had no valid linearisation, the Jacobian pass the call has to run
 * counts as a linearisation (pba_counters.linearize_launches under profiling, and the pass count the NEXT pba_solve resets before it
 * reports summary.num_jacobian_passes); after a pba_solve or a pba_linearize the point has one and nothing is counted.
 * PBA_ERR_INVALID with a message in pba_last_error, before any launch: a non-NULL pointer for a block family the mode holds constant;
 * a free camera of the full mode without a residual block (its block of H is zero; the message names the slot); multi-rank engines;
 * the precision-sweep flags; the inverse-depth parameterisation in the full mode.  PBA_ERR_STATE as pba_linearize gives it.
 * PBA_ERR_NUMERIC: a non-positive or non-finite pivot in any block -- H is singular, nothing is written to cam_cov / point_cov, and
 * info names the first offender (point blocks are examined before the camera matrix). */
typedef struct pba_covariance_info {
  int32_t n_cam;            /* rows of cam_cov: 6 x the program's camera columns; 0 in the structure-only mode */
  int32_t point_dim;        /* 3; 1 in the inverse-depth mode; 0 in the pose-only mode */
  int32_t num_residuals, num_parameters;   /* of the program, so that a caller can form 2 cost / (m - n) */
  double  cost;             /* program cost at the point (no fixed_cost) */
  double  min_cam_pivot;    /* smallest Cholesky pivot of the UNIT-DIAGONAL camera matrix, in (0, 1]; 1 when n_cam = 0 */
  double  min_point_pivot;  /* the same over all point blocks; 1 when the points are constant */
  int32_t failed_is_point, failed_index;   /* after PBA_ERR_NUMERIC: where the first non-positive / non-finite pivot was (point
                                            * index, or row of cam_cov); else 0, -1 */
} pba_covariance_info;
int pba_covariance(pba_engine* e, double* cam_cov, double* point_cov, pba_covariance_info* info);

/* ---- camera prior: what a sliding window remembers of the frames it evicted ------------------------------------
 * ONE extra residual block on the camera blocks `slots`, with a constant Jacobian and no loss function, in information form (a
 * marginalisation prior is singular -- it carries the gauge freedom -- so a square-root form cannot hold it).  Ceres: a CostFunction
 * over those camera blocks with the constant Jacobian Lambda^1/2.  With d = the current cameras of `slots` minus x0:
 *     E(d) = c + eta^T d + d^T Lambda d / 2,   gradient over the free slots eta + Lambda d,   Gauss-Newton block Lambda.
 * k = 0 clears (the pointers may be NULL).  slots [k] ascending, each below the n_frames of the cameras that are set; x0 [k][6];
 * Lambda [6k][6k] row-major, symmetric (the lower triangle enters the reduced system, whole rows the gradient); eta [6k]; c >= 0.
 * An anchored slot takes part in d but has no column.  The term enters every cost the LM loop sees (the linearisation cost, the
 * candidate cost, summary.initial_cost and final_cost, pba_linearize's cost: E is added last, after the photometric sum), the camera
 * gradient and its norms, the column norms that fix the Jacobi scale and the LM diagonal (diag U + diag Lambda), U of the reduced
 * system and the reduced right-hand side.  A free camera that has no residual block but is in the prior becomes a live column (it
 * counts in x_norm).  summary.num_residual_blocks and num_residuals keep counting the PHOTOMETRIC blocks only.
 * Also takes priors that do not come from a marginalisation (GPS / IMU, a previous covariance's inverse).
 * Scope: the full mode on narrow windows (<= 16 slots, <= 15 free cameras), single rank, any anchor mask.  pba_solve runs the
 * host-stepped driver while a prior is set.  Every sum has a fixed order: two fresh engines give the same bits.
 * State: the prior is an input of the linearisation -- setting or clearing it drops the linearisation, as a pba_set_frame_* does;
 * pba_set_cameras / pba_set_cameras_anchored clear it (a prior belongs to one set of cameras); pba_set_problem keeps it.
 * PBA_ERR_INVALID with a message in pba_last_error, before anything is stored: the cameras are not set; k outside 0..n_frames; slots
 * not ascending or >= n_frames; non-finite input; c < 0; multi-rank transports, the precision-sweep flags, wide windows, the
 * points-constant and cameras-constant modes, the inverse-depth mode -- whichever call comes second; pba_covariance and pba_solve_batch
 * refuse an engine that holds a prior.  After a refused call the engine holds what it held before. */
int pba_set_camera_prior(pba_engine* e, int32_t k, const int32_t* slots, const double* x0, const double* Lambda, const double* eta, double c);

/* ---- point prior: the depth a point was created from, kept as a factor ------------------------------------------
 * ONE extra residual block on every point's parameter block, with a constant Jacobian and no loss function, in information form (a
 * depth factor Lambda = n n^T / sigma^2 has rank 1, so a square-root form of full rank cannot hold it).  For point i, with
 * d = X_i - x0_i:     E_i = d^T Lambda_i d / 2,   gradient Lambda_i d,   Gauss-Newton block Lambda_i.
 * x0 [n_points][3]; Lambda6 [n_points][6] = the upper triangle row by row (00 01 02 11 12 22).  A point with Lambda_i = 0 has no prior.
 * x0 == NULL && Lambda6 == NULL clears.  E_pts = sum_i E_i enters every cost the LM loop sees (the linearisation cost, the candidate
 * cost, summary.initial_cost and final_cost, pba_linearize's cost: added last, after the photometric sum); Lambda_i d joins the point
 * gradient and its norms, diag Lambda_i the column norms that fix the Jacobi scale and the LM diagonal, Lambda_i the point block V_i
 * before damping.  summary.num_residual_blocks and num_residuals keep counting the PHOTOMETRIC blocks only; pba_get_block_costs and
 * the quantiles of pba_cull and pba_admit stay over the photometric blocks.
 * Scope: the full mode at every window shape of 2..32 slots and any anchor mask -- the engine eliminates through the wide chain
 * while a point prior is set, also on a narrow window, and pba_solve runs the host-stepped driver -- and the cameras-constant mode;
 * pba_covariance in both (V_i includes Lambda_i: rank-1 depth priors close the gauge of a window with one constant camera).  Single
 * rank.  Every sum has a fixed order: two fresh engines give the same bits.
 * State: the prior is an input of the linearisation -- setting or clearing it drops the linearisation; pba_set_problem clears it (a
 * prior belongs to one set of points); pba_set_cameras* keep it; an applied pba_cull gathers its rows with the surviving points; an
 * applied pba_admit leaves them alone.
 * PBA_ERR_INVALID with a message in pba_last_error, before anything is stored: no problem set; n_points differs from the problem's;
 * exactly one pointer NULL; a non-finite entry; a negative diagonal entry of a Lambda_i (beyond that positive semidefiniteness is the
 * caller's: an indefinite Lambda_i shows up as a point block that is not positive definite, an invalid step); multi-rank transports,
 * the precision-sweep flags, the points-constant mode, the inverse-depth mode, the camera prior (hence pba_marginalize) -- whichever
 * call comes second; pba_solve_batch refuses an engine that holds a point prior.  After a refused call the engine holds what it held
 * before.  A device error during the upload (PBA_ERR_HIP) leaves the engine without a point prior. */
int pba_set_point_prior(pba_engine* e, int32_t n_points, const double* x0, const double* Lambda6);

/* The marginalisation that produces such a prior: the Schur complement, at the current (best) state, of the cameras that leave and of
 * every point they see.  M = the points with at least one observation in a slot of drop_mask; the factors are every residual block
 * of a point of M (in any slot) plus the engine's current prior if one is set (re-expanded at the current cameras, which is exact:
 * priors chain from window to window); marginalised are the free dropped cameras and the points of M; kept are the free slots
 * outside drop_mask in ascending order -- all of them, the rows of one no factor touches are exact zeros; anchored cameras are
 * constants.  With H, g the loss-corrected Gauss-Newton matrix and gradient of those factors (no damping, no Jacobi scaling):
 *     Lambda = H_KK - H_Km H_mm^-1 H_mK,   eta = g_K - H_Km H_mm^-1 g_m,   c = cost_M - g_m^T H_mm^-1 g_m / 2 (+ the old prior's E),
 *     x0 = the current cameras of K (byte for byte).
 * The points go first, through the equilibrated 3x3 Cholesky factor pba_covariance uses, then the free dropped cameras through a
 * unit-diagonal Cholesky of their block; pivots are reported as in pba_covariance_info.  Lambda is symmetric bit for bit, every sum
 * has a fixed order.  Outputs are sized for k = n_frames: slots [PBA_MAX_FRAMES], x0 [.][6], Lambda row-major and eta; what is written is the
 * [6k][6k] matrix and the [6k] vector of the k that info reports (without info: the free slots outside drop_mask).
 * The call runs pba_linearize when the current point has no valid linearisation (counted exactly as pba_covariance counts it) and
 * moves nothing else of the LM state.  The result is what pba_set_camera_prior takes once the window has slid (the kept ring slots
 * keep their numbers).  c can come out a rounding error below zero on a window whose marginalised blocks fit exactly.
 * PBA_ERR_INVALID: an empty mask; bits at or above n_frames; no kept free camera; every mode the prior refuses.  PBA_ERR_NUMERIC: a
 * non-positive or non-finite pivot -- nothing is written but info, which names the first offender (point blocks are examined first;
 * for a camera failed_index is the row of the dropped cameras' block, 6 x its index among them + the parameter). */
typedef struct pba_marginal_info {
  int32_t k, n_points, n_blocks;     /* kept camera columns / 6; marginalised points; their residual blocks */
  double  cost;                      /* loss-corrected cost of those blocks */
  double  min_point_pivot, min_cam_pivot;   /* unit-diagonal pivots, as pba_covariance_info; 1 when there is nothing to factorise */
  int32_t failed_is_point, failed_index;
} pba_marginal_info;
int pba_marginalize(pba_engine* e, uint32_t drop_mask, int32_t* slots, double* x0, double* Lambda, double* eta, double* c, pba_marginal_info* info);

/* ---- outlier culling: the pass the reference leaves as a TODO after ceres::Solve (photobundle.cc:833-836) ---------
 * pba_get_block_costs: c_o, the loss-corrected cost rho(|r|^2) / 2 of every residual block at the current (best) state, in the order
 * of pba_set_problem's observation list (entry 5 of pba_get_obs_records, byte for byte).
 * pba_cull: the verdict over those costs, and with apply != 0 the engine's problem replaced by the survivors, all on the device.
 * The rule, with n blocks:
 *     k = (int64) floor(quantile * (double)(n - 1));  quantile_cost = the k-th smallest c_o (0-based) in the order of the IEEE bit patterns
 *     read as unsigned 64-bit integers (numeric order for the non-negative costs, NaN last), over ALL blocks of the problem in every mode;
 *     threshold = factor > 0 ? fmax(min_cost, factor * quantile_cost) : min_cost;
 *     block o is over the threshold iff !(c_o <= threshold) (a non-finite cost always is);
 *     point p stays iff at least min_observations of its blocks are not over; otherwise all of its blocks go (n_blocks_by_point_rule counts
 *     those that were not over themselves) and the point leaves.  Survivors keep their relative order, points and blocks alike.
 * block_keep [n_obs before] (1: the block stays) and point_map [n_points before] (new index, or -1) are written on PBA_OK and on the
 * "would leave no point" refusal; info whenever the verdict was reached.
 * Both calls run pba_linearize when the current point has no valid linearisation (counted exactly as pba_covariance counts it) and move
 * nothing else of the LM state.  apply == 0, or nothing to remove: the engine is untouched (applied = 0; a following pba_solve gives the
 * bits it would have given without the call).
 * An applied cull (apply != 0, at least one block removed) leaves the engine as if pba_set_problem had been called with the surviving
 * lists and the survivors' current parameters byte for byte (in the inverse-depth mode: rho and the rays) -- except that the cameras and
 * the anchor mask, the camera prior, the inverse-depth mode and the points-constant / cameras-constant switches stay as they are.  The
 * linearisation is dropped as pba_set_problem drops it: pba_step wants a pba_linearize first.  Descriptors, points and rays never leave the
 * device; the keep bytes and the point map travel to the host, which rebuilds the tile tables.
 * Every count is an integer sum and the order statistic an exact radix select: two fresh engines give the same bytes.
 * Narrow and wide windows, any anchor mask, inverse depth, both constant modes, an engine holding a prior, engines of pba_solve_batch.
 * PBA_ERR_INVALID with a message in pba_last_error, before any launch, the engine unchanged: options outside their ranges; multi-rank
 * engines; the precision-sweep flags.  After the verdict, the engine unchanged, info and the tables filled: apply != 0 and no point would
 * be left.  PBA_ERR_NUMERIC: factor * quantile_cost is not finite (engine unchanged; info holds the counts before, quantile_cost and the
 * non-finite product as threshold).  PBA_ERR_STATE as pba_linearize gives it. */
int pba_get_block_costs(pba_engine* e, double* cost /* [n_obs] */);

typedef struct pba_cull_options {
  double  min_cost;          /* >= 0, finite: floor of the threshold */
  double  factor;            /* >= 0, finite; 0: threshold = min_cost alone */
  double  quantile;          /* in [0, 1]; read when factor > 0 */
  int32_t min_observations;  /* >= 1: a point stays only with at least this many surviving blocks */
  int32_t apply;             /* 0: verdict only, the engine is not changed */
} pba_cull_options;

typedef struct pba_cull_info {
  int32_t n_blocks_before, n_blocks_after, n_points_before, n_points_after;
  int32_t n_blocks_over_threshold;   /* removed by their own cost */
  int32_t n_blocks_by_point_rule;    /* removed because their point fell below min_observations */
  double  quantile_cost, threshold;
  int32_t applied;                   /* 1 when the engine's problem was replaced */
} pba_cull_info;

int pba_cull(pba_engine* e, const pba_cull_options* o,
             uint8_t* block_keep /* [n_obs before], nullable */,
             int32_t* point_map  /* [n_points before]: new index or -1, nullable */,
             pba_cull_info* info /* nullable */);

/* ---- re-observation: the residual blocks the window should have, found once the solve has made the poses good -----------------
 * A residual block enters through addFrame's one ZNCC test under the INITIAL pose (photobundle.cc:512-542); pba_admit looks at the pairs
 * that test lost, at the refined state.  It is the counterpart of pba_cull: that call only ever shortens tracks, this one lengthens them.
 * Candidates.  A candidate is a pair (p, s) that passes every one of these tests:
 *     p is a point of the problem;
 *     s is a bit of slot_mask;
 *     (p, s) is NOT in the observation list;
 *     at the current (best) state, the one pba_get_state returns, X_c = R_s X_p + t_s has z >= min_depth;
 *     u = fx x / z + cx and v = fy y / z + cy satisfy border <= u <= cols - 1 - border and border <= v <= rows - 1 - border (as doubles).
 * Every comparison fails on a non-finite value.  In the inverse-depth mode X_p = origin + direction / rho.
 * Candidates are ordered by point ascending, then slot ascending: the order of the cand_* arrays.
 * With border smaller than the patch radius the patch may cross the image edge: legal, the sampler's clamped taps serve it as they serve
 * any such block.
 * Candidate cost.  c = rho(|r|^2) / 2 of the residual block (p, s) at the current state: the engine's sampler, the patch weights, every
 * channel, the engine's Huber threshold -- the number pba_get_block_costs would report for the block, computed by the kernel that computes
 * those (the candidate list is handed to the Jacobian pass as an observation list of its own).
 * The verdict, with n blocks in the problem:
 *     k and quantile_cost as in pba_cull, over the costs of the blocks ALREADY in the problem (not the candidates);
 *     threshold = factor > 0 ? fmax(min_cost, factor * quantile_cost) : min_cost;
 *     candidate i is taken iff c_i <= threshold (a non-finite cost never is).
 * cand_point, cand_slot, cand_cost, cand_take [capacity], each nullable: the first n_written = min(n_candidates, capacity) candidates; the
 * counts in info are the full ones whatever the capacity.  capacity = 0 with null pointers is a count.
 * The call runs pba_linearize when the current point has no valid linearisation (counted exactly as pba_covariance counts it) and moves
 * nothing else of the LM state: the candidates are evaluated into buffers of the call's own, no record, cost or counter of the engine moves.
 * apply == 0, or nothing taken: the engine is untouched (applied = 0; a following pba_solve gives the bits it would have given without the
 * call).
 * An applied admission (apply != 0, at least one candidate taken) leaves the engine as if pba_set_problem had been called with the merged
 * lists -- per point the union of its old and its taken slots, ascending -- and the current parameters byte for byte (in the inverse-depth
 * mode: rho and the rays) -- except that the cameras and the anchor mask, the camera prior, the inverse-depth mode and the points-constant /
 * cameras-constant switches stay as they are.  The point set does not change: no row of the points, descriptors or rays moves.  The merged
 * lists are written on the device into fresh buffers that are swapped in; the candidate list and the take bytes travel to the host, which
 * rebuilds the tile tables.  The linearisation is dropped as pba_set_problem drops it: pba_step wants a pba_linearize first.  A free camera
 * that had no residual block may gain some and become a live column.
 * Every count is an integer sum and the order statistic an exact radix select: two fresh engines give the same bytes.
 * Narrow and wide windows, any anchor mask, inverse depth, both constant modes, an engine holding a prior, engines of pba_solve_batch; every
 * channel count and patch radius, unit and Gaussian weights.
 * PBA_ERR_INVALID with a message in pba_last_error, before any launch, the engine unchanged: options outside their ranges; slot_mask zero,
 * with a bit at or above n_frames, or on a slot without a frame; capacity < 0; multi-rank engines; the precision-sweep flags.
 * PBA_ERR_NUMERIC: factor * quantile_cost is not finite (engine unchanged, nothing written to the cand_* arrays; info holds the counts
 * before, n_candidates, quantile_cost and the non-finite product as threshold).  PBA_ERR_STATE as pba_linearize gives it. */
typedef struct pba_admit_options {
  uint32_t slot_mask;        /* slots that may gain blocks; non-zero, bits < n_frames, each holding a frame */
  double   min_depth;        /* > 0, finite: z of the point in the camera must be >= this */
  int32_t  border;           /* >= 0; the projection must satisfy border <= u <= cols-1-border, border <= v <= rows-1-border (doubles) */
  double   min_cost, factor, quantile;   /* the threshold, exactly pba_cull's form and ranges */
  int32_t  apply;            /* 0: verdict only */
} pba_admit_options;

typedef struct pba_admit_info {
  int32_t n_blocks_before, n_blocks_after, n_points;
  int32_t n_candidates, n_admitted;
  int32_t n_written;         /* entries written to the cand_* arrays = min(n_candidates, capacity) */
  double  quantile_cost, threshold;
  int32_t applied;           /* 1 when the engine's observation lists were replaced */
} pba_admit_info;

int pba_admit(pba_engine* e, const pba_admit_options* o, int32_t capacity,
              int32_t* cand_point, int32_t* cand_slot, double* cand_cost, uint8_t* cand_take,  /* [capacity], each nullable */
              pba_admit_info* info /* nullable */);

/* ---- several independent windows on one device ------------------------------------------------------------ */
#define PBA_MAX_BATCH 64
/* Solves n independent windows together: one launch of each phase of a pipelined LM iteration serves every window still running.
 * Each window's result equals its own pba_solve bit for bit (summary, iteration log, cameras, points; wall-clock fields aside).
 * options: [n] or NULL for the defaults of pba_default_solver_options; summaries: [n]; iterations: [n][max_iterations_out] or NULL.
 * Every check comes before any device call; PBA_ERR_INVALID / PBA_ERR_STATE refuse the whole batch, with the offending index and the
 * reason in pba_last_error of engines[0] and of that engine:  1 <= n <= PBA_MAX_BATCH; engines non-null, each once, all on one device;
 * every engine ready (PBA_ERR_STATE), single-rank, narrow (<= 15 free cameras), without the precision-sweep flags or profiling, with
 * options the pipelined driver takes; one kernel key (patch radius, channel count, unit or Gaussian weights) for all.  Windows may differ
 * in everything else (image size, K, points, frames, fixed slot, Huber threshold, options, inverse depth).  Synchronous like pba_solve;
 * afterwards pba_solve_driver names "batched".  A timed-out wait makes every engine of the batch unusable. */
int pba_solve_batch(pba_engine* const* engines, int32_t n, const pba_solver_options* options,
                    pba_solver_summary* summaries, pba_iteration_summary* iterations, int32_t max_iterations_out);

/* ---- multi-GPU: points are sharded across ranks, one all-reduce of the reduced camera system per solve --- */
/* RCCL transport (one process per GPU): rank 0 calls pba_comm_unique_id, broadcasts the 128 bytes out of band. */
int pba_comm_unique_id(void* id128);
int pba_comm_init_rccl(pba_engine* e, const void* id128, int32_t rank, int32_t world);
/* Host-staged transport: fn must sum `n` doubles in place across all ranks (op 0) or take the max (op 1). */
typedef int (*pba_allreduce_fn)(double* buf, int64_t n, int32_t op, void* ctx);
int pba_comm_init_callback(pba_engine* e, pba_allreduce_fn fn, void* ctx, int32_t rank, int32_t world);

/* Device-side exchange (optional, after pba_comm_init_rccl / pba_comm_init_callback, collective: every rank calls it):
 * the two per-step all-reduces become flag-and-slot reads of peer-mapped mailboxes (hipIpc*, fine-grained device memory)
 * inside small kernels on the engine's stream -- no collective launch per LM step, sums in rank order (bit-identical on all
 * ranks).  The base transport carries the IPC handles and stays the fallback: the call returns PBA_OK whether or not the
 * mapping succeeded (every rank takes the same decision); pba_comm_transport names what is in use ("rccl", "rccl+peer",
 * "callback", "callback+peer", "none").  Waits are bounded by PBA_WAIT_TIMEOUT_S -> PBA_ERR_COMM. */
int pba_comm_enable_peer_exchange(pba_engine* e);
const char* pba_comm_transport(const pba_engine* e);
/* Ranks the transport itself reports (ncclCommCount for RCCL, the callback's world otherwise; 1 without a transport). */
int pba_comm_rank_count(const pba_engine* e);

/* Per-kernel accounting.  pba_set_profiling mode 0: off.  1 (what pba_reset_counters switches on): HIP events around
 * every kernel of the host-stepped driver -- each bracket ends with an event record (a cache write-back the pipelined run
 * does not pay) and the exchanges are timed too.  2: device time stamps inside the ASYNCHRONOUS pipeline (single rank):
 * the three kernels of an LM iteration run back to back, the interval between two consecutive kernel ends is a kernel's
 * share of the iteration; nothing is added to the stream.  pba_get_counters reports whichever mode is on. */
int pba_set_profiling(pba_engine* e, int32_t mode);
int pba_get_counters(pba_engine* e, pba_counters* c);
int pba_reset_counters(pba_engine* e);

/* Which driver ran the LAST pba_solve: "resident" (the whole solve as ONE cooperative launch, every workgroup keeping its tiles'
 * state in registers across the iterations: windows that fit one resident round of workgroups -- <= 2 x 128 observations per CU --
 * on a single rank, patch radius <= 2, <= 8 free cameras; PBA_RESIDENT=0 switches it off), "pipelined" (three kernels per
 * iteration enqueued ahead of the device-side decisions), "host-stepped" (PBA_ASYNC=0, event profiling), "batched" (pba_solve_batch),
 * "none".  They take the same decisions on the same numbers; "resident", "pipelined" and "batched" are bit-identical. */
const char* pba_solve_driver(const pba_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* PBA_H */
