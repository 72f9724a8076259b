/*
 * pba_stereo.h -- C-ABI of the MI355X stereo block matcher (exported from libpba_hip.so next to pba.h).
 *
 * Replaces step 1 of the reference's per-frame pipeline (apps/run_kitti.cc:39-47, src/dataset.cc:105-137): OpenCV 2.4
 * cvFindStereoCorrespondenceBM as set up by src/stereo_algorithm.cc:246-265, plus disparityToDepth (src/imgproc.cc:280-322)
 * fused into its epilogue.  The arithmetic is this project's statement of OpenCV 2.4 StereoBM (generic C path, XSOBEL
 * prefilter, no speckle filter, no left-right check); DESIGN.md "Stereo block matching" holds the spec.  Bit parity with an
 * OpenCV binary is not pinned: none exists on the machines this project is tested on.
 *
 * The handle is separate from pba_engine and touches none of its state.  Functions return 0 or a negative pba_status
 * (pba.h); they never throw.  Host buffers are caller-owned and only used during the call.  One host thread per handle.
 * There is no CPU fallback: pba_stereo_create fails with PBA_ERR_NO_DEVICE when no GPU is visible.
 */
#ifndef PBA_STEREO_H
#define PBA_STEREO_H

#include <stdint.h>

#include "pba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pba_stereo pba_stereo;

#define PBA_STEREO_PREFILTER_NORMALIZED_RESPONSE 0   /* refused */
#define PBA_STEREO_PREFILTER_XSOBEL 1

/* names and defaults of reference src/stereo_algorithm.cc:249-264 (the OpenCV 2.4 CvStereoBMState fields) */
typedef struct pba_stereo_bm_params {
  int32_t pre_filter_type;        /* XSOBEL (1) only */
  int32_t pre_filter_size;        /* odd, 5..255 (checked as OpenCV does; XSOBEL does not use it) */
  int32_t pre_filter_cap;         /* 1..63 */
  int32_t sad_window_size;        /* odd, 5..255, <= min(rows, cols) */
  int32_t min_disparity;          /* any; min_disparity - 1 and the largest disparity must fit the int16 output (|.| <= 2047) */
  int32_t number_of_disparities;  /* > 0, multiple of 16; no default (the reference requires the key) */
  int32_t texture_threshold;      /* >= 0 */
  int32_t uniqueness_ratio;       /* >= 0 */
  int32_t speckle_window_size;    /* 0 only (speckle filtering is not built) */
  int32_t speckle_range;          /* unused while speckle_window_size = 0 */
  int32_t try_smaller_windows;    /* 0 only */
  int32_t disp12_max_diff;        /* < 0 only (no left-right check) */
} pba_stereo_bm_params;

/* XSOBEL, 9, 31, 15, 0, 0 (must be set), 10, 15, 0, 0, 0, -1 */
void pba_stereo_default_params(pba_stereo_bm_params* p);

/* Checks p as pba_stereo_create does, without touching a device; rows = cols = 0 skips the checks that need the image size.
 * PBA_ERR_INVALID carries its reason in pba_stereo_last_error(NULL). */
int pba_stereo_validate_params(int32_t rows, int32_t cols, const pba_stereo_bm_params* p);

/* Validates p (PBA_ERR_INVALID before any device call), then allocates the device and pinned host buffers of a rows x cols
 * matcher on HIP device `device`. */
int pba_stereo_create(int32_t rows, int32_t cols, const pba_stereo_bm_params* p, int32_t device, pba_stereo** out);

/* left, right: rows*cols u8, row-major.  disp16 (nullable): int16 disparity with 4 fractional bits, FILTERED =
 * (min_disparity - 1) * 16.  depth (nullable): fp32 depth = d > 0.01 ? bf * (1 / d) : -0.1 with d = disp16 / 16, every
 * pixel (FILTERED included).  Only the outputs asked for are copied back.  Synchronous: returns when they are written. */
int pba_stereo_compute(pba_stereo* s, const uint8_t* left, const uint8_t* right, float bf, int16_t* disp16, float* depth);

/* Message of the last failure on s; with s = NULL, of the calling thread's last failed pba_stereo_create. */
const char* pba_stereo_last_error(const pba_stereo* s);

void pba_stereo_destroy(pba_stereo* s);

/* Test hook: the XSOBEL-prefiltered pair of the last pba_stereo_compute (rows*cols u8 each). */
int pba_stereo_get_prefiltered(pba_stereo* s, uint8_t* left, uint8_t* right);

/* Timing of the last pba_stereo_compute from device events: kernels_ms = prefilter start .. matcher end, total_ms = upload
 * start .. last copy-back end.  Either pointer may be NULL. */
int pba_stereo_get_timing(pba_stereo* s, float* kernels_ms, float* total_ms);

#ifdef __cplusplus
}
#endif

#endif
