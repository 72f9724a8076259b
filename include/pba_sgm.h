/*
 * pba_sgm.h -- C-ABI of the MI355X semi-global stereo matcher (exported from libpba_hip.so next to pba.h and pba_stereo.h).
 *
 * The reference's StereoAlgorithm = SGM (its SgmStereo / SGMStereo classes, src/stereo_algorithm.cc): capped Sobel and census
 * prefilter, half-pixel interval cost + weighted census hamming, box aggregation, two passes of two paths with penalties
 * P1 / P2 in saturating int16, first-minimum winner with a double-precision sub-pixel step, speckle filter (100 pixels,
 * 2 * disparityFactor), left-right check on the left map, and disparityToDepth fused into the last kernel.  The arithmetic is
 * held bit for bit to fixtures made by the reference's own code (tests/golden/sgm); DESIGN.md 4.10 holds the spec.
 *
 * The handle is separate from pba_engine and pba_stereo and touches none of their state.  Functions return 0 or a negative
 * pba_status (pba.h); they never throw.  Host buffers are caller-owned and only used during the call.  One host thread per
 * handle.  There is no CPU fallback: pba_sgm_create fails with PBA_ERR_NO_DEVICE when no GPU is visible.
 */
#ifndef PBA_SGM_H
#define PBA_SGM_H

#include <stdint.h>

#include "pba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pba_sgm pba_sgm;

/* keys and defaults of the reference's SgmStereo::Config (src/stereo_algorithm.cc:229-237, :393-402) */
typedef struct pba_sgm_params {
  int32_t number_of_disparities;     /* numberOfDisparities 128: > 0, multiple of 16, <= cols */
  int32_t sobel_cap_value;           /* sobelCapValue 15: any; used as min(max(v, 15), 127) | 1, as the reference does */
  int32_t census_radius;             /* censusRadius 2: 1 or 2 */
  int32_t window_radius;             /* windowRadius 2: 0..9, and rows >= window_radius + 1 */
  int32_t smoothness_penalty_small;  /* smoothnessPenaltySmall 100: 0 <= small < large <= 32767 */
  int32_t smoothness_penalty_large;  /* smoothnessPenaltyLarge 1600 */
  int32_t consistency_threshold;     /* consistencyThreshold 1: >= 0 */
  int32_t reserved;                  /* 0 */
  double disparity_factor;           /* disparityFactor 256: integer-valued, >= 1, number_of_disparities * factor <= 65536 */
  double census_weight_factor;       /* censusWeightFactor 1/6: >= 0 */
} pba_sgm_params;

void pba_sgm_default_params(pba_sgm_params* p);

/* Checks p as pba_sgm_create does, without touching a device; rows = cols = 0 skips the checks that need the image size.
 * PBA_ERR_INVALID carries its reason, with the reference's key name, in pba_sgm_last_error(NULL). */
int pba_sgm_validate_params(int32_t rows, int32_t cols, const pba_sgm_params* p);

/* Validates p (PBA_ERR_INVALID before any device call), then allocates every device and pinned host buffer of a
 * rows x cols matcher on HIP device `device` (two int16 sum volumes and one uint16 cost volume of rows*cols*D each). */
int pba_sgm_create(int32_t rows, int32_t cols, const pba_sgm_params* p, int32_t device, pba_sgm** out);

/* left, right: rows*cols u8, row-major.  Outputs, each nullable, rows*cols: disp_scaled = the left uint16 map after the
 * left-right check (disparity * disparity_factor, 0 = invalid); disparity = (float)(disp_scaled / disparity_factor);
 * depth = disparity > 0.01f ? bf * (1.0f / disparity) : -0.1f.  Only the outputs asked for are copied back.  Synchronous. */
int pba_sgm_compute(pba_sgm* s, const uint8_t* left, const uint8_t* right, float bf, uint16_t* disp_scaled, float* disparity,
                    float* depth);

/* Message of the last failure on s; with s = NULL, of the calling thread's last failed pba_sgm_create / validate. */
const char* pba_sgm_last_error(const pba_sgm* s);

void pba_sgm_destroy(pba_sgm* s);

/* Timing of the last pba_sgm_compute from device events: kernels_ms = first kernel start .. last kernel end, total_ms =
 * upload start .. last copy-back end.  Either pointer may be NULL. */
int pba_sgm_get_timing(pba_sgm* s, float* kernels_ms, float* total_ms);

/* Test hook: one intermediate of the last pba_sgm_compute, copied to buf. */
#define PBA_SGM_STAGE_SOBEL_LEFT 0          /* u8  rows*cols */
#define PBA_SGM_STAGE_SOBEL_RIGHT 1         /* u8  rows*cols (not mirrored) */
#define PBA_SGM_STAGE_CENSUS_LEFT 2         /* i32 rows*cols */
#define PBA_SGM_STAGE_CENSUS_RIGHT 3        /* i32 rows*cols */
#define PBA_SGM_STAGE_COST_LEFT 4           /* u16 rows*cols*D, d fastest */
#define PBA_SGM_STAGE_SUM_LEFT 5            /* i16 rows*cols*D: the four path costs of the left solve, summed */
#define PBA_SGM_STAGE_DISP_LEFT_RAW 6       /* u16 rows*cols, before the speckle filter */
#define PBA_SGM_STAGE_DISP_RIGHT_RAW 7
#define PBA_SGM_STAGE_DISP_LEFT_FILTERED 8  /* u16 rows*cols, after the speckle filter, before the left-right check */
#define PBA_SGM_STAGE_DISP_RIGHT_FILTERED 9
#define PBA_SGM_STAGE_COUNT 10
int pba_sgm_get_stage(pba_sgm* s, int32_t stage, void* buf);

#ifdef __cplusplus
}
#endif

#endif
