// pba_device.h -- device-side data layout shared by the kernels and the engine (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pba.h"
#include "pba_lm_rules.h"      // the scalar block of a step (Scal), LmState and the trust-region rules
#include "pba_slot_rule.h"     // anchor mask -> (is_free, free_index) of a window slot

namespace pba {

constexpr int kMaxFrames = 16;        // camera tables of the narrow kernels (windows of <= 15 free cameras)
constexpr int kMaxFramesWide = 32;    // PBA_MAX_FRAMES: camera tables of the wide-window chain (pba_wide.h)
constexpr int kMaxRadius = 5;

// Packed frame texel (one u32 per pixel), bit-exact for u8 frames:
//   bits  0..7   I                      (photobundle.cc:231: image.cast<float>() -> integers 0..255)
//   bits  8..17  2*Gx  two's complement (imgproc.cc:38: 0.5f * (I[x+1] - I[x-1]) -> multiples of 0.5 in +-127.5)
//   bits 18..27  2*Gy  two's complement (imgproc.cc:39)
// Border rows/columns carry zero gradients (imgproc.cc:34-35, 42-43, 79-80, 93-94).
__host__ __device__ inline uint32_t pack_texel(int I, int gx2, int gy2) {
  return (uint32_t)(I & 0xff) | ((uint32_t)(gx2 & 0x3ff) << 8) | ((uint32_t)(gy2 & 0x3ff) << 18);
}

// Per-camera geometry, recomputed whenever the cameras change (k_cam_geom).
//   value path   : the exact operation order of ceres::AngleAxisRotatePoint (call site photobundle.cc:700)
//   R[9]         : row-major d(xw)/d(point)   (Rodrigues matrix, or I + [w]x in the small-angle branch)
//   dR[3][9]     : row-major d(xw)/d(w_k) = dR[k] * point   (R [B_k]x, B = (w w^T + (R^T - I)[w]x) / theta^2;
//                  [e_k]x in the small-angle branch, i.e. the derivative of the code as written)
struct CamGeom {
  double aa[3];
  double t[3];
  double w[3];     // aa * (1/theta)
  double ct, st;   // cos(theta), sin(theta)
  double R[9];
  double dR[27];
  int32_t rodrigues;  // theta^2 > DBL_EPSILON
  int32_t is_free;    // 0 for a constant (anchored) camera
  int32_t free_index; // index among free cameras, -1 if constant
  int32_t pad;
};

}  // namespace pba
