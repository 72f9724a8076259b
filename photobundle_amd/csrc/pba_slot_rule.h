// pba_slot_rule.h -- THE rule that turns the anchor mask of pba_set_cameras_anchored into the camera columns of the reduced program:
// slot c is constant when bit c of the mask is set (Ceres: SetParameterBlockConstant on that camera block); the free slots keep
// their ascending order, so the free index of slot c is the number of free slots below it.  Every place that needs the rule calls
// it here: cam_geom_one / cam_geom_finish on the device, and on the host whatever sizes n_free, n_pairs, part_stride, the solve
// tables and the co-observation lists of the wide chain.  No HIP header is needed: plain C++ compiles it (tests/native does).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PBA_SLOT_FN __host__ __device__ inline
#else
#define PBA_SLOT_FN inline
#endif

namespace pba {

// the mask of the one-slot call: pba_set_cameras(e, cams, n, fixed_slot)
PBA_SLOT_FN uint32_t slot_mask_of_fixed(int fixed_slot) { return fixed_slot < 0 ? 0u : 1u << fixed_slot; }

PBA_SLOT_FN int slot_is_free(uint32_t anchor_mask, int c) { return ((anchor_mask >> c) & 1u) ? 0 : 1; }

// index of slot c among the free slots, -1 for an anchored slot
PBA_SLOT_FN int slot_free_index(uint32_t anchor_mask, int c) {
  if ((anchor_mask >> c) & 1u) return -1;
  return c - __builtin_popcount(anchor_mask & ((1u << c) - 1u));
}

// free slots among the first n_frames (n_frames <= 32)
PBA_SLOT_FN int slot_count_free(uint32_t anchor_mask, int n_frames) {
  const uint32_t window = n_frames >= 32 ? 0xffffffffu : (1u << n_frames) - 1u;
  return n_frames - __builtin_popcount(anchor_mask & window);
}

}  // namespace pba
