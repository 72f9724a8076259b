// pba_admit.h -- re-observation (pba_admit): the (point, slot) pairs that are NOT in the observation list but whose projection at the current
// state lies inside the image, the verdict over their block costs, and the observation lists merged with the ones that were taken.
//   k_admit_enum     one lane per point: the camera records of the window in LDS once per workgroup; the point's present-slot mask from
//                    pt_begin / obs_slot; for every slot of slot_mask that is not present the geometric test -> a 32-bit candidate mask
//                    per point, and the workgroup's candidate count
//   k_admit_offsets  ONE workgroup: exclusive scan of the workgroup sums (two columns), and the totals (the k_cull_offsets pattern)
//   k_admit_fill     one lane per point: scan inside the workgroup -> first candidate of the point; writes the candidate list (point
//                    ascending, slot ascending) and, per point, where its candidates begin
//   (the candidates' costs come from the Jacobian-pass kernel itself, launched by the engine over the candidate list: row 5 of its records)
//   k_admit_verdict  one lane per candidate: taken iff cost <= threshold; the take byte, and the slot's bit into the point's taken mask
//                    (an integer OR: the result does not depend on the order)
//   k_admit_count    one lane per point: blocks after = blocks before + bits of the taken mask; workgroup sums (blocks after, taken)
//   k_admit_merge    one lane per point: scan inside the workgroup -> the point's first block in the merged list (the new pt_begin); writes
//                    old | taken slots ascending into FRESH arrays (the engine swaps them in)
// Every count is an integer sum; nothing here adds floating-point numbers across lanes: two engines give the same bytes.
// Included by pba_engine.hip (after pba_cull.h: the workgroup scan and the select are shared).
#pragma once
#include "pba_cull.h"
#include "pba_kernels.h"

namespace pba {

constexpr int kAdmitThreads = kCullThreads;      // (cull_block_scan serves 256 lanes)
constexpr int kAdmitTotals = 2;

struct AdmitParams {
  const double* xyz;            // [n_points][3] point parameters of the current state
  const double* rays;           // inverse-depth variant (point_world), else null
  const CamGeom* geom;          // [n_frames] of the current state
  const int32_t* pt_begin;      // [n_points + 1]
  const uint8_t* obs_slot;      // [n_obs]
  const uint64_t* sel;          // k_cull_finish over the costs of the problem's own blocks: sel[1] = threshold
  const double* cand_cost;      // [n_cand] row 5 of the candidates' records
  uint32_t* cand_mask;          // [n_points]
  uint32_t* take_mask;          // [n_points] zero before k_admit_verdict
  int32_t* cand_begin;          // [n_points] first candidate of the point
  int32_t* cand_point;          // [n_cand]
  uint8_t* cand_slot;           // [n_cand]
  uint8_t* cand_take;           // [n_cand]
  uint2* part;                  // [point blocks] workgroup sums
  uint2* off;                   // [point blocks] their exclusive scan
  int32_t* tot;                 // [kAdmitTotals]
  int32_t* obs_point_new;       // [n_obs + taken] merged
  uint8_t* obs_slot_new;
  int32_t* pt_begin_new;        // [n_points + 1]
  double fx, fy, cx, cy;
  double min_depth, u_lo, u_hi, v_lo, v_hi;      // the border box, as doubles
  uint32_t slot_mask;
  int32_t n_points, n_frames, n_cand, n_part;
};

// Sum of one value per lane over the workgroup, in every lane.  sh: [kCullBins]
__device__ __forceinline__ uint32_t admit_block_total(uint32_t incl, uint32_t* sh) {
  if (threadIdx.x == kAdmitThreads - 1) sh[0] = incl;
  __syncthreads();
  const uint32_t t = sh[0];
  __syncthreads();
  return t;
}

// z >= min_depth and (u, v) inside the box; every comparison fails on a non-finite value
__device__ __forceinline__ bool admit_in_view(const AdmitParams& p, const CamGeom& g, const double X[3]) {
  double xw[3], u, v;
  transform_point(g, X, xw);
  if (!(xw[2] >= p.min_depth)) return false;
  project_point(xw, p.fx, p.fy, p.cx, p.cy, u, v);
  return u >= p.u_lo && u <= p.u_hi && v >= p.v_lo && v <= p.v_hi;
}

__global__ __launch_bounds__(kAdmitThreads) void k_admit_enum(AdmitParams p) {
  __shared__ CamGeom s_geom[kMaxFramesWide];
  __shared__ uint32_t sh[kCullBins];
  const int tid = threadIdx.x;
  stage_geom<kAdmitThreads, false, kMaxFramesWide>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const int pt = blockIdx.x * kAdmitThreads + tid;
  uint32_t cand = 0;
  if (pt < p.n_points) {
    uint32_t present = 0;
    const int o1 = p.pt_begin[pt + 1];
    for (int o = p.pt_begin[pt]; o < o1; ++o) present |= 1u << p.obs_slot[o];
    const double prm[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
    double X[3], qd[3];
    point_world(p.rays, pt, prm, X, qd);
    uint32_t todo = p.slot_mask & ~present;
    while (todo) {
      const int s = __ffs((int)todo) - 1;
      todo &= todo - 1;
      if (s < p.n_frames && admit_in_view(p, s_geom[s], X)) cand |= 1u << s;
    }
    p.cand_mask[pt] = cand;
  }
  const uint32_t total = admit_block_total(cull_block_scan((uint32_t)__popc(cand), sh), sh);
  if (tid == 0) p.part[blockIdx.x] = make_uint2(total, 0u);
}

__global__ __launch_bounds__(kAdmitThreads) void k_admit_offsets(AdmitParams p) {
  __shared__ uint32_t sh[kCullBins];
  uint32_t carry_x = 0, carry_y = 0;
  for (int base = 0; base < p.n_part; base += kAdmitThreads) {
    const int b = base + threadIdx.x;
    const uint2 v = b < p.n_part ? p.part[b] : make_uint2(0u, 0u);
    const uint32_t ix = cull_block_scan(v.x, sh), iy = cull_block_scan(v.y, sh);
    if (b < p.n_part) p.off[b] = make_uint2(carry_x + ix - v.x, carry_y + iy - v.y);
    carry_x += admit_block_total(ix, sh);
    carry_y += admit_block_total(iy, sh);
  }
  if (threadIdx.x == 0) { p.tot[0] = (int)carry_x; p.tot[1] = (int)carry_y; }
}

__global__ __launch_bounds__(kAdmitThreads) void k_admit_fill(AdmitParams p) {
  __shared__ uint32_t sh[kCullBins];
  const int pt = blockIdx.x * kAdmitThreads + threadIdx.x;
  uint32_t cand = pt < p.n_points ? p.cand_mask[pt] : 0u;
  const uint32_t cnt = (uint32_t)__popc(cand);
  const uint32_t incl = cull_block_scan(cnt, sh);
  if (pt >= p.n_points) return;
  int dst = (int)(p.off[blockIdx.x].x + incl - cnt);
  p.cand_begin[pt] = dst;
  while (cand) {
    const int s = __ffs((int)cand) - 1;
    cand &= cand - 1;
    if (dst < p.n_cand) { p.cand_point[dst] = pt; p.cand_slot[dst] = (uint8_t)s; }
    ++dst;
  }
}

__global__ __launch_bounds__(kAdmitThreads) void k_admit_verdict(AdmitParams p) {
  const int i = blockIdx.x * kAdmitThreads + threadIdx.x;
  if (i >= p.n_cand) return;
  const double thr = __longlong_as_double((long long)p.sel[1]);
  const bool take = p.cand_cost[i] <= thr;      // (a non-finite cost never is)
  p.cand_take[i] = take ? 1 : 0;
  if (take) atomicOr(&p.take_mask[p.cand_point[i]], 1u << p.cand_slot[i]);
}

__global__ __launch_bounds__(kAdmitThreads) void k_admit_count(AdmitParams p) {
  __shared__ uint32_t sh[kCullBins];
  const int pt = blockIdx.x * kAdmitThreads + threadIdx.x;
  uint32_t after = 0, taken = 0;
  if (pt < p.n_points) {
    taken = (uint32_t)__popc(p.take_mask[pt]);
    after = (uint32_t)(p.pt_begin[pt + 1] - p.pt_begin[pt]) + taken;
  }
  const uint32_t ta = admit_block_total(cull_block_scan(after, sh), sh), tt = admit_block_total(cull_block_scan(taken, sh), sh);
  if (threadIdx.x == 0) p.part[blockIdx.x] = make_uint2(ta, tt);
}

// n_after: blocks of the merged list (k_admit_offsets' first total, read by the host): the bound of every store
__global__ __launch_bounds__(kAdmitThreads) void k_admit_merge(AdmitParams p, int32_t n_after) {
  __shared__ uint32_t sh[kCullBins];
  const int pt = blockIdx.x * kAdmitThreads + threadIdx.x;
  uint32_t taken = 0;
  int o0 = 0, o1 = 0;
  if (pt < p.n_points) { taken = p.take_mask[pt]; o0 = p.pt_begin[pt]; o1 = p.pt_begin[pt + 1]; }
  const uint32_t cnt = (uint32_t)(o1 - o0) + (uint32_t)__popc(taken);
  const uint32_t incl = cull_block_scan(cnt, sh);
  if (pt >= p.n_points) return;
  int dst = (int)(p.off[blockIdx.x].x + incl - cnt);
  p.pt_begin_new[pt] = dst;
  if (pt == p.n_points - 1) p.pt_begin_new[p.n_points] = dst + (int)cnt;
  // two ascending runs, merged: the old slots in list order, the taken slots by lowest bit
  int o = o0;
  while (o < o1 || taken) {
    const int s_old = o < o1 ? (int)p.obs_slot[o] : 64, s_new = taken ? __ffs((int)taken) - 1 : 64;
    int s;
    if (s_old < s_new) { s = s_old; ++o; }
    else { s = s_new; taken &= taken - 1; }
    if (dst < n_after) { p.obs_point_new[dst] = pt; p.obs_slot_new[dst] = (uint8_t)s; }
    ++dst;
  }
}

}  // namespace pba
