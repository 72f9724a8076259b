// pba_batch.h -- batched twins of one pipelined LM iteration: N independent narrow windows of one kernel key (patch radius,
// channel count, unit or Gaussian weights) share ONE launch of each phase (pba_solve_batch).
//
// Every window keeps its own decomposition: the launch grid is the concatenation of the windows' solo grids, a block-prefix table
// maps the global workgroup index to (window, local block, local grid), and the workgroup then runs exactly what the solo kernel runs
// with that local block and grid (the same device bodies: schur_body, reduce_solve_wg, sample_wg, sample_mc_wg).  The per-window
// parameter structs sit in a device table built once per batch; what changes from launch to launch (which windows take part, in which
// variant, with which sequence number) travels in the kernel arguments.  Sums, tickets, trust-region state and logs are the window's
// own, so every window computes the bits of its solo solve.
#pragma once
#include "pba_kernels.h"

namespace pba {

constexpr int kMaxBatch = 64;     // PBA_MAX_BATCH
constexpr int kBatchSampleWaves = 4;   // the solo sampling kernels' workgroup (pba_engine.hip: kSampleWaves)

// One window of a batch.  Variant 0 | 1 of each phase:
//   schur / rsolve: [0] full iteration (kind 1), [1] gradient-only final pass (kind 2, which also decides and flushes)
//   sample:         [0] first linearisation (kind 0), [1] candidate pass of a full iteration (kind 1)
struct BatchWindow {
  SchurParams schur[2];
  ReduceSolveParams rsolve[2];
  SampleParams sample[2];
  const float* frames_mc;         // channel planes (multi-channel descriptors), else null
  int32_t channels;
};

// One launch of one phase: entries k < n are windows win[k] with workgroups [begin[k], begin[k + 1]) of the grid.
// mode[k]: bit 0 = variant, bit 1 = init_scale (first iteration: Jacobi scales are formed).  seq[k]: the window's sequence number
// of this enqueue (its k_schur publishes seq - 1, the step before).
struct BatchLaunch {
  const BatchWindow* tab;
  int32_t n;
  int32_t begin[kMaxBatch + 1];
  uint8_t win[kMaxBatch];
  uint8_t mode[kMaxBatch];
  unsigned long long seq[kMaxBatch];
};

// entry of global workgroup b: the last k with begin[k] <= b (binary search over the uniform prefix table)
__device__ __forceinline__ int batch_entry(const BatchLaunch& L, const int b) {
  int lo = 0, hi = L.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (L.begin[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// k_schur for every window of the launch (the same publication, selection and body as the solo kernel)
__global__ __launch_bounds__(kTile, 2) void k_schur_batch(const BatchLaunch L) {
  const int k = batch_entry(L, (int)blockIdx.x);
  const int b0 = L.begin[k], lb = (int)blockIdx.x - b0, lgrid = L.begin[k + 1] - b0;
  const int mode = L.mode[k];
  SchurParams p = L.tab[L.win[k]].schur[mode & 1];
  p.init_scale = (mode >> 1) & 1;
  p.pub_seq = L.seq[k] - 1;
  if (!schur_prologue(p, false, lb, (int)threadIdx.x)) return;
  __shared__ __attribute__((aligned(16))) char smem[kSchurSmemBytes];
  schur_body<const void>(p, smem, (int)threadIdx.x, lb, lgrid, nullptr, nullptr, true);
}

// k_reduce_solve for every window of the launch; dynamic LDS = the largest window's solve
__global__ __launch_bounds__(kReduceThreads) void k_reduce_solve_batch(const BatchLaunch L) {
  extern __shared__ __attribute__((aligned(16))) char dyn_smem[];
  const int k = batch_entry(L, (int)blockIdx.x);
  const int b0 = L.begin[k], lb = (int)blockIdx.x - b0, lgrid = L.begin[k + 1] - b0;
  const int mode = L.mode[k];
  ReduceSolveParams rsp = L.tab[L.win[k]].rsolve[mode & 1];
  rsp.so.init_scale = (mode >> 1) & 1;
  if (mode & 1) rsp.fin.seq = L.seq[k];
  reduce_solve_wg(rsp, dyn_smem, lb, lgrid, (int)threadIdx.x);
}

// the fused sampling kernel (k_sample / k_sample_mc, JAC) for every window of the launch
template <int R, bool UNITW>
__global__ __launch_bounds__(kBatchSampleWaves * 64) __attribute__((amdgpu_waves_per_eu((R <= 2 ? PBA_SAMPLE_WAVES_PER_SIMD : (R >= 4 ? PBA_SAMPLE_WAVES_LARGE : 2)), (R <= 2 ? PBA_SAMPLE_WAVES_PER_SIMD : (R >= 4 ? PBA_SAMPLE_WAVES_LARGE : 2)))))
void k_sample_batch(const BatchLaunch L) {
  const int k = batch_entry(L, (int)blockIdx.x);
  const int b0 = L.begin[k], lb = (int)blockIdx.x - b0, lgrid = L.begin[k + 1] - b0;
  const int mode = L.mode[k];
  SampleParams p = L.tab[L.win[k]].sample[mode & 1];
  if (mode & 1) p.seq = L.seq[k];
  if (!sample_prologue<true>(p, false, lb, (int)threadIdx.x)) return;
  __shared__ SampleSmem<R, kBatchSampleWaves> sm;
  ResLane<R> unused;
  sample_wg<R, true, kBatchSampleWaves, true, UNITW, false, false, kMaxFrames, true>(p, sm, unused, xcd_logical_block(lb, lgrid), lgrid, (int)threadIdx.x);
}

template <int R, bool UNITW>
__global__ __launch_bounds__(kBatchSampleWaves * 64) __attribute__((amdgpu_waves_per_eu(PBA_MC_WAVES(R), PBA_MC_WAVES(R)))) void k_sample_mc_batch(const BatchLaunch L) {
  const int k = batch_entry(L, (int)blockIdx.x);
  const int b0 = L.begin[k], lb = (int)blockIdx.x - b0, lgrid = L.begin[k + 1] - b0;
  const int mode = L.mode[k];
  const BatchWindow& bw = L.tab[L.win[k]];
  SampleParams p = bw.sample[mode & 1];
  if (mode & 1) p.seq = L.seq[k];
  if (!sample_prologue<true>(p, false, lb, (int)threadIdx.x)) return;
  sample_mc_wg<R, true, kBatchSampleWaves, true, UNITW>(p, bw.frames_mc, bw.channels, lb, lgrid, (int)threadIdx.x);
}

}  // namespace pba
