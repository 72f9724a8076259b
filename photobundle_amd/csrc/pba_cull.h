// pba_cull.h -- outlier culling (pba_cull, pba_get_block_costs): the verdict over the loss-corrected block costs of a Jacobian pass
// (row 5 of rec[cur]), the order statistic it needs, and the compaction of the problem to the survivors.
//   k_cull_hist      radix select over the 64-bit patterns, most significant byte first: pass p counts byte p of every value whose
//                    higher bytes equal the bucket path of the passes before it.  Bins are privatised in LDS (one 256-bin table per
//                    workgroup, a run of equal bins is counted in a register first), then added to the pass's global table.  Integer
//                    atomics only: a count does not depend on the order of its increments.  Every workgroup re-derives the bucket
//                    path from the finished tables of the earlier passes (cull_walk), so no kernel sits between two passes.
//   k_cull_finish    ONE workgroup: walks all eight tables to the pattern of rank k, then the threshold of the rule.
//   k_cull_verdict   one lane per point: its blocks that are not over the threshold, in list order; the point rule; per workgroup
//                    the integer sums (surviving points, surviving blocks, blocks over, blocks by the point rule)
//   k_cull_offsets   ONE workgroup: exclusive scan of the workgroup sums, and the totals
//   k_cull_index     one lane per point: scan inside the workgroup -> new point index (or -1), destination of every block (or -1),
//                    keep byte of every block
//   k_cull_gather_obs / k_cull_gather_rows   survivors to FRESH buffers (the engine swaps them in: an in-place parallel compaction
//                    would race): observation arrays with the point index renumbered; rows of xyz, rays, descriptors
// Orders are by IEEE bit pattern read as an unsigned 64-bit integer: numeric order for non-negative doubles, +inf behind every
// finite value, NaN last.  Nothing here adds floating-point numbers; two engines give the same bytes.
// Included by pba_engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pba {

constexpr int kCullThreads = 256;
constexpr int kCullBins = 256;          // one byte per pass
constexpr int kCullPasses = 8;
constexpr int kCullHistGridMax = 512;   // workgroups of a histogram pass (grid-stride beyond)
constexpr int kCullSelWords = 3;        // k_cull_finish: pattern of rank k | threshold (as a pattern) | factor * quantile_cost non-finite
constexpr int kCullTotals = 4;          // k_cull_offsets: surviving points | surviving blocks | blocks over | blocks by the point rule

struct CullSelectParams {
  const uint64_t* v;      // [n] patterns
  uint32_t* hist;         // [kCullPasses][kCullBins], zero before pass 0
  int64_t n;
  uint32_t k;             // rank, 0-based, < n
  int32_t pass;
};

// Inclusive scan of one value per lane over the 256 lanes of the workgroup.  sh: [kCullBins]
__device__ __forceinline__ uint32_t cull_block_scan(uint32_t x, uint32_t* sh) {
  const int t = threadIdx.x;
  sh[t] = x;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < kCullBins; off <<= 1) {
    const uint32_t add = t >= off ? sh[t - off] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const uint32_t r = sh[t];
  __syncthreads();
  return r;
}

// The bucket path through the tables of passes 0 .. passes - 1: `prefix` = those bytes (the highest in the lowest position's place, i.e.
// the value's top 8 * passes bits shifted down), `k` = the rank inside the bucket.  Called by all 256 lanes.  sh: [kCullBins + 2]
__device__ __forceinline__ void cull_walk(const uint32_t* __restrict__ hist, int passes, uint32_t k, uint32_t* sh, uint64_t* prefix, uint32_t* k_out) {
  uint64_t pre = 0;
  for (int p = 0; p < passes; ++p) {
    const uint32_t c = hist[p * kCullBins + threadIdx.x];
    const uint32_t incl = cull_block_scan(c, sh);
    if (incl - c <= k && k < incl) { sh[kCullBins] = threadIdx.x; sh[kCullBins + 1] = k - (incl - c); }      // exactly one lane
    __syncthreads();
    pre = (pre << 8) | sh[kCullBins];
    k = sh[kCullBins + 1];
    __syncthreads();
  }
  *prefix = pre;
  *k_out = k;
}

__global__ __launch_bounds__(kCullThreads) void k_cull_hist(CullSelectParams sp) {
  __shared__ uint32_t sh_walk[kCullBins + 2];
  __shared__ uint32_t sh_bins[kCullBins];
  uint64_t prefix;
  uint32_t k;
  cull_walk(sp.hist, sp.pass, sp.k, sh_walk, &prefix, &k);
  sh_bins[threadIdx.x] = 0;
  __syncthreads();
  const int shift = 56 - 8 * sp.pass;
  int run_bin = -1;
  uint32_t run = 0;
  for (int64_t i = (int64_t)blockIdx.x * kCullThreads + threadIdx.x; i < sp.n; i += (int64_t)gridDim.x * kCullThreads) {
    const uint64_t b = sp.v[i];
    if (sp.pass > 0 && (b >> (shift + 8)) != prefix) continue;
    const int bin = (int)((b >> shift) & 255u);
    if (bin == run_bin) { ++run; continue; }
    if (run) atomicAdd(&sh_bins[run_bin], run);
    run_bin = bin;
    run = 1;
  }
  if (run) atomicAdd(&sh_bins[run_bin], run);
  __syncthreads();
  const uint32_t c = sh_bins[threadIdx.x];
  if (c) atomicAdd(&sp.hist[sp.pass * kCullBins + threadIdx.x], c);
}

// sel[0] = the pattern of rank k; with rule != 0 also sel[1] = threshold, sel[2] = 1 when factor * quantile_cost is not finite
__global__ __launch_bounds__(kCullThreads) void k_cull_finish(CullSelectParams sp, uint64_t* sel, int rule, double min_cost, double factor) {
  __shared__ uint32_t sh_walk[kCullBins + 2];
  uint64_t bits;
  uint32_t k;
  cull_walk(sp.hist, kCullPasses, sp.k, sh_walk, &bits, &k);
  if (threadIdx.x != 0) return;
  sel[0] = bits;
  if (!rule) return;
  const double q = __longlong_as_double((long long)bits);
  double thr = min_cost;
  uint64_t bad = 0;
  if (factor > 0.0) {
    const double fq = factor * q;
    if (!isfinite(fq)) { bad = 1; thr = fq; }
    else thr = fmax(min_cost, fq);
  }
  sel[1] = (uint64_t)__double_as_longlong(thr);
  sel[2] = bad;
}

struct CullParams {
  const double* cost;           // [n_obs] row 5 of the records
  const uint64_t* sel;          // k_cull_finish
  const int32_t* pt_begin;      // [n_points + 1]
  const int32_t* obs_point;     // [n_obs]
  const uint8_t* obs_slot;
  int32_t* pt_cnt;              // [n_points] surviving blocks of the point (0: the point leaves)
  int4* part;                   // [blocks] sums of a workgroup's points: surviving points, surviving blocks, over, by the point rule
  int2* off;                    // [blocks] exclusive scan of part.x, part.y
  int32_t* tot;                 // [kCullTotals]
  int32_t* point_map;           // [n_points]
  int32_t* obs_dst;             // [n_obs]
  uint8_t* keep;                // [n_obs]
  int32_t* obs_point_new;       // [n_obs] gathered
  uint8_t* obs_slot_new;
  int32_t n_points, n_obs, n_part, min_observations;
};

__device__ __forceinline__ bool cull_over(double c, double thr) { return !(c <= thr); }

// Sum of an int4 over the workgroup, in lane 0.  sh: [4][kCullThreads]
__device__ __forceinline__ int4 cull_block_sum(int4 v, int32_t* sh) {
  const int t = threadIdx.x;
  sh[t] = v.x; sh[kCullThreads + t] = v.y; sh[2 * kCullThreads + t] = v.z; sh[3 * kCullThreads + t] = v.w;
  __syncthreads();
  for (int off = kCullThreads / 2; off > 0; off >>= 1) {
    if (t < off)
      for (int c = 0; c < 4; ++c) sh[c * kCullThreads + t] += sh[c * kCullThreads + t + off];
    __syncthreads();
  }
  return make_int4(sh[0], sh[kCullThreads], sh[2 * kCullThreads], sh[3 * kCullThreads]);
}

__global__ __launch_bounds__(kCullThreads) void k_cull_verdict(CullParams cp) {
  __shared__ int32_t sh[4 * kCullThreads];
  const int p = blockIdx.x * kCullThreads + threadIdx.x;
  const double thr = __longlong_as_double((long long)cp.sel[1]);
  int4 mine = make_int4(0, 0, 0, 0);
  if (p < cp.n_points) {
    const int o0 = cp.pt_begin[p], o1 = cp.pt_begin[p + 1];
    int ok = 0;
    for (int o = o0; o < o1; ++o) ok += cull_over(cp.cost[o], thr) ? 0 : 1;
    const bool stays = ok >= cp.min_observations;
    cp.pt_cnt[p] = stays ? ok : 0;
    mine = make_int4(stays ? 1 : 0, stays ? ok : 0, (o1 - o0) - ok, stays ? 0 : ok);
  }
  const int4 s = cull_block_sum(mine, sh);
  if (threadIdx.x == 0) cp.part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kCullThreads) void k_cull_offsets(CullParams cp) {
  __shared__ uint32_t sh[kCullBins];
  uint32_t carry_x = 0, carry_y = 0, sum_z = 0, sum_w = 0;
  for (int base = 0; base < cp.n_part; base += kCullThreads) {
    const int b = base + threadIdx.x;
    const int4 v = b < cp.n_part ? cp.part[b] : make_int4(0, 0, 0, 0);
    const uint32_t ix = cull_block_scan((uint32_t)v.x, sh), iy = cull_block_scan((uint32_t)v.y, sh);
    const uint32_t iz = cull_block_scan((uint32_t)v.z, sh), iw = cull_block_scan((uint32_t)v.w, sh);
    if (b < cp.n_part) cp.off[b] = make_int2((int)(carry_x + ix - (uint32_t)v.x), (int)(carry_y + iy - (uint32_t)v.y));
    sh[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == kCullThreads - 1) { sh[0] = ix; sh[1] = iy; sh[2] = iz; sh[3] = iw; }
    __syncthreads();
    carry_x += sh[0]; carry_y += sh[1]; sum_z += sh[2]; sum_w += sh[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) { cp.tot[0] = (int)carry_x; cp.tot[1] = (int)carry_y; cp.tot[2] = (int)sum_z; cp.tot[3] = (int)sum_w; }
}

__global__ __launch_bounds__(kCullThreads) void k_cull_index(CullParams cp) {
  __shared__ uint32_t sh[kCullBins];
  const int p = blockIdx.x * kCullThreads + threadIdx.x;
  const double thr = __longlong_as_double((long long)cp.sel[1]);
  const int cnt = p < cp.n_points ? cp.pt_cnt[p] : 0;
  const uint32_t stays = cnt > 0 ? 1u : 0u;
  const uint32_t ip = cull_block_scan(stays, sh), io = cull_block_scan((uint32_t)cnt, sh);
  if (p >= cp.n_points) return;
  const int2 off = cp.off[blockIdx.x];
  cp.point_map[p] = stays ? off.x + (int)(ip - stays) : -1;
  int dst = off.y + (int)(io - (uint32_t)cnt);
  const int o0 = cp.pt_begin[p], o1 = cp.pt_begin[p + 1];
  for (int o = o0; o < o1; ++o) {
    const bool k = stays && !cull_over(cp.cost[o], thr);
    cp.keep[o] = k ? 1 : 0;
    cp.obs_dst[o] = k ? dst++ : -1;
  }
}

__global__ __launch_bounds__(kCullThreads) void k_cull_gather_obs(CullParams cp) {
  const int o = blockIdx.x * kCullThreads + threadIdx.x;
  if (o >= cp.n_obs) return;
  const int d = cp.obs_dst[o];
  if (d < 0) return;
  cp.obs_point_new[d] = cp.point_map[cp.obs_point[o]];
  cp.obs_slot_new[d] = cp.obs_slot[o];
}

// dst[map[r]][.] = src[r][.] for every row with map[r] >= 0; one lane per element
template <class T>
__global__ __launch_bounds__(kCullThreads) void k_cull_gather_rows(const T* __restrict__ src, T* __restrict__ dst, const int32_t* __restrict__ map,
                                                                   int32_t n_rows, int32_t row_len) {
  const int64_t total = (int64_t)n_rows * row_len;
  for (int64_t i = (int64_t)blockIdx.x * kCullThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kCullThreads) {
    const int64_t r = i / row_len;
    const int32_t m = map[r];
    if (m >= 0) dst[(int64_t)m * row_len + (i - r * row_len)] = src[i];
  }
}

inline int cull_hist_grid(int64_t n) {
  const int64_t g = (n + 4 * kCullThreads - 1) / (4 * kCullThreads);
  return (int)(g < 1 ? 1 : g > kCullHistGridMax ? kCullHistGridMax : g);
}

// The select, enqueued: zeroed tables, eight passes, the finish.  hist: [kCullPasses][kCullBins]; sel: [kCullSelWords]
inline void cull_enqueue_select(hipStream_t st, const uint64_t* v, int64_t n, uint32_t k, uint32_t* hist, uint64_t* sel, int rule, double min_cost,
                                double factor) {
  (void)hipMemsetAsync(hist, 0, sizeof(uint32_t) * kCullPasses * kCullBins, st);
  CullSelectParams sp{v, hist, n, k, 0};
  const int grid = cull_hist_grid(n);
  for (int p = 0; p < kCullPasses; ++p) {
    sp.pass = p;
    hipLaunchKernelGGL(k_cull_hist, dim3(grid), dim3(kCullThreads), 0, st, sp);
  }
  hipLaunchKernelGGL(k_cull_finish, dim3(1), dim3(kCullThreads), 0, st, sp, sel, rule, min_cost, factor);
}

}  // namespace pba
