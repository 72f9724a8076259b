// pba_point_prior.h -- the point prior (pba_set_point_prior): one extra residual block on every point's parameter block, in information
// form.  With d = X_i - x0_i:
//   E_i = d^T Lambda_i d / 2,   gradient Lambda_i d,   Gauss-Newton block Lambda_i   (constant Jacobian, no loss).
// Lambda_i is stored as the upper triangle row by row (00 01 02 11 12 22: the kPointsSys order) and may be rank deficient (a depth factor
// n n^T / sigma^2) or zero (no prior on that point).  The prior touches V_i, g_i and the cost only, so it is an addend inside the
// one-lane-per-point kernels that form V_i and g_i (k_wide_point<true>, k_points_system<true>, k_cov_point<true>: point_prior_terms below,
// after the observation loop and before scale, damping and factorisation) and an addend to the costs:
//   k_point_prior_cost   E_pts = sum_i E_i at a given point array: per lane in point order, butterfly per wave, the waves in order, one
//                        partial per workgroup; the LAST workgroup to arrive (integer ticket) adds the partials in block order and
//                        adds the sum to *add_to
// No floating-point atomics: two fresh engines give the same bits.  Included by pba_engine.hip after pba_kernels.h.
#pragma once
#include "pba_kernels.h"

namespace pba {

constexpr int kPointPriorThreads = 256;
constexpr int kPointPriorMaxGrid = 256;       // workgroups of k_point_prior_cost at the most (grid-stride beyond 65 536 points): one partial per thread of the last one

// L = Lambda_pt (upper triangle row by row), Ld = Lambda_pt (X - x0_pt), row by row
__device__ __forceinline__ void point_prior_terms(const double* __restrict__ x0, const double* __restrict__ L6, size_t pt, const double X[3],
                                                  double L[6], double Ld[3], double d[3]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) L[k] = L6[6 * pt + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = X[k] - x0[3 * pt + k];
  Ld[0] = L[0] * d[0] + L[1] * d[1] + L[2] * d[2];
  Ld[1] = L[1] * d[0] + L[3] * d[1] + L[4] * d[2];
  Ld[2] = L[2] * d[0] + L[4] * d[1] + L[5] * d[2];
}

struct PointPriorCostParams {
  const double* xyz;             // [n_points][3] the points E is evaluated at
  const double* x0;              // [n_points][3]
  const double* L6;              // [n_points][6]
  double* part;                  // [gridDim.x]
  unsigned int* ticket;          // zero between launches
  double* add_to;                // *add_to += E_pts; may be null
  double* out;                   // *out = E_pts; may be null
  int32_t n_points;
};

__global__ __launch_bounds__(kPointPriorThreads) void k_point_prior_cost(PointPriorCostParams p) {
  __shared__ double s_red[kPointPriorThreads / 64];
  __shared__ double s_part[kPointPriorMaxGrid];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  double E = 0.0;
  for (size_t pt = (size_t)blockIdx.x * kPointPriorThreads + tid; pt < (size_t)p.n_points; pt += (size_t)gridDim.x * kPointPriorThreads) {
    const double X[3] = {p.xyz[3 * pt], p.xyz[3 * pt + 1], p.xyz[3 * pt + 2]};
    double L[6], Ld[3], d[3];
    point_prior_terms(p.x0, p.L6, pt, X, L, Ld, d);
    E += 0.5 * (d[0] * Ld[0] + d[1] * Ld[1] + d[2] * Ld[2]);
  }
  E = wave_sum(E);
  if ((tid & 63) == 0) s_red[tid >> 6] = E;
  __syncthreads();
  if (tid == 0) {
    double v = s_red[0];
#pragma unroll
    for (int w = 1; w < kPointPriorThreads / 64; ++w) v += s_red[w];
    store_agent(p.part + blockIdx.x, v);
    // the partial is ordered before the ticket (release on the way in), the last workgroup's reads after it (acquire)
    const unsigned t = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;      // (uniform per workgroup)
  if (tid < (int)gridDim.x) s_part[tid] = load_agent(p.part + tid);
  __syncthreads();
  if (tid != 0) return;
  *p.ticket = 0;
  double sum = 0.0;
  for (unsigned b = 0; b < gridDim.x; ++b) sum += s_part[b];      // block order
  if (p.add_to) *p.add_to += sum;
  if (p.out) *p.out = sum;
}

}  // namespace pba
