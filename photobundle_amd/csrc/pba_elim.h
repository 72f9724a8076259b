// pba_elim.h -- the point elimination that pba_covariance (pba_cov.h) and pba_marginalize (pba_prior.h) share: the points leave the
// undamped, unscaled normal equations of the per-observation records of a Jacobian pass, and a dense camera system is left.  Every
// point block is factorised in its unit-diagonal form D^-1/2 V D^-1/2 (D = diag V), so that the reported pivots are scale-free.
//   elim_observation, elim_times_factor   the products of one observation: Ac, Ap, M Ap, and G = (M Ap) X^T
//   elim_add_point_block                  V += Ap^T M Ap of one observation
//   elim_factor_point                     the equilibrated 3x3 (1x1) Cholesky of V: ok, smallest pivot, P = V^-1 and its factor X
//                                         (k_marg_point keeps this arithmetic written out: see there)
//   elim_point_partial                    the workgroup row smallest pivot | first failing point | sums of a one-lane-per-point kernel
//   k_elim_pair                           one workgroup per pair of camera columns a <= b: S(a, b) = [a == b] U_a - sum_p W_a P W_b^T,
//                                         dense, both triangles; P enters as its triangular factor (P = X^T X); two forms of one body:
//                                         the points of a slot mask only (marginalisation), or every point with the inverse-depth
//                                         chain rule, no elimination at all and the diagonal pairs only as options (covariance)
// The calls run once per window and are not in the LM loop: the kernels recompute the projection Jacobians where they need them and
// keep nothing per observation.  Every sum has a fixed order (per lane in point order, butterfly per wave, the waves in order; no
// floating-point atomics).  Included by pba_cov.h and pba_prior.h.
#pragma once
#include "pba_kernels.h"

namespace pba {

constexpr int kElimThreads = 256;
constexpr int kElimWaves = kElimThreads / 64;
// a workgroup row of a point kernel: smallest pivot | first failing point (kElimNone: none) | n_sums sums, the cost first
constexpr int elim_part_width(int n_sums) { return 2 + n_sums; }
constexpr double kElimNone = 1e300;    // "no failing index" (an index is compared with fmin)

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}

__device__ __forceinline__ bool elim_pivot_ok(double d) { return d > 0.0 && isfinite(d); }

// one of the observations [o0, o1) of a point is in a slot of the mask
__device__ __forceinline__ bool elim_in_set(const uint8_t* __restrict__ obs_slot, int o0, int o1, uint32_t slot_mask) {
  bool in = false;
  for (int o = o0; o < o1; ++o) in = in || ((slot_mask >> obs_slot[o]) & 1u);
  return in;
}

// Ac, M Ap and M of observation o (point X, camera g); rays: the inverse-depth chain rule on the point Jacobian
__device__ __forceinline__ void elim_observation(const CamGeom& g, const double X[3], const double* rays, const double qd[3],
                                                 const double* __restrict__ rec, int64_t rs, int o, double fx, double fy,
                                                 double Ac[2][6], double MAp[2][3], double Ap[2][3], double M[3]) {
  double xw[3];
  transform_point(g, X, xw);
  projection_jacobians(g, X, xw, fx, fy, Ac, Ap);
  point_jacobian(rays, qd, Ap);
  M[0] = rec[o]; M[1] = rec[rs + o]; M[2] = rec[2 * rs + o];
#pragma unroll
  for (int k = 0; k < 3; ++k) { MAp[0][k] = M[0] * Ap[0][k] + M[1] * Ap[1][k]; MAp[1][k] = M[1] * Ap[0][k] + M[2] * Ap[1][k]; }
}

// G = B X^T for a 2x3 B and the lower triangular X (00 10 11 20 21 22)
__device__ __forceinline__ void elim_times_factor(const double B[2][3], const double Xm[6], double G[2][3]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    G[r][0] = B[r][0] * Xm[0];
    G[r][1] = B[r][0] * Xm[1] + B[r][1] * Xm[2];
    G[r][2] = B[r][0] * Xm[3] + B[r][1] * Xm[4] + B[r][2] * Xm[5];
  }
}

// V += Ap^T (M Ap) of one observation; V: upper triangle row by row (00 01 02 11 12 22).  A point kernel adds its observations in list order
__device__ __forceinline__ void elim_add_point_block(const double Ap[2][3], const double MAp[2][3], double V[6]) {
  V[0] += Ap[0][0] * MAp[0][0] + Ap[1][0] * MAp[1][0];
  V[1] += Ap[0][0] * MAp[0][1] + Ap[1][0] * MAp[1][1];
  V[2] += Ap[0][0] * MAp[0][2] + Ap[1][0] * MAp[1][2];
  V[3] += Ap[0][1] * MAp[0][1] + Ap[1][1] * MAp[1][1];
  V[4] += Ap[0][1] * MAp[0][2] + Ap[1][1] * MAp[1][2];
  V[5] += Ap[0][2] * MAp[0][2] + Ap[1][2] * MAp[1][2];
}

// The point block V (dim free parameters: 3, or 1) in its unit-diagonal form -- a10 a20 a21 are correlations, the pivots are 1, d1, d2.
// Returns whether every pivot is positive and finite; then piv = the smallest one (left alone otherwise and for dim == 1),
// Pm = V^-1 (upper triangle row by row) and Xm its factor, V^-1 = X^T X, X = L^-1 D^-1/2 lower triangular (00 10 11 20 21 22).
// The caller passes Pm and Xm zeroed: they stay so after a failure, and dim == 1 gives Pm[0] alone.
__device__ __forceinline__ bool elim_factor_point(const double V[6], int dim, double& piv, double Pm[6], double Xm[6]) {
  bool ok = elim_pivot_ok(V[0]);
  if (dim == 1) {
    if (ok) Pm[0] = 1.0 / V[0];
    return ok;
  }
  ok = ok && elim_pivot_ok(V[3]) && elim_pivot_ok(V[5]);
  const double e0 = 1.0 / sqrt(ok ? V[0] : 1.0), e1 = 1.0 / sqrt(ok ? V[3] : 1.0), e2 = 1.0 / sqrt(ok ? V[5] : 1.0);
  const double l10 = V[1] * e0 * e1, l20 = V[2] * e0 * e2, a21 = V[4] * e1 * e2;
  const double d1 = 1.0 - l10 * l10;
  ok = ok && elim_pivot_ok(d1);
  const double l11 = sqrt(ok ? d1 : 1.0);
  const double l21 = (a21 - l20 * l10) / l11;
  const double d2 = 1.0 - l20 * l20 - l21 * l21;
  ok = ok && elim_pivot_ok(d2);
  const double l22 = sqrt(ok ? d2 : 1.0);
  if (ok) {
    piv = fmin(d1, d2);
    // X = L^-1 (lower), inverse = X^T X, then the scales again
    const double x11 = 1.0 / l11, x22 = 1.0 / l22;
    const double x10 = -l10 * x11;
    const double x21 = -l21 * x11 * x22;
    const double x20 = -(l20 + l21 * x10) * x22;
    Pm[0] = e0 * e0 * (1.0 + x10 * x10 + x20 * x20);
    Pm[1] = e0 * e1 * (x10 * x11 + x20 * x21);
    Pm[2] = e0 * e2 * (x20 * x22);
    Pm[3] = e1 * e1 * (x11 * x11 + x21 * x21);
    Pm[4] = e1 * e2 * (x21 * x22);
    Pm[5] = e2 * e2 * (x22 * x22);
    Xm[0] = e0; Xm[1] = x10 * e0; Xm[2] = x11 * e1; Xm[3] = x20 * e0; Xm[4] = x21 * e1; Xm[5] = x22 * e2;
  }
  return ok;
}

// The workgroup row of a one-lane-per-point kernel, row[elim_part_width(kSums)], kSums = 1 or 2 (sum1 is not read when kSums == 1).
// Butterfly per wave, the waves in order.
template <int kSums>
__device__ __forceinline__ void elim_point_partial(double piv, double bad, double sum0, double sum1, double* __restrict__ row) {
  static_assert(kSums == 1 || kSums == 2, "one or two sums");
  __shared__ double s_red[kElimWaves][elim_part_width(kSums)];
  const int tid = threadIdx.x, wave = tid >> 6;
  piv = wave_min(piv); bad = wave_min(bad); sum0 = wave_sum(sum0);
  if constexpr (kSums > 1) sum1 = wave_sum(sum1);
  if ((tid & 63) == 0) {
    s_red[wave][0] = piv; s_red[wave][1] = bad; s_red[wave][2] = sum0;
    if constexpr (kSums > 1) s_red[wave][3] = sum1;
  }
  __syncthreads();
  if (tid == 0) {
    double m = s_red[0][0], b = s_red[0][1], c = s_red[0][2], q = 0.0;
    if constexpr (kSums > 1) q = s_red[0][3];
    for (int w = 1; w < kElimWaves; ++w) {
      m = fmin(m, s_red[w][0]); b = fmin(b, s_red[w][1]); c += s_red[w][2];
      if constexpr (kSums > 1) q += s_red[w][3];
    }
    row[0] = m; row[1] = b; row[2] = c;
    if constexpr (kSums > 1) row[3] = q;
  }
}

struct ElimPairParams {
  const double* xyz;
  const double* rays;            // inverse-depth variant, else null
  const CamGeom* geom;
  const double* rec;             // [6][rec_stride] records of the Jacobian pass
  const int32_t* pt_begin;
  const uint8_t* obs_slot;
  const double* X;               // [n_points][6] factor of V^-1 (a point kernel); null: no elimination (pose-only mode, S = blockdiag U, diag_only)
  const double* z;               // [n_points][3] X g_p (k_marg_grad), else null
  double* S;                     // [n][n] row-major, n = 6 n_cols, both triangles from the one computed value
  double* r;                     // [n] reduced gradient (k_marg_grad), else null
  int64_t rec_stride;
  int32_t n_points, n_cols;
  int32_t diag_only;             // the grid holds the diagonal pairs (a, a) only; the rest of S was cleared by the caller
  uint32_t point_mask;           // kSubset: the points with an observation in a slot of the mask only
  double fx, fy;
  uint8_t slot_of_col[kMaxFramesWide];
};

// Workgroup q: the pair (a, b), a <= b, of camera columns enumerated row by row (diag_only: the pair (q, q)).  Its lanes walk the points (stride kElimThreads); a
// point contributes for every observation l in slot(a) and m in slot(b): -Ac_l^T (G_l G_m^T) Ac_m with G = (M Ap) X^T, and on the
// diagonal U_l = Ac_l^T M Ac_l.  The elimination goes through the triangular factor X of V^-1, not through V^-1 itself: that is the
// Cholesky elimination of the point from H, backward stable, so a singular direction of H (an open gauge) comes out as a pivot at
// the rounding level of H and not at eps x cond(V).  Sums: per lane in point order, butterfly per wave, the waves in order.
// kSubset: the marginalisation's form -- the points of point_mask only, world points, X given, every pair; else the covariance's form,
// every point, with rays, a null X and diag_only as run-time options.  (One form with all four at run time cost the marginalisation
// 3 % of its pair kernel: profiles/refactor/elimination_ab_timing.txt.)
template <bool kSubset>
__global__ __launch_bounds__(kElimThreads) void k_elim_pair(ElimPairParams p) {
  const double* rays = kSubset ? nullptr : p.rays;
  const bool eliminate = kSubset || p.X != nullptr;
  __shared__ CamGeom s_geom[2];
  __shared__ double s_red[kElimWaves][36];
  const int tid = threadIdx.x;
  const int nc = p.n_cols, n = 6 * nc;
  int a = 0, rem = blockIdx.x;
  if (!kSubset && p.diag_only) { a = blockIdx.x; rem = 0; }
  else while (rem >= nc - a) { rem -= nc - a; ++a; }
  const int b = a + rem;
  const int sa = p.slot_of_col[a], sb = p.slot_of_col[b];
  if (tid == 0) { s_geom[0] = p.geom[sa]; s_geom[1] = p.geom[sb]; }
  __syncthreads();
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  for (int pt = tid; pt < p.n_points; pt += kElimThreads) {
    const int o0 = p.pt_begin[pt], o1 = p.pt_begin[pt + 1];
    bool seen_a = false, seen_b = false;
    for (int o = o0; o < o1; ++o) { const int s = p.obs_slot[o]; seen_a = seen_a || s == sa; seen_b = seen_b || s == sb; }
    if (!seen_a || !seen_b || (kSubset && !elim_in_set(p.obs_slot, o0, o1, p.point_mask))) continue;
    const double prm[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
    double X[3], qd[3], Xm[6] = {0, 0, 0, 0, 0, 0};
    point_world(rays, pt, prm, X, qd);
    if (eliminate) {
#pragma unroll
      for (int k = 0; k < 6; ++k) Xm[k] = p.X[6 * (size_t)pt + k];
    }
    for (int l = o0; l < o1; ++l) {
      if (p.obs_slot[l] != sa) continue;
      double Aca[2][6], MApa[2][3], Apa[2][3], Ma[3];
      elim_observation(s_geom[0], X, rays, qd, p.rec, p.rec_stride, l, p.fx, p.fy, Aca, MApa, Apa, Ma);
      if (a == b) {
        double MAc[2][6];
#pragma unroll
        for (int j = 0; j < 6; ++j) { MAc[0][j] = Ma[0] * Aca[0][j] + Ma[1] * Aca[1][j]; MAc[1][j] = Ma[1] * Aca[0][j] + Ma[2] * Aca[1][j]; }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) acc[6 * i + j] += Aca[0][i] * MAc[0][j] + Aca[1][i] * MAc[1][j];
      }
      if (!eliminate) continue;
      double Ga[2][3];
      elim_times_factor(MApa, Xm, Ga);
      for (int m = o0; m < o1; ++m) {
        if (p.obs_slot[m] != sb) continue;
        double Acb[2][6], MApb[2][3], Apb[2][3], Mb[3];
        elim_observation(s_geom[1], X, rays, qd, p.rec, p.rec_stride, m, p.fx, p.fy, Acb, MApb, Apb, Mb);
        double Gb[2][3], N[2][2], Z[2][6];
        elim_times_factor(MApb, Xm, Gb);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int t = 0; t < 2; ++t) N[r][t] = Ga[r][0] * Gb[t][0] + Ga[r][1] * Gb[t][1] + Ga[r][2] * Gb[t][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int j = 0; j < 6; ++j) Z[r][j] = N[r][0] * Acb[0][j] + N[r][1] * Acb[1][j];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) acc[6 * i + j] -= Aca[0][i] * Z[0][j] + Aca[1][i] * Z[1][j];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 36; ++k) {
    const double v = wave_sum(acc[k]);
    if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < 36) {
    double v = s_red[0][tid];
#pragma unroll
    for (int w = 1; w < kElimWaves; ++w) v += s_red[w][tid];
    const int i = tid / 6, j = tid - 6 * i;
    // block (a, b) and its mirror; a diagonal block keeps its lower triangle on both sides (the dense Cholesky kernels read the lower one)
    if (a != b) {
      p.S[(size_t)(6 * a + i) * n + 6 * b + j] = v;
      p.S[(size_t)(6 * b + j) * n + 6 * a + i] = v;
    } else if (i >= j) {
      p.S[(size_t)(6 * a + i) * n + 6 * a + j] = v;
      p.S[(size_t)(6 * a + j) * n + 6 * a + i] = v;
    }
  }
}

}  // namespace pba
