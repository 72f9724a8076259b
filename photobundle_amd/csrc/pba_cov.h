// pba_cov.h -- covariance output (pba_covariance): blocks of (J^T J)^-1 of the reduced program of the mode that is on, from the
// per-observation records of a Jacobian pass.  No damping and no Jacobi scaling enter the result; every block is factorised in its
// unit-diagonal form D^-1/2 A D^-1/2 (D = diag A), so that the reported pivots are scale-free, and the inverse is unscaled again.
//   k_cov_point    one lane per point: V = sum Ap^T M Ap in list order, P = V^-1 through the equilibrated 3x3 (1x1) Cholesky, the
//                  smallest pivot, the first failing point and the program cost of every workgroup
//   k_cov_schur    one workgroup per pair of camera columns a <= b: S(a, b) = [a == b] U_a - sum_p W_a P W_b^T, dense, both triangles;
//                  P enters as its triangular factor (P = X^T X)
//   k_cov_invert   ONE workgroup: the packed lower triangle of the unit-diagonal S in LDS, in place Cholesky -> L^-1 -> L^-T L^-1,
//                  the smallest pivot, the dense symmetric inverse unscaled into HBM
//   k_cov_points   one lane per point: P + sum_{l, m} Y_l^T Sigma_cc[a_l, a_m] Y_m, Y_l = W_l P, observations in list order
// The call runs once per solve and is not in the LM loop: the kernels recompute the projection Jacobians where they need them and
// keep nothing per observation.  Every sum has a fixed order (no floating-point atomics).  Everything is written to buffers that
// belong to this header: nothing of the LM state (point scales, point records, packed system, scalar block) is touched.
// Included by pba_engine.hip after pba_kernels.h and pba_solve.h.
#pragma once
#include "pba_kernels.h"

namespace pba {

constexpr int kCovThreads = 256;
constexpr int kCovWaves = kCovThreads / 64;
constexpr int kCovPart = 3;            // per workgroup of k_cov_point: smallest pivot | first failing point (kCovNone: none) | cost
constexpr double kCovNone = 1e300;     // "no failing index" (an index is compared with fmin)
constexpr int kCovInvertT = 1024;

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}

__device__ __forceinline__ bool cov_pivot_ok(double d) { return d > 0.0 && isfinite(d); }

// Ac, M Ap and M of observation o (point X, camera g); rays: the inverse-depth chain rule on the point Jacobian
__device__ __forceinline__ void cov_observation(const CamGeom& g, const double X[3], const double* rays, const double qd[3],
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
__device__ __forceinline__ void cov_times_factor(const double B[2][3], const double Xm[6], double G[2][3]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    G[r][0] = B[r][0] * Xm[0];
    G[r][1] = B[r][0] * Xm[1] + B[r][1] * Xm[2];
    G[r][2] = B[r][0] * Xm[3] + B[r][1] * Xm[4] + B[r][2] * Xm[5];
  }
}

struct CovPointParams {
  const double* xyz;
  const double* rays;            // inverse-depth variant, else null
  const CamGeom* geom;
  const double* rec;             // [6][rec_stride] records of the Jacobian pass
  const int32_t* pt_begin;
  const uint8_t* obs_slot;
  double* P;                     // [n_points][6] V^-1, upper triangle row by row (00 01 02 11 12 22); null: the points are constant
  double* X;                     // [n_points][6] its factor, V^-1 = X^T X, X lower triangular row by row (00 10 11 20 21 22); may be null
  double* pp;                    // [n_points][9] point covariance = P (structure-only mode), else null
  double* part;                  // [gridDim.x][kCovPart]
  int64_t rec_stride;
  int32_t n_points, n_frames, dim;   // dim: free parameters per point (3, or 1 in the inverse-depth mode)
  uint32_t cost_mask;            // slots whose residual blocks are in the program
  double fx, fy;
};

__global__ __launch_bounds__(kCovThreads) void k_cov_point(CovPointParams p) {
  __shared__ CamGeom s_geom[kMaxFramesWide];
  __shared__ double s_red[kCovWaves][kCovPart];
  const int tid = threadIdx.x;
  stage_geom<kCovThreads, false, kMaxFramesWide>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const int pt = blockIdx.x * kCovThreads + tid;
  double piv = 1.0, bad = kCovNone, cost = 0.0;
  if (pt < p.n_points) {
    const double prm[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
    double X[3], qd[3];
    point_world(p.rays, pt, prm, X, qd);
    double V[6] = {0, 0, 0, 0, 0, 0};
    const int o1 = p.pt_begin[pt + 1];
    for (int o = p.pt_begin[pt]; o < o1; ++o) {      // list order
      const int slot = p.obs_slot[o];
      if ((p.cost_mask >> slot) & 1u) cost += p.rec[5 * p.rec_stride + o];
      if (!p.P) continue;
      double Ac[2][6], MAp[2][3], Ap[2][3], M[3];
      cov_observation(s_geom[slot], X, p.rays, qd, p.rec, p.rec_stride, o, p.fx, p.fy, Ac, MAp, Ap, M);
      V[0] += Ap[0][0] * MAp[0][0] + Ap[1][0] * MAp[1][0];
      V[1] += Ap[0][0] * MAp[0][1] + Ap[1][0] * MAp[1][1];
      V[2] += Ap[0][0] * MAp[0][2] + Ap[1][0] * MAp[1][2];
      V[3] += Ap[0][1] * MAp[0][1] + Ap[1][1] * MAp[1][1];
      V[4] += Ap[0][1] * MAp[0][2] + Ap[1][1] * MAp[1][2];
      V[5] += Ap[0][2] * MAp[0][2] + Ap[1][2] * MAp[1][2];
    }
    if (p.P) {
      double Pm[6] = {0, 0, 0, 0, 0, 0}, Xm[6] = {0, 0, 0, 0, 0, 0};
      bool ok = cov_pivot_ok(V[0]);
      if (p.dim == 1) {
        if (ok) Pm[0] = 1.0 / V[0];
      } else {
        ok = ok && cov_pivot_ok(V[3]) && cov_pivot_ok(V[5]);
        // unit-diagonal block: a10 a20 a21 are correlations, the pivots are 1, d1, d2
        const double e0 = 1.0 / sqrt(ok ? V[0] : 1.0), e1 = 1.0 / sqrt(ok ? V[3] : 1.0), e2 = 1.0 / sqrt(ok ? V[5] : 1.0);
        const double l10 = V[1] * e0 * e1, l20 = V[2] * e0 * e2, a21 = V[4] * e1 * e2;
        const double d1 = 1.0 - l10 * l10;
        ok = ok && cov_pivot_ok(d1);
        const double l11 = sqrt(ok ? d1 : 1.0);
        const double l21 = (a21 - l20 * l10) / l11;
        const double d2 = 1.0 - l20 * l20 - l21 * l21;
        ok = ok && cov_pivot_ok(d2);
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
      }
      if (!ok) bad = (double)pt;
#pragma unroll
      for (int k = 0; k < 6; ++k) p.P[6 * (size_t)pt + k] = Pm[k];
      if (p.X) {
#pragma unroll
        for (int k = 0; k < 6; ++k) p.X[6 * (size_t)pt + k] = Xm[k];
      }
      if (p.pp) {
        double* o9 = p.pp + 9 * (size_t)pt;
        o9[0] = Pm[0]; o9[1] = Pm[1]; o9[2] = Pm[2]; o9[3] = Pm[1]; o9[4] = Pm[3]; o9[5] = Pm[4]; o9[6] = Pm[2]; o9[7] = Pm[4]; o9[8] = Pm[5];
      }
    }
  }
  // workgroup partials: butterfly per wave, the waves in order
  piv = wave_min(piv); bad = wave_min(bad); cost = wave_sum(cost);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = piv; s_red[tid >> 6][1] = bad; s_red[tid >> 6][2] = cost; }
  __syncthreads();
  if (tid == 0) {
    double m = s_red[0][0], b = s_red[0][1], c = s_red[0][2];
    for (int w = 1; w < kCovWaves; ++w) { m = fmin(m, s_red[w][0]); b = fmin(b, s_red[w][1]); c += s_red[w][2]; }
    p.part[kCovPart * blockIdx.x] = m; p.part[kCovPart * blockIdx.x + 1] = b; p.part[kCovPart * blockIdx.x + 2] = c;
  }
}

struct CovSchurParams {
  const double* xyz;
  const double* rays;
  const CamGeom* geom;
  const double* rec;
  const int32_t* pt_begin;
  const uint8_t* obs_slot;
  const double* X;               // [n_points][6] factor of V^-1 (k_cov_point); null: no elimination (pose-only mode, S = blockdiag U, diag_only)
  double* S;                     // [n][n] row-major, n = 6 n_cols
  int64_t rec_stride;
  int32_t n_points, n_frames, n_cols;
  int32_t diag_only;             // the grid holds the diagonal pairs (a, a) only; the rest of S was cleared by the caller
  double fx, fy;
  uint8_t slot_of_col[kMaxFramesWide];
};

// Workgroup q: the pair (a, b), a <= b, of camera columns enumerated row by row (diag_only: the pair (q, q)).  Its lanes walk the points (stride kCovThreads); a
// point contributes for every observation l in slot(a) and m in slot(b): -Ac_l^T (G_l G_m^T) Ac_m with G = (M Ap) X^T, and on the
// diagonal U_l = Ac_l^T M Ac_l.  The elimination goes through the triangular factor X of V^-1, not through V^-1 itself: that is the
// Cholesky elimination of the point from H, backward stable, so a singular direction of H (an open gauge) comes out as a pivot at
// the rounding level of H and not at eps x cond(V).  Sums: per lane in point order, butterfly per wave, the waves in order.
__global__ __launch_bounds__(kCovThreads) void k_cov_schur(CovSchurParams p) {
  __shared__ CamGeom s_geom[2];
  __shared__ double s_red[kCovWaves][36];
  const int tid = threadIdx.x;
  const int nc = p.n_cols, n = 6 * nc;
  int a = 0, rem = blockIdx.x;
  if (p.diag_only) { a = blockIdx.x; rem = 0; }
  else while (rem >= nc - a) { rem -= nc - a; ++a; }
  const int b = a + rem;
  const int sa = p.slot_of_col[a], sb = p.slot_of_col[b];
  if (tid == 0) { s_geom[0] = p.geom[sa]; s_geom[1] = p.geom[sb]; }
  __syncthreads();
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  for (int pt = tid; pt < p.n_points; pt += kCovThreads) {
    const int o0 = p.pt_begin[pt], o1 = p.pt_begin[pt + 1];
    bool seen_a = false, seen_b = false;
    for (int o = o0; o < o1; ++o) { const int s = p.obs_slot[o]; seen_a = seen_a || s == sa; seen_b = seen_b || s == sb; }
    if (!seen_a || !seen_b) continue;
    const double prm[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
    double X[3], qd[3], Xm[6] = {0, 0, 0, 0, 0, 0};
    point_world(p.rays, pt, prm, X, qd);
    if (p.X) {
#pragma unroll
      for (int k = 0; k < 6; ++k) Xm[k] = p.X[6 * (size_t)pt + k];
    }
    for (int l = o0; l < o1; ++l) {
      if (p.obs_slot[l] != sa) continue;
      double Aca[2][6], MApa[2][3], Apa[2][3], Ma[3];
      cov_observation(s_geom[0], X, p.rays, qd, p.rec, p.rec_stride, l, p.fx, p.fy, Aca, MApa, Apa, Ma);
      if (a == b) {
        double MAc[2][6];
#pragma unroll
        for (int j = 0; j < 6; ++j) { MAc[0][j] = Ma[0] * Aca[0][j] + Ma[1] * Aca[1][j]; MAc[1][j] = Ma[1] * Aca[0][j] + Ma[2] * Aca[1][j]; }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) acc[6 * i + j] += Aca[0][i] * MAc[0][j] + Aca[1][i] * MAc[1][j];
      }
      if (!p.X) continue;
      double Ga[2][3];
      cov_times_factor(MApa, Xm, Ga);
      for (int m = o0; m < o1; ++m) {
        if (p.obs_slot[m] != sb) continue;
        double Acb[2][6], MApb[2][3], Apb[2][3], Mb[3];
        cov_observation(s_geom[1], X, p.rays, qd, p.rec, p.rec_stride, m, p.fx, p.fy, Acb, MApb, Apb, Mb);
        double Gb[2][3], N[2][2], Z[2][6];
        cov_times_factor(MApb, Xm, Gb);
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
    for (int w = 1; w < kCovWaves; ++w) v += s_red[w][tid];
    const int i = tid / 6, j = tid - 6 * i;
    // block (a, b) and its mirror; a diagonal block keeps its lower triangle on both sides (k_cov_invert reads the lower one)
    if (a != b) {
      p.S[(size_t)(6 * a + i) * n + 6 * b + j] = v;
      p.S[(size_t)(6 * b + j) * n + 6 * a + i] = v;
    } else if (i >= j) {
      p.S[(size_t)(6 * a + i) * n + 6 * a + j] = v;
      p.S[(size_t)(6 * a + j) * n + 6 * a + i] = v;
    }
  }
}

// =====================================================================================================
// Inverse of the symmetric n x n matrix S (n <= 192): ONE workgroup, the packed lower triangle of the unit-diagonal matrix
// D^-1/2 S D^-1/2 in LDS (row r at tri_index(r): 148 KB at n = 192) plus the n scales.  Three in-place sweeps:
//   1. right-looking Cholesky, one column at a time; every thread reads the pivot, so the smallest one needs no reduction;
//   2. X = L^-1, rows in ascending order: row i needs L's row i and the finished rows above it;
//   3. X^T X, rows in ascending order: entry (i, j) sums X(k, i) X(k, j) over k >= i, rows that are not yet overwritten.
// A pivot that is not positive or not finite ends the kernel: info = {smallest pivot so far, its column}, C is not written.
// =====================================================================================================
__host__ __device__ inline size_t cov_invert_smem_bytes(int n) { return sizeof(double) * ((size_t)tri_index(n) + (size_t)n); }

struct CovInvertParams {
  const double* S;               // [n][n] (lower triangle read)
  double* C;                     // [n][n] the inverse, symmetric bit for bit
  double* info;                  // [2] smallest pivot of the unit-diagonal matrix | failing column, -1: none
  int32_t n;
};

__global__ __launch_bounds__(kCovInvertT) void k_cov_invert(CovInvertParams p) {
  extern __shared__ __attribute__((aligned(16))) char cov_smem[];
  const int n = p.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* A = reinterpret_cast<double*>(cov_smem);     // packed lower triangle
  double* dinv = A + tri_index(n);                     // [n] 1 / sqrt(S_ii)
  __shared__ int s_bad;
  if (tid == 0) s_bad = -1;
  __syncthreads();
  if (tid < n) {
    const double d = p.S[(size_t)tid * n + tid];
    if (!cov_pivot_ok(d)) atomicMax(&s_bad, n - 1 - tid);      // (integer, order-free: the FIRST bad diagonal entry wins)
    dinv[tid] = 1.0 / sqrt(cov_pivot_ok(d) ? d : 1.0);
  }
  __syncthreads();
  if (s_bad >= 0) {
    if (tid == 0) { p.info[0] = 0.0; p.info[1] = (double)(n - 1 - s_bad); }
    return;
  }
  for (int r = wave; r < n; r += kCovInvertT / 64)
    for (int c = lane; c <= r; c += 64) A[tri_index(r) + c] = (r == c) ? 1.0 : p.S[(size_t)r * n + c] * dinv[r] * dinv[c];
  __syncthreads();
  // ---- 1. A = L L^T ---------------------------------------------------------------------------------------------------
  double piv = 1.0;
  for (int j = 0; j < n; ++j) {
    const double d = A[tri_index(j) + j];      // (uniform: every thread takes the same decision)
    if (!cov_pivot_ok(d)) {
      if (tid == 0) { p.info[0] = piv; p.info[1] = (double)j; }
      return;
    }
    piv = fmin(piv, d);
    const double ljj = sqrt(d);
    __syncthreads();                           // every thread has read the pivot
    const int r = j + tid;
    if (r == j) A[tri_index(j) + j] = ljj;
    else if (r < n) A[tri_index(r) + j] /= ljj;
    __syncthreads();
    for (int rr = j + 1 + wave; rr < n; rr += kCovInvertT / 64) {
      const double lrj = A[tri_index(rr) + j];
      for (int c = j + 1 + lane; c <= rr; c += 64) A[tri_index(rr) + c] -= lrj * A[tri_index(c) + j];
    }
    __syncthreads();
  }
  // ---- 2. X = L^-1 -----------------------------------------------------------------------------------------------------
  for (int i = 0; i < n; ++i) {
    const double xii = 1.0 / A[tri_index(i) + i];
    double x = xii;
    if (tid < i) {
      double s = 0.0;
      for (int k = tid; k < i; ++k) s += A[tri_index(i) + k] * A[tri_index(k) + tid];
      x = -s * xii;
    }
    __syncthreads();                           // row i of L has been read
    if (tid <= i) A[tri_index(i) + tid] = x;
    __syncthreads();
  }
  // ---- 3. X^T X --------------------------------------------------------------------------------------------------------
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
    if (tid <= i)
      for (int k = i; k < n; ++k) s += A[tri_index(k) + i] * A[tri_index(k) + tid];
    __syncthreads();                           // row i of X has been read
    if (tid <= i) A[tri_index(i) + tid] = s;
    __syncthreads();
  }
  // ---- unscale, both triangles from the one stored value ---------------------------------------------------------------
  for (int r = wave; r < n; r += kCovInvertT / 64)
    for (int c = lane; c <= r; c += 64) {
      const double v = A[tri_index(r) + c] * dinv[r] * dinv[c];
      p.C[(size_t)r * n + c] = v;
      p.C[(size_t)c * n + r] = v;
    }
  if (tid == 0) { p.info[0] = piv; p.info[1] = -1.0; }
}

struct CovPointsParams {
  const double* xyz;
  const CamGeom* geom;
  const double* rec;
  const int32_t* pt_begin;
  const uint8_t* obs_slot;
  const double* P;               // [n_points][6]
  const double* C;               // [n][n] camera covariance (k_cov_invert)
  double* pp;                    // [n_points][9]
  int64_t rec_stride;
  int32_t n_points, n_frames, n;
  double fx, fy;
  int8_t col_of_slot[kMaxFramesWide];      // camera column of a slot, -1: constant
};

// Y = W P = Ac^T ((M Ap) P), 6x3
__device__ __forceinline__ void cov_point_factor(const CamGeom& g, const double X[3], const double* __restrict__ rec, int64_t rs, int o,
                                                 double fx, double fy, const double Pm[6], double Y[6][3]) {
  double Ac[2][6], MAp[2][3], Ap[2][3], M[3], Q[2][3];
  cov_observation(g, X, nullptr, nullptr, rec, rs, o, fx, fy, Ac, MAp, Ap, M);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    Q[r][0] = MAp[r][0] * Pm[0] + MAp[r][1] * Pm[1] + MAp[r][2] * Pm[2];
    Q[r][1] = MAp[r][0] * Pm[1] + MAp[r][1] * Pm[3] + MAp[r][2] * Pm[4];
    Q[r][2] = MAp[r][0] * Pm[2] + MAp[r][1] * Pm[4] + MAp[r][2] * Pm[5];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) Y[i][k] = Ac[0][i] * Q[0][k] + Ac[1][i] * Q[1][k];
}

// One lane per point (full mode, world points).  The double loop over the point's free-camera observations recomputes Y_m inside:
// at most 32 x 32 small products per point, once per solve.  A point seen by constant cameras only keeps P.
__global__ __launch_bounds__(kCovThreads) void k_cov_points(CovPointsParams p) {
  __shared__ CamGeom s_geom[kMaxFramesWide];
  const int tid = threadIdx.x;
  stage_geom<kCovThreads, false, kMaxFramesWide>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const int pt = blockIdx.x * kCovThreads + tid;
  if (pt >= p.n_points) return;
  const double X[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
  double Pm[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) Pm[k] = p.P[6 * (size_t)pt + k];
  double out[6] = {Pm[0], Pm[1], Pm[2], Pm[3], Pm[4], Pm[5]};      // upper triangle row by row
  const int o0 = p.pt_begin[pt], o1 = p.pt_begin[pt + 1];
  for (int l = o0; l < o1; ++l) {
    const int sl = p.obs_slot[l], cl = p.col_of_slot[sl];
    if (cl < 0) continue;
    double Yl[6][3], Z[6][3];
    cov_point_factor(s_geom[sl], X, p.rec, p.rec_stride, l, p.fx, p.fy, Pm, Yl);
#pragma unroll
    for (int i = 0; i < 6; ++i) { Z[i][0] = 0.0; Z[i][1] = 0.0; Z[i][2] = 0.0; }
    for (int m = o0; m < o1; ++m) {
      const int sm = p.obs_slot[m], cm = p.col_of_slot[sm];
      if (cm < 0) continue;
      double Ym[6][3];
      cov_point_factor(s_geom[sm], X, p.rec, p.rec_stride, m, p.fx, p.fy, Pm, Ym);
      const double* Cb = p.C + (size_t)(6 * cl) * p.n + 6 * cm;      // block (a_l, a_m), read through L2 by every lane
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const double c = Cb[(size_t)i * p.n + j];
          Z[i][0] += c * Ym[j][0]; Z[i][1] += c * Ym[j][1]; Z[i][2] += c * Ym[j][2];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      out[0] += Yl[i][0] * Z[i][0]; out[1] += Yl[i][0] * Z[i][1]; out[2] += Yl[i][0] * Z[i][2];
      out[3] += Yl[i][1] * Z[i][1]; out[4] += Yl[i][1] * Z[i][2]; out[5] += Yl[i][2] * Z[i][2];
    }
  }
  double* o9 = p.pp + 9 * (size_t)pt;
  o9[0] = out[0]; o9[1] = out[1]; o9[2] = out[2]; o9[3] = out[1]; o9[4] = out[3]; o9[5] = out[4]; o9[6] = out[2]; o9[7] = out[4]; o9[8] = out[5];
}

}  // namespace pba
