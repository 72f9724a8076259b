// pba_cov.h -- covariance output (pba_covariance): blocks of (J^T J)^-1 of the reduced program of the mode that is on, from the
// per-observation records of a Jacobian pass.  No damping and no Jacobi scaling enter the result; every block is factorised in its
// unit-diagonal form D^-1/2 A D^-1/2 (D = diag A), so that the reported pivots are scale-free, and the inverse is unscaled again.
//   k_cov_point    one lane per point: V in list order, P = V^-1 and its factor through the shared point factorisation (pba_elim.h),
//                  the smallest pivot, the first failing point and the program cost of every workgroup
//   k_elim_pair    (pba_elim.h) the reduced camera matrix S, dense, both triangles
//   k_cov_invert   ONE workgroup: the packed lower triangle of the unit-diagonal S in LDS, in place Cholesky -> L^-1 -> L^-T L^-1,
//                  the smallest pivot, the dense symmetric inverse unscaled into HBM
//   k_cov_points   one lane per point: P + sum_{l, m} Y_l^T Sigma_cc[a_l, a_m] Y_m, Y_l = W_l P, observations in list order
// Every sum has a fixed order (no floating-point atomics).  Everything is written to buffers of the two off-loop calls: nothing of the
// LM state (point scales, point records, packed system, scalar block) is touched.
// Included by pba_engine.hip after pba_kernels.h and pba_solve.h.
#pragma once
#include "pba_elim.h"
#include "pba_point_prior.h"

namespace pba {

constexpr int kCovPart = elim_part_width(1);      // per workgroup of k_cov_point: smallest pivot | first failing point | cost
constexpr int kCovInvertT = 1024;

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
  const double* prior_x0;        // point prior (pba_point_prior.h), read by k_cov_point<true> only: [n_points][3]
  const double* prior_L6;        // [n_points][6]
};

// kPrior: the point prior's Lambda_i joins V after the observation loop, before the factorisation (free world points only)
template <bool kPrior>
__global__ __launch_bounds__(kElimThreads) void k_cov_point(CovPointParams p) {
  __shared__ CamGeom s_geom[kMaxFramesWide];
  const int tid = threadIdx.x;
  stage_geom<kElimThreads, false, kMaxFramesWide>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const int pt = blockIdx.x * kElimThreads + tid;
  double piv = 1.0, bad = kElimNone, cost = 0.0;
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
      elim_observation(s_geom[slot], X, p.rays, qd, p.rec, p.rec_stride, o, p.fx, p.fy, Ac, MAp, Ap, M);
      elim_add_point_block(Ap, MAp, V);
    }
    if (p.P) {
      if constexpr (kPrior) {
#pragma unroll
        for (int k = 0; k < 6; ++k) V[k] += p.prior_L6[6 * (size_t)pt + k];
      }
      double Pm[6] = {0, 0, 0, 0, 0, 0}, Xm[6] = {0, 0, 0, 0, 0, 0};
      if (!elim_factor_point(V, p.dim, piv, Pm, Xm)) bad = (double)pt;
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
  elim_point_partial<1>(piv, bad, cost, 0.0, p.part + kCovPart * (size_t)blockIdx.x);
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
    if (!elim_pivot_ok(d)) atomicMax(&s_bad, n - 1 - tid);      // (integer, order-free: the FIRST bad diagonal entry wins)
    dinv[tid] = 1.0 / sqrt(elim_pivot_ok(d) ? d : 1.0);
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
    if (!elim_pivot_ok(d)) {
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
  elim_observation(g, X, nullptr, nullptr, rec, rs, o, fx, fy, Ac, MAp, Ap, M);
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
__global__ __launch_bounds__(kElimThreads) void k_cov_points(CovPointsParams p) {
  __shared__ CamGeom s_geom[kMaxFramesWide];
  const int tid = threadIdx.x;
  stage_geom<kElimThreads, false, kMaxFramesWide>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const int pt = blockIdx.x * kElimThreads + tid;
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
