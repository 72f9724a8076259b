// pba_points.h -- structure-only solves (pba_set_cameras_constant): every camera is a constant parameter block, so the normal equations
// are block diagonal, one 3x3 block per point (1x1 in the inverse-depth mode), and there is neither a Schur complement nor a reduced
// solve.  The Jacobian and cost passes are the unchanged sampling kernels (their per-observation records do not depend on what is
// free); this header adds
//   k_points_system    records -> V_p = sum Ap^T M Ap (6) and g_p = -sum Ap^T b (3) of every point, one lane per point over the point's
//                      contiguous observations in list order, fp64, no floating-point atomics; kept in HBM for the re-solve after a
//                      rejected step
//   k_points_solve     per point, in registers: Jacobi scaling, damping, exact 3x3 Cholesky, both substitutions, step, candidate point
//                      into the other parity; the point's step scalars leave as one row per wave (butterfly sums, no LDS)
//   k_points_finalize  fixed-order sum of the rows and of the block costs, candidate cost, publication of the scalar block
// The camera Jacobian is never formed and the cameras are never written.
#pragma once
#include "pba_kernels.h"
#include "pba_point_prior.h"

namespace pba {

constexpr int kPointsThreads = 256;
constexpr int kPointsWaves = kPointsThreads / 64;
constexpr int kPointsSys = 9;          // per point: V row by row, upper triangle (00 01 02 11 12 22) | g (3); stored [kPointsSys][n_points]
constexpr int kPointsRow = 6;          // per wave of k_points_solve: mcc | step^2 | x^2 | |g|^2 | max |g| | a block failed

struct PointsSystemParams {
  const double* xyz;
  const double* rays;          // inverse-depth variant (point_world), else null
  const CamGeom* geom;
  const double* rec;           // [6][rec_stride] records of the Jacobian pass
  const int32_t* pt_begin;     // [n_points + 1]
  const uint8_t* obs_slot;
  double* sys;                 // [kPointsSys][n_points]
  int64_t rec_stride;
  int32_t n_points, n_frames;
  double fx, fy;
  const double* prior_x0;      // point prior (pba_point_prior.h), read by k_points_system<true> only: [n_points][3]
  const double* prior_L6;      // [n_points][6]
};

// kPrior: the point prior's Lambda_i joins V_p and Lambda_i (X - x0_i) joins g_p after the observation loop
template <bool kPrior>
__global__ __launch_bounds__(kPointsThreads) void k_points_system(PointsSystemParams p) {
  __shared__ CamGeom s_geom[kMaxFramesWide];
  const int tid = threadIdx.x;
  stage_geom<kPointsThreads, false, kMaxFramesWide>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const size_t pt = (size_t)blockIdx.x * kPointsThreads + tid;
  if (pt >= (size_t)p.n_points) return;
  const double prm[3] = {p.xyz[3 * pt], p.xyz[3 * pt + 1], p.xyz[3 * pt + 2]};
  double X[3], qd[3];
  point_world(p.rays, (int)pt, prm, X, qd);
  double v[kPointsSys];
#pragma unroll
  for (int k = 0; k < kPointsSys; ++k) v[k] = 0.0;
  const int o1 = p.pt_begin[pt + 1];
  for (int o = p.pt_begin[pt]; o < o1; ++o) {      // list order: the sum depends on the problem's shape only
    const CamGeom& g = s_geom[p.obs_slot[o]];
    double xw[3], Ac[2][6], Ap[2][3];
    transform_point(g, X, xw);
    projection_jacobians(g, X, xw, p.fx, p.fy, Ac, Ap);      // (Ac is dead code here: the camera Jacobian is not used)
    point_jacobian(p.rays, qd, Ap);
    const double m0 = p.rec[0 * p.rec_stride + o], m1 = p.rec[1 * p.rec_stride + o], m2 = p.rec[2 * p.rec_stride + o];
    const double b0 = p.rec[3 * p.rec_stride + o], b1 = p.rec[4 * p.rec_stride + o];
    double MAp[2][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { MAp[0][k] = m0 * Ap[0][k] + m1 * Ap[1][k]; MAp[1][k] = m1 * Ap[0][k] + m2 * Ap[1][k]; }
    v[0] += Ap[0][0] * MAp[0][0] + Ap[1][0] * MAp[1][0];
    v[1] += Ap[0][0] * MAp[0][1] + Ap[1][0] * MAp[1][1];
    v[2] += Ap[0][0] * MAp[0][2] + Ap[1][0] * MAp[1][2];
    v[3] += Ap[0][1] * MAp[0][1] + Ap[1][1] * MAp[1][1];
    v[4] += Ap[0][1] * MAp[0][2] + Ap[1][1] * MAp[1][2];
    v[5] += Ap[0][2] * MAp[0][2] + Ap[1][2] * MAp[1][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[6 + k] += -(Ap[0][k] * b0 + Ap[1][k] * b1);      // J^T r = -Ap^T b
  }
  if constexpr (kPrior) {      // (free world points: pba_set_point_prior refuses the inverse-depth mode)
    double L[6], Ld[3], d[3];
    point_prior_terms(p.prior_x0, p.prior_L6, pt, prm, L, Ld, d);
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += L[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[6 + k] += Ld[k];
  }
#pragma unroll
  for (int k = 0; k < kPointsSys; ++k) p.sys[(size_t)k * p.n_points + pt] = v[k];
}

struct PointsSolveParams {
  const double* sys;           // [kPointsSys][n_points]
  const double* xyz;           // current point parameters [n_points][3]
  double* xyz_cand;
  double* sp;                  // [n_points][3] Jacobi scales (written when init_scale)
  double* part;                // [gridDim.x * kPointsWaves][kPointsRow]
  double* V_dbg;               // [n_points][9] scaled + damped blocks, row-major (test hook), may be null
  double* rhs_dbg;             // [n_points][3] scaled gradient
  int32_t n_points, dim;       // dim: free parameters per point (3, or 1 in the inverse-depth mode: the rest never move)
  int32_t init_scale, jacobi, grad_only;
  double radius, min_diag, max_diag;
};

__global__ __launch_bounds__(kPointsThreads) void k_points_solve(PointsSolveParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t pt = (size_t)blockIdx.x * kPointsThreads + tid;
  const size_t n = (size_t)p.n_points;
  const bool write_step = !(p.grad_only && !p.init_scale);
  double sum4[4] = {0.0, 0.0, 0.0, 0.0};      // mcc, step^2, x^2, |g|^2
  double gmax = 0.0, bad = 0.0;
  if (pt < n) {
    double V[6], g[3], X[3], s[3], D2[3], gs[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) V[k] = p.sys[(size_t)k * n + pt];
#pragma unroll
    for (int k = 0; k < 3; ++k) { g[k] = p.sys[(size_t)(6 + k) * n + pt]; X[k] = p.xyz[3 * pt + k]; }
    const double vd[3] = {V[0], V[3], V[5]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const bool in = k < p.dim;
      if (p.init_scale) { s[k] = (in && p.jacobi) ? 1.0 / (1.0 + sqrt(vd[k])) : 1.0; p.sp[3 * pt + k] = s[k]; }
      else s[k] = p.sp[3 * pt + k];
      D2[k] = in ? fmin(fmax(s[k] * s[k] * vd[k], p.min_diag), p.max_diag) / p.radius : 0.0;
      gs[k] = in ? s[k] * g[k] : 0.0;
      if (in) { gmax = fmax(gmax, fabs(g[k])); sum4[3] += g[k] * g[k]; }
    }
    // scaled + damped block; a parameter outside the program keeps a unit pivot and a zero right-hand side
    const double a00 = s[0] * V[0] * s[0] + D2[0];
    const double a10 = s[1] * V[1] * s[0], a20 = s[2] * V[2] * s[0], a21 = s[2] * V[4] * s[1];
    const double a11 = p.dim > 1 ? s[1] * V[3] * s[1] + D2[1] : 1.0;
    const double a22 = p.dim > 2 ? s[2] * V[5] * s[2] + D2[2] : 1.0;
    if (p.V_dbg && write_step) {
      double* vo = p.V_dbg + 9 * pt;
      vo[0] = a00; vo[1] = a10; vo[2] = a20; vo[3] = a10; vo[4] = p.dim > 1 ? a11 : 0.0; vo[5] = a21; vo[6] = a20; vo[7] = a21; vo[8] = p.dim > 2 ? a22 : 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) p.rhs_dbg[3 * pt + k] = gs[k];
    }
    // Cholesky L L^T, then the two triangular solves
    bool ok = true;
    double piv = a00;
    if (!(piv > 0.0) || !isfinite(piv)) { ok = false; piv = 1.0; }
    const double l00 = sqrt(piv), l10 = a10 / l00, l20 = a20 / l00;
    piv = a11 - l10 * l10;
    if (!(piv > 0.0) || !isfinite(piv)) { ok = false; piv = 1.0; }
    const double l11 = sqrt(piv), l21 = (a21 - l20 * l10) / l11;
    piv = a22 - l20 * l20 - l21 * l21;
    if (!(piv > 0.0) || !isfinite(piv)) { ok = false; piv = 1.0; }
    const double l22 = sqrt(piv);
    double y[3];
    y[0] = gs[0] / l00;
    y[1] = (gs[1] - l10 * y[0]) / l11;
    y[2] = (gs[2] - l20 * y[0] - l21 * y[1]) / l22;
    y[2] = y[2] / l22;
    y[1] = (y[1] - l21 * y[2]) / l11;
    y[0] = (y[0] - l10 * y[1] - l20 * y[2]) / l00;
#pragma unroll
    for (int k = 0; k < 3; ++k) if (!isfinite(y[k])) ok = false;
    if (!ok) { y[0] = y[1] = y[2] = 0.0; bad = 1.0; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double d = -s[k] * y[k];
      sum4[0] += 0.5 * y[k] * gs[k] + 0.5 * D2[k] * y[k] * y[k];
      sum4[1] += d * d;
      sum4[2] += X[k] * X[k];
      if (write_step) p.xyz_cand[3 * pt + k] = X[k] + d;
    }
  }
  wave_sum_n(sum4);
  gmax = wave_max(gmax);
  bad = wave_max(bad);
  if (lane == 0) {
    double* row = p.part + ((size_t)blockIdx.x * kPointsWaves + wave) * kPointsRow;
    row[0] = sum4[0]; row[1] = sum4[1]; row[2] = sum4[2]; row[3] = sum4[3]; row[4] = gmax; row[5] = bad;
  }
}

struct PointsFinalizeParams {
  const double* part;          // [n_rows][kPointsRow], workgroup-major
  const double* cost_lin;      // block costs / failure flags of the Jacobian pass at the current point
  const int32_t* fail_lin;
  const double* cost_cand;     // ... of the candidate pass (n_cand == 0: a gradient-only step, no candidate)
  const int32_t* fail_cand;
  double* scal;
  double* host_scal;
  unsigned long long* host_seq;
  unsigned long long seq;
  int32_t n_rows, n_lin, n_cand;
};

// Thread t adds rows t, t + 256, ... in ascending order, then the 256 sums go through one binary tree: the order depends on the number
// of rows (the problem's shape) only.  A failed block anywhere makes the whole step a zero step (LinearSolver failure in Ceres).
// kPrior leaves the scalar block on the device: the point prior's costs are added behind it, then k_publish publishes.
template <bool kPrior>
__global__ __launch_bounds__(kPointsThreads) void k_points_finalize(PointsFinalizeParams p) {
  __shared__ double s_red[6][kPointsThreads];
  __shared__ double s_mx[2][kPointsThreads];
  __shared__ int s_f[2][kPointsThreads];
  const int tid = threadIdx.x;
  double a[6] = {0, 0, 0, 0, 0, 0}, mx[2] = {0, 0};
  int f[2] = {0, 0};
  for (int r = tid; r < p.n_rows; r += kPointsThreads) {
    const double* row = p.part + (size_t)r * kPointsRow;
    a[0] += row[0]; a[1] += row[1]; a[2] += row[2]; a[3] += row[3];
    mx[0] = fmax(mx[0], row[4]); mx[1] = fmax(mx[1], row[5]);
  }
  for (int b = tid; b < p.n_lin; b += kPointsThreads) { a[4] += p.cost_lin[b]; f[0] |= p.fail_lin[b]; }
  for (int b = tid; b < p.n_cand; b += kPointsThreads) { a[5] += p.cost_cand[b]; f[1] |= p.fail_cand[b]; }
#pragma unroll
  for (int k = 0; k < 6; ++k) s_red[k][tid] = a[k];
  s_mx[0][tid] = mx[0]; s_mx[1][tid] = mx[1]; s_f[0][tid] = f[0]; s_f[1][tid] = f[1];
  __syncthreads();
  for (int s = kPointsThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < 6; ++k) s_red[k][tid] += s_red[k][tid + s];
      s_mx[0][tid] = fmax(s_mx[0][tid], s_mx[0][tid + s]); s_mx[1][tid] = fmax(s_mx[1][tid], s_mx[1][tid + s]);
      s_f[0][tid] |= s_f[0][tid + s]; s_f[1][tid] |= s_f[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool ok = s_mx[1][0] == 0.0;
    p.scal[kMccPts] = ok ? s_red[0][0] : 0.0; p.scal[kStep2Pts] = ok ? s_red[1][0] : 0.0; p.scal[kX2Pts] = s_red[2][0];
    p.scal[kGnorm2Pts] = s_red[3][0]; p.scal[kGmaxPts] = s_mx[0][0];
    p.scal[kSolveOk] = ok ? 1.0 : 0.0; p.scal[kSchurFail] = 0.0;
    p.scal[kCostLin] = s_red[4][0]; p.scal[kEvalFailLin] = (double)s_f[0][0];
    if (p.n_cand > 0) { p.scal[kCandCost] = s_red[5][0]; p.scal[kEvalFailCand] = (double)s_f[1][0]; }
    // the cameras are constant: they enter none of the step scalars
    p.scal[kMccCams] = 0.0; p.scal[kStep2Cams] = 0.0; p.scal[kX2Cams] = 0.0; p.scal[kGmaxCams] = 0.0; p.scal[kGnorm2Cams] = 0.0;
  }
  if constexpr (!kPrior) {
    __syncthreads();
    publish_scal(p.scal, p.host_scal, tid, blockDim.x);
    publish_seq(p.host_seq, p.seq, tid);
  }
}

}  // namespace pba
