// pba_pose.h -- pose-only solves (pba_set_points_constant): every point is a constant parameter block, so the normal equations
// are block diagonal, one 6x6 block per free camera, and there is no Schur complement.  The Jacobian and cost passes are the
// unchanged sampling kernels (their per-observation records do not depend on what is free); this header adds
//   k_pose_system    records -> per-workgroup partial sums of U_a = sum Ac^T M Ac (21), g_a = -sum Ac^T b (6) and the block costs (1)
//                    of every window slot, one lane per observation, fp64, fixed summation order, no floating-point atomics
//   k_pose_solve     fixed-order sum of the partials (kept for the re-solve after a rejected step), Jacobi scaling, damping, one
//                    exact 6x6 Cholesky per camera (one lane each), step scalars, candidate cameras and their geometry
//   k_pose_finalize  candidate cost of the program + publication of the step's scalar block
// The point Jacobian is never formed and the points are never written.
#pragma once
#include "pba_kernels.h"

namespace pba {

constexpr int kPoseVals = 28;          // per slot: upper triangle of U row by row (21) | g (6) | sum of the slot's block costs
constexpr int kPoseThreads = 256;
constexpr int kPoseWaves = kPoseThreads / 64;
constexpr int kPoseMaxGrid = 512;      // workgroups of k_pose_system (rows of the partial buffer)
constexpr int kPoseFixedCost = 24;     // slot of the scalar block: cost of the residual blocks of the constant camera
static_assert(kPoseFixedCost > kGnorm2Pts && kPoseFixedCost < kNumScal, "a free slot of the scalar block");

__host__ __device__ constexpr int pose_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }   // i <= j
static_assert(pose_tri(5, 5) == 20, "21 entries");

struct PoseSystemParams {
  const double* xyz;
  const double* rays;          // inverse-depth variant (point_world), else null
  const CamGeom* geom;
  const double* rec;           // [6][rec_stride] records of the Jacobian pass
  const int32_t* obs_point;
  const uint8_t* obs_slot;
  double* partial;             // [gridDim.x][n_frames * kPoseVals]
  int64_t rec_stride;
  int32_t n_obs, n_frames;
  double fx, fy;
};

// One lane per observation, tiles of 256 observations dealt to the workgroups round robin.  A wave sums its 64 lanes per slot with
// the butterfly of wave_sum_n (slots in ascending order, lanes of other slots contribute zeros), adds the result to its own row of
// LDS, and the four rows are added in wave order at the end: the order depends on the problem's shape only.
__global__ __launch_bounds__(kPoseThreads) void k_pose_system(PoseSystemParams p) {
  __shared__ CamGeom s_geom[kMaxFramesWide];
  __shared__ double s_wave[kPoseWaves][kMaxFramesWide * kPoseVals];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  stage_geom<kPoseThreads, false, kMaxFramesWide>(p.geom, s_geom, p.n_frames, tid);
  for (int k = tid; k < kPoseWaves * kMaxFramesWide * kPoseVals; k += kPoseThreads) (&s_wave[0][0])[k] = 0.0;
  __syncthreads();
  const int n_tiles = (p.n_obs + kPoseThreads - 1) / kPoseThreads;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int o = tile * kPoseThreads + tid;
    double v[kPoseVals];
#pragma unroll
    for (int k = 0; k < kPoseVals; ++k) v[k] = 0.0;
    int slot = -1;
    if (o < p.n_obs) {
      slot = p.obs_slot[o];
      const CamGeom& g = s_geom[slot];
      v[27] = p.rec[5 * p.rec_stride + o];
      if (g.free_index >= 0) {
        const int pt = p.obs_point[o];
        const double prm[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
        double X[3], qd[3], xw[3], Ac[2][6], Ap[2][3];
        point_world(p.rays, pt, prm, X, qd);
        transform_point(g, X, xw);
        projection_jacobians(g, X, xw, p.fx, p.fy, Ac, Ap);      // (Ap is dead code here: the point Jacobian is not used)
        const double m0 = p.rec[0 * p.rec_stride + o], m1 = p.rec[1 * p.rec_stride + o], m2 = p.rec[2 * p.rec_stride + o];
        const double b0 = p.rec[3 * p.rec_stride + o], b1 = p.rec[4 * p.rec_stride + o];
        double t0[6], t1[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { t0[k] = m0 * Ac[0][k] + m1 * Ac[1][k]; t1[k] = m1 * Ac[0][k] + m2 * Ac[1][k]; }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int j = i; j < 6; ++j) v[pose_tri(i, j)] = Ac[0][i] * t0[j] + Ac[1][i] * t1[j];
          v[21 + i] = -(Ac[0][i] * b0 + Ac[1][i] * b1);      // J^T r = -Ac^T b (the records hold b of the residual's negative)
        }
      }
    }
    unsigned present = slot >= 0 ? 1u << slot : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) present |= __shfl_xor(present, off);
    while (present) {
      const int s = __builtin_ctz(present);
      present &= present - 1;
      double t[kPoseVals];
#pragma unroll
      for (int k = 0; k < kPoseVals; ++k) t[k] = (slot == s) ? v[k] : 0.0;
      wave_sum_n(t);
      double mine = 0.0;
#pragma unroll
      for (int k = 0; k < kPoseVals; ++k) if (lane == k) mine = t[k];
      if (lane < kPoseVals) s_wave[wave][s * kPoseVals + lane] += mine;      // lane k owns entry k: no cross-lane hazard
    }
  }
  __syncthreads();
  const int E = p.n_frames * kPoseVals;
  for (int k = tid; k < E; k += kPoseThreads) {
    double a = s_wave[0][k];
#pragma unroll
    for (int w = 1; w < kPoseWaves; ++w) a += s_wave[w][k];
    p.partial[(size_t)blockIdx.x * E + k] = a;
  }
}

struct PoseSolveParams {
  const double* partial;       // [n_parts][n_frames * kPoseVals]
  double* sums;                // [n_frames * kPoseVals + 2]: the reduced sums | sum of all block costs | evaluation-failed flag
  const double* block_cost;    // block costs / failure flags of the Jacobian pass at the current point
  const int32_t* block_fail;
  const double* cams;          // current cameras [n_frames][6]
  double* cams_cand;
  double* delta_c;             // [n_frames][6]
  double* sc;                  // [2][6 n_free]: Jacobi scales | column-is-live flags (written when init_scale)
  double* S_dbg;               // [n*n] dense copy of the block-diagonal system (test hook), may be null
  double* rhs_dbg;
  double* scal;
  const CamGeom* geom;
  CamGeom* geom_cand;
  int32_t n_parts, n_cost_blocks, reduce;      // reduce == 0: the sums of an earlier launch are reused (re-solve after a rejected step)
  int32_t n_frames, n_free, init_scale, jacobi, grad_only;
  uint32_t anchor_mask;        // constant slots: their blocks leave the program, their cost is the fixed cost
  double radius, min_diag, max_diag;
};

__global__ __launch_bounds__(kPoseThreads) void k_pose_solve(PoseSolveParams p) {
  __shared__ double s_sums[kMaxFramesWide * kPoseVals];
  __shared__ double s_red[kPoseThreads];
  __shared__ int s_f[kPoseThreads];
  __shared__ double s_cam[kMaxFramesWide][6];      // mcc, step^2, x^2, max |g|, |g|^2, solve failed
  const int tid = threadIdx.x;
  const int E = p.n_frames * kPoseVals, n = 6 * p.n_free;
  if (p.reduce) {
    for (int k = tid; k < E; k += kPoseThreads) {
      double a = 0.0;
      for (int b = 0; b < p.n_parts; ++b) a += p.partial[(size_t)b * E + k];      // workgroup order
      s_sums[k] = a;
      p.sums[k] = a;
    }
    double c = 0.0; int f = 0;
    for (int b = tid; b < p.n_cost_blocks; b += kPoseThreads) { c += p.block_cost[b]; f |= p.block_fail[b]; }
    s_red[tid] = c; s_f[tid] = f;
    __syncthreads();
    for (int s = kPoseThreads / 2; s > 0; s >>= 1) {
      if (tid < s) { s_red[tid] += s_red[tid + s]; s_f[tid] |= s_f[tid + s]; }
      __syncthreads();
    }
    if (tid == 0) { p.sums[E] = s_red[0]; p.sums[E + 1] = (double)s_f[0]; }
  } else {
    for (int k = tid; k < E; k += kPoseThreads) s_sums[k] = p.sums[k];
    if (tid == 0) { s_red[0] = p.sums[E]; s_f[0] = p.sums[E + 1] > 0.5 ? 1 : 0; }
    __syncthreads();
  }
  const bool write_step = !(p.grad_only && !p.init_scale);
  if (p.S_dbg && write_step) {
    for (int k = tid; k < n * n; k += kPoseThreads) p.S_dbg[k] = 0.0;
    __syncthreads();
  }
  if (tid < p.n_frames) {
    const int c = tid, fa = p.geom[c].free_index;
    double mcc = 0.0, st2 = 0.0, x2 = 0.0, gmax = 0.0, gn2 = 0.0, bad = 0.0;
    double d[6] = {0, 0, 0, 0, 0, 0};
    if (fa >= 0) {
      const double* u = s_sums + c * kPoseVals;
      double sc[6], D2[6], gs[6], y[6], L[6][6];
      double live = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double du = u[pose_tri(i, i)];
        double s;
        if (p.init_scale) { s = p.jacobi ? 1.0 / (1.0 + sqrt(du)) : 1.0; p.sc[6 * fa + i] = s; p.sc[n + 6 * fa + i] = du > 0.0 ? 1.0 : 0.0; live += du > 0.0 ? 1.0 : 0.0; }
        else { s = p.sc[6 * fa + i]; live += p.sc[n + 6 * fa + i]; }
        sc[i] = s;
        D2[i] = fmin(fmax(s * s * du, p.min_diag), p.max_diag) / p.radius;
        const double g = u[21 + i];
        gs[i] = s * g;
        gmax = fmax(gmax, fabs(g));
        gn2 += g * g;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i][j] = sc[i] * u[pose_tri(j, i)] * sc[j] + (i == j ? D2[i] : 0.0);
      if (p.S_dbg && write_step) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            p.S_dbg[(size_t)(6 * fa + i) * n + 6 * fa + j] = L[i][j];
            p.S_dbg[(size_t)(6 * fa + j) * n + 6 * fa + i] = L[i][j];
          }
          p.rhs_dbg[6 * fa + i] = gs[i];
        }
      }
      // Cholesky L L^T, then the two triangular solves
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double a = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) a -= L[j][k] * L[j][k];
        if (!(a > 0.0) || !isfinite(a)) { ok = false; a = 1.0; }
        const double l = sqrt(a), il = 1.0 / l;
        L[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
          double b = L[i][j];
#pragma unroll
          for (int k = 0; k < j; ++k) b -= L[i][k] * L[j][k];
          L[i][j] = b * il;
        }
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double b = gs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) b -= L[i][k] * y[k];
        y[i] = b / L[i][i];
      }
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double b = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) b -= L[k][i] * y[k];
        y[i] = b / L[i][i];
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        if (!isfinite(y[i])) ok = false;
        if (!ok) y[i] = 0.0;
      }
      if (!ok) bad = 1.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        mcc += 0.5 * y[i] * gs[i] + 0.5 * D2[i] * y[i] * y[i];
        d[i] = -sc[i] * y[i];
        st2 += d[i] * d[i];
        if (live > 0.0) x2 += p.cams[6 * c + i] * p.cams[6 * c + i];      // a free camera without residual blocks is not in the program
      }
    }
    if (write_step) {
      double cam6[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        cam6[i] = p.cams[6 * c + i] + d[i];
        p.delta_c[6 * c + i] = d[i];
        p.cams_cand[6 * c + i] = cam6[i];
      }
      cam_geom_one(cam6 - 6 * c, p.geom_cand, c, p.anchor_mask);
    }
    s_cam[c][0] = mcc; s_cam[c][1] = st2; s_cam[c][2] = x2; s_cam[c][3] = gmax; s_cam[c][4] = gn2; s_cam[c][5] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    double mcc = 0.0, st2 = 0.0, x2 = 0.0, gmax = 0.0, gn2 = 0.0, bad = 0.0;
    for (int c = 0; c < p.n_frames; ++c) {      // slot order
      mcc += s_cam[c][0]; st2 += s_cam[c][1]; x2 += s_cam[c][2]; gmax = fmax(gmax, s_cam[c][3]); gn2 += s_cam[c][4]; bad = fmax(bad, s_cam[c][5]);
    }
    double fixed = 0.0;      // loss-corrected cost of the anchored cameras' blocks, slot order
    for (int c = 0; c < p.n_frames; ++c) if (!slot_is_free(p.anchor_mask, c)) fixed += s_sums[c * kPoseVals + 27];
    p.scal[kMccCams] = mcc; p.scal[kStep2Cams] = st2; p.scal[kX2Cams] = x2; p.scal[kGmaxCams] = gmax; p.scal[kGnorm2Cams] = gn2;
    p.scal[kSolveOk] = bad == 0.0 ? 1.0 : 0.0;
    p.scal[kCostLin] = s_red[0] - fixed;
    p.scal[kPoseFixedCost] = fixed;
    p.scal[kEvalFailLin] = (double)s_f[0];
    // the points are constant: they enter none of the step scalars
    p.scal[kMccPts] = 0.0; p.scal[kStep2Pts] = 0.0; p.scal[kX2Pts] = 0.0; p.scal[kGmaxPts] = 0.0; p.scal[kGnorm2Pts] = 0.0; p.scal[kSchurFail] = 0.0;
  }
}

// Candidate cost of the program (all block costs of the candidate pass minus the constant camera's, which never change) and the
// publication of the scalar block; the counterpart of k_finalize_step.
__global__ __launch_bounds__(kPoseThreads) void k_pose_finalize(const double* __restrict__ block_cost, const int32_t* __restrict__ block_fail,
                                                                int n_cost_blocks, double* __restrict__ scal, double* host_scal,
                                                                unsigned long long* host_seq, unsigned long long seq) {
  __shared__ double s_red[kPoseThreads];
  __shared__ int s_f[kPoseThreads];
  const int tid = threadIdx.x;
  double c = 0.0; int f = 0;
  for (int b = tid; b < n_cost_blocks; b += kPoseThreads) { c += block_cost[b]; f |= block_fail[b]; }
  s_red[tid] = c; s_f[tid] = f;
  __syncthreads();
  for (int s = kPoseThreads / 2; s > 0; s >>= 1) {
    if (tid < s) { s_red[tid] += s_red[tid + s]; s_f[tid] |= s_f[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) { scal[kCandCost] = s_red[0] - scal[kPoseFixedCost]; scal[kEvalFailCand] = (double)s_f[0]; }
  __syncthreads();
  publish_scal(scal, host_scal, tid, blockDim.x);
  publish_seq(host_seq, seq, tid);
}

}  // namespace pba
