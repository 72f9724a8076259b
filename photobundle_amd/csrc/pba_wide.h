// pba_wide.h -- wide windows: 16 to 32 free cameras (n = 6 n_free <= 192).  The narrow kernels give every thread of a
// 128-lane tile one 6x6 pair block (k_schur: <= 128 pairs = 15 free cameras) and keep the whole augmented reduced matrix
// plus ~22 KB of tables in one workgroup's LDS (k_reduce_solve); neither holds at 32 free cameras.  Here:
//   k_wide_point     one lane per point: V, g_p, damping, P (the arithmetic of k_schur's P2), the point record of the
//                    back-substitution, and one factor record per free-camera observation;
//   k_wide_pairs     fixed chunks of a per-pair list of co-observations (built on the host once per window shape): the
//                    6x6 Schur terms of one camera pair, plus U, r, g_c on the diagonal pairs;
//   k_wide_assemble  chunk sums in chunk order -> the packed "tri" layout of pba_solve.h, and the tail values;
//   k_solve_wide     scaling, damping, Cholesky of the augmented matrix (packed lower triangle in LDS, six-column panels),
//                    backward substitution, then solve_epilogue.
// Every sum has a fixed order (no atomics): runs are reproducible.  Included by pba_engine.hip after pba_kernels.h.
#pragma once
#include "pba_point_prior.h"

namespace pba {

constexpr int kWideMinFree = 16;          // the first window that k_schur's tile (kTile pairs) cannot hold
constexpr int kWideFac = 32;              // doubles per observation factor: Ac (12) | M Ap (6) | Q = (M Ap) P (6) | bq (2) | M (3) | b (2) | pad
constexpr int kWideChunk = 2048;          // co-observations per workgroup of the pair stage
constexpr int kWideVals = 69;             // pair-stage sums: T (36, row-major) | U (21, sym6) | r (6) | g_c (6)
constexpr int kWideThreads = 256;

struct WidePointParams {
  const double* xyz;
  const CamGeom* geom;
  const double* rec;             // SoA [6][rec_stride] records of the Jacobian pass
  const int32_t* pt_begin;
  const uint8_t* obs_slot;
  double* sp;                    // [n_points][3] Jacobi scale of the point columns (written when init_scale)
  double* ptrec;                 // [n_points][12] P | g_p | D_p^2 (layout of k_schur, read by k_backsub)
  double* fac;                   // [n_obs][kWideFac]
  double* part;                  // [gridDim.x][3] max |g_p|, sum g_p^2, point block failed
  int64_t rec_stride;
  int32_t n_points, n_frames, init_scale, jacobi;
  double fx, fy, inv_radius, min_diag, max_diag;
  const double* prior_x0;        // point prior (pba_point_prior.h), read by k_wide_point<true> only: [n_points][3]
  const double* prior_L6;        // [n_points][6]
};

// kPrior: the point prior's Lambda_i joins V and Lambda_i (X - x0_i) joins g_p after the observation loop, before scale, damping and factor
template <bool kPrior>
__global__ __launch_bounds__(kWideThreads) void k_wide_point(WidePointParams p) {
  __shared__ CamGeom s_geom[kMaxFramesWide];
  __shared__ double s_red[kWideThreads / 64][3];
  const int tid = threadIdx.x;
  stage_geom<kWideThreads, false, kMaxFramesWide>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const int pt = blockIdx.x * kWideThreads + tid;
  double gmax = 0.0, gn2 = 0.0, fail = 0.0;
  if (pt < p.n_points) {
    const double X[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
    const int o0 = p.pt_begin[pt], o1 = p.pt_begin[pt + 1];
    const int64_t rs = p.rec_stride;
    // V = sum Ap^T M Ap, g_p = -sum Ap^T b, in observation order (k_schur's point totals)
    double V[6] = {0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0};
    for (int o = o0; o < o1; ++o) {
      const CamGeom& g = s_geom[p.obs_slot[o]];
      double xw[3], Ac[2][6], Ap[2][3];
      transform_point(g, X, xw);
      projection_jacobians(g, X, xw, p.fx, p.fy, Ac, Ap);
      const double M0 = p.rec[o], M1 = p.rec[rs + o], M2 = p.rec[2 * rs + o], b0 = p.rec[3 * rs + o], b1 = p.rec[4 * rs + o];
      double MAp[2][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) { MAp[0][k] = M0 * Ap[0][k] + M1 * Ap[1][k]; MAp[1][k] = M1 * Ap[0][k] + M2 * Ap[1][k]; }
      double v[9];
      v[0] = Ap[0][0] * MAp[0][0] + Ap[1][0] * MAp[1][0];
      v[1] = Ap[0][0] * MAp[0][1] + Ap[1][0] * MAp[1][1];
      v[2] = Ap[0][0] * MAp[0][2] + Ap[1][0] * MAp[1][2];
      v[3] = Ap[0][1] * MAp[0][1] + Ap[1][1] * MAp[1][1];
      v[4] = Ap[0][1] * MAp[0][2] + Ap[1][1] * MAp[1][2];
      v[5] = Ap[0][2] * MAp[0][2] + Ap[1][2] * MAp[1][2];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[6 + k] = -(Ap[0][k] * b0 + Ap[1][k] * b1);
#pragma unroll
      for (int k = 0; k < 6; ++k) V[k] += v[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) gp[k] += v[6 + k];
    }
    if constexpr (kPrior) {
      double L[6], Ld[3], d[3];
      point_prior_terms(p.prior_x0, p.prior_L6, (size_t)pt, X, L, Ld, d);
#pragma unroll
      for (int k = 0; k < 6; ++k) V[k] += L[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) gp[k] += Ld[k];
    }
    // damping and the point block's inverse: k_schur P2
    double s[3];
    const double vd[3] = {V[0], V[3], V[5]};
    if (p.init_scale) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { s[k] = p.jacobi ? 1.0 / (1.0 + sqrt(vd[k])) : 1.0; p.sp[3 * (size_t)pt + k] = s[k]; }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = p.sp[3 * (size_t)pt + k];
    }
    double D2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) D2[k] = fmin(fmax(s[k] * s[k] * vd[k], p.min_diag), p.max_diag) * p.inv_radius;
    const double a00 = s[0] * s[0] * V[0] + D2[0], a01 = s[0] * s[1] * V[1], a02 = s[0] * s[2] * V[2];
    const double a11 = s[1] * s[1] * V[3] + D2[1], a12 = s[1] * s[2] * V[4], a22 = s[2] * s[2] * V[5] + D2[2];
    bool pd = a00 > 0.0;
    const double i00 = fast_rsqrt(a00);
    const double l10 = a01 * i00, l20 = a02 * i00;
    const double d1 = a11 - l10 * l10;
    pd = pd && d1 > 0.0;
    const double i11 = fast_rsqrt(d1);
    const double l21 = (a12 - l20 * l10) * i11;
    const double d2 = a22 - l20 * l20 - l21 * l21;
    pd = pd && d2 > 0.0;
    const double i22 = fast_rsqrt(d2);
    double Pm[6] = {0, 0, 0, 0, 0, 0};
    if (pd) {
      const double i10 = -l10 * i00 * i11;
      const double i21 = -l21 * i11 * i22;
      const double i20 = -(l20 * i00 + l21 * i10) * i22;
      const double v00 = i00 * i00 + i10 * i10 + i20 * i20;
      const double v01 = i10 * i11 + i20 * i21;
      const double v02 = i20 * i22;
      const double v11 = i11 * i11 + i21 * i21;
      const double v12 = i21 * i22;
      const double v22 = i22 * i22;
      Pm[0] = s[0] * s[0] * v00; Pm[1] = s[0] * s[1] * v01; Pm[2] = s[0] * s[2] * v02;
      Pm[3] = s[1] * s[1] * v11; Pm[4] = s[1] * s[2] * v12; Pm[5] = s[2] * s[2] * v22;
    } else {
      fail = 1.0;      // a damped point block that is not positive definite: the step is invalid (kSchurFail)
    }
    double* pr = p.ptrec + 12 * (size_t)pt;
#pragma unroll
    for (int k = 0; k < 6; ++k) pr[k] = Pm[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { pr[6 + k] = gp[k]; pr[9 + k] = D2[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { gmax = fmax(gmax, fabs(gp[k])); gn2 += gp[k] * gp[k]; }
    // one factor record per free-camera observation (the Jacobians again: recomputing them is cheaper than keeping 18 doubles
    // per observation of up to 32 in registers)
    const double Pg[3] = {Pm[0] * gp[0] + Pm[1] * gp[1] + Pm[2] * gp[2], Pm[1] * gp[0] + Pm[3] * gp[1] + Pm[4] * gp[2],
                          Pm[2] * gp[0] + Pm[4] * gp[1] + Pm[5] * gp[2]};
    for (int o = o0; o < o1; ++o) {
      const CamGeom& g = s_geom[p.obs_slot[o]];
      if (g.free_index < 0) continue;
      double xw[3], Ac[2][6], Ap[2][3];
      transform_point(g, X, xw);
      projection_jacobians(g, X, xw, p.fx, p.fy, Ac, Ap);
      const double M0 = p.rec[o], M1 = p.rec[rs + o], M2 = p.rec[2 * rs + o], b0 = p.rec[3 * rs + o], b1 = p.rec[4 * rs + o];
      double MAp[2][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) { MAp[0][k] = M0 * Ap[0][k] + M1 * Ap[1][k]; MAp[1][k] = M1 * Ap[0][k] + M2 * Ap[1][k]; }
      double f[kWideFac];
#pragma unroll
      for (int j = 0; j < 6; ++j) { f[j] = Ac[0][j]; f[6 + j] = Ac[1][j]; }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        f[12 + 3 * r] = MAp[r][0]; f[13 + 3 * r] = MAp[r][1]; f[14 + 3 * r] = MAp[r][2];
        f[18 + 3 * r] = MAp[r][0] * Pm[0] + MAp[r][1] * Pm[1] + MAp[r][2] * Pm[2];
        f[19 + 3 * r] = MAp[r][0] * Pm[1] + MAp[r][1] * Pm[3] + MAp[r][2] * Pm[4];
        f[20 + 3 * r] = MAp[r][0] * Pm[2] + MAp[r][1] * Pm[4] + MAp[r][2] * Pm[5];
      }
      // r_l = g_c,l - W_l (P g_p) = -Ac^T (b + (M Ap)(P g_p)): the 2-vector bq
      f[24] = b0 + (MAp[0][0] * Pg[0] + MAp[0][1] * Pg[1] + MAp[0][2] * Pg[2]);
      f[25] = b1 + (MAp[1][0] * Pg[0] + MAp[1][1] * Pg[1] + MAp[1][2] * Pg[2]);
      f[26] = M0; f[27] = M1; f[28] = M2; f[29] = b0; f[30] = b1; f[31] = 0.0;
      double2* dst = reinterpret_cast<double2*>(p.fac + (size_t)o * kWideFac);
#pragma unroll
      for (int k = 0; k < kWideFac / 2; ++k) dst[k] = make_double2(f[2 * k], f[2 * k + 1]);
    }
  }
  // block partials: butterfly per wave, the waves in order
  gmax = wave_max(gmax);
  gn2 = wave_sum(gn2);
  fail = wave_max(fail);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = gmax; s_red[tid >> 6][1] = gn2; s_red[tid >> 6][2] = fail; }
  __syncthreads();
  if (tid == 0) {
    double m = s_red[0][0], a = s_red[0][1], f = s_red[0][2];
    for (int w = 1; w < kWideThreads / 64; ++w) { m = fmax(m, s_red[w][0]); a += s_red[w][1]; f = fmax(f, s_red[w][2]); }
    p.part[3 * blockIdx.x] = m; p.part[3 * blockIdx.x + 1] = a; p.part[3 * blockIdx.x + 2] = f;
  }
}

struct WidePairParams {
  const double* fac;             // [n_obs][kWideFac]
  const int2* ent;               // co-observations (observation of camera a, observation of camera b), pair-major, point order
  const int4* chunk;             // [gridDim.x] {first entry, end, diagonal pair, pair}
  double* out;                   // [gridDim.x][kWideVals]
};

// T(a, b) -= Ac_a^T (Q_a (M Ap)_b^T) Ac_b over the chunk's co-observations (the rank-2 form of k_schur's pair blocks); a diagonal
// pair also sums U_l = Ac^T M Ac, r_l = -Ac^T bq and g_c,l = -Ac^T b of its observations (entries (l, l)).
__global__ __launch_bounds__(kWideThreads) void k_wide_pairs(WidePairParams p) {
  __shared__ double s_red[kWideThreads / 64][kWideVals];
  const int tid = threadIdx.x;
  const int4 ck = p.chunk[blockIdx.x];
  const bool diag = ck.z != 0;
  double acc[kWideVals];
#pragma unroll
  for (int k = 0; k < kWideVals; ++k) acc[k] = 0.0;
  for (int e = ck.x + tid; e < ck.y; e += kWideThreads) {
    const int2 l = p.ent[e];
    const double2* Fa = reinterpret_cast<const double2*>(p.fac + (size_t)l.x * kWideFac);
    const double2* Fb = reinterpret_cast<const double2*>(p.fac + (size_t)l.y * kWideFac);
    double fa[12], qa[6], fb[12], mb[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { const double2 v = Fa[k]; fa[2 * k] = v.x; fa[2 * k + 1] = v.y; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double2 v = Fa[9 + k]; qa[2 * k] = v.x; qa[2 * k + 1] = v.y; }
#pragma unroll
    for (int k = 0; k < 6; ++k) { const double2 v = Fb[k]; fb[2 * k] = v.x; fb[2 * k + 1] = v.y; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double2 v = Fb[6 + k]; mb[2 * k] = v.x; mb[2 * k + 1] = v.y; }
    double N[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int t = 0; t < 2; ++t) N[r][t] = fma(qa[3 * r + 2], mb[3 * t + 2], fma(qa[3 * r + 1], mb[3 * t + 1], qa[3 * r] * mb[3 * t]));
    double Z[2][6];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 6; ++j) Z[r][j] = fma(N[r][1], fb[6 + j], N[r][0] * fb[j]);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[6 * i + j] = fma(-fa[6 + i], Z[1][j], fma(-fa[i], Z[0][j], acc[6 * i + j]));
    if (diag) {      // (uniform per workgroup)
      const double2 t0 = Fa[12], t1 = Fa[13], t2 = Fa[14], t3 = Fa[15];
      const double bq0 = t0.x, bq1 = t0.y, M0 = t1.x, M1 = t1.y, M2 = t2.x, b0 = t2.y, b1 = t3.x;
      double MAc[2][6];
#pragma unroll
      for (int j = 0; j < 6; ++j) { MAc[0][j] = M0 * fa[j] + M1 * fa[6 + j]; MAc[1][j] = M1 * fa[j] + M2 * fa[6 + j]; }
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[36 + sym6(i, j)] += fa[i] * MAc[0][j] + fa[6 + i] * MAc[1][j];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        acc[57 + j] += -(fa[j] * bq0 + fa[6 + j] * bq1);
        acc[63 + j] += -(fa[j] * b0 + fa[6 + j] * b1);
      }
    }
  }
  const int nv = diag ? kWideVals : 36;
#pragma unroll
  for (int k = 0; k < 36; ++k) {
    const double v = wave_sum(acc[k]);
    if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
  }
  if (diag) {
#pragma unroll
    for (int k = 36; k < kWideVals; ++k) {
      const double v = wave_sum(acc[k]);
      if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
    }
  }
  __syncthreads();
  if (tid < kWideVals) {
    double v = 0.0;
    if (tid < nv) {
      v = s_red[0][tid];
#pragma unroll
      for (int w = 1; w < kWideThreads / 64; ++w) v += s_red[w][tid];
    }
    p.out[(size_t)blockIdx.x * kWideVals + tid] = v;
  }
}

struct WideAssembleParams {
  const double* chunk_sums;      // [n_chunks][kWideVals]
  const int32_t* pair_chunk;     // [n_pairs + 1] first chunk of every pair
  const double* pt_part;         // [n_pt_blocks][3] (k_wide_point)
  int32_t n_pt_blocks;
  const double* block_cost; const int32_t* block_fail; int32_t n_cost_blocks;     // Jacobian pass at the linearisation point
  double* packed;                // tri layout (pba_solve.h)
  double* scal;
  int32_t n_free, n_pairs;
};

// Workgroup q < n_pairs: pair q (enumerated row by row, (a, a..nf-1)); workgroup n_pairs: the tail (cost at the linearisation
// point, point-gradient statistics, point-block failure).  All sums in chunk / block order.
__global__ __launch_bounds__(128) void k_wide_assemble(WideAssembleParams p) {
  __shared__ double s_v[kWideVals];
  __shared__ double s_t[2][4];
  __shared__ int s_f[2];
  const int tid = threadIdx.x;
  const int q = blockIdx.x;
  const int nf = p.n_free, n = 6 * nf, TRI = tri_index(n + 1);
  if (q < p.n_pairs) {
    int a = 0, rem = q;
    while (rem >= nf - a) { rem -= nf - a; ++a; }
    const int b = a + rem;
    const bool diag = a == b;
    if (tid < kWideVals) {
      double v = 0.0;
      for (int c = p.pair_chunk[q]; c < p.pair_chunk[q + 1]; ++c) v += p.chunk_sums[(size_t)c * kWideVals + tid];
      s_v[tid] = v;
    }
    __syncthreads();
    if (tid < 36) {
      const int i = tid / 6, j = tid - 6 * i;
      // entry (6a + i, 6b + j) of the upper triangle = (row 6b + j, column 6a + i) of the lower one; a diagonal block keeps j >= i
      if (!diag || j >= i) p.packed[tri_index(6 * b + j) + 6 * a + i] = s_v[tid] + (diag ? s_v[36 + sym6(i, j)] : 0.0);
    } else if (diag && tid < 42) {
      const int i = tid - 36;
      p.packed[tri_index(n) + 6 * a + i] = s_v[57 + i];            // rhs = row n of the augmented matrix
      p.packed[TRI + 6 * a + i] = s_v[63 + i];                     // g_c
      p.packed[TRI + n + 6 * a + i] = s_v[36 + sym6(i, i)];        // diag(U)
    }
    return;
  }
  double cost = 0.0, gn2 = 0.0, gmax = 0.0, fl = 0.0;
  int ff = 0;
  for (int k = tid; k < p.n_cost_blocks; k += 128) { cost += p.block_cost[k]; ff |= p.block_fail[k]; }
  for (int k = tid; k < p.n_pt_blocks; k += 128) {
    gmax = fmax(gmax, p.pt_part[3 * k]); gn2 += p.pt_part[3 * k + 1]; fl = fmax(fl, p.pt_part[3 * k + 2]);
  }
  cost = wave_sum(cost); gn2 = wave_sum(gn2); gmax = wave_max(gmax); fl = wave_max(fl);
  ff = __any(ff) ? 1 : 0;
  if ((tid & 63) == 0) { s_t[tid >> 6][0] = cost; s_t[tid >> 6][1] = gn2; s_t[tid >> 6][2] = gmax; s_t[tid >> 6][3] = fl; s_f[tid >> 6] = ff; }
  __syncthreads();
  if (tid == 0) {
    p.packed[TRI + 2 * n] = s_t[0][0] + s_t[1][0];
    p.packed[TRI + 2 * n + 1] = s_t[0][1] + s_t[1][1];
    p.packed[tri_index(n) + n] = 0.0;                                // the unused corner (n, n)
    p.scal[kGmaxPts] = fmax(s_t[0][2], s_t[1][2]);
    p.scal[kSchurFail] = fmax(s_t[0][3], s_t[1][3]);
    p.scal[kEvalFailLin] = (double)(s_f[0] | s_f[1]);
  }
}

// =====================================================================================================
// Reduced solve of a wide window: ONE workgroup, the packed lower triangle of the augmented matrix [S y; y^T .] in LDS
// (tri_index(n + 2) doubles: 150 KB at n = 192), plus y, sc, D2, gcs, gc.  Right-looking Cholesky in six-column panels --
// every thread of the panel rows factorises the 6x6 diagonal block itself and solves its own row; the trailing update goes
// by (row, six-column block) items from the window-shape table (solve_tables) -- three barriers per panel.  The rhs row
// factorises along (its factor row is L^-1 y), backward substitution by panels.  A pivot that is not positive (or not finite)
// marks the step invalid exactly as the narrow solve does; the epilogue is solve_epilogue.
// =====================================================================================================
constexpr int kSolveWideT = 1024;
__host__ __device__ inline size_t solve_wide_smem_bytes(int n) {
  const size_t N1 = (size_t)n + 1;
  return sizeof(double) * ((size_t)tri_index(n + 1) + 5 * N1);
}

__global__ __launch_bounds__(kSolveWideT) void k_solve_wide(SolveParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int nf = p.n_free, n = 6 * nf, N1 = n + 1, TRI = tri_index(N1);
  double* A = reinterpret_cast<double*>(smem_raw);     // packed lower triangle, row r at tri_index(r)
  double* y = A + TRI;                                 // [N1] solution of the scaled system
  double* sc = y + N1;
  double* D2 = sc + N1;
  double* gcs = D2 + N1;
  double* gc = gcs + N1;
  __shared__ int s_ok;
  const int tid = threadIdx.x;
  if (tid < n) {
    const double du = p.packed[TRI + n + tid];
    const double g = p.packed[TRI + tid];
    double s;
    if (p.init_scale) { s = p.jacobi ? 1.0 / (1.0 + sqrt(du)) : 1.0; p.sc[tid] = s; p.sc[n + tid] = du > 0.0 ? 1.0 : 0.0; }
    else s = p.sc[tid];
    sc[tid] = s;
    D2[tid] = fmin(fmax(s * s * du, p.min_diag), p.max_diag) / p.radius;
    gc[tid] = g;
    gcs[tid] = s * g;
  }
  if (tid == n) sc[n] = 1.0;
  if (tid == 0) s_ok = 1;
  __syncthreads();
  for (int t = tid; t < TRI; t += kSolveWideT) {
    const uint32_t w = p.tab[t];
    const int r = (int)(w >> 16), c = (int)(w & 0xffffu);
    double v = sc[c] * p.packed[t] * sc[r];
    if (r == c) v = (r < n) ? v + D2[r] : 0.0;
    A[t] = v;
  }
  __syncthreads();
  if (p.S_dbg) {
    for (int k = tid; k < n * n; k += kSolveWideT) {
      const int r = k / n, c = k - r * n;
      p.S_dbg[k] = (r >= c) ? A[tri_index(r) + c] : A[tri_index(c) + r];
    }
    for (int i = tid; i < n; i += kSolveWideT) p.rhs_dbg[i] = A[tri_index(n) + i];
  }
  // ---- factorisation: A = L L^T, row n becomes L^-1 y --------------------------------------------------------------
  const int n_items = (nf > 1) ? solve_item_base(nf, N1) : 0;
  for (int k = 0; k < nf; ++k) {
    const int c0 = 6 * k;
    const int r = c0 + tid;
    double l[6] = {0, 0, 0, 0, 0, 0};
    bool pd = true;
    if (r <= n) {
      double L[21], rd[6];
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int m = 0; m <= i; ++m) L[i * (i + 1) / 2 + m] = A[tri_index(c0 + i) + c0 + m];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double d = L[j * (j + 1) / 2 + j];
#pragma unroll
        for (int m = 0; m < j; ++m) d = fma(-L[j * (j + 1) / 2 + m], L[j * (j + 1) / 2 + m], d);
        const bool ok = (d > 0.0) && isfinite(d);
        pd = pd && ok;
        const double ljj = sqrt(ok ? d : 1.0);
        L[j * (j + 1) / 2 + j] = ljj;
        rd[j] = 1.0 / ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
          double v = L[i * (i + 1) / 2 + j];
#pragma unroll
          for (int m = 0; m < j; ++m) v = fma(-L[i * (i + 1) / 2 + m], L[j * (j + 1) / 2 + m], v);
          L[i * (i + 1) / 2 + j] = v * rd[j];
        }
      }
      const int own = r - c0;
      if (own < 6) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int m = 0; m <= i; ++m) if (i == own) l[m] = L[i * (i + 1) / 2 + m];      // (entries right of the diagonal: not stored)
      } else {
        const double* arow = A + tri_index(r) + c0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          double v = arow[j];
#pragma unroll
          for (int m = 0; m < j; ++m) v = fma(-l[m], L[j * (j + 1) / 2 + m], v);
          l[j] = v * rd[j];
        }
      }
    }
    __syncthreads();      // every reader of the diagonal block and of its own row is done
    if (r <= n) {
      const int own = r - c0;
#pragma unroll
      for (int m = 0; m < 6; ++m) if (own >= 6 || m <= own) A[tri_index(r) + c0 + m] = l[m];
      if (own == 0 && !pd) s_ok = 0;
    }
    __syncthreads();
    for (int it = (k + 1 < nf ? solve_item_base(k + 1, N1) : n_items) + tid; it < n_items; it += kSolveWideT) {
      const uint32_t wd = p.tab[TRI + it];
      const int rr = (int)(wd & 0xffffu), j = (int)(wd >> 16);
      const double* lr = A + tri_index(rr) + c0;
      double wr[6];
#pragma unroll
      for (int m = 0; m < 6; ++m) wr[m] = lr[m];
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        const int c = 6 * j + e;
        if (c > rr) break;
        const double* lc = A + tri_index(c) + c0;
        double acc = A[tri_index(rr) + c];
#pragma unroll
        for (int m = 0; m < 6; ++m) acc = fma(-wr[m], lc[m], acc);
        A[tri_index(rr) + c] = acc;
      }
    }
    __syncthreads();
  }
  // ---- backward substitution L^T x = z (z = row n), panel by panel --------------------------------------------------
  double* z = A + tri_index(n);
  for (int k = nf - 1; k >= 0; --k) {
    const int c0 = 6 * k;
    if (tid == 0) {
      for (int j = c0 + 5; j >= c0; --j) {
        double v = z[j];
        for (int i = j + 1; i < c0 + 6; ++i) v = fma(-A[tri_index(i) + j], y[i], v);
        y[j] = v / A[tri_index(j) + j];
      }
    }
    __syncthreads();
    if (tid < c0) {
      double v = z[tid];
#pragma unroll
      for (int m = 0; m < 6; ++m) v = fma(-A[tri_index(c0 + m) + tid], y[c0 + m], v);
      z[tid] = v;
    }
    __syncthreads();
  }
  solve_epilogue<kSolveWideT>(p, n, y, sc, D2, gcs, gc, s_ok != 0, tid);
}

}  // namespace pba
