// pba_prior.h -- the camera prior (pba_set_camera_prior) and the marginalisation that produces one (pba_marginalize).
//
// The prior is ONE extra residual block on the camera blocks `slots`, in information form: with d = cameras(slots) - x0,
//   E(d) = c + eta^T d + d^T Lambda d / 2,   gradient eta + Lambda d,   Gauss-Newton block Lambda  (constant Jacobian, no loss).
// It touches cameras only, so it is an addend to the packed reduced system (pba_solve.h) between the reduction of the Schur partials
// and the reduced solve, and an addend to the candidate cost:
//   k_prior          ONE workgroup: d, the mat-vec Lambda d row by row, E; adds g / diag Lambda / Lambda / E to the packed sums, or to a
//                    dense system (pba_marginalize), and / or E to a scalar (the candidate cost), and / or writes g | E out
// The marginalisation eliminates the points M that the dropped slots see, then the free dropped cameras, from the undamped, unscaled
// normal equations of M's residual blocks (plus the current prior):
//   k_marg_point     one lane per point of M: V, g_p, the equilibrated 3x3 Cholesky factor X of V^-1 (the arithmetic of k_cov_point),
//                    z = X g_p; per workgroup the smallest pivot, the first failing point, the cost of M's blocks, |z|^2 / 2
//   k_marg_schur     one workgroup per pair of free camera columns: the pair block of U - sum_M W P W^T (k_cov_schur restricted to M;
//                    pba_cov.h itself stays as it is, so that pba_covariance keeps its bits)
//   k_marg_grad      one workgroup per free camera column: g_c - sum_M W V^-1 g_p = -sum Ac^T (b + G z)
//   k_marg_eliminate ONE workgroup: unit-diagonal Cholesky of the dropped cameras' block S_DD, Y = L^-1 D^-1/2 [S_DK | r_D],
//                    Lambda = S_KK - Y^T Y (lower triangle computed, mirrored), eta = r_K - Y^T y, |y|^2 / 2
// Every sum has a fixed order; there are no floating-point atomics: two fresh engines give the same bits.
// Included by pba_engine.hip after pba_cov.h.
#pragma once
#include "pba_cov.h"

namespace pba {

constexpr int kPriorThreads = 128;
constexpr int kPriorMaxDim = 6 * kMaxFrames;
static_assert(kPriorMaxDim <= kPriorThreads, "one thread per prior row");

struct PriorParams {
  const double* x0;              // [6 k]
  const double* eta;             // [6 k]
  const double* Lambda;          // [6 k][6 k] row-major
  const double* cams;            // [n_frames][6] the cameras the term is evaluated at
  double* out;                   // [6 k + 1] gradient over all prior rows | E; may be null
  double* packed;                // packed reduced system (tri layout) to add to; may be null
  double* S;                     // dense [ld][ld] system and its gradient r [ld] to add to (pba_marginalize); may be null
  double* r;
  double* add_to;                // *add_to += E; may be null
  double c;
  int32_t k, n_free, ld;
  uint8_t slot[kMaxFrames];      // slot of prior block i
  int8_t col[kMaxFrames];        // its camera column in the destination, -1: the slot is constant there
};

__global__ __launch_bounds__(kPriorThreads) void k_prior(PriorParams p) {
  __shared__ double s_d[kPriorMaxDim], s_t[kPriorMaxDim];
  __shared__ double s_E;
  const int tid = threadIdx.x, m = 6 * p.k;
  if (tid < m) s_d[tid] = p.cams[6 * p.slot[tid / 6] + tid % 6] - p.x0[tid];
  __syncthreads();
  double g = 0.0;
  if (tid < m) {
    const double* row = p.Lambda + (size_t)tid * m;
    double w = 0.0;
    for (int j = 0; j < m; ++j) w += row[j] * s_d[j];      // row order
    g = p.eta[tid] + w;
    s_t[tid] = p.eta[tid] * s_d[tid] + 0.5 * s_d[tid] * w;
  }
  __syncthreads();
  if (tid == 0) {
    double E = p.c;
    for (int i = 0; i < m; ++i) E += s_t[i];
    s_E = E;
  }
  __syncthreads();
  const double E = s_E;
  if (p.out) {
    if (tid < m) p.out[tid] = g;
    if (tid == 0) p.out[m] = E;
  }
  if (p.add_to && tid == 0) *p.add_to += E;
  const int ca = tid < m ? p.col[tid / 6] : -1;
  if (p.packed) {
    // every destination belongs to one thread: row ci of the triangle, entry ci of the rhs row, of g and of diag U; the cost
    const int n = 6 * p.n_free, TRI = tri_index(n + 1);
    if (ca >= 0) {
      const int ci = 6 * ca + tid % 6;
      const double* row = p.Lambda + (size_t)tid * m;
      for (int j = 0; j <= tid; ++j) {
        const int cb = p.col[j / 6];
        if (cb >= 0) p.packed[tri_index(ci) + 6 * cb + j % 6] += row[j];      // (slots ascend: columns do)
      }
      p.packed[tri_index(n) + ci] += g;
      p.packed[TRI + ci] += g;
      p.packed[TRI + n + ci] += row[tid];
    }
    if (tid == 0) p.packed[TRI + 2 * n] += E;
  }
  if (p.S && ca >= 0) {
    const int ci = 6 * ca + tid % 6;
    for (int j = 0; j < m; ++j) {
      const int cb = p.col[j / 6];
      if (cb < 0) continue;
      const double v = j <= tid ? p.Lambda[(size_t)tid * m + j] : p.Lambda[(size_t)j * m + tid];      // the lower triangle, both ways
      p.S[(size_t)ci * p.ld + 6 * cb + j % 6] += v;
    }
    p.r[ci] += g;
  }
}

// =====================================================================================================
// marginalisation
// =====================================================================================================
constexpr int kMargPart = 4;           // per workgroup of k_marg_point: smallest pivot | first failing point (kCovNone) | cost | |z|^2 / 2

struct MargPointParams {
  const double* xyz;
  const CamGeom* geom;
  const double* rec;             // [6][rec_stride] records of the Jacobian pass
  const int32_t* pt_begin;
  const uint8_t* obs_slot;
  double* X;                     // [n_points][6] factor of V^-1 (lower triangular, row by row); zero outside M
  double* z;                     // [n_points][3] X g_p; zero outside M
  double* part;                  // [gridDim.x][kMargPart]
  int64_t rec_stride;
  int32_t n_points, n_frames;
  uint32_t drop_mask;
  double fx, fy;
};

// the point is in M: one of its observations is in a dropped slot
__device__ __forceinline__ bool marg_in_set(const uint8_t* __restrict__ obs_slot, int o0, int o1, uint32_t drop_mask) {
  bool in = false;
  for (int o = o0; o < o1; ++o) in = in || ((drop_mask >> obs_slot[o]) & 1u);
  return in;
}

__global__ __launch_bounds__(kCovThreads) void k_marg_point(MargPointParams p) {
  __shared__ CamGeom s_geom[kMaxFrames];
  __shared__ double s_red[kCovWaves][kMargPart];
  const int tid = threadIdx.x;
  stage_geom<kCovThreads, false, kMaxFrames>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const int pt = blockIdx.x * kCovThreads + tid;
  double piv = 1.0, bad = kCovNone, cost = 0.0, zz = 0.0;
  if (pt < p.n_points) {
    const int o0 = p.pt_begin[pt], o1 = p.pt_begin[pt + 1];
    double Xm[6] = {0, 0, 0, 0, 0, 0}, zv[3] = {0, 0, 0};
    if (marg_in_set(p.obs_slot, o0, o1, p.drop_mask)) {
      const double X[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
      double V[6] = {0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0};
      for (int o = o0; o < o1; ++o) {      // list order
        cost += p.rec[5 * p.rec_stride + o];
        double Ac[2][6], MAp[2][3], Ap[2][3], M[3];
        cov_observation(s_geom[p.obs_slot[o]], X, nullptr, nullptr, p.rec, p.rec_stride, o, p.fx, p.fy, Ac, MAp, Ap, M);
        const double b0 = p.rec[3 * p.rec_stride + o], b1 = p.rec[4 * p.rec_stride + o];
        V[0] += Ap[0][0] * MAp[0][0] + Ap[1][0] * MAp[1][0];
        V[1] += Ap[0][0] * MAp[0][1] + Ap[1][0] * MAp[1][1];
        V[2] += Ap[0][0] * MAp[0][2] + Ap[1][0] * MAp[1][2];
        V[3] += Ap[0][1] * MAp[0][1] + Ap[1][1] * MAp[1][1];
        V[4] += Ap[0][1] * MAp[0][2] + Ap[1][1] * MAp[1][2];
        V[5] += Ap[0][2] * MAp[0][2] + Ap[1][2] * MAp[1][2];
#pragma unroll
        for (int k = 0; k < 3; ++k) gp[k] -= Ap[0][k] * b0 + Ap[1][k] * b1;      // g = -A^T b
      }
      // unit-diagonal block: a10 a20 a21 are correlations, the pivots are 1, d1, d2 (k_cov_point's factorisation)
      bool ok = cov_pivot_ok(V[0]) && cov_pivot_ok(V[3]) && cov_pivot_ok(V[5]);
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
        const double x11 = 1.0 / l11, x22 = 1.0 / l22;
        const double x10 = -l10 * x11;
        const double x21 = -l21 * x11 * x22;
        const double x20 = -(l20 + l21 * x10) * x22;
        Xm[0] = e0; Xm[1] = x10 * e0; Xm[2] = x11 * e1; Xm[3] = x20 * e0; Xm[4] = x21 * e1; Xm[5] = x22 * e2;
        zv[0] = Xm[0] * gp[0];
        zv[1] = Xm[1] * gp[0] + Xm[2] * gp[1];
        zv[2] = Xm[3] * gp[0] + Xm[4] * gp[1] + Xm[5] * gp[2];
        zz = 0.5 * (zv[0] * zv[0] + zv[1] * zv[1] + zv[2] * zv[2]);
      } else {
        bad = (double)pt;
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) p.X[6 * (size_t)pt + k] = Xm[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p.z[3 * (size_t)pt + k] = zv[k];
  }
  // workgroup partials: butterfly per wave, the waves in order
  piv = wave_min(piv); bad = wave_min(bad); cost = wave_sum(cost); zz = wave_sum(zz);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = piv; s_red[tid >> 6][1] = bad; s_red[tid >> 6][2] = cost; s_red[tid >> 6][3] = zz; }
  __syncthreads();
  if (tid == 0) {
    double m = s_red[0][0], b = s_red[0][1], c = s_red[0][2], q = s_red[0][3];
    for (int w = 1; w < kCovWaves; ++w) { m = fmin(m, s_red[w][0]); b = fmin(b, s_red[w][1]); c += s_red[w][2]; q += s_red[w][3]; }
    double* o4 = p.part + kMargPart * (size_t)blockIdx.x;
    o4[0] = m; o4[1] = b; o4[2] = c; o4[3] = q;
  }
}

struct MargSchurParams {
  const double* xyz;
  const CamGeom* geom;
  const double* rec;
  const int32_t* pt_begin;
  const uint8_t* obs_slot;
  const double* X;               // [n_points][6] (k_marg_point)
  const double* z;               // [n_points][3]
  double* S;                     // [n][n] row-major, n = 6 n_cols, both triangles from the one computed value
  double* r;                     // [n] reduced gradient
  int64_t rec_stride;
  int32_t n_points, n_cols;
  uint32_t drop_mask;
  double fx, fy;
  uint8_t slot_of_col[kMaxFrames];
};

// Workgroup q: the pair (a, b), a <= b, of camera columns enumerated row by row.  k_cov_schur's walk and sums (per lane in point order,
// butterfly per wave, the waves in order) over the points of M only.
__global__ __launch_bounds__(kCovThreads) void k_marg_schur(MargSchurParams p) {
  __shared__ CamGeom s_geom[2];
  __shared__ double s_red[kCovWaves][36];
  const int tid = threadIdx.x;
  const int nc = p.n_cols, n = 6 * nc;
  int a = 0, rem = blockIdx.x;
  while (rem >= nc - a) { rem -= nc - a; ++a; }
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
    if (!seen_a || !seen_b || !marg_in_set(p.obs_slot, o0, o1, p.drop_mask)) continue;
    const double X[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
    double Xm[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) Xm[k] = p.X[6 * (size_t)pt + k];
    for (int l = o0; l < o1; ++l) {
      if (p.obs_slot[l] != sa) continue;
      double Aca[2][6], MApa[2][3], Apa[2][3], Ma[3];
      cov_observation(s_geom[0], X, nullptr, nullptr, p.rec, p.rec_stride, l, p.fx, p.fy, Aca, MApa, Apa, Ma);
      if (a == b) {
        double MAc[2][6];
#pragma unroll
        for (int j = 0; j < 6; ++j) { MAc[0][j] = Ma[0] * Aca[0][j] + Ma[1] * Aca[1][j]; MAc[1][j] = Ma[1] * Aca[0][j] + Ma[2] * Aca[1][j]; }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) acc[6 * i + j] += Aca[0][i] * MAc[0][j] + Aca[1][i] * MAc[1][j];
      }
      double Ga[2][3];
      cov_times_factor(MApa, Xm, Ga);
      for (int m = o0; m < o1; ++m) {
        if (p.obs_slot[m] != sb) continue;
        double Acb[2][6], MApb[2][3], Apb[2][3], Mb[3];
        cov_observation(s_geom[1], X, nullptr, nullptr, p.rec, p.rec_stride, m, p.fx, p.fy, Acb, MApb, Apb, Mb);
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
    if (a != b) {
      p.S[(size_t)(6 * a + i) * n + 6 * b + j] = v;
      p.S[(size_t)(6 * b + j) * n + 6 * a + i] = v;
    } else if (i >= j) {
      p.S[(size_t)(6 * a + i) * n + 6 * a + j] = v;
      p.S[(size_t)(6 * a + j) * n + 6 * a + i] = v;
    }
  }
}

// Workgroup a: the reduced gradient of camera column a over the points of M, r_a = sum_l -Ac_l^T (b_l + G_l z), G_l = (M Ap)_l X^T
__global__ __launch_bounds__(kCovThreads) void k_marg_grad(MargSchurParams p) {
  __shared__ CamGeom s_geom;
  __shared__ double s_red[kCovWaves][6];
  const int tid = threadIdx.x;
  const int a = blockIdx.x, sa = p.slot_of_col[a];
  if (tid == 0) s_geom = p.geom[sa];
  __syncthreads();
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int pt = tid; pt < p.n_points; pt += kCovThreads) {
    const int o0 = p.pt_begin[pt], o1 = p.pt_begin[pt + 1];
    bool seen = false;
    for (int o = o0; o < o1; ++o) seen = seen || p.obs_slot[o] == sa;
    if (!seen || !marg_in_set(p.obs_slot, o0, o1, p.drop_mask)) continue;
    const double X[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
    double Xm[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) Xm[k] = p.X[6 * (size_t)pt + k];
    const double z0 = p.z[3 * (size_t)pt], z1 = p.z[3 * (size_t)pt + 1], z2 = p.z[3 * (size_t)pt + 2];
    for (int l = o0; l < o1; ++l) {
      if (p.obs_slot[l] != sa) continue;
      double Ac[2][6], MAp[2][3], Ap[2][3], M[3], G[2][3];
      cov_observation(s_geom, X, nullptr, nullptr, p.rec, p.rec_stride, l, p.fx, p.fy, Ac, MAp, Ap, M);
      cov_times_factor(MAp, Xm, G);
      const double t0 = p.rec[3 * p.rec_stride + l] + (G[0][0] * z0 + G[0][1] * z1 + G[0][2] * z2);
      const double t1 = p.rec[4 * p.rec_stride + l] + (G[1][0] * z0 + G[1][1] * z1 + G[1][2] * z2);
#pragma unroll
      for (int i = 0; i < 6; ++i) acc[i] -= Ac[0][i] * t0 + Ac[1][i] * t1;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double v = wave_sum(acc[k]);
    if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < 6) {
    double v = s_red[0][tid];
#pragma unroll
    for (int w = 1; w < kCovWaves; ++w) v += s_red[w][tid];
    p.r[6 * a + tid] = v;
  }
}

// Elimination of the dropped free cameras D from [S r]: ONE workgroup.  LDS: the unit-diagonal S_DD [nd][nd + 1] (lower triangle), then
// Y [nd][nk + 1] = D^-1/2 [S_DK | r_D], then the nd scales.  A pivot that is not positive or not finite ends the kernel:
// info = {smallest pivot so far, its row of S_DD, .}, nothing else is written.  nd = 0: Lambda = S_KK, eta = r_K.
constexpr int kMargElimThreads = 256;
__host__ __device__ inline size_t marg_eliminate_smem_bytes(int nd, int nk) {
  return sizeof(double) * ((size_t)nd * (nd + 1) + (size_t)nd * (nk + 1) + (size_t)nd + 1);
}
struct MargEliminateParams {
  const double* S;               // [n][n], n = 6 (nd_cams + nk_cams)
  const double* r;               // [n]
  double* Lambda;                // [nk][nk] symmetric bit for bit
  double* eta;                   // [nk]
  double* info;                  // [3] smallest pivot of the unit-diagonal S_DD | failing row, -1: none | |y|^2 / 2
  int32_t n, nd_cams, nk_cams;
  uint8_t col_d[kMaxFrames];     // camera columns of S that are eliminated / kept, ascending
  uint8_t col_k[kMaxFrames];
};

__global__ __launch_bounds__(kMargElimThreads) void k_marg_eliminate(MargEliminateParams p) {
  extern __shared__ __attribute__((aligned(16))) char marg_smem[];
  constexpr int T = kMargElimThreads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = p.n, nd = 6 * p.nd_cams, nk = 6 * p.nk_cams, ld = nd + 1, ly = nk + 1;
  double* A = reinterpret_cast<double*>(marg_smem);      // [nd][ld]
  double* Y = A + (size_t)nd * ld;                       // [nd][ly]
  double* dinv = Y + (size_t)nd * ly;                    // [nd]
  __shared__ int s_bad;
  auto row_d = [&](int i) { return 6 * (int)p.col_d[i / 6] + i % 6; };
  auto row_k = [&](int i) { return 6 * (int)p.col_k[i / 6] + i % 6; };
  if (tid == 0) {
    int bad = -1;
    for (int i = 0; i < nd && bad < 0; ++i)
      if (!cov_pivot_ok(p.S[(size_t)row_d(i) * n + row_d(i)])) bad = i;      // the FIRST bad diagonal entry
    s_bad = bad;
  }
  __syncthreads();
  if (s_bad >= 0) {
    if (tid == 0) { p.info[0] = 0.0; p.info[1] = (double)s_bad; p.info[2] = 0.0; }
    return;
  }
  for (int i = tid; i < nd; i += T) dinv[i] = 1.0 / sqrt(p.S[(size_t)row_d(i) * n + row_d(i)]);
  __syncthreads();
  for (int i = wave; i < nd; i += T / 64) {
    const int ri = row_d(i);
    for (int c = lane; c <= i; c += 64) A[(size_t)i * ld + c] = (i == c) ? 1.0 : p.S[(size_t)ri * n + row_d(c)] * dinv[i] * dinv[c];
    for (int c = lane; c < ly; c += 64) Y[(size_t)i * ly + c] = (c < nk ? p.S[(size_t)ri * n + row_k(c)] : p.r[ri]) * dinv[i];
  }
  __syncthreads();
  // ---- S_DD = L L^T, right-looking, one column at a time; every thread reads the pivot ------------------------------------------------
  double piv = 1.0;
  for (int j = 0; j < nd; ++j) {
    const double d = A[(size_t)j * ld + j];
    if (!cov_pivot_ok(d)) {
      if (tid == 0) { p.info[0] = piv; p.info[1] = (double)j; p.info[2] = 0.0; }
      return;
    }
    piv = fmin(piv, d);
    const double ljj = sqrt(d);
    __syncthreads();                           // every thread has read the pivot
    for (int rr = j + tid; rr < nd; rr += T) A[(size_t)rr * ld + j] = (rr == j) ? ljj : A[(size_t)rr * ld + j] / ljj;
    __syncthreads();
    for (int rr = j + 1 + wave; rr < nd; rr += T / 64) {
      const double lrj = A[(size_t)rr * ld + j];
      for (int c = j + 1 + lane; c <= rr; c += 64) A[(size_t)rr * ld + c] -= lrj * A[(size_t)c * ld + j];
    }
    __syncthreads();
  }
  // ---- Y <- L^-1 Y: one thread per column, rows in ascending order ----------------------------------------------------------------------
  for (int c = tid; c < ly; c += T) {
    for (int i = 0; i < nd; ++i) {
      double v = Y[(size_t)i * ly + c];
      for (int k = 0; k < i; ++k) v -= A[(size_t)i * ld + k] * Y[(size_t)k * ly + c];
      Y[(size_t)i * ly + c] = v / A[(size_t)i * ld + i];
    }
  }
  __syncthreads();
  // ---- Lambda = S_KK - Y^T Y (i >= j computed, mirrored), eta = r_K - Y^T y ------------------------------------------------------------------
  for (int t = tid; t < nk * (nk + 1) / 2; t += T) {
    int i, j;
    tri_row_col(t, i, j);
    double v = p.S[(size_t)row_k(i) * n + row_k(j)];
    for (int d = 0; d < nd; ++d) v -= Y[(size_t)d * ly + i] * Y[(size_t)d * ly + j];
    p.Lambda[(size_t)i * nk + j] = v;
    p.Lambda[(size_t)j * nk + i] = v;
  }
  for (int i = tid; i < nk; i += T) {
    double v = p.r[row_k(i)];
    for (int d = 0; d < nd; ++d) v -= Y[(size_t)d * ly + i] * Y[(size_t)d * ly + nk];
    p.eta[i] = v;
  }
  if (tid == 0) {
    double q = 0.0;
    for (int d = 0; d < nd; ++d) q += Y[(size_t)d * ly + nk] * Y[(size_t)d * ly + nk];
    p.info[0] = piv; p.info[1] = -1.0; p.info[2] = 0.5 * q;
  }
}

}  // namespace pba
