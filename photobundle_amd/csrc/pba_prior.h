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
//   k_marg_point     one lane per point of M: V, g_p, the equilibrated 3x3 Cholesky factor X of V^-1 (elim_factor_point's arithmetic),
//                    z = X g_p; per workgroup the smallest pivot, the first failing point, the cost of M's blocks, |z|^2 / 2
//   k_elim_pair      (pba_elim.h) one workgroup per pair of free camera columns: the pair block of U - sum_M W P W^T, the points of M
//                    selected by the mask of the dropped slots
//   k_marg_grad      one workgroup per free camera column: g_c - sum_M W V^-1 g_p = -sum Ac^T (b + G z)
//   k_marg_eliminate ONE workgroup: unit-diagonal Cholesky of the dropped cameras' block S_DD, Y = L^-1 D^-1/2 [S_DK | r_D],
//                    Lambda = S_KK - Y^T Y (lower triangle computed, mirrored), eta = r_K - Y^T y, |y|^2 / 2
// Every sum has a fixed order; there are no floating-point atomics: two fresh engines give the same bits.
// Included by pba_engine.hip after pba_cov.h.
#pragma once
#include "pba_elim.h"

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
constexpr int kMargPart = elim_part_width(2);      // per workgroup of k_marg_point: smallest pivot | first failing point | cost | |z|^2 / 2

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
  uint32_t drop_mask;            // the point is in M: one of its observations is in a dropped slot
  double fx, fy;
};

__global__ __launch_bounds__(kElimThreads) void k_marg_point(MargPointParams p) {
  __shared__ CamGeom s_geom[kMaxFrames];
  const int tid = threadIdx.x;
  stage_geom<kElimThreads, false, kMaxFrames>(p.geom, s_geom, p.n_frames, tid);
  __syncthreads();
  const int pt = blockIdx.x * kElimThreads + tid;
  double piv = 1.0, bad = kElimNone, cost = 0.0, zz = 0.0;
  if (pt < p.n_points) {
    const int o0 = p.pt_begin[pt], o1 = p.pt_begin[pt + 1];
    double Xm[6] = {0, 0, 0, 0, 0, 0}, zv[3] = {0, 0, 0};
    if (elim_in_set(p.obs_slot, o0, o1, p.drop_mask)) {
      const double X[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
      double V[6] = {0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0};
      for (int o = o0; o < o1; ++o) {      // list order
        cost += p.rec[5 * p.rec_stride + o];
        double Ac[2][6], MAp[2][3], Ap[2][3], M[3];
        elim_observation(s_geom[p.obs_slot[o]], X, nullptr, nullptr, p.rec, p.rec_stride, o, p.fx, p.fy, Ac, MAp, Ap, M);
        const double b0 = p.rec[3 * p.rec_stride + o], b1 = p.rec[4 * p.rec_stride + o];
        // (elim_add_point_block, written out: through the function this kernel is allocated 64 registers instead of 70 and its other
        // code runs 0.76 us longer at 5 000 and at 50 000 points, profiles/refactor/elimination_ab_timing.txt)
        V[0] += Ap[0][0] * MAp[0][0] + Ap[1][0] * MAp[1][0];
        V[1] += Ap[0][0] * MAp[0][1] + Ap[1][0] * MAp[1][1];
        V[2] += Ap[0][0] * MAp[0][2] + Ap[1][0] * MAp[1][2];
        V[3] += Ap[0][1] * MAp[0][1] + Ap[1][1] * MAp[1][1];
        V[4] += Ap[0][1] * MAp[0][2] + Ap[1][1] * MAp[1][2];
        V[5] += Ap[0][2] * MAp[0][2] + Ap[1][2] * MAp[1][2];
#pragma unroll
        for (int k = 0; k < 3; ++k) gp[k] -= Ap[0][k] * b0 + Ap[1][k] * b1;      // g = -A^T b
      }
      // elim_factor_point's arithmetic, written out: with the shared function in its place (z formed here or inside it, with or without
      // its inverse) the compiler's code for this kernel gives another z, and the reduced gradient and eta move in their last bits against
      // tests/golden/elimination_bits.json.  A change to the factorisation is made in both places.
      bool ok = elim_pivot_ok(V[0]) && elim_pivot_ok(V[3]) && elim_pivot_ok(V[5]);
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
  elim_point_partial<2>(piv, bad, cost, zz, p.part + kMargPart * (size_t)blockIdx.x);
}

// Workgroup a: the reduced gradient of camera column a over the points of M, r_a = sum_l -Ac_l^T (b_l + G_l z), G_l = (M Ap)_l X^T
__global__ __launch_bounds__(kElimThreads) void k_marg_grad(ElimPairParams p) {
  __shared__ CamGeom s_geom;
  __shared__ double s_red[kElimWaves][6];
  const int tid = threadIdx.x;
  const int a = blockIdx.x, sa = p.slot_of_col[a];
  if (tid == 0) s_geom = p.geom[sa];
  __syncthreads();
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int pt = tid; pt < p.n_points; pt += kElimThreads) {
    const int o0 = p.pt_begin[pt], o1 = p.pt_begin[pt + 1];
    bool seen = false;
    for (int o = o0; o < o1; ++o) seen = seen || p.obs_slot[o] == sa;
    if (!seen || !elim_in_set(p.obs_slot, o0, o1, p.point_mask)) continue;
    const double X[3] = {p.xyz[3 * (size_t)pt], p.xyz[3 * (size_t)pt + 1], p.xyz[3 * (size_t)pt + 2]};
    double Xm[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) Xm[k] = p.X[6 * (size_t)pt + k];
    const double z0 = p.z[3 * (size_t)pt], z1 = p.z[3 * (size_t)pt + 1], z2 = p.z[3 * (size_t)pt + 2];
    for (int l = o0; l < o1; ++l) {
      if (p.obs_slot[l] != sa) continue;
      double Ac[2][6], MAp[2][3], Ap[2][3], M[3], G[2][3];
      elim_observation(s_geom, X, nullptr, nullptr, p.rec, p.rec_stride, l, p.fx, p.fy, Ac, MAp, Ap, M);
      elim_times_factor(MAp, Xm, G);
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
    for (int w = 1; w < kElimWaves; ++w) v += s_red[w][tid];
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
      if (!elim_pivot_ok(p.S[(size_t)row_d(i) * n + row_d(i)])) bad = i;      // the FIRST bad diagonal entry
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
    if (!elim_pivot_ok(d)) {
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
