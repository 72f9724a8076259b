// pba_sgm.hip -- semi-global stereo matching (the reference's StereoAlgorithm = SGM, restated in DESIGN.md 4.10) on gfx950, behind
// the C-ABI of include/pba_sgm.h.  Every volume is [rows][cols][D] with d fastest.  Kernels per pair, in launch order:
//
//   k_sgm_prefilter   one thread per pixel of both images: capped Sobel (u8) and the census code (i32).
//   k_sgm_rowagg      one thread per (y, x, d): the pixel cost (half-pixel interval cost on the Sobel rows + weighted census hamming,
//                     added in u8) summed over x - r .. x + r with clamped columns -> A (u16).
//   k_sgm_cost        one thread per (x, d), serial over y: row 0 in wrapping u16, the rows below it by the saturating int16
//                     recurrence C[y] = (C[y-1] -s A[max(y-r-1, 0)]) +s A[y+r] -> C_L (u16), written once.  C_R is never
//                     materialised: C_R(y, x, d) = C_L(y, x + dd, dd), dd = min(d, W - 1 - x).
//   k_sgm_path  x 4   one wave per line (a row or a column) of one image, lanes over d, serial along the line; the previous
//                     pixel's path costs live in LDS (double buffered, SHRT_MAX sentinels at d = -1 and d = D), the running
//                     minimum goes through a wave reduction.  Launched forward-row, forward-column, backward-row, backward-column;
//                     each launch read-modify-writes the sum volume S with a saturating add, so S saturates where the reference's
//                     does.  blockIdx.y picks the image; the right solve's S lives in A's storage (dead after k_sgm_cost).
//   k_sgm_wta         one thread per pixel of both solves: first minimum of S, sub-pixel step in fp64 (correctly rounded
//                     divisions, no contraction), uint16 map.
//   k_ccl_*           speckle filter of both maps: union-find over the edge rule (integer atomicMin on parent links), component
//                     sizes by integer atomicAdd on the root, then the zeroing pass.  Roots are component minima and sizes are
//                     counts, so neither depends on scheduling.
//   k_sgm_lr_depth    left-right check of the left map, float disparity and the fused depth.
//
// There is no CPU fallback: pba_sgm_create fails with PBA_ERR_NO_DEVICE when no GPU is visible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/pba_sgm.h"
#include "pba_handle.h"

namespace {

constexpr int kWave = 64;
constexpr int kSpeckleSize = 100;
constexpr int kMaxLdsDisparities = 16368;   // 2 * (D + 2) int16 of path state within 64 KiB of LDS

struct HammingTable {
  uint8_t v[26];   // (u8)(hamming * censusWeightFactor) for hamming = 0 .. 25, formed on the host in double
};

__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }

// blockIdx.z = image (0 left, 1 right); img / sobel / census hold the two images back to back
__global__ __launch_bounds__(256) void k_sgm_prefilter(const uint8_t* __restrict__ img, uint8_t* __restrict__ sobel,
                                                       int32_t* __restrict__ census, int H, int W, int cap, int cr) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= W) return;
  const size_t npix = (size_t)H * W;
  const uint8_t* I = img + blockIdx.z * npix;
  int s = cap;
  if (x > 0 && x < W - 1 && y > 0 && y < H - 1) {
    const uint8_t* a = I + (size_t)(y - 1) * W;
    const uint8_t* b = I + (size_t)y * W;
    const uint8_t* c = I + (size_t)(y + 1) * W;
    const int v = (a[x + 1] + 2 * b[x + 1] + c[x + 1]) - (a[x - 1] + 2 * b[x - 1] + c[x - 1]);
    s = v > cap ? 2 * cap : (v < -cap ? 0 : v + cap);
  }
  const int centre = I[(size_t)y * W + x];
  int code = 0;
  for (int oy = -cr; oy <= cr; ++oy)
    for (int ox = -cr; ox <= cr; ++ox) {
      code <<= 1;
      const int yy = y + oy, xx = x + ox;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W && I[(size_t)yy * W + xx] >= centre) code += 1;
    }
  const size_t o = blockIdx.z * npix + (size_t)y * W + x;
  sobel[o] = (uint8_t)s;
  census[o] = code;
}

// min and max of a Sobel row's value at x and its two half-pixel neighbours (integer halves; the row ends repeat the centre)
__device__ __forceinline__ void half_interval(const uint8_t* __restrict__ row, int W, int x, int& c, int& lo, int& hi) {
  c = row[x];
  const int l = x > 0 ? (c + row[x - 1]) / 2 : c;
  const int r = x < W - 1 ? (c + row[x + 1]) / 2 : c;
  lo = min(min(l, r), c);
  hi = max(max(l, r), c);
}

// grid (ceil(W * D / 256), H): A[y][x][d] = sum over i = -r .. r of the pixel cost at (y, clamp(x + i), d)
__global__ __launch_bounds__(256) void k_sgm_rowagg(const uint8_t* __restrict__ sobel, const int32_t* __restrict__ census,
                                                    uint16_t* __restrict__ A, int H, int W, int D, int r, HammingTable ht) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (e >= W * D) return;
  const int x = e / D, d = e - x * D;
  const size_t npix = (size_t)H * W;
  const uint8_t* sl = sobel + (size_t)y * W;
  const uint8_t* sr = sobel + npix + (size_t)y * W;
  const int32_t* cl = census + (size_t)y * W;
  const int32_t* cr = census + npix + (size_t)y * W;
  int sum = 0;
  for (int i = -r; i <= r; ++i) {
    const int xx = min(max(x + i, 0), W - 1);
    const int xr = max(xx - d, 0);   // d > x repeats d = x
    int lc, lmin, lmax, rc, rmin, rmax;
    half_interval(sl, W, xx, lc, lmin, lmax);
    half_interval(sr, W, xr, rc, rmin, rmax);
    const int l2r = max(max(0, lc - rmax), rmin - lc);
    const int r2l = max(max(0, rc - lmax), lmin - rc);
    const int ham = __popc((unsigned)(cl[xx] ^ cr[xr]));
    sum += (min(l2r, r2l) + ht.v[ham]) & 0xFF;
  }
  A[((size_t)y * W) * D + e] = (uint16_t)sum;   // <= 19 * 255
}

// grid ceil(W * D / 256): thread (x, d) walks down its column of the volume
__global__ __launch_bounds__(256) void k_sgm_cost(const uint16_t* __restrict__ A, uint16_t* __restrict__ C, int H, int W, int D, int r) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= W * D) return;
  const size_t row = (size_t)W * D;
  unsigned top = (unsigned)(r + 1) * A[e];
  for (int i = 1; i <= r; ++i) top += A[i * row + e];   // rows >= r + 1 is validated
  C[e] = (uint16_t)top;
  int prev = (int16_t)(uint16_t)top;
  const bool col0 = e < D;
  for (int y = 1; y < H; ++y) {
    int cur = 0;
    if (y + r < H && !col0) {
      cur = sat16(sat16(prev - (int)A[(size_t)max(y - r - 1, 0) * row + e]) + (int)A[(size_t)(y + r) * row + e]);
      prev = cur;
    }
    C[(size_t)y * row + e] = (uint16_t)(int16_t)cur;
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, kWave));
  return v;
}

// One wave per line.  grid (lines, 2 images), 64 threads, LDS 2 * (D + 2) int16.  column = 0: line = row y, n = W steps along x;
// column = 1: line = column x, n = H steps along y.  first = 1 writes S, else S = S +s L.
__global__ __launch_bounds__(kWave) void k_sgm_path(const uint16_t* __restrict__ C, int16_t* __restrict__ S0, int16_t* __restrict__ S1,
                                                    int H, int W, int D, int p1, int p2, int column, int reverse, int first) {
  extern __shared__ int16_t lds[];
  const int lane = threadIdx.x;
  const int line = blockIdx.x;
  const bool right = blockIdx.y == 1;
  int16_t* __restrict__ S = right ? S1 : S0;
  const int n = column ? H : W;
  int16_t* prev = lds + 1;             // prev[-1] and prev[D] are the sentinels
  int16_t* cur = lds + (D + 2) + 1;
  for (int d = lane; d < D; d += kWave) {
    prev[d] = 0;
    cur[d] = 0;
  }
  if (lane == 0) {
    prev[-1] = SHRT_MAX;
    prev[D] = SHRT_MAX;
    cur[-1] = SHRT_MAX;
    cur[D] = SHRT_MAX;
  }
  __syncthreads();
  int prev_min = 0;
  for (int i = 0; i < n; ++i) {
    const int pos = reverse ? n - 1 - i : i;
    const int y = column ? pos : line;
    const int x = column ? line : pos;
    const size_t pix = (size_t)y * W + x;
    const int pm = (int16_t)(prev_min + p2);   // formed in int, truncated (not saturated), as the reference's cast does
    int lmin = SHRT_MAX;
    for (int d = lane; d < D; d += kWave) {
      int cost;
      if (right) {
        const int dd = min(d, W - 1 - x);
        cost = (int16_t)C[(pix + dd) * D + dd];
      } else {
        cost = (int16_t)C[pix * D + d];
      }
      int c = min((int)prev[d], sat16(prev[d - 1] + p1));
      c = min(c, sat16(prev[d + 1] + p1));
      c = min(c, pm);
      const int L = sat16(sat16(c - pm) + cost);
      cur[d] = (int16_t)L;
      lmin = min(lmin, L);
      const size_t o = pix * D + d;
      S[o] = first ? (int16_t)L : (int16_t)sat16(S[o] + L);
    }
    prev_min = wave_min(lmin);
    int16_t* t = prev;
    prev = cur;
    cur = t;
    __syncthreads();
  }
}

// The fp64 steps of the reference, with plain operators and contraction off: IEEE divisions, every product and sum rounded on
// its own, as the host computes them.

// (int)(bd * F + (r - l) / (c - l or c - r) / 2 * F + 0.5).  c is the FIRST minimum, so l > c, and in the second branch
// r >= l > c: neither denominator is zero.
__device__ __forceinline__ int subpixel(int bd, int c, int l, int r, double factor) {
#pragma clang fp contract(off)
  const double den = r < l ? (double)(c - l) : (double)(c - r);
  const double q = (double)(r - l) / den / 2.0 * factor;
  const double base = (double)bd * factor;
  const double sum = base + q;
  return (int)(sum + 0.5);
}

__device__ __forceinline__ int scaled(int bd, double factor) {
#pragma clang fp contract(off)
  return (int)((double)bd * factor);
}

// (int)(v / F + 0.5)
__device__ __forceinline__ int rounded_disparity(int v, double factor) {
#pragma clang fp contract(off)
  const double q = (double)v / factor;
  return (int)(q + 0.5);
}

// grid (ceil(H * W / 256), 2 images): first minimum over d and the sub-pixel step
__global__ __launch_bounds__(256) void k_sgm_wta(const int16_t* __restrict__ S0, const int16_t* __restrict__ S1, uint16_t* __restrict__ raw,
                                                 int npix, int D, double factor) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const int16_t* __restrict__ s = (blockIdx.y ? S1 : S0) + (size_t)p * D;
  int best = s[0], bd = 0;
  for (int d = 1; d < D; ++d) {
    const int v = s[d];
    if (v < best) {
      best = v;
      bd = d;
    }
  }
  int out;
  if (bd > 0 && bd < D - 1)
    out = subpixel(bd, best, s[bd - 1], s[bd + 1], factor);
  else
    out = scaled(bd, factor);
  raw[(size_t)blockIdx.y * npix + p] = (uint16_t)out;
}

// --- speckle filter: union-find over the edge rule (both non-zero, |a - b| <= max_diff, 4-connected) ---

__device__ __forceinline__ int uf_find(int* parent, int i) {
  int p = __atomic_load_n(parent + i, __ATOMIC_RELAXED);
  while (p != i) {
    i = p;
    p = __atomic_load_n(parent + i, __ATOMIC_RELAXED);
  }
  return i;
}

// links the larger root under the smaller; a root only ever gets a smaller parent, so the final root is the component's minimum
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  bool done = false;
  while (!done) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) {
      done = true;
    } else {
      if (a > b) {
        const int t = a;
        a = b;
        b = t;
      }
      const int old = atomicMin(parent + b, a);
      done = old == b;
      b = old;
    }
  }
}

__global__ __launch_bounds__(256) void k_ccl_init(int* __restrict__ parent, int* __restrict__ size, int npix) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  parent[(size_t)blockIdx.y * npix + p] = p;
  size[(size_t)blockIdx.y * npix + p] = 0;
}

__global__ __launch_bounds__(256) void k_ccl_merge(const uint16_t* __restrict__ raw, int* __restrict__ parent, int H, int W, int max_diff) {
  const int npix = H * W;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const uint16_t* img = raw + (size_t)blockIdx.y * npix;
  int* par = parent + (size_t)blockIdx.y * npix;
  const int v = img[p];
  if (v == 0) return;
  const int y = p / W, x = p - y * W;
  if (x + 1 < W) {
    const int u = img[p + 1];
    if (u != 0 && abs(v - u) <= max_diff) uf_union(par, p, p + 1);
  }
  if (y + 1 < H) {
    const int u = img[p + W];
    if (u != 0 && abs(v - u) <= max_diff) uf_union(par, p, p + W);
  }
}

__global__ __launch_bounds__(256) void k_ccl_count(const uint16_t* __restrict__ raw, int* __restrict__ parent, int* __restrict__ root,
                                                   int* __restrict__ size, int npix) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const size_t base = (size_t)blockIdx.y * npix;
  if (raw[base + p] == 0) {
    root[base + p] = p;
    return;
  }
  const int r = uf_find(parent + base, p);
  root[base + p] = r;
  atomicAdd(size + base + r, 1);
}

__global__ __launch_bounds__(256) void k_ccl_apply(const uint16_t* __restrict__ raw, const int* __restrict__ root,
                                                   const int* __restrict__ size, uint16_t* __restrict__ filtered, int npix) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const size_t base = (size_t)blockIdx.y * npix;
  const uint16_t v = raw[base + p];
  filtered[base + p] = (v != 0 && size[base + root[base + p]] <= kSpeckleSize) ? (uint16_t)0 : v;
}

// left-right check of the left map (filtered holds left, right), float disparity, depth; each output nullable
__global__ __launch_bounds__(256) void k_sgm_lr_depth(const uint16_t* __restrict__ filtered, int H, int W, double factor, int threshold,
                                                      float bf, uint16_t* __restrict__ disp_scaled, float* __restrict__ disparity,
                                                      float* __restrict__ depth) {
  const int npix = H * W;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const int y = p / W, x = p - y * W;
  int v = filtered[p];
  if (v != 0) {
    const int lv = rounded_disparity(v, factor);
    if (x - lv < 0) {
      v = 0;
    } else {
      const int rv = rounded_disparity(filtered[(size_t)npix + p - lv], factor);
      if (rv == 0 || abs(lv - rv) > threshold) v = 0;
    }
  }
  const float d = (float)((double)v / factor);
  if (disp_scaled) disp_scaled[p] = (uint16_t)v;
  if (disparity) disparity[p] = d;
  if (depth) depth[p] = d > 0.01f ? __fmul_rn(bf, __fdiv_rn(1.0f, d)) : -0.1f;
}

}  // namespace

struct pba_sgm : pba::Handle {      // (device, stream, err, mem, events)
  int rows = 0, cols = 0;
  pba_sgm_params p{};
  int cap = 15;
  HammingTable ht{};
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // upload start, kernels start, kernels end, copy-back end
  uint8_t* d_img = nullptr;       // left, right
  uint8_t* d_sobel = nullptr;     // left, right
  int32_t* d_census = nullptr;    // left, right
  uint16_t* d_agg = nullptr;      // A; after k_sgm_cost its storage holds the right solve's S
  uint16_t* d_cost = nullptr;     // C_L
  int16_t* d_sum = nullptr;       // S of the left solve
  uint16_t* d_raw = nullptr;      // left, right maps before the speckle filter
  uint16_t* d_filtered = nullptr; // left, right maps after it
  int* d_parent = nullptr;        // union-find links, roots, sizes: left, right
  int* d_root = nullptr;
  int* d_size = nullptr;
  uint16_t* d_disp = nullptr;     // outputs
  float* d_disparity = nullptr;
  float* d_depth = nullptr;
  uint8_t* h_img = nullptr;       // pinned staging of the pair
  uint16_t* h_disp = nullptr;     // pinned copy-back buffers
  float* h_disparity = nullptr;
  float* h_depth = nullptr;
  bool computed = false;
};

namespace {

using pba::MemKind;      // (fail and create_bail are found through the handle argument)
constexpr auto create_fail = pba::create_fail<pba_sgm>;

int effective_cap(int v) { return std::min(std::max(v, 15), 127) | 1; }

// the setters of the reference's SGMStereo plus the sizes its buffers silently assume
int validate(int32_t rows, int32_t cols, const pba_sgm_params* p) {
  const bool sized = !(rows == 0 && cols == 0);
  if (sized && (rows <= 0 || cols <= 0 || (int64_t)rows * cols >= (1ll << 30)))
    return create_fail(PBA_ERR_INVALID, "image size %d x %d out of range", rows, cols);
  if (p->number_of_disparities <= 0 || p->number_of_disparities % 16 != 0)
    return create_fail(PBA_ERR_INVALID, "numberOfDisparities %d must be a positive multiple of 16", p->number_of_disparities);
  if (sized && p->number_of_disparities > cols)
    return create_fail(PBA_ERR_INVALID, "numberOfDisparities %d must be <= cols = %d", p->number_of_disparities, cols);
  if (p->number_of_disparities > kMaxLdsDisparities)
    return create_fail(PBA_ERR_INVALID, "numberOfDisparities %d exceeds what the path kernel's LDS holds (%d)", p->number_of_disparities,
                       kMaxLdsDisparities);
  if (sized && (int64_t)rows * cols * p->number_of_disparities >= (1ll << 31))
    return create_fail(PBA_ERR_INVALID, "numberOfDisparities %d: the %d x %d x D cost volume exceeds 2^31 elements",
                       p->number_of_disparities, rows, cols);
  if (p->census_radius < 1 || p->census_radius > 2)
    return create_fail(PBA_ERR_INVALID, "censusRadius %d must be 1 or 2", p->census_radius);
  if (p->window_radius < 0 || p->window_radius > 9)
    return create_fail(PBA_ERR_INVALID, "windowRadius %d must be within 0..9", p->window_radius);
  if (sized && rows < p->window_radius + 1)
    return create_fail(PBA_ERR_INVALID, "windowRadius %d needs rows >= windowRadius + 1, image has %d", p->window_radius, rows);
  if (p->smoothness_penalty_small < 0)
    return create_fail(PBA_ERR_INVALID, "smoothnessPenaltySmall %d must be >= 0", p->smoothness_penalty_small);
  if (p->smoothness_penalty_large > 32767 || p->smoothness_penalty_large <= p->smoothness_penalty_small)
    return create_fail(PBA_ERR_INVALID, "smoothnessPenaltyLarge %d must be within smoothnessPenaltySmall + 1 = %d .. 32767",
                       p->smoothness_penalty_large, p->smoothness_penalty_small + 1);
  if (p->consistency_threshold < 0)
    return create_fail(PBA_ERR_INVALID, "consistencyThreshold %d must be >= 0", p->consistency_threshold);
  if (!(p->disparity_factor >= 1.0) || p->disparity_factor != std::floor(p->disparity_factor) ||
      p->disparity_factor * p->number_of_disparities > 65536.0)
    return create_fail(PBA_ERR_INVALID, "disparityFactor %g must be an integer >= 1 with numberOfDisparities * disparityFactor <= 65536",
                       p->disparity_factor);
  if (!(p->census_weight_factor >= 0.0) || !(p->census_weight_factor * 25.0 < 2147483648.0))
    return create_fail(PBA_ERR_INVALID, "censusWeightFactor %g must be >= 0 (and finite)", p->census_weight_factor);
  if (p->reserved != 0) return create_fail(PBA_ERR_INVALID, "reserved must be 0");
  return PBA_OK;
}

inline dim3 grid1(size_t n, unsigned y = 1, unsigned z = 1) { return dim3((unsigned)((n + 255) / 256), y, z); }

}  // namespace

extern "C" {

void pba_sgm_default_params(pba_sgm_params* p) {
  if (!p) return;
  p->number_of_disparities = 128;   // reference src/stereo_algorithm.cc:393-402
  p->sobel_cap_value = 15;
  p->census_radius = 2;
  p->window_radius = 2;
  p->smoothness_penalty_small = 100;
  p->smoothness_penalty_large = 1600;
  p->consistency_threshold = 1;
  p->reserved = 0;
  p->disparity_factor = 256.0;
  p->census_weight_factor = 1.0 / 6.0;
}

int pba_sgm_validate_params(int32_t rows, int32_t cols, const pba_sgm_params* p) {
  if (!p) return create_fail(PBA_ERR_INVALID, "params is NULL");
  return validate(rows, cols, p);
}

const char* pba_sgm_last_error(const pba_sgm* s) { return s ? s->err.c_str() : pba::create_error<pba_sgm>().c_str(); }

void pba_sgm_destroy(pba_sgm* s) { pba::handle_destroy(s); }

int pba_sgm_create(int32_t rows, int32_t cols, const pba_sgm_params* p, int32_t device, pba_sgm** out) {
  if (!out) return create_fail(PBA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!p) return create_fail(PBA_ERR_INVALID, "params is NULL");
  if (rows == 0 && cols == 0) return create_fail(PBA_ERR_INVALID, "image size 0 x 0");
  int rc = validate(rows, cols, p);
  if (rc) return rc;
  if (!pba::device_exists(device))
    return create_fail(PBA_ERR_NO_DEVICE, "no HIP device %d (the semi-global matcher has no CPU fallback)", device);
  pba_sgm* s = new pba_sgm();
  s->rows = rows;
  s->cols = cols;
  s->p = *p;
  s->cap = effective_cap(p->sobel_cap_value);
  for (int h = 0; h < 26; ++h) s->ht.v[h] = (uint8_t)(int)(h * p->census_weight_factor);
  const size_t npix = (size_t)rows * cols, nvol = npix * p->number_of_disparities;
  if ((rc = pba::handle_open(s, device))) return create_bail(s, rc, pba_sgm_destroy);
  for (hipEvent_t& e : s->ev)
    if ((rc = pba::handle_event(s, &e))) return create_bail(s, rc, pba_sgm_destroy);
  const MemKind dev = MemKind::device, pin = MemKind::pinned;
  if (s->mem.reserve(&s->d_img, dev, 2 * npix) || s->mem.reserve(&s->d_sobel, dev, 2 * npix) || s->mem.reserve(&s->d_census, dev, 2 * npix) ||
      s->mem.reserve(&s->d_agg, dev, nvol) || s->mem.reserve(&s->d_cost, dev, nvol) || s->mem.reserve(&s->d_sum, dev, nvol) ||
      s->mem.reserve(&s->d_raw, dev, 2 * npix) || s->mem.reserve(&s->d_filtered, dev, 2 * npix) || s->mem.reserve(&s->d_parent, dev, 2 * npix) ||
      s->mem.reserve(&s->d_root, dev, 2 * npix) || s->mem.reserve(&s->d_size, dev, 2 * npix) || s->mem.reserve(&s->d_disp, dev, npix) ||
      s->mem.reserve(&s->d_disparity, dev, npix) || s->mem.reserve(&s->d_depth, dev, npix))
    return create_bail(s, fail(s, PBA_ERR_HIP, "device allocation for %zu pixels x %d disparities failed", npix, p->number_of_disparities),
                       pba_sgm_destroy);
  if (s->mem.reserve(&s->h_img, pin, 2 * npix) || s->mem.reserve(&s->h_disp, pin, npix) || s->mem.reserve(&s->h_disparity, pin, npix) ||
      s->mem.reserve(&s->h_depth, pin, npix))
    return create_bail(s, fail(s, PBA_ERR_HIP, "pinned host allocation of %zu pixels failed", npix), pba_sgm_destroy);
  *out = s;
  return PBA_OK;
}

int pba_sgm_compute(pba_sgm* s, const uint8_t* left, const uint8_t* right, float bf, uint16_t* disp_scaled, float* disparity,
                    float* depth) {
  if (!s) return PBA_ERR_INVALID;
  if (!left || !right) return fail(s, PBA_ERR_INVALID, "pba_sgm_compute: left and right must not be NULL");
  PBA_HIP_TRY(s, hipSetDevice(s->device));
  const int H = s->rows, W = s->cols, D = s->p.number_of_disparities, r = s->p.window_radius;
  const size_t npix = (size_t)H * W;
  const size_t row = (size_t)W * D;
  hipStream_t st = s->stream;
  std::memcpy(s->h_img, left, npix);
  std::memcpy(s->h_img + npix, right, npix);
  PBA_HIP_TRY(s, hipEventRecord(s->ev[0], st));
  PBA_HIP_TRY(s, hipMemcpyAsync(s->d_img, s->h_img, 2 * npix, hipMemcpyHostToDevice, st));
  PBA_HIP_TRY(s, hipEventRecord(s->ev[1], st));
  hipLaunchKernelGGL(k_sgm_prefilter, dim3((W + 255) / 256, H, 2), dim3(256), 0, st, s->d_img, s->d_sobel, s->d_census, H, W, s->cap,
                     s->p.census_radius);
  hipLaunchKernelGGL(k_sgm_rowagg, grid1(row, H), dim3(256), 0, st, s->d_sobel, s->d_census, s->d_agg, H, W, D, r, s->ht);
  hipLaunchKernelGGL(k_sgm_cost, grid1(row), dim3(256), 0, st, s->d_agg, s->d_cost, H, W, D, r);
  PBA_HIP_TRY(s, hipGetLastError());
  int16_t* s_right = reinterpret_cast<int16_t*>(s->d_agg);
  const size_t lds = 2 * (size_t)(D + 2) * sizeof(int16_t);
  for (int pass = 0; pass < 2; ++pass)
    for (int column = 0; column < 2; ++column)
      hipLaunchKernelGGL(k_sgm_path, dim3(column ? W : H, 2), dim3(kWave), lds, st, s->d_cost, s->d_sum, s_right, H, W, D,
                         s->p.smoothness_penalty_small, s->p.smoothness_penalty_large, column, pass, (pass == 0 && column == 0) ? 1 : 0);
  PBA_HIP_TRY(s, hipGetLastError());
  hipLaunchKernelGGL(k_sgm_wta, grid1(npix, 2), dim3(256), 0, st, s->d_sum, s_right, s->d_raw, (int)npix, D, s->p.disparity_factor);
  hipLaunchKernelGGL(k_ccl_init, grid1(npix, 2), dim3(256), 0, st, s->d_parent, s->d_size, (int)npix);
  hipLaunchKernelGGL(k_ccl_merge, grid1(npix, 2), dim3(256), 0, st, s->d_raw, s->d_parent, H, W, (int)(2 * s->p.disparity_factor));
  hipLaunchKernelGGL(k_ccl_count, grid1(npix, 2), dim3(256), 0, st, s->d_raw, s->d_parent, s->d_root, s->d_size, (int)npix);
  hipLaunchKernelGGL(k_ccl_apply, grid1(npix, 2), dim3(256), 0, st, s->d_raw, s->d_root, s->d_size, s->d_filtered, (int)npix);
  hipLaunchKernelGGL(k_sgm_lr_depth, grid1(npix), dim3(256), 0, st, s->d_filtered, H, W, s->p.disparity_factor,
                     s->p.consistency_threshold, bf, disp_scaled ? s->d_disp : nullptr, disparity ? s->d_disparity : nullptr,
                     depth ? s->d_depth : nullptr);
  PBA_HIP_TRY(s, hipGetLastError());
  PBA_HIP_TRY(s, hipEventRecord(s->ev[2], st));
  if (disp_scaled) PBA_HIP_TRY(s, hipMemcpyAsync(s->h_disp, s->d_disp, npix * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  if (disparity) PBA_HIP_TRY(s, hipMemcpyAsync(s->h_disparity, s->d_disparity, npix * sizeof(float), hipMemcpyDeviceToHost, st));
  if (depth) PBA_HIP_TRY(s, hipMemcpyAsync(s->h_depth, s->d_depth, npix * sizeof(float), hipMemcpyDeviceToHost, st));
  PBA_HIP_TRY(s, hipEventRecord(s->ev[3], st));
  PBA_HIP_TRY(s, hipStreamSynchronize(st));
  if (disp_scaled) std::memcpy(disp_scaled, s->h_disp, npix * sizeof(uint16_t));
  if (disparity) std::memcpy(disparity, s->h_disparity, npix * sizeof(float));
  if (depth) std::memcpy(depth, s->h_depth, npix * sizeof(float));
  s->computed = true;
  return PBA_OK;
}

int pba_sgm_get_timing(pba_sgm* s, float* kernels_ms, float* total_ms) {
  if (!s) return PBA_ERR_INVALID;
  if (!s->computed) return fail(s, PBA_ERR_STATE, "pba_sgm_get_timing before pba_sgm_compute");
  if (kernels_ms) PBA_HIP_TRY(s, hipEventElapsedTime(kernels_ms, s->ev[1], s->ev[2]));
  if (total_ms) PBA_HIP_TRY(s, hipEventElapsedTime(total_ms, s->ev[0], s->ev[3]));
  return PBA_OK;
}

int pba_sgm_get_stage(pba_sgm* s, int32_t stage, void* buf) {
  if (!s) return PBA_ERR_INVALID;
  if (!buf) return fail(s, PBA_ERR_INVALID, "pba_sgm_get_stage: NULL output");
  if (!s->computed) return fail(s, PBA_ERR_STATE, "pba_sgm_get_stage before pba_sgm_compute");
  const size_t npix = (size_t)s->rows * s->cols, nvol = npix * s->p.number_of_disparities;
  const void* src = nullptr;
  size_t bytes = 0;
  switch (stage) {
    case PBA_SGM_STAGE_SOBEL_LEFT: src = s->d_sobel; bytes = npix; break;
    case PBA_SGM_STAGE_SOBEL_RIGHT: src = s->d_sobel + npix; bytes = npix; break;
    case PBA_SGM_STAGE_CENSUS_LEFT: src = s->d_census; bytes = npix * sizeof(int32_t); break;
    case PBA_SGM_STAGE_CENSUS_RIGHT: src = s->d_census + npix; bytes = npix * sizeof(int32_t); break;
    case PBA_SGM_STAGE_COST_LEFT: src = s->d_cost; bytes = nvol * sizeof(uint16_t); break;
    case PBA_SGM_STAGE_SUM_LEFT: src = s->d_sum; bytes = nvol * sizeof(int16_t); break;
    case PBA_SGM_STAGE_DISP_LEFT_RAW: src = s->d_raw; bytes = npix * sizeof(uint16_t); break;
    case PBA_SGM_STAGE_DISP_RIGHT_RAW: src = s->d_raw + npix; bytes = npix * sizeof(uint16_t); break;
    case PBA_SGM_STAGE_DISP_LEFT_FILTERED: src = s->d_filtered; bytes = npix * sizeof(uint16_t); break;
    case PBA_SGM_STAGE_DISP_RIGHT_FILTERED: src = s->d_filtered + npix; bytes = npix * sizeof(uint16_t); break;
    default: return fail(s, PBA_ERR_INVALID, "pba_sgm_get_stage: unknown stage %d", stage);
  }
  PBA_HIP_TRY(s, hipSetDevice(s->device));
  PBA_HIP_TRY(s, hipMemcpy(buf, src, bytes, hipMemcpyDeviceToHost));
  return PBA_OK;
}

}  // extern "C"
