// pba_stereo.hip -- stereo block matching (OpenCV 2.4 StereoBM as restated in DESIGN.md "Stereo block matching") on gfx950,
// behind the C-ABI of include/pba_stereo.h.  Two kernels per pair:
//
//   k_stereo_prefilter  one thread per pixel of both images: XSOBEL prefilter into u8; the same pass writes the FILTERED
//                       disparity (and its depth) of every pixel outside the valid region, which the matcher never visits.
//   k_stereo_bm         one 256-thread workgroup per 64 x 8 tile of the valid region.  The prefiltered left rows and the right
//                       rows plus (ndisp - 1) extra columns, window halo included, are staged in LDS once (when they fit in
//                       64 KiB; otherwise both are read from global memory through L1/L2, same arithmetic).  The disparity loop
//                       is the outer loop: per disparity the workgroup forms the horizontal window sums of all tile rows + halo
//                       (u16, exact: w * 2 cap <= 32130) in LDS, sliding along 4-column runs, then every lane sums its column
//                       vertically for 2 output rows (sliding) and folds the cost into its pixels' running winner state.  The
//                       state is O(1) per pixel: best cost and disparity, the costs next to it and the minimum cost away from it
//                       (prefix minimum up to the winner - 2, running minimum after the winner + 1), which is all that the
//                       uniqueness test and the sub-pixel fit need, so the 128-cost vector is never stored.
//
// There is no CPU fallback: pba_stereo_create fails with PBA_ERR_NO_DEVICE when no GPU is visible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "../../include/pba_stereo.h"
#include "pba_handle.h"

namespace {

constexpr int kTX = 64;                          // tile columns: one lane each in the vertical pass
constexpr int kTY = 8;                           // tile rows
constexpr int kThreads = 256;
constexpr int kRowsPerThread = kTY / (kThreads / kTX);   // 2
constexpr int kRun = 4;                          // columns per sliding run of the horizontal pass
constexpr int kRunsPerRow = kTX / kRun;
constexpr size_t kLdsBudget = 64 * 1024;

struct Roi {
  int x0, x1, y0, y1;   // valid region [x0, x1) x [y0, y1); empty when x0 >= x1 or y0 >= y1
};

// d > 0.01 ? Bf * (1 / d) : -0.1, two correctly rounded fp32 operations (no v_rcp_f32, no contraction)
__device__ __forceinline__ float disp_to_depth(int v, float bf) {
  const float d = (float)v * 0.0625f;
  return d > 0.01f ? __fmul_rn(bf, __fdiv_rn(1.0f, d)) : -0.1f;
}

// blockIdx.z = image (0 left, 1 right); img/pf hold the two images back to back
__global__ __launch_bounds__(256) void k_stereo_prefilter(const uint8_t* __restrict__ img, uint8_t* __restrict__ pf, int H, int W,
                                                          int cap, int16_t* __restrict__ disp, float* __restrict__ depth, Roi roi,
                                                          int filtered, float bf) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  const int k = blockIdx.z;
  if (x >= W) return;
  const size_t npix = (size_t)H * W;
  const uint8_t* I = img + k * npix;
  int P = cap;
  // columns 0 and W-1, and the last row of an odd-height image (OpenCV filters rows in pairs), stay at cap
  if (x > 0 && x < W - 1 && !((H & 1) && y == H - 1)) {
    const int ym = y == 0 ? 1 : y - 1;            // reflect-101
    const int yp = y == H - 1 ? H - 2 : y + 1;
    const uint8_t* a = I + (size_t)ym * W;
    const uint8_t* b = I + (size_t)y * W;
    const uint8_t* c = I + (size_t)yp * W;
    const int v = (a[x + 1] - a[x - 1]) + 2 * (b[x + 1] - b[x - 1]) + (c[x + 1] - c[x - 1]);
    P = min(max(v, -cap), cap) + cap;
  }
  pf[k * npix + (size_t)y * W + x] = (uint8_t)P;
  if (k == 0 && !(x >= roi.x0 && x < roi.x1 && y >= roi.y0 && y < roi.y1)) {
    disp[(size_t)y * W + x] = (int16_t)filtered;
    if (depth) depth[(size_t)y * W + x] = disp_to_depth(filtered, bf);
  }
}

// Horizontal window sums of the tile rows [0, nhrow) and columns [0, ncol) into hbuf (row stride kTX).  kTexture: |L - cap|
// (the texture sum), else |L(x) - R(x - D)| with the right column offset by d = maxD - D inside the staged right rows.
template <bool kStaged, bool kTexture>
__device__ __forceinline__ void hpass(uint16_t* hbuf, const uint8_t* lsrc, int lstride, const uint8_t* rsrc, int rstride, int w,
                                      int ncol, int nhrow, int d, int cap) {
  const int nrun = nhrow * kRunsPerRow;
  for (int q = threadIdx.x; q < nrun; q += kThreads) {
    const int row = q / kRunsPerRow;
    const int c0 = (q % kRunsPerRow) * kRun;
    if (c0 >= ncol) continue;
    const uint8_t* L = lsrc + (size_t)row * lstride;
    const uint8_t* R = rsrc + (size_t)row * rstride + d;
    int h = 0;
    for (int k = 0; k < w; ++k) h += abs((int)L[c0 + k] - (kTexture ? cap : (int)R[c0 + k]));
    hbuf[row * kTX + c0] = (uint16_t)h;
    const int ce = min(c0 + kRun, ncol);
    for (int c = c0 + 1; c < ce; ++c) {
      h += abs((int)L[c + w - 1] - (kTexture ? cap : (int)R[c + w - 1])) - abs((int)L[c - 1] - (kTexture ? cap : (int)R[c - 1]));
      hbuf[row * kTX + c] = (uint16_t)h;
    }
  }
}

// Vertical window sums of lane column c for the thread's kRowsPerThread output rows starting at q0 (sliding).
__device__ __forceinline__ void vpass(const uint16_t* hbuf, int c, int q0, int w, int* out) {
  int s = 0;
  for (int j = 0; j < w; ++j) s += hbuf[(q0 + j) * kTX + c];
  out[0] = s;
#pragma unroll
  for (int i = 1; i < kRowsPerThread; ++i) {
    s += (int)hbuf[(q0 + i - 1 + w) * kTX + c] - (int)hbuf[(q0 + i - 1) * kTX + c];
    out[i] = s;
  }
}

template <bool kStaged>
__global__ __launch_bounds__(256) void k_stereo_bm(const uint8_t* __restrict__ pf, int H, int W, int r, int cap, int min_d, int ndisp,
                                                   int tex_thresh, int uniq, Roi roi, int16_t* __restrict__ disp,
                                                   float* __restrict__ depth, float bf) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int w = 2 * r + 1;
  const int max_d = min_d + ndisp - 1;
  const int x0 = roi.x0 + blockIdx.x * kTX;
  const int y0 = roi.y0 + blockIdx.y * kTY;
  const int ncol = min(x0 + kTX, roi.x1) - x0;   // >= 1
  const int nrow = min(y0 + kTY, roi.y1) - y0;   // >= 1
  const int nhrow = nrow + 2 * r;
  const int hrows = kTY + 2 * r;
  uint16_t* hbuf = reinterpret_cast<uint16_t*>(smem);
  const uint8_t* PL = pf;
  const uint8_t* PR = pf + (size_t)H * W;
  // tile origin (row 0 / column 0 of the staged blocks) in image coordinates: left (y0 - r, x0 - r), right (y0 - r, x0 - r - maxD).
  // Inside the valid region every window read of a computed pixel lies in the image (DESIGN.md "Stereo block matching").
  const uint8_t* lsrc;
  const uint8_t* rsrc;
  int lstride, rstride;
  if (kStaged) {
    const int lw = kTX + 2 * r, rw = lw + ndisp - 1;
    uint8_t* lt = smem + (size_t)hrows * kTX * sizeof(uint16_t);
    uint8_t* rt = lt + (size_t)hrows * lw;
    for (int i = threadIdx.x; i < hrows * lw; i += kThreads) {
      const int y = y0 - r + i / lw, x = x0 - r + i % lw;
      lt[i] = (y >= 0 && y < H && x >= 0 && x < W) ? PL[(size_t)y * W + x] : 0;
    }
    for (int i = threadIdx.x; i < hrows * rw; i += kThreads) {
      const int y = y0 - r + i / rw, x = x0 - r - max_d + i % rw;
      rt[i] = (y >= 0 && y < H && x >= 0 && x < W) ? PR[(size_t)y * W + x] : 0;
    }
    lsrc = lt; lstride = lw;
    rsrc = rt; rstride = rw;
    __syncthreads();
  } else {
    lsrc = PL + (size_t)(y0 - r) * W + (x0 - r);
    rsrc = PR + (size_t)(y0 - r) * W + (x0 - r - max_d);
    lstride = rstride = W;
  }

  const int c = threadIdx.x % kTX;
  const int q0 = (threadIdx.x / kTX) * kRowsPerThread;
  const bool active = c < ncol && q0 < nrow;

  int tsum[kRowsPerThread];
  hpass<kStaged, true>(hbuf, lsrc, lstride, rsrc, rstride, w, ncol, nhrow, 0, cap);
  __syncthreads();
  if (active) vpass(hbuf, c, q0, w, tsum);
  __syncthreads();

  int cmin[kRowsPerThread], dbest[kRowsPerThread], clo[kRowsPerThread], chi[kRowsPerThread];
  int farlo[kRowsPerThread], farhi[kRowsPerThread], pm1[kRowsPerThread], pm2[kRowsPerThread], prev[kRowsPerThread];
#pragma unroll
  for (int i = 0; i < kRowsPerThread; ++i) {
    cmin[i] = INT_MAX; dbest[i] = min_d; clo[i] = chi[i] = INT_MAX;
    farlo[i] = farhi[i] = pm1[i] = pm2[i] = prev[i] = INT_MAX;
  }
  // ascending D with <=: a tie goes to the larger disparity (OpenCV scans d = maxD - D with a strict <)
  for (int D = min_d; D <= max_d; ++D) {
    hpass<kStaged, false>(hbuf, lsrc, lstride, rsrc, rstride, w, ncol, nhrow, max_d - D, cap);
    __syncthreads();
    if (active) {
      int cost[kRowsPerThread];
      vpass(hbuf, c, q0, w, cost);
#pragma unroll
      for (int i = 0; i < kRowsPerThread; ++i) {
        const int v = cost[i];
        if (v <= cmin[i]) {
          cmin[i] = v; dbest[i] = D; clo[i] = prev[i]; chi[i] = INT_MAX; farlo[i] = pm2[i]; farhi[i] = INT_MAX;
        } else if (D == dbest[i] + 1) {
          chi[i] = v;
        } else {
          farhi[i] = min(farhi[i], v);
        }
        pm2[i] = pm1[i];
        pm1[i] = min(pm1[i], v);
        prev[i] = v;
      }
    }
    __syncthreads();
  }
  if (!active) return;
  const int filtered = (min_d - 1) * 16;
#pragma unroll
  for (int i = 0; i < kRowsPerThread; ++i) {
    const int q = q0 + i;
    if (q >= nrow) break;
    int lo = clo[i], hi = chi[i];
    if (dbest[i] == max_d) hi = lo;
    if (dbest[i] == min_d) lo = hi;
    int out;
    if (tsum[i] < tex_thresh) {
      out = filtered;
    } else if (uniq > 0 && (long long)min(farlo[i], farhi[i]) <= (long long)cmin[i] + (long long)cmin[i] * uniq / 100) {
      out = filtered;
    } else {
      const int den = lo + hi - 2 * cmin[i] + abs(lo - hi);
      const int frac = den ? (lo - hi) * 256 / den : 0;
      out = (dbest[i] * 256 + frac + 15) >> 4;
    }
    const size_t o = (size_t)(y0 + q) * W + (x0 + c);
    disp[o] = (int16_t)out;
    if (depth) depth[o] = disp_to_depth(out, bf);
  }
}

}  // namespace

struct pba_stereo : pba::Handle {      // (device, stream, err, mem, events)
  int rows = 0, cols = 0;
  pba_stereo_bm_params p{};
  Roi roi{};
  bool staged = false;
  size_t lds = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // upload start, kernels start, kernels end, copy-back end
  uint8_t* d_img = nullptr;      // left, right
  uint8_t* d_pf = nullptr;       // prefiltered left, right
  int16_t* d_disp = nullptr;
  float* d_depth = nullptr;
  uint8_t* h_img = nullptr;      // pinned staging of the pair
  int16_t* h_disp = nullptr;     // pinned copy-back buffers
  float* h_depth = nullptr;
  bool computed = false;
};

namespace {

using pba::MemKind;      // (fail and create_bail are found through the handle argument)
constexpr auto create_fail = pba::create_fail<pba_stereo>;

// the checks of OpenCV 2.4 cvFindStereoCorrespondenceBM that apply, plus the options this matcher does not build
int validate(int32_t rows, int32_t cols, const pba_stereo_bm_params* p) {
  const bool sized = !(rows == 0 && cols == 0);
  if (sized && (rows <= 0 || cols <= 0 || (int64_t)rows * cols >= (1ll << 30)))
    return create_fail(PBA_ERR_INVALID, "image size %d x %d out of range", rows, cols);
  if (p->pre_filter_type != PBA_STEREO_PREFILTER_XSOBEL)
    return create_fail(PBA_ERR_INVALID, "preFilterType %d not supported: only XSOBEL (1) is built (NORMALIZED_RESPONSE is not)",
                       p->pre_filter_type);
  if (p->pre_filter_size < 5 || p->pre_filter_size > 255 || p->pre_filter_size % 2 == 0)
    return create_fail(PBA_ERR_INVALID, "preFilterSize %d must be odd and within 5..255", p->pre_filter_size);
  if (p->pre_filter_cap < 1 || p->pre_filter_cap > 63)
    return create_fail(PBA_ERR_INVALID, "preFilterCap %d must be within 1..63", p->pre_filter_cap);
  if (p->sad_window_size < 5 || p->sad_window_size > 255 || p->sad_window_size % 2 == 0 ||
      (sized && p->sad_window_size > std::min(rows, cols)))
    return create_fail(PBA_ERR_INVALID, "SADWindowSize %d must be odd, within 5..255 and <= min(rows, cols) = %d", p->sad_window_size,
                       std::min(rows, cols));
  if (p->number_of_disparities <= 0 || p->number_of_disparities % 16 != 0)
    return create_fail(PBA_ERR_INVALID, "numberOfDisparities %d must be a positive multiple of 16", p->number_of_disparities);
  if (p->min_disparity < -2047 || (int64_t)p->min_disparity + p->number_of_disparities - 1 > 2047)
    return create_fail(PBA_ERR_INVALID, "disparity range [%d, %lld] does not fit the int16 output (|D| <= 2047)", p->min_disparity,
                       (long long)p->min_disparity + p->number_of_disparities - 1);
  if (p->texture_threshold < 0) return create_fail(PBA_ERR_INVALID, "textureThreshold %d must be >= 0", p->texture_threshold);
  if (p->uniqueness_ratio < 0) return create_fail(PBA_ERR_INVALID, "uniquenessRatio %d must be >= 0", p->uniqueness_ratio);
  if (p->speckle_window_size != 0)
    return create_fail(PBA_ERR_INVALID, "speckleWindowSize %d not supported: speckle filtering is not built (0 only)",
                       p->speckle_window_size);
  if (p->try_smaller_windows != 0)
    return create_fail(PBA_ERR_INVALID, "trySmallerWindows %d not supported (0 only)", p->try_smaller_windows);
  if (p->disp12_max_diff >= 0)
    return create_fail(PBA_ERR_INVALID, "disp12MaxDiff %d not supported: the left-right check is not built (< 0 only)",
                       p->disp12_max_diff);
  return PBA_OK;
}

}  // namespace

extern "C" {

void pba_stereo_default_params(pba_stereo_bm_params* p) {
  if (!p) return;
  p->pre_filter_type = PBA_STEREO_PREFILTER_XSOBEL;   // reference src/stereo_algorithm.cc:251
  p->pre_filter_size = 9;
  p->pre_filter_cap = 31;
  p->sad_window_size = 15;
  p->min_disparity = 0;
  p->number_of_disparities = 0;                      // the reference requires the key (:258)
  p->texture_threshold = 10;
  p->uniqueness_ratio = 15;
  p->speckle_window_size = 0;
  p->speckle_range = 0;
  p->try_smaller_windows = 0;
  p->disp12_max_diff = -1;
}

int pba_stereo_validate_params(int32_t rows, int32_t cols, const pba_stereo_bm_params* p) {
  if (!p) return create_fail(PBA_ERR_INVALID, "params is NULL");
  return validate(rows, cols, p);
}

const char* pba_stereo_last_error(const pba_stereo* s) { return s ? s->err.c_str() : pba::create_error<pba_stereo>().c_str(); }

void pba_stereo_destroy(pba_stereo* s) { pba::handle_destroy(s); }

int pba_stereo_create(int32_t rows, int32_t cols, const pba_stereo_bm_params* p, int32_t device, pba_stereo** out) {
  if (!out) return create_fail(PBA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!p) return create_fail(PBA_ERR_INVALID, "params is NULL");
  if (rows == 0 && cols == 0) return create_fail(PBA_ERR_INVALID, "image size 0 x 0");
  int rc = validate(rows, cols, p);
  if (rc) return rc;
  if (!pba::device_exists(device))
    return create_fail(PBA_ERR_NO_DEVICE, "no HIP device %d (the stereo matcher has no CPU fallback)", device);
  pba_stereo* s = new pba_stereo();
  s->rows = rows;
  s->cols = cols;
  s->p = *p;
  const int r = p->sad_window_size / 2;
  const int min_d = p->min_disparity, max_d = min_d + p->number_of_disparities - 1;
  // valid region: the spec's [max(0, maxD) + r, min(W, W - minD) - r), further bounded by W + minD - r so that for minD < 0 no
  // window reads beyond the right image (DESIGN.md "Stereo block matching")
  s->roi.x0 = std::max(0, max_d) + r;
  s->roi.x1 = std::min(cols, std::min(cols - min_d, cols + min_d)) - r;
  s->roi.y0 = r;
  s->roi.y1 = rows - r;
  const size_t hbytes = (size_t)(kTY + 2 * r) * kTX * sizeof(uint16_t);
  const size_t staged = (size_t)(kTY + 2 * r) * (2 * (kTX + 2 * r) + p->number_of_disparities - 1);
  s->staged = hbytes + staged <= kLdsBudget;
  s->lds = s->staged ? hbytes + staged : hbytes;
  const size_t npix = (size_t)rows * cols;
  if ((rc = pba::handle_open(s, device))) return create_bail(s, rc, pba_stereo_destroy);
  for (hipEvent_t& e : s->ev)
    if ((rc = pba::handle_event(s, &e))) return create_bail(s, rc, pba_stereo_destroy);
  if (s->mem.reserve(&s->d_img, MemKind::device, 2 * npix) || s->mem.reserve(&s->d_pf, MemKind::device, 2 * npix) ||
      s->mem.reserve(&s->d_disp, MemKind::device, npix) || s->mem.reserve(&s->d_depth, MemKind::device, npix))
    return create_bail(s, fail(s, PBA_ERR_HIP, "device allocation of %zu pixels failed", npix), pba_stereo_destroy);
  if (s->mem.reserve(&s->h_img, MemKind::pinned, 2 * npix) || s->mem.reserve(&s->h_disp, MemKind::pinned, npix) ||
      s->mem.reserve(&s->h_depth, MemKind::pinned, npix))
    return create_bail(s, fail(s, PBA_ERR_HIP, "pinned host allocation of %zu pixels failed", npix), pba_stereo_destroy);
  *out = s;
  return PBA_OK;
}

int pba_stereo_compute(pba_stereo* s, const uint8_t* left, const uint8_t* right, float bf, int16_t* disp16, float* depth) {
  if (!s) return PBA_ERR_INVALID;
  if (!left || !right) return fail(s, PBA_ERR_INVALID, "pba_stereo_compute: left and right must not be NULL");
  PBA_HIP_TRY(s, hipSetDevice(s->device));
  const int H = s->rows, W = s->cols;
  const size_t npix = (size_t)H * W;
  const pba_stereo_bm_params& p = s->p;
  const int filtered = (p.min_disparity - 1) * 16;
  float* d_depth = depth ? s->d_depth : nullptr;
  // the caller's buffers are only borrowed: one pinned staging copy, then an async upload (pageable copy + sync is much slower)
  std::memcpy(s->h_img, left, npix);
  std::memcpy(s->h_img + npix, right, npix);
  PBA_HIP_TRY(s, hipEventRecord(s->ev[0], s->stream));
  PBA_HIP_TRY(s, hipMemcpyAsync(s->d_img, s->h_img, 2 * npix, hipMemcpyHostToDevice, s->stream));
  PBA_HIP_TRY(s, hipEventRecord(s->ev[1], s->stream));
  hipLaunchKernelGGL(k_stereo_prefilter, dim3((W + 255) / 256, H, 2), dim3(256), 0, s->stream, s->d_img, s->d_pf, H, W,
                     p.pre_filter_cap, s->d_disp, d_depth, s->roi, filtered, bf);
  PBA_HIP_TRY(s, hipGetLastError());
  if (s->roi.x0 < s->roi.x1 && s->roi.y0 < s->roi.y1) {
    const dim3 grid((s->roi.x1 - s->roi.x0 + kTX - 1) / kTX, (s->roi.y1 - s->roi.y0 + kTY - 1) / kTY);
    const int r = p.sad_window_size / 2;
    if (s->staged)
      hipLaunchKernelGGL(k_stereo_bm<true>, grid, dim3(kThreads), s->lds, s->stream, s->d_pf, H, W, r, p.pre_filter_cap, p.min_disparity,
                         p.number_of_disparities, p.texture_threshold, p.uniqueness_ratio, s->roi, s->d_disp, d_depth, bf);
    else
      hipLaunchKernelGGL(k_stereo_bm<false>, grid, dim3(kThreads), s->lds, s->stream, s->d_pf, H, W, r, p.pre_filter_cap, p.min_disparity,
                         p.number_of_disparities, p.texture_threshold, p.uniqueness_ratio, s->roi, s->d_disp, d_depth, bf);
    PBA_HIP_TRY(s, hipGetLastError());
  }
  PBA_HIP_TRY(s, hipEventRecord(s->ev[2], s->stream));
  if (disp16) PBA_HIP_TRY(s, hipMemcpyAsync(s->h_disp, s->d_disp, npix * sizeof(int16_t), hipMemcpyDeviceToHost, s->stream));
  if (depth) PBA_HIP_TRY(s, hipMemcpyAsync(s->h_depth, s->d_depth, npix * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  PBA_HIP_TRY(s, hipEventRecord(s->ev[3], s->stream));
  PBA_HIP_TRY(s, hipStreamSynchronize(s->stream));
  if (disp16) std::memcpy(disp16, s->h_disp, npix * sizeof(int16_t));
  if (depth) std::memcpy(depth, s->h_depth, npix * sizeof(float));
  s->computed = true;
  return PBA_OK;
}

int pba_stereo_get_prefiltered(pba_stereo* s, uint8_t* left, uint8_t* right) {
  if (!s) return PBA_ERR_INVALID;
  if (!left || !right) return fail(s, PBA_ERR_INVALID, "pba_stereo_get_prefiltered: NULL output");
  if (!s->computed) return fail(s, PBA_ERR_STATE, "pba_stereo_get_prefiltered before pba_stereo_compute");
  PBA_HIP_TRY(s, hipSetDevice(s->device));
  const size_t npix = (size_t)s->rows * s->cols;
  PBA_HIP_TRY(s, hipMemcpy(left, s->d_pf, npix, hipMemcpyDeviceToHost));
  PBA_HIP_TRY(s, hipMemcpy(right, s->d_pf + npix, npix, hipMemcpyDeviceToHost));
  return PBA_OK;
}

int pba_stereo_get_timing(pba_stereo* s, float* kernels_ms, float* total_ms) {
  if (!s) return PBA_ERR_INVALID;
  if (!s->computed) return fail(s, PBA_ERR_STATE, "pba_stereo_get_timing before pba_stereo_compute");
  if (kernels_ms) PBA_HIP_TRY(s, hipEventElapsedTime(kernels_ms, s->ev[1], s->ev[2]));
  if (total_ms) PBA_HIP_TRY(s, hipEventElapsedTime(total_ms, s->ev[0], s->ev[3]));
  return PBA_OK;
}

}  // extern "C"
