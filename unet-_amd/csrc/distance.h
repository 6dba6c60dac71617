// distance.h — the mask rules of the reference's robust frame loop (infer_video_robust.py) that had no device path:
// cv2.distanceTransform(mask, DIST_L2 | DIST_L1 | DIST_C, 3) with the ring band_in <= dist <= band_out of
// restrict_tape_to_cable_ring (:169-198) fused into it, keep_best_cable_cc's selection (:102-160), apply_roi_limit
// (:201-216) and the median of _measure_diameters (:372-387).
//
// The transform is OpenCV's published distanceTransform_3x3: a 16.16 fixed-point chamfer distance with weights HV (a step
// along a row or column) and DIAG (a diagonal step), capped at DT_CAP = INT_MAX >> 2, converted as (float)t * 2^-16.  Its
// two sequential raster scans are not ported.  Their integer result is the minimum over the zero pixels q of
// DIAG * min(|dx|, |dy|) + HV * (max(|dx|, |dy|) - min(|dx|, |dy|)), and that cost does not fall when |dy| grows, so per
// column only the vertically nearest zero pixel matters:
//   t(x, y) = min over x' of cost(|x - x'|, g(x', y)),   g(x', y) = rows to the nearest zero pixel of column x'
// Integer minima do not depend on order, so the result is bit for bit the two-pass one.
//
//   dt_bits_kernel     per column and band of 32 rows: the zero pixels as one 32-bit word; any zero at all -> flag[b]
//   dt_column_kernel   g as uint16 [B,H,W] from those words (DT_NONE: the column has no zero pixel)
//   dt_row_kernel      one workgroup per frame row, the row of g in LDS; every thread searches outward from dx = 0 and
//                      stops when HV * dx >= best.  Writes the float map and / or the ring mask.  With the ring alone the
//                      search starts from a bound just above `hi`, so it never looks further than the band is wide.
//   best_cable_select_kernel   keep[] of keep_best_cable_cc from unetpp_components' stats (cc_apply_kernel writes the mask)
//   roi_box_kernel / roi_apply_kernel   bounding box by integer atomicMax (exact in any order), then the cut
//   row_median_kernel  median of the widths > 1 of unetpp_row_widths by a bitwise selection, float64
//
// Sums stay in 32 bits: best <= DT_CAP < 2^29 bounds dx below 8579, and both terms of a cost are clamped where they
// already exceed the cap (DIAG * 8192 >= 2^29 and HV * 16384 > 2^29 for all three metrics), so a cost is below 2^32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "components.h"

namespace unetpp {

constexpr int DT_THREADS = 256;
constexpr int DT_WAVE = 64;
constexpr int DT_BAND = 32;                                  // rows per word of dt_bits_kernel
constexpr unsigned DT_NONE = 0xffffu;                        // g: no zero pixel in this column
constexpr unsigned DT_CAP = 0x7fffffffu >> 2;                // 536,870,911 = 8192 * 65536 - 1
constexpr unsigned DT_MAX_A = 8192, DT_MAX_C = 16384;        // clamps of the two terms of a cost (see above)

// is the pixel non-zero in the transform's sense: foreground of (mask, match), or its complement with `invert`
__device__ __forceinline__ bool dt_nonzero(unsigned v, int match, int invert) { return cc_is_fg(v, match) != (invert != 0); }

// grid (ceil(W / 256), ceil(H / 32), B).  bits uint32 [B,nbands,W]: bit r = row 32 band + r of the column is a zero pixel.
__global__ void __launch_bounds__(DT_THREADS) dt_bits_kernel(const uint8_t* __restrict__ src, int H, int W, int match, int invert,
                                                            unsigned* __restrict__ bits, int* __restrict__ flag) {
  const int x = blockIdx.x * DT_THREADS + threadIdx.x, band = blockIdx.y, b = blockIdx.z;
  const int nbands = gridDim.y, y0 = band * DT_BAND, rows = min(DT_BAND, H - y0);
  unsigned z = 0;
  if (x < W) {
    const uint8_t* p = src + ((size_t)b * H + y0) * W + x;
    for (int r = 0; r < rows; ++r) z |= (unsigned)!dt_nonzero(p[(size_t)r * W], match, invert) << r;
    bits[((size_t)b * nbands + band) * W + x] = z;
  }
  if (__syncthreads_or(z != 0) && threadIdx.x == 0) atomicOr(&flag[b], 1);
}

// same grid.  g uint16 [B,H,W] = min(|y - y'|) over the zero pixels (x, y') of the column, DT_NONE without one.
__global__ void __launch_bounds__(DT_THREADS) dt_column_kernel(const unsigned* __restrict__ bits, int H, int W, uint16_t* __restrict__ g) {
  const int x = blockIdx.x * DT_THREADS + threadIdx.x, band = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  const int nbands = gridDim.y, y0 = band * DT_BAND, rows = min(DT_BAND, H - y0);
  const unsigned* col = bits + (size_t)b * nbands * W + x;
  const unsigned z = col[(size_t)band * W];
  int above = -1, below = -1;                                // rows of the nearest zero pixels outside this band
  for (int k = band - 1; k >= 0; --k) {
    const unsigned w = col[(size_t)k * W];
    if (w) { above = k * DT_BAND + 31 - __clz(w); break; }
  }
  for (int k = band + 1; k < nbands; ++k) {
    const unsigned w = col[(size_t)k * W];
    if (w) { below = k * DT_BAND + __ffs(w) - 1; break; }
  }
  uint16_t* out = g + ((size_t)b * H + y0) * W + x;
  for (int r = 0; r < rows; ++r) {
    const int y = y0 + r;
    const unsigned lo = z & (0xffffffffu >> (31 - r)), hi = z >> r;            // zero pixels at or above / at or below row r
    const int up = lo ? r - (31 - __clz(lo)) : (above >= 0 ? y - above : (int)DT_NONE);
    const int dn = hi ? __ffs(hi) - 1 : (below >= 0 ? below - y : (int)DT_NONE);
    out[(size_t)r * W] = (uint16_t)min(up, dn);                // distances are < H <= 65535 = DT_NONE
  }
}

struct DtRing {                                              // the fused epilogue of dt_row_kernel
  const uint8_t* mask1;                                      // may be nullptr: no second condition
  int match1;
  float lo, hi;
  unsigned out_value;
};

__device__ __forceinline__ unsigned dt_cost(unsigned dx, unsigned gv, unsigned hv, unsigned diag) {
  const unsigned a = min(dx, gv), c = max(dx, gv) - a;
  return diag * min(a, DT_MAX_A) + hv * min(c, DT_MAX_C);
}

// grid (H, B), dynamic LDS 2 W bytes.  start = DT_CAP for the exact map; with the ring alone any bound above every t whose
// distance can still be <= hi.  dist float32 [B,H,W] and / or ring uint8 [B,H,W]; either may be nullptr.
__global__ void __launch_bounds__(DT_THREADS) dt_row_kernel(const uint16_t* __restrict__ g, const int* __restrict__ flag, int H, int W,
                                                           unsigned hv, unsigned diag, unsigned start, float* __restrict__ dist,
                                                           DtRing ring, uint8_t* __restrict__ ring_out) {
  extern __shared__ uint16_t dt_g[];                          // [W]
  const int y = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const size_t row = ((size_t)b * H + y) * W;
  const bool any_zero = flag[b] != 0;                        // uniform: a frame without a zero pixel is DT_CAP everywhere
  if (any_zero) {
    for (int x = t; x < W; x += DT_THREADS) dt_g[x] = g[row + x];
    __syncthreads();
  }
  for (int x = t; x < W; x += DT_THREADS) {
    unsigned best = start, g0 = DT_NONE;
    if (any_zero) {
      g0 = dt_g[x];
      if (g0 != DT_NONE) best = min(best, hv * min(g0, DT_MAX_C));
      const int reach = max(x, W - 1 - x);
      for (int dx = 1; dx <= reach && hv * (unsigned)dx < best; ++dx) {        // best < 2^29: dx stays below 8579
        if (x - dx >= 0) {
          const unsigned gv = dt_g[x - dx];
          if (gv != DT_NONE) best = min(best, dt_cost((unsigned)dx, gv, hv, diag));
        }
        if (x + dx < W) {
          const unsigned gv = dt_g[x + dx];
          if (gv != DT_NONE) best = min(best, dt_cost((unsigned)dx, gv, hv, diag));
        }
      }
    }
    const float d = (float)min(best, DT_CAP) * (1.0f / 65536.0f);
    if (dist) dist[row + x] = d;
    if (ring_out) {
      bool in = g0 != 0 && ring.lo <= d && d <= ring.hi;      // g == 0: the source pixel itself is a zero pixel
      if (in && ring.mask1) in = cc_is_fg(ring.mask1[row + x], ring.match1);
      ring_out[row + x] = in ? (uint8_t)ring.out_value : 0;
    }
  }
}

// ---- keep_best_cable_cc (infer_video_robust.py:102-160) -------------------------------------------------------------------
struct BestCableRule { double min_area, min_aspect; int min_h, max_w, H, W; };

__device__ __forceinline__ bool best_cable_candidate(const int* s, const BestCableRule& r, double* score) {
#pragma clang fp contract(off)
  const int w = s[2], h = s[3];
  const double area = (double)s[4];
  if (area < r.min_area) return false;
  if (h < r.min_h) return false;
  if (w > r.max_w) return false;
  const double aspect = (double)h / ((double)w + 1e-6);
  if (aspect < r.min_aspect) return false;
  *score = ((double)h / (double)r.H) * 3.0 + fmin(aspect, 12.0) * 0.5 + (area / ((double)r.H * (double)r.W)) * 0.5;
  return true;                                               // best_score starts at -1e9; a score is >= 0
}

// grid (B).  keep uint8 [B,K]: 1 on the first component with the strictly greatest score; num > K keeps nothing.
__global__ void __launch_bounds__(CC_THREADS) best_cable_select_kernel(const int* __restrict__ num, const int* __restrict__ stats, int K,
                                                                      BestCableRule r, uint8_t* __restrict__ keep) {
  __shared__ double sc[CC_THREADS];
  __shared__ int lb[CC_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const int* st = stats + (size_t)b * K * 5;
  const int n = num[b] <= K ? num[b] : 0;
  double bs = 0.0;
  int best = -1;
  for (int l = 1 + t; l < n; l += CC_THREADS) {              // ascending labels: '>' keeps the first of equal scores
    double s;
    if (best_cable_candidate(st + (size_t)l * 5, r, &s) && (best < 0 || s > bs)) { bs = s; best = l; }
  }
  sc[t] = bs; lb[t] = best;
  __syncthreads();
  for (int d = CC_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) {
      const int ol = lb[t + d];
      const double os = sc[t + d];
      if (ol >= 0 && (lb[t] < 0 || os > sc[t] || (os == sc[t] && ol < lb[t]))) { sc[t] = os; lb[t] = ol; }
    }
    __syncthreads();
  }
  best = lb[0];
  for (int l = t; l < K; l += CC_THREADS) keep[(size_t)b * K + l] = (l == best) ? 1 : 0;
}

// ---- apply_roi_limit (infer_video_robust.py:201-216) ----------------------------------------------------------------------
// box int32 [B,4] = {max(W - 1 - x), max(H - 1 - y), max x, max y} over the non-zero pixels, all -1 before (memset 0xff).
// grid (ceil(H / 4), B): one wave per row.
__global__ void __launch_bounds__(DT_THREADS) roi_box_kernel(const uint8_t* __restrict__ cable, int H, int W, int* __restrict__ box) {
  const int wave = threadIdx.x / DT_WAVE, lane = threadIdx.x % DT_WAVE;
  const int y = blockIdx.x * (DT_THREADS / DT_WAVE) + wave, b = blockIdx.y;
  if (y >= H) return;
  const uint8_t* p = cable + ((size_t)b * H + y) * W;
  int first = -1, last = -1;
  for (int x = lane; x < W; x += DT_WAVE)
    if (p[x]) { if (first < 0) first = x; last = x; }
  int nfirst = first < 0 ? -1 : W - 1 - first;               // a maximum again
#pragma unroll
  for (int d = DT_WAVE / 2; d > 0; d >>= 1) {
    nfirst = max(nfirst, __shfl_xor(nfirst, d, DT_WAVE));
    last = max(last, __shfl_xor(last, d, DT_WAVE));
  }
  if (lane == 0 && last >= 0) {
    int* o = box + (size_t)b * 4;
    atomicMax(&o[0], nfirst); atomicMax(&o[1], H - 1 - y); atomicMax(&o[2], last); atomicMax(&o[3], y);
  }
}

// grid (ceil(W / 1024), H, B), four pixels per thread.  out = mask inside the padded, clipped box, 0 outside and everywhere
// when the cable is empty.
__global__ void __launch_bounds__(DT_THREADS) roi_apply_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ box, int H, int W,
                                                              int pad, int vec, uint8_t* __restrict__ out) {
  const int x0 = (blockIdx.x * DT_THREADS + threadIdx.x) * 4, y = blockIdx.y, b = blockIdx.z;
  if (x0 >= W) return;
  const int* o = box + (size_t)b * 4;
  const bool some = o[2] >= 0;
  const int x1 = max(0, W - 1 - o[0] - pad), y1 = max(0, H - 1 - o[1] - pad);
  const int x2 = min(W - 1, o[2] + pad), y2 = min(H - 1, o[3] + pad);
  const bool row_in = some && y >= y1 && y <= y2;
  const size_t at = ((size_t)b * H + y) * W + x0;
  if (vec) {                                                 // W % 4 == 0 and both pointers 4-byte aligned
    unsigned v = row_in ? *reinterpret_cast<const unsigned*>(mask + at) : 0u, keep = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j >= x1 && x0 + j <= x2) keep |= 0xffu << (8 * j);
    *reinterpret_cast<unsigned*>(out + at) = v & keep;
  } else {
    for (int j = 0; j < 4 && x0 + j < W; ++j) out[at + j] = (row_in && x0 + j >= x1 && x0 + j <= x2) ? mask[at + j] : 0;
  }
}

// ---- the median of _measure_diameters (infer_video_robust.py:372-387) ----------------------------------------------------
// widths float32 [B,2,H] of unetpp_row_widths (integers 0..65535).  A row has more than one foreground pixel exactly when
// its width is above 1.  grid (2, B): median float64 [B,2] = np.median of the widths > 1 (the middle value, or the mean
// of the two middle ones), 0 when no row qualifies.  The k-th smallest by a selection from the top bit down: a candidate
// bit stays when at most k values lie below the candidate.
__global__ void __launch_bounds__(DT_THREADS) row_median_kernel(const float* __restrict__ widths, int H, double* __restrict__ median) {
  __shared__ unsigned s_cnt[2][DT_THREADS / DT_WAVE][2];
  const int p = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const float* w = widths + ((size_t)b * 2 + p) * H;
  auto block_sum2 = [&](unsigned a, unsigned c, int parity, unsigned* ra, unsigned* rc) {
#pragma unroll
    for (int d = DT_WAVE / 2; d > 0; d >>= 1) { a += __shfl_xor(a, d, DT_WAVE); c += __shfl_xor(c, d, DT_WAVE); }
    if (t % DT_WAVE == 0) { s_cnt[parity][t / DT_WAVE][0] = a; s_cnt[parity][t / DT_WAVE][1] = c; }
    __syncthreads();
    *ra = s_cnt[parity][0][0] + s_cnt[parity][1][0] + s_cnt[parity][2][0] + s_cnt[parity][3][0];
    *rc = s_cnt[parity][0][1] + s_cnt[parity][1][1] + s_cnt[parity][2][1] + s_cnt[parity][3][1];
  };
  unsigned mine = 0, n, unused;
  for (int y = t; y < H; y += DT_THREADS) mine += w[y] > 1.0f;
  int parity = 0;
  block_sum2(mine, 0u, parity, &n, &unused);
  parity ^= 1;
  double med = 0.0;
  if (n) {                                                   // uniform
    const unsigned klo = (n - 1) / 2, khi = n / 2;
    unsigned lo = 0, hi = 0;
    for (int bit = 16; bit >= 0; --bit) {                    // widths are <= 65535 < 2^17
      const unsigned tl = lo | (1u << bit), th = hi | (1u << bit);
      unsigned cl = 0, ch = 0;
      for (int y = t; y < H; y += DT_THREADS) {
        const float v = w[y];
        if (v > 1.0f) { const unsigned u = (unsigned)v; cl += u < tl; ch += u < th; }
      }
      block_sum2(cl, ch, parity, &cl, &ch);
      parity ^= 1;
      if (cl <= klo) lo = tl;
      if (ch <= khi) hi = th;
    }
    med = ((double)lo + (double)hi) * 0.5;                   // odd n: lo == hi
  }
  if (t == 0) median[(size_t)b * 2 + p] = med;
}

}  // namespace unetpp
