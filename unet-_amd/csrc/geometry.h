// geometry.h — the measurement step of the reference's frame loop on the device: per-row widths and areas of two
// binary planes, their Gaussian smoothing / valid rows / medians (compute_diameter_metrics, compute_thickness_profile,
// src/utils/geometry_enhanced.py:45-225; diameter_profile_from_masks, src/utils/geometry.py:28-64) and the per-frame
// reduction of a component statistics table (analyze_defects, geometry_enhanced.py:286-311).
//
//   row_widths_kernel          one 64-lane wave per mask row, four rows per workgroup; first / last column by
//                              __ballot (64 bits) over the lanes' own hits, area by popcount; one global atomicAdd per
//                              workgroup and plane
//   width_profile_kernel       one workgroup per frame: widths with a reflect-101 halo in LDS, the symmetric column
//                              filter in float32 without contraction, valid rows, medians by a bitwise selection on
//                              the float bits (valid values are > 0, so their bits order as the values do)
//   components_summary_kernel  one workgroup per frame: count, filtered count, filtered area sum, largest area
//
// No workgroup waits for another; the only cross-workgroup results are integer atomicAdds, so the bits do not depend on
// arrival order.  Limits: GEO_MAX_ROWS = 4096 rows and GEO_MAX_TAPS = 127 taps for width_profile_kernel (its LDS is
// 2 * (4096 + 126) floats = 33,776 bytes plus 64 bytes of reduction slots; the smoothed values live in registers,
// 16 rows x 2 planes per thread).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "components.h"

namespace unetpp {

constexpr int GEO_THREADS = 256;
constexpr int GEO_WAVE = 64;
constexpr int GEO_ROWS_PER_WG = GEO_THREADS / GEO_WAVE;     // 4
constexpr int GEO_PX = 16;                                  // bytes per lane and pass: one 16-byte load
constexpr int GEO_PASS = GEO_WAVE * GEO_PX;                 // 1,024 columns per pass of a wave
constexpr int GEO_MAX_ROWS = 4096;
constexpr int GEO_MAX_TAPS = 127;
constexpr int GEO_MAX_R = GEO_MAX_TAPS / 2;                 // 63
constexpr int GEO_ROWS_PER_THREAD = GEO_MAX_ROWS / GEO_THREADS;   // 16

struct GeoTaps { float t[GEO_MAX_R + 1]; };                 // t[j] = taps[r + j]: the centre and one half of a symmetric kernel

struct GeoProfileOut { float dc_px, dt_px; int valid_rows; };

// 16 foreground bits of columns [col, col + 16) of one row; columns from W on read as background.
__device__ __forceinline__ unsigned geo_fg16(const uint8_t* __restrict__ row, int col, int W, int vec, int match) {
  unsigned bits = 0;
  if (col >= W) return 0;
  if (vec) {                                   // W % 16 == 0 and the mask is 16-byte aligned: the 16 pixels exist
    const uint4 v = *reinterpret_cast<const uint4*>(row + col);
    const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < GEO_PX; ++j) bits |= (unsigned)cc_is_fg((wv[j >> 2] >> (8 * (j & 3))) & 0xffu, match) << j;
  } else {
    const int n = min(GEO_PX, W - col);
    for (int j = 0; j < n; ++j) bits |= (unsigned)cc_is_fg(row[col + j], match) << j;
  }
  return bits;
}

__device__ __forceinline__ int geo_wave_sum(int v) {
#pragma unroll
  for (int d = GEO_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, GEO_WAVE);
  return v;
}

// grid (ceil(H / 4), B), 256 threads.  widths float32 [B,2,H], area uint32 [B,2] (zeroed by the caller on the stream).
// mask1 == nullptr: plane 1 is empty.
__global__ void __launch_bounds__(GEO_THREADS) row_widths_kernel(const uint8_t* __restrict__ mask0, int match0,
                                                                const uint8_t* __restrict__ mask1, int match1, int H, int W,
                                                                int vec0, int vec1, float* __restrict__ widths,
                                                                unsigned* __restrict__ area) {
  __shared__ unsigned s_cnt[GEO_ROWS_PER_WG][2];
  const int wave = threadIdx.x / GEO_WAVE, lane = threadIdx.x % GEO_WAVE;
  const int y = blockIdx.x * GEO_ROWS_PER_WG + wave, b = blockIdx.y;
  int cnt[2] = {0, 0};
  if (y < H) {
    const size_t off = ((size_t)b * H + y) * W;
    int first[2] = {-1, -1}, last[2] = {-1, -1};
    for (int c0 = 0; c0 < W; c0 += GEO_PASS) {
      const int col = c0 + lane * GEO_PX;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const uint8_t* m = p ? mask1 : mask0;
        if (!m) continue;                                   // uniform
        const unsigned bits = geo_fg16(m + off, col, W, p ? vec1 : vec0, p ? match1 : match0);
        cnt[p] += __popc(bits);
        const unsigned long long hit = __ballot(bits != 0);
        if (hit) {                                          // uniform: the lowest and the highest lane with a hit
          const int lf = __ffsll((long long)hit) - 1, ll = 63 - __clzll((long long)hit);
          const unsigned bf = __shfl(bits, lf, GEO_WAVE), bl = __shfl(bits, ll, GEO_WAVE);
          if (first[p] < 0) first[p] = c0 + lf * GEO_PX + __ffs(bf) - 1;
          last[p] = c0 + ll * GEO_PX + 31 - __clz(bl);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      cnt[p] = geo_wave_sum(cnt[p]);
      if (lane == 0) widths[((size_t)b * 2 + p) * H + y] = first[p] < 0 ? 0.0f : (float)(last[p] - first[p] + 1);
    }
  }
  if (lane == 0) { s_cnt[wave][0] = (unsigned)cnt[0]; s_cnt[wave][1] = (unsigned)cnt[1]; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned a = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
    if (a) atomicAdd(&area[(size_t)b * 2 + threadIdx.x], a);
  }
}

// cv2.borderInterpolate(p, n, BORDER_REFLECT_101), with its loop for a border wider than the image
__device__ __forceinline__ int geo_reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
  return p;
}

// Sum over the workgroup of four 16-bit counters packed in 64 bits (each total <= 4096).  `slots` is 2 x 4 values,
// used alternately (parity) so that one barrier per call suffices.
__device__ __forceinline__ unsigned long long geo_block_sum4(unsigned long long v, unsigned long long* slots, int parity) {
#pragma unroll
  for (int d = GEO_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, GEO_WAVE);
  unsigned long long* s = slots + parity * GEO_ROWS_PER_WG;
  if (threadIdx.x % GEO_WAVE == 0) s[threadIdx.x / GEO_WAVE] = v;
  __syncthreads();
  return s[0] + s[1] + s[2] + s[3];
}

// grid (B), 256 threads, dynamic LDS 2 * (H + 2 r) floats.  widths float32 [B,2,H] -> smoothed float32 [B,2,H],
// valid uint8 [B,H], delta float32 [B,H] = smoothed plane 1 - plane 0 (may be nullptr), out [B].
__global__ void __launch_bounds__(GEO_THREADS) width_profile_kernel(const float* __restrict__ widths, int H, GeoTaps taps, int r,
                                                                   int min_valid_rows, float* __restrict__ smoothed,
                                                                   uint8_t* __restrict__ valid, float* __restrict__ delta,
                                                                   GeoProfileOut* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ float geo_w[];                          // [2][H + 2 r]
  __shared__ unsigned long long slots[2 * GEO_ROWS_PER_WG];
  const int t = threadIdx.x, b = blockIdx.x, L = H + 2 * r;
  const float* src = widths + (size_t)b * 2 * H;
  for (int i = t; i < 2 * L; i += GEO_THREADS) {
    const int p = i >= L, k = i - p * L;
    geo_w[i] = src[(size_t)p * H + geo_reflect101(k - r, H)];
  }
  __syncthreads();
  float s0[GEO_ROWS_PER_THREAD], s1[GEO_ROWS_PER_THREAD];   // rows t, t + 256, ...: registers (the loop is unrolled)
  unsigned vbits = 0;
#pragma unroll
  for (int i = 0; i < GEO_ROWS_PER_THREAD; ++i) {
    const int y = t + i * GEO_THREADS;
    float a = 0.0f, c = 0.0f;
    if (y < H) {
      const float* w0 = geo_w + r + y;
      const float* w1 = w0 + L;
      a = taps.t[0] * w0[0];
      c = taps.t[0] * w1[0];
      for (int j = 1; j <= r; ++j) {
        const float tj = taps.t[j];
        a = a + tj * (w0[j] + w0[-j]);
        c = c + tj * (w1[j] + w1[-j]);
      }
      const bool v = a > 0.0f && c > 0.0f;
      vbits |= (unsigned)v << i;
      smoothed[(size_t)b * 2 * H + y] = a;
      smoothed[((size_t)b * 2 + 1) * H + y] = c;
      valid[(size_t)b * H + y] = v ? 1 : 0;
      if (delta) delta[(size_t)b * H + y] = c - a;
    }
    s0[i] = a; s1[i] = c;
  }
  int parity = 0;
  const int n = (int)(geo_block_sum4((unsigned long long)__popc(vbits), slots, parity) & 0xffffu);
  parity ^= 1;
  float med0 = 0.0f, med1 = 0.0f;
  if (n >= min_valid_rows) {                                // uniform
    // The k-th smallest (0-based) of the valid values of each plane for k = (n - 1) / 2 and n / 2, all four at once:
    // from the top bit down, a candidate bit stays when at most k values lie below the candidate.
    const unsigned klo = (unsigned)(n - 1) / 2, khi = (unsigned)n / 2;
    unsigned a_lo = 0, a_hi = 0, c_lo = 0, c_hi = 0;
    for (int bit = 30; bit >= 0; --bit) {                   // valid values are positive floats: bit 31 is clear
      const unsigned m = 1u << bit;
      const unsigned ta_lo = a_lo | m, ta_hi = a_hi | m, tc_lo = c_lo | m, tc_hi = c_hi | m;
      unsigned long long cnt = 0;
#pragma unroll
      for (int i = 0; i < GEO_ROWS_PER_THREAD; ++i) {
        if ((vbits >> i) & 1u) {
          const unsigned ua = __float_as_uint(s0[i]), uc = __float_as_uint(s1[i]);
          cnt += (unsigned long long)(ua < ta_lo) | ((unsigned long long)(ua < ta_hi) << 16) |
                 ((unsigned long long)(uc < tc_lo) << 32) | ((unsigned long long)(uc < tc_hi) << 48);
        }
      }
      cnt = geo_block_sum4(cnt, slots, parity);
      parity ^= 1;
      if ((unsigned)(cnt & 0xffffu) <= klo) a_lo = ta_lo;
      if ((unsigned)((cnt >> 16) & 0xffffu) <= khi) a_hi = ta_hi;
      if ((unsigned)((cnt >> 32) & 0xffffu) <= klo) c_lo = tc_lo;
      if ((unsigned)((cnt >> 48) & 0xffffu) <= khi) c_hi = tc_hi;
    }
    // np.median: the middle element, or the float32 sum of the two middle ones halved (odd n: both are the same
    // element and (x + x) / 2 is x again unless x + x overflows, which widths cannot)
    if (n & 1) { med0 = __uint_as_float(a_lo); med1 = __uint_as_float(c_lo); }
    else {
      med0 = (__uint_as_float(a_lo) + __uint_as_float(a_hi)) * 0.5f;
      med1 = (__uint_as_float(c_lo) + __uint_as_float(c_hi)) * 0.5f;
    }
  }
  if (t == 0) { out[b].dc_px = med0; out[b].dt_px = med1; out[b].valid_rows = n; }
}

// grid (B), 256 threads.  num int32 [B], stats int32 [B,K,5] (may be nullptr: only the count is formed) ->
// out int64 [B,4] = {max(0, num - 1), labels 1 .. min(num, K) - 1 with area >= min_area, their area sum, largest area}.
__global__ void __launch_bounds__(GEO_THREADS) components_summary_kernel(const int* __restrict__ num, const int* __restrict__ stats, int K,
                                                                        long long min_area, long long* __restrict__ out) {
  __shared__ long long s_cnt[GEO_ROWS_PER_WG], s_sum[GEO_ROWS_PER_WG], s_max[GEO_ROWS_PER_WG];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nb = num[b], n = nb < K ? nb : K;
  long long cnt = 0, sum = 0, mx = 0;
  if (stats) {
    const int* st = stats + (size_t)b * K * 5;
    for (int l = 1 + t; l < n; l += GEO_THREADS) {
      const long long a = st[(size_t)l * 5 + 4];
      if (a >= min_area) { ++cnt; sum += a; }
      if (a > mx) mx = a;
    }
  }
#pragma unroll
  for (int d = GEO_WAVE / 2; d > 0; d >>= 1) {
    cnt += __shfl_xor(cnt, d, GEO_WAVE);
    sum += __shfl_xor(sum, d, GEO_WAVE);
    const long long o = __shfl_xor(mx, d, GEO_WAVE);
    mx = o > mx ? o : mx;
  }
  if (t % GEO_WAVE == 0) { s_cnt[t / GEO_WAVE] = cnt; s_sum[t / GEO_WAVE] = sum; s_max[t / GEO_WAVE] = mx; }
  __syncthreads();
  if (t == 0) {
    long long c = 0, s = 0, m = 0;
    for (int w = 0; w < GEO_ROWS_PER_WG; ++w) { c += s_cnt[w]; s += s_sum[w]; m = s_max[w] > m ? s_max[w] : m; }
    long long* o = out + (size_t)b * 4;
    o[0] = nb > 1 ? (long long)nb - 1 : 0; o[1] = c; o[2] = s; o[3] = m;
  }
}

}  // namespace unetpp
