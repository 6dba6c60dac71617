// roi_loop.h — device kernels of the two 3-class frame loops that decide things per frame from the frame itself:
// infer_video_roi.py (detect_roi_by_projection :23-57, adaptive_thresholding :60-97, ultra_strict_threshold :100-125,
// refine_mask_by_geometry :128-167, the crop / resize / paste of infer_frame :200-247) and infer_video_3class_full.py
// (select_primary_component :85-114).  unet_amd/roi_loop.py holds the NumPy form of each; include/unetpp_roi.h the entries.
//
// Every per-frame decision stays on the device as a small table the next kernel reads:
//   roi         int32 [B,4]    (x_min, x_max, found, valid): the column range of the cable, valid = x_max > x_min
//   thresholds  float32 [B,3]  (t_cable, t_tape, bg_margin) of that frame's own probability means
// Every result is an integer sum, a maximum or a comparison: none depends on the order in which threads, waves or
// workgroups arrive.  Double arithmetic that restates a Python expression is compiled without contraction, so that a
// product and a sum stay two roundings.
//
// Arithmetic
//   column counts   c[x] = the non-zero pixels of column x (int32)
//   box sum         S[i] = sum of c[k] over m - 29 <= k <= m, 0 <= k < W, with m = i + (n - 1 - n / 2), n = min(W, 30), for
//                   0 <= i < max(W, 30): np.convolve(c, ones(30), mode='same'), whose result has max(W, 30) entries
//   decision        column i is significant when 10 S[i] > 3 max S (the reference's smooth > 0.3 * max on sums 255 / 30 times
//                   as large); first and last significant i are scaled as int(i * (W / 512)), margin = int((x_max - x_min) *
//                   0.1), x_min = max(0, x_min - margin), x_max = min(W, x_max + margin), all in float64; no significant
//                   column: (int(W * 0.25), int(W * 0.75)) and found = 0
//   crop / resize   OpenCV's 11-bit fixed-point INTER_LINEAR (oracle cv2_resize_linear_u8_np), the coefficients formed per
//                   thread: fx = (float)((d + 0.5) * (1 / (n_dst / n_src)) - 0.5), s = floor(fx), fx -= s, both clamped at the
//                   borders with fx = 0, a0 = rint((1 - fx) * 2048), a1 = rint(fx * 2048) in float32; horizontal pass
//                   p0 a0 + p1 a1 in int32, vertical pass (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2
//   means           sum of floor(clamp(p, 0, 1) * 2^32) per plane in uint64 (pm_q32 of probmap.h), one 64-bit atomic per
//                   workgroup and plane; mean = (float)((double)sum / ((double)n * 2^32)); max of max(p, 0)
//   thresholds      float32: t_cable = mean1 > 0.3 ? min(0.85, mean1 + 0.4) : 0.5; t_tape = mean2 > 0.15 ? min(0.85, mean2 + 0.5)
//                   : 0.55; bg_margin = max(0.2, 1 - mean0)
//   ultra strict    winner = first maximum of p0, p1, p2; class k in {1, 2}: winner == k and pk >= t_k and pk > p0 * 2 and
//                   pk >= p0 + bg_margin (the sum rounded to float32)
//   paste           OpenCV's INTER_NEAREST: source index min(floor(d * (1 / (n_dst / n_src))), n_src - 1) in float64
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "components.h"
#include "probmap.h"

namespace unetpp {

constexpr int ROI_THREADS = 256;
constexpr int ROI_WAVES = ROI_THREADS / 64;
constexpr int ROI_BAND = 32;                 // rows one thread of the column count walks
constexpr int ROI_BOX = 30;                  // the reference's smoothing window

// ---- 1. the cable's column range ----------------------------------------------------------------------------------------------
// counts[b][x] += the non-zero pixels of column x in rows [32 by, 32 by + 32); counts zeroed before the launch.
// Grid (ceil(W / 256), ceil(H / 32), B): a wave reads 64 consecutive bytes of a row.
__global__ void __launch_bounds__(ROI_THREADS) roi_column_count_kernel(const uint8_t* __restrict__ edges, int H, int W, int* __restrict__ counts) {
  const int x = blockIdx.x * ROI_THREADS + threadIdx.x, b = blockIdx.z;
  if (x >= W) return;
  const int y0 = blockIdx.y * ROI_BAND, y1 = min(y0 + ROI_BAND, H);
  const uint8_t* p = edges + ((size_t)b * H + y0) * W + x;
  int n = 0;
  for (int y = y0; y < y1; ++y, p += W) n += *p != 0;
  if (n) atomicAdd(counts + (size_t)b * W + x, n);
}

__device__ __forceinline__ int roi_box_sum(const int* __restrict__ c, int W, int i) {
  const int n = W < ROI_BOX ? W : ROI_BOX;
  const int m = i + (n - 1 - n / 2);
  const int lo = max(m - (ROI_BOX - 1), 0), hi = min(m, W - 1);
  int s = 0;
  for (int k = lo; k <= hi; ++k) s += c[k];
  return s;
}

// roi[b] = (x_min, x_max, found, valid) from counts[b].  Grid (B).  H <= 65535, so 10 S <= 10 * 30 * 65535 fits an int.
__global__ void __launch_bounds__(ROI_THREADS) roi_decide_kernel(const int* __restrict__ counts, int W, int* __restrict__ roi) {
#pragma clang fp contract(off)
  __shared__ int s_max, s_first, s_last;
  const int b = blockIdx.x, t = threadIdx.x;
  const int* c = counts + (size_t)b * W;
  const int n_out = W < ROI_BOX ? ROI_BOX : W;
  if (t == 0) { s_max = 0; s_first = n_out; s_last = -1; }
  __syncthreads();
  int mx = 0;
  for (int i = t; i < n_out; i += ROI_THREADS) mx = max(mx, roi_box_sum(c, W, i));
  if (mx) atomicMax(&s_max, mx);
  __syncthreads();
  const int top = 3 * s_max;
  int first = n_out, last = -1;
  for (int i = t; i < n_out; i += ROI_THREADS)
    if (10 * roi_box_sum(c, W, i) > top) { first = min(first, i); last = i; }
  if (last >= 0) { atomicMin(&s_first, first); atomicMax(&s_last, last); }
  __syncthreads();
  if (t == 0) {
    int x_min, x_max;
    const int found = s_last >= 0;
    if (found) {
      const double scale = (double)W / 512.0;
      x_min = (int)((double)s_first * scale);
      x_max = (int)((double)s_last * scale);
      const int margin = (int)((double)(x_max - x_min) * 0.1);
      x_min = max(0, x_min - margin);
      x_max = min(W, x_max + margin);
    } else {
      x_min = (int)((double)W * 0.25);
      x_max = (int)((double)W * 0.75);
    }
    int* o = roi + (size_t)b * 4;
    o[0] = x_min; o[1] = x_max; o[2] = found; o[3] = x_max > x_min;
  }
}

// ---- 2. crop and resize ---------------------------------------------------------------------------------------------------------
struct RoiCoef { int s0, s1, a0, a1; };

__device__ __forceinline__ RoiCoef roi_linear_coef(int d, int n_src, int n_dst) {
#pragma clang fp contract(off)
  const double scale = 1.0 / ((double)n_dst / (double)n_src);
  float fx = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(fx);
  fx = fx - (float)s;
  if (s < 0) { fx = 0.0f; s = 0; }
  if (s >= n_src - 1) { fx = 0.0f; s = n_src - 1; }
  RoiCoef c;
  c.s0 = s;
  c.s1 = min(s + 1, n_src - 1);
  c.a0 = (int)rintf((1.0f - fx) * 2048.0f);
  c.a1 = (int)rintf(fx * 2048.0f);
  return c;
}

// out[b] uint8 [OH,OW,C] = the resize of frames[b][:, x_min:x_max] (uint8 [H,W,C]); zeros for a frame whose roi is not
// valid.  Grid (ceil(OW / 256), OH, B), one output pixel per thread.  The range is clamped to the frame before it is used.
__global__ void __launch_bounds__(ROI_THREADS) roi_crop_resize_kernel(const uint8_t* __restrict__ frames, int H, int W, int C,
                                                                     const int* __restrict__ roi, int OH, int OW, uint8_t* __restrict__ out) {
  const int x = blockIdx.x * ROI_THREADS + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= OW) return;
  const int* r = roi + (size_t)b * 4;
  const int x_min = min(max(r[0], 0), W), x_max = min(max(r[1], 0), W);
  uint8_t* dst = out + (((size_t)b * OH + y) * OW + x) * C;
  if (!r[3] || x_max <= x_min) {
    for (int c = 0; c < C; ++c) dst[c] = 0;
    return;
  }
  const RoiCoef cx = roi_linear_coef(x, x_max - x_min, OW), cy = roi_linear_coef(y, H, OH);
  const uint8_t* row0 = frames + (((size_t)b * H + cy.s0) * W + x_min) * C;
  const uint8_t* row1 = frames + (((size_t)b * H + cy.s1) * W + x_min) * C;
  for (int c = 0; c < C; ++c) {
    const int S0 = (int)row0[(size_t)cx.s0 * C + c] * cx.a0 + (int)row0[(size_t)cx.s1 * C + c] * cx.a1;
    const int S1 = (int)row1[(size_t)cx.s0 * C + c] * cx.a0 + (int)row1[(size_t)cx.s1 * C + c] * cx.a1;
    const int v = (((cy.a0 * (S0 >> 4)) >> 16) + ((cy.a1 * (S1 >> 4)) >> 16) + 2) >> 2;
    dst[c] = (uint8_t)min(max(v, 0), 255);
  }
}

// ---- 3. the thresholds of a frame's own means ----------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long roi_wave_sum64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// sums[b][c] += sum of pm_q32(p), maxbits[b][c] = max of the bits of max(p, 0), over plane c < 3 of frame b of probs float32
// [B,C,HW]; both zeroed before the launch.  Grid (ceil(HW / 4096), 3, B).
__global__ void __launch_bounds__(ROI_THREADS) roi_plane_sums_kernel(const float* __restrict__ probs, int C, unsigned HW_,
                                                                    unsigned long long* __restrict__ sums, unsigned* __restrict__ maxbits) {
  __shared__ unsigned long long s_sum[ROI_WAVES];
  __shared__ unsigned s_max[ROI_WAVES];
  const long long HW = HW_;
  const int t = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const long long i0 = ((long long)blockIdx.x * ROI_THREADS + t) * PM_PX;
  unsigned long long q = 0ull;
  unsigned mx = 0u;
  if (i0 < HW) {
    float v[PM_PX];
    const int n = pm_load16(probs + ((size_t)b * C + c) * HW, i0, HW, 1, 0, v);
#pragma unroll
    for (int j = 0; j < PM_PX; ++j)
      if (j < n) {
        q += pm_q32(v[j]);
        if (v[j] > 0.0f) mx = max(mx, __float_as_uint(v[j]));          // positive floats order as their bits
      }
  }
  q = roi_wave_sum64(q);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, d, 64));
  if ((t & 63) == 0) { s_sum[t >> 6] = q; s_max[t >> 6] = mx; }
  __syncthreads();
  if (t == 0) {
    unsigned long long total = 0ull;
    unsigned m = 0u;
#pragma unroll
    for (int w = 0; w < ROI_WAVES; ++w) { total += s_sum[w]; m = max(m, s_max[w]); }
    if (total) atomicAdd(sums + (size_t)b * 3 + c, total);
    if (m) atomicMax(maxbits + (size_t)b * 3 + c, m);
  }
}

// thresholds, means, maxima float32 [B,3] from the sums.  Grid (ceil(B / 256)).
__global__ void __launch_bounds__(ROI_THREADS) roi_thresholds_kernel(const unsigned long long* __restrict__ sums, const unsigned* __restrict__ maxbits,
                                                                    int B, unsigned HW, float* __restrict__ thresholds, float* __restrict__ means,
                                                                    float* __restrict__ maxima) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * ROI_THREADS + threadIdx.x;
  if (b >= B) return;
  float m[3];
  for (int c = 0; c < 3; ++c) {
    m[c] = (float)((double)sums[(size_t)b * 3 + c] / ((double)HW * 4294967296.0));
    means[(size_t)b * 3 + c] = m[c];
    maxima[(size_t)b * 3 + c] = __uint_as_float(maxbits[(size_t)b * 3 + c]);
  }
  const float tc = m[1] + 0.4f, tt = m[2] + 0.5f, bm = 1.0f - m[0];
  thresholds[(size_t)b * 3 + 0] = m[1] > 0.3f ? (tc < 0.85f ? tc : 0.85f) : 0.5f;
  thresholds[(size_t)b * 3 + 1] = m[2] > 0.15f ? (tt < 0.85f ? tt : 0.85f) : 0.55f;
  thresholds[(size_t)b * 3 + 2] = bm > 0.2f ? bm : 0.2f;
}

// ---- 4. ultra_strict_threshold with the thresholds of the frame's table ------------------------------------------------------
__device__ __forceinline__ void roi_store16_u8(uint8_t* __restrict__ dst, int n, const unsigned (&w)[4]) {
  if (n == PM_PX && pm_aligned16(dst)) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int j = 0; j < PM_PX; ++j)
      if (j < n) dst[j] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// cable, tape uint8 [B,HW] from planes 0..2 of probs float32 [B,C,HW] and thresholds float32 [B,3].  Grid
// (ceil(HW / 4096), B); 16 pixels per thread, each plane and each output by 16-byte accesses where its own address allows.
__global__ void __launch_bounds__(ROI_THREADS) roi_ultra_strict_kernel(const float* __restrict__ probs, int C, unsigned HW_,
                                                                      const float* __restrict__ thresholds, uint8_t* __restrict__ cable,
                                                                      uint8_t* __restrict__ tape) {
#pragma clang fp contract(off)
  const long long HW = HW_;
  const int b = blockIdx.y;
  const long long i0 = ((long long)blockIdx.x * ROI_THREADS + threadIdx.x) * PM_PX;
  if (i0 >= HW) return;
  const float t_cable = thresholds[(size_t)b * 3], t_tape = thresholds[(size_t)b * 3 + 1], margin = thresholds[(size_t)b * 3 + 2];
  const float* frame = probs + (size_t)b * C * HW;
  float p0[PM_PX], p1[PM_PX], p2[PM_PX];
  const int n = pm_load16(frame, i0, HW, 1, 0, p0);
  pm_load16(frame + HW, i0, HW, 1, 0, p1);
  pm_load16(frame + 2 * HW, i0, HW, 1, 0, p2);
  unsigned wc[4] = {0, 0, 0, 0}, wt[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < PM_PX; ++j) {
    const float bg = p0[j], c = p1[j], t = p2[j];
    const float twice = bg * 2.0f, floor_ = bg + margin;
    const bool win1 = c > bg && !(t > c), win2 = t > bg && t > c;            // np.argmax: the first maximum
    const bool mc = win1 && c >= t_cable && c > twice && c >= floor_;
    const bool mt = win2 && t >= t_tape && t > twice && t >= floor_;
    wc[j >> 2] |= (mc ? 1u : 0u) << (8 * (j & 3));
    wt[j >> 2] |= (mt ? 1u : 0u) << (8 * (j & 3));
  }
  roi_store16_u8(cable + (size_t)b * HW + i0, n, wc);
  roi_store16_u8(tape + (size_t)b * HW + i0, n, wt);
}

// ---- 5. two component rules on the tables of unetpp_components -----------------------------------------------------------------
enum { ROI_RULE_GEOMETRY = 0, ROI_RULE_PRIMARY = 1 };
struct RoiCcRule { double min_area, min_aspect, wide_width, edge_lo, edge_hi, large_area; };

// refine_mask_by_geometry's loop body (:141-165): does component l stay.
__device__ __forceinline__ bool roi_geometry_keeps(const int* s, const unsigned long long* sm, const RoiCcRule& r, int W) {
#pragma clang fp contract(off)
  const double area = (double)s[4], w = (double)s[2], h = (double)s[3];
  if (area < r.min_area) return false;
  if (w > 0.0) {
    const double aspect = h / w;
    if (aspect < r.min_aspect && w > r.wide_width) return false;
  }
  const double cx = (double)(long long)((double)sm[0] / area);               // int(centroids[i][0])
  if (cx < (double)W * r.edge_lo || cx > (double)W * r.edge_hi)
    if (area < r.large_area) return false;
  return true;
}

// select_primary_component's loop body (:96-107): is component l a candidate, and its score.
__device__ __forceinline__ bool roi_primary_candidate(const int* s, const unsigned long long* sm, const RoiCcRule& r, int W, double* score) {
#pragma clang fp contract(off)
  const double area = (double)s[4];
  if (area < r.min_area) return false;
  const double aspect = (double)s[3] / fmax(1.0, (double)s[2]);
  if (aspect < r.min_aspect) return false;
  const double cx = (double)sm[0] / area;
  const double center_dist = fabs(cx - (double)W * 0.5) / fmax(1.0, (double)W);
  const double partial = area * aspect;
  *score = partial * (1.0 - center_dist);
  return *score > -1.0;                                      // best_score starts at -1.0
}

// keep uint8 [B,K] of one rule; a frame with num > K keeps nothing.  Grid (B).
__global__ void __launch_bounds__(CC_THREADS) roi_cc_select_kernel(const int* __restrict__ num, const int* __restrict__ stats,
                                                                  const unsigned long long* __restrict__ sums, int W, int K, int rule, RoiCcRule r,
                                                                  uint8_t* __restrict__ keep) {
  __shared__ double sc[CC_THREADS];
  __shared__ int lb[CC_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const int* st = stats + (size_t)b * K * 5;
  const unsigned long long* sm = sums + (size_t)b * K * 2;
  uint8_t* kp = keep + (size_t)b * K;
  const int n = num[b] <= K ? num[b] : 0;
  int best = -1;
  if (rule == ROI_RULE_PRIMARY) {
    double bs = 0.0;
    for (int l = 1 + t; l < n; l += CC_THREADS) {            // ascending labels: '>' keeps the first of equal scores
      double s;
      if (roi_primary_candidate(st + (size_t)l * 5, sm + (size_t)l * 2, r, W, &s) && (best < 0 || s > bs)) { bs = s; best = l; }
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
  }
  for (int l = t; l < K; l += CC_THREADS) {
    bool k = false;
    if (l >= 1 && l < n) k = rule == ROI_RULE_PRIMARY ? l == best : roi_geometry_keeps(st + (size_t)l * 5, sm + (size_t)l * 2, r, W);
    kp[l] = k ? 1 : 0;
  }
}

// ---- 6. resize the masks back and paste them into the frame ----------------------------------------------------------------------
__device__ __forceinline__ int roi_nearest_index(int d, int n_src, int n_dst) {
#pragma clang fp contract(off)
  const double ifx = 1.0 / ((double)n_dst / (double)n_src);
  return min((int)floor((double)d * ifx), n_src - 1);
}

// out0, out1 uint8 [B,OH,OW]: columns [x_min, x_max) hold the nearest resize of mask0, mask1 uint8 [B,MH,MW] to
// (x_max - x_min) x OH, every other pixel 0; all 0 for a frame whose roi is not valid.  Grid (ceil(OW / 256), OH, B).
__global__ void __launch_bounds__(ROI_THREADS) roi_paste_kernel(const uint8_t* __restrict__ mask0, const uint8_t* __restrict__ mask1, int MH, int MW,
                                                               const int* __restrict__ roi, int OH, int OW, uint8_t* __restrict__ out0,
                                                               uint8_t* __restrict__ out1) {
  const int x = blockIdx.x * ROI_THREADS + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= OW) return;
  const int* r = roi + (size_t)b * 4;
  const int x_min = min(max(r[0], 0), OW), x_max = min(max(r[1], 0), OW);
  const size_t at = ((size_t)b * OH + y) * OW + x;
  uint8_t v0 = 0, v1 = 0;
  if (r[3] && x >= x_min && x < x_max) {
    const size_t src = ((size_t)b * MH + roi_nearest_index(y, MH, OH)) * MW + roi_nearest_index(x - x_min, MW, x_max - x_min);
    v0 = mask0[src];
    v1 = mask1[src];
  }
  out0[at] = v0;
  out1[at] = v1;
}

}  // namespace unetpp
