// multiclass.h — what the 6- and 7-class video loops (infer_video.py, infer_video_v3_high_quality.py, infer_video_optimized.py)
// do around the network, on the device:
//   quality_sums_kernel / quality_finish_kernel   FrameQualityGate.check: BGR -> grey and five integer sums per frame, then the
//                                                 statistics and the decision in float64 from the sums
//   threshold_classes_kernel                      five probability planes, resized in place, -> one bit map per pixel
//   merge_classes_kernel                          class planes cut from one uint8 map by a table, one morphology program per plane
//                                                 in LDS (the band and halo machinery of morphology.h), a priority merge, and the
//                                                 per-value table count / x0 / y0 / x1 / y1 of the merged map
//   overlay_kernel                                overlay_mask: the region blend and the cv2.addWeighted form
// Every sum is an integer sum, a minimum or a maximum: no result depends on the order in which workgroups arrive.  The float
// rules are float32 in the order written in multiclass.py, contraction off.  unet_amd/multiclass.py holds the NumPy forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "edges.h"
#include "morphology.h"

namespace unetpp {

constexpr int MC_THREADS = 256;

__device__ __forceinline__ unsigned mc_byte(const unsigned w[4], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// ---- the frame quality gate ---------------------------------------------------------------------------------------------------
constexpr int QG_TW = 128, QG_TH = 16, QG_PX = 8;            // a workgroup's tile; pixels of a row one thread owns
constexpr int QG_LDS_W = QG_TW + 4;                          // tile + one halo column either side, rows 4-byte aligned
constexpr int QG_SUMS = 5;                                   // sum g, sum g^2, sum L, sum L^2, sum |g - g_prev|
static_assert(QG_TW / QG_PX * QG_TH == MC_THREADS, "one thread per QG_PX pixels of the tile");

// gray [B,H,W] = cvtColor(BGR2GRAY) of bgr [B,H,W,3]; sums[b][0..4] += the five sums of frame b over this tile (zero before the
// launch).  L is the ksize-1 Laplacian with BORDER_REFLECT_101.  The previous frame of frame b > 0 is frame b - 1 of the batch,
// whose grey value is formed from its BGR pixel here (its grey frame is being written by other workgroups of this launch); the
// previous frame of frame 0 is prev_gray [H,W], and without it the difference is 0.
// Per workgroup: sum g^2 <= 2048 * 255^2 and sum L^2 <= 2048 * 1020^2 < 2^32, so the partial sums are 32-bit; one 64-bit
// atomic per sum.  Grid (ceil(W / QG_TW), ceil(H / QG_TH), B).
__global__ void __launch_bounds__(MC_THREADS) quality_sums_kernel(const uint8_t* __restrict__ bgr, const uint8_t* __restrict__ prev_gray, int H,
                                                                 int W, int vec_out, uint8_t* __restrict__ gray,
                                                                 unsigned long long* __restrict__ sums) {
  __shared__ uint8_t g[QG_TH + 2][QG_LDS_W];
  __shared__ unsigned part[MC_THREADS / 64][QG_SUMS];
  const int t = threadIdx.x, b = blockIdx.z;
  const int x0 = (int)blockIdx.x * QG_TW, y0 = (int)blockIdx.y * QG_TH;
  const size_t frame = (size_t)b * H * W;
  const uint8_t* f = bgr + frame * 3;
  for (int i = t; i < (QG_TH + 2) * (QG_TW + 2); i += MC_THREADS) {
    const int r = i / (QG_TW + 2), c = i - r * (QG_TW + 2);
    const uint8_t* s = f + ((size_t)ed_reflect(y0 + r - 1, H) * W + ed_reflect(x0 + c - 1, W)) * 3;      // always inside the frame
    g[r][c] = (uint8_t)gray_of_bgr(s[0], s[1], s[2]);
  }
  __syncthreads();
  const int r = t / (QG_TW / QG_PX), cx = (t % (QG_TW / QG_PX)) * QG_PX;
  const int y = y0 + r, xs = x0 + cx;
  unsigned s1 = 0, s2 = 0, sl2 = 0, sd = 0;
  int sl = 0;
  if (y < H && xs < W) {
    const int n = min(QG_PX, W - xs);
    const uint8_t* fp = b > 0 ? f - (size_t)H * W * 3 + ((size_t)y * W + xs) * 3 : nullptr;
    const uint8_t* pg = b == 0 && prev_gray ? prev_gray + (size_t)y * W + xs : nullptr;
    unsigned wv[2] = {0, 0};
    for (int j = 0; j < n; ++j) {
      const int c = cx + j + 1;
      const int gv = g[r + 1][c];
      const int lap = (int)g[r][c] + (int)g[r + 2][c] + (int)g[r + 1][c - 1] + (int)g[r + 1][c + 1] - 4 * gv;
      s1 += (unsigned)gv; s2 += (unsigned)(gv * gv);
      sl += lap; sl2 += (unsigned)(lap * lap);
      if (fp) sd += (unsigned)abs(gv - gray_of_bgr(fp[3 * j], fp[3 * j + 1], fp[3 * j + 2]));
      else if (pg) sd += (unsigned)abs(gv - (int)pg[j]);
      wv[j >> 2] |= (unsigned)gv << (8 * (j & 3));
    }
    uint8_t* dst = gray + frame + (size_t)y * W + xs;
    if (vec_out && n == QG_PX) *reinterpret_cast<uint2*>(dst) = make_uint2(wv[0], wv[1]);
    else for (int j = 0; j < n; ++j) dst[j] = (uint8_t)(wv[j >> 2] >> (8 * (j & 3)));
  }
  unsigned v[QG_SUMS] = {s1, s2, (unsigned)sl, sl2, sd};     // sl: two's complement, the wrap-around sum is the signed sum
#pragma unroll
  for (int k = 0; k < QG_SUMS; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += (unsigned)__shfl_xor((int)v[k], d, 64);
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < QG_SUMS; ++k) part[t >> 6][k] = v[k];
  }
  __syncthreads();
  if (t < QG_SUMS) {
    unsigned n = 0;
#pragma unroll
    for (int wv = 0; wv < MC_THREADS / 64; ++wv) n += part[wv][t];
    const unsigned long long add = t == 2 ? (unsigned long long)(long long)(int)n : (unsigned long long)n;
    if (add) atomicAdd(sums + (size_t)b * QG_SUMS + t, add);
  }
}

// The correctly rounded float64 of (nh * 2^64 + nl) / d for d > 0: a bit-serial division that keeps the first 55 significant
// quotient bits and a sticky bit, then rounds to 53 bits, ties to even (what Python's int / int gives).
__device__ inline double mc_ratio(unsigned long long nh, unsigned long long nl, unsigned long long d) {
  if (!(nh | nl)) return 0.0;
  unsigned long long rem = 0, q = 0;
  int nb = 0, i = 127;
  for (;; --i) {
    const unsigned long long bit = i >= 64 ? (nh >> (i - 64)) & 1ull : i >= 0 ? (nl >> i) & 1ull : 0ull;
    const bool carry = (rem >> 63) != 0;
    rem = (rem << 1) | bit;
    const bool qb = carry || rem >= d;
    if (qb) rem -= d;
    if (nb || qb) { q = (q << 1) | (qb ? 1ull : 0ull); ++nb; }
    if (nb == 55) break;
  }
  bool sticky = rem != 0;
  if (i > 64) sticky = sticky || nl != 0 || (nh & ((1ull << (i - 64)) - 1ull)) != 0;
  else if (i == 64) sticky = sticky || nl != 0;
  else if (i > 0) sticky = sticky || (nl & ((1ull << i) - 1ull)) != 0;
  const unsigned low = (unsigned)(q & 3ull);
  unsigned long long q53 = q >> 2;
  if (low == 3u || (low == 2u && (sticky || (q53 & 1ull)))) ++q53;
  return ldexp((double)q53, i + 2);
}

// (n * s2 - s1^2) / n^2 for |s1| = a1: the variance of n integers from their exact sums; n < 2^32.
__device__ inline double mc_variance(unsigned long long n, unsigned long long a1, unsigned long long s2) {
  const unsigned long long ph = __umul64hi(n, s2), pl = n * s2, qh = __umul64hi(a1, a1), ql = a1 * a1;
  const unsigned long long lo = pl - ql, hi = ph - qh - (pl < ql ? 1ull : 0ull);      // >= 0 by Cauchy-Schwarz
  return mc_ratio(hi, lo, n * n);
}

// FrameQualityGate.check's statistics and tests from the sums, one thread per frame.  reason: 0 disabled, 1 glitch
// (std < glitch_flat_th), 2 motion blur (lap_var < blur_th and mad > motion_th), 3 too flat (std < flat_th), 4 ok.
__global__ void quality_finish_kernel(const unsigned long long* __restrict__ sums, int B, unsigned long long n, int enable, double blur_th,
                                      double flat_th, double motion_th, double glitch_flat_th, uint8_t* __restrict__ is_bad,
                                      uint8_t* __restrict__ reason, double* __restrict__ lap_var, double* __restrict__ gray_std,
                                      double* __restrict__ mad) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const unsigned long long* s = sums + (size_t)b * QG_SUMS;
  const double sd = sqrt(mc_variance(n, s[0], s[1]));
  if (!enable) {
    is_bad[b] = 0; reason[b] = 0; lap_var[b] = 0.0; gray_std[b] = sd; mad[b] = 0.0;
    return;
  }
  const long long l1 = (long long)s[2];
  const double lv = mc_variance(n, (unsigned long long)(l1 < 0 ? -l1 : l1), s[3]);
  const double m = mc_ratio(0ull, s[4], n);
  int why = 4;
  if (sd < glitch_flat_th) why = 1;
  else if (lv < blur_th && m > motion_th) why = 2;
  else if (sd < flat_th) why = 3;
  is_bad[b] = why != 4; reason[b] = (uint8_t)why; lap_var[b] = lv; gray_std[b] = sd; mad[b] = m;
}

// ---- probability planes -> class bits -------------------------------------------------------------------------------------------
constexpr int TC_PLANES = 5, TC_PX = 4;
struct ThresholdArgs {
  long long chan_off[TC_PLANES];    // float offset of plane k inside a frame
  long long frame_stride;           // floats from one frame to the next
  int pixel_stride;                 // floats from one pixel of a plane to the next
  int sh, sw, H, W, resize;         // the planes' size, the bit map's size, resize = the two differ
  float thr[TC_PLANES], ratio;
};

// out uint8 [B,H,W]: bit 0 cable >= thr0 and cable > tape * ratio, bit 1 tape >= thr1 and tape > cable * ratio, bits 2..4
// plane k >= thr k.  With resize each plane is sampled at (H, W) as the float32 INTER_LINEAR resize does: xtab / ytab entry
// {s0, s1, bits of 1 - f, bits of f}; horizontal S[s0] a0 + S[s1] a1 on both rows, then r0 b0 + r1 b1.  NaN sets no bit.
// Grid (ceil(W / (TC_PX * 256)), H, B).
__global__ void __launch_bounds__(MC_THREADS) threshold_classes_kernel(const float* __restrict__ prob, const ThresholdArgs A,
                                                                      const int4* __restrict__ xtab, const int4* __restrict__ ytab, int vec_out,
                                                                      uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  const int xs = ((int)blockIdx.x * MC_THREADS + (int)threadIdx.x) * TC_PX, y = blockIdx.y;
  if (xs >= A.W) return;
  const int n = min(TC_PX, A.W - xs);
  const float* fb = prob + (size_t)blockIdx.z * A.frame_stride;
  int4 yt = make_int4(y, y, 0, 0);
  if (A.resize) yt = ytab[y];
  const float b0 = __int_as_float(yt.z), b1 = __int_as_float(yt.w);
  unsigned packed = 0;
  for (int j = 0; j < n; ++j) {
    const int x = xs + j;
    int4 xt = make_int4(x, x, 0, 0);
    if (A.resize) xt = xtab[x];
    const float a0 = __int_as_float(xt.z), a1 = __int_as_float(xt.w);
    float p[TC_PLANES];
#pragma unroll
    for (int k = 0; k < TC_PLANES; ++k) {
      const float* pl = fb + A.chan_off[k];
      const size_t row0 = (size_t)yt.x * A.sw;
      if (!A.resize) {
        p[k] = pl[(row0 + xt.x) * A.pixel_stride];
      } else {
        const size_t row1 = (size_t)yt.y * A.sw;
        const float r0 = pl[(row0 + xt.x) * A.pixel_stride] * a0 + pl[(row0 + xt.y) * A.pixel_stride] * a1;
        const float r1 = pl[(row1 + xt.x) * A.pixel_stride] * a0 + pl[(row1 + xt.y) * A.pixel_stride] * a1;
        p[k] = r0 * b0 + r1 * b1;
      }
    }
    unsigned bits = 0;
    if (p[0] >= A.thr[0] && p[0] > p[1] * A.ratio) bits |= 1u;
    if (p[1] >= A.thr[1] && p[1] > p[0] * A.ratio) bits |= 2u;
#pragma unroll
    for (int k = 2; k < TC_PLANES; ++k)
      if (p[k] >= A.thr[k]) bits |= 1u << k;
    packed |= bits << (8 * j);
  }
  uint8_t* dst = out + ((size_t)blockIdx.z * A.H + y) * A.W + xs;
  if (vec_out && n == TC_PX) *reinterpret_cast<unsigned*>(dst) = packed;
  else for (int j = 0; j < n; ++j) dst[j] = (uint8_t)(packed >> (8 * j));
}

// ---- class planes, their morphology programs, the priority merge and the class table --------------------------------------------
constexpr int MC_MAX_PLANES = 6;
constexpr int MC_TABLE_COLS = 5;                              // count, x0, y0, x1, y1
constexpr int MC_LDS_WORDS = 7296;                            // 64-bit words of dynamic LDS: 57 KB beside the 5.25 KB of static tables
enum { MC_OPEN = 6, MC_CLOSE = 7 };                           // beside MORPH_DILATE and MORPH_ERODE

struct MergeStep { int plane, op, elem, iters; };
struct MergeArgs {
  MorphElem elem[MORPH_MAX_ELEMENTS];
  MergeStep step[MORPH_MAX_STEPS];
  int out_value[MC_MAX_PLANES];     // 1..255, or -1: the input pixel's own value
  uint8_t lut[256];                 // input value -> the set of planes it belongs to (bit k = plane k)
  int n_steps, n_planes;
  int H, W, wpr;
  int band, up, rows;
  int cw, hl, tw;
  int vec_in, vec_out, table_classes;      // table_classes = 0: no table
};

// The run of equal output values a thread is in, kept in registers; a value change sends it to the workgroup's table in LDS.
struct McRun { int key, n, x0, y0, x1, y1; };
__device__ __forceinline__ void mc_run_flush(const McRun& r, int (*tab)[256], int classes) {
  if (!r.n || r.key >= classes) return;
  atomicAdd(&tab[0][r.key], r.n);
  atomicMin(&tab[1][r.key], r.x0); atomicMin(&tab[2][r.key], r.y0);
  atomicMax(&tab[3][r.key], r.x1); atomicMax(&tab[4][r.key], r.y1);
}
__device__ __forceinline__ void mc_run_add(McRun& r, int key, int n, int xa, int xb, int y, int (*tab)[256], int classes) {
  if (key != r.key) {
    mc_run_flush(r, tab, classes);
    r.key = key; r.n = 0; r.x0 = r.y0 = INT_MAX; r.x1 = r.y1 = -1;
  }
  r.n += n; r.x0 = min(r.x0, xa); r.x1 = max(r.x1, xb); r.y0 = min(r.y0, y); r.y1 = max(r.y1, y);
}

// table int32 [B,classes,5]: count 0, x0 = y0 = 0xffffffff (the unsigned minimum's identity, -1 as int32), x1 = y1 = -1.
__global__ void merge_table_init_kernel(int* __restrict__ table, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  int* p = table + (size_t)i * MC_TABLE_COLS;
  p[0] = 0; p[1] = p[2] = p[3] = p[4] = -1;
}

// grid (tiles in x, bands, B), MORPH_THREADS threads, dynamic LDS = (n_planes + 2) * rows * tw * 8 bytes: the class planes,
// then two scratch planes the steps of a program alternate between.  Tiling, halo and border rule are morph_program_kernel's.
//   1. every plane's bits of the tile's window, all from one read of the map: bit k of lut[value]
//   2. per plane its steps in order (open = erode then dilate, close = dilate then erode, each `iters` times); the result is
//      copied back to the plane
//   3. per core pixel the planes in order, a later one overwriting an earlier: out_value[k], or the input's own value
//   4. the table of the output values below table_classes: per workgroup in LDS, then one atomic add / min / max per non-empty
//      value.  x0 and y0 are unsigned minima (0xffffffff = none), x1 and y1 signed maxima (-1 = none).
// out may be NULL (the table alone).
__global__ void __launch_bounds__(MORPH_THREADS) merge_classes_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out,
                                                                     int* __restrict__ table, const MergeArgs A) {
  static_assert(MORPH_THREADS == 256, "one thread per table entry");
  extern __shared__ unsigned long long mc_lds[];
  __shared__ uint8_t lut[256];
  __shared__ int tab[MC_TABLE_COLS][256];
  const int t = threadIdx.x;
  MorphTile tl;
  tl.y_org = (int)blockIdx.y * A.band - A.up;
  tl.w_org = (int)blockIdx.x * A.cw - A.hl;
  tl.rows = A.rows; tl.tw = A.tw; tl.H = A.H; tl.wpr = A.wpr;
  tl.tail = (A.W & 63) ? (1ull << (A.W & 63)) - 1ull : ~0ull;
  const int pw = A.rows * A.tw;
  const size_t frame = (size_t)blockIdx.z * A.H * A.W;
  const uint8_t* src_frame = mask + frame;
  lut[t] = A.lut[t];
  tab[0][t] = 0; tab[1][t] = tab[2][t] = INT_MAX; tab[3][t] = tab[4][t] = -1;
  __syncthreads();

  // 1. one item = 16 pixels = one unsigned short of every plane
  unsigned short* p16 = reinterpret_cast<unsigned short*>(mc_lds);
  const int items = pw * 4;
  for (int it = t; it < items; it += MORPH_THREADS) {
    const int wc = it >> 2, r = wc / A.tw, c = wc - r * A.tw;
    const int y = tl.y_org + r, gw = tl.w_org + c, x = gw * 64 + (it & 3) * 16;
    unsigned bits[MC_MAX_PLANES] = {0, 0, 0, 0, 0, 0};
    if (y >= 0 && y < A.H && gw >= 0 && x < A.W) {
      const uint8_t* s = src_frame + (size_t)y * A.W + x;
      const int left = A.W - x;
      if (A.vec_in && left >= 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(s);
        const unsigned wv[4] = {v.x, v.y, v.z, v.w};
        const unsigned same = (wv[0] & 0xffu) * 0x01010101u;
        if (wv[0] == same && wv[1] == same && wv[2] == same && wv[3] == same) {
          const unsigned m = lut[wv[0] & 0xffu];
#pragma unroll
          for (int k = 0; k < MC_MAX_PLANES; ++k) bits[k] = ((m >> k) & 1u) ? 0xffffu : 0u;
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const unsigned m = lut[mc_byte(wv, j)];
#pragma unroll
            for (int k = 0; k < MC_MAX_PLANES; ++k) bits[k] |= ((m >> k) & 1u) << j;
          }
        }
      } else {
        for (int j = 0; j < 16 && j < left; ++j) {
          const unsigned m = lut[s[j]];
#pragma unroll
          for (int k = 0; k < MC_MAX_PLANES; ++k) bits[k] |= ((m >> k) & 1u) << j;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < MC_MAX_PLANES; ++k)
      if (k < A.n_planes) p16[(size_t)k * pw * 4 + it] = (unsigned short)bits[k];
  }
  __syncthreads();

  // 2. the programs; every branch below is uniform over the workgroup
  unsigned long long* const s0 = mc_lds + (size_t)A.n_planes * pw;
  unsigned long long* const s1 = s0 + pw;
  for (int k = 0; k < A.n_planes; ++k) {
    unsigned long long* const P = mc_lds + (size_t)k * pw;
    const unsigned long long* cur = P;
    for (int s = 0; s < A.n_steps; ++s) {
      const MergeStep st = A.step[s];
      if (st.plane != k) continue;
      const int halves = st.op == MC_OPEN || st.op == MC_CLOSE ? 2 : 1;
      for (int h = 0; h < halves; ++h) {
        const bool erode = st.op == MORPH_ERODE || (st.op == MC_OPEN && h == 0) || (st.op == MC_CLOSE && h == 1);
        for (int i = 0; i < st.iters; ++i) {
          unsigned long long* const o = cur == s0 ? s1 : s0;
          morph_step_plane(cur, o, A.elem[st.elem], erode, tl);
          __syncthreads();
          cur = o;
        }
      }
    }
    if (cur != P) {
      for (int i = t; i < pw; i += MORPH_THREADS) P[i] = cur[i];
      __syncthreads();
    }
  }

  // 3. and 4. the core of the tile
  McRun run{0, 0, INT_MAX, INT_MAX, -1, -1};
  const int core = A.band * A.cw * 4;
  for (int it = t; it < core; it += MORPH_THREADS) {
    const int wc = it >> 2, rb = wc / A.cw, cb = wc - rb * A.cw;
    const int r = rb + A.up, c = cb + A.hl;
    const int y = tl.y_org + r, x = (tl.w_org + c) * 64 + (it & 3) * 16;
    if (y >= A.H || x >= A.W) continue;
    const int n = min(16, A.W - x);
    unsigned pb[MC_MAX_PLANES], any = 0, own = 0;
#pragma unroll
    for (int k = 0; k < MC_MAX_PLANES; ++k) {
      pb[k] = k < A.n_planes ? (unsigned)p16[(size_t)k * pw * 4 + (size_t)(r * A.tw + c) * 4 + (it & 3)] : 0u;
      if (n < 16) pb[k] &= (1u << n) - 1u;
      any |= pb[k];
      if (k < A.n_planes && A.out_value[k] < 0) own |= pb[k];
    }
    unsigned iw[4] = {0, 0, 0, 0}, ow[4] = {0, 0, 0, 0};
    if (own) {
      const uint8_t* s = src_frame + (size_t)y * A.W + x;
      if (A.vec_in && n == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(s);
        iw[0] = v.x; iw[1] = v.y; iw[2] = v.z; iw[3] = v.w;
      } else {
        for (int j = 0; j < n; ++j) iw[j >> 2] |= (unsigned)s[j] << (8 * (j & 3));
      }
    }
    if (any) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < MC_MAX_PLANES; ++k)
          if ((pb[k] >> j) & 1u) v = A.out_value[k] < 0 ? mc_byte(iw, j) : (unsigned)A.out_value[k];
        ow[j >> 2] |= v << (8 * (j & 3));
      }
    }
    if (out) {
      uint8_t* d = out + frame + (size_t)y * A.W + x;
      if (A.vec_out && n == 16) *reinterpret_cast<uint4*>(d) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
      else for (int j = 0; j < n; ++j) d[j] = (uint8_t)mc_byte(ow, j);
    }
    if (A.table_classes) {
      if (!any) {
        mc_run_add(run, 0, n, x, x + n - 1, y, tab, A.table_classes);
      } else {
        int j0 = 0;
        for (int j = 1; j <= n; ++j) {
          if (j < n && mc_byte(ow, j) == mc_byte(ow, j0)) continue;
          mc_run_add(run, (int)mc_byte(ow, j0), j - j0, x + j0, x + j - 1, y, tab, A.table_classes);
          j0 = j;
        }
      }
    }
  }
  if (!A.table_classes) return;
  mc_run_flush(run, tab, A.table_classes);
  __syncthreads();
  if (t < A.table_classes && tab[0][t]) {
    int* p = table + ((size_t)blockIdx.z * A.table_classes + t) * MC_TABLE_COLS;
    atomicAdd(p + 0, tab[0][t]);
    atomicMin(reinterpret_cast<unsigned*>(p + 1), (unsigned)tab[1][t]);
    atomicMin(reinterpret_cast<unsigned*>(p + 2), (unsigned)tab[2][t]);
    atomicMax(p + 3, tab[3][t]);
    atomicMax(p + 4, tab[4][t]);
  }
}

// ---- the overlay ----------------------------------------------------------------------------------------------------------------
constexpr int OV_PX = 16;
struct OverlayColors { uint32_t c[256]; };                    // b | g << 8 | r << 16 | has-colour << 24
enum { OV_REGION = 0, OV_WEIGHTED = 1 };

// frames, out uint8 [N,3] and mask uint8 [N] over the N = B * H * W pixels of the batch; one thread per 16 pixels, three
// 16-byte loads and stores when the three pointers are 16-byte aligned (vec) and the 16 pixels exist, bytes otherwise.
//   OV_REGION    mask > 0: uint8(w0 f + w1 c) truncated, c = the value's colour, black without one; else f
//   OV_WEIGHTED  saturate_cast<uchar>(f w0 + p w1), p = the colour where the value has one, else f; rounds to nearest even
// Products and the sum in float32, contraction off.
__global__ void __launch_bounds__(MC_THREADS) overlay_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ mask, size_t N,
                                                            const OverlayColors C, float w0, float w1, int mode, int vec,
                                                            uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ uint32_t col[256];
  col[threadIdx.x] = C.c[threadIdx.x];
  __syncthreads();
  const size_t p0 = ((size_t)blockIdx.x * MC_THREADS + threadIdx.x) * OV_PX;
  if (p0 >= N) return;
  const int n = (int)min((size_t)OV_PX, N - p0);
  const bool wide = vec && n == OV_PX;
  unsigned mw[4] = {0, 0, 0, 0}, fw[12], ow[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) fw[k] = ow[k] = 0;
  const uint8_t* fs = frames + p0 * 3;
  if (wide) {
    const uint4 m = *reinterpret_cast<const uint4*>(mask + p0);
    mw[0] = m.x; mw[1] = m.y; mw[2] = m.z; mw[3] = m.w;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const uint4 v = reinterpret_cast<const uint4*>(fs)[q];
      fw[4 * q] = v.x; fw[4 * q + 1] = v.y; fw[4 * q + 2] = v.z; fw[4 * q + 3] = v.w;
    }
  } else {
    for (int j = 0; j < n; ++j) mw[j >> 2] |= (unsigned)mask[p0 + j] << (8 * (j & 3));
    for (int j = 0; j < 3 * n; ++j) fw[j >> 2] |= (unsigned)fs[j] << (8 * (j & 3));
  }
#pragma unroll
  for (int j = 0; j < OV_PX; ++j) {
    const unsigned m = mc_byte(mw, j);
    const uint32_t cv = col[m];
    const bool has = m != 0 && (cv >> 24) != 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int i = 3 * j + ch;
      const unsigned f = (fw[i >> 2] >> (8 * (i & 3))) & 0xffu;
      unsigned v = f;
      if (mode == OV_REGION) {
        if (m != 0) {
          const float cc = has ? (float)((cv >> (8 * ch)) & 0xffu) : 0.0f;
          const float a = w0 * (float)f, bb = w1 * cc;
          v = (unsigned)(int)(a + bb) & 0xffu;
        }
      } else {
        const float pp = has ? (float)((cv >> (8 * ch)) & 0xffu) : (float)f;
        const float a = (float)f * w0, bb = pp * w1;
        const float s = rintf(a + bb);
        v = (unsigned)(int)fminf(fmaxf(s, 0.0f), 255.0f);
      }
      ow[i >> 2] |= v << (8 * (i & 3));
    }
  }
  uint8_t* d = out + p0 * 3;
  if (wide) {
#pragma unroll
    for (int q = 0; q < 3; ++q) reinterpret_cast<uint4*>(d)[q] = make_uint4(ow[4 * q], ow[4 * q + 1], ow[4 * q + 2], ow[4 * q + 3]);
  } else {
    for (int j = 0; j < 3 * n; ++j) d[j] = (uint8_t)((ow[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

}  // namespace unetpp
