// enhance.h — the grey-frame enhancement in front of the network (preprocess_frame, src/refactor/preprocess.py:12-91):
// the grey / colour decision, BGR -> grey, CLAHE, the gamma table, the bilateral filter and grey -> BGR.
// unet_amd/enhance.py restates the arithmetic in NumPy; every result here equals it bit for bit.
//
// Launch sequence of unetpp_enhance_u8 (no workgroup ever waits for another; every hand-over crosses a kernel boundary;
// nothing returns to the host, the decision byte included):
//   memset                 histograms and channel-difference sums = 0
//   enhance_stats_kernel   one workgroup per 4,096 pixels of one CLAHE tile of the EXTENDED image (the reflected rows and
//                          columns OpenCV appends when the grid does not divide the image count, by reflected
//                          coordinates): grey with gray_of_bgr (edges.h), the grey plane, a histogram per wave in LDS,
//                          one integer atomicAdd per non-empty bin and workgroup, three uint64 atomicAdds of the
//                          |b - g|, |g - r|, |r - b| sums.  Integer sums: the bits do not depend on arrival order.
//   clahe_lut_kernel       one workgroup per tile and frame, one thread per bin: clip, redistribute (closed form of the
//                          residual walk), integer prefix sum, float32 scale and round -> uint8 table.  Tile 0 of every
//                          frame also turns the three sums into the decision byte (one double division).
//   enhance_apply_kernel   one workgroup per 32 x 128 output tile: the tables of the CLAHE tiles its window touches,
//                          the gamma table, the 256 colour weights and the taps -> LDS; CLAHE interpolation + gamma
//                          for the window (tile + halo of `radius`, at reflected global coordinates, so a workgroup
//                          seam inside the image sees no border rule) -> LDS uint8; the bilateral taps from LDS; store.
//                          A frame whose decision byte is 0 is copied through.
//
// Float rules (interpolation and filter): float32, the order written in enhance.py, contraction off, correctly rounded
// division (the compiler's default; no fast-math flag), rounding by __float2int_rn.
//
// LDS of enhance_apply_kernel: window 40 x 136 = 5,440 B, gamma 256 B, colour weights 1,024 B, taps 81 x 6 B, plus the
// dynamic part: 256 B per CLAHE tile the window can touch (EnhApplyArgs::lut_rows x lut_cols; at most the whole 16 x 16
// grid = 64 KB, of 160 KB).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edges.h"

namespace unetpp {

constexpr int EN_THREADS = 256;
constexpr int EN_WAVE = 64;
constexpr int EN_WAVES = EN_THREADS / EN_WAVE;
constexpr int EN_CHUNK = EN_THREADS * 16;      // pixels of one tile a stats workgroup takes
constexpr int EN_MAX_GRID = 16;
constexpr int EN_MAX_R = 4;
constexpr int EN_MAX_TAPS = (2 * EN_MAX_R + 1) * (2 * EN_MAX_R + 1);   // 81
constexpr int EN_TH = 32, EN_TW = 128;         // core tile of the apply kernel
constexpr int EN_WH = EN_TH + 2 * EN_MAX_R, EN_WW = EN_TW + 2 * EN_MAX_R;   // window at the widest radius
constexpr int EN_GROUP = 4;                    // pixels of a row one thread finishes at a time

struct EnhGrid {                               // CLAHE geometry (enhance.clahe_geometry)
  int tiles_x, tiles_y, tw, th;                // tile size of the extended image
  int ext_h, ext_w;                            // extended size (== h, w when the grid divides both)
};

struct EnhTables {                             // host tables, passed by value in the kernel arguments
  float color_w[256];
  float space_w[EN_MAX_TAPS];
  signed char dy[EN_MAX_TAPS], dx[EN_MAX_TAPS];
  unsigned char gamma[256];
  int n_taps, radius;                          // radius 0: no filter
  int has_gamma;
};

struct EnhApplyArgs {
  EnhGrid g;
  int do_clahe;                                // 0: the window is the grey image itself (bilateral alone)
  int lut_rows, lut_cols;                      // CLAHE tiles per side the dynamic LDS has room for
  int cin, cout;                               // channels of the source frames (copy-through) and of the output
  int vec;                                     // w % 4 == 0 and the output is 4-byte aligned
};

// BORDER_REFLECT_101 of an index at most n - 1 outside [0, n)
__device__ __forceinline__ int en_reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}

// max(sums) / n < threshold in double: is_grayscale_frame's comparison (np.mean of exact integers is this division)
__device__ __forceinline__ unsigned char en_decide(const unsigned long long* __restrict__ sums, double n, double threshold) {
  unsigned long long m = sums[0];
  if (sums[1] > m) m = sums[1];
  if (sums[2] > m) m = sums[2];
  return (double)m / n < threshold ? 1 : 0;
}

// grid (chunks of a tile, tiles, B).  src uint8 [B,h,w,cin] (cin 1 or 3) -> gray uint8 [B,h,w] (nullptr: not written),
// hist uint32 [B,tiles,256] (nullptr: none), sums uint64 [B,3] (nullptr: none); hist and sums zeroed by the caller.
__global__ void __launch_bounds__(EN_THREADS) enhance_stats_kernel(const uint8_t* __restrict__ src, int h, int w, int cin, EnhGrid g,
                                                                  uint8_t* __restrict__ gray, unsigned* __restrict__ hist,
                                                                  unsigned long long* __restrict__ sums) {
  __shared__ unsigned s_hist[EN_WAVES][256];
  __shared__ unsigned s_sum[EN_WAVES][3];
  const int t = threadIdx.x, wave = t / EN_WAVE, lane = t % EN_WAVE;
  const int tile = blockIdx.y, b = blockIdx.z;
  const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  const int area = g.tw * g.th;
  for (int i = t; i < EN_WAVES * 256; i += EN_THREADS) (&s_hist[0][0])[i] = 0;
  __syncthreads();
  const size_t frame = (size_t)b * h * w;
  unsigned d0 = 0, d1 = 0, d2 = 0;             // <= 16 * 255 each
  const int i0 = blockIdx.x * EN_CHUNK + t;
  for (int k = 0; k < EN_CHUNK / EN_THREADS; ++k) {
    const int i = i0 + k * EN_THREADS;
    if (i >= area) break;
    const int ry = i / g.tw, rx = i - ry * g.tw;
    const int ye = ty * g.th + ry, xe = tx * g.tw + rx;      // inside the extended image
    const int y = en_reflect(ye, h), x = en_reflect(xe, w);  // inside the image: the extension is at most 16 < h, w
    const size_t p = frame + (size_t)y * w + x;
    int v;
    if (cin == 3) {
      const uint8_t* s = src + p * 3;
      const int bb = s[0], gg = s[1], rr = s[2];
      v = gray_of_bgr(bb, gg, rr);
      if (ye < h && xe < w) { d0 += abs(bb - gg); d1 += abs(gg - rr); d2 += abs(rr - bb); }
    } else {
      v = src[p];
    }
    if (gray && ye < h && xe < w) gray[p] = (uint8_t)v;
    if (hist) atomicAdd(&s_hist[wave][v], 1u);
  }
  if (sums) {
#pragma unroll
    for (int d = EN_WAVE / 2; d > 0; d >>= 1) {
      d0 += __shfl_xor(d0, d, EN_WAVE); d1 += __shfl_xor(d1, d, EN_WAVE); d2 += __shfl_xor(d2, d, EN_WAVE);
    }
    if (lane == 0) { s_sum[wave][0] = d0; s_sum[wave][1] = d1; s_sum[wave][2] = d2; }
  }
  __syncthreads();
  if (hist) {
    const unsigned c = s_hist[0][t] + s_hist[1][t] + s_hist[2][t] + s_hist[3][t];
    if (c) atomicAdd(&hist[((size_t)b * gridDim.y + tile) * 256 + t], c);
  }
  if (sums && t < 3) {
    const unsigned long long s = (unsigned long long)s_sum[0][t] + s_sum[1][t] + s_sum[2][t] + s_sum[3][t];
    if (s) atomicAdd(&sums[(size_t)b * 3 + t], s);
  }
}

// grid (ceil(B / 256)), 256 threads: decisions[b] from sums [B,3] (unetpp_gray_decision; the fused sequence decides in
// clahe_lut_kernel).
__global__ void __launch_bounds__(EN_THREADS) enhance_decide_kernel(const unsigned long long* __restrict__ sums, int batch, double n,
                                                                   double threshold, uint8_t* __restrict__ decisions) {
  const int b = blockIdx.x * EN_THREADS + threadIdx.x;
  if (b < batch) decisions[b] = en_decide(sums + (size_t)b * 3, n, threshold);
}

// grid (tiles, B), 256 threads = one per bin.  hist uint32 [B,tiles,256] -> luts uint8 [B,tiles,256].
// clip 0: no clipping.  decisions (may be nullptr): written by tile 0; `always` != 0 forces 1.
__global__ void __launch_bounds__(EN_THREADS) clahe_lut_kernel(const unsigned* __restrict__ hist, int clip, float lut_scale,
                                                              uint8_t* __restrict__ luts, const unsigned long long* __restrict__ sums,
                                                              double n, double threshold, int always, uint8_t* __restrict__ decisions) {
#pragma clang fp contract(off)
  __shared__ unsigned s_part[2][EN_WAVES];
  const int t = threadIdx.x, wave = t / EN_WAVE, lane = t % EN_WAVE;
  const size_t base = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256;
  unsigned v = hist[base + t];
  if (clip > 0) {
    unsigned excess = v > (unsigned)clip ? v - (unsigned)clip : 0u;
    v = v > (unsigned)clip ? (unsigned)clip : v;
#pragma unroll
    for (int d = EN_WAVE / 2; d > 0; d >>= 1) excess += __shfl_xor(excess, d, EN_WAVE);
    if (lane == 0) s_part[0][wave] = excess;
    __syncthreads();
    const unsigned clipped = s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3];
    const unsigned batch = clipped >> 8, residual = clipped & 255u;
    v += batch;
    if (residual) {                            // the walk `for (i = 0; i < 256 && residual > 0; i += step, --residual) ++bin[i]`
      const unsigned step = 256u / residual;   // >= 1
      if (t % step == 0 && t / step < residual) ++v;
    }
  }
  unsigned c = v;                              // inclusive prefix sum over the 256 bins
#pragma unroll
  for (int d = 1; d < EN_WAVE; d <<= 1) {
    const unsigned o = __shfl_up(c, d, EN_WAVE);
    if (lane >= d) c += o;
  }
  if (lane == EN_WAVE - 1) s_part[1][wave] = c;
  __syncthreads();
  for (int k = 0; k < wave; ++k) c += s_part[1][k];
  int q = __float2int_rn((float)c * lut_scale);
  q = q < 0 ? 0 : (q > 255 ? 255 : q);
  luts[base + t] = (uint8_t)q;
  if (decisions && blockIdx.x == 0 && t == 0)
    decisions[blockIdx.y] = always ? 1 : en_decide(sums + (size_t)blockIdx.y * 3, n, threshold);
}

// (t1, t2, a, a1) of CLAHE_Interpolation_Body for coordinate p: tile size `tile`, `tiles` tiles
__device__ __forceinline__ void en_axis(int p, float inv, int tiles, int* t1, int* t2, float* a, float* a1) {
#pragma clang fp contract(off)
  const float tf = (float)p * inv - 0.5f;
  const float fl = floorf(tf);
  *a = tf - fl;
  *a1 = 1.0f - *a;
  const int i = (int)fl;
  *t1 = i < 0 ? 0 : i;
  *t2 = i + 1 < tiles - 1 ? i + 1 : tiles - 1;
}

// grid (tiles in x, tiles in y, B), dynamic LDS A.lut_rows * A.lut_cols * 256 bytes (0 without CLAHE).
// gray uint8 [B,h,w]; luts uint8 [B,tiles,256]; decisions uint8 [B] (nullptr: every frame is enhanced);
// frames: the source of the copy-through, uint8 [B,h,w,cin]; out uint8 [B,h,w,cout].
__global__ void __launch_bounds__(EN_THREADS) enhance_apply_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ luts,
                                                                  const uint8_t* __restrict__ decisions, const uint8_t* __restrict__ frames,
                                                                  int h, int w, EnhApplyArgs A, EnhTables T, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) uint8_t en_lut[];   // [lny][lnx][256]
  __shared__ uint8_t s_win[EN_WH * EN_WW];     // enhanced window, global (gy0 - r + row, gx0 - r + col), reflected
  __shared__ float s_cw[256];
  __shared__ float s_sw[EN_MAX_TAPS];
  __shared__ short s_off[EN_MAX_TAPS];         // dy * ww + dx
  __shared__ uint8_t s_gamma[256];
  const int t = threadIdx.x;
  const int gy0 = blockIdx.y * EN_TH, gx0 = blockIdx.x * EN_TW, b = blockIdx.z;
  const size_t frame = (size_t)b * h * w;
  const int rows = min(EN_TH, h - gy0), cols = min(EN_TW, w - gx0);     // >= 1: the grid covers the image
  if (decisions && !decisions[b]) {            // uniform: a colour frame is copied through (cin == cout here)
    const int cn = A.cout, n = cols * cn;
    for (int i = t; i < rows * n; i += EN_THREADS) {
      const int ry = i / n, rx = i - ry * n;
      const size_t p = (frame + (size_t)(gy0 + ry) * w + gx0) * cn + rx;
      out[p] = frames[p];
    }
    return;
  }
  const int r = T.radius;
  const int wh = rows + 2 * r, ww = cols + 2 * r;
  // the CLAHE tiles the window touches: its reflected coordinates lie in [lo, hi] on each axis (h, w > r)
  const float inv_tw = 1.0f / (float)A.g.tw, inv_th = 1.0f / (float)A.g.th;
  int ty_lo = 0, tx_lo = 0, lny = 0, lnx = 0;
  if (A.do_clahe) {
    int t1, t2, u1, u2; float a, a1;
    en_axis(max(gy0 - r, 0), inv_th, A.g.tiles_y, &t1, &t2, &a, &a1);
    en_axis(min(gy0 + rows - 1 + r, h - 1), inv_th, A.g.tiles_y, &u1, &u2, &a, &a1);
    ty_lo = t1; lny = min(u2 - t1 + 1, A.lut_rows);
    en_axis(max(gx0 - r, 0), inv_tw, A.g.tiles_x, &t1, &t2, &a, &a1);
    en_axis(min(gx0 + cols - 1 + r, w - 1), inv_tw, A.g.tiles_x, &u1, &u2, &a, &a1);
    tx_lo = t1; lnx = min(u2 - t1 + 1, A.lut_cols);
    const uint8_t* L = luts + (size_t)b * A.g.tiles_x * A.g.tiles_y * 256;
    const int words = lny * lnx * 64;          // 4 bytes at a time: the tables are 256-byte aligned
    for (int i = t; i < words; i += EN_THREADS) {
      const int tl = i >> 6, k = i & 63;
      const int ly = tl / lnx, lx = tl - ly * lnx;
      reinterpret_cast<unsigned*>(en_lut)[i] =
          reinterpret_cast<const unsigned*>(L + ((size_t)(ty_lo + ly) * A.g.tiles_x + tx_lo + lx) * 256)[k];
    }
  }
  s_cw[t] = T.color_w[t];
  s_gamma[t] = T.gamma[t];
  if (t < T.n_taps) { s_sw[t] = T.space_w[t]; s_off[t] = (short)((int)T.dy[t] * ww + (int)T.dx[t]); }
  __syncthreads();
  const uint8_t* gsrc = gray + frame;
  for (int i = t; i < wh * ww; i += EN_THREADS) {
    const int ry = i / ww, rx = i - ry * ww;
    const int y = en_reflect(gy0 - r + ry, h), x = en_reflect(gx0 - r + rx, w);   // rows, cols end inside the image: in range
    int v = gsrc[(size_t)y * w + x];
    if (A.do_clahe) {
      int y1, y2, x1, x2; float ya, ya1, xa, xa1;
      en_axis(y, inv_th, A.g.tiles_y, &y1, &y2, &ya, &ya1);
      en_axis(x, inv_tw, A.g.tiles_x, &x1, &x2, &xa, &xa1);
      y1 = min(max(y1 - ty_lo, 0), lny - 1); y2 = min(max(y2 - ty_lo, 0), lny - 1);   // no-ops: see lut_rows / lut_cols
      x1 = min(max(x1 - tx_lo, 0), lnx - 1); x2 = min(max(x2 - tx_lo, 0), lnx - 1);
      const float l11 = (float)en_lut[(y1 * lnx + x1) * 256 + v], l12 = (float)en_lut[(y1 * lnx + x2) * 256 + v];
      const float l21 = (float)en_lut[(y2 * lnx + x1) * 256 + v], l22 = (float)en_lut[(y2 * lnx + x2) * 256 + v];
      const float res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
      v = __float2int_rn(res);
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
    if (T.has_gamma) v = s_gamma[v];
    s_win[i] = (uint8_t)v;
  }
  __syncthreads();
  // groups of 4 pixels of a row; consecutive threads take consecutive groups
  const int gpr = (cols + EN_GROUP - 1) / EN_GROUP;
  for (int gi = t; gi < rows * gpr; gi += EN_THREADS) {
    const int ry = gi / gpr, cx = (gi - ry * gpr) * EN_GROUP;
    const int npx = min(EN_GROUP, cols - cx);
    unsigned px[EN_GROUP] = {0, 0, 0, 0};
    for (int j = 0; j < npx; ++j) {
      const uint8_t* c = s_win + (ry + r) * ww + cx + j + r;
      int q = c[0];
      if (r) {
        float sum = 0.0f, wsum = 0.0f;
        const int v0 = q;
        for (int k = 0; k < T.n_taps; ++k) {
          const int val = c[s_off[k]];
          const float wgt = s_sw[k] * s_cw[abs(val - v0)];
          sum = sum + (float)val * wgt;
          wsum = wsum + wgt;
        }
        q = __float2int_rn(sum / wsum);
        q = q < 0 ? 0 : (q > 255 ? 255 : q);
      }
      px[j] = (unsigned)q;
    }
    const size_t p = frame + (size_t)(gy0 + ry) * w + gx0 + cx;
    if (A.cout == 1) {
      if (A.vec && npx == EN_GROUP) {
        *reinterpret_cast<unsigned*>(out + p) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
      } else {
        for (int j = 0; j < npx; ++j) out[p + j] = (uint8_t)px[j];
      }
    } else {
      uint8_t* o = out + p * 3;
      if (A.vec && npx == EN_GROUP) {          // 12 bytes: three words
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
        o4[0] = px[0] * 0x010101u | (px[1] << 24);
        o4[1] = px[1] * 0x0101u | (px[2] * 0x0101u << 16);
        o4[2] = px[2] | (px[3] * 0x010101u << 8);
      } else {
        for (int j = 0; j < npx; ++j) { o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = (uint8_t)px[j]; }
      }
    }
  }
}

}  // namespace unetpp
