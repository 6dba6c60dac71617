// nlmeans.h — cv2.fastNlMeansDenoising(img, None, h, 7, 21) for one 8-bit channel: the 'fastNlMeans' denoiser of
// enhance_grayscale_frame (src/refactor/preprocess.py:68-69).  unet_amd/nlmeans.py restates OpenCV's published
// FastNlMeansDenoisingInvoker<uchar, int, unsigned, DistSquared, int> in NumPy; every result here equals it bit for bit.
// All arithmetic is integer, so the order of the sums is free.
//
// One launch for the whole batch, grid (tiles in x, tiles in y, B), 256 threads.  A workgroup owns 128 rows x 64 columns of
// output.  It stages in LDS, as bytes, that tile plus a halo of 13 = 3 + 10 pixels of channel 0 of the source, at
// BORDER_REFLECT_101 coordinates (so a workgroup seam inside the image sees no border rule and the loops below have no
// bounds checks), and the non-zero prefix of the weight table (uint16; at most 8,192 entries) followed by one 0.
//
// Sharing of the patch distances.  A thread owns 8 rows x 4 columns of pixels.  Their 7 x 7 patches lie in 14 rows x 10
// columns around them; that part of the centre window stays in registers for all 441 offsets (14 x 3 words).  Per offset
// (dy, dx) the thread reads the 14 x 10 bytes of the shifted window from LDS and takes the 140 differences once; per row the
// four 7-term sums of squares share their common terms (13 multiply-adds for the 4 columns); down the columns the 7-row sum
// slides (one addition and one subtraction per pixel): 14 x 13 / 32 = 5.7 multiply-adds per pixel and offset instead of 49.
// Then per pixel
//   w = table[min(D >> 6, n)] (slot n holds 0: an index past the prefix costs no second test),
//   est += w * shifted centre value, wsum += w            (uint32: est reaches 2,147,440,680 on a constant 255 image)
// and at the end out = (est + wsum / 2) / wsum, unsigned.  The centre offset has D = 0, so wsum >= table[0] > 0.
//
// LDS: window 154 rows x 104 bytes = 16,016 B (90 used per row; a row starts 2 bytes in so that every thread's register
// copy is word aligned; the row stride of 104 puts the 2 x 16 threads of one LDS lane group on 32 different banks), table
// (8,192 + 2) x 2 = 16,388 B: 32,404 B per workgroup, so LDS alone would allow 5 workgroups on a CU's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unetpp {

constexpr int NLM_T = 7, NLM_S = 21;                       // template and search window: the only sizes the reference uses
constexpr int NLM_TH = NLM_T / 2, NLM_SH = NLM_S / 2, NLM_BORDER = NLM_TH + NLM_SH;      // 3, 10, 13
constexpr int NLM_SHIFT = 6;                               // 2^6 >= 49
constexpr int NLM_MAX_WEIGHTS = 8192;                      // longest non-zero prefix of the table (h up to about 39)
constexpr int NLM_MIN_SIDE = NLM_BORDER + 1;               // the border never reflects twice
constexpr int NLM_THREADS = 256;
constexpr int NLM_PY = 8, NLM_PX = 4;                      // pixels of one thread
constexpr int NLM_GY = 16, NLM_GX = 16;                    // threads of a workgroup
constexpr int NLM_TILE_H = NLM_GY * NLM_PY, NLM_TILE_W = NLM_GX * NLM_PX;              // 128 x 64
constexpr int NLM_WIN_H = NLM_TILE_H + 2 * NLM_BORDER, NLM_WIN_W = NLM_TILE_W + 2 * NLM_BORDER;   // 154 x 90
constexpr int NLM_PAD = 2;                                 // (NLM_PAD + NLM_SH) % 4 == 0
constexpr int NLM_STRIDE = 104;                            // >= NLM_PAD + NLM_WIN_W, % 4 == 0, 2 * stride % 32 == 16
constexpr int NLM_AH = NLM_PY + 2 * NLM_TH, NLM_AW = NLM_PX + 2 * NLM_TH;              // 14 x 10: what a thread's patches cover
constexpr int NLM_AWORDS = (NLM_AW + 3) / 4;
static_assert(NLM_THREADS == NLM_GY * NLM_GX && (NLM_PAD + NLM_SH) % 4 == 0 && NLM_STRIDE % 4 == 0, "layout");
static_assert(NLM_STRIDE >= NLM_PAD + NLM_SH + (NLM_GX - 1) * NLM_PX + 4 * NLM_AWORDS, "the register copy stays inside its row");
static_assert((1 << NLM_SHIFT) >= NLM_T * NLM_T && (1 << (NLM_SHIFT - 1)) < NLM_T * NLM_T, "shift");

// BORDER_REFLECT_101 of an index at most n - 1 outside [0, n)
__device__ __forceinline__ int nlm_reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}

// src uint8 [B,h,w,cin], channel 0 is filtered; out uint8 [B,h,w,cout], the result replicated.  h, w >= 14.
// decisions uint8 [B] or nullptr: a frame with 0 is copied through (cin == cout then).  weights uint16 [n_w], 1 <= n_w <= 8192.
// vec: w % 4 == 0 and out is 4-byte aligned.
__global__ void __launch_bounds__(NLM_THREADS) nlmeans_kernel(const uint8_t* __restrict__ src, int h, int w, int cin, int cout,
                                                             const uint8_t* __restrict__ decisions, const uint16_t* __restrict__ weights,
                                                             int n_w, int vec, uint8_t* __restrict__ out) {
  __shared__ __align__(16) uint8_t s_win[NLM_WIN_H * NLM_STRIDE];
  __shared__ uint16_t s_w[NLM_MAX_WEIGHTS + 2];
  const int t = threadIdx.x;
  const int gy0 = blockIdx.y * NLM_TILE_H, gx0 = blockIdx.x * NLM_TILE_W, b = blockIdx.z;
  const size_t frame = (size_t)b * h * w;
  const int rows = min(NLM_TILE_H, h - gy0), cols = min(NLM_TILE_W, w - gx0);       // >= 1: the grid covers the image
  if (decisions && !decisions[b]) {            // uniform: the frame is copied through, every channel
    const int n = cols * cout;
    for (int i = t; i < rows * n; i += NLM_THREADS) {
      const int ry = i / n, rx = i - ry * n;
      const size_t p = (frame + (size_t)(gy0 + ry) * w + gx0) * cout + rx;
      out[p] = src[p];
    }
    return;
  }
  for (int i = t; i <= n_w; i += NLM_THREADS) s_w[i] = i < n_w ? weights[i] : (uint16_t)0;
  // the window rows and columns the pixels inside the image read: global (gy0 - 13 + ry, gx0 - 13 + rx), reflected; the
  // last of them lies 13 past the image at most, and h, w >= 14
  const int wh = rows + 2 * NLM_BORDER, ww = cols + 2 * NLM_BORDER;
  for (int i = t; i < wh * ww; i += NLM_THREADS) {
    const int ry = i / ww, rx = i - ry * ww;
    const int y = nlm_reflect(gy0 - NLM_BORDER + ry, h), x = nlm_reflect(gx0 - NLM_BORDER + rx, w);
    s_win[ry * NLM_STRIDE + NLM_PAD + rx] = src[(frame + (size_t)y * w + x) * cin];
  }
  __syncthreads();
  const int tx = t % NLM_GX, ty = t / NLM_GX;
  const int py0 = ty * NLM_PY, px0 = tx * NLM_PX;
  if (py0 >= rows || px0 >= cols) return;      // no barrier follows
  // the thread's 14 x 10 part of the centre window: window rows py0 + 10 .., columns px0 + 10 ..
  const uint8_t* pa = s_win + (py0 + NLM_SH) * NLM_STRIDE + NLM_PAD + NLM_SH + px0;
  unsigned a[NLM_AH][NLM_AWORDS];
#pragma unroll
  for (int r = 0; r < NLM_AH; ++r)
#pragma unroll
    for (int j = 0; j < NLM_AWORDS; ++j) a[r][j] = reinterpret_cast<const unsigned*>(pa + r * NLM_STRIDE)[j];
  unsigned est[NLM_PY][NLM_PX], wsum[NLM_PY][NLM_PX];
#pragma unroll
  for (int o = 0; o < NLM_PY; ++o)
#pragma unroll
    for (int c = 0; c < NLM_PX; ++c) est[o][c] = wsum[o][c] = 0u;

#pragma unroll 1
  for (int dy = -NLM_SH; dy <= NLM_SH; ++dy) {
#pragma unroll 1
    for (int dx = -NLM_SH; dx <= NLM_SH; ++dx) {
      const uint8_t* pb = pa + dy * NLM_STRIDE + dx;           // rows 0 .. 153 and columns 0 .. 89 of the window: see the header
      int rs[NLM_AH][NLM_PX];                                  // 7-term row sums; a row is dead 7 rows later
      unsigned centre[NLM_PY][NLM_PX];
      int D[NLM_PX] = {0, 0, 0, 0};
      int idx[NLM_PY][NLM_PX];                                 // D >> 6, at most n_w (that slot holds 0)
#pragma unroll
      for (int r = 0; r < NLM_AH; ++r) {
#pragma unroll
        for (int j = 0; j < NLM_AWORDS; ++j) asm volatile("" : "+v"(a[r][j]));   // keeps the 140 byte extractions from being hoisted into registers
        int d[NLM_AW];
#pragma unroll
        for (int k = 0; k < NLM_AW; ++k) {
          const int bv = pb[r * NLM_STRIDE + k];
          d[k] = (int)((a[r][k >> 2] >> (8 * (k & 3))) & 255u) - bv;
          if (r >= NLM_TH && r < NLM_TH + NLM_PY && k >= NLM_TH && k < NLM_TH + NLM_PX) centre[r - NLM_TH][k - NLM_TH] = (unsigned)bv;
        }
        // the four 7-term sums of squares over d[c .. c + 6] as 13 multiply-adds: they share d[3..6], then d[2], d[1] / d[7], d[8]
        static_assert(NLM_PX == 4 && NLM_T == 7, "the sharing below is written for four columns of 7 terms");
        const int m = d[6] * d[6] + (d[5] * d[5] + (d[4] * d[4] + d[3] * d[3]));
        const int m2 = d[2] * d[2] + m, m12 = d[1] * d[1] + m2;
        const int m7 = d[7] * d[7] + m, m78 = d[8] * d[8] + m7;
        rs[r][0] = d[0] * d[0] + m12;
        rs[r][1] = d[7] * d[7] + m12;
        rs[r][2] = d[8] * d[8] + (d[7] * d[7] + m2);
        rs[r][3] = d[9] * d[9] + m78;
#pragma unroll
        for (int c = 0; c < NLM_PX; ++c) {
          D[c] += rs[r][c];
          if (r >= NLM_T) D[c] -= rs[r - NLM_T][c];
        }
        if (r >= NLM_T - 1) {                                  // the patches of pixel row r - 6 are complete
#pragma unroll
          for (int c = 0; c < NLM_PX; ++c) idx[r - (NLM_T - 1)][c] = min(D[c] >> NLM_SHIFT, n_w);
        }
      }
      // the 32 table reads together, after the distances: one wait for them instead of one per pixel row
      unsigned wgt[NLM_PY][NLM_PX];
#pragma unroll
      for (int o = 0; o < NLM_PY; ++o)
#pragma unroll
        for (int c = 0; c < NLM_PX; ++c) wgt[o][c] = s_w[idx[o][c]];
#pragma unroll
      for (int o = 0; o < NLM_PY; ++o)
#pragma unroll
        for (int c = 0; c < NLM_PX; ++c) {
          est[o][c] += wgt[o][c] * centre[o][c];
          wsum[o][c] += wgt[o][c];
        }
    }
  }

#pragma unroll
  for (int o = 0; o < NLM_PY; ++o) {
    if (py0 + o >= rows) break;
    unsigned px[NLM_PX];
#pragma unroll
    for (int c = 0; c < NLM_PX; ++c) px[c] = (est[o][c] + wsum[o][c] / 2u) / wsum[o][c];
    const int npx = min(NLM_PX, cols - px0);
    const size_t p = frame + (size_t)(gy0 + py0 + o) * w + gx0 + px0;
    if (cout == 1) {
      if (vec && npx == NLM_PX) {
        *reinterpret_cast<unsigned*>(out + p) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
      } else {
#pragma unroll
        for (int c = 0; c < NLM_PX; ++c) if (c < npx) out[p + c] = (uint8_t)px[c];
      }
    } else {
      uint8_t* q = out + p * 3;
      if (vec && npx == NLM_PX) {                              // 12 bytes: three words
        unsigned* q4 = reinterpret_cast<unsigned*>(q);
        q4[0] = px[0] * 0x010101u | (px[1] << 24);
        q4[1] = px[1] * 0x0101u | (px[2] * 0x0101u << 16);
        q4[2] = px[2] | (px[3] * 0x010101u << 8);
      } else {
#pragma unroll
        for (int c = 0; c < NLM_PX; ++c) if (c < npx) { q[3 * c] = q[3 * c + 1] = q[3 * c + 2] = (uint8_t)px[c]; }
      }
    }
  }
}

}  // namespace unetpp
