// raw_frames.h — raw camera frames on the device (include/unetpp_raw.h; unet_amd/raw_frames.py holds the NumPy forms):
//   rf_to_bgr_kernel   the Bayer demosaic of GigECameraHarvester._to_bgr (src/camera/gige_harvester.py:101-114): one byte per
//                      pixel in, the BGR frame and / or its grey conversion out
//   rf_resize_kernel   the same demosaic fused into the resize of preprocess_image (infer_two_stage_burr.py:122-127): from the raw
//                      bytes to the network's uint8 input, demosaicing only the taps the resize reads
// Everything is integer: OpenCV's bilinear Bayer2RGB_<uchar>, its 15-bit BGR2GRAY and its 11-bit fixed-point INTER_LINEAR.
//
// Arithmetic
//   interior pixel  (1 <= y <= H - 2, 1 <= x <= W - 2) a measured channel is the raw byte; at a red or blue site green is
//                   (N + S + W + E + 2) >> 2 and the opposite colour (NW + NE + SW + SE + 2) >> 2; at a green site the colour that
//                   shares the row is (W + E + 1) >> 1 and the other (N + S + 1) >> 1
//   border          out[y, x] = interior[clamp(y, 1, H - 2), clamp(x, 1, W - 2)]
//   sites           the red site's (row parity, column parity) is the kernels' (RY, RX); blue is the opposite corner of the cell
//   mono            (v, v, v), no border rule
//   grey            (3735 B + 19235 G + 9798 R + 16384) >> 15
//   resize          roi_linear_coef of roi_loop.h per axis; horizontal pass p0 a0 + p1 a1 in int32, vertical pass
//                   (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "roi_loop.h"

namespace unetpp {

constexpr int RF_THREADS = 256;
constexpr int RF_TW = 128, RF_TH = 16;                 // rf_to_bgr_kernel's tile: 32 x 8 threads of 4 x 2 pixels (two Bayer cells) each
constexpr int RF_RAW_X = 16;                           // the byte of a staged raw row that holds column x0; column x0 - 1 lies at 15
constexpr int RF_RAW_STRIDE = RF_RAW_X + RF_TW + 16;   // 160: every 16-byte chunk of a row lands on a 16-byte slot
constexpr int RF_BGR_STRIDE = 392;                     // (RF_TW + 1) * 3 = 387 bytes and the 4 rf_store_row may read past them, in dwords
constexpr int RF_GRAY_STRIDE = 136;                    // RF_TW + 1 = 129 bytes, likewise
constexpr int RF_OTW = 32, RF_OTH = 32;                // rf_resize_kernel's output tile: 32 x 8 threads, four rows each
constexpr int RF_OUT_STRIDE = RF_OTW * 3 + 4;
constexpr int RF_RECT_BYTES = 16384;                   // the staged source rectangle of one output tile; a larger one is read in place

struct RfPx { int b, g, r; };

// One pixel from its 3 x 3 raw neighbourhood.  red_row: the pixel's row holds red sites; red_col: its column does.
__device__ __forceinline__ RfPx rf_demosaic(int nw, int n, int ne, int w, int c, int e, int sw, int s, int se, bool red_row, bool red_col, bool mono) {
  RfPx o;
  if (mono) {
    o.b = o.g = o.r = c;
  } else if (red_row == red_col) {                       // a red or a blue site
    const int cross = (n + s + w + e + 2) >> 2, diag = (nw + ne + sw + se + 2) >> 2;
    o.g = cross;
    o.r = red_row ? c : diag;
    o.b = red_row ? diag : c;
  } else {                                               // a green site
    const int hor = (w + e + 1) >> 1, ver = (n + s + 1) >> 1;
    o.g = c;
    o.r = red_row ? hor : ver;
    o.b = red_row ? ver : hor;
  }
  return o;
}

__device__ __forceinline__ int rf_gray(const RfPx& p) { return (3735 * p.b + 19235 * p.g + 9798 * p.r + 16384) >> 15; }

// n bytes of an LDS row (4-byte aligned, readable up to n + 3) to dst at ANY alignment, by the `nl` lanes of which this is lane l:
// the 16-byte chunks are cut where dst's address is a multiple of 16, so every chunk that lies wholly inside the row goes out as
// one 16-byte store whatever the pointer is, and only the row's first and last bytes are stored one by one.
__device__ __forceinline__ void rf_store_row(const uint8_t* __restrict__ srow, int n, uint8_t* __restrict__ dst, int l, int nl) {
  const int s = (int)((uintptr_t)dst & 15u);
  const int nchunk = (s + n + 15) >> 4;
  for (int c = l; c < nchunk; c += nl) {
    const int i0 = 16 * c - s;                             // the row byte the chunk starts with
    if (i0 >= 0 && i0 + 16 <= n) {
      const unsigned* w = reinterpret_cast<const unsigned*>(srow + (i0 & ~3));
      const int sh = 8 * (i0 & 3);
      unsigned v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (unsigned)((((unsigned long long)w[k + 1] << 32) | w[k]) >> sh);
      *reinterpret_cast<uint4*>(dst + i0) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
      for (int j = 0; j < 16; ++j) {
        const int i = i0 + j;
        if (i >= 0 && i < n) dst[i] = srow[i];
      }
    }
  }
}

// ---- 1. raw -> BGR and / or grey -----------------------------------------------------------------------------------------------
// Grid (tiles in x, tiles in y, B).  A Bayer frame has ceil((W - 1) / 128) x ceil((H - 1) / 16) tiles: where W - 1 (H - 1) is a
// multiple of the tile, the last tile also stores column W - 1 (row H - 1), which is a copy of its neighbour, so the pixel a
// border pixel copies always lies in the same tile.  A mono frame has ceil(W / 128) x ceil(H / 16) tiles and no border rule.
//   1. the tile's raw rows and a one-pixel halo go to LDS, coordinates clamped to the frame: 16-byte loads where vec_in says the
//      pointer and both strides are multiples of 16 and the chunk lies inside the row, bytes elsewhere; the LDS holds the same
//      bytes either way
//   2. every thread demosaics a 4 x 2 block that starts on an even row and column, so each pixel's site kind is a constant of its
//      place in the block; BGR and grey go to LDS (only interior pixels are read from there afterwards)
//   3. in tiles on the frame's border the copied columns, then the copied rows, are filled in LDS
//   4. the rows go out through rf_store_row
template <int RY, int RX, bool MONO>
__global__ void __launch_bounds__(RF_THREADS) rf_to_bgr_kernel(const uint8_t* __restrict__ raw, long long row_stride, long long frame_stride, int H, int W,
                                                              int vec_in, uint8_t* __restrict__ bgr, uint8_t* __restrict__ gray) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[(RF_TH + 2) * RF_RAW_STRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t s_bgr[(RF_TH + 1) * RF_BGR_STRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t s_gray[(RF_TH + 1) * RF_GRAY_STRIDE];
  const int t = threadIdx.x, x0 = blockIdx.x * RF_TW, y0 = blockIdx.y * RF_TH, f = blockIdx.z;
  const uint8_t* src = raw + (long long)f * frame_stride;

  constexpr int CHUNKS = (RF_TH + 2) * (RF_TW / 16), HALO = 2 * (RF_TH + 2);
  static_assert(CHUNKS + HALO <= RF_THREADS, "one staging task per thread");
  if (t < CHUNKS) {
    const int ly = t / (RF_TW / 16), c = t % (RF_TW / 16);
    const int y = min(max(y0 - 1 + ly, 0), H - 1), x = x0 + 16 * c;
    const uint8_t* row = src + (long long)y * row_stride;
    uint4 v;
    if (vec_in && x + 16 <= W) {
      v = *reinterpret_cast<const uint4*>(row + x);
    } else {
      unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j >> 2] |= (unsigned)row[min(x + j, W - 1)] << (8 * (j & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(s_raw + ly * RF_RAW_STRIDE + RF_RAW_X + 16 * c) = v;
  } else if (t < CHUNKS + HALO) {
    const int ly = (t - CHUNKS) >> 1, east = (t - CHUNKS) & 1;
    const int y = min(max(y0 - 1 + ly, 0), H - 1), x = east ? min(x0 + RF_TW, W - 1) : max(x0 - 1, 0);
    s_raw[ly * RF_RAW_STRIDE + (east ? RF_RAW_X + RF_TW : RF_RAW_X - 1)] = src[(long long)y * row_stride + x];
  }
  __syncthreads();

  {
    const int tx = t & 31, ty = t >> 5;
    int v[4][6];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned* p = reinterpret_cast<const unsigned*>(s_raw + (2 * ty + r) * RF_RAW_STRIDE + RF_RAW_X - 4 + 4 * tx);
      const unsigned d0 = p[0], d1 = p[1], d2 = p[2];
      v[r][0] = (int)(d0 >> 24);
      v[r][1] = (int)(d1 & 255u); v[r][2] = (int)((d1 >> 8) & 255u); v[r][3] = (int)((d1 >> 16) & 255u); v[r][4] = (int)(d1 >> 24);
      v[r][5] = (int)(d2 & 255u);
    }
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      unsigned wb[3] = {0u, 0u, 0u}, wg = 0u;
#pragma unroll
      for (int pc = 0; pc < 4; ++pc) {
        const RfPx px = rf_demosaic(v[pr][pc], v[pr][pc + 1], v[pr][pc + 2], v[pr + 1][pc], v[pr + 1][pc + 1], v[pr + 1][pc + 2], v[pr + 2][pc],
                                    v[pr + 2][pc + 1], v[pr + 2][pc + 2], pr == RY, (pc & 1) == RX, MONO);
        wb[(3 * pc) >> 2] |= (unsigned)px.b << (8 * ((3 * pc) & 3));
        wb[(3 * pc + 1) >> 2] |= (unsigned)px.g << (8 * ((3 * pc + 1) & 3));
        wb[(3 * pc + 2) >> 2] |= (unsigned)px.r << (8 * ((3 * pc + 2) & 3));
        wg |= (unsigned)rf_gray(px) << (8 * pc);
      }
      if (bgr) {
        unsigned* o = reinterpret_cast<unsigned*>(s_bgr + (2 * ty + pr) * RF_BGR_STRIDE + 12 * tx);
        o[0] = wb[0]; o[1] = wb[1]; o[2] = wb[2];
      }
      if (gray) *reinterpret_cast<unsigned*>(s_gray + (2 * ty + pr) * RF_GRAY_STRIDE + 4 * tx) = wg;
    }
  }
  __syncthreads();

  int nx = min(RF_TW, W - x0), ny = min(RF_TH, H - y0);
  if (!MONO) {
    if (W - x0 == RF_TW + 1) nx = RF_TW + 1;
    if (H - y0 == RF_TH + 1) ny = RF_TH + 1;
    const bool left = x0 == 0, right = x0 + nx == W, top = y0 == 0, bottom = y0 + ny == H;      // the same in every thread
    if (left || right) {
      const int xr = W - 1 - x0;                           // >= 1: the last tile starts at or before column W - 2
      if (t < RF_TH) {
        uint8_t* pb = s_bgr + t * RF_BGR_STRIDE;
        uint8_t* pg = s_gray + t * RF_GRAY_STRIDE;
        if (left) {
          if (bgr) { pb[0] = pb[3]; pb[1] = pb[4]; pb[2] = pb[5]; }
          if (gray) pg[0] = pg[1];
        }
        if (right) {
          if (bgr) { pb[3 * xr] = pb[3 * xr - 3]; pb[3 * xr + 1] = pb[3 * xr - 2]; pb[3 * xr + 2] = pb[3 * xr - 1]; }
          if (gray) pg[xr] = pg[xr - 1];
        }
      }
      __syncthreads();
    }
    if (top || bottom) {
      const int yb = H - 1 - y0;                           // >= 1, likewise
      for (int i = t; i < 3 * nx; i += RF_THREADS) {
        if (bgr && top) s_bgr[i] = s_bgr[RF_BGR_STRIDE + i];
        if (bgr && bottom) s_bgr[yb * RF_BGR_STRIDE + i] = s_bgr[(yb - 1) * RF_BGR_STRIDE + i];
      }
      for (int i = t; i < nx; i += RF_THREADS) {
        if (gray && top) s_gray[i] = s_gray[RF_GRAY_STRIDE + i];
        if (gray && bottom) s_gray[yb * RF_GRAY_STRIDE + i] = s_gray[(yb - 1) * RF_GRAY_STRIDE + i];
      }
      __syncthreads();
    }
  }

  const int sub = t >> 5, l = t & 31;
  for (int r = sub; r < ny; r += RF_THREADS / 32) {
    const size_t at = ((size_t)f * H + (size_t)(y0 + r)) * W + x0;
    if (bgr) rf_store_row(s_bgr + r * RF_BGR_STRIDE, 3 * nx, bgr + 3 * at, l, 32);
    if (gray) rf_store_row(s_gray + r * RF_GRAY_STRIDE, nx, gray + at, l, 32);
  }
}

// ---- 2. raw -> crop -> resize, the BGR frame never written ------------------------------------------------------------------------
// out uint8 [B,OH,OW,3] = the INTER_LINEAR resize to OW x OH of the crop [cy0, cy0 + CH) x [cx0, cx0 + CW) of the demosaiced frame.
// Grid (ceil(OW / 32), ceil(OH / 32), B); thread (tx, ty) of 32 x 8 computes column tx of rows ty, ty + 8, ty + 16, ty + 24 of the
// tile.  An output pixel reads two source columns X0 <= X1 <= X0 + 1 and two rows likewise; demosaiced pixel (Y, X) is the interior
// pixel (clamp(Y, 1, H - 2), clamp(X, 1, W - 2)), so the four taps lie in the 4 x 4 raw block whose second row and column are the
// clamped (Y0, X0).  The coefficients are monotone in the output index, so the tile's first and last pixel bound the raw rectangle
// all its blocks lie in.  The workgroup forms the tile's 32 + 32 coefficient sets once (roi_linear_coef, no host table: a double
// division apiece), stages that rectangle in LDS once (when it fits RF_RECT_BYTES; a steeper reduction reads its taps in place),
// and every thread demosaics the four taps of each of its pixels at their own site kinds and runs the two fixed-point passes.  The
// rows go out through rf_store_row.  The tile is this large because a workgroup is one chain of latencies (coefficients, barrier,
// the rectangle's loads, barrier, taps, barrier, stores): 32 x 8 tiles spent most of their time waiting in it.
__global__ void __launch_bounds__(RF_THREADS) rf_resize_kernel(const uint8_t* __restrict__ raw, long long row_stride, long long frame_stride, int H, int W,
                                                              int ry, int rx, int mono, int cx0, int cy0, int CW, int CH, int OH, int OW,
                                                              uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_rect[RF_RECT_BYTES];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[RF_OTH * RF_OUT_STRIDE];
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
  const int ox0 = blockIdx.x * RF_OTW, oy0 = blockIdx.y * RF_OTH, f = blockIdx.z;
  const int nx = min(RF_OTW, OW - ox0), ny = min(RF_OTH, OH - oy0);
  const uint8_t* src = raw + (long long)f * frame_stride;
  const int lo = mono ? 0 : 1;                               // the stencil's centres lie in [lo, n - 1 - lo]

  // the coefficients of the tile's columns and rows, formed once each; an index past the output's edge repeats the last one.
  // The first and the last of them bound the tile's rectangle.
  __shared__ RoiCoef s_cx[RF_OTW], s_cy[RF_OTH];
  if (t < RF_OTW) s_cx[t] = roi_linear_coef(min(ox0 + t, OW - 1), CW, OW);
  else if (t < RF_OTW + RF_OTH) s_cy[t - RF_OTW] = roi_linear_coef(min(oy0 + t - RF_OTW, OH - 1), CH, OH);
  __syncthreads();
  const int col_lo = max(min(max(cx0 + s_cx[0].s0, lo), W - 1 - lo) - 1, 0);
  const int col_hi = min(min(max(cx0 + s_cx[nx - 1].s0, lo), W - 1 - lo) + 2, W - 1);
  const int row_lo = max(min(max(cy0 + s_cy[0].s0, lo), H - 1 - lo) - 1, 0);
  const int row_hi = min(min(max(cy0 + s_cy[ny - 1].s0, lo), H - 1 - lo) + 2, H - 1);
  const int nc = col_hi - col_lo + 1, nr = row_hi - row_lo + 1, stride = (nc + 3) & ~3;
  const bool staged = (long long)nr * stride <= RF_RECT_BYTES;
  if (staged) {
    for (int r = t >> 6; r < nr; r += RF_THREADS / 64) {
      const uint8_t* row = src + (long long)(row_lo + r) * row_stride + col_lo;
      for (int c = t & 63; c < nc; c += 64) s_rect[r * stride + c] = row[c];
    }
  }
  __syncthreads();

  if (tx < nx) {
    const RoiCoef cx = s_cx[tx];
    const int X0 = min(max(cx0 + cx.s0, lo), W - 1 - lo), X1 = min(max(cx0 + cx.s1, lo), W - 1 - lo);
    const bool dx = X1 != X0, red_col0 = (X0 & 1) == rx;
    int xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = min(max(X0 - 1 + j, col_lo), col_hi);      // a clamped row or column is one no tap's stencil reads
    for (int oy = ty; oy < ny; oy += RF_THREADS / RF_OTW) {
      const RoiCoef cy = s_cy[oy];
      const int Y0 = min(max(cy0 + cy.s0, lo), H - 1 - lo), Y1 = min(max(cy0 + cy.s1, lo), H - 1 - lo);
      int n[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int y = min(max(Y0 - 1 + i, row_lo), row_hi);
        if (staged) {
          const uint8_t* p = s_rect + (y - row_lo) * stride;
#pragma unroll
          for (int j = 0; j < 4; ++j) n[i][j] = (int)p[xs[j] - col_lo];
        } else {
          const uint8_t* p = src + (long long)y * row_stride;
#pragma unroll
          for (int j = 0; j < 4; ++j) n[i][j] = (int)p[xs[j]];
        }
      }
      RfPx d[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          d[a][b] = rf_demosaic(n[a][b], n[a][b + 1], n[a][b + 2], n[a + 1][b], n[a + 1][b + 1], n[a + 1][b + 2], n[a + 2][b], n[a + 2][b + 1],
                                n[a + 2][b + 2], ((Y0 + a) & 1) == ry, red_col0 != (b != 0), mono != 0);
      const bool dy = Y1 != Y0;
      const RfPx t00 = d[0][0], t01 = dx ? d[0][1] : d[0][0], t10 = dy ? d[1][0] : d[0][0];
      const RfPx t11 = dy ? (dx ? d[1][1] : d[1][0]) : t01;
      const int p00[3] = {t00.b, t00.g, t00.r}, p01[3] = {t01.b, t01.g, t01.r}, p10[3] = {t10.b, t10.g, t10.r}, p11[3] = {t11.b, t11.g, t11.r};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int S0 = p00[c] * cx.a0 + p01[c] * cx.a1, S1 = p10[c] * cx.a0 + p11[c] * cx.a1;
        const int v = (((cy.a0 * (S0 >> 4)) >> 16) + ((cy.a1 * (S1 >> 4)) >> 16) + 2) >> 2;
        s_out[oy * RF_OUT_STRIDE + 3 * tx + c] = (uint8_t)min(max(v, 0), 255);
      }
    }
  }
  __syncthreads();

  for (int r = ty; r < ny; r += RF_THREADS / RF_OTW)
    rf_store_row(s_out + r * RF_OUT_STRIDE, 3 * nx, out + (((size_t)f * OH + (size_t)(oy0 + r)) * OW + ox0) * 3, tx, 32);
}

}  // namespace unetpp
