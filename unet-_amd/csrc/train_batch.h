// train_batch.h — training batches on the device (include/unetpp_train_batch.h; unet_amd/train_batch.py holds the NumPy forms):
//   tb_crop_rects_kernel  the tape-focused crop of src/data/advanced_dataset.py:148-186: the k-th pixel of a class in raster
//                         order and the integer lines :165-180, one workgroup per sample, the rectangle left in a device table
//   tb_batch_kernel       what the reference's dataset classes do per pixel (src/data/dataset.py:82-101 and :115-131,
//                         src/data/patch_dataset.py:175-231): crop, fliplr / flipud / rot90, a byte look-up on the taps, the
//                         INTER_LINEAR resize, flips after it, the HSV brightness step, / 255 and HWC -> CHW for the image; the
//                         same geometry through the INTER_NEAREST resize and one class look-up for the mask
// The dataset stays resident as two uint8 arenas (RGB images [h,w,3], masks [h,w]) with an item table int64 [n,4] = (image
// offset, mask offset, h, w).  No intermediate image exists in memory: an output pixel maps its four taps back through the
// geometry to bytes of the arena (staged in LDS tile by tile).  Every output byte is written once, no atomics: nothing depends on the order in which threads arrive.
// Everything read from a device table (item, rectangle, look-up rows) is checked against the arenas' sizes before it is used;
// a sample whose plan row or rectangle does not fit is written as zeros, never read out of range.
//
// Arithmetic
//   resize      roi_linear_coef of roi_loop.h per axis, from the sample's own crop size after geometry A; horizontal pass
//               p0 a0 + p1 a1 in int32, vertical pass (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2.  Equal sizes
//               give a0 = 2048, a1 = 0 and the source byte.
//   nearest     source index min(floor(d * (1 / (n_dst / n_src))), n_src - 1) in float64
//   geometry A  the resize's source is V = rot90(flipud(fliplr(crop)), k); V[Y, X] = M[my, mx] with (my, mx) = (Y, X), (X, cw - 1
//               - Y), (ch - 1 - Y, cw - 1 - X), (ch - 1 - X, Y) for k = 0..3 and M[y, x] = crop[flip_v ? ch - 1 - y : y][flip_h ? cw
//               - 1 - x : x]
//   geometry B  out[y, x] = resized[post_flip_v ? OH - 1 - y : y][post_flip_h ? OW - 1 - x : x]
//   RGB -> HSV  v = max, diff = v - min, s = (diff sdiv[v] + 2048) >> 12, h = (v == r ? g - b : v == g ? b - r + 2 diff : r - g +
//               4 diff), h = (h hdiv[diff] + 2048) >> 12, h += 180 when negative; sdiv[i] = rint((255 << 12) / i), hdiv[i] =
//               rint((180 << 12) / (6 i)) in float64, both 0 at 0 (formed once per workgroup)
//   HSV -> RGB  float32, no contraction: hf = fmod(h (6.f / 180.f), 6), sector = floor(hf), hf -= sector; s and v times (1.f /
//               255.f); tab = (v, v (1 - s), v (1 - s hf), v (1 - s (1 - hf))), (b, g, r) picked by the sector table; s == 0: v
//               thrice; each channel rint(x 255.f) saturated
//   / 255       __fdiv_rn((float)i, 255.f), formed once per workgroup
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "raw_frames.h"

namespace unetpp {

constexpr int TB_THREADS = 256;
constexpr int TB_TW = 32, TB_TH = 32;                  // the output tile: 32 x 8 threads, four rows each
constexpr int TB_PLAN = 16;                            // int32 columns of a plan row
constexpr int TB_ITEM = 4;                             // int64 columns of an item row
constexpr int TB_RECT = 6, TB_REQUEST = 5;
constexpr int TB_F32_STRIDE = 4 * TB_TW + 4;           // bytes of a float row in LDS: rf_store_row may read 4 past the row
constexpr int TB_U8_STRIDE = 3 * TB_TW + 4;
constexpr int TB_MASK_STRIDE = TB_TW + 4;
constexpr int TB_RECT_BYTES = 32768;                   // the staged source rectangle of one output tile; a larger one is read in place
constexpr int TB_SEG = 16;                             // bytes of the mask one thread of tb_crop_rects_kernel compares per pass
enum { TB_OUT_CHW_F32 = 0, TB_OUT_HWC_RGB = 1, TB_OUT_HWC_BGR = 2 };
// plan columns
enum { TBP_ITEM = 0, TBP_RECT_ROW, TBP_X1, TBP_Y1, TBP_X2, TBP_Y2, TBP_FLIP_H, TBP_FLIP_V, TBP_ROT, TBP_BYTE_LUT, TBP_POST_FLIP_H,
       TBP_POST_FLIP_V, TBP_VALUE_LUT };

struct TbItem { long long image, mask; int h, w; bool ok; };

// Row `item` of the table, valid only when the item lies wholly inside both arenas.
__device__ __forceinline__ TbItem tb_item(const long long* __restrict__ items, int n_items, int item, long long images_bytes,
                                          long long masks_bytes, bool need_images) {
  TbItem it;
  it.ok = false; it.image = it.mask = 0; it.h = it.w = 0;
  if (item < 0 || item >= n_items) return it;
  const long long* r = items + (size_t)item * TB_ITEM;
  const long long io = r[0], mo = r[1], h = r[2], w = r[3];
  if (h < 1 || w < 1 || h > 65535 || w > 65535 || h * w > (long long)INT_MAX) return it;
  if (mo < 0 || mo > masks_bytes - h * w) return it;
  if (need_images && (io < 0 || io > images_bytes - 3 * h * w)) return it;
  it.image = io; it.mask = mo; it.h = (int)h; it.w = (int)w; it.ok = true;
  return it;
}

// ---- 1. the data-dependent rectangle ------------------------------------------------------------------------------------------------
// rects[b] = (x1, y1, x2, y2, n_found, valid) for requests[b] = (item, k, crop_h, crop_w, class).  Grid (B).
// The item's mask is one run of h w bytes, so raster order is byte order.  The run is cut into 16-byte segments at the ADDRESS's
// multiples of 16; a pass gives each thread one segment: a 16-byte load (bytes for the segments that hang over the ends), a byte
// compare into a 16-bit match word and a popcount.  A scan over the workgroup (shuffles in the wave, four wave totals in LDS)
// gives every segment the number of matches before it; the thread whose segment holds the k-th match looks inside its match
// word for the bit.  All passes run, because n_found is part of the result.
__device__ __forceinline__ int tb_nth_bit(unsigned bits, int n) {
  for (int i = 0; i < n; ++i) bits &= bits - 1;            // drop the n lowest set bits
  return __ffs((int)bits) - 1;
}

__global__ void __launch_bounds__(TB_THREADS) tb_crop_rects_kernel(const uint8_t* __restrict__ masks, long long masks_bytes,
                                                                  const long long* __restrict__ items, int n_items,
                                                                  const int* __restrict__ requests, int* __restrict__ rects) {
  __shared__ int s_wave[2][TB_THREADS / 64];
  __shared__ long long s_pos;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  const int* rq = requests + (size_t)b * TB_REQUEST;
  const long long k = rq[1];
  const int crop_h = rq[2], crop_w = rq[3], cls = rq[4];
  int* out = rects + (size_t)b * TB_RECT;
  const TbItem it = tb_item(items, n_items, rq[0], 0, masks_bytes, false);
  if (!it.ok) {                                              // the same in every thread
    if (t < TB_RECT) out[t] = 0;
    return;
  }
  const uint8_t* base = masks + it.mask;
  const long long n = (long long)it.h * it.w;
  const long long head = (long long)((uintptr_t)base & 15u);
  const long long nseg = (head + n + TB_SEG - 1) / TB_SEG;
  if (t == 0) s_pos = -1;
  long long running = 0;
  int parity = 0;
  for (long long c0 = 0; c0 < nseg; c0 += TB_THREADS, parity ^= 1) {
    const long long c = c0 + t, i0 = TB_SEG * c - head;
    unsigned bits = 0;
    if (c < nseg) {
      if (i0 >= 0 && i0 + TB_SEG <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + i0);
        const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < TB_SEG; ++j) bits |= (unsigned)(((wds[j >> 2] >> (8 * (j & 3))) & 255u) == (unsigned)cls) << j;
      } else {
        for (int j = 0; j < TB_SEG; ++j)
          if (i0 + j >= 0 && i0 + j < n) bits |= (unsigned)((unsigned)base[i0 + j] == (unsigned)cls) << j;
      }
    }
    const int cnt = __popc(bits);
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    if (lane == 63) s_wave[parity][wave] = incl;
    __syncthreads();                                         // also orders s_pos = -1 before the first write below
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < TB_THREADS / 64; ++w) {
      const int v = s_wave[parity][w];
      before += w < wave ? v : 0;
      total += v;
    }
    const long long excl = running + before + (incl - cnt);
    if (k >= excl && k < excl + cnt) s_pos = i0 + tb_nth_bit(bits, (int)(k - excl));      // one thread at most
    running += total;
  }
  __syncthreads();
  if (t == 0) {
    const int h = it.h, w = it.w;
    int x1 = 0, y1 = 0, x2 = w, y2 = h, valid = 1;
    const long long pos = s_pos;
    if (running > 0) {
      if (pos < 0 || crop_h < 1 || crop_w < 1) {
        valid = 0;                                           // k outside 0 .. n_found - 1 (a stale count), or no crop size
      } else {
        const int cy = (int)(pos / w), cx = (int)(pos % w);
        y1 = max(0, cy - crop_h / 2);
        y2 = min(h, cy + crop_h / 2);
        x1 = max(0, cx - crop_w / 2);
        x2 = min(w, cx + crop_w / 2);
        if (y2 - y1 < crop_h) {
          if (y1 == 0) y2 = min(h, y1 + crop_h);
          else y1 = max(0, y2 - crop_h);
        }
        if (x2 - x1 < crop_w) {
          if (x1 == 0) x2 = min(w, x1 + crop_w);
          else x1 = max(0, x2 - crop_w);
        }
      }
    }
    out[0] = x1; out[1] = y1; out[2] = x2; out[3] = y2;
    out[4] = (int)(running > (long long)INT_MAX ? (long long)INT_MAX : running);
    out[5] = valid;
  }
}

// ---- 2. the batch ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tb_nearest(int d, int n_src, int n_dst) {
#pragma clang fp contract(off)
  const double scale = 1.0 / ((double)n_dst / (double)n_src);
  return min((int)floor((double)d * scale), n_src - 1);
}

struct TbGeom { int x1, y1, cw, ch, flip_h, flip_v, rot; };

struct TbPos { int y, x; };

// The item's pixel (row, column) that V[Y, X] is.
__device__ __forceinline__ TbPos tb_source(const TbGeom& g, int Y, int X) {
  int my, mx;
  switch (g.rot) {
    case 0: my = Y; mx = X; break;
    case 1: my = X; mx = g.cw - 1 - Y; break;
    case 2: my = g.ch - 1 - Y; mx = g.cw - 1 - X; break;
    default: my = g.ch - 1 - X; mx = Y; break;
  }
  TbPos q;
  q.y = g.y1 + (g.flip_v ? g.ch - 1 - my : my);
  q.x = g.x1 + (g.flip_h ? g.cw - 1 - mx : mx);
  return q;
}

// The tile's source rectangle in LDS.  Row r of it holds the item's row r_lo + r from column c_lo on, 3 bytes a pixel, at the
// byte the row's ADDRESS has modulo 16, so that every 16 bytes between two 16-byte boundaries of the source go from memory to
// LDS as one load and one store.
struct TbStage { int r_lo, c_lo, stride, on; };

__device__ __forceinline__ int tb_stage_at(const TbStage& st, const uint8_t* __restrict__ img, int w, TbPos q) {
  const int off = (int)((uintptr_t)(img + 3 * ((long long)q.y * w + st.c_lo)) & 15u);
  return (q.y - st.r_lo) * st.stride + off + 3 * (q.x - st.c_lo);
}

__device__ __forceinline__ int tb_sat_u8(float x) {
  return (int)fminf(fmaxf(rintf(x), 0.0f), 255.0f);
}

// The brightness step for one RGB pixel: v through `table`.
__device__ __forceinline__ void tb_value_scale(int& r, int& g, int& b, const uint8_t* __restrict__ table, const int* __restrict__ sdiv,
                                               const int* __restrict__ hdiv) {
#pragma clang fp contract(off)
  const int v = max(max(r, g), b), diff = v - min(min(r, g), b);
  const int s = min(max((diff * sdiv[v] + (1 << 11)) >> 12, 0), 255);
  int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h * hdiv[diff] + (1 << 11)) >> 12;
  h += h < 0 ? 180 : 0;
  h = min(max(h, 0), 255);
  const int v2 = table[v];
  float hf = (float)h * (6.0f / 180.0f);
  const float sf = (float)s * (1.0f / 255.0f), vf = (float)v2 * (1.0f / 255.0f);
  float fb, fg, fr;
  if (sf == 0.0f) {
    fb = fg = fr = vf;
  } else {
    hf = fmodf(hf, 6.0f);
    int sector = (int)floorf(hf);
    hf = hf - (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; hf = 0.0f; }
    float tab[4];
    tab[0] = vf;
    tab[1] = vf * (1.0f - sf);
    tab[2] = vf * (1.0f - sf * hf);
    tab[3] = vf * (1.0f - sf * (1.0f - hf));
    // (b, g, r) per sector: {1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}, two bits each
    const unsigned code_b = (0x2u << 10) | (0x0u << 8) | (0x0u << 6) | (0x3u << 4) | (0x1u << 2) | 0x1u;
    const unsigned code_g = (0x1u << 10) | (0x1u << 8) | (0x2u << 6) | (0x0u << 4) | (0x0u << 2) | 0x3u;
    const unsigned code_r = (0x0u << 10) | (0x3u << 8) | (0x1u << 6) | (0x1u << 4) | (0x2u << 2) | 0x0u;
    const int ib = (int)((code_b >> (2 * sector)) & 3u), ig = (int)((code_g >> (2 * sector)) & 3u), ir = (int)((code_r >> (2 * sector)) & 3u);
    fb = ib == 0 ? tab[0] : ib == 1 ? tab[1] : ib == 2 ? tab[2] : tab[3];
    fg = ig == 0 ? tab[0] : ig == 1 ? tab[1] : ig == 2 ? tab[2] : tab[3];
    fr = ir == 0 ? tab[0] : ir == 1 ? tab[1] : ir == 2 ? tab[2] : tab[3];
  }
  b = tb_sat_u8(fb * 255.0f);
  g = tb_sat_u8(fg * 255.0f);
  r = tb_sat_u8(fr * 255.0f);
}

// image_out: float32 [B,3,OH,OW] (format 0) or uint8 [B,OH,OW,3] (1: RGB, 2: BGR); target_out uint8 [B,OH,OW].
// Grid (ceil(OW / 32), ceil(OH / 32), B); thread (tx, ty) of 32 x 8 computes column tx of rows ty, ty + 8, ty + 16, ty + 24 of
// the tile into LDS, and the rows leave through rf_store_row: 16-byte stores cut at the destination's own 16-byte boundaries,
// at any alignment and any OW.
// The image's taps come from LDS.  The coefficients are monotone in the output index, so the tile's first and last column and
// row bound the rectangle of V its taps lie in; geometry A maps that rectangle to a rectangle of the item (a flip or a rotation
// permutes and mirrors the axes).  The workgroup stages it in 16-byte slots along the item's rows, so that global loads stay
// row-contiguous whatever the rotation is.  A rectangle that holds more bytes than the tile's taps read (a reduction steeper than
// about 1.4 per axis) or more than TB_RECT_BYTES is read in place instead: staging would load bytes no tap uses.  The mask's
// single nearest tap is read in place.
__global__ void __launch_bounds__(TB_THREADS) tb_batch_kernel(const uint8_t* __restrict__ images, long long images_bytes,
                                                             const uint8_t* __restrict__ masks, long long masks_bytes,
                                                             const long long* __restrict__ items, int n_items,
                                                             const int* __restrict__ plan, const int* __restrict__ rects, int n_rects,
                                                             const uint8_t* __restrict__ luts, int n_luts,
                                                             const uint8_t* __restrict__ class_lut, int OH, int OW, int format,
                                                             void* __restrict__ image_out, uint8_t* __restrict__ target_out) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint8_t s_img[3 * TB_TH * TB_F32_STRIDE + 16];
  __shared__ __attribute__((aligned(16))) uint8_t s_msk[TB_TH * TB_MASK_STRIDE + 16];
  __shared__ __attribute__((aligned(16))) uint8_t s_rect[TB_RECT_BYTES];
  __shared__ RoiCoef s_cx[TB_TW], s_cy[TB_TH];
  __shared__ int s_nx[TB_TW], s_ny[TB_TH];
  __shared__ int s_sdiv[256], s_hdiv[256];
  __shared__ float s_div[256];
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
  const int ox0 = blockIdx.x * TB_TW, oy0 = blockIdx.y * TB_TH, b = blockIdx.z;
  const int nx = min(TB_TW, OW - ox0), ny = min(TB_TH, OH - oy0);
  const int* p = plan + (size_t)b * TB_PLAN;

  // the sample: everything below is the same in every thread of the workgroup
  const TbItem it = tb_item(items, n_items, p[TBP_ITEM], images_bytes, masks_bytes, true);
  TbGeom g;
  bool ok = it.ok;
  {
    int x1 = p[TBP_X1], y1 = p[TBP_Y1], x2 = p[TBP_X2], y2 = p[TBP_Y2];
    const int row = p[TBP_RECT_ROW];
    if (row >= 0) {
      if (rects && row < n_rects) {
        const int* r = rects + (size_t)row * TB_RECT;
        x1 = r[0]; y1 = r[1]; x2 = r[2]; y2 = r[3];
      } else {
        ok = false;
      }
    }
    x1 = min(max(x1, 0), it.w); x2 = min(max(x2, 0), it.w);
    y1 = min(max(y1, 0), it.h); y2 = min(max(y2, 0), it.h);
    g.x1 = x1; g.y1 = y1; g.cw = x2 - x1; g.ch = y2 - y1;
    g.flip_h = p[TBP_FLIP_H] != 0; g.flip_v = p[TBP_FLIP_V] != 0; g.rot = p[TBP_ROT] & 3;
    ok = ok && g.cw >= 1 && g.ch >= 1;
  }
  const int byte_row = p[TBP_BYTE_LUT], value_row = p[TBP_VALUE_LUT];
  ok = ok && byte_row < n_luts && value_row < n_luts && (luts || (byte_row < 0 && value_row < 0));
  const uint8_t* byte_lut = byte_row >= 0 && ok ? luts + (size_t)byte_row * 256 : nullptr;
  const uint8_t* value_lut = value_row >= 0 && ok ? luts + (size_t)value_row * 256 : nullptr;
  const int post_h = p[TBP_POST_FLIP_H] != 0, post_v = p[TBP_POST_FLIP_V] != 0;
  const int vw = (g.rot & 1) ? g.ch : g.cw, vh = (g.rot & 1) ? g.cw : g.ch;          // the resize's source

  if (ok) {
    if (t < TB_TW) {
      const int rx = min(ox0 + t, OW - 1), sx = post_h ? OW - 1 - rx : rx;
      s_cx[t] = roi_linear_coef(sx, vw, OW);
      s_nx[t] = tb_nearest(sx, vw, OW);
    } else if (t < TB_TW + TB_TH) {
      const int ry = min(oy0 + t - TB_TW, OH - 1), sy = post_v ? OH - 1 - ry : ry;
      s_cy[t - TB_TW] = roi_linear_coef(sy, vh, OH);
      s_ny[t - TB_TW] = tb_nearest(sy, vh, OH);
    }
    if (value_lut) {
      s_sdiv[t] = t ? (int)rint((double)(255 << 12) / (double)t) : 0;
      s_hdiv[t] = t ? (int)rint((double)(180 << 12) / (6.0 * (double)t)) : 0;
    }
    if (format == TB_OUT_CHW_F32) s_div[t] = __fdiv_rn((float)t, 255.0f);
  }
  __syncthreads();

  const uint8_t* img = images + it.image;
  const uint8_t* msk = masks + it.mask;
  TbStage st;
  st.r_lo = st.c_lo = st.stride = st.on = 0;
  if (ok) {
    const TbPos a = tb_source(g, min(s_cy[0].s0, s_cy[ny - 1].s0), min(s_cx[0].s0, s_cx[nx - 1].s0));
    const TbPos z = tb_source(g, max(s_cy[0].s1, s_cy[ny - 1].s1), max(s_cx[0].s1, s_cx[nx - 1].s1));
    st.r_lo = min(a.y, z.y); st.c_lo = min(a.x, z.x);
    const int nr = max(a.y, z.y) - st.r_lo + 1, nb = 3 * (max(a.x, z.x) - st.c_lo + 1);
    st.stride = (nb + 15 + 15) & ~15;                          // the row's first byte lies at 0..15
    // staged when it fits and holds no more bytes than the taps read (12 a pixel): measured at 1080 x 1920 -> 512 x 512, where
    // the rectangle is twice the taps, staging took 193 us a batch of 16 and reading in place 83 us
    st.on = (long long)nr * st.stride <= TB_RECT_BYTES && (long long)nr * nb <= 12LL * nx * ny;
    if (st.on) {
      const int cpr = st.stride >> 4, total = nr * cpr;        // 16-byte slots per row; slot k of row r is task r cpr + k
#pragma unroll 4
      for (int task = t; task < total; task += TB_THREADS) {
        const int r = task / cpr, c = task - r * cpr;
        const uint8_t* A = img + 3 * ((long long)(st.r_lo + r) * it.w + st.c_lo);
        const int off = (int)((uintptr_t)A & 15u), i0 = 16 * c - off;
        uint8_t* L = s_rect + r * st.stride + 16 * c;          // L[j] = A[i0 + j]
        if (i0 >= 0 && i0 + 16 <= nb) {
          *reinterpret_cast<uint4*>(L) = *reinterpret_cast<const uint4*>(A + i0);
        } else if (i0 + 16 > 0 && i0 < nb) {
          for (int j = 0; j < 16; ++j)
            if (i0 + j >= 0 && i0 + j < nb) L[j] = A[i0 + j];
        }
      }
    }
  }
  __syncthreads();

  if (tx < nx) {
    for (int oy = ty; oy < ny; oy += TB_THREADS / TB_TW) {
      int px[3] = {0, 0, 0}, m = 0;
      if (ok) {
        const RoiCoef cx = s_cx[tx], cy = s_cy[oy];
        const TbPos q00 = tb_source(g, cy.s0, cx.s0), q01 = tb_source(g, cy.s0, cx.s1);
        const TbPos q10 = tb_source(g, cy.s1, cx.s0), q11 = tb_source(g, cy.s1, cx.s1);
        const uint8_t *t00, *t01, *t10, *t11;
        if (st.on) {
          t00 = s_rect + tb_stage_at(st, img, it.w, q00); t01 = s_rect + tb_stage_at(st, img, it.w, q01);
          t10 = s_rect + tb_stage_at(st, img, it.w, q10); t11 = s_rect + tb_stage_at(st, img, it.w, q11);
        } else {
          t00 = img + 3 * ((long long)q00.y * it.w + q00.x); t01 = img + 3 * ((long long)q01.y * it.w + q01.x);
          t10 = img + 3 * ((long long)q10.y * it.w + q10.x); t11 = img + 3 * ((long long)q11.y * it.w + q11.x);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          int p00 = t00[c], p01 = t01[c], p10 = t10[c], p11 = t11[c];
          if (byte_lut) { p00 = byte_lut[p00]; p01 = byte_lut[p01]; p10 = byte_lut[p10]; p11 = byte_lut[p11]; }
          const int S0 = p00 * cx.a0 + p01 * cx.a1, S1 = p10 * cx.a0 + p11 * cx.a1;
          const int v = (((cy.a0 * (S0 >> 4)) >> 16) + ((cy.a1 * (S1 >> 4)) >> 16) + 2) >> 2;
          px[c] = min(max(v, 0), 255);
        }
        if (value_lut) tb_value_scale(px[0], px[1], px[2], value_lut, s_sdiv, s_hdiv);
        const TbPos qm = tb_source(g, s_ny[oy], s_nx[tx]);
        m = msk[(long long)qm.y * it.w + qm.x];
        if (class_lut) m = class_lut[m];
      }
      s_msk[oy * TB_MASK_STRIDE + tx] = (uint8_t)m;
      if (format == TB_OUT_CHW_F32) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          *reinterpret_cast<float*>(s_img + (c * TB_TH + oy) * TB_F32_STRIDE + 4 * tx) = ok ? s_div[px[c]] : 0.0f;
      } else {
        uint8_t* o = s_img + oy * TB_U8_STRIDE + 3 * tx;
        const bool swap = format == TB_OUT_HWC_BGR;
        o[0] = (uint8_t)px[swap ? 2 : 0]; o[1] = (uint8_t)px[1]; o[2] = (uint8_t)px[swap ? 0 : 2];
      }
    }
  }
  __syncthreads();

  for (int r = ty; r < ny; r += TB_THREADS / TB_TW) {
    const size_t row = (size_t)b * OH + (size_t)(oy0 + r);
    rf_store_row(s_msk + r * TB_MASK_STRIDE, nx, target_out + row * OW + ox0, tx, 32);
    if (format == TB_OUT_CHW_F32) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* dst = reinterpret_cast<float*>(image_out) + (((size_t)b * 3 + c) * OH + (size_t)(oy0 + r)) * OW + ox0;
        rf_store_row(s_img + (c * TB_TH + r) * TB_F32_STRIDE, 4 * nx, reinterpret_cast<uint8_t*>(dst), tx, 32);
      }
    } else {
      rf_store_row(s_img + r * TB_U8_STRIDE, 3 * nx, reinterpret_cast<uint8_t*>(image_out) + (row * OW + ox0) * 3, tx, 32);
    }
  }
}

}  // namespace unetpp
