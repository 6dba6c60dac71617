// two_stage.h — the two-stage loop's own steps on the device (include/unetpp_two_stage.h; unet_amd/two_stage.py holds the NumPy forms):
//   ts_masks_kernel    (pred == 1) and (pred == 2), cv2.resize(INTER_NEAREST) to the frame, the ROI clip and the two sums of
//                      infer_two_stage_burr.py:303-314, :333-334 in one launch that reads pred once
//   ts_overlay_kernel  the four chained addWeighted passes of visualize_two_stage (:132-153) as one look-up per byte, and the
//                      burr count of :321
//   ts_rotate_kernel   cv2.rotate (:276) as tile transposes through LDS
// Everything is integer.  Rows leave through rf_store_row (raw_frames.h): 16-byte stores cut at the destination's own 16-byte
// boundaries, whatever the pointer is.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "raw_frames.h"

namespace unetpp {

constexpr int TS_THREADS = 256;

// 16 bytes at any address.  The packed type tells the compiler the alignment is 1; gfx950 under amdhsa runs with unaligned
// global access enabled, so this stays one 16-byte load.
struct __attribute__((packed, aligned(1))) TsU4 { unsigned v[4]; };
__device__ __forceinline__ void ts_load16(const uint8_t* p, unsigned* v) {
  const TsU4 t = *reinterpret_cast<const TsU4*>(p);
  v[0] = t.v[0]; v[1] = t.v[1]; v[2] = t.v[2]; v[3] = t.v[3];
}

__device__ __forceinline__ unsigned ts_wave_sum(unsigned v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ---- 1. the two class masks and their sums ----------------------------------------------------------------------------------------
// Grid (ceil(FW / 256), ceil(FH / 8), B); a workgroup owns a 256 x 8 tile of the frame, thread (q, r) of 64 x 4 the columns
// 4 q .. 4 q + 3 of rows r and r + 4.  resizeNN's source index is min(floor(d * ifx), n_src - 1) with ifx = 1 / (n_dst / n_src) in
// double, formed on the host; the product is one correctly rounded double multiplication here, as there.  Both masks of the tile
// go to LDS as dwords and leave through rf_store_row; the set pixels are summed per wave, then per workgroup in LDS, and one
// 64-bit atomic per class adds them to counts[f] (skipped when the tile has none).
constexpr int TS_MW = 256, TS_MH = 8, TS_MSTRIDE = TS_MW + 16;

__global__ void __launch_bounds__(TS_THREADS) ts_masks_kernel(const uint8_t* __restrict__ pred, int SH, int SW, int FH, int FW, double ifx, double ify, int x1,
                                                             int y1, int x2, int y2, uint8_t* __restrict__ cable, uint8_t* __restrict__ tape,
                                                             unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) uint8_t s_c[TS_MH * TS_MSTRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t s_t[TS_MH * TS_MSTRIDE];
  __shared__ unsigned s_n[2];
  const int t = threadIdx.x, q = t & 63, r = t >> 6;
  const int x0 = blockIdx.x * TS_MW, y0 = blockIdx.y * TS_MH, f = blockIdx.z;
  const int nx = min(TS_MW, FW - x0), ny = min(TS_MH, FH - y0);
  if (t < 2) s_n[t] = 0u;
  int sx[4];
  bool in_x[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int dx = x0 + 4 * q + j;
    sx[j] = min((int)floor(__dmul_rn((double)dx, ifx)), SW - 1);
    in_x[j] = dx >= x1 && dx < x2 && dx < FW;
  }
  unsigned nc = 0u, nt = 0u;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int ly = r + 4 * k, dy = y0 + ly;
    unsigned wc = 0u, wt = 0u;
    if (dy < FH && dy >= y1 && dy < y2) {
      const int sy = min((int)floor(__dmul_rn((double)dy, ify)), SH - 1);
      const uint8_t* row = pred + ((size_t)f * SH + (size_t)sy) * SW;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (in_x[j]) {
          const unsigned v = row[sx[j]];
          wc |= (v == 1u ? 1u : 0u) << (8 * j);
          wt |= (v == 2u ? 1u : 0u) << (8 * j);
        }
      }
    }
    *reinterpret_cast<unsigned*>(s_c + ly * TS_MSTRIDE + 4 * q) = wc;
    *reinterpret_cast<unsigned*>(s_t + ly * TS_MSTRIDE + 4 * q) = wt;
    nc += __popc(wc);
    nt += __popc(wt);
  }
  nc = ts_wave_sum(nc);
  nt = ts_wave_sum(nt);
  __syncthreads();                                           // s_n is zero, the tile is in LDS
  if ((t & 63) == 0) {
    if (nc) atomicAdd(&s_n[0], nc);
    if (nt) atomicAdd(&s_n[1], nt);
  }
  const int sub = t >> 5, l = t & 31;
  if (sub < ny) {
    const size_t at = ((size_t)f * FH + (size_t)(y0 + sub)) * FW + x0;
    rf_store_row(s_c + sub * TS_MSTRIDE, nx, cable + at, l, 32);
    rf_store_row(s_t + sub * TS_MSTRIDE, nx, tape + at, l, 32);
  }
  __syncthreads();
  if (t < 2 && s_n[t]) atomicAdd(&counts[2 * (size_t)f + t], (unsigned long long)s_n[t]);
}

// ---- 2. the overlay: out byte = table[state][channel][frame byte] ---------------------------------------------------------------------
// state = 8 inside + 4 cable + 2 tape + burr (inside: x1 <= x < x2 and y1 <= y < y2; a mask is set where its byte is non-zero);
// the table uint8 [16,3,256] comes from the NumPy form itself (two_stage.overlay_table), so no float is formed here.
// Grid (spans, B).  A frame's 3 HW bytes are cut into spans of 48 bytes = 16 whole pixels whose first byte lies on a 16-byte
// boundary of the OUTPUT: with a = the frame's output address modulo 16 the spans start at 48 k - pad, pad = a + 16 j for the
// j that makes pad a multiple of 3 (0 <= pad < 48), so a span starts with a pixel's first byte.  A thread takes one span:
// three 16-byte loads of the frame and one of each mask at whatever address they have, 48 look-ups in LDS, three aligned 16-byte
// stores.  The first and the last span of a frame may be ragged and go byte by byte.  The burr pixels are summed per wave, per
// workgroup in LDS, and one 64-bit atomic adds them to burr_count[f].
constexpr int TS_OV_TABLE = 16 * 3 * 256;

__global__ void __launch_bounds__(TS_THREADS) ts_overlay_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ cable,
                                                               const uint8_t* __restrict__ tape, const uint8_t* __restrict__ burr, int H, int W, int x1, int y1,
                                                               int x2, int y2, const uint8_t* __restrict__ table, uint8_t* __restrict__ out,
                                                               unsigned long long* __restrict__ burr_count) {
  __shared__ __attribute__((aligned(16))) uint8_t tab[TS_OV_TABLE];
  __shared__ unsigned s_n;
  const int t = threadIdx.x, f = blockIdx.y;
  const int hw = H * W;                                      // <= 2^30
  const long long n3 = 3ll * hw;
  const uint8_t* fr = frames + (size_t)f * (size_t)n3;
  uint8_t* o = out + (size_t)f * (size_t)n3;
  const uint8_t* mc = cable + (size_t)f * hw;
  const uint8_t* mt = tape + (size_t)f * hw;
  const uint8_t* mb = burr + (size_t)f * hw;
  const int a = (int)((uintptr_t)o & 15u);
  const int pad = a + 16 * ((3 - a % 3) % 3);
  const long long i0 = ((long long)blockIdx.x * TS_THREADS + t) * 48 - pad;
  const int p0 = (int)(((long long)blockIdx.x * TS_THREADS + t) * 16) - pad / 3;
  const bool live = i0 < n3;
  const bool whole = i0 >= 0 && i0 + 48 <= n3;

  unsigned in[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, vc[4] = {0u, 0u, 0u, 0u}, vt[4] = {0u, 0u, 0u, 0u}, vb[4] = {0u, 0u, 0u, 0u};
  if (whole) {
    ts_load16(fr + i0, in);
    ts_load16(fr + i0 + 16, in + 4);
    ts_load16(fr + i0 + 32, in + 8);
    ts_load16(mc + p0, vc);
    ts_load16(mt + p0, vt);
    ts_load16(mb + p0, vb);
  } else if (live) {
#pragma unroll
    for (int j = 0; j < 48; ++j)
      if (i0 + j >= 0 && i0 + j < n3) in[j >> 2] |= (unsigned)fr[i0 + j] << (8 * (j & 3));
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int p = p0 + j;
      if (p >= 0 && p < hw) {
        vc[j >> 2] |= (unsigned)mc[p] << (8 * (j & 3));
        vt[j >> 2] |= (unsigned)mt[p] << (8 * (j & 3));
        vb[j >> 2] |= (unsigned)mb[p] << (8 * (j & 3));
      }
    }
  }

  if (t == 0) s_n = 0u;
  if (((uintptr_t)table & 15u) == 0) {
    const uint4* src = reinterpret_cast<const uint4*>(table);
    uint4* dst = reinterpret_cast<uint4*>(tab);
    for (int k = t; k < TS_OV_TABLE / 16; k += TS_THREADS) dst[k] = src[k];
  } else {
    for (int k = t; k < TS_OV_TABLE; k += TS_THREADS) tab[k] = table[k];
  }
  __syncthreads();

  unsigned res[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  unsigned nb = 0u;
  if (live) {
    const int ps = max(p0, 0);
    int y = ps / W, x = ps - y * W;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int p = p0 + j;
      if (p >= 0 && p < hw) {
        const unsigned sh = 8 * (j & 3);
        const unsigned c = (vc[j >> 2] >> sh) & 0xffu, tp = (vt[j >> 2] >> sh) & 0xffu, b = (vb[j >> 2] >> sh) & 0xffu;
        const bool inside = x >= x1 && x < x2 && y >= y1 && y < y2;
        const unsigned state = (inside ? 8u : 0u) | (c ? 4u : 0u) | (tp ? 2u : 0u) | (b ? 1u : 0u);
        nb += b ? 1u : 0u;
        const uint8_t* row = tab + state * 768u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int k = 3 * j + ch;
          const unsigned v = (in[k >> 2] >> (8 * (k & 3))) & 0xffu;
          res[k >> 2] |= (unsigned)row[ch * 256 + v] << (8 * (k & 3));
        }
        if (++x == W) { x = 0; ++y; }
      }
    }
    if (whole) {
      uint4* dst = reinterpret_cast<uint4*>(o + i0);
      dst[0] = make_uint4(res[0], res[1], res[2], res[3]);
      dst[1] = make_uint4(res[4], res[5], res[6], res[7]);
      dst[2] = make_uint4(res[8], res[9], res[10], res[11]);
    } else {
#pragma unroll
      for (int j = 0; j < 48; ++j)
        if (i0 + j >= 0 && i0 + j < n3) o[i0 + j] = (uint8_t)((res[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
  }
  nb = ts_wave_sum(nb);
  if ((t & 63) == 0 && nb) atomicAdd(&s_n, nb);
  __syncthreads();
  if (t == 0 && s_n) atomicAdd(&burr_count[f], (unsigned long long)s_n);
}

// ---- 3. cv2.rotate ---------------------------------------------------------------------------------------------------------------------
// code 0 (90 degrees clockwise)          out[y, x] = in[H - 1 - x, y]          out is W x H
// code 1 (180 degrees)                   out[y, x] = in[H - 1 - y, W - 1 - x]  out is H x W
// code 2 (90 degrees counter-clockwise)  out[y, x] = in[x, W - 1 - y]          out is W x H
// Grid (ceil(OW / 32), ceil(OH / 32), B) over the OUTPUT.  The source rectangle of a 32 x 32 output tile is a 32 x 32 rectangle of
// the input (clipped by the frame): its rows go to LDS with consecutive threads on consecutive bytes, the output tile is formed in a
// second LDS buffer with the transpose read from the first (row stride 32 C + 1 bytes), and its rows leave through rf_store_row.
constexpr int TS_RT = 32;

template <int C>
__global__ void __launch_bounds__(TS_THREADS) ts_rotate_kernel(const uint8_t* __restrict__ in, int H, int W, int code, uint8_t* __restrict__ out) {
  constexpr int IN_STRIDE = TS_RT * C + 1, OUT_STRIDE = (TS_RT * C + 3 + 3) & ~3;
  __shared__ uint8_t s_in[TS_RT * IN_STRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[TS_RT * OUT_STRIDE];
  const int t = threadIdx.x, f = blockIdx.z;
  const int OH = code == 1 ? H : W, OW = code == 1 ? W : H;
  const int ox0 = blockIdx.x * TS_RT, oy0 = blockIdx.y * TS_RT;
  const int nx = min(TS_RT, OW - ox0), ny = min(TS_RT, OH - oy0);
  // the source rectangle [sy0, sy0 + nsy) x [sx0, sx0 + nsx)
  int sy0, sx0, nsy, nsx;
  if (code == 0) { nsy = nx; nsx = ny; sy0 = H - ox0 - nx; sx0 = oy0; }
  else if (code == 1) { nsy = ny; nsx = nx; sy0 = H - oy0 - ny; sx0 = W - ox0 - nx; }
  else { nsy = nx; nsx = ny; sy0 = ox0; sx0 = W - oy0 - ny; }
  const uint8_t* src = in + (size_t)f * H * W * C;
  const int row_bytes = nsx * C;
  for (int i = t; i < nsy * row_bytes; i += TS_THREADS) {
    const int ry = i / row_bytes, rb = i - ry * row_bytes;
    s_in[ry * IN_STRIDE + rb] = src[((size_t)(sy0 + ry) * W + sx0) * C + rb];
  }
  __syncthreads();
  const int out_bytes = nx * C;
  for (int i = t; i < ny * out_bytes; i += TS_THREADS) {
    const int ly = i / out_bytes, ob = i - ly * out_bytes, lx = ob / C, c = ob - lx * C;
    int ry, rx;                                              // the source pixel inside the rectangle
    if (code == 0) { ry = nsy - 1 - lx; rx = ly; }
    else if (code == 1) { ry = nsy - 1 - ly; rx = nsx - 1 - lx; }
    else { ry = lx; rx = nsx - 1 - ly; }
    s_out[ly * OUT_STRIDE + ob] = s_in[ry * IN_STRIDE + rx * C + c];
  }
  __syncthreads();
  const int sub = t >> 5, l = t & 31;
  for (int r = sub; r < ny; r += TS_THREADS / 32)
    rf_store_row(s_out + r * OUT_STRIDE, out_bytes, out + (((size_t)f * OH + (size_t)(oy0 + r)) * OW + ox0) * C, l, 32);
}

}  // namespace unetpp
