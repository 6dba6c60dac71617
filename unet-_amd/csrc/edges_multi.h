// edges_multi.h — the grey-level front end of the reference's two other stage-2 burr detectors:
//   detect_burrs_enhanced  (infer_enhanced_burr.py:69-138): Canny | normalised Sobel magnitude | |Laplacian|
//   get_burr_mask_dog      (src/refactor/burr_detector.py:69-118): blur(3, 1.0) - blur(7, 2.0) inside the band
//   has_burr               (src/refactor/burr_detector.py:121-133): count of non-zero pixels
// unet_amd/edges.py restates each in NumPy; every result is exact and the tests compare for equality.
//
// Tiling as edge_map_kernel (edges.h): one 256-thread workgroup per 32 x 128 tile of one frame, thread t owning 16
// pixels of row t / 8; the grey tile and its halo in LDS, loaded from reflected global coordinates (BORDER_REFLECT_101,
// the default of cv2.Sobel, cv2.Laplacian and cv2.GaussianBlur), so a tile seam inside the image sees no border rule
// and the halo is recomputed, never exchanged.  No workgroup waits for another.
//
// Launch sequence of unetpp_edges_union_u8 (hand-overs cross kernel boundaries on one stream):
//   memset smax[B] = 0
//   sobel_max_kernel    s = dx^2 + dy^2 per pixel of the tile -> max in the wave (__shfl_xor) -> max over the 4 waves
//                       (LDS) -> ONE atomicMax per workgroup into smax[frame].  Integer max: the same bits in any order.
//   edge_union_kernel   lane 0 turns smax[frame] and the Sobel threshold into the smallest passing s (sobel_s_threshold,
//                       fp64, contraction off) and broadcasts it through LDS; per pixel s >= that, (|lap| & 255) > t,
//                       OR with the Canny byte.  16 bytes in, 16 bytes out per thread; in place on the Canny image is fine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edges.h"

namespace unetpp {

constexpr int EM_GW = ED_TW + 2, EM_GH = ED_TH + 2;     // grey window of the 3x3 operators: halo 1
constexpr int EM_GS = 132;                              // its row stride: 33 dwords, so the 8 rows of a wave start on 8 banks

// Grey tile + halo of `halo` into LDS, reflected at the image border.  rows x cols = window, gs = LDS row stride.
__device__ __forceinline__ void em_load_tile(const uint8_t* __restrict__ src, int H, int W, int gy0, int gx0, int halo, int rows,
                                             int cols, int gs, uint8_t* G) {
  for (int i = threadIdx.x; i < rows * cols; i += ED_THREADS) {
    const int ry = i / cols, rx = i - ry * cols;
    const int y = ed_reflect(gy0 - halo + ry, H), x = ed_reflect(gx0 - halo + rx, W);
    G[ry * gs + rx] = src[(size_t)y * W + x];
  }
}

// dx^2 + dy^2 of the 3x3 Sobel operator (<= 2 * 1020^2) and the ksize = 1 Laplacian at the 16 pixels from window
// position (row + 1, lx0 + 1): three rows of 18 bytes, column sums shared between neighbours.
//   V[c] = top + 2 mid + bottom, D[c] = bottom - top;  dx = V[c + 1] - V[c - 1],  dy = D[c - 1] + 2 D[c] + D[c + 1]
template <bool WANT_LAP>
__device__ __forceinline__ void em_sobel_row(const uint8_t* G, int row, int lx0, int (&s)[CC_PX], int (&lap)[CC_PX]) {
  const uint8_t* top = G + row * EM_GS + lx0;
  const uint8_t* mid = top + EM_GS;
  const uint8_t* bot = mid + EM_GS;
  int V[CC_PX + 2], D[CC_PX + 2], M[CC_PX + 2], T[CC_PX + 2];
#pragma unroll
  for (int c = 0; c < CC_PX + 2; ++c) {
    const int a = top[c], m = mid[c], b = bot[c];
    V[c] = a + 2 * m + b;
    D[c] = b - a;
    M[c] = m;
    T[c] = a + b;
  }
#pragma unroll
  for (int j = 0; j < CC_PX; ++j) {
    const int dx = V[j + 2] - V[j], dy = D[j] + 2 * D[j + 1] + D[j + 2];
    s[j] = dx * dx + dy * dy;
    if (WANT_LAP) lap[j] = T[j + 1] + M[j] + M[j + 2] - 4 * M[j + 1];
  }
}

// smax[frame] = max over the frame of dx^2 + dy^2; grid (tiles in x, tiles in y, B); smax zeroed before the launch.
__global__ void __launch_bounds__(ED_THREADS) sobel_max_kernel(const uint8_t* __restrict__ gray, int H, int W, unsigned* __restrict__ smax) {
  __shared__ __attribute__((aligned(16))) uint8_t G[EM_GH * EM_GS];
  __shared__ unsigned wave_max[ED_THREADS / 64];
  const int t = threadIdx.x;
  const int gy0 = blockIdx.y * ED_TH, gx0 = blockIdx.x * ED_TW;
  em_load_tile(gray + (size_t)blockIdx.z * H * W, H, W, gy0, gx0, 1, EM_GH, EM_GW, EM_GS, G);
  __syncthreads();
  const int row = t >> 3, lx0 = (t & 7) * CC_PX;
  unsigned m = 0;
  if (gy0 + row < H && gx0 + lx0 < W) {
    int s[CC_PX], lap[CC_PX];
    em_sobel_row<false>(G, row, lx0, s, lap);
#pragma unroll
    for (int j = 0; j < CC_PX; ++j)
      if (gx0 + lx0 + j < W) m = max(m, (unsigned)s[j]);   // only pixels inside the image count
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
  if ((t & 63) == 0) wave_max[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    m = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
    if (m) atomicMax(smax + blockIdx.z, m);
  }
}

// unet_amd/edges.py sobel_s_threshold: the smallest integer s in [0, smax] with
// (int)(sqrt((double)s) / sqrt((double)smax) * 255.0) > thr, smax + 1 where none passes, 1 for smax == 0 (no Sobel
// edges on a constant frame).  sqrt, division and product are IEEE fp64 and never fused, as NumPy evaluates them.
__device__ __noinline__ unsigned em_sobel_s_threshold(unsigned smax, int thr) {
#pragma clang fp contract(off)
  if (smax == 0) return 1u;
  if (thr < 0) return 0u;
  const double root_max = __dsqrt_rn((double)smax);
  auto passes = [&](unsigned s) { return (int)(__ddiv_rn(__dsqrt_rn((double)s), root_max) * 255.0) > thr; };
  const double k = __ddiv_rn((double)(thr + 1), 255.0);
  const double est = floor(k * k * (double)smax);
  unsigned c = (unsigned)fmin(fmax(est, 0.0), (double)smax);
  if (passes(c)) {
    while (c > 0 && passes(c - 1)) --c;
  } else {
    while (c <= smax && !passes(c)) ++c;
  }
  return c;
}

// out = canny | (s >= s_thr ? 255 : 0) | ((|lap| & 255) > lap_thr ? 255 : 0); grid (tiles in x, tiles in y, B).
// vec_ok: W % 16 == 0 and canny and out 16-byte aligned.  out == canny is allowed: a thread reads its own 16 bytes
// before it writes them and nobody else touches them.
__global__ void __launch_bounds__(ED_THREADS) edge_union_kernel(const uint8_t* __restrict__ gray, const uint8_t* canny, int H, int W,
                                                               const unsigned* __restrict__ smax, int sobel_thr, int lap_thr, int vec_ok,
                                                               uint8_t* out) {
  __shared__ __attribute__((aligned(16))) uint8_t G[EM_GH * EM_GS];
  __shared__ unsigned s_thr_lds;
  const int t = threadIdx.x;
  const int gy0 = blockIdx.y * ED_TH, gx0 = blockIdx.x * ED_TW;
  const size_t frame = (size_t)blockIdx.z * H * W;
  if (t == 0) s_thr_lds = em_sobel_s_threshold(smax[blockIdx.z], sobel_thr);
  em_load_tile(gray + frame, H, W, gy0, gx0, 1, EM_GH, EM_GW, EM_GS, G);
  __syncthreads();
  const int row = t >> 3, lx0 = (t & 7) * CC_PX;
  const int gy = gy0 + row, gxs = gx0 + lx0;
  if (gy >= H || gxs >= W) return;
  const unsigned s_thr = s_thr_lds;
  const size_t off = frame + (size_t)gy * W + gxs;
  unsigned wv[4];
  if (vec_ok) {
    const uint4 v = *reinterpret_cast<const uint4*>(canny + off);
    wv[0] = v.x; wv[1] = v.y; wv[2] = v.z; wv[3] = v.w;
  } else {
    wv[0] = wv[1] = wv[2] = wv[3] = 0;
    for (int j = 0; j < CC_PX && gxs + j < W; ++j) wv[j >> 2] |= (unsigned)canny[off + j] << (8 * (j & 3));
  }
  int s[CC_PX], lap[CC_PX];
  em_sobel_row<true>(G, row, lx0, s, lap);
#pragma unroll
  for (int j = 0; j < CC_PX; ++j)
    if ((unsigned)s[j] >= s_thr || (abs(lap[j]) & 255) > lap_thr) wv[j >> 2] |= 255u << (8 * (j & 3));
  if (vec_ok) {
    *reinterpret_cast<uint4*>(out + off) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  } else {
    for (int j = 0; j < CC_PX && gxs + j < W; ++j) out[off + j] = (uint8_t)((wv[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// ---- difference of Gaussians inside the band ------------------------------------------------------------------------
// out = 255 where band != 0 and max(blur1 - blur2, 0) > threshold (cv2.subtract saturates; the reference's np.abs
// after it is a no-op).  Both blurs are cv2.GaussianBlur's 8-bit path as in edge_map_kernel: horizontal pass into an
// 8.8 plane, vertical pass into 32 bits, (acc + 32768) >> 16.  Both kernels travel centred in 7 taps (zeros outside
// their own length), so one horizontal and one vertical pass serve both.
// LDS: grey 38 x 140 = 5320 B + two 8.8 planes of 38 x 136 x 2 = 10336 B each = 25992 B: 6 workgroups per CU.
constexpr int DG_HALO = ED_MAX_R;                        // 3
constexpr int DG_GW = ED_TW + 2 * DG_HALO, DG_GH = ED_TH + 2 * DG_HALO;   // 134 x 38
constexpr int DG_GS = 140;                               // grey row stride: 35 dwords
constexpr int DG_HS = ED_TW + 8;                         // 8.8 row stride in elements: 272 B, 4 banks past a bank row

struct DogTaps {                                         // each kernel centred: t[3 - n / 2 + k] = taps[k], 0 elsewhere
  int t1[ED_MAX_TAPS], t2[ED_MAX_TAPS];
};

// grid (tiles in x, tiles in y, B).  A workgroup whose band tile is all zero stores zeros and leaves after the one
// barrier every thread reaches (__syncthreads_or); otherwise a thread whose own 16 band bytes are zero takes part in
// the shared passes and both barriers and skips only its own vertical pass.
__global__ void __launch_bounds__(ED_THREADS) dog_band_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ band, int H, int W,
                                                             DogTaps taps, int threshold, int vec_ok, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t G[DG_GH * DG_GS];
  __shared__ __attribute__((aligned(16))) uint16_t H1[DG_GH * DG_HS];
  __shared__ __attribute__((aligned(16))) uint16_t H2[DG_GH * DG_HS];
  const int t = threadIdx.x;
  const int gy0 = blockIdx.y * ED_TH, gx0 = blockIdx.x * ED_TW;
  const size_t frame = (size_t)blockIdx.z * H * W;
  const int row = t >> 3, lx0 = (t & 7) * CC_PX;
  const int gy = gy0 + row, gxs = gx0 + lx0;
  const bool inside = gy < H && gxs < W;
  const size_t off = frame + (size_t)gy * W + gxs;
  unsigned bw[4] = {0, 0, 0, 0};
  if (inside) {
    if (vec_ok) {
      const uint4 v = *reinterpret_cast<const uint4*>(band + off);
      bw[0] = v.x; bw[1] = v.y; bw[2] = v.z; bw[3] = v.w;
    } else {
      for (int j = 0; j < CC_PX && gxs + j < W; ++j) bw[j >> 2] |= (unsigned)band[off + j] << (8 * (j & 3));
    }
  }
  const bool mine = (bw[0] | bw[1] | bw[2] | bw[3]) != 0;
  unsigned wv[4] = {0, 0, 0, 0};
  if (__syncthreads_or(mine)) {                          // the same answer in every thread: the branch is uniform
    em_load_tile(gray + frame, H, W, gy0, gx0, DG_HALO, DG_GH, DG_GW, DG_GS, G);
    __syncthreads();
    // horizontal pass: 4 output columns per item from 10 grey bytes (three aligned words)
    for (int i = t; i < DG_GH * (ED_TW / 4); i += ED_THREADS) {
      const int ry = i / (ED_TW / 4), cx = (i - ry * (ED_TW / 4)) * 4;
      const unsigned* gw = reinterpret_cast<const unsigned*>(G + ry * DG_GS + cx);
      const unsigned w0 = gw[0], w1 = gw[1], w2 = gw[2];
      int g[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g[k] = (w0 >> (8 * k)) & 0xffu; g[4 + k] = (w1 >> (8 * k)) & 0xffu; g[8 + k] = (w2 >> (8 * k)) & 0xffu;
      }
      unsigned a1[4], a2[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        int x1 = 0, x2 = 0;
#pragma unroll
        for (int k = 0; k < ED_MAX_TAPS; ++k) { x1 += taps.t1[k] * g[c + k]; x2 += taps.t2[k] * g[c + k]; }
        a1[c] = (unsigned)x1; a2[c] = (unsigned)x2;    // <= 255 * 256
      }
      *reinterpret_cast<uint2*>(H1 + ry * DG_HS + cx) = make_uint2(a1[0] | (a1[1] << 16), a1[2] | (a1[3] << 16));
      *reinterpret_cast<uint2*>(H2 + ry * DG_HS + cx) = make_uint2(a2[0] | (a2[1] << 16), a2[2] | (a2[3] << 16));
    }
    __syncthreads();
    if (mine) {
      int acc1[CC_PX], acc2[CC_PX];
#pragma unroll
      for (int j = 0; j < CC_PX; ++j) acc1[j] = acc2[j] = 0;
#pragma unroll
      for (int k = 0; k < ED_MAX_TAPS; ++k) {
        const uint4* p1 = reinterpret_cast<const uint4*>(H1 + (row + k) * DG_HS + lx0);
        const uint4* p2 = reinterpret_cast<const uint4*>(H2 + (row + k) * DG_HS + lx0);
        const uint4 u[2] = {p1[0], p1[1]}, v[2] = {p2[0], p2[1]};
        const unsigned uw[8] = {u[0].x, u[0].y, u[0].z, u[0].w, u[1].x, u[1].y, u[1].z, u[1].w};
        const unsigned vw[8] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w};
#pragma unroll
        for (int j = 0; j < CC_PX; ++j) {
          acc1[j] += taps.t1[k] * (int)((uw[j >> 1] >> (16 * (j & 1))) & 0xffffu);
          acc2[j] += taps.t2[k] * (int)((vw[j >> 1] >> (16 * (j & 1))) & 0xffffu);
        }
      }
#pragma unroll
      for (int j = 0; j < CC_PX; ++j) {
        const int d = max(((acc1[j] + 32768) >> 16) - ((acc2[j] + 32768) >> 16), 0);    // cv2.subtract saturates at 0
        if (((bw[j >> 2] >> (8 * (j & 3))) & 0xffu) && d > threshold) wv[j >> 2] |= 255u << (8 * (j & 3));
      }
    }
  }
  if (!inside) return;
  if (vec_ok) {
    *reinterpret_cast<uint4*>(out + off) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  } else {
    for (int j = 0; j < CC_PX && gxs + j < W; ++j) out[off + j] = (uint8_t)((wv[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// counts[frame] += non-zero bytes of the frame; grid (chunks of 4096 pixels, B); counts zeroed before the launch.
// One atomicAdd per workgroup; integer sums are the same bits in any order.
__global__ void __launch_bounds__(ED_THREADS) count_nonzero_kernel(const uint8_t* __restrict__ mask, int HW, int vec_ok,
                                                                  unsigned* __restrict__ counts) {
  __shared__ unsigned wave_sum[ED_THREADS / 64];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * CC_CHUNK + t * CC_PX;
  unsigned n = 0;
  if (i0 < HW) {
    unsigned wv[4];
    ed_load16(mask + (size_t)blockIdx.y * HW, i0, HW, vec_ok, wv);
#pragma unroll
    for (int j = 0; j < CC_PX; ++j) n += ((wv[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += (unsigned)__shfl_xor((int)n, d, 64);
  if ((t & 63) == 0) wave_sum[t >> 6] = n;
  __syncthreads();
  if (t == 0) {
    n = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    if (n) atomicAdd(counts + blockIdx.y, n);
  }
}

}  // namespace unetpp
