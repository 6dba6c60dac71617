// edges.h — the grey-level front end of the reference's stage-2 burr detection (infer_two_stage_burr.py:50-119,
// src/refactor/burr_detector.py:11-66): BGR -> grey, Gaussian blur, Canny, and the Laplacian threshold inside a band.
// All arithmetic is integer (unet_amd/edges.py restates it in NumPy), so every result is exact.
//
// Launch sequence of unetpp_canny_u8 (no workgroup ever waits for another; every hand-over crosses a kernel boundary):
//   edge_map_kernel     one workgroup per 32 x 128 tile: grey tile + halo -> LDS, blur (fused, up to 7 taps), 3x3 Sobel,
//                       |dx| + |dy|, non-maximum suppression, the two thresholds -> map {0, 1 = weak, 2 = strong}
//   cc_tile_kernel / cc_merge_kernel / cc_compress_kernel (components.h) on map != 0, connectivity 8:
//                       parent[p] = root of p's component of candidates
//   edge_seed_kernel    map == 2 sets flag[root]
//   edge_apply_kernel   out = flag[root] ? 255 : 0
// A root is the smallest pixel index of its component and a flag is only ever set to 1, so the result is the same
// bits whatever order the stores land in.
//
// Three border rules meet in edge_map_kernel (OpenCV's published GaussianBlur / Canny):
//   the blur reflects the grey image at the image border (BORDER_REFLECT_101);
//   Sobel replicates the BLURRED image there (BORDER_REPLICATE): a pixel outside the image counts as the blurred
//     value at the clamped coordinate, which is not the blur of reflected coordinates;
//   the gradient magnitude outside the image is 0.
// The tile halo is recomputed from global coordinates, so a tile seam inside the image sees none of these rules.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "components.h"

namespace unetpp {

constexpr int ED_TW = CC_TW, ED_TH = CC_TH;  // core tile: the tile of cc_tile_kernel, 256 threads x 16 pixels of a row
constexpr int ED_THREADS = 256;
constexpr int ED_MAX_TAPS = 7, ED_MAX_R = ED_MAX_TAPS / 2;
constexpr int ED_HALO = 2;                   // Sobel (1) + non-maximum suppression (1)
constexpr int ED_BW = ED_TW + 2 * ED_HALO, ED_BH = ED_TH + 2 * ED_HALO;   // blurred window
constexpr int ED_GW = ED_BW + 2 * ED_MAX_R, ED_GH = ED_BH + 2 * ED_MAX_R; // grey window at the widest blur
constexpr int ED_GS = ED_GW + 2;             // grey row stride (bytes)
constexpr int ED_MW = ED_TW + 2, ED_MH = ED_TH + 2;                       // magnitude window
constexpr int ED_TG22 = 13573;               // tan(22.5 deg) in 15 fractional bits, OpenCV's TG22

struct EdgeTaps {                            // 8.8 fixed point, n odd, sum 256; n = 1, t = {256} is the identity
  int n;
  int t[ED_MAX_TAPS];
};

// BORDER_REFLECT_101 of an index that is at most n - 1 outside [0, n); indices further out (only ever reached for
// pixels whose result is not used) are clamped so that every address stays inside the frame.
__device__ __forceinline__ int ed_reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return min(max(i, 0), n - 1);
}

// grid (tiles in x, tiles in y, B).  BLUR_ONLY: out = the blurred image (uint8), else the candidate map.
template <bool BLUR_ONLY>
__global__ void __launch_bounds__(ED_THREADS) edge_map_kernel(const uint8_t* __restrict__ gray, int H, int W, EdgeTaps taps, int low,
                                                             int high, int vec_ok, uint8_t* __restrict__ out) {
  __shared__ uint8_t G[ED_GH * ED_GS];       // grey, global (gy0 - 2 - r + row, gx0 - 2 - r + col), reflected
  __shared__ uint16_t Hh[ED_GH * ED_BW];     // horizontal pass, 8.8: rows as G, columns gx0 - 2 + col
  __shared__ uint8_t Bl[ED_BH * ED_BW];      // blurred, global (gy0 - 2 + row, gx0 - 2 + col)
  __shared__ uint16_t M[ED_MH * ED_MW];      // |dx| + |dy| (<= 2040), global (gy0 - 1 + row, gx0 - 1 + col), 0 outside
  const int t = threadIdx.x;
  const int gy0 = blockIdx.y * ED_TH, gx0 = blockIdx.x * ED_TW;
  const int r = taps.n >> 1;
  const int gh = ED_BH + 2 * r, gw = ED_BW + 2 * r;
  const size_t frame = (size_t)blockIdx.z * H * W;
  const uint8_t* src = gray + frame;
  for (int i = t; i < gh * gw; i += ED_THREADS) {
    const int ry = i / gw, rx = i - ry * gw;
    const int y = ed_reflect(gy0 - ED_HALO - r + ry, H), x = ed_reflect(gx0 - ED_HALO - r + rx, W);
    G[ry * ED_GS + rx] = src[(size_t)y * W + x];
  }
  __syncthreads();
  for (int i = t; i < gh * ED_BW; i += ED_THREADS) {
    const int ry = i / ED_BW, cx = i - ry * ED_BW;
    int acc = 0;
    for (int k = 0; k < taps.n; ++k) acc += taps.t[k] * G[ry * ED_GS + cx + k];
    Hh[i] = (uint16_t)acc;                   // <= 255 * 256
  }
  __syncthreads();
  for (int i = t; i < ED_BH * ED_BW; i += ED_THREADS) {
    const int by = i / ED_BW, cx = i - by * ED_BW;
    int acc = 0;
    for (int k = 0; k < taps.n; ++k) acc += taps.t[k] * Hh[(by + k) * ED_BW + cx];
    Bl[i] = (uint8_t)((acc + 32768) >> 16);
  }
  __syncthreads();
  const int row = t >> 3, lx0 = (t & 7) * CC_PX;
  const int gy = gy0 + row, gxs = gx0 + lx0;
  if (BLUR_ONLY) {
    if (gy < H && gxs < W) {
      uint8_t* dst = out + frame + (size_t)gy * W + gxs;
      const uint8_t* b = Bl + (row + ED_HALO) * ED_BW + lx0 + ED_HALO;
      if (vec_ok) {                          // W % 16 == 0 and out is 16-byte aligned: the 16 pixels exist
        unsigned wv[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < CC_PX; ++j) wv[j >> 2] |= (unsigned)b[j] << (8 * (j & 3));
        *reinterpret_cast<uint4*>(dst) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
      } else {
        for (int j = 0; j < CC_PX && gxs + j < W; ++j) dst[j] = b[j];
      }
    }
    return;
  }
  // Sobel of the blurred image at (y, x) inside the image, neighbours clamped to the image (BORDER_REPLICATE).
  // y in [gy0 - 1, gy0 + ED_TH] and x likewise, so every clamped neighbour lies in the blurred window.
  auto sobel = [&](int y, int x, int* dx, int* dy) {
    const int ym = max(y - 1, 0) - (gy0 - ED_HALO), yc = y - (gy0 - ED_HALO), yp = min(y + 1, H - 1) - (gy0 - ED_HALO);
    const int xm = max(x - 1, 0) - (gx0 - ED_HALO), xc = x - (gx0 - ED_HALO), xp = min(x + 1, W - 1) - (gx0 - ED_HALO);
    const int a = Bl[ym * ED_BW + xm], b = Bl[ym * ED_BW + xc], c = Bl[ym * ED_BW + xp];
    const int d = Bl[yc * ED_BW + xm], f = Bl[yc * ED_BW + xp];
    const int g = Bl[yp * ED_BW + xm], h = Bl[yp * ED_BW + xc], k = Bl[yp * ED_BW + xp];
    *dx = (c + 2 * f + k) - (a + 2 * d + g);
    *dy = (g + 2 * h + k) - (a + 2 * b + c);
  };
  for (int i = t; i < ED_MH * ED_MW; i += ED_THREADS) {
    const int my = i / ED_MW, mx = i - my * ED_MW;
    const int y = gy0 - 1 + my, x = gx0 - 1 + mx;
    int m = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      int dx, dy;
      sobel(y, x, &dx, &dy);
      m = abs(dx) + abs(dy);
    }
    M[i] = (uint16_t)m;
  }
  __syncthreads();
  if (gy >= H || gxs >= W) return;
  unsigned wv[4] = {0, 0, 0, 0};
#pragma unroll 4
  for (int j = 0; j < CC_PX; ++j) {
    const int gx = gxs + j;
    if (gx >= W) break;
    const uint16_t* mc = M + (row + 1) * ED_MW + lx0 + j + 1;
    const int m = mc[0];
    if (m <= low) continue;
    int dx, dy;
    sobel(gy, gx, &dx, &dy);
    const int x = abs(dx), y = abs(dy) << 15;
    const int tg22x = x * ED_TG22;
    bool keep;
    if (y < tg22x) {
      keep = m > mc[-1] && m >= mc[1];
    } else if (y > tg22x + (x << 16)) {
      keep = m > mc[-ED_MW] && m >= mc[ED_MW];
    } else {
      const int s = (dx ^ dy) < 0 ? -1 : 1;
      keep = m > mc[-ED_MW - s] && m > mc[ED_MW + s];
    }
    if (keep) wv[j >> 2] |= (m > high ? 2u : 1u) << (8 * (j & 3));
  }
  uint8_t* dst = out + frame + (size_t)gy * W + gxs;
  if (vec_ok) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  } else {
    for (int j = 0; j < CC_PX && gxs + j < W; ++j) dst[j] = (uint8_t)((wv[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// 16 consecutive bytes of a per-frame uint8 array from i0 (a multiple of 16) as four words; 0 past the frame's end.
__device__ __forceinline__ void ed_load16(const uint8_t* __restrict__ a, int i0, int HW, int vec, unsigned (&wv)[4]) {
  if (vec && i0 + CC_PX <= HW) {
    const uint4 v = *reinterpret_cast<const uint4*>(a + i0);
    wv[0] = v.x; wv[1] = v.y; wv[2] = v.z; wv[3] = v.w;
  } else {
    wv[0] = wv[1] = wv[2] = wv[3] = 0;
    for (int j = 0; j < CC_PX && i0 + j < HW; ++j) wv[j >> 2] |= (unsigned)a[i0 + j] << (8 * (j & 3));
  }
}

// flag[root of p] = 1 for every strong pixel p; grid (chunks, B).  `parent` is final (cc_compress_kernel is complete):
// parent[p] is p's root.  Every store writes the same value, so their order does not matter.
__global__ void __launch_bounds__(ED_THREADS) edge_seed_kernel(const uint8_t* __restrict__ map, const int* __restrict__ parent, int HW,
                                                              int vec_ok, uint8_t* __restrict__ flag) {
  const int i0 = blockIdx.x * CC_CHUNK + threadIdx.x * CC_PX;
  if (i0 >= HW) return;
  const size_t frame = (size_t)blockIdx.y * HW;
  unsigned wv[4];
  ed_load16(map + frame, i0, HW, vec_ok, wv);
  if (!((wv[0] | wv[1] | wv[2] | wv[3]) & 0x02020202u)) return;
  const int* par = parent + frame;
  int last = -1;
#pragma unroll
  for (int j = 0; j < CC_PX; ++j) {
    if (((wv[j >> 2] >> (8 * (j & 3))) & 0xffu) != 2u) continue;
    const int root = par[i0 + j];            // i0 + j < HW: the map is 0 past the end
    if (root >= 0 && root != last) { flag[frame + root] = 1; last = root; }
  }
}

// out = flag[root] ? 255 : 0; grid (chunks, B), one 16-byte store per thread
__global__ void __launch_bounds__(ED_THREADS) edge_apply_kernel(const int* __restrict__ parent, const uint8_t* __restrict__ flag, int HW,
                                                               int par_vec, int out_vec, uint8_t* __restrict__ out) {
  const int i0 = blockIdx.x * CC_CHUNK + threadIdx.x * CC_PX;
  if (i0 >= HW) return;
  const size_t frame = (size_t)blockIdx.y * HW;
  const uint8_t* fl = flag + frame;
  int p[CC_PX];
  cc_load16(parent + frame, i0, HW, par_vec, p);
  unsigned wv[4] = {0, 0, 0, 0};
  int last = -1;
  unsigned last_v = 0;
#pragma unroll
  for (int j = 0; j < CC_PX; ++j) {
    if (p[j] < 0) continue;
    if (p[j] != last) { last = p[j]; last_v = fl[last] ? 255u : 0u; }
    wv[j >> 2] |= last_v << (8 * (j & 3));
  }
  uint8_t* dst = out + frame;
  if (out_vec && i0 + CC_PX <= HW) {
    *reinterpret_cast<uint4*>(dst + i0) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  } else {
    for (int j = 0; j < CC_PX && i0 + j < HW; ++j) dst[i0 + j] = (uint8_t)((wv[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// src/refactor/burr_detector.py:44-51: out = 255 where band != 0 and (|laplacian| & 255) > threshold, else 0.  The
// Laplacian is cv2's ksize = 1 kernel (4 neighbours - 4 centre) with BORDER_REFLECT_101; `& 255` is what the
// reference's np.abs(lap).astype(np.uint8) does to values above 255.  One thread per 16 pixels of a row;
// grid (ceil(H * ceil(W / 16) / 256), B).
__global__ void __launch_bounds__(ED_THREADS) laplacian_band_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ band,
                                                                   int H, int W, int threshold, int vec_ok, uint8_t* __restrict__ out) {
  const int segs = (W + CC_PX - 1) / CC_PX;
  const int item = blockIdx.x * ED_THREADS + threadIdx.x;
  if (item >= H * segs) return;
  const int y = item / segs, x0 = (item - y * segs) * CC_PX;
  const size_t frame = (size_t)blockIdx.y * H * W;
  const uint8_t* bd = band + frame + (size_t)y * W + x0;
  uint8_t* dst = out + frame + (size_t)y * W + x0;
  unsigned bw[4];
  if (vec_ok) {
    const uint4 v = *reinterpret_cast<const uint4*>(bd);
    bw[0] = v.x; bw[1] = v.y; bw[2] = v.z; bw[3] = v.w;
  } else {
    bw[0] = bw[1] = bw[2] = bw[3] = 0;
    for (int j = 0; j < CC_PX && x0 + j < W; ++j) bw[j >> 2] |= (unsigned)bd[j] << (8 * (j & 3));
  }
  unsigned wv[4] = {0, 0, 0, 0};
  if (bw[0] | bw[1] | bw[2] | bw[3]) {
    const uint8_t* g = gray + frame;
    const uint8_t* up = g + (size_t)ed_reflect(y - 1, H) * W;
    const uint8_t* mid = g + (size_t)y * W;
    const uint8_t* down = g + (size_t)ed_reflect(y + 1, H) * W;
#pragma unroll 4
    for (int j = 0; j < CC_PX; ++j) {
      const int x = x0 + j;
      if (x >= W) break;
      if (!((bw[j >> 2] >> (8 * (j & 3))) & 0xffu)) continue;
      const int lap = (int)up[x] + (int)down[x] + (int)mid[ed_reflect(x - 1, W)] + (int)mid[ed_reflect(x + 1, W)] - 4 * (int)mid[x];
      if ((abs(lap) & 255) > threshold) wv[j >> 2] |= 255u << (8 * (j & 3));
    }
  }
  if (vec_ok) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  } else {
    for (int j = 0; j < CC_PX && x0 + j < W; ++j) dst[j] = (uint8_t)((wv[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// cv2.cvtColor(BGR2GRAY) of OpenCV 4 for uint8: (3735 B + 19235 G + 9798 R + 16384) >> 15 (also enhance.h)
__device__ __forceinline__ int gray_of_bgr(int b, int g, int r) { return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15; }

// One thread per pixel; grid (ceil(HW / 256), B).
__global__ void __launch_bounds__(ED_THREADS) gray_kernel(const uint8_t* __restrict__ bgr, int HW, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * ED_THREADS + threadIdx.x;
  if (i >= HW) return;
  const size_t p = (size_t)blockIdx.y * HW + i;
  const uint8_t* s = bgr + p * 3;
  out[p] = (uint8_t)gray_of_bgr(s[0], s[1], s[2]);
}

}  // namespace unetpp
