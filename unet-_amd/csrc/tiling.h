// tiling.h — sliding-window inference on the device (SlidingWindowInference.predict, tools/inference_binary_patch.py:
// 19-115; OptimizedSlidingWindowInference.predict, tools/inference_binary_optimized.py:21-113): cut frames into the
// patch batch, gate patches, fold the per-patch maps back into one image.  unet_amd/tiling.py is the NumPy form.
//
//   tile_gather_u8_kernel   frames uint8 [B,H,W,3] -> patches uint8 [B*P,T,T,3]: crop at the patch origin, np.pad's
//                           reflect at the bottom and right (k >= H reads 2 (H - 1) - k), cv2's uint8 INTER_LINEAR
//                           resize patch_size -> T with the integer tables of resize_linear_u8_kernel, optional
//                           channel reversal; a thread produces 4 consecutive output bytes
//   tile_gate_f32_kernel    one workgroup per patch: score = max over T x T of maps[n, gate_class], include = score >= thr
//   tile_blend_f32_kernel   gather form, one thread per output pixel: for every patch that covers the pixel, in plan
//                           order (i outer, j inner), the bilinear sample of its [C,T,T] map at the patch-local
//                           coordinate (horizontal pass first, then vertical, float tables of the host) is added to a
//                           float32 accumulator per class; then acc / (count + 1e-8f), IEEE division, first maximum.
//
// The order of the additions is fixed per pixel by the plan, so the blend needs no atomics, no workgroup waits for
// another, and the bits do not depend on scheduling.  The blend is compiled without contraction (the pragma sits in the
// kernel's body, so that it ends with it): a * b + c * d must round each product, as NumPy does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unetpp {

constexpr int TILE_MAX_AXIS = 64;      // patch origins per axis
constexpr int TILE_MAX_CLASSES = 8;
constexpr int TILE_THREADS = 256;
constexpr int TILE_WAVE = 64;
constexpr int TILE_BLEND_ROWS = TILE_THREADS / TILE_WAVE;     // a workgroup of the blend is 64 x 4 pixels

struct TilePlan {                      // patch (i, j) starts at (oy[i], ox[j]); its index in a frame is i * nx + j
  int ny, nx;
  int oy[TILE_MAX_AXIS], ox[TILE_MAX_AXIS];
};

// grid (ceil(3 T / 1024), T, B * P), 256 threads.  xtab / ytab: resize tables patch_size -> T, {s0, s1, a0, a1}.
// The host has checked that every origin o satisfies 0 <= o and o + patch_size - 1 <= 2 (n - 1) on its axis.
__global__ void __launch_bounds__(TILE_THREADS) tile_gather_u8_kernel(const uint8_t* __restrict__ frames, int H, int W, TilePlan plan,
                                                                     int T, int swap_rb, const int4* __restrict__ xtab,
                                                                     const int4* __restrict__ ytab, uint8_t* __restrict__ patches) {
  const int row_bytes = T * 3;
  const int i0 = (blockIdx.x * TILE_THREADS + threadIdx.x) * 4;
  if (i0 >= row_bytes) return;
  const int P = plan.ny * plan.nx;
  const int n = blockIdx.z, b = n / P, p = n - b * P;
  const int oy = plan.oy[p / plan.nx], ox = plan.ox[p % plan.nx];
  const int dy = blockIdx.y;
  const int4 yt = ytab[dy];
  int y0 = oy + yt.x, y1 = oy + yt.y;
  if (y0 >= H) y0 = 2 * (H - 1) - y0;
  if (y1 >= H) y1 = 2 * (H - 1) - y1;
  const uint8_t* r0 = frames + ((size_t)b * H + y0) * (size_t)W * 3;
  const uint8_t* r1 = frames + ((size_t)b * H + y1) * (size_t)W * 3;
  uint32_t packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {                              // 3 T is a multiple of 4: the four bytes exist
    const int i = i0 + j;
    const int dx = i / 3, c = i - dx * 3;
    const int cs = swap_rb ? 2 - c : c;
    const int4 xt = xtab[dx];
    int x0 = ox + xt.x, x1 = ox + xt.y;
    if (x0 >= W) x0 = 2 * (W - 1) - x0;
    if (x1 >= W) x1 = 2 * (W - 1) - x1;
    const int S0 = (int)r0[x0 * 3 + cs] * xt.z + (int)r0[x1 * 3 + cs] * xt.w;
    const int S1 = (int)r1[x0 * 3 + cs] * xt.z + (int)r1[x1 * 3 + cs] * xt.w;
    int v = (((yt.z * (S0 >> 4)) >> 16) + ((yt.w * (S1 >> 4)) >> 16) + 2) >> 2;
    v = min(max(v, 0), 255);
    packed |= (uint32_t)v << (8 * j);
  }
  *reinterpret_cast<uint32_t*>(patches + ((size_t)n * T + dy) * (size_t)row_bytes + i0) = packed;
}

// grid (N), 256 threads.  maps float32 [N,C,T,T] -> scores float32 [N], include uint8 [N].
__global__ void __launch_bounds__(TILE_THREADS) tile_gate_f32_kernel(const float* __restrict__ maps, int C, int T, int gate_class,
                                                                    float thr, float* __restrict__ scores,
                                                                    uint8_t* __restrict__ include) {
  __shared__ float s_max[TILE_THREADS / TILE_WAVE];
  const int n = blockIdx.x, t = threadIdx.x;
  const int count = T * T;                                   // a multiple of 4: T is even, and the host checked the alignment
  const float4* src = reinterpret_cast<const float4*>(maps + ((size_t)n * C + gate_class) * (size_t)count);
  float m = -INFINITY;
  for (int i = t; i < count / 4; i += TILE_THREADS) {
    const float4 v = src[i];
    m = fmaxf(fmaxf(m, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
  }
#pragma unroll
  for (int d = TILE_WAVE / 2; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, TILE_WAVE));
  if (t % TILE_WAVE == 0) s_max[t / TILE_WAVE] = m;
  __syncthreads();
  if (t == 0) {
    m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    scores[n] = m;
    include[n] = m >= thr ? 1 : 0;
  }
}

// grid (ceil(W / 64), ceil(H / 4), B), 256 threads: thread (x, y) of the 64 x 4 workgroup owns one output pixel, so a
// wave reads consecutive columns of one map row (taps T / patch_size apart) and writes 64 consecutive pixels.
// maps float32 [B*P,C,T,T]; xtab / ytab: float resize tables T -> patch_size, {s0, s1, bits(a0), bits(a1)};
// include uint8 [B*P] or nullptr; mask uint8 [B,H,W]; output float32 [B,H,W,C] or nullptr.
template <int C>
__global__ void __launch_bounds__(TILE_THREADS) tile_blend_f32_kernel(const float* __restrict__ maps, TilePlan plan, int patch_size, int T,
                                                                     const int4* __restrict__ xtab, const int4* __restrict__ ytab,
                                                                     const uint8_t* __restrict__ include, int H, int W,
                                                                     uint8_t* __restrict__ mask, float* __restrict__ output) {
#pragma clang fp contract(off)
  const int X = blockIdx.x * TILE_WAVE + threadIdx.x % TILE_WAVE;
  const int Y = blockIdx.y * TILE_BLEND_ROWS + threadIdx.x / TILE_WAVE;
  if (X >= W || Y >= H) return;
  const int b = blockIdx.z, P = plan.ny * plan.nx;
  const size_t plane = (size_t)T * T;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0f;
  float count = 0.0f;
  for (int i = 0; i < plan.ny; ++i) {
    const int ly = Y - plan.oy[i];
    if ((unsigned)ly >= (unsigned)patch_size) continue;
    const int4 yt = ytab[ly];
    const float b0 = __int_as_float(yt.z), b1 = __int_as_float(yt.w);
    for (int j = 0; j < plan.nx; ++j) {
      const int lx = X - plan.ox[j];
      if ((unsigned)lx >= (unsigned)patch_size) continue;
      const size_t n = (size_t)b * P + (size_t)(i * plan.nx + j);
      if (include && !include[n]) continue;
      const int4 xt = xtab[lx];
      const float a0 = __int_as_float(xt.z), a1 = __int_as_float(xt.w);
      const float* m0 = maps + n * C * plane + (size_t)yt.x * T;
      const float* m1 = maps + n * C * plane + (size_t)yt.y * T;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float h0 = m0[c * plane + xt.x] * a0 + m0[c * plane + xt.y] * a1;
        const float h1 = m1[c * plane + xt.x] * a0 + m1[c * plane + xt.y] * a1;
        acc[c] = acc[c] + (h0 * b0 + h1 * b1);
      }
      count = count + 1.0f;
    }
  }
  const float denom = count + 1e-8f;
  const size_t px = ((size_t)b * H + Y) * (size_t)W + X;
  int best = 0;
  float best_v = 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float v = acc[c] / denom;                          // correctly rounded: hipcc's default for fp32 division
    if (output) output[px * C + c] = v;
    if (c == 0 || v > best_v) { best_v = v; best = c; }
  }
  mask[px] = (uint8_t)best;
}

}  // namespace unetpp
