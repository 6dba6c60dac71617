// simple_loops.h — the pixel and component rules of the spatial, fixed and simple video loops, on the device:
//   sl_pixel_rules_kernel        relative_threshold (infer_video_spatial.py:71-98) and simple_threshold
//                                (infer_video_simple_v2.py:36-58): three float32 probabilities per pixel -> two uint8 masks
//   sl_keep_select_kernel        keep[] of the area / box-width rule from unetpp_components' stats (cc_apply_kernel writes the mask):
//                                filter_by_size_and_shape (infer_video_fixed.py:85-105) and the tape and burr filters of
//                                infer_video_simple_optimized.py:194-226
//   sl_tape_sums_kernel, sl_tape_filtered_kernel, sl_tape_finish_kernel, sl_tape_apply_kernel
//                                spatial_filter_tape (infer_video_simple_optimized.py:88-137) with its decision in a table
//   sl_column_band_kernel        mask & create_vertical_focus_region (infer_video_spatial.py:56-68, :155-156)
//   sl_join_kernel               masks joined into one map of bits, the input of the merge launch that ends predict
//                                (infer_video_simple.py:148-152, infer_video_simple_optimized.py:228-232)
// Every sum is an integer sum and every extreme an integer maximum: no result depends on the order in which workgroups arrive.
// The float rules are float32 in the order written in simple_loops.py, contraction off.  unet_amd/simple_loops.py holds the
// NumPy forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unetpp {

constexpr int SL_THREADS = 256;
constexpr int SL_WAVE = 64;
constexpr int SL_PX = 4;                                     // consecutive pixels of one frame a thread owns
constexpr int SL_TABLE = 6;                                  // columns of the tape table
enum { SL_RULE_RELATIVE = 0, SL_RULE_CONFIDENCE = 1 };

// ---- 1. the two pixel rules ---------------------------------------------------------------------------------------------------
// np.argmax over three values: the first maximum, and the first NaN when there is one.
__device__ __forceinline__ int sl_argmax3(float v0, float v1, float v2) {
  int best = 0;
  float bv = v0;
  if (bv == bv && (v1 > bv || v1 != v1)) { best = 1; bv = v1; }
  if (bv == bv && (v2 > bv || v2 != v2)) best = 2;
  return best;
}

// (cable, tape) as bits 0 and 1.  a, b: the two ratios (relative) or the threshold twice (confidence), float32 already.
__device__ __forceinline__ unsigned sl_pixel_rule(int rule, float bg, float cable, float tape, float a, float b) {
#pragma clang fp contract(off)
  bool c, t;
  if (rule == SL_RULE_RELATIVE) {
    c = cable > bg * a;
    t = tape > bg * b;
    if (c && t) { c = cable >= tape; t = !c; }
  } else {
    const int winner = sl_argmax3(bg, cable, tape);
    c = winner == 1 && cable >= a;
    t = winner == 2 && tape >= b;
  }
  return (c ? 1u : 0u) | (t ? 2u : 0u);
}

// probs: channel c of pixel i of frame f at probs[f * frame_stride + c * plane_stride + i * pixel_stride] (elements), channels
// 0..2 read.  cable, tape uint8 [B,HW].  Grid (ceil(HW / (SL_THREADS * SL_PX)), B).  The four pixels are read with one 16-byte
// load per plane where pixel_stride is 1 and the address allows it, and written with one 4-byte store where the address does.
__global__ void __launch_bounds__(SL_THREADS) sl_pixel_rules_kernel(const float* __restrict__ probs, long long frame_stride, long long plane_stride,
                                                                   long long pixel_stride, long long HW, int rule, float a, float b,
                                                                   uint8_t* __restrict__ cable, uint8_t* __restrict__ tape) {
  const long long i0 = ((long long)blockIdx.x * SL_THREADS + threadIdx.x) * SL_PX;
  if (i0 >= HW) return;
  const int f = blockIdx.y;
  const int n = (int)(HW - i0 < SL_PX ? HW - i0 : SL_PX);
  const float* p = probs + (long long)f * frame_stride + i0 * pixel_stride;
  float v[3][SL_PX];
  const bool vec_in = pixel_stride == 1 && n == SL_PX && (((uintptr_t)p | (uintptr_t)(p + plane_stride) | (uintptr_t)(p + 2 * plane_stride)) & 15u) == 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* q = p + c * plane_stride;
    if (vec_in) {
      const float4 x = *reinterpret_cast<const float4*>(q);
      v[c][0] = x.x; v[c][1] = x.y; v[c][2] = x.z; v[c][3] = x.w;
    } else {
#pragma unroll
      for (int j = 0; j < SL_PX; ++j) v[c][j] = j < n ? q[j * pixel_stride] : 0.0f;
    }
  }
  unsigned cw = 0, tw = 0;
#pragma unroll
  for (int j = 0; j < SL_PX; ++j) {
    const unsigned r = sl_pixel_rule(rule, v[0][j], v[1][j], v[2][j], a, b);
    cw |= (r & 1u) << (8 * j);
    tw |= ((r >> 1) & 1u) << (8 * j);
  }
  uint8_t* oc = cable + (long long)f * HW + i0;
  uint8_t* ot = tape + (long long)f * HW + i0;
  if (n == SL_PX && ((uintptr_t)oc & 3u) == 0) *reinterpret_cast<unsigned*>(oc) = cw;
  else for (int j = 0; j < n; ++j) oc[j] = (uint8_t)(cw >> (8 * j));
  if (n == SL_PX && ((uintptr_t)ot & 3u) == 0) *reinterpret_cast<unsigned*>(ot) = tw;
  else for (int j = 0; j < n; ++j) ot[j] = (uint8_t)(tw >> (8 * j));
}

// ---- 2. the area / box-width rule -----------------------------------------------------------------------------------------------
// grid (B).  keep uint8 [B,K]: 1 on every component with min_area <= area <= max_area and width >= min_width; a frame with
// num > K keeps nothing.  stats int32 [B,K,5] = LEFT, TOP, WIDTH, HEIGHT, AREA, row 0 the background.
__global__ void __launch_bounds__(SL_THREADS) sl_keep_select_kernel(const int* __restrict__ num, const int* __restrict__ stats, int K, int min_area,
                                                                   int max_area, int min_width, uint8_t* __restrict__ keep) {
  const int b = blockIdx.x;
  const int* st = stats + (size_t)b * K * 5;
  const int n = num[b] <= K ? num[b] : 0;
  for (int l = threadIdx.x; l < K; l += SL_THREADS) {
    bool k = false;
    if (l >= 1 && l < n) {
      const int width = st[(size_t)l * 5 + 2], area = st[(size_t)l * 5 + 4];
      k = area >= min_area && area <= max_area && width >= min_width;
    }
    keep[(size_t)b * K + l] = k ? 1 : 0;
  }
}

// ---- 3. spatial_filter_tape -------------------------------------------------------------------------------------------------------
// The table int32 [B,6] while it is being built (zero before the first launch): {max(W - x) over the cable's non-zero pixels,
// max(x + 1) over them, sum of the tape's values, sum of tape & 1 over the valid columns, 0, 0}; 0 in the first two = no cable.
// sl_tape_finish_kernel rewrites it as {x_min, x_max, original_area, filtered_area, verdict, 0}.
struct SlRanges { int l0, l1, r0, r1; };

// the two column ranges of :116-121 from the cable's extent (all values non-negative: C division is Python's //)
__device__ __forceinline__ SlRanges sl_ranges(int x_min, int x_max, int W) {
  const int cw = x_max - x_min;
  SlRanges r;
  r.l0 = max(0, x_min - cw / 2);
  r.l1 = x_min + cw / 3;
  r.r0 = max(x_min + 2 * cw / 3, x_max - cw / 3);
  r.r1 = min(W, x_max + cw / 2);
  return r;
}
__device__ __forceinline__ bool sl_valid(const SlRanges& r, int x) { return (x >= r.l0 && x < r.l1) || (x >= r.r0 && x < r.r1); }
// a mask byte as the filter reads it: the byte itself for match < 0, else 1 where it equals match and 0 where it does not
__device__ __forceinline__ unsigned sl_read(unsigned v, int match) { return match < 0 ? v : (v == (unsigned)match ? 1u : 0u); }

// grid (ceil(H / 4), B): one wave per row.
__global__ void __launch_bounds__(SL_THREADS) sl_tape_sums_kernel(const uint8_t* __restrict__ tape, int tape_match, const uint8_t* __restrict__ cable,
                                                                 int cable_match, int H, int W, int* __restrict__ table) {
  const int wave = threadIdx.x / SL_WAVE, lane = threadIdx.x % SL_WAVE;
  const int y = blockIdx.x * (SL_THREADS / SL_WAVE) + wave, b = blockIdx.y;
  if (y >= H) return;
  const size_t row = ((size_t)b * H + y) * W;
  int lo = 0, hi = 0, sum = 0;
  for (int x = lane; x < W; x += SL_WAVE) {
    if (sl_read(cable[row + x], cable_match)) { lo = max(lo, W - x); hi = x + 1; }
    sum += (int)sl_read(tape[row + x], tape_match);
  }
#pragma unroll
  for (int d = SL_WAVE / 2; d > 0; d >>= 1) {
    lo = max(lo, __shfl_xor(lo, d, SL_WAVE));
    hi = max(hi, __shfl_xor(hi, d, SL_WAVE));
    sum += __shfl_xor(sum, d, SL_WAVE);
  }
  if (lane == 0) {
    int* t = table + (size_t)b * SL_TABLE;
    if (hi) { atomicMax(&t[0], lo); atomicMax(&t[1], hi); }
    if (sum) atomicAdd(&t[2], sum);
  }
}

// grid (ceil(H / 4), B): one wave per row; reads the extent the launch before completed.
__global__ void __launch_bounds__(SL_THREADS) sl_tape_filtered_kernel(const uint8_t* __restrict__ tape, int tape_match, int H, int W,
                                                                     int* __restrict__ table) {
  const int wave = threadIdx.x / SL_WAVE, lane = threadIdx.x % SL_WAVE;
  const int y = blockIdx.x * (SL_THREADS / SL_WAVE) + wave, b = blockIdx.y;
  if (y >= H) return;
  int* t = table + (size_t)b * SL_TABLE;
  if (t[1] == 0 || t[2] == 0) return;                        // no cable or no tape: the frame is returned as it came
  const SlRanges r = sl_ranges(W - t[0], t[1] - 1, W);
  const size_t row = ((size_t)b * H + y) * W;
  int sum = 0;
  for (int x = lane; x < W; x += SL_WAVE)
    if (sl_valid(r, x)) sum += (int)(sl_read(tape[row + x], tape_match) & 1u);
#pragma unroll
  for (int d = SL_WAVE / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d, SL_WAVE);
  if (lane == 0 && sum) atomicAdd(&t[3], sum);
}

// grid (ceil(B / SL_THREADS)): one thread per frame.  verdict = 1 where the filtered tape is the result.
__global__ void __launch_bounds__(SL_THREADS) sl_tape_finish_kernel(int B, int W, int* __restrict__ table) {
  const int b = blockIdx.x * SL_THREADS + threadIdx.x;
  if (b >= B) return;
  int* t = table + (size_t)b * SL_TABLE;
  const bool some = t[1] != 0;
  const int original = t[2], filtered = t[3];
  t[0] = some ? W - t[0] : -1;
  t[1] = some ? t[1] - 1 : -1;
  t[4] = (some && original > 0 && !(2LL * filtered < (long long)original)) ? 1 : 0;
  t[5] = 0;
}

// grid (ceil(W / 1024), H, B), four pixels per thread.  With t the tape as sl_read gives it: out = t & 1 in the valid columns and
// 0 in the others where the verdict is 1, t itself where it is 0.
__global__ void __launch_bounds__(SL_THREADS) sl_tape_apply_kernel(const uint8_t* __restrict__ tape, int tape_match, const int* __restrict__ table,
                                                                  int H, int W, int vec, uint8_t* __restrict__ out) {
  const int x0 = (blockIdx.x * SL_THREADS + threadIdx.x) * 4, y = blockIdx.y, b = blockIdx.z;
  if (x0 >= W) return;
  const int* t = table + (size_t)b * SL_TABLE;
  const bool filter = t[4] != 0;
  SlRanges r{0, 0, 0, 0};
  if (filter) r = sl_ranges(t[0], t[1], W);
  const size_t at = ((size_t)b * H + y) * W + x0;
  const int n = min(4, W - x0);
  unsigned in = 0, res = 0;
  if (vec) in = *reinterpret_cast<const unsigned*>(tape + at);      // W % 4 == 0 and both pointers 4-byte aligned
  else for (int j = 0; j < n; ++j) in |= (unsigned)tape[at + j] << (8 * j);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned v = sl_read((in >> (8 * j)) & 0xffu, tape_match);
    res |= (filter ? (sl_valid(r, x0 + j) ? (v & 1u) : 0u) : v) << (8 * j);
  }
  if (vec) *reinterpret_cast<unsigned*>(out + at) = res;
  else for (int j = 0; j < n; ++j) out[at + j] = (uint8_t)(res >> (8 * j));
}

// ---- 4. the focus band --------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 1024), H, B), four pixels per thread.  out = mask & 1 in columns [x_start, x_end), 0 in the others.
__global__ void __launch_bounds__(SL_THREADS) sl_column_band_kernel(const uint8_t* __restrict__ mask, int H, int W, int x_start, int x_end, int vec,
                                                                   uint8_t* __restrict__ out) {
  const int x0 = (blockIdx.x * SL_THREADS + threadIdx.x) * 4, y = blockIdx.y, b = blockIdx.z;
  if (x0 >= W) return;
  const size_t at = ((size_t)b * H + y) * W + x0;
  if (vec) {                                                 // W % 4 == 0 and both pointers 4-byte aligned
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j >= x_start && x0 + j < x_end) keep |= 1u << (8 * j);
    *reinterpret_cast<unsigned*>(out + at) = *reinterpret_cast<const unsigned*>(mask + at) & keep;
  } else {
    for (int j = 0; j < 4 && x0 + j < W; ++j) out[at + j] = (x0 + j >= x_start && x0 + j < x_end) ? (uint8_t)(mask[at + j] & 1) : (uint8_t)0;
  }
}

// ---- 5. joining masks into one map of bits ----------------------------------------------------------------------------------------------
// n bytes, flat.  out = (a & and_a) | (b != 0 ? or_b : 0) | (c != 0 ? or_c : 0); b and c may be NULL.  Grid (ceil(n / 1024)), four
// bytes per thread; vec = n % 4 == 0 and every pointer 4-byte aligned.
__global__ void __launch_bounds__(SL_THREADS) sl_join_kernel(const uint8_t* __restrict__ a, unsigned and_a, const uint8_t* __restrict__ b,
                                                            unsigned or_b, const uint8_t* __restrict__ c, unsigned or_c, long long n, int vec,
                                                            uint8_t* __restrict__ out) {
  const long long i0 = ((long long)blockIdx.x * SL_THREADS + threadIdx.x) * 4;
  if (i0 >= n) return;
  const int m = (int)(n - i0 < 4 ? n - i0 : 4);
  unsigned va = 0, vb = 0, vc = 0, res = 0;
  if (vec) {
    va = *reinterpret_cast<const unsigned*>(a + i0);
    if (b) vb = *reinterpret_cast<const unsigned*>(b + i0);
    if (c) vc = *reinterpret_cast<const unsigned*>(c + i0);
  } else {
    for (int j = 0; j < m; ++j) {
      va |= (unsigned)a[i0 + j] << (8 * j);
      if (b) vb |= (unsigned)b[i0 + j] << (8 * j);
      if (c) vc |= (unsigned)c[i0 + j] << (8 * j);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned x = ((va >> (8 * j)) & and_a & 0xffu) | (((vb >> (8 * j)) & 0xffu) ? or_b : 0u) | (((vc >> (8 * j)) & 0xffu) ? or_c : 0u);
    res |= (x & 0xffu) << (8 * j);
  }
  if (vec) *reinterpret_cast<unsigned*>(out + i0) = res;
  else for (int j = 0; j < m; ++j) out[i0 + j] = (uint8_t)(res >> (8 * j));
}

}  // namespace unetpp
