// loss.h — the five sums per frame and class that every loss of the reference's src/models/losses.py is a function of
// (cross-entropy, Dice, Focal, Tversky and their two combinations): one pass over float32 logits [B,C,H W] and a uint8
// target [B,H W].  include/unetpp_loss.h states the arithmetic; unet_amd/loss.py (loss_sums_np) performs the same float32
// operations in NumPy and returns the same bits.  Every accumulation is an integer sum: no result depends on the order in
// which threads, waves or workgroups arrive.
//
// Overflow, for H W <= 2^22 pixels per frame: T <= 2^22; a pixel adds at most 2^32 to P and I (p <= 1), so they stay below
// 2^54; a pixel adds at most rint(131072 * 2^24) = 2^41 to NLL and FOC (the clamp), so they stay at or below 2^63.  The
// per-thread, per-wave and per-workgroup partial sums are parts of those and bounded by them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace unetpp {

constexpr int LS_THREADS = 256, LS_WAVES = LS_THREADS / 64;
constexpr int LS_GROUP = 4;                                   // pixels per load: 16 bytes of a class plane, 4 of the target
constexpr int LS_ITERS = 4;                                   // groups per thread
constexpr int LS_SPAN = LS_THREADS * LS_GROUP * LS_ITERS;     // positions one workgroup owns (4096)
constexpr int LS_MAX_CLASSES = 8, LS_COLUMNS = 5;             // columns: T, P, I, NLL, FOC
constexpr int LS_MAX_GAMMA = 4;
constexpr unsigned LS_MAX_PIXELS = 1u << 22;

// exp(d) for d <= 0 (Cephes expf as explicit float32 operations, never fused): 0 below -87, else 2^n * (1 + r + r^2 poly(r))
// with n = rint(d log2 e) and r = (d - n C1) - n C2, ln 2 = C1 + C2.  The result is a normal number, so ldexpf is exact.
__device__ __forceinline__ float ls_exp32(float d) {
#pragma clang fp contract(off)
  const float x = fmaxf(d, -87.0f);
  const float n = rintf(0x1.715476p+0f * x);                  // log2 e
  float r = x - n * 0x1.63p-1f;                               // C1 = 0.693359375
  r = r - n * -0x1.bd0106p-13f;                               // C2 = -2.12194440e-4
  float q = 0x1.a0d2cep-13f;                                  // 1.9875691500e-4
  q = q * r + 0x1.6e879cp-10f;                                // 1.3981999507e-3
  q = q * r + 0x1.111210p-7f;                                 // 8.3334519073e-3
  q = q * r + 0x1.555382p-5f;                                 // 4.1665795894e-2
  q = q * r + 0x1.555554p-3f;                                 // 1.6666665459e-1
  q = q * r + 0.5f;                                           // 5.0000001201e-1 rounds to 0.5
  float y = q * (r * r) + r;
  y = y + 1.0f;
  return d < -87.0f ? 0.0f : ldexpf(y, (int)n);
}

// log(s) for s >= 1 (Cephes logf, the same way): s = f 2^e with f in [0.5, 1); below sqrt(1/2) e -= 1 and x = (f + f) - 1,
// else x = f - 1; y = poly(x) x x^2 + e C2 - x^2 / 2; log = (x + y) + e C1.  ls_log32(1) == 0.
__device__ __forceinline__ float ls_log32(float s) {
#pragma clang fp contract(off)
  int e;
  const float f = frexpf(s, &e);
  const bool low = f < 0x1.6a09e6p-1f;                        // sqrt(1/2)
  const float fe = (float)(e - (low ? 1 : 0));
  const float x = (low ? f + f : f) - 1.0f;
  const float z = x * x;
  float q = 0x1.204376p-4f;                                   // 7.0376836292e-2
  q = q * x + -0x1.d7a370p-4f;                                // -1.1514610310e-1
  q = q * x + 0x1.de4a34p-4f;                                 // 1.1676998740e-1
  q = q * x + -0x1.fcba9ep-4f;                                // -1.2420140846e-1
  q = q * x + 0x1.23d37ep-3f;                                 // 1.4249322787e-1
  q = q * x + -0x1.555ca0p-3f;                                // -1.6668057665e-1
  q = q * x + 0x1.999d58p-3f;                                 // 2.0000714765e-1
  q = q * x + -0x1.fffff8p-3f;                                // -2.4999993993e-1
  q = q * x + 0x1.555554p-2f;                                 // 3.3333331174e-1
  float y = q * x * z;
  y = y + -0x1.bd0106p-13f * fe;
  y = y + -0.5f * z;
  const float r = x + y;
  return r + 0x1.63p-1f * fe;
}

// floor(p 2^32) for 0 <= p <= 1: the product is exact, and below 2^32 unless p == 1
__device__ __forceinline__ unsigned long long ls_q32(float p) {
  const float v = p * 4294967296.0f;
  return v >= 4294967296.0f ? (1ull << 32) : (unsigned long long)(unsigned)fminf(v, 4294967040.0f);
}

// rint(min(v, 131072) 2^24) for v >= 0 (+inf included): the product is exact, at most 2^41
__device__ __forceinline__ unsigned long long ls_q24(float v) { return (unsigned long long)rintf(fminf(v, 131072.0f) * 16777216.0f); }

__device__ __forceinline__ unsigned long long ls_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// table[frame][c] += (T, P, I, NLL, FOC); outside[frame] += (pixels with target >= C, the others with a non-finite logit).
// Both are zeroed before the launch.  Grid (ceil((HW + 3) / LS_SPAN), B); 2 <= C <= 8, 0 <= gamma <= 4, HW <= 2^22.  One
// instantiation per class count: the class loops unroll to C without a branch and a 3-class frame does not pay for the
// registers of 8 (DESIGN.md 5.21 has both forms measured).
//
// Positions.  A workgroup owns LS_SPAN consecutive positions of one frame; position q holds pixel q - pad, where pad
// (0..3) is the element offset of the frame's class-0 plane from a 16-byte boundary.  So every group of 4 positions of
// plane 0 starts on a 16-byte boundary whatever b C HW is.  Alignment is handled PER PLANE: plane c of the frame lies c HW
// elements further, so it shares plane 0's alignment exactly when c HW is a multiple of 4; such a plane is read with one
// 16-byte load per group, any other plane with four 4-byte loads, and so are the groups that hang over the frame's head or
// tail (inside the frame only).  The target is read 4 bytes per group when the group's first byte is 4-byte aligned, else
// byte by byte.
//
// Sums.  Each thread keeps the C sums of P in 64-bit registers.  The target-class terms (T, I, NLL, FOC) go to the run the
// thread is in (a real target is mostly one class); when the class changes the run is added to the wave's LDS table with
// 64-bit LDS adds, and at the end a wave whose runs agree adds one reduced run.  P and the outside counters are reduced
// across the wave by shuffles.  The workgroup then issues one global 64-bit atomic per non-zero entry.
template <int C>
__global__ void __launch_bounds__(LS_THREADS) loss_sums_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ target, unsigned HW_,
                                                              int gamma, unsigned long long* __restrict__ table,
                                                              unsigned* __restrict__ outside) {
#pragma clang fp contract(off)
  __shared__ unsigned long long acc[LS_WAVES][LS_MAX_CLASSES][LS_COLUMNS];
  __shared__ unsigned out_n[LS_WAVES][2];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const long long HW = HW_;
  const size_t frame = blockIdx.y;
  const float* lf = logits + frame * (size_t)C * HW_;
  const uint8_t* tf = target + frame * HW_;
  const int pad = (int)(((uintptr_t)lf >> 2) & 3u);
  const long long first = (long long)blockIdx.x * LS_SPAN - pad;
  if (first >= HW) return;                                      // the spare workgroup of a frame with a small pad
  for (int j = t; j < LS_WAVES * LS_MAX_CLASSES * LS_COLUMNS; j += LS_THREADS) (&acc[0][0][0])[j] = 0;
  if (t < LS_WAVES * 2) (&out_n[0][0])[t] = 0;
  __syncthreads();
  const bool target_vec = (((long long)(uintptr_t)tf + first) & 3) == 0;

  unsigned long long P[LS_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < LS_MAX_CLASSES; ++c) P[c] = 0;
  int run_c = 0;
  unsigned run_t = 0, bad_target = 0, bad_logit = 0;
  unsigned long long run_i = 0, run_nll = 0, run_foc = 0;
  unsigned long long* mine = &acc[wave][0][0];
  auto flush = [&]() {
    unsigned long long* row = mine + run_c * LS_COLUMNS;
    atomicAdd(row + 0, (unsigned long long)run_t);
    atomicAdd(row + 2, run_i);
    atomicAdd(row + 3, run_nll);
    atomicAdd(row + 4, run_foc);
  };

#pragma unroll 1
  for (int it = 0; it < LS_ITERS; ++it) {
    const long long i0 = first + (long long)(it * LS_THREADS + t) * LS_GROUP;
    if (i0 >= HW) break;
    const bool full = i0 >= 0 && i0 + LS_GROUP <= HW;
    float x[LS_MAX_CLASSES][LS_GROUP];
#pragma unroll
    for (int c = 0; c < LS_MAX_CLASSES; ++c) {
      if (c < C) {
        const float* p = lf + (size_t)c * HW_;
        if (full && (((unsigned)c * HW_) & 3u) == 0) {
          const float4 v = *reinterpret_cast<const float4*>(p + i0);
          x[c][0] = v.x; x[c][1] = v.y; x[c][2] = v.z; x[c][3] = v.w;
        } else {
#pragma unroll
          for (int j = 0; j < LS_GROUP; ++j) x[c][j] = (i0 + j >= 0 && i0 + j < HW) ? p[i0 + j] : 0.0f;
        }
      }
    }
    unsigned tw = 0;
    if (full && target_vec) {
      tw = *reinterpret_cast<const unsigned*>(tf + i0);
    } else {
#pragma unroll
      for (int j = 0; j < LS_GROUP; ++j)
        if (i0 + j >= 0 && i0 + j < HW) tw |= (unsigned)tf[i0 + j] << (8 * j);
    }
#pragma unroll
    for (int j = 0; j < LS_GROUP; ++j) {
      if (i0 + j < 0 || i0 + j >= HW) continue;
      const int tv = (int)((tw >> (8 * j)) & 0xffu);
      if (tv >= C) { ++bad_target; continue; }
      unsigned nonfinite = 0;
#pragma unroll
      for (int c = 0; c < LS_MAX_CLASSES; ++c)
        if (c < C) nonfinite |= (unsigned)((__float_as_uint(x[c][j]) & 0x7f800000u) == 0x7f800000u);
      if (nonfinite) { ++bad_logit; continue; }
      float m = x[0][j];
#pragma unroll
      for (int c = 1; c < LS_MAX_CLASSES; ++c)
        if (c < C) m = x[c][j] > m ? x[c][j] : m;
      float e[LS_MAX_CLASSES];
      float s = 0.0f, d_t = 0.0f, p_t = 0.0f;
#pragma unroll
      for (int c = 0; c < LS_MAX_CLASSES; ++c) {
        if (c < C) {
          const float d = x[c][j] - m;                          // -inf when the difference leaves float32: e = 0
          e[c] = ls_exp32(d);
          s = c == 0 ? e[0] : s + e[c];
          if (c == tv) d_t = d;
        }
      }
      unsigned long long q_t = 0;
#pragma unroll
      for (int c = 0; c < LS_MAX_CLASSES; ++c) {
        if (c < C) {
          const float p = __fdiv_rn(e[c], s);
          const unsigned long long q = ls_q32(p);
          P[c] += q;
          if (c == tv) { p_t = p; q_t = q; }
        }
      }
      const float nll = fmaxf(0.0f, ls_log32(s) - d_t);
      const float om = 1.0f - p_t;
      float wgt = 1.0f;
#pragma unroll
      for (int g = 0; g < LS_MAX_GAMMA; ++g)
        if (g < gamma) wgt = wgt * om;
      const float foc = wgt * nll;
      if (tv != run_c) {
        if (run_t) flush();
        run_c = tv;
        run_t = 0;
        run_i = run_nll = run_foc = 0;
      }
      ++run_t;
      run_i += q_t;
      run_nll += ls_q24(nll);
      run_foc += ls_q24(foc);
    }
  }

  // the run each thread is still in: one reduced add per wave when all of its runs are of one class
  const unsigned long long has = __ballot(run_t != 0);
  if (has) {
    const int k0 = __shfl(run_c, __ffsll((long long)has) - 1, 64);
    if (__all(run_t == 0 || run_c == k0)) {
      const unsigned long long n = ls_wave_sum((unsigned long long)run_t), si = ls_wave_sum(run_i), sn = ls_wave_sum(run_nll),
                               sf = ls_wave_sum(run_foc);
      if (lane == 0) { run_c = k0; run_t = (unsigned)n; run_i = si; run_nll = sn; run_foc = sf; flush(); }
    } else if (run_t) {
      flush();
    }
  }
#pragma unroll
  for (int c = 0; c < LS_MAX_CLASSES; ++c) {
    if (c < C) {
      const unsigned long long sp = ls_wave_sum(P[c]);
      if (lane == 0) mine[c * LS_COLUMNS + 1] = sp;              // the only writer of this entry
    }
  }
  const unsigned long long nb = ls_wave_sum(((unsigned long long)bad_target << 32) | bad_logit);      // each below 2^13 per wave
  if (lane == 0) { out_n[wave][0] = (unsigned)(nb >> 32); out_n[wave][1] = (unsigned)nb; }
  __syncthreads();
  if (t < C * LS_COLUMNS) {
    unsigned long long n = 0;
#pragma unroll
    for (int wv = 0; wv < LS_WAVES; ++wv) n += (&acc[wv][0][0])[t];
    if (n) atomicAdd(table + frame * (size_t)(C * LS_COLUMNS) + t, n);
  } else if (t >= 64 && t < 66) {
    unsigned n = 0;
#pragma unroll
    for (int wv = 0; wv < LS_WAVES; ++wv) n += out_n[wv][t - 64];
    if (n) atomicAdd(outside + frame * 2 + (t - 64), n);
  }
}

}  // namespace unetpp
