// loss_grad.h — the gradient of the reference's criteria (CombinedLoss, AdvancedCombinedLoss of src/models/losses.py) with
// respect to the logits, in one pass: float32 logits [B,C,H W] and a uint8 target [B,H W] are read once, the float32 gradient
// [B,C,H W] is written once.  include/unetpp_loss_grad.h states the arithmetic; unet_amd/loss_grad.py (loss_grad_np) performs
// the same float32 operations in NumPy and returns the same bits.  Everything that couples pixels (the Dice and Tversky
// ratios, the means of cross-entropy and Focal) is in the coefficient table coef [B,C,4] = (A, G, K_ce, K_foc) the host
// derives from the five sums of loss.h, so a pixel's gradient depends on that pixel alone: no atomics, no arrival order.
// The softmax, exp32 and log32 are those of loss.h (included, not copied), as is the position scheme.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "loss.h"

namespace unetpp {

constexpr int LG_COEF = 4;                                    // A, G, K_ce, K_foc per (frame, class)

// grad[frame][c][pixel], every element exactly once.  Grid (ceil((HW + 3) / LS_SPAN), B), as loss_sums_kernel<C>.
//
// Positions are those of loss.h: a workgroup owns LS_SPAN positions of a frame, position q holds pixel q - pad with pad the
// element offset of the frame's class-0 LOGIT plane from a 16-byte boundary; a plane of the logits is read with 16-byte
// loads when c HW is a multiple of 4.  The gradient has a phase of its own: plane c of the gradient frame is written with
// 16-byte stores when (gpad + c HW - pad) is a multiple of 4 (gpad the same offset of the gradient frame) and the group
// lies wholly inside the frame, else element by element inside the frame only.
//
// grad == logits is allowed (the entry refuses any other overlap): a thread reads all C values of its four pixels before it
// stores any, and no other thread touches those pixels.  Hence neither pointer is __restrict__.
template <int C>
__global__ void __launch_bounds__(LS_THREADS) loss_grad_kernel(const float* logits, const uint8_t* __restrict__ target, unsigned HW_, int gamma,
                                                              const float* __restrict__ coef, const float* __restrict__ scale_p, float* grad) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  const long long HW = HW_;
  const size_t frame = blockIdx.y;
  const float* lf = logits + frame * (size_t)C * HW_;
  float* gf = grad + frame * (size_t)C * HW_;
  const uint8_t* tf = target + frame * HW_;
  const unsigned pad = (unsigned)(((uintptr_t)lf >> 2) & 3u), gpad = (unsigned)(((uintptr_t)gf >> 2) & 3u);
  const long long first = (long long)blockIdx.x * LS_SPAN - (long long)pad;
  if (first >= HW) return;                                      // the spare workgroup of a frame with a small pad
  const bool target_vec = (((long long)(uintptr_t)tf + first) & 3) == 0;
  const bool scaled = scale_p != nullptr;
  const float scale = scaled ? *scale_p : 1.0f;
  const float gam = (float)gamma;
  float A[LS_MAX_CLASSES], G[LS_MAX_CLASSES], KC[LS_MAX_CLASSES], KF[LS_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < LS_MAX_CLASSES; ++c) {
    if (c < C) {
      const float* k = coef + (frame * (size_t)C + c) * LG_COEF;
      A[c] = k[0]; G[c] = k[1]; KC[c] = k[2]; KF[c] = k[3];
    }
  }

#pragma unroll 1
  for (int it = 0; it < LS_ITERS; ++it) {
    const long long i0 = first + (long long)(it * LS_THREADS + t) * LS_GROUP;
    if (i0 >= HW) break;
    const bool full = i0 >= 0 && i0 + LS_GROUP <= HW;
    float x[LS_MAX_CLASSES][LS_GROUP];                          // the logits, then the gradient
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
      unsigned special = (unsigned)(tv >= C);
#pragma unroll
      for (int c = 0; c < LS_MAX_CLASSES; ++c)
        if (c < C) special |= (unsigned)((__float_as_uint(x[c][j]) & 0x7f800000u) == 0x7f800000u);
      if (special) {                                            // the pixels the forward leaves out of every sum
#pragma unroll
        for (int c = 0; c < LS_MAX_CLASSES; ++c)
          if (c < C) x[c][j] = 0.0f;
        continue;
      }
      float m = x[0][j];
#pragma unroll
      for (int c = 1; c < LS_MAX_CLASSES; ++c)
        if (c < C) m = x[c][j] > m ? x[c][j] : m;
      float e[LS_MAX_CLASSES];
      float s = 0.0f, d_t = 0.0f, p_t = 0.0f, a_t = 0.0f, kc_t = 0.0f, kf_t = 0.0f;
#pragma unroll
      for (int c = 0; c < LS_MAX_CLASSES; ++c) {
        if (c < C) {
          const float d = x[c][j] - m;                          // -inf when the difference leaves float32: e = 0
          e[c] = ls_exp32(d);
          s = c == 0 ? e[0] : s + e[c];
          if (c == tv) { d_t = d; a_t = A[c]; kc_t = KC[c]; kf_t = KF[c]; }
        }
      }
      float dot = 0.0f;
#pragma unroll
      for (int c = 0; c < LS_MAX_CLASSES; ++c) {
        if (c < C) {
          const float p = __fdiv_rn(e[c], s);
          e[c] = p;
          if (c == tv) p_t = p;
          const float u = c == tv ? G[c] + a_t : G[c];
          const float pu = p * u;
          dot = c == 0 ? pu : dot + pu;
        }
      }
      const float nll = fminf(fmaxf(0.0f, ls_log32(s) - d_t), 131072.0f);
      const float om = 1.0f - p_t;
      float w1 = 1.0f;
#pragma unroll
      for (int g = 1; g < LS_MAX_GAMMA; ++g)
        if (g < gamma) w1 = w1 * om;
      const float wg = gamma >= 1 ? w1 * om : 1.0f;
      const float phi = gamma == 0 ? 1.0f : wg + ((gam * p_t) * w1) * nll;
      const float k = kc_t + kf_t * phi;
#pragma unroll
      for (int c = 0; c < LS_MAX_CLASSES; ++c) {
        if (c < C) {
          const float p = e[c];
          const float u = c == tv ? G[c] + a_t : G[c];
          const float r = p * (u - dot);
          const float y = c == tv ? p - 1.0f : p;
          float g = k * y + r;
          if (scaled) g = g * scale;
          x[c][j] = g;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < LS_MAX_CLASSES; ++c) {
      if (c < C) {
        float* p = gf + (size_t)c * HW_;
        if (full && ((gpad + (unsigned)c * HW_ + 4u - pad) & 3u) == 0) {
          *reinterpret_cast<float4*>(p + i0) = make_float4(x[c][0], x[c][1], x[c][2], x[c][3]);
        } else {
#pragma unroll
          for (int j = 0; j < LS_GROUP; ++j)
            if (i0 + j >= 0 && i0 + j < HW) p[i0 + j] = x[c][j];
        }
      }
    }
  }
}

// dst[i] = src[i] for 0 <= src[i] <= 254, else 255 (ignore_index -100 and every other value no class can have).  A thread
// owns the 16 destination bytes between two 16-byte boundaries OF THE DESTINATION: one 16-byte store, and eight 16-byte loads
// when the source of that group is 16-byte aligned too (it is 8-byte aligned by type), else sixteen 8-byte loads; the groups
// that hang over the head or the tail go element by element inside [0, n).
constexpr int LN_THREADS = 256, LN_GROUP = 16;

__device__ __forceinline__ unsigned ln_narrow(long long v) { return (unsigned long long)v <= 254ull ? (unsigned)v : 255u; }

__global__ void __launch_bounds__(LN_THREADS) loss_narrow_kernel(const long long* __restrict__ src, long long n, uint8_t* __restrict__ dst) {
  const long long head = (long long)((uintptr_t)dst & 15u);
  const long long i0 = ((long long)blockIdx.x * LN_THREADS + threadIdx.x) * LN_GROUP - head;
  if (i0 >= n) return;
  if (i0 >= 0 && i0 + LN_GROUP <= n) {
    long long v[LN_GROUP];
    if ((((uintptr_t)(src + i0)) & 15u) == 0) {
#pragma unroll
      for (int j = 0; j < LN_GROUP; j += 2) {
        const longlong2 q = *reinterpret_cast<const longlong2*>(src + i0 + j);
        v[j] = q.x; v[j + 1] = q.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < LN_GROUP; ++j) v[j] = src[i0 + j];
    }
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < LN_GROUP; ++j) w[j >> 2] |= ln_narrow(v[j]) << (8 * (j & 3));
    *reinterpret_cast<uint4*>(dst + i0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll 1
    for (int j = 0; j < LN_GROUP; ++j)
      if (i0 + j >= 0 && i0 + j < n) dst[i0 + j] = (uint8_t)ln_narrow(src[i0 + j]);
  }
}

}  // namespace unetpp
