// evaluation.h — device kernels that compare two uint8 masks: the joint histogram of (target, pred) that every number of
// the reference's compute_metrics / compute_confusion_matrix (src/utils/metrics.py) and iou_per_class (tools/eval.py)
// is a function of, and the disagreement of two masks with the logit margin at the pixels that differ.  Everything is an
// integer sum, a minimum or a maximum: no result depends on the order in which workgroups arrive.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace unetpp {

constexpr int EV_THREADS = 256, EV_WAVES = EV_THREADS / 64;
constexpr int EV_VEC = 16;                                    // bytes of each mask one thread loads at a time
constexpr int EV_ITERS = 2;                                   // loads per thread
constexpr int EV_SPAN = EV_THREADS * EV_VEC * EV_ITERS;       // pixels one workgroup owns (8192)
constexpr int EV_MAX_CLASSES = 16;
constexpr int EV_MAX_BINS = EV_MAX_CLASSES * EV_MAX_CLASSES + 2;      // counts, then ignored, then invalid

// A workgroup owns EV_SPAN consecutive *positions* of one frame; position q holds pixel q - pad, where pad (0..15) is the
// frame's first address modulo 16 (0 without vector loads).  So every group of 16 positions starts on a 16-byte boundary
// whatever the frame's offset b * H * W is; the groups that hang over the frame's head or tail are read byte by byte,
// and only inside the frame.
//
// Loads positions [i0 + pad, i0 + pad + 16) of two frames: pixels i0 .. i0 + 15, -16 < i0 < HW.  Returns the mask of the
// pixels that exist; the others read as 0 in both.
__device__ __forceinline__ unsigned ev_load_pair(const uint8_t* __restrict__ f0, const uint8_t* __restrict__ f1, long long i0, long long HW,
                                                 int vec_ok, unsigned w0[4], unsigned w1[4]) {
  if (vec_ok && i0 >= 0 && i0 + EV_VEC <= HW) {
    const uint4 a = *reinterpret_cast<const uint4*>(f0 + i0);
    const uint4 b = *reinterpret_cast<const uint4*>(f1 + i0);
    w0[0] = a.x; w0[1] = a.y; w0[2] = a.z; w0[3] = a.w;
    w1[0] = b.x; w1[1] = b.y; w1[2] = b.z; w1[3] = b.w;
    return 0xffffu;
  }
  unsigned live = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) w0[k] = w1[k] = 0;
#pragma unroll
  for (int j = 0; j < EV_VEC; ++j) {
    const long long i = i0 + j;
    if (i >= 0 && i < HW) {
      w0[j >> 2] |= (unsigned)f0[i] << (8 * (j & 3));
      w1[j >> 2] |= (unsigned)f1[i] << (8 * (j & 3));
      live |= 1u << j;
    }
  }
  return live;
}

__device__ __forceinline__ unsigned ev_byte(const unsigned w[4], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

__device__ __forceinline__ unsigned ev_wave_sum(unsigned n) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += (unsigned)__shfl_xor((int)n, d, 64);
  return n;
}

// counts[frame][t * C + p] += pixels with target t and pred p, both < C and the target not `ignore`;
// outside[frame][0] += pixels whose target is `ignore`; outside[frame][1] += the remaining ones with t >= C or p >= C;
// total[bin] += the same, all frames, 64-bit, when total is given.  counts and outside are zeroed before the launch.
// Grid (ceil((HW + 15) / EV_SPAN), B).
//
// Contention: a real mask is mostly one bin.  Each thread folds the run of equal bins it is in into a register (a group
// of 16 equal pixels is one comparison) and touches LDS only when the bin changes; each wave has its own LDS histogram;
// a wave whose threads all end in the same bin adds it once.  The workgroup then issues one global atomic per non-zero
// bin.  No counter is narrower than 32 bits.
__global__ void __launch_bounds__(EV_THREADS) confusion_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target, unsigned HW,
                                                              int C, int ignore, int vec_ok, unsigned* __restrict__ counts,
                                                              unsigned* __restrict__ outside, unsigned long long* __restrict__ total) {
  __shared__ unsigned hist[EV_WAVES][EV_MAX_BINS];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.y * HW;
  const uint8_t* pf = pred + base;
  const uint8_t* tf = target + base;
  const int pad = vec_ok ? (int)((uintptr_t)pf & 15u) : 0;      // the same for both masks: vec_ok says so
  const long long first = (long long)blockIdx.x * EV_SPAN - pad;
  if (first >= (long long)HW) return;                           // the spare workgroup of a frame with a small pad
  for (int j = t; j < EV_WAVES * EV_MAX_BINS; j += EV_THREADS) (&hist[0][0])[j] = 0;
  __syncthreads();
  unsigned* h = hist[t >> 6];
  const int CC = C * C;
  int run_key = 0;
  unsigned run_n = 0;
  auto key_of = [&](unsigned tv, unsigned pv) -> int {
    return (int)tv == ignore ? CC : (tv >= (unsigned)C || pv >= (unsigned)C) ? CC + 1 : (int)(tv * C + pv);
  };
  auto step = [&](int key, unsigned n) {
    if (key == run_key) {
      run_n += n;
    } else {
      if (run_n) atomicAdd(&h[run_key], run_n);
      run_key = key;
      run_n = n;
    }
  };
#pragma unroll
  for (int it = 0; it < EV_ITERS; ++it) {
    const long long i0 = first + (long long)(it * EV_THREADS + t) * EV_VEC;
    if (i0 >= (long long)HW) break;
    unsigned tw[4], pw[4];
    const unsigned live = ev_load_pair(tf, pf, i0, HW, vec_ok, tw, pw);
    if (live == 0xffffu) {
      const unsigned t0 = tw[0] & 0xffu, p0 = pw[0] & 0xffu;
      const unsigned ts = t0 * 0x01010101u, ps = p0 * 0x01010101u;
      if (tw[0] == ts && tw[1] == ts && tw[2] == ts && tw[3] == ts && pw[0] == ps && pw[1] == ps && pw[2] == ps && pw[3] == ps) {
        step(key_of(t0, p0), EV_VEC);
      } else {
#pragma unroll
        for (int j = 0; j < EV_VEC; ++j) step(key_of(ev_byte(tw, j), ev_byte(pw, j)), 1);
      }
    } else {
#pragma unroll
      for (int j = 0; j < EV_VEC; ++j)
        if ((live >> j) & 1u) step(key_of(ev_byte(tw, j), ev_byte(pw, j)), 1);
    }
  }
  // the run each thread is still in: one LDS add per wave when the whole wave is in the same bin
  const int k0 = __builtin_amdgcn_readfirstlane(run_key);
  if (__all(run_key == k0)) {
    const unsigned n = ev_wave_sum(run_n);
    if ((t & 63) == 0 && n) atomicAdd(&h[k0], n);
  } else if (run_n) {
    atomicAdd(&h[run_key], run_n);
  }
  __syncthreads();
  for (int j = t; j < CC + 2; j += EV_THREADS) {
    unsigned n = 0;
#pragma unroll
    for (int wv = 0; wv < EV_WAVES; ++wv) n += hist[wv][j];
    if (n) {
      if (j < CC) atomicAdd(counts + (size_t)blockIdx.y * CC + j, n);
      else atomicAdd(outside + (size_t)blockIdx.y * 2 + (j - CC), n);
      if (total) atomicAdd(total + j, (unsigned long long)n);
    }
  }
}

// Per frame, over the pixels with a != b: n_diff += their number; first = min(their linear index) (0xffffffff, the int32
// -1, before the launch and when there is none); with logits [B,C,HW] over those with both values < C:
// max_margin = max |logits[a] - logits[b]| through atomicMax on the bits of the non-negative float (0.0 before the launch),
// n_nan += those whose margin is NaN (they stay out of the maximum).  Logits are read at differing pixels only.
// Same grid and positions as confusion_kernel.  One atomic per output and workgroup, none from a workgroup without a
// difference.
__global__ void __launch_bounds__(EV_THREADS) mask_disagreement_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, unsigned HW,
                                                                      const float* __restrict__ logits, int C, int vec_ok,
                                                                      unsigned* __restrict__ n_diff, unsigned* __restrict__ first_idx,
                                                                      unsigned* __restrict__ max_margin, unsigned* __restrict__ n_nan) {
  __shared__ unsigned part[EV_WAVES][4];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.y * HW;
  const uint8_t* af = a + base;
  const uint8_t* bf = b + base;
  const float* lf = logits ? logits + base * (size_t)C : nullptr;
  const int pad = vec_ok ? (int)((uintptr_t)af & 15u) : 0;
  const long long first = (long long)blockIdx.x * EV_SPAN - pad;
  if (first >= (long long)HW) return;
  unsigned n = 0, fi = 0xffffffffu, nn = 0;
  float mx = 0.0f;
#pragma unroll
  for (int it = 0; it < EV_ITERS; ++it) {
    const long long i0 = first + (long long)(it * EV_THREADS + t) * EV_VEC;
    if (i0 >= (long long)HW) break;
    unsigned aw[4], bw[4];
    ev_load_pair(af, bf, i0, HW, vec_ok, aw, bw);             // pixels that do not exist read as 0 in both: equal
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (aw[k] == bw[k]) continue;
#pragma unroll
      for (int j = 4 * k; j < 4 * k + 4; ++j) {
        const unsigned av = ev_byte(aw, j), bv = ev_byte(bw, j);
        if (av == bv) continue;
        const unsigned i = (unsigned)(i0 + j);
        ++n;
        fi = min(fi, i);
        if (lf && av < (unsigned)C && bv < (unsigned)C) {
          const float m = fabsf(lf[(size_t)av * HW + i] - lf[(size_t)bv * HW + i]);
          if (m != m) ++nn;
          else mx = fmaxf(mx, m);
        }
      }
    }
  }
  unsigned mb = __float_as_uint(mx);                          // non-negative floats order as their bits
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n += (unsigned)__shfl_xor((int)n, d, 64);
    nn += (unsigned)__shfl_xor((int)nn, d, 64);
    fi = min(fi, (unsigned)__shfl_xor((int)fi, d, 64));
    mb = max(mb, (unsigned)__shfl_xor((int)mb, d, 64));
  }
  if ((t & 63) == 0) { part[t >> 6][0] = n; part[t >> 6][1] = fi; part[t >> 6][2] = mb; part[t >> 6][3] = nn; }
  __syncthreads();
  if (t == 0) {
    n = nn = mb = 0;
    fi = 0xffffffffu;
#pragma unroll
    for (int wv = 0; wv < EV_WAVES; ++wv) {
      n += part[wv][0];
      fi = min(fi, part[wv][1]);
      mb = max(mb, part[wv][2]);
      nn += part[wv][3];
    }
    if (n) {
      atomicAdd(n_diff + blockIdx.y, n);
      atomicMin(first_idx + blockIdx.y, fi);
      if (mb) atomicMax(max_margin + blockIdx.y, mb);
      if (nn) atomicAdd(n_nan + blockIdx.y, nn);
    }
  }
}

}  // namespace unetpp
