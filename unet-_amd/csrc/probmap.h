// probmap.h — device kernels that read a float32 probability plane together with a mask or a label image: the rules of the
// reference's tools/inference_binary_optimized.py on the softmax map (apply_hysteresis :116-136,
// apply_morphological_and_filtering :139-176, scan_thresholds :179-270).  Every result is a comparison of float32 values or
// an integer sum: none depends on the order in which threads, waves or workgroups arrive.
//
// A plane is channel `ch` of an interleaved array float32 [B,HW,S]: pixel i of frame b is prob[(b * HW + i) * S + ch].
// A thread owns PM_PX = 16 consecutive pixels of one frame, a workgroup PM_SPAN = 4096.  The 16 pixels are read with
// 16-byte loads when S is 1 or 2, all 16 exist and their first byte is 16-byte aligned (S = 2 loads whole pixels and picks
// the channel); otherwise one float at a time, and only pixels below HW.  The byte and label arrays beside the plane
// follow the same rule, each by its own address.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "components.h"

namespace unetpp {

constexpr int PM_THREADS = 256, PM_WAVES = PM_THREADS / 64;
constexpr int PM_PX = 16;
constexpr int PM_SPAN = PM_THREADS * PM_PX;
constexpr int PM_MAX_THRESHOLDS = 256;
constexpr int PM_MAX_BINS = 2 * (PM_MAX_THRESHOLDS + 1) + 1;     // [target matches?][k], then the ignored pixels
constexpr int PM_TAB = 512;                                      // slots of a workgroup's label table
constexpr int PM_PROBES = 8;

struct PmThresholds { float t[PM_MAX_THRESHOLDS]; };            // a kernel argument: nothing is allocated or copied per call

__device__ __forceinline__ bool pm_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Pixels i0 .. i0 + 15 of a frame's plane (frame = the frame's first float of the array, ch not yet added); i0 < HW.
// Returns how many exist (1..16); the others read as NaN.
__device__ __forceinline__ int pm_load16(const float* __restrict__ frame, long long i0, long long HW, int S, int ch, float (&v)[PM_PX]) {
  const int n = (int)(HW - i0 < PM_PX ? HW - i0 : PM_PX);
  const float* p = frame + i0 * S;
  if (n == PM_PX && S == 1 && pm_aligned16(p)) {
    const float4* s = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float4 t = s[q]; v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w; }
  } else if (n == PM_PX && S == 2 && pm_aligned16(p)) {
    const float4* s = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int q = 0; q < 8; ++q) { const float4 t = s[q]; v[2 * q] = ch ? t.y : t.x; v[2 * q + 1] = ch ? t.w : t.z; }
  } else {
#pragma unroll
    for (int j = 0; j < PM_PX; ++j) v[j] = j < n ? p[(long long)j * S + ch] : __uint_as_float(0x7fc00000u);
  }
  return n;
}

// Bytes i0 .. i0 + n - 1 of a frame's uint8 image; the others read as 0.
__device__ __forceinline__ void pm_load16_u8(const uint8_t* __restrict__ frame, long long i0, int n, unsigned (&b)[PM_PX]) {
  const uint8_t* p = frame + i0;
  if (n == PM_PX && pm_aligned16(p)) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int j = 0; j < PM_PX; ++j) b[j] = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
  } else {
#pragma unroll
    for (int j = 0; j < PM_PX; ++j) b[j] = j < n ? p[j] : 0u;
  }
}

// ---- a. threshold levels ------------------------------------------------------------------------------------------------------
// codes[b][i] = (p >= t_low) + (p >= t_high): 0, 1 or 2 with t_low <= t_high; NaN compares false twice.  Grid
// (ceil(HW / PM_SPAN), B).
__global__ void __launch_bounds__(PM_THREADS) prob_levels_kernel(const float* __restrict__ prob, int S, int ch, unsigned HW_, float t_low,
                                                                float t_high, uint8_t* __restrict__ codes) {
  const long long HW = HW_;
  const long long i0 = ((long long)blockIdx.x * PM_THREADS + threadIdx.x) * PM_PX;
  if (i0 >= HW) return;
  float v[PM_PX];
  const int n = pm_load16(prob + (size_t)blockIdx.y * HW * S, i0, HW, S, ch, v);
  unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < PM_PX; ++j) w[j >> 2] |= ((v[j] >= t_low ? 1u : 0u) + (v[j] >= t_high ? 1u : 0u)) << (8 * (j & 3));
  uint8_t* dst = codes + (size_t)blockIdx.y * HW + i0;
  if (n == PM_PX && pm_aligned16(dst)) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int j = 0; j < PM_PX; ++j)
      if (j < n) dst[j] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// ---- b. the one-pass threshold scan -----------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pm_wave_sum(unsigned n) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += (unsigned)__shfl_xor((int)n, d, 64);
  return n;
}

// counts[b][g][k] += pixels of frame b whose probability has k thresholds <= it (0..T; NaN: 0) and whose target is not
// `ignore`, g = 1 where the target matches target_class (< 0: non-zero); outside[b] += pixels whose target is `ignore`;
// total[...] += the same over all frames (2 (T + 1) counts, then outside), 64-bit, when total is given.  counts and outside
// are zeroed before the launch.  Grid (ceil(HW / PM_SPAN), B).
//
// The thresholds sit in LDS; a pixel is placed by binary search, but only when it leaves the bin of the pixel before it:
// the bin's two bounds stay in registers, so a plateau costs two comparisons per pixel.  Contention is evaluation.h's:
// each thread folds the run of equal bins it is in into a register and touches LDS when the bin changes; each wave has
// its own LDS histogram; a wave whose threads all end in one bin adds it once; the workgroup issues one global atomic
// per non-zero bin.  No counter is narrower than 32 bits.
__global__ void __launch_bounds__(PM_THREADS) prob_threshold_hist_kernel(const float* __restrict__ prob, int S, int ch,
                                                                        const uint8_t* __restrict__ target, unsigned HW_, PmThresholds th,
                                                                        int T, int target_class, int ignore, unsigned* __restrict__ counts,
                                                                        unsigned* __restrict__ outside, unsigned long long* __restrict__ total) {
  __shared__ unsigned hist[PM_WAVES][PM_MAX_BINS];
  __shared__ float thr[PM_MAX_THRESHOLDS];
  const int t = threadIdx.x;
  const long long HW = HW_;
  const int nb = T + 1, nbins = 2 * nb + 1;
  for (int j = t; j < PM_WAVES * PM_MAX_BINS; j += PM_THREADS) (&hist[0][0])[j] = 0;
  if (t < T) thr[t] = th.t[t];
  __syncthreads();
  unsigned* h = hist[t >> 6];
  int run_key = 0;
  unsigned run_n = 0;
  const long long i0 = ((long long)blockIdx.x * PM_THREADS + t) * PM_PX;
  if (i0 < HW) {
    float v[PM_PX];
    unsigned tv[PM_PX];
    const int n = pm_load16(prob + (size_t)blockIdx.y * HW * S, i0, HW, S, ch, v);
    pm_load16_u8(target + (size_t)blockIdx.y * HW, i0, n, tv);
    int k = 0;
    float lo = __uint_as_float(0x7f800000u), hi = __uint_as_float(0xff800000u);      // an empty interval: the first pixel searches
#pragma unroll
    for (int j = 0; j < PM_PX; ++j) {
      if (j >= n) continue;
      const float p = v[j];
      if (!(p >= lo && p < hi)) {                             // NaN and +inf search every time, and land right
        int a = 0, b = T;                                     // the number of thresholds <= p; every comparison with NaN is false: 0
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (thr[mid] <= p) a = mid + 1; else b = mid;
        }
        k = a;
        lo = k > 0 ? thr[k - 1] : __uint_as_float(0xff800000u);
        hi = k < T ? thr[k] : __uint_as_float(0x7f800000u);
      }
      const bool g = target_class < 0 ? tv[j] != 0u : (int)tv[j] == target_class;
      const int key = (int)tv[j] == ignore ? 2 * nb : (g ? nb : 0) + k;
      if (key == run_key) {
        ++run_n;
      } else {
        if (run_n) atomicAdd(&h[run_key], run_n);
        run_key = key;
        run_n = 1;
      }
    }
  }
  // the run each thread is still in: one LDS add per wave when the whole wave is in the same bin
  const int k0 = __builtin_amdgcn_readfirstlane(run_key);
  if (__all(run_key == k0)) {
    const unsigned n = pm_wave_sum(run_n);
    if ((t & 63) == 0 && n) atomicAdd(&h[k0], n);
  } else if (run_n) {
    atomicAdd(&h[run_key], run_n);
  }
  __syncthreads();
  for (int j = t; j < nbins; j += PM_THREADS) {
    unsigned n = 0;
#pragma unroll
    for (int wv = 0; wv < PM_WAVES; ++wv) n += hist[wv][j];
    if (n) {
      if (j < 2 * nb) atomicAdd(counts + (size_t)blockIdx.y * 2 * nb + j, n);
      else atomicAdd(outside + blockIdx.y, n);
      if (total) atomicAdd(total + j, (unsigned long long)n);
    }
  }
}

// ---- c. probability sums per component ------------------------------------------------------------------------------------------
// q(p) = floor(clamp(p, 0, 1) * 2^32) from the float's bits: p = m * 2^(E - 150) with the 24-bit significand m (no hidden
// bit and E = 1 for a subnormal), so q = m shifted by E - 118, left by at most 8 (p < 1 means E <= 126) or right, bits
// falling off the end.  q(p >= 1) = 2^32, q(p <= 0) = q(NaN) = 0.
__device__ __forceinline__ unsigned long long pm_q32(float p) {
  if (!(p > 0.0f)) return 0ull;
  if (p >= 1.0f) return 1ull << 32;
  const unsigned u = __float_as_uint(p), e = u >> 23;         // the sign is clear
  const unsigned m = e ? (u & 0x7fffffu) | 0x800000u : (u & 0x7fffffu);
  const int s = (int)(e ? e : 1u) - 118;
  return s >= 0 ? (unsigned long long)m << s : (s > -24 ? (unsigned long long)(m >> -s) : 0ull);
}

__device__ __forceinline__ void pm_label_add(int* key, unsigned long long* val, unsigned long long* sums, int l, unsigned long long q) {
  unsigned slot = ((unsigned)l * 2654435761u) >> 23;         // 9 bits
  for (int k = 0; k < PM_PROBES; ++k, slot = (slot + 1) & (PM_TAB - 1)) {
    const int old = atomicCAS(&key[slot], -1, l);
    if (old == -1 || old == l) { atomicAdd(&val[slot], q); return; }
  }
  atomicAdd(sums + l, q);                                     // no slot within PM_PROBES: straight to global memory
}

// sums[b][l] += the q of every pixel with label l, 1 <= l <= K (sums holds K + 1 rows per frame, zeroed before the launch;
// row 0, the background, stays 0).  Each thread folds the run of equal labels it is in into a 64-bit register; the runs
// meet in the workgroup's LDS table, which goes to global memory with one 64-bit integer atomic per label and workgroup.
// Grid (ceil(HW / PM_SPAN), B).
__global__ void __launch_bounds__(PM_THREADS) components_prob_sum_kernel(const int* __restrict__ labels, const float* __restrict__ prob, int S,
                                                                        int ch, int HW_, int K, unsigned long long* __restrict__ sums) {
  __shared__ int key[PM_TAB];
  __shared__ unsigned long long val[PM_TAB];
  const long long HW = HW_;
  for (int s = threadIdx.x; s < PM_TAB; s += PM_THREADS) { key[s] = -1; val[s] = 0ull; }
  __syncthreads();
  sums += (size_t)blockIdx.y * ((size_t)K + 1);
  const long long i0 = ((long long)blockIdx.x * PM_THREADS + threadIdx.x) * PM_PX;
  if (i0 < HW) {
    const int* lab = labels + (size_t)blockIdx.y * HW;
    int l[PM_PX];
    cc_load16(lab, (int)i0, (int)HW, pm_aligned16(lab + i0), l);      // -1 past the frame's end
    bool any = false;
#pragma unroll
    for (int j = 0; j < PM_PX; ++j) any |= l[j] > 0;
    if (any) {                                                // the plane is read where there is a component
      float v[PM_PX];
      pm_load16(prob + (size_t)blockIdx.y * HW * S, i0, HW, S, ch, v);
      int run_l = 0;
      unsigned long long run_q = 0ull;
#pragma unroll
      for (int j = 0; j < PM_PX; ++j) {
        const int lj = (l[j] > 0 && l[j] <= K) ? l[j] : 0;
        if (lj != run_l) {
          if (run_l) pm_label_add(key, val, sums, run_l, run_q);
          run_l = lj;
          run_q = 0ull;
        }
        if (lj) run_q += pm_q32(v[j]);
      }
      if (run_l) pm_label_add(key, val, sums, run_l, run_q);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < PM_TAB; s += PM_THREADS)
    if (key[s] >= 0) atomicAdd(sums + key[s], val[s]);
}

// ---- d. the mean-probability rule ------------------------------------------------------------------------------------------------
// keep[b][l] = 1 <= l < num[b] <= K and area >= min_area and sum >= thr_q * area, the product formed in 128 bits; a frame
// with num > K keeps nothing, as cc_select_kernel decides.  Grid (B); cc_apply_kernel paints the mask.
__global__ void __launch_bounds__(CC_THREADS) cc_select_mean_kernel(const int* __restrict__ num, const int* __restrict__ stats,
                                                                   const unsigned long long* __restrict__ sums, int K, long long min_area,
                                                                   unsigned long long thr_q, uint8_t* __restrict__ keep) {
  const int b = blockIdx.x;
  const int* st = stats + (size_t)b * K * 5;
  const unsigned long long* sm = sums + (size_t)b * ((size_t)K + 1);
  const int n = num[b] <= K ? num[b] : 0;
  for (int l = threadIdx.x; l < K; l += CC_THREADS) {
    bool k = false;
    if (l >= 1 && l < n) {
      const long long area = st[(size_t)l * 5 + 4];
      k = area >= min_area && __umul64hi(thr_q, (unsigned long long)area) == 0ull && sm[l] >= thr_q * (unsigned long long)area;
    }
    keep[(size_t)b * K + l] = k ? 1 : 0;
  }
}

}  // namespace unetpp
