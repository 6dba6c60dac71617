// The two kernels of include/optim/unetpp_optim.h; the arithmetic and its order are specified there, operation by operation,
// and unet_amd/optim.py repeats them in NumPy.  Compiled with -ffp-contract=off: every product and sum below is rounded on
// its own.  Both kernels are streaming and memory-bound: launch A reads 4n bytes, launch B reads 16n and writes 12n (16n with
// zero_grads), 16 bytes per lane and access when the buffers are 16-byte aligned (VEC), 4 otherwise, same element ownership.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/optim/unetpp_optim.h"

namespace optim {

constexpr int THREADS = 256;                    // one workgroup; vector j of a chunk belongs to thread j % THREADS
constexpr int GRANULE = 8192;                   // chunk(n) is a multiple of this many elements
constexpr int MAX_PARTIALS = 1024;              // parts(n) <= this for every n <= MAX_N
constexpr long long MAX_N = 1ll << 27;
constexpr int SLOT_WORDS = 8;                   // uint32 words per state slot
enum { ST_STEP = 0, ST_SCALE = 1, ST_TRACKER = 2, ST_NORM = 3, ST_FOUND_INF = 4 };

__host__ __device__ inline long long chunk_of(long long n) {
  const long long per = (long long)GRANULE * MAX_PARTIALS;
  return GRANULE * ((n + per - 1) / per);
}
__host__ __device__ inline int parts_of(long long n) { return (int)((n + chunk_of(n) - 1) / chunk_of(n)); }

// elements i .. i+3 of a buffer whose valid range ends at `end`; what lies past it reads as +0
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ src, long long i, long long end, float x[4]) {
  if (VEC && i + 4 <= end) {
    const float4 q = *reinterpret_cast<const float4*>(src + i);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = i + k < end ? src[i + k] : 0.0f;
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ dst, long long i, long long end, const float x[4]) {
  if (VEC && i + 4 <= end) {
    *reinterpret_cast<float4*>(dst + i) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < end) dst[i + k] = x[k];
  }
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void grad_norm_kernel(const float* __restrict__ g, long long n, long long chunk,
                                                            double* __restrict__ partial, uint32_t* __restrict__ flag) {
  const long long base = (long long)blockIdx.x * chunk;
  const long long end = n < base + chunk ? n : base + chunk;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = base + 4 * (long long)threadIdx.x; i < end; i += 4 * THREADS) {
    float x[4];
    load4<VEC>(g, i, end, x);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = (double)x[k];
      a[k] = a[k] + d * d;
    }
  }
  double v = (a[0] + a[1]) + (a[2] + a[3]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
  __shared__ double waves[THREADS / 64];
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = ((waves[0] + waves[1]) + waves[2]) + waves[3];
    partial[blockIdx.x] = s;
    flag[blockIdx.x] = isfinite(s) ? 0u : 1u;
  }
}

struct GroupScalars {                           // one group's float32 scalars, see the header
  float lr, wd, eps, mu, beta2, decay, omb1, omb2, ss, rbc2;
};

__device__ inline double pow_int(double b, int e) {
  double r = 1.0;
  while (e) {
    if (e & 1) r = r * b;
    e >>= 1;
    if (e) b = b * b;
  }
  return r;
}

template <int KIND>
__device__ __forceinline__ void update(float g, float& p, float& m, float& v, const GroupScalars& s, float mult, bool first) {
  g = g * mult;
  if (KIND == UNETPP_OPTIM_ADAMW) {
    if (s.wd != 0.0f) p = p * s.decay;
  } else {
    if (s.wd != 0.0f) g = g + s.wd * p;
  }
  if (KIND == UNETPP_OPTIM_SGD) {
    if (s.mu != 0.0f) {
      m = first ? g : m * s.mu + g;
      g = m;
    }
    p = p - s.lr * g;
  } else {
    m = m + (g - m) * s.omb1;
    v = v * s.beta2 + (g * g) * s.omb2;
    // not __fsqrt_rn: the HIP headers map it to the native (1 ulp) square root; the builtin is the correctly rounded one
    const float d = __fdiv_rn(__builtin_sqrtf(v), s.rbc2) + s.eps;
    p = p - __fdiv_rn(s.ss * m, d);
  }
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(THREADS) void step_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long long n, long long chunk, int parts,
                                                       const double* __restrict__ partial, const uint32_t* __restrict__ flag,
                                                       unetpp_optim_groups G, unetpp_optim_step_args A, uint32_t* state,
                                                       uint32_t* scaler_state) {
  __shared__ double s_partial[MAX_PARTIALS];
  __shared__ GroupScalars s_group[UNETPP_OPTIM_MAX_GROUPS];
  __shared__ long long s_end[UNETPP_OPTIM_MAX_GROUPS];
  const int tid = threadIdx.x;
  int bad = 0;
  for (int i = tid; i < parts; i += THREADS) {
    s_partial[i] = partial[i];
    bad |= (int)flag[i];
  }
  const bool found_inf = __syncthreads_or(bad) != 0;          // also the barrier that publishes s_partial
  double S = 0.0;
  for (int i = 0; i < parts; ++i) S = S + s_partial[i];

  const bool use_scaler = scaler_state != nullptr;
  const int step = (int)state[A.parity * SLOT_WORDS + ST_STEP];
  const uint32_t* rd = use_scaler ? scaler_state + A.scaler_parity * SLOT_WORDS : nullptr;
  const float scale = use_scaler ? __uint_as_float(rd[ST_SCALE]) : 1.0f;
  const int tracker = use_scaler ? (int)rd[ST_TRACKER] : 0;
  const float inv_scale = use_scaler ? __fdiv_rn(1.0f, scale) : 1.0f;
  const float total_norm = (float)__dsqrt_rn(S) * inv_scale;
  float coef = 1.0f;
  if (A.use_clip) {
    coef = __fdiv_rn(A.max_norm, total_norm + 1e-6f);
    if (coef > 1.0f) coef = 1.0f;
  }
  const float mult = inv_scale * coef;
  const bool skip = use_scaler && found_inf;
  const int t = step + 1;

  if (tid < G.n_groups) {
    const double lr = G.lr[tid], wd = G.weight_decay[tid];
    GroupScalars s;
    s.lr = (float)lr;
    s.wd = (float)wd;
    s.eps = (float)G.eps[tid];
    s.mu = (float)G.momentum[tid];
    s.beta2 = (float)G.beta2[tid];
    s.decay = (float)(1.0 - lr * wd);
    s.omb1 = (float)(1.0 - G.beta1[tid]);
    s.omb2 = (float)(1.0 - G.beta2[tid]);
    const double bc1 = 1.0 - pow_int(G.beta1[tid], t), bc2 = 1.0 - pow_int(G.beta2[tid], t);
    s.ss = (float)(lr / bc1);
    s.rbc2 = (float)__dsqrt_rn(bc2);
    s_group[tid] = s;
    s_end[tid] = G.end[tid];
  }
  __syncthreads();

  if (blockIdx.x == 0 && tid == 0) {
    uint32_t* wr = state + (1 - A.parity) * SLOT_WORDS;
    wr[ST_STEP] = (uint32_t)(skip ? step : t);
    wr[ST_NORM] = __float_as_uint(total_norm);
    wr[ST_FOUND_INF] = found_inf ? 1u : 0u;
    if (use_scaler) {
      float scale2 = scale;
      int tracker2 = tracker;
      if (found_inf) {
        scale2 = scale * A.backoff_factor;
        tracker2 = 0;
      } else if (tracker + 1 == A.growth_interval) {
        const float grown = scale * A.growth_factor;
        if (isfinite(grown)) scale2 = grown;
        tracker2 = 0;
      } else {
        tracker2 = tracker + 1;
      }
      uint32_t* ws = scaler_state + (1 - A.scaler_parity) * SLOT_WORDS;
      ws[ST_SCALE] = __float_as_uint(scale2);
      ws[ST_TRACKER] = (uint32_t)tracker2;
    }
  }

  const long long base = (long long)blockIdx.x * chunk;
  const long long end = n < base + chunk ? n : base + chunk;
  const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (skip) {
    if (A.zero_grads)
      for (long long i = base + 4 * (long long)tid; i < end; i += 4 * THREADS) store4<VEC>(g, i, end, zero);
    return;
  }
  const bool first = t == 1;
  for (long long i = base + 4 * (long long)tid; i < end; i += 4 * THREADS) {
    float xg[4], xp[4], xm[4] = {0.0f, 0.0f, 0.0f, 0.0f}, xv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    load4<VEC>(g, i, end, xg);
    load4<VEC>(p, i, end, xp);
    if (KIND != UNETPP_OPTIM_SGD || m) load4<VEC>(m, i, end, xm);
    if (KIND != UNETPP_OPTIM_SGD) load4<VEC>(v, i, end, xv);
    int grp = 0;
    while (grp < G.n_groups - 1 && i >= s_end[grp]) ++grp;
    GroupScalars s = s_group[grp];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k && grp < G.n_groups - 1 && i + k >= s_end[grp]) {       // a group boundary inside the vector
        while (grp < G.n_groups - 1 && i + k >= s_end[grp]) ++grp;
        s = s_group[grp];
      }
      update<KIND>(xg[k], xp[k], xm[k], xv[k], s, mult, first);
    }
    store4<VEC>(p, i, end, xp);
    if (KIND != UNETPP_OPTIM_SGD || m) store4<VEC>(m, i, end, xm);
    if (KIND != UNETPP_OPTIM_SGD) store4<VEC>(v, i, end, xv);
    if (A.zero_grads) store4<VEC>(g, i, end, zero);
  }
}

}  // namespace optim
