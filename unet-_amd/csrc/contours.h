// contours.h — the tail of the refactored frame loop (infer_video_refactored.py:366-405) without border following:
// external contours as the 8-connected components of `inside` (everything but the background reachable from beyond the
// frame), their contourArea as a sum over 2 x 2 windows, the smallest enclosing circle of the largest one from its row
// extremes, paste_roi_mask and the three chained blends of create_overlay.  include/unetpp_contours.h states the
// arithmetic; unet_amd/contours.py holds the NumPy forms.  Every sum is an integer and every predicate is evaluated in
// integers, so no result depends on the order in which threads, waves or workgroups arrive.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace unetpp {

constexpr int CT_THREADS = 256, CT_WAVES = CT_THREADS / 64;
constexpr int CT_PX = 16;                                    // bytes one thread owns in the flat kernels: one 16-byte store
constexpr int CT_MAX_SIDE = 4095;                            // coordinates below 2^12: the in-circle determinant stays below 2^52
constexpr int CT_MAX_POINTS = 2 * CT_MAX_SIDE + 2;           // two row extremes per row
constexpr int CT_WIN = 8;                                    // windows of one row a thread of the area kernel owns
constexpr unsigned CT_NO_ROW = 0xffffffffu;

// ---- 1. plane[i] = 1 where the pixel is background (mask != match_class; match_class < 0: mask == 0).  Flat over the batch;
// the plane starts a workspace part (16-byte aligned), the mask is read 16 bytes at a time when `mask_vec`.
__global__ void __launch_bounds__(CT_THREADS) ct_background_kernel(const uint8_t* __restrict__ mask, size_t n, int match_class, int mask_vec,
                                                                  uint8_t* __restrict__ plane) {
  const size_t i0 = ((size_t)blockIdx.x * CT_THREADS + threadIdx.x) * CT_PX;
  if (i0 >= n) return;
  const bool whole = i0 + CT_PX <= n;
  unsigned in[4] = {0, 0, 0, 0};
  if (whole && mask_vec) {
    const uint4 v = *reinterpret_cast<const uint4*>(mask + i0);
    in[0] = v.x; in[1] = v.y; in[2] = v.z; in[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < CT_PX; ++j)
      if (i0 + j < n) in[j >> 2] |= (unsigned)mask[i0 + j] << (8 * (j & 3));
  }
  unsigned out[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < CT_PX; ++j) {
    const int v = (int)((in[j >> 2] >> (8 * (j & 3))) & 0xffu);
    const bool fg = match_class < 0 ? v != 0 : v == match_class;
    if (!fg) out[j >> 2] |= 1u << (8 * (j & 3));
  }
  if (whole) {
    *reinterpret_cast<uint4*>(plane + i0) = make_uint4(out[0], out[1], out[2], out[3]);
  } else {
    for (int j = 0; j < CT_PX && i0 + j < n; ++j) plane[i0 + j] = (uint8_t)((out[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// ---- 2. flags[frame][l] = 1 for every background label l (connectivity 4) with a pixel on the frame's edge: the zero padding
// joins exactly those into the outside.  flags is cleared before the launch; grid (ceil((2 W + 2 H) / 256), B).  Several
// threads may store the same 1 to one byte.
__global__ void __launch_bounds__(CT_THREADS) ct_edge_flags_kernel(const int* __restrict__ bg_labels, int H, int W, uint8_t* __restrict__ flags) {
  const int k = blockIdx.x * CT_THREADS + threadIdx.x;
  if (k >= 2 * W + 2 * H) return;
  int y, x;
  if (k < W) { y = 0; x = k; }
  else if (k < 2 * W) { y = H - 1; x = k - W; }
  else if (k < 2 * W + H) { y = k - 2 * W; x = 0; }
  else { y = k - 2 * W - H; x = W - 1; }
  const size_t hw = (size_t)H * W;
  const int l = bg_labels[blockIdx.y * hw + (size_t)y * W + x];
  if (l > 0 && (size_t)l <= hw) flags[blockIdx.y * (hw + 1) + l] = 1;
}

__device__ __forceinline__ bool ct_is_outside(const int* __restrict__ lab, const uint8_t* __restrict__ fl, int H, int W, int y, int x) {
  if (y < 0 || y >= H || x < 0 || x >= W) return true;
  const int l = lab[(size_t)y * W + x];
  return l > 0 && fl[l];
}

// ---- 3. inside = every pixel that is not outside background; border = foreground with a 4-neighbour that is outside
// background or beyond the frame.  Flat over the batch, 16 pixels per thread; `inside` starts a workspace part, `border`
// (optional) is the caller's and gets 16-byte stores when `border_vec`.
__global__ void __launch_bounds__(CT_THREADS) ct_inside_kernel(const int* __restrict__ bg_labels, const uint8_t* __restrict__ flags, int B, int H, int W,
                                                              int border_vec, uint8_t* __restrict__ inside, uint8_t* __restrict__ border) {
  const size_t hw = (size_t)H * W, n = hw * B;
  const size_t i0 = ((size_t)blockIdx.x * CT_THREADS + threadIdx.x) * CT_PX;
  if (i0 >= n) return;
  const bool whole = i0 + CT_PX <= n;
  int b = (int)(i0 / hw);
  size_t r = i0 - (size_t)b * hw;
  int y = (int)(r / W), x = (int)(r - (size_t)y * W);
  unsigned in[4] = {0, 0, 0, 0}, bd[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < CT_PX; ++j) {
    if (i0 + j < n) {
      const int* lab = bg_labels + (size_t)b * hw;
      const uint8_t* fl = flags + (size_t)b * (hw + 1);
      const int l = lab[(size_t)y * W + x];
      const bool fg = l == 0;
      if (fg || !fl[l]) in[j >> 2] |= 1u << (8 * (j & 3));
      if (border && fg &&
          (ct_is_outside(lab, fl, H, W, y - 1, x) || ct_is_outside(lab, fl, H, W, y + 1, x) || ct_is_outside(lab, fl, H, W, y, x - 1) ||
           ct_is_outside(lab, fl, H, W, y, x + 1)))
        bd[j >> 2] |= 1u << (8 * (j & 3));
      if (++x == W) {
        x = 0;
        if (++y == H) { y = 0; ++b; }
      }
    }
  }
  if (whole) {
    *reinterpret_cast<uint4*>(inside + i0) = make_uint4(in[0], in[1], in[2], in[3]);
    if (border && border_vec) *reinterpret_cast<uint4*>(border + i0) = make_uint4(bd[0], bd[1], bd[2], bd[3]);
  }
  if (!whole || (border && !border_vec)) {
    for (int j = 0; j < CT_PX && i0 + j < n; ++j) {
      if (!whole) inside[i0 + j] = (uint8_t)((in[j >> 2] >> (8 * (j & 3))) & 0xffu);
      if (border && !(whole && border_vec)) border[i0 + j] = (uint8_t)((bd[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
  }
}

__device__ __forceinline__ long long ct_wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ---- 4. area2[frame][l] += over the 2 x 2 windows of pixel centres whose inside pixels carry label l: 2 where all four are
// inside, 1 where exactly three are (the inside pixels of one window are 8-neighbours, so they share a label).  Window
// (wy, wx) holds the pixels (wy - 1 .. wy, wx - 1 .. wx), 0 <= wy <= H, 0 <= wx <= W: the windows that hang over the frame
// edge are included.  Grid (ceil((W + 1) / (256 CT_WIN)), H + 1, B); area2 is cleared before the launch.
// A thread owns CT_WIN consecutive windows of one row and keeps the sum of the run of one label it is in; a run that ends
// goes to global memory with one 64-bit atomic.  At the end a wave whose runs all carry one label (the usual case: one large
// component) reduces them by shuffles, and the workgroup merges its waves' results through LDS: one atomic per label.
__global__ void __launch_bounds__(CT_THREADS) ct_area_kernel(const int* __restrict__ labels, int H, int W, int K,
                                                            unsigned long long* __restrict__ area2) {
  __shared__ int w_lab[CT_WAVES];
  __shared__ long long w_sum[CT_WAVES];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int wy = blockIdx.y;
  const size_t hw = (size_t)H * W;
  const int* lab = labels + blockIdx.z * hw;
  unsigned long long* out = area2 + (size_t)blockIdx.z * K;
  const int wx0 = (blockIdx.x * CT_THREADS + t) * CT_WIN;
  const int* up = wy >= 1 ? lab + (size_t)(wy - 1) * W : nullptr;
  const int* dn = wy < H ? lab + (size_t)wy * W : nullptr;
  int run_l = 0;
  long long run_s = 0;
  auto px = [&](const int* row, int x) { return (row && x >= 0 && x < W) ? row[x] : 0; };
  int a = px(up, wx0 - 1), c = px(dn, wx0 - 1);
#pragma unroll
  for (int j = 0; j < CT_WIN; ++j) {
    const int wx = wx0 + j;
    const int b = px(up, wx), d = px(dn, wx);
    if (wx <= W) {
      const int cnt = (a > 0) + (b > 0) + (c > 0) + (d > 0);
      if (cnt >= 3) {
        const int l = max(max(a, b), max(c, d));
        if (l != run_l) {
          if (run_s && run_l < K) atomicAdd(out + run_l, (unsigned long long)run_s);
          run_l = l;
          run_s = 0;
        }
        run_s += cnt - 2;
      }
    }
    a = b; c = d;
  }
  // the run each thread is still in
  const unsigned long long has = __ballot(run_s != 0);
  int wl = 0;
  long long ws = 0;
  if (has) {
    const int l0 = __shfl(run_l, __ffsll((long long)has) - 1, 64);
    if (__all(run_s == 0 || run_l == l0)) {
      ws = ct_wave_sum(run_s);
      wl = l0;
    } else if (run_s && run_l < K) {
      atomicAdd(out + run_l, (unsigned long long)run_s);
    }
  }
  if (lane == 0) { w_lab[wave] = wl; w_sum[wave] = ws; }
  __syncthreads();
  if (t < CT_WAVES && w_sum[t] != 0) {                       // the first wave with a label adds the sums of all waves with it
    bool first = true;
    long long s = 0;
    for (int k = 0; k < CT_WAVES; ++k) {
      if (w_sum[k] != 0 && w_lab[k] == w_lab[t]) {
        if (k < t) first = false;
        s += w_sum[k];
      }
    }
    if (first && w_lab[t] < K) atomicAdd(out + w_lab[t], (unsigned long long)s);
  }
}

// ---- 5. the frame's chosen label: the largest area2 among labels 1 .. min(num, K) - 1, the lowest label on ties; 0 for a frame
// without foreground.  Grid (B).  Writes support[frame] = {0, 0, 0, 0, 0, 0, 0, chosen}.
__global__ void __launch_bounds__(CT_THREADS) ct_choose_kernel(const int* __restrict__ num, const unsigned long long* __restrict__ area2, int K,
                                                              int* __restrict__ support) {
  __shared__ unsigned long long s_a[CT_THREADS];
  __shared__ int s_l[CT_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const unsigned long long* ar = area2 + (size_t)b * K;
  const int n = min(num[b], K);
  unsigned long long best = 0;
  int bl = 0;
  for (int l = 1 + t; l < n; l += CT_THREADS)                // ascending labels: '>' keeps the first of equal areas
    if (bl == 0 || ar[l] > best) { best = ar[l]; bl = l; }
  s_a[t] = best; s_l[t] = bl;
  __syncthreads();
  for (int d = CT_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) {
      const int ol = s_l[t + d];
      const unsigned long long oa = s_a[t + d];
      if (ol > 0 && (s_l[t] == 0 || oa > s_a[t] || (oa == s_a[t] && ol < s_l[t]))) { s_a[t] = oa; s_l[t] = ol; }
    }
    __syncthreads();
  }
  if (t < 8) support[(size_t)b * 8 + t] = t == 7 ? s_l[0] : 0;
}

// ---- 6. rows[frame][y] = first | last << 16 of the columns with labels == chosen, CT_NO_ROW for a row without one.  One wave
// per row; grid (H, B), 64 threads.
__global__ void __launch_bounds__(64) ct_row_extremes_kernel(const int* __restrict__ labels, const int* __restrict__ support, int H, int W,
                                                            unsigned* __restrict__ rows) {
  const int y = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int chosen = support[(size_t)b * 8 + 7];
  int lo = W, hi = -1;
  if (chosen > 0) {
    const int* row = labels + ((size_t)b * H + y) * W;
    for (int x = lane; x < W; x += 64)
      if (row[x] == chosen) { lo = min(lo, x); hi = x; }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = min(lo, __shfl_xor(lo, d, 64));
    hi = max(hi, __shfl_xor(hi, d, 64));
  }
  if (lane == 0) rows[(size_t)b * H + y] = hi < 0 ? CT_NO_ROW : ((unsigned)lo | (unsigned)hi << 16);
}

// The circle 1, 2 or 3 integer points define, and "is p strictly outside it" in integers: 1 point: p differs; 2 points (a
// diameter): (p - a).(p - b) > 0; 3 points: the in-circle determinant times the orientation, both relative to the first point.
// Coordinates are below 2^12, so the squares are below 2^25 and each of the six products of the determinant below 2^50.
struct CtCircle { int n, ax, ay, bx, by, cx, cy; };

__device__ __forceinline__ bool ct_outside(const CtCircle& c, int x, int y) {
  if (c.n == 1) return x != c.ax || y != c.ay;
  if (c.n == 2) return (x - c.ax) * (x - c.bx) + (y - c.ay) * (y - c.by) > 0;
  const long long bx = c.bx - c.ax, by = c.by - c.ay, cx = c.cx - c.ax, cy = c.cy - c.ay, px = x - c.ax, py = y - c.ay;
  const long long b2 = bx * bx + by * by, c2 = cx * cx + cy * cy, p2 = px * px + py * py;
  const long long det = bx * (cy * p2 - c2 * py) - by * (cx * p2 - c2 * px) + b2 * (cx * py - cy * px);
  const long long orient = bx * cy - by * cx;
  return (det > 0 && orient > 0) || (det < 0 && orient < 0);
}

// The first index in [lo, hi) whose point lies outside c, or hi: every thread scans its own indices upwards and stops at its
// first hit, the hits are reduced to the smallest.  All threads of the workgroup call it together and get the same answer;
// `red` holds two sets of per-wave results, used alternately, so that one barrier per call is enough.
__device__ __forceinline__ int ct_first_outside(const unsigned* pts, int lo, int hi, const CtCircle& c, int (*red)[CT_WAVES], int& phase) {
  int best = hi;
  for (int i = lo + (int)threadIdx.x; i < hi; i += CT_THREADS) {
    const unsigned p = pts[i];
    if (ct_outside(c, (int)(p & 0xffffu), (int)(p >> 16))) { best = i; break; }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = min(best, __shfl_xor(best, d, 64));
  int* mine = red[phase & 1];
  if ((threadIdx.x & 63) == 0) mine[threadIdx.x >> 6] = best;
  __syncthreads();
  best = min(min(mine[0], mine[1]), min(mine[2], mine[3]));
  ++phase;
  return best;
}

// ---- 7. the support set of the smallest circle around the row extremes of the chosen label; one workgroup per frame, grid (B).
// The points (at most 2 H <= 8190, one where a row's first and last column coincide) are packed x | y << 16 into LDS.  The
// incremental algorithm (support_set_np of unet_amd/contours.py: a point outside the circle so far lies on the circle of the
// points up to it; three nested "first point outside" scans) is right for any order and for repeated points, and fast when
// its first points already span the set.  So the list starts with the top-most, left-most, right-most and bottom-most point
// (copies; they appear again further on) and goes on with all points in a fixed scattered order (position = index * stride
// mod n, the stride a prime that does not divide n), so that it does not meet them sorted either.
// Writes support[frame] = {count, x0, y0, x1, y1, x2, y2, chosen}; count = 0 for a frame without foreground.
constexpr int CT_SEEDS = 4;

__global__ void __launch_bounds__(CT_THREADS) ct_circle_kernel(const unsigned* __restrict__ rows, int H, int* __restrict__ support) {
  __shared__ unsigned pts[CT_MAX_POINTS + CT_SEEDS];
  __shared__ unsigned ext[CT_SEEDS];                         // top, left (x << 16 | y), right (x << 16 | y), bottom
  __shared__ int scan[CT_THREADS];
  __shared__ int red[2][CT_WAVES];
  const int b = blockIdx.x, t = threadIdx.x;
  const unsigned* rw = rows + (size_t)b * H;
  const int per = (H + CT_THREADS - 1) / CT_THREADS, y0 = t * per, y1 = min(H, y0 + per);
  int cnt = 0;
  unsigned left = 0xffffffffu, right = 0;
  for (int y = y0; y < y1; ++y) {
    const unsigned r = rw[y];
    if (r == CT_NO_ROW) continue;
    cnt += (r & 0xffffu) == (r >> 16) ? 1 : 2;
    left = min(left, (r & 0xffffu) << 16 | (unsigned)y);
    right = max(right, (r >> 16) << 16 | (unsigned)y);
  }
  scan[t] = cnt;
  if (t == 0) { ext[1] = 0xffffffffu; ext[2] = 0; }
  __syncthreads();
  if (cnt) { atomicMin(&ext[1], left); atomicMax(&ext[2], right); }
  for (int d = 1; d < CT_THREADS; d <<= 1) {                  // inclusive prefix sums
    const int v = t >= d ? scan[t - d] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const int n0 = scan[CT_THREADS - 1];
  if (n0 == 0) return;                                       // ct_choose_kernel wrote the empty row
  const int stride = n0 % 7919 ? 7919 : 7907;
  int idx = scan[t] - cnt;
  for (int y = y0; y < y1; ++y) {
    const unsigned r = rw[y];
    if (r == CT_NO_ROW) continue;
    const unsigned lo = r & 0xffffu, hi = r >> 16;
    if (idx == 0) ext[0] = lo | (unsigned)y << 16;
    pts[CT_SEEDS + (int)(((long long)idx++ * stride) % n0)] = lo | (unsigned)y << 16;
    if (hi != lo) pts[CT_SEEDS + (int)(((long long)idx++ * stride) % n0)] = hi | (unsigned)y << 16;
    if (idx == n0) ext[3] = hi | (unsigned)y << 16;
  }
  __syncthreads();
  if (t < CT_SEEDS) pts[t] = (t == 1 || t == 2) ? (ext[t] >> 16 | (ext[t] & 0xffffu) << 16) : ext[t];
  __syncthreads();
  const int n = n0 + CT_SEEDS;
  auto X = [&](int i) { return (int)(pts[i] & 0xffffu); };
  auto Y = [&](int i) { return (int)(pts[i] >> 16); };
  int phase = 0;
  CtCircle c{1, X(0), Y(0), 0, 0, 0, 0};
  int i = 1;
  while ((i = ct_first_outside(pts, i, n, c, red, phase)) < n) {
    c = CtCircle{2, X(i), Y(i), X(0), Y(0), 0, 0};
    int j = 1;
    while ((j = ct_first_outside(pts, j, i, c, red, phase)) < i) {
      c = CtCircle{2, X(i), Y(i), X(j), Y(j), 0, 0};
      int k = 0;
      while ((k = ct_first_outside(pts, k, j, c, red, phase)) < j) {
        c = CtCircle{3, X(i), Y(i), X(j), Y(j), X(k), Y(k)};
        ++k;
      }
      ++j;
    }
    ++i;
  }
  if (t == 0) {
    int* s = support + (size_t)b * 8;
    s[0] = c.n;
    s[1] = c.ax; s[2] = c.ay;
    s[3] = c.n >= 2 ? c.bx : 0; s[4] = c.n >= 2 ? c.by : 0;
    s[5] = c.n >= 3 ? c.cx : 0; s[6] = c.n >= 3 ? c.cy : 0;
  }
}

// ---- 8. paste_roi_mask for a batch: out[frame] = zeros with masks[frame][:ph, :pw] at (x1, y1).  Flat over the batch; position q
// of the launch holds output byte q - pad, pad = the output's address modulo 16, so every thread's 16 bytes start on a
// 16-byte boundary whatever the pointer is; the groups that hang over the head or the tail are stored byte by byte.
__global__ void __launch_bounds__(CT_THREADS) ct_paste_kernel(const uint8_t* __restrict__ masks, int B, int h, int w, int x1, int y1, int pw, int ph,
                                                             int OH, int OW, int pad, uint8_t* __restrict__ out) {
  const long long ohw = (long long)OH * OW, n = ohw * B;
  const long long i0 = ((long long)blockIdx.x * CT_THREADS + threadIdx.x) * CT_PX - pad;
  if (i0 >= n) return;
  const long long s0 = i0 < 0 ? 0 : i0;
  int b = (int)(s0 / ohw);
  long long r = s0 - (long long)b * ohw;
  int y = (int)(r / OW), x = (int)(r - (long long)y * OW);
  unsigned v[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < CT_PX; ++j) {
    const long long i = i0 + j;
    if (i >= 0 && i < n) {
      const int sx = x - x1, sy = y - y1;
      if (sx >= 0 && sx < pw && sy >= 0 && sy < ph) v[j >> 2] |= (unsigned)masks[((size_t)b * h + sy) * w + sx] << (8 * (j & 3));
      if (++x == OW) {
        x = 0;
        if (++y == OH) { y = 0; ++b; }
      }
    }
  }
  if (i0 >= 0 && i0 + CT_PX <= n) {
    *reinterpret_cast<uint4*>(out + i0) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
    for (int j = 0; j < CT_PX; ++j)
      if (i0 + j >= 0 && i0 + j < n) out[i0 + j] = (uint8_t)((v[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

// ---- 9. the three chained blends of create_overlay: out byte = T2[ T1[ T0[frame byte] ] ], each look-up applied only where
// its mask (cable, tape, burr) is non-zero; T[m][channel][256] comes from the host (the reference's float64 expression).
// Flat over the 3 n bytes of the batch, positions as in ct_paste_kernel; the frame is read 16 bytes at a time when it shares
// the output's address modulo 16 (`in_vec`).
struct CtOverlayTable { uint32_t w[3 * 3 * 256 / 4]; };

__global__ void __launch_bounds__(CT_THREADS) ct_overlay_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ cable,
                                                               const uint8_t* __restrict__ tape, const uint8_t* __restrict__ burr, long long n_bytes,
                                                               CtOverlayTable table, int pad, int in_vec, uint8_t* __restrict__ out) {
  __shared__ uint32_t tab_w[3 * 3 * 256 / 4];
  for (int k = threadIdx.x; k < 3 * 3 * 256 / 4; k += CT_THREADS) tab_w[k] = table.w[k];
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab_w);
  const long long i0 = ((long long)blockIdx.x * CT_THREADS + threadIdx.x) * CT_PX - pad;
  if (i0 >= n_bytes) return;
  const bool whole = i0 >= 0 && i0 + CT_PX <= n_bytes;
  unsigned in[4] = {0, 0, 0, 0};
  if (whole && in_vec) {
    const uint4 v = *reinterpret_cast<const uint4*>(frames + i0);
    in[0] = v.x; in[1] = v.y; in[2] = v.z; in[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < CT_PX; ++j)
      if (i0 + j >= 0 && i0 + j < n_bytes) in[j >> 2] |= (unsigned)frames[i0 + j] << (8 * (j & 3));
  }
  const long long s0 = i0 < 0 ? 0 : i0;
  long long pix = s0 / 3;
  int ch = (int)(s0 - pix * 3);
  unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < CT_PX; ++j) {
    const long long i = i0 + j;
    if (i >= 0 && i < n_bytes) {
      unsigned v = (in[j >> 2] >> (8 * (j & 3))) & 0xffu;
      if (cable[pix]) v = tab[(0 * 3 + ch) * 256 + v];
      if (tape[pix]) v = tab[(1 * 3 + ch) * 256 + v];
      if (burr[pix]) v = tab[(2 * 3 + ch) * 256 + v];
      o[j >> 2] |= v << (8 * (j & 3));
      if (++ch == 3) { ch = 0; ++pix; }
    }
  }
  if (whole) {
    *reinterpret_cast<uint4*>(out + i0) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    for (int j = 0; j < CT_PX; ++j)
      if (i0 + j >= 0 && i0 + j < n_bytes) out[i0 + j] = (uint8_t)((o[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
}

}  // namespace unetpp
