// components.h — connected components of a uint8 mask on the device (cv2.connectedComponentsWithStats' results
// with scipy's label order) and the reference's three component filters.
//
// Launch sequence of unetpp_components (every hand-over between workgroups that is not an atomic on `parent`
// crosses a kernel boundary; no workgroup ever waits for another):
//   cc_tile_kernel      union-find of one 32 x 128 tile in LDS; parent[p] = smallest pixel index of p's component
//                       INSIDE the tile (per-frame linear index), -1 for background
//   cc_merge_kernel     pixels on tile edges union their components across the edge in the global parent array
//   cc_compress_kernel  parent[p] = root of p (the smallest index of the whole component); counts roots per chunk
//   cc_scan_kernel      per frame: exclusive scan of the chunk counts in raster order, num = roots + 1
//   cc_number_kernel    roots get their dense number (raster order of first pixels): parent[root] = -(number + 1)
//   cc_relabel_kernel   labels[p] = number of p's root; stats and coordinate sums, one update per horizontal run,
//                       summed per chunk in an LDS table first
//   cc_finish_stats_kernel  bounding boxes from their accumulation form to LEFT, TOP, WIDTH, HEIGHT
// Everything is integer arithmetic and every root is the SMALLEST index of its component, so labels, num, stats and
// sums are the same bits whatever order the atomics land in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unetpp {

constexpr int CC_TW = 128, CC_TH = 32;       // tile of cc_tile_kernel: 256 threads x 16 pixels of one row
constexpr int CC_THREADS = 256;
constexpr int CC_PX = 16;                    // pixels per thread everywhere (one 16-byte mask load / store)
constexpr int CC_CHUNK = CC_THREADS * CC_PX; // raster chunk of the per-pixel kernels
constexpr int CC_TAB = 512;                  // slots of the per-chunk stats table
constexpr int CC_PROBES = 8;

enum { CC_RULE_LARGEST = 0, CC_RULE_SPATIAL = 1, CC_RULE_CABLE_SHAPE = 2, CC_RULE_BOX = 3 };

struct CcRule {                              // unetpp_cc_rule / unetpp_cc_box_rule, as the kernels take them
  double min_area, min_width, max_width, min_height_ratio, min_aspect, max_center_offset, roi_width;
  double max_area, max_aspect, min_side;     // CC_RULE_BOX
};
__host__ __device__ __forceinline__ bool cc_keeps_all(int rule) { return rule == CC_RULE_SPATIAL || rule == CC_RULE_BOX; }

__device__ __forceinline__ bool cc_is_fg(unsigned v, int match_class) { return match_class < 0 ? v != 0 : (int)v == match_class; }

// ---- union-find in LDS (one tile) ---------------------------------------------------------------------------
__device__ __forceinline__ int cc_ld_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int cc_find_lds(const int* lab, int a) {
  // Terminates: lab[x] <= x for every foreground x at all times (it starts at x's run start and only atomicMin
  // lowers it), so the walk strictly decreases until it meets lab[a] == a; index 0 can only point to itself.
  for (int p; (p = cc_ld_lds(lab + a)) != a;) a = p;
  return a;
}

__device__ __forceinline__ void cc_union_lds(int* lab, int a, int b) {
  // Terminates: every pass either returns or replaces a by a strictly smaller index (old < a), and find only
  // lowers a and b; both are bounded below by 0.  A read of lab that is already out of date is harmless: entries
  // only decrease and stay inside the component, so an old value is merely a longer way to the same root, and the
  // atomicMin returns the true previous value, which decides whether this pass did the link (old == a) or a was
  // linked elsewhere meanwhile (then old, a's true parent, still has to be joined with b).
  for (;;) {
    a = cc_find_lds(lab, a);
    b = cc_find_lds(lab, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
}

// ---- union-find in the global parent array (across tiles, across workgroups and XCDs) ------------------------
__device__ __forceinline__ int cc_ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find_global(const int* parent, int a) {
  // Terminates for the reason given at cc_find_lds: parent[x] <= x always, strictly smaller unless x is a root.
  // The loads are agent-scope atomics, so they are served where the other workgroups' atomicMin lands (L2 / memory)
  // and not from this CU's L1; a value that is out of date all the same only lengthens the walk (see cc_union_lds).
  for (int p; (p = cc_ld_agent(parent + a)) != a;) a = p;
  return a;
}

__device__ __forceinline__ void cc_union_global(int* parent, int a, int b) {
  // Same loop and same termination argument as cc_union_lds; atomicMin on global memory is device scope.
  for (;;) {
    a = cc_find_global(parent, a);
    b = cc_find_global(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

// 16 consecutive entries of a per-frame int array from i0 (a multiple of 16); -1 (background) past the frame's end.
// vec: the frame is 16-byte aligned and HW % 4 == 0.  Plain loads: for entries no other workgroup writes in the launch.
__device__ __forceinline__ void cc_load16(const int* __restrict__ a, int i0, int HW, int vec, int (&v)[CC_PX]) {
  if (vec && i0 + CC_PX <= HW) {
    const int4* s = reinterpret_cast<const int4*>(a + i0);
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int4 t = s[q]; v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w; }
  } else {
#pragma unroll
    for (int j = 0; j < CC_PX; ++j) v[j] = i0 + j < HW ? a[i0 + j] : -1;
  }
}

// ---- 1. tile-local labelling --------------------------------------------------------------------------------
// grid (tiles in x, tiles in y, B), 256 threads; thread t owns 16 pixels of tile row t / 8.
__global__ void __launch_bounds__(CC_THREADS) cc_tile_kernel(const uint8_t* __restrict__ mask, int H, int W, int match_class,
                                                            int conn8, int vec_ok, int* __restrict__ parent) {
  __shared__ int lab[CC_TH * CC_TW];
  const int t = threadIdx.x, row = t >> 3, lx0 = (t & 7) * CC_PX;
  const int gy = blockIdx.y * CC_TH + row, gx0 = blockIdx.x * CC_TW + lx0;
  const size_t frame = (size_t)blockIdx.z * H * W;
  unsigned fgbits = 0;
  if (gy < H && gx0 < W) {
    const uint8_t* src = mask + frame + (size_t)gy * W + gx0;
    if (vec_ok) {                              // W % 16 == 0 and the mask is 16-byte aligned: the 16 pixels exist
      const uint4 v = *reinterpret_cast<const uint4*>(src);
      const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < CC_PX; ++j) fgbits |= (unsigned)cc_is_fg((wv[j >> 2] >> (8 * (j & 3))) & 0xffu, match_class) << j;
    } else {
      for (int j = 0; j < CC_PX && gx0 + j < W; ++j) fgbits |= (unsigned)cc_is_fg(src[j], match_class) << j;
    }
  }
  const int base = row * CC_TW + lx0;
  __shared__ unsigned fgs[CC_THREADS];         // every thread's 16 foreground bits, for its neighbours' tests below
  fgs[t] = fgbits;
  int run = -1;
#pragma unroll
  for (int j = 0; j < CC_PX; ++j) {            // pixels of a run inside the 16 start out pointing at the run's first pixel
    const bool f = (fgbits >> j) & 1u;
    if (f && run < 0) run = base + j;
    if (!f) run = -1;
    lab[base + j] = run;
  }
  __syncthreads();
  // Each foreground pixel joins its already-visited neighbours (W, and N / NW / NE in the row above), worked out as
  // 16-bit masks from the neighbouring threads' bits.  Skipped joins are implied by others: inside the 16 pixels the
  // run start already links W; p-N follows from p-W, W-NW and NW-N when all four are foreground (W-NW holds by
  // induction along the row, which starts at the tile edge); with N set, NW and NE hang on N through the row above.
  {
    const int seg = t & 7;
    const unsigned n = row > 0 ? fgs[t - 8] : 0u;
    const unsigned wl = seg > 0 ? (fgs[t - 1] >> 15) & 1u : 0u;
    const unsigned nwl = row > 0 && seg > 0 ? (fgs[t - 9] >> 15) & 1u : 0u;
    const unsigned ner = row > 0 && seg < 7 ? fgs[t - 7] & 1u : 0u;
    const unsigned w = ((fgbits << 1) | wl) & 0xffffu, nw = ((n << 1) | nwl) & 0xffffu, ne = (n >> 1) | (ner << 15);
    if (fgbits & wl) cc_union_lds(lab, base, base - 1);
    for (unsigned m = fgbits & n & ~(w & nw); m; m &= m - 1) {
      const int p = base + __ffs(m) - 1;
      cc_union_lds(lab, p, p - CC_TW);
    }
    if (conn8) {
      for (unsigned m = fgbits & ~n & nw & ~w; m; m &= m - 1) {
        const int p = base + __ffs(m) - 1;
        cc_union_lds(lab, p, p - CC_TW - 1);
      }
      for (unsigned m = fgbits & ~n & ne; m; m &= m - 1) {
        const int p = base + __ffs(m) - 1;
        cc_union_lds(lab, p, p - CC_TW + 1);
      }
    }
  }
  __syncthreads();
  if (gy < H && gx0 < W) {
    int* dst = parent + frame + (size_t)gy * W + gx0;
    int r[CC_PX];
#pragma unroll
    for (int j = 0; j < CC_PX; ++j) {          // one walk per run: only a run's first pixel was ever linked, the rest point at it
      if (((fgbits >> j) & 1u) && (j == 0 || !((fgbits >> (j - 1)) & 1u))) {
        const int l = cc_find_lds(lab, base + j);           // local raster order = global raster order inside a tile
        run = (blockIdx.y * CC_TH + (l >> 7)) * W + blockIdx.x * CC_TW + (l & (CC_TW - 1));
      }
      r[j] = ((fgbits >> j) & 1u) ? run : -1;
    }
    if (vec_ok) {                              // W % 16 == 0: all 16 pixels exist and the row segment is 64-byte aligned
#pragma unroll
      for (int q = 0; q < 4; ++q) reinterpret_cast<int4*>(dst)[q] = make_int4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
    } else {
      for (int j = 0; j < CC_PX && gx0 + j < W; ++j) dst[j] = r[j];
    }
  }
}

// ---- 2. merge across tile edges -----------------------------------------------------------------------------
// One thread per pixel of the first row of every tile but the top ones (`nrow` rows) and of the two columns either
// side of every vertical tile edge (`ncol` edges); grid (ceil(items / 256), B).  Other workgroups change `parent`
// during this launch: the union-find reads it through agent-scope atomics only.
__global__ void __launch_bounds__(CC_THREADS) cc_merge_kernel(int* __restrict__ parent, int H, int W, int conn8, int nrow, int ncol) {
  int* par = parent + (size_t)blockIdx.y * H * W;
  int item = blockIdx.x * CC_THREADS + threadIdx.x;
  int y, x;
  if (item < nrow * W) {
    y = (item / W + 1) * CC_TH; x = item % W;
  } else {
    item -= nrow * W;
    if (item >= 2 * ncol * H) return;
    const int c = item / H;
    y = item % H; x = ((c >> 1) + 1) * CC_TW - 1 + (c & 1);
    if (x >= W) return;
  }
  const int p = y * W + x;
  // Foreground tests read only the sign of an entry, which never changes after cc_tile_kernel: plain loads.
  if (par[p] < 0) return;
  const int ty = y / CC_TH, tx = x / CC_TW;
  const bool has_w = x > 0, has_n = y > 0, has_e = x + 1 < W;
  const bool w = has_w && par[p - 1] >= 0, n = has_n && par[p - W] >= 0;
  const bool nw = has_w && has_n && par[p - W - 1] >= 0, ne = has_n && has_e && par[p - W + 1] >= 0;
  const bool w_far = (x - 1) / CC_TW != tx, n_far = (y - 1) / CC_TH != ty, e_far = (x + 1) / CC_TW != tx;
  // The joins cc_tile_kernel makes, restricted to neighbours in another tile, with the same implied ones left out:
  // p-N when W and NW are set too (p-W and NW-N are row neighbours, W-NW by induction along the row; whichever of
  // these pairs straddles a tile edge is joined by this launch, the others were joined in LDS), NW / NE when N is set.
  if (w && w_far) cc_union_global(par, p, p - 1);
  if (n) {
    if (n_far && !(w && nw)) cc_union_global(par, p, p - W);
  } else if (conn8) {
    if (nw && !w && (n_far || w_far)) cc_union_global(par, p, p - W - 1);
    if (ne && (n_far || e_far)) cc_union_global(par, p, p - W + 1);
  }
}

// ---- 3. compress + count roots ------------------------------------------------------------------------------
// After the merge launch the set of roots is final (parent[r] == r), only the trees are deep.  Each pixel looks its
// root up and stores it.  Pixels of other workgroups store at the same time, so the loads stay agent-scope atomics;
// a store only ever replaces a parent by the true root of the same tree (smaller or equal), which keeps the
// invariant the find loop rests on.  A pixel's OWN entry is written by no other thread in this launch (the merge
// launch before it is complete), so it is read with a plain 16-byte load; only the walk goes through atomics.
// grid (chunks, B).
__global__ void __launch_bounds__(CC_THREADS) cc_compress_kernel(int* __restrict__ parent, int HW, int vec_ok, int* __restrict__ chunk_count) {
  int* par = parent + (size_t)blockIdx.y * HW;
  const int i0 = blockIdx.x * CC_CHUNK + threadIdx.x * CC_PX;
  int own[CC_PX];
  cc_load16(par, i0, HW, vec_ok, own);
  int roots = 0, last_p = -1, last_r = -1;
#pragma unroll
  for (int j = 0; j < CC_PX; ++j) {
    const int i = i0 + j, p = own[j];
    if (p < 0) continue;
    if (p == i) { ++roots; continue; }
    if (p != last_p) { last_p = p; last_r = cc_find_global(par, p); }
    if (last_r != p) __hip_atomic_store(par + i, last_r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __shared__ int red[CC_THREADS];
  red[threadIdx.x] = roots;
  __syncthreads();
  for (int s = CC_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) chunk_count[blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// exclusive scan of CC_THREADS values in LDS (Hillis-Steele); returns this thread's offset, *total the sum
__device__ __forceinline__ int cc_block_exscan(int v, int* buf, int* total) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int d = 1; d < CC_THREADS; d <<= 1) {
    const int add = t >= d ? buf[t - d] : 0;
    __syncthreads();
    buf[t] += add;
    __syncthreads();
  }
  const int incl = buf[t];
  *total = buf[CC_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// ---- 4. per-frame exclusive scan of the chunk counts; grid (B) ----------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) cc_scan_kernel(int* __restrict__ chunk_count, int nchunk, int* __restrict__ num) {
  __shared__ int buf[CC_THREADS];
  int* cnt = chunk_count + (size_t)blockIdx.x * nchunk;
  int carry = 0;
  for (int c0 = 0; c0 < nchunk; c0 += CC_THREADS) {
    const int c = c0 + threadIdx.x;
    const int v = c < nchunk ? cnt[c] : 0;
    int total;
    const int off = cc_block_exscan(v, buf, &total);
    if (c < nchunk) cnt[c] = carry + off;
    carry += total;
  }
  if (threadIdx.x == 0) num[blockIdx.x] = carry + 1;        // cv2's num_labels: the background counts
}

// ---- 5. number the roots in raster order; grid (chunks, B) ---------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) cc_number_kernel(int* __restrict__ parent, int HW, int vec_ok, const int* __restrict__ chunk_off) {
  __shared__ int buf[CC_THREADS];
  int* par = parent + (size_t)blockIdx.y * HW;
  const int i0 = blockIdx.x * CC_CHUNK + threadIdx.x * CC_PX;
  int own[CC_PX];
  cc_load16(par, i0, HW, vec_ok, own);
  unsigned rootbits = 0;
#pragma unroll
  for (int j = 0; j < CC_PX; ++j) rootbits |= (unsigned)(own[j] == i0 + j) << j;
  int total;
  int k = chunk_off[blockIdx.y * gridDim.x + blockIdx.x] + cc_block_exscan(__popc(rootbits), buf, &total);
  for (int j = 0; j < CC_PX; ++j)
    if ((rootbits >> j) & 1u) par[i0 + j] = -(++k + 1);      // number k >= 1 stored as -(k + 1) <= -2; background stays -1
}

// ---- 6. relabel + stats ----------------------------------------------------------------------------------------
struct CcTable {
  int key[CC_TAB];
  unsigned area[CC_TAB], sx[CC_TAB], sy[CC_TAB];            // a chunk holds 4096 pixels: 4096 * 65535 fits 32 bits
  int ileft[CC_TAB], itop[CC_TAB], right1[CC_TAB], bottom1[CC_TAB];
};

// Accumulation form of a stats row: {W - left, H - top, right + 1, bottom + 1, area}: all grow from zero, so the
// array starts as a memset and an untouched row stays zero.
__device__ __forceinline__ void cc_stats_global(int* stats, unsigned long long* sums, int label, unsigned area, unsigned long long sx,
                                                unsigned long long sy, int ileft, int itop, int right1, int bottom1) {
  int* s = stats + (size_t)label * 5;
  atomicMax(s + 0, ileft); atomicMax(s + 1, itop); atomicMax(s + 2, right1); atomicMax(s + 3, bottom1);
  atomicAdd(reinterpret_cast<unsigned*>(s + 4), area);
  atomicAdd(sums + (size_t)label * 2, sx);
  atomicAdd(sums + (size_t)label * 2 + 1, sy);
}

// grid (chunks, B).  labels: 16 consecutive pixels per thread.  With stats != nullptr each thread cuts its pixels into
// horizontal runs of one label and adds each run (area = length, sum x = length * (x0 + x1) / 2, sum y = length * y,
// box from x0, x1, y) to the chunk's LDS table; the table goes to global memory with one set of integer atomics per
// label and chunk.  A run that finds no slot within CC_PROBES goes to global memory directly.
__global__ void __launch_bounds__(CC_THREADS) cc_relabel_kernel(const int* __restrict__ parent, int H, int W, int K, int vec_ok,
                                                               int* __restrict__ labels, int* __restrict__ stats,
                                                               unsigned long long* __restrict__ sums) {
  __shared__ CcTable tab;
  const int HW = H * W;
  const int* par = parent + (size_t)blockIdx.y * HW;
  int* lab = labels + (size_t)blockIdx.y * HW;
  if (stats) {
    stats += (size_t)blockIdx.y * K * 5;
    sums += (size_t)blockIdx.y * K * 2;
    for (int s = threadIdx.x; s < CC_TAB; s += CC_THREADS) {
      tab.key[s] = -1; tab.area[s] = 0; tab.sx[s] = 0; tab.sy[s] = 0;
      tab.ileft[s] = 0; tab.itop[s] = 0; tab.right1[s] = 0; tab.bottom1[s] = 0;
    }
    __syncthreads();
  }
  const int i0 = blockIdx.x * CC_CHUNK + threadIdx.x * CC_PX;
  int out[CC_PX];
  cc_load16(par, i0, HW, vec_ok, out);
#pragma unroll
  for (int j = 0; j < CC_PX; ++j) {
    int p = out[j];
    if (p >= 0) p = par[p];                                  // the root's entry holds the number
    out[j] = p == -1 ? 0 : -p - 1;
  }
  if (vec_ok && i0 + CC_PX <= HW) {
    int4* d = reinterpret_cast<int4*>(lab + i0);
    for (int q = 0; q < 4; ++q) d[q] = make_int4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
  } else {
    for (int j = 0; j < CC_PX && i0 + j < HW; ++j) lab[i0 + j] = out[j];
  }
  if (!stats) return;
  if (i0 < HW) {
    int y = i0 / W, x = i0 - y * W;
    int j = 0;
    const int nj = min(CC_PX, HW - i0);
    while (j < nj) {
      const int l = out[j], x0 = x;
      int len = 1;
      while (j + len < nj && x + len < W && out[j + len] == l) ++len;
      const int x1 = x0 + len - 1;
      if (l < K) {
        const unsigned a = (unsigned)len, rsx = (unsigned)(len * (x0 + x1) / 2), rsy = (unsigned)(len * y);
        unsigned slot = ((unsigned)l * 2654435761u) >> 23;    // 9 bits
        bool done = false;
        for (int k = 0; k < CC_PROBES && !done; ++k, slot = (slot + 1) & (CC_TAB - 1)) {
          const int old = atomicCAS(&tab.key[slot], -1, l);
          if (old == -1 || old == l) {
            atomicAdd(&tab.area[slot], a); atomicAdd(&tab.sx[slot], rsx); atomicAdd(&tab.sy[slot], rsy);
            atomicMax(&tab.ileft[slot], W - x0); atomicMax(&tab.itop[slot], H - y);
            atomicMax(&tab.right1[slot], x1 + 1); atomicMax(&tab.bottom1[slot], y + 1);
            done = true;
          }
        }
        if (!done) cc_stats_global(stats, sums, l, a, rsx, rsy, W - x0, H - y, x1 + 1, y + 1);
      }
      j += len; x += len;
      if (x >= W) { x = 0; ++y; }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < CC_TAB; s += CC_THREADS)
    if (tab.key[s] >= 0)
      cc_stats_global(stats, sums, tab.key[s], tab.area[s], tab.sx[s], tab.sy[s], tab.ileft[s], tab.itop[s], tab.right1[s], tab.bottom1[s]);
}

// ---- 7. boxes to cv2's columns; grid (ceil(K / 256), B) -------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) cc_finish_stats_kernel(int* __restrict__ stats, int H, int W, int K) {
  const int l = blockIdx.x * CC_THREADS + threadIdx.x;
  if (l >= K) return;
  int* s = stats + ((size_t)blockIdx.y * K + l) * 5;
  if (s[4] == 0) return;                                     // rows past num, or an empty background: all zero
  const int left = W - s[0], top = H - s[1];
  s[2] -= left; s[3] -= top; s[0] = left; s[1] = top;
}

// ---- filters --------------------------------------------------------------------------------------------------------
// cc_select_kernel, grid (B): the rule's predicate per component in fp64 (SPATIAL and BOX keep every component that
// passes) and, for the rules that keep one component,
// the first of the best (lowest label among equal scores) -> keep[B][K].  A frame with more components than the
// stats hold (num > K) keeps nothing.  The arithmetic restates the reference line by line; no contraction, so that a
// product and a sum stay two roundings as in NumPy.
__device__ __forceinline__ bool cc_candidate(const int* st, const unsigned long long* sm, int l, int rule, const CcRule& r, int H, double* score) {
#pragma clang fp contract(off)
  const int* s = st + (size_t)l * 5;
  const double area = (double)s[4], w = (double)s[2], h = (double)s[3];
  if (rule == CC_RULE_LARGEST) { *score = area; return area >= r.min_area; }
  if (rule == CC_RULE_SPATIAL) {
    *score = 0.0;
    return area > r.min_area && r.min_width <= w && w <= r.max_width && h >= (double)H * r.min_height_ratio;
  }
  if (rule == CC_RULE_BOX) {                                 // the loop of detect_burrs_on_cable, infer_two_stage_burr.py:103-117
    *score = 0.0;
    const double aspect = fmax(w, h) / (fmin(w, h) + 1e-6);
    return r.min_area <= area && area <= r.max_area && aspect < r.max_aspect && w > r.min_side && h > r.min_side;
  }
  if (area < r.min_area) return false;
  const double aspect = fmax(w, h) / (fmin(w, h) + 1e-6);
  if (aspect < r.min_aspect) return false;
  const double cx = (double)sm[(size_t)l * 2] / area;
  const double roi_center_x = r.roi_width / 2.0;
  const double off = fabs(cx - roi_center_x) / r.roi_width;
  if (off > r.max_center_offset) return false;
  const double sc = area * aspect * (1.0 - off);
  *score = sc;
  return sc > -1.0;                                          // best_score starts at -1 in the reference
}

__global__ void __launch_bounds__(CC_THREADS) cc_select_kernel(const int* __restrict__ num, const int* __restrict__ stats,
                                                              const unsigned long long* __restrict__ sums, int H, int K, int rule,
                                                              CcRule r, uint8_t* __restrict__ keep) {
  __shared__ double sc[CC_THREADS];
  __shared__ int lb[CC_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const int* st = stats + (size_t)b * K * 5;
  const unsigned long long* sm = sums + (size_t)b * K * 2;
  uint8_t* kp = keep + (size_t)b * K;
  const int n = num[b] <= K ? num[b] : 0;
  int best = -1;
  if (!cc_keeps_all(rule)) {
    double bs = 0.0;
    for (int l = 1 + t; l < n; l += CC_THREADS) {            // ascending labels: '>' keeps the first of equal scores
      double s;
      if (cc_candidate(st, sm, l, rule, r, H, &s) && (best < 0 || s > bs)) { bs = s; best = l; }
    }
    sc[t] = bs; lb[t] = best;
    __syncthreads();
    for (int d = CC_THREADS / 2; d > 0; d >>= 1) {
      if (t < d) {
        const int ol = lb[t + d];
        const double os = sc[t + d];
        if (ol >= 0 && (lb[t] < 0 || os > sc[t] || (os == sc[t] && ol < lb[t]))) { sc[t] = os; lb[t] = ol; }
      }
      __syncthreads();
    }
    best = lb[0];
  }
  for (int l = t; l < K; l += CC_THREADS) {
    bool k = false;
    double s;
    if (l >= 1 && l < n) k = cc_keeps_all(rule) ? cc_candidate(st, sm, l, rule, r, H, &s) : l == best;
    kp[l] = k ? 1 : 0;
  }
}

// out = keep[label] ? out_value : 0; grid (chunks, B), one 16-byte store per thread
__global__ void __launch_bounds__(CC_THREADS) cc_apply_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ keep, int HW, int K,
                                                             int vec_ok, unsigned out_value, uint8_t* __restrict__ out) {
  const int i0 = blockIdx.x * CC_CHUNK + threadIdx.x * CC_PX;
  if (i0 >= HW) return;
  const int* lab = labels + (size_t)blockIdx.y * HW;
  const uint8_t* kp = keep + (size_t)blockIdx.y * K;
  uint8_t* dst = out + (size_t)blockIdx.y * HW;
  if (vec_ok && i0 + CC_PX <= HW) {
    unsigned wv[4] = {0, 0, 0, 0};
    const int4* src = reinterpret_cast<const int4*>(lab + i0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 v = src[q];
      const int l[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (l[k] > 0 && l[k] < K && kp[l[k]]) wv[q] |= out_value << (8 * k);
    }
    *reinterpret_cast<uint4*>(dst + i0) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  } else {
    for (int j = 0; j < CC_PX && i0 + j < HW; ++j) {
      const int l = lab[i0 + j];
      dst[i0 + j] = (l > 0 && l < K && kp[l]) ? (uint8_t)out_value : 0;
    }
  }
}

}  // namespace unetpp
