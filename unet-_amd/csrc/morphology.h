// morphology.h — binary morphology programs on uint8 class masks (cv2.dilate / erode / morphologyEx with a
// structuring element, BORDER_CONSTANT with morphologyDefaultBorderValue), one launch per program.
//
// morph_program_kernel: a workgroup owns a tile of `band` rows x `cw` 64-pixel words of one frame plus a halo of the
// program's total reach on every side (recomputed, never exchanged: no workgroup waits for another).  The tile's
// foreground bits of mask0 / mask1 are packed into LDS (planes 0, 1: one bit per pixel, bit j of word k = pixel
// 64 k + j of the row), every step of the program runs on whole LDS planes (planes 2, 3 are scratch, plane 4 is the
// kernel's own ping-pong buffer for iterations), and the result plane's core goes out as out_value / 0 bytes.
//
//   dilate(x)(p) = OR  over the element's non-zeros (i, j) of x(p + (j - ax, i - ay))      (not reflected: cv2's)
//   erode(x)(p)  = AND over the same offsets = ~dilate(~x)(p) with the SAME offsets
// Border rule: a pixel outside the image never contributes (0 for a dilate, 1 for an erode, i.e. 0 of ~x).  It is
// applied where a step READS its source (morph_step_plane: source rows outside the image are skipped, words outside
// it are masked to 0 and the bits past W in a row's last word are cleared, all after the erode's inversion), so it
// holds before every step and every iteration whatever an earlier step left in the halo rows or in the bits past W.
//
// Per output word: the element's rows arrive sorted by their run (lo, hi) of column offsets; the source rows of one
// run are ORed first (three words: left neighbour, own, right neighbour; kw <= 63 keeps the reach inside them), then
// ONE shift-and-OR doubling (morph_widen) widens the run, so an ellipse costs one doubling per distinct run
// (E15: 5, E21: 7, E25: 8), not one per row.
//
// The rect-element shortcut of cv2 (n iterations = one pass with an enlarged element and a scaled anchor) is not
// imitated: iterations repeat the step.  It gives the same result except for an anchor that is not the centre.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "components.h"

namespace unetpp {

constexpr int MORPH_THREADS = 256;
constexpr int MORPH_MAX_STEPS = 8, MORPH_MAX_ELEMENTS = 4, MORPH_MAX_K = 63;
constexpr int MORPH_USER_PLANES = 4, MORPH_PLANES = 5;      // plane 4: the kernel's ping-pong buffer
constexpr int MORPH_PLANE_WORDS = 1536;                     // 5 planes x 1536 words x 8 bytes = 60 KB of LDS at most
constexpr int MORPH_MAX_REACH = 126;                        // sum of iterations * (k - 1) over the morphological steps, per axis

enum { MORPH_DILATE = 0, MORPH_ERODE = 1, MORPH_AND = 2, MORPH_ANDNOT = 3, MORPH_OR = 4, MORPH_COPY = 5 };

struct MorphRow { signed char dy, lo, hi, pad; };           // source row offset i - ay, column offsets first - ax .. last - ax
struct MorphElem { int nrows; MorphRow row[MORPH_MAX_K]; }; // non-empty rows only, sorted by (lo, hi)
struct MorphStep { int op, dst, a, b, elem, iters; };
struct MorphArgs {
  MorphElem elem[MORPH_MAX_ELEMENTS];
  MorphStep step[MORPH_MAX_STEPS];
  int n_steps, result;
  int H, W, wpr;                    // wpr = words per image row
  int band, up, rows;               // core rows, halo rows above, rows in LDS (band + up + down)
  int cw, hl, tw;                   // core words, halo words to the left, words per LDS row (cw + hl + hr)
  int match0, match1;
  unsigned out_value;
  int vec0, vec1, vec_out;          // 16-byte accesses allowed (W % 16 == 0 and the pointer is 16-byte aligned)
};

struct MorphTile {                  // where this workgroup's LDS window lies in the image
  int y_org, w_org;                 // image row of LDS row 0, image word of LDS column 0
  int rows, tw, H, wpr;
  unsigned long long tail;          // valid bits of a row's last word
};

// 16 foreground bits of 16 consecutive mask bytes
__device__ __forceinline__ unsigned morph_bits16(const uint4 v, int match_class) {
  const unsigned wv[4] = {v.x, v.y, v.z, v.w};
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) bits |= (unsigned)cc_is_fg((wv[j >> 2] >> (8 * (j & 3))) & 0xffu, match_class) << j;
  return bits;
}

// Plane <- foreground bits of the tile's window of `mask` (all zero for mask == nullptr and outside the image).
// One item = 16 pixels = one unsigned short of the plane; four independent 16-byte loads in flight per thread.
__device__ __forceinline__ void morph_load_plane(unsigned long long* plane, const uint8_t* __restrict__ mask, int match_class, int vec,
                                                 const MorphTile& t, int W) {
  unsigned short* p16 = reinterpret_cast<unsigned short*>(plane);
  const int items = t.rows * t.tw * 4;
  for (int base = threadIdx.x; base < items; base += MORPH_THREADS * 4) {
    uint4 v[4];
    int kind[4];                    // 0: zeros, 1: v holds 16 bytes, 2: ragged (read byte by byte)
    const uint8_t* src[4];
    int left[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = base + u * MORPH_THREADS;
      kind[u] = 0; src[u] = nullptr; left[u] = 0;
      v[u] = make_uint4(0, 0, 0, 0);
      if (it >= items || !mask) continue;
      const int wc = it >> 2, r = wc / t.tw, c = wc - r * t.tw;
      const int y = t.y_org + r, gw = t.w_org + c, x = gw * 64 + (it & 3) * 16;
      if (y < 0 || y >= t.H || gw < 0 || x >= W) continue;
      src[u] = mask + (size_t)y * W + x;
      left[u] = W - x;
      if (vec && left[u] >= 16) { kind[u] = 1; v[u] = *reinterpret_cast<const uint4*>(src[u]); }
      else kind[u] = 2;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = base + u * MORPH_THREADS;
      if (it >= items) continue;
      unsigned bits = 0;
      if (kind[u] == 1) bits = morph_bits16(v[u], match_class);
      else if (kind[u] == 2)
        for (int j = 0; j < 16 && j < left[u]; ++j) bits |= (unsigned)cc_is_fg(src[u][j], match_class) << j;
      p16[it] = (unsigned short)bits;
    }
  }
}

// OR over d in [lo, hi] of the 192-bit window (t0 = left word, t1 = own, t2 = right) read at pixel offset d, for the
// own word: x = the 128 bits of the window from bit 64 + lo, then x |= x >> s by doubling until the run's n = hi - lo + 1
// offsets are covered (s <= 31: n <= 63), result = the low 64 bits.  -62 <= lo <= hi <= 62.  On 32-bit words: the
// funnel shifts are v_alignbit_b32, full rate, where a 64-bit shift is not.
__device__ __forceinline__ unsigned long long morph_widen(unsigned long long t0, unsigned long long t1, unsigned long long t2, int lo, int hi) {
  const unsigned w0 = (unsigned)t0, w1 = (unsigned)(t0 >> 32), w2 = (unsigned)t1, w3 = (unsigned)(t1 >> 32), w4 = (unsigned)t2,
                 w5 = (unsigned)(t2 >> 32);
  const int sh = 64 + lo, q = sh >> 5;          // 2 <= sh <= 126
  const unsigned b = (unsigned)(sh & 31);
  unsigned a0, a1, a2, a3, a4;
  if (q == 0) { a0 = w0; a1 = w1; a2 = w2; a3 = w3; a4 = w4; }
  else if (q == 1) { a0 = w1; a1 = w2; a2 = w3; a3 = w4; a4 = w5; }
  else if (q == 2) { a0 = w2; a1 = w3; a2 = w4; a3 = w5; a4 = 0; }
  else { a0 = w3; a1 = w4; a2 = w5; a3 = 0; a4 = 0; }
  unsigned x0 = __builtin_amdgcn_alignbit(a1, a0, b), x1 = __builtin_amdgcn_alignbit(a2, a1, b),
           x2 = __builtin_amdgcn_alignbit(a3, a2, b), x3 = __builtin_amdgcn_alignbit(a4, a3, b);
  const int n = hi - lo + 1;
  for (int cov = 1; cov < n;) {
    const unsigned s = (unsigned)min(cov, n - cov);          // 1 .. 31
    x0 |= __builtin_amdgcn_alignbit(x1, x0, s);
    x1 |= __builtin_amdgcn_alignbit(x2, x1, s);
    x2 |= __builtin_amdgcn_alignbit(x3, x2, s);
    x3 |= x3 >> s;
    cov += (int)s;
  }
  return ((unsigned long long)x1 << 32) | x0;
}

// dst = dilate(src) (inv = false) or erode(src) (inv = true) over the whole LDS window; dst != src.
// The border rule lives in the three column masks (0 for a word outside the LDS window or the image, the valid bits
// for a row's last word) and in the range [dmin, dmax] of source-row offsets that stay inside the window and the image;
// an erode reads ~src through them, so what lies outside contributes nothing to either.
__device__ __forceinline__ void morph_step_plane(const unsigned long long* src, unsigned long long* dst, const MorphElem& E, bool inv,
                                                 const MorphTile& t) {
  const int pw = t.rows * t.tw;
  const unsigned long long flip = inv ? ~0ull : 0ull;
  for (int idx = threadIdx.x; idx < pw; idx += MORPH_THREADS) {
    const int r = idx / t.tw, c = idx - r * t.tw, gw = t.w_org + c, y = t.y_org + r;
    auto colmask = [&](int cc, int g) -> unsigned long long {
      if (cc < 0 || cc >= t.tw || g < 0 || g >= t.wpr) return 0ull;
      return g == t.wpr - 1 ? t.tail : ~0ull;
    };
    const unsigned long long m0 = colmask(c - 1, gw - 1), m1 = colmask(c, gw), m2 = colmask(c + 1, gw + 1);
    const int i0 = c > 0 ? -1 : 0, i2 = c + 1 < t.tw ? 1 : 0;          // a masked-out neighbour reads the own word instead
    const int dmin = max(-r, -y), dmax = min(t.rows - 1 - r, t.H - 1 - y);
    unsigned long long acc = 0, t0 = 0, t1 = 0, t2 = 0;
    int lo = E.row[0].lo, hi = E.row[0].hi;
    for (int k = 0; k < E.nrows; ++k) {
      const MorphRow row = E.row[k];
      if (row.lo != lo || row.hi != hi) {
        acc |= morph_widen(t0 & m0, t1 & m1, t2 & m2, lo, hi);
        t0 = t1 = t2 = 0;
        lo = row.lo; hi = row.hi;
      }
      if (row.dy < dmin || row.dy > dmax) continue;                      // outside the image: contributes nothing
      const unsigned long long* p = src + (r + row.dy) * t.tw + c;
      if (row.lo < 0) t0 |= p[i0] ^ flip;
      t1 |= p[0] ^ flip;
      if (row.hi > 0) t2 |= p[i2] ^ flip;
    }
    acc |= morph_widen(t0 & m0, t1 & m1, t2 & m2, lo, hi);
    dst[idx] = acc ^ flip;
  }
}

// grid (tiles in x, bands, B), MORPH_THREADS threads, dynamic LDS = MORPH_PLANES * rows * tw * 8 bytes.
__global__ void __launch_bounds__(MORPH_THREADS) morph_program_kernel(const uint8_t* __restrict__ mask0, const uint8_t* __restrict__ mask1,
                                                                     uint8_t* __restrict__ out, const MorphArgs A) {
  extern __shared__ unsigned long long morph_lds[];
  MorphTile t;
  t.y_org = (int)blockIdx.y * A.band - A.up;
  t.w_org = (int)blockIdx.x * A.cw - A.hl;
  t.rows = A.rows; t.tw = A.tw; t.H = A.H; t.wpr = A.wpr;
  t.tail = (A.W & 63) ? (1ull << (A.W & 63)) - 1ull : ~0ull;
  const int pw = A.rows * A.tw;
  const size_t frame = (size_t)blockIdx.z * A.H * A.W;
  morph_load_plane(morph_lds, mask0 + frame, A.match0, A.vec0, t, A.W);
  morph_load_plane(morph_lds + pw, mask1 ? mask1 + frame : nullptr, A.match1, A.vec1, t, A.W);
  __syncthreads();

  unsigned long long* const tmp = morph_lds + (size_t)(MORPH_PLANES - 1) * pw;
  for (int s = 0; s < A.n_steps; ++s) {
    const MorphStep st = A.step[s];
    unsigned long long* const dst = morph_lds + (size_t)st.dst * pw;
    const unsigned long long* const a = morph_lds + (size_t)st.a * pw;
    if (st.op == MORPH_DILATE || st.op == MORPH_ERODE) {
      // iteration it writes dst when an even number of iterations follow it, else tmp, so that the last one lands in
      // dst; with dst == a the first must go to tmp: for an odd count the roles swap and tmp is copied at the end
      const int n = st.iters;
      const bool swap = st.dst == st.a && (n & 1);
      const unsigned long long* cur = a;
      for (int it = 0; it < n; ++it) {
        const bool to_dst = (((n - 1 - it) & 1) == 0) != swap;
        unsigned long long* o = to_dst ? dst : tmp;
        morph_step_plane(cur, o, A.elem[st.elem], st.op == MORPH_ERODE, t);
        __syncthreads();
        cur = o;
      }
      if (cur != dst) {
        for (int i = threadIdx.x; i < pw; i += MORPH_THREADS) dst[i] = cur[i];
        __syncthreads();
      }
    } else {
      const unsigned long long* const b = morph_lds + (size_t)st.b * pw;
      for (int i = threadIdx.x; i < pw; i += MORPH_THREADS) {
        const unsigned long long va = a[i], vb = b[i];
        dst[i] = st.op == MORPH_AND ? (va & vb) : st.op == MORPH_ANDNOT ? (va & ~vb) : st.op == MORPH_OR ? (va | vb) : va;
      }
      __syncthreads();
    }
  }

  // the core of the result plane: 16 pixels (one unsigned short of the plane, one 16-byte store) per item
  const unsigned short* res16 = reinterpret_cast<const unsigned short*>(morph_lds + (size_t)A.result * pw);
  const int items = A.band * A.cw * 4;
  for (int it = threadIdx.x; it < items; it += MORPH_THREADS) {
    const int wc = it >> 2, rb = wc / A.cw, cb = wc - rb * A.cw;
    const int r = rb + A.up, c = cb + A.hl;
    const int y = t.y_org + r, x = (t.w_org + c) * 64 + (it & 3) * 16;
    if (y >= A.H || x >= A.W) continue;
    const unsigned bits = res16[(r * A.tw + c) * 4 + (it & 3)];
    uint8_t* d = out + frame + (size_t)y * A.W + x;
    if (A.vec_out && x + 16 <= A.W) {
      unsigned wv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned nb = (bits >> (4 * q)) & 0xfu;
        wv[q] = ((nb & 1u) | ((nb & 2u) << 7) | ((nb & 4u) << 14) | ((nb & 8u) << 21)) * A.out_value;
      }
      *reinterpret_cast<uint4*>(d) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
    } else {
      for (int j = 0; j < 16 && x + j < A.W; ++j) d[j] = ((bits >> j) & 1u) ? (uint8_t)A.out_value : (uint8_t)0;
    }
  }
}

}  // namespace unetpp
