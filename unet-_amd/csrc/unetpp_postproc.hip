// unetpp_postproc.hip — the post-processing entry points of the C ABI (include/unetpp.h): mask statistics, connected
// components and their filters, the grey-level burr detectors, measurements, the distance transform and the robust loop's mask rules,
// grey-frame enhancement and denoising, evaluation, the probability-map rules, morphology, the two resizes and the tiling of sliding-window inference.  Each entry checks its arguments and queues kernels on the caller's
// stream.  Of an engine this file sees unetpp_engine_common (abi_common.h) and nothing else: no tensor, layer, arena or stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/unetpp_contours.h"
#include "../../include/unetpp_loss.h"
#include "../../include/unetpp_loss_grad.h"
#include "../../include/unetpp_raw.h"
#include "../../include/unetpp_roi.h"
#include "../../include/unetpp_simple_loops.h"
#include "../../include/unetpp_train_batch.h"
#include "../../include/unetpp_two_stage.h"
#include "abi_common.h"
#include "components.h"
#include "contours.h"
#include "distance.h"
#include "edges.h"
#include "edges_multi.h"
#include "enhance.h"
#include "evaluation.h"
#include "frame_kernels.h"
#include "geometry.h"
#include "loss.h"
#include "loss_grad.h"
#include "morphology.h"
#include "multiclass.h"
#include "nlmeans.h"
#include "probmap.h"
#include "raw_frames.h"
#include "roi_loop.h"
#include "simple_loops.h"
#include "tiling.h"
#include "train_batch.h"
#include "two_stage.h"

using namespace unetpp;

// ---- the vocabulary of the checks and launches: written once, each entry passes its own limits ---------------------------
namespace {

#define REQUIRE_ARGS(e, all_given)           \
  if (!(e)) return UNETPP_E_INVALID;         \
  if (!(all_given)) return fail(e, UNETPP_E_INVALID, "null argument")

// every entry ends with it: a launch the runtime refused shows here
int launched(unetpp_engine* e) {
  HIP_TRY(e, hipGetLastError());
  return UNETPP_OK;
}

// The limits differ between entries on purpose: the smallest side an algorithm takes, the largest a grid dimension or a
// 16-bit coordinate holds, h * w <= 2^30 where pixel indices are 32-bit.  batch is always a grid dimension.
struct ShapeLimits { int min_side, max_side; bool pixel_cap; };
constexpr int MAX_DIM = 65535;
constexpr ShapeLimits MASK_SHAPE{1, MAX_DIM, true}, EDGE_SHAPE{8, MAX_DIM, true}, BAND_SHAPE{2, MAX_DIM, true},
                      GRAY_SHAPE{1, INT_MAX, true}, ROWS_SHAPE{1, MAX_DIM, false}, NLM_SHAPE{NLM_MIN_SIDE, MAX_DIM, true};
bool shape_ok(int batch, int h, int w, const ShapeLimits& lim) {
  return batch >= 1 && batch <= MAX_DIM && h >= lim.min_side && w >= lim.min_side && h <= lim.max_side && w <= lim.max_side &&
         (!lim.pixel_cap || (size_t)h * w <= (1u << 30));
}

// do [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const char* p = (const char*)a; const char* q = (const char*)b;
  return p < q + nb && q < p + na;
}

// may a kernel use 16-byte loads / stores: rows (or images) of n bytes behind 16-byte aligned pointers
template <class... P>
int vec16(int n, const P*... p) { return n % 16 == 0 && (((uintptr_t)p | ... | (uintptr_t)0) % 16) == 0; }

dim3 tile_grid(int w, int h, int tw, int th, int batch) {
  return dim3((unsigned)((w + tw - 1) / tw), (unsigned)((h + th - 1) / th), (unsigned)batch);
}

}  // namespace

// One C block to the end of the file: the entry points, and next to each family its own checks and layouts (static).
extern "C" {

int unetpp_mask_stats(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, uint32_t* dev_counts,
                      int32_t* dev_row_min, int32_t* dev_row_max, void* stream) {
  REQUIRE_ARGS(e, dev_mask && dev_counts && dev_row_min && dev_row_max);
  if (batch < 1 || h < 1 || w < 1) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int C = unetpp_common(e)->cfg.num_classes;
  HIP_TRY(e, hipMemsetAsync(dev_counts, 0, (size_t)batch * C * sizeof(uint32_t), s));
  hipLaunchKernelGGL(mask_stats_kernel, dim3((unsigned)h, (unsigned)batch), dim3(256), 0, s, dev_mask, C, h, w,
                     (unsigned*)dev_counts, (int*)dev_row_min, (int*)dev_row_max);
  return launched(e);
}

// ---- connected components + the reference's component filters (components.h) -----------------------------------
struct CcWorkspace {
  size_t parent = 0, chunks = 0, keep = 0, total = 0;   // byte offsets
  int nchunk = 0;
};
static bool cc_layout(int batch, int h, int w, int capacity, CcWorkspace* ws) {
  if (!shape_ok(batch, h, w, MASK_SHAPE) || capacity < 2) return false;
  const size_t hw = (size_t)h * w;
  ws->nchunk = (int)((hw + CC_CHUNK - 1) / CC_CHUNK);
  Carve c;
  ws->parent = c.take(hw * batch * sizeof(int));
  ws->chunks = c.take((size_t)ws->nchunk * batch * sizeof(int));
  ws->keep = c.take((size_t)capacity * batch);
  ws->total = c.end;
  return true;
}
// The labelling chain both users share: union-find inside the tiles, merge across their borders, path compression.
// Afterwards parent[] holds every pixel's root (-1: background) and chunks[] the number of roots in each raster chunk.
static void launch_roots(hipStream_t s, const uint8_t* mask, int batch, int h, int w, int match_class, int conn8, int mask_vec, int nchunk,
                         int* parent, int* chunks) {
  const dim3 blk(CC_THREADS), tiles = tile_grid(w, h, CC_TW, CC_TH, batch);
  const int ntx = (int)tiles.x, nty = (int)tiles.y, hw = h * w;
  hipLaunchKernelGGL(cc_tile_kernel, tiles, blk, 0, s, mask, h, w, match_class, conn8, mask_vec, parent);
  const long long items = (long long)(nty - 1) * w + 2LL * (ntx - 1) * h;
  if (items > 0)
    hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)((items + CC_THREADS - 1) / CC_THREADS), (unsigned)batch), blk, 0, s, parent, h, w,
                       conn8, nty - 1, ntx - 1);
  hipLaunchKernelGGL(cc_compress_kernel, dim3((unsigned)nchunk, (unsigned)batch), blk, 0, s, parent, hw, (int)(hw % 4 == 0), chunks);
}
// The launches both filters end with: keep[] = the components the rule keeps, then dev_out = out_value where a pixel's label is kept.
static int launch_select_apply(unetpp_engine* e, hipStream_t s, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats,
                               const uint64_t* dev_sums, int batch, int h, int w, int capacity, int rule, const CcRule& r, uint8_t out_value,
                               uint8_t* dev_out, void* dev_workspace) {
  CcWorkspace ws;
  if (!cc_layout(batch, h, w, capacity, &ws)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  ENTER_DEVICE(e);
  const int hw = h * w;
  uint8_t* keep = (uint8_t*)dev_workspace + ws.keep;
  hipLaunchKernelGGL(cc_select_kernel, dim3((unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_num, (const int*)dev_stats,
                     (const unsigned long long*)dev_sums, h, capacity, rule, r, keep);
  hipLaunchKernelGGL(cc_apply_kernel, dim3((unsigned)ws.nchunk, (unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_labels,
                     (const uint8_t*)keep, hw, capacity, vec16(hw, dev_labels, dev_out), (unsigned)out_value, dev_out);
  return launched(e);
}

size_t unetpp_components_workspace_bytes(int batch, int h, int w, int capacity) {
  CcWorkspace ws;
  return cc_layout(batch, h, w, capacity, &ws) ? ws.total : 0;
}

int unetpp_components(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, int match_class, int connectivity,
                      int capacity, int32_t* dev_labels, int32_t* dev_num, int32_t* dev_stats, uint64_t* dev_sums,
                      void* dev_workspace, void* stream) {
  REQUIRE_ARGS(e, dev_mask && dev_labels && dev_num && dev_workspace);
  if ((dev_stats == nullptr) != (dev_sums == nullptr)) return fail(e, UNETPP_E_INVALID, "dev_stats and dev_sums go together (both or neither)");
  if (connectivity != 4 && connectivity != 8) return fail(e, UNETPP_E_INVALID, "connectivity must be 4 or 8, got %d", connectivity);
  if (capacity < 2) return fail(e, UNETPP_E_INVALID, "capacity %d: at least 2 rows (background + one component)", capacity);
  if (match_class > 255) return fail(e, UNETPP_E_INVALID, "match_class %d out of range", match_class);
  CcWorkspace ws;
  if (!cc_layout(batch, h, w, capacity, &ws)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  if ((uintptr_t)dev_workspace % 16) return fail(e, UNETPP_E_INVALID, "dev_workspace must be 16-byte aligned");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w, conn8 = connectivity == 8;
  int* parent = (int*)((char*)dev_workspace + ws.parent);
  int* chunks = (int*)((char*)dev_workspace + ws.chunks);
  const dim3 blk(CC_THREADS), per_px((unsigned)ws.nchunk, (unsigned)batch);
  if (dev_stats) {
    HIP_TRY(e, hipMemsetAsync(dev_stats, 0, (size_t)batch * capacity * 5 * sizeof(int32_t), s));
    HIP_TRY(e, hipMemsetAsync(dev_sums, 0, (size_t)batch * capacity * 2 * sizeof(uint64_t), s));
  }
  launch_roots(s, dev_mask, batch, h, w, match_class, conn8, vec16(w, dev_mask), ws.nchunk, parent, chunks);
  const int par_vec = hw % 4 == 0;             // the workspace is 16-byte aligned and `parent` starts it
  hipLaunchKernelGGL(cc_scan_kernel, dim3((unsigned)batch), blk, 0, s, chunks, ws.nchunk, (int*)dev_num);
  hipLaunchKernelGGL(cc_number_kernel, per_px, blk, 0, s, parent, hw, par_vec, (const int*)chunks);
  const int lab_vec = par_vec && (uintptr_t)dev_labels % 16 == 0;
  hipLaunchKernelGGL(cc_relabel_kernel, per_px, blk, 0, s, (const int*)parent, h, w, capacity, lab_vec, (int*)dev_labels, (int*)dev_stats,
                     (unsigned long long*)dev_sums);
  if (dev_stats)
    hipLaunchKernelGGL(cc_finish_stats_kernel, dim3((unsigned)((capacity + CC_THREADS - 1) / CC_THREADS), (unsigned)batch), blk, 0, s,
                       (int*)dev_stats, h, w, capacity);
  return launched(e);
}

int unetpp_components_filter(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats,
                             const uint64_t* dev_sums, int batch, int h, int w, int capacity, int rule, const unetpp_cc_rule* params,
                             uint8_t out_value, uint8_t* dev_out, void* dev_workspace, void* stream) {
  REQUIRE_ARGS(e, dev_labels && dev_num && dev_stats && dev_sums && params && dev_out && dev_workspace);
  if (rule != UNETPP_CC_LARGEST && rule != UNETPP_CC_SPATIAL && rule != UNETPP_CC_CABLE_SHAPE) return fail(e, UNETPP_E_INVALID, "unknown rule %d", rule);
  if (capacity < 2) return fail(e, UNETPP_E_INVALID, "capacity %d: at least 2 rows (background + one component)", capacity);
  if (rule == UNETPP_CC_CABLE_SHAPE && !(params->roi_width > 0)) return fail(e, UNETPP_E_INVALID, "roi_width must be positive");
  CcRule r{params->min_area, params->min_width, params->max_width, params->min_height_ratio, params->min_aspect,
           params->max_center_offset, params->roi_width};
  return launch_select_apply(e, (hipStream_t)stream, dev_labels, dev_num, dev_stats, dev_sums, batch, h, w, capacity, rule, r, out_value, dev_out,
                             dev_workspace);
}

int unetpp_components_filter_box(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats,
                                 int batch, int h, int w, int capacity, const unetpp_cc_box_rule* params, uint8_t out_value,
                                 uint8_t* dev_out, void* dev_workspace, void* stream) {
  REQUIRE_ARGS(e, dev_labels && dev_num && dev_stats && params && dev_out && dev_workspace);
  if (capacity < 2) return fail(e, UNETPP_E_INVALID, "capacity %d: at least 2 rows (background + one component)", capacity);
  if (std::isnan(params->min_area) || std::isnan(params->max_area) || std::isnan(params->max_aspect) || std::isnan(params->min_side))
    return fail(e, UNETPP_E_INVALID, "box rule: NaN parameter");
  CcRule r{};
  r.min_area = params->min_area; r.max_area = params->max_area; r.max_aspect = params->max_aspect; r.min_side = params->min_side;
  return launch_select_apply(e, (hipStream_t)stream, dev_labels, dev_num, dev_stats, nullptr, batch, h, w, capacity, (int)CC_RULE_BOX, r, out_value,
                             dev_out, dev_workspace);      // the box rule reads no sums
}

// ---- grey-level front end of the burr detection (edges.h) -----------------------------------------------------------
struct CannyWorkspace {
  size_t parent = 0, chunks = 0, map = 0, flags = 0, total = 0;   // byte offsets
  int nchunk = 0;
};
static bool canny_layout(int batch, int h, int w, CannyWorkspace* ws) {
  if (!shape_ok(batch, h, w, EDGE_SHAPE)) return false;
  const size_t hw = (size_t)h * w;
  ws->nchunk = (int)((hw + CC_CHUNK - 1) / CC_CHUNK);
  Carve c;
  ws->parent = c.take(hw * batch * sizeof(int));
  ws->chunks = c.take((size_t)ws->nchunk * batch * sizeof(int));
  ws->map = c.take(hw * batch);
  ws->flags = c.take(hw * batch);
  ws->total = c.end;
  return true;
}
// The blur / Canny family tells a call that makes no sense from a shape its kernels do not take.
static int edge_shape_check(unetpp_engine* e, int batch, int h, int w) {
  if (batch < 1 || h < 1 || w < 1) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  if (!shape_ok(batch, h, w, EDGE_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "shape %dx%dx%d outside 8 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  return UNETPP_OK;
}
// taps == NULL: no blur (the identity tap).  Otherwise n_taps odd, <= 7, every tap in [0,256], sum 256, symmetric or not.
static int edge_taps(unetpp_engine* e, const int32_t* taps, int n_taps, EdgeTaps* out) {
  std::memset(out, 0, sizeof *out);
  if (!taps) { out->n = 1; out->t[0] = 256; return UNETPP_OK; }
  if (n_taps < 1 || n_taps % 2 == 0) return fail(e, UNETPP_E_INVALID, "n_taps %d: must be odd and positive", n_taps);
  if (n_taps > ED_MAX_TAPS) return fail(e, UNETPP_E_UNSUPPORTED, "n_taps %d: at most %d", n_taps, ED_MAX_TAPS);
  int sum = 0;
  for (int k = 0; k < n_taps; ++k) {
    if (taps[k] < 0 || taps[k] > 256) return fail(e, UNETPP_E_INVALID, "tap %d = %d not in [0,256]", k, (int)taps[k]);
    out->t[k] = taps[k];
    sum += taps[k];
  }
  if (sum != 256) return fail(e, UNETPP_E_INVALID, "taps sum to %d, not 256", sum);
  out->n = n_taps;
  return UNETPP_OK;
}

int unetpp_gray_u8(unetpp_engine* e, const uint8_t* dev_bgr, int batch, int h, int w, uint8_t* dev_gray, void* stream) {
  REQUIRE_ARGS(e, dev_bgr && dev_gray);
  if (!shape_ok(batch, h, w, GRAY_SHAPE)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  ENTER_DEVICE(e);
  const int hw = h * w;
  hipLaunchKernelGGL(gray_kernel, dim3((unsigned)((hw + ED_THREADS - 1) / ED_THREADS), (unsigned)batch), dim3(ED_THREADS), 0, (hipStream_t)stream,
                     dev_bgr, hw, dev_gray);
  return launched(e);
}

int unetpp_canny_layout(int h, int w, int* tile_rows, int* tile_cols) {
  if (!tile_rows || !tile_cols) return fail(nullptr, UNETPP_E_INVALID, "null argument");
  if (!shape_ok(1, h, w, EDGE_SHAPE)) return fail(nullptr, UNETPP_E_UNSUPPORTED, "bad shape %dx%d", h, w);
  *tile_rows = ED_TH;
  *tile_cols = ED_TW;
  return UNETPP_OK;
}

size_t unetpp_canny_workspace_bytes(int batch, int h, int w) {
  CannyWorkspace ws;
  return canny_layout(batch, h, w, &ws) ? ws.total : 0;
}

int unetpp_gaussian_blur_u8(unetpp_engine* e, const uint8_t* dev_gray, int batch, int h, int w, const int32_t* taps, int n_taps,
                            uint8_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_gray && dev_out && taps);
  if (const int rc = edge_shape_check(e, batch, h, w)) return rc;
  EdgeTaps T;
  if (const int rc = edge_taps(e, taps, n_taps, &T)) return rc;
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_gray, n, dev_out, n)) return fail(e, UNETPP_E_INVALID, "dev_out aliases dev_gray: workgroups read halo pixels their neighbours write");
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(edge_map_kernel<true>, tile_grid(w, h, ED_TW, ED_TH, batch), dim3(ED_THREADS), 0, (hipStream_t)stream, dev_gray, h, w, T, 0,
                     0, vec16(w, dev_out), dev_out);
  return launched(e);
}

int unetpp_canny_u8(unetpp_engine* e, const uint8_t* dev_gray, int batch, int h, int w, const int32_t* taps, int n_taps, double low,
                    double high, uint8_t* dev_out, void* dev_workspace, void* stream) {
  REQUIRE_ARGS(e, dev_gray && dev_out && dev_workspace);
  if (const int rc = edge_shape_check(e, batch, h, w)) return rc;
  CannyWorkspace ws;
  canny_layout(batch, h, w, &ws);                            // fails for a bad shape only
  if (!(low >= 0) || !(high >= 0)) return fail(e, UNETPP_E_INVALID, "thresholds must be non-negative numbers");
  if ((uintptr_t)dev_workspace % 16) return fail(e, UNETPP_E_INVALID, "dev_workspace must be 16-byte aligned");
  EdgeTaps T;
  if (const int rc = edge_taps(e, taps, n_taps, &T)) return rc;
  if (low > high) std::swap(low, high);                      // cv2.Canny does the same
  const int ilow = (int)std::floor(std::min(low, 1e6)), ihigh = (int)std::floor(std::min(high, 1e6));
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  int* parent = (int*)((char*)dev_workspace + ws.parent);
  int* chunks = (int*)((char*)dev_workspace + ws.chunks);
  uint8_t* map = (uint8_t*)dev_workspace + ws.map;
  uint8_t* flags = (uint8_t*)dev_workspace + ws.flags;
  static_assert(ED_TW == CC_TW && ED_TH == CC_TH && ED_THREADS == CC_THREADS, "the edge map is labelled in cc_tile_kernel's tiles");
  const dim3 blk(ED_THREADS), per_px((unsigned)ws.nchunk, (unsigned)batch);
  HIP_TRY(e, hipMemsetAsync(flags, 0, (size_t)batch * hw, s));
  const int row_vec = vec16(w);                              // map starts on a 256-byte boundary of the workspace
  hipLaunchKernelGGL(edge_map_kernel<false>, tile_grid(w, h, ED_TW, ED_TH, batch), blk, 0, s, dev_gray, h, w, T, ilow, ihigh, row_vec, map);
  launch_roots(s, map, batch, h, w, -1, 1, row_vec, ws.nchunk, parent, chunks);
  hipLaunchKernelGGL(edge_seed_kernel, per_px, blk, 0, s, (const uint8_t*)map, (const int*)parent, hw, vec16(hw), flags);
  hipLaunchKernelGGL(edge_apply_kernel, per_px, blk, 0, s, (const int*)parent, (const uint8_t*)flags, hw, (int)(hw % 4 == 0),
                     vec16(hw, dev_out), dev_out);
  return launched(e);
}

int unetpp_laplacian_band_u8(unetpp_engine* e, const uint8_t* dev_gray, const uint8_t* dev_band, int batch, int h, int w, int threshold,
                             uint8_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_gray && dev_band && dev_out);
  if (!shape_ok(batch, h, w, BAND_SHAPE)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_gray, n, dev_out, n)) return fail(e, UNETPP_E_INVALID, "dev_out aliases dev_gray: threads read neighbours that others write");
  ENTER_DEVICE(e);
  const long long items = (long long)h * ((w + CC_PX - 1) / CC_PX);
  hipLaunchKernelGGL(laplacian_band_kernel, dim3((unsigned)((items + ED_THREADS - 1) / ED_THREADS), (unsigned)batch), dim3(ED_THREADS), 0,
                     (hipStream_t)stream, dev_gray, dev_band, h, w, threshold, vec16(w, dev_band, dev_out), dev_out);
  return launched(e);
}

// ---- the multi-scale and the DoG burr detectors, has_burr (edges_multi.h) ---------------------------------------
size_t unetpp_edges_union_workspace_bytes(int batch) {
  return batch >= 1 && batch <= 65535 ? align_up((size_t)batch * sizeof(uint32_t), 256) : 0;
}

int unetpp_edges_union_u8(unetpp_engine* e, const uint8_t* dev_gray, const uint8_t* dev_canny, int batch, int h, int w,
                          int sobel_threshold, int laplacian_threshold, void* dev_workspace, uint8_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_gray && dev_canny && dev_workspace && dev_out);
  if (const int rc = edge_shape_check(e, batch, h, w)) return rc;
  if ((uintptr_t)dev_workspace % 16) return fail(e, UNETPP_E_INVALID, "dev_workspace must be 16-byte aligned");
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_gray, n, dev_out, n)) return fail(e, UNETPP_E_INVALID, "dev_out aliases dev_gray: workgroups read halo pixels their neighbours write");
  if (dev_out != dev_canny && overlaps(dev_canny, n, dev_out, n))
    return fail(e, UNETPP_E_INVALID, "dev_out overlaps dev_canny: in place means the same pointer");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  unsigned* smax = (unsigned*)dev_workspace;
  const dim3 blk(ED_THREADS), tiles = tile_grid(w, h, ED_TW, ED_TH, batch);
  const int sthr = std::min(std::max(sobel_threshold, -1), 255), lthr = std::min(std::max(laplacian_threshold, -1), 255);
  HIP_TRY(e, hipMemsetAsync(smax, 0, (size_t)batch * sizeof(unsigned), s));
  hipLaunchKernelGGL(sobel_max_kernel, tiles, blk, 0, s, dev_gray, h, w, smax);
  hipLaunchKernelGGL(edge_union_kernel, tiles, blk, 0, s, dev_gray, dev_canny, h, w, (const unsigned*)smax, sthr, lthr,
                     vec16(w, dev_canny, dev_out), dev_out);
  return launched(e);
}

int unetpp_dog_band_u8(unetpp_engine* e, const uint8_t* dev_gray, const uint8_t* dev_band, int batch, int h, int w, const int32_t* taps1,
                       int n1, const int32_t* taps2, int n2, int threshold, uint8_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_gray && dev_band && dev_out && taps1 && taps2);
  if (const int rc = edge_shape_check(e, batch, h, w)) return rc;
  EdgeTaps T1, T2;
  if (const int rc = edge_taps(e, taps1, n1, &T1)) return rc;
  if (const int rc = edge_taps(e, taps2, n2, &T2)) return rc;
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_gray, n, dev_out, n) || overlaps(dev_band, n, dev_out, n))
    return fail(e, UNETPP_E_INVALID, "dev_out aliases an input: workgroups read halo pixels their neighbours write");
  DogTaps D;
  std::memset(&D, 0, sizeof D);
  for (int k = 0; k < T1.n; ++k) D.t1[ED_MAX_R - T1.n / 2 + k] = T1.t[k];
  for (int k = 0; k < T2.n; ++k) D.t2[ED_MAX_R - T2.n / 2 + k] = T2.t[k];
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(dog_band_kernel, tile_grid(w, h, ED_TW, ED_TH, batch), dim3(ED_THREADS), 0, (hipStream_t)stream, dev_gray, dev_band, h, w, D,
                     std::min(std::max(threshold, -1), 255), vec16(w, dev_band, dev_out), dev_out);
  return launched(e);
}

int unetpp_count_nonzero_u8(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, uint32_t* dev_counts, void* stream) {
  REQUIRE_ARGS(e, dev_mask && dev_counts);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  HIP_TRY(e, hipMemsetAsync(dev_counts, 0, (size_t)batch * sizeof(uint32_t), s));
  hipLaunchKernelGGL(count_nonzero_kernel, dim3((unsigned)((hw + CC_CHUNK - 1) / CC_CHUNK), (unsigned)batch), dim3(ED_THREADS), 0, s, dev_mask, hw,
                     vec16(hw, dev_mask), (unsigned*)dev_counts);
  return launched(e);
}

// ---- measurements: row widths, width profile, component summary (geometry.h) -------------------------------------------
int unetpp_row_widths(unetpp_engine* e, const uint8_t* dev_mask0, int match0, const uint8_t* dev_mask1, int match1, int batch, int h,
                      int w, float* dev_widths, uint32_t* dev_area, void* stream) {
  REQUIRE_ARGS(e, dev_mask0 && dev_widths && dev_area);
  if (!shape_ok(batch, h, w, ROWS_SHAPE)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  if (match0 > 255 || match1 > 255) return fail(e, UNETPP_E_INVALID, "match class %d / %d out of range", match0, match1);
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(e, hipMemsetAsync(dev_area, 0, (size_t)batch * 2 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(row_widths_kernel, dim3((unsigned)((h + GEO_ROWS_PER_WG - 1) / GEO_ROWS_PER_WG), (unsigned)batch), dim3(GEO_THREADS), 0, s,
                     dev_mask0, match0, dev_mask1, match1, h, w, vec16(w, dev_mask0), vec16(w, dev_mask1), dev_widths, (unsigned*)dev_area);
  return launched(e);
}

int unetpp_width_profile(unetpp_engine* e, const float* dev_widths, int batch, int h, const float* taps, int n_taps, int min_valid_rows,
                         float* dev_smoothed, uint8_t* dev_valid, float* dev_delta, unetpp_width_profile_out* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_widths && taps && dev_smoothed && dev_valid && dev_out);
  if (batch < 1 || batch > 65535 || h < 1) return fail(e, UNETPP_E_INVALID, "bad shape %dx%d", batch, h);
  if (h > GEO_MAX_ROWS) return fail(e, UNETPP_E_INVALID, "width_profile: %d rows, at most %d", h, GEO_MAX_ROWS);
  if (n_taps < 1 || n_taps > GEO_MAX_TAPS || n_taps % 2 == 0) return fail(e, UNETPP_E_INVALID, "n_taps %d: odd, 1..%d", n_taps, GEO_MAX_TAPS);
  if (min_valid_rows < 1) return fail(e, UNETPP_E_INVALID, "min_valid_rows %d: at least 1", min_valid_rows);
  const int r = n_taps / 2;
  GeoTaps gt{};
  for (int j = 0; j <= r; ++j) {
    if (!std::isfinite(taps[r + j]) || !(taps[r + j] == taps[r - j])) return fail(e, UNETPP_E_INVALID, "taps must be finite and symmetric");
    gt.t[j] = taps[r + j];
  }
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  static_assert(sizeof(unetpp_width_profile_out) == sizeof(GeoProfileOut), "width profile record");
  hipLaunchKernelGGL(width_profile_kernel, dim3((unsigned)batch), dim3(GEO_THREADS), 2 * (size_t)(h + 2 * r) * sizeof(float), s, dev_widths, h,
                     gt, r, min_valid_rows, dev_smoothed, dev_valid, dev_delta, (GeoProfileOut*)dev_out);
  return launched(e);
}

int unetpp_components_summary(unetpp_engine* e, const int32_t* dev_num, const int32_t* dev_stats, int batch, int capacity, int64_t min_area,
                              int64_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_num && dev_out);
  if (batch < 1 || batch > 65535) return fail(e, UNETPP_E_INVALID, "bad batch %d", batch);
  if (capacity < 2) return fail(e, UNETPP_E_INVALID, "capacity %d: at least 2 rows (background + one component)", capacity);
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(components_summary_kernel, dim3((unsigned)batch), dim3(GEO_THREADS), 0, (hipStream_t)stream, (const int*)dev_num,
                     (const int*)dev_stats, capacity, (long long)min_area, (long long*)dev_out);
  return launched(e);
}

// ---- the robust loop's mask rules: distance transform + ring, best cable, ROI limit, row median (distance.h) ---------------
// These entries answer every bad argument but a NULL engine with UNETPP_E_UNSUPPORTED.
#define REQUIRE_ROBUST(e, all_given)         \
  if (!(e)) return UNETPP_E_INVALID;         \
  if (!(all_given)) return fail(e, UNETPP_E_UNSUPPORTED, "null argument")

struct DtWorkspace { size_t bits = 0, g = 0, flag = 0, total = 0; int nbands = 0; };
static bool dt_layout(int batch, int h, int w, DtWorkspace* ws) {
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return false;
  ws->nbands = (h + DT_BAND - 1) / DT_BAND;
  Carve c;
  ws->bits = c.take((size_t)batch * ws->nbands * w * sizeof(unsigned));
  ws->g = c.take((size_t)batch * h * w * sizeof(uint16_t));
  ws->flag = c.take((size_t)batch * sizeof(int));
  ws->total = c.end;
  return true;
}

size_t unetpp_distance_workspace_bytes(int batch, int h, int w) {
  DtWorkspace ws;
  return dt_layout(batch, h, w, &ws) ? ws.total : 0;
}

int unetpp_distance_transform_u8(unetpp_engine* e, const uint8_t* dev_src, int match_class, int invert, int batch, int h, int w, int metric,
                                 float* dev_dist, const uint8_t* dev_mask1, int match1, float lo, float hi, uint8_t out_value,
                                 uint8_t* dev_ring, void* dev_workspace, void* stream) {
  REQUIRE_ROBUST(e, dev_src && dev_workspace && (dev_dist || dev_ring));
  DtWorkspace ws;
  if (!dt_layout(batch, h, w, &ws)) return fail(e, UNETPP_E_UNSUPPORTED, "shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  unsigned hv, diag;                                         // cvRound(0.955f * 65536), cvRound(1.3693f * 65536); 1, 2; 1, 1
  switch (metric) {
    case UNETPP_DIST_L2: hv = 62587; diag = 89738; break;
    case UNETPP_DIST_L1: hv = 65536; diag = 131072; break;
    case UNETPP_DIST_C: hv = 65536; diag = 65536; break;
    default: return fail(e, UNETPP_E_UNSUPPORTED, "unknown metric %d", metric);
  }
  if (match_class > 255 || match1 > 255) return fail(e, UNETPP_E_UNSUPPORTED, "match class %d / %d out of range", match_class, match1);
  if (dev_ring && out_value == 0) return fail(e, UNETPP_E_UNSUPPORTED, "out_value must not be 0");
  if ((uintptr_t)dev_workspace % 16) return fail(e, UNETPP_E_UNSUPPORTED, "dev_workspace must be 16-byte aligned");
  if ((uintptr_t)dev_dist % 4) return fail(e, UNETPP_E_UNSUPPORTED, "dev_dist must be 4-byte aligned");
  // The ring alone needs no distance above hi: the search starts from a bound two pixels beyond it (the conversion to
  // float32 moves a value by less than 2^-23 of itself).
  unsigned start = DT_CAP;
  if (!dev_dist && hi < 8000.0f) start = (unsigned)((double)(hi > 0.0f ? hi : 0.0f) * 65536.0) + 2u * 65536u;
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  char* wsp = (char*)dev_workspace;
  unsigned* bits = (unsigned*)(wsp + ws.bits);
  uint16_t* g = (uint16_t*)(wsp + ws.g);
  int* flag = (int*)(wsp + ws.flag);
  const size_t lds = (size_t)w * sizeof(uint16_t);
  if (lds > 32 * 1024) HIP_TRY(e, allow_full_lds((const void*)dt_row_kernel, unetpp_common(e)->cfg.device, 128 * 1024));
  HIP_TRY(e, hipMemsetAsync(flag, 0, (size_t)batch * sizeof(int), s));
  const dim3 cols((unsigned)((w + DT_THREADS - 1) / DT_THREADS), (unsigned)ws.nbands, (unsigned)batch);
  hipLaunchKernelGGL(dt_bits_kernel, cols, dim3(DT_THREADS), 0, s, dev_src, h, w, match_class, invert != 0, bits, flag);
  hipLaunchKernelGGL(dt_column_kernel, cols, dim3(DT_THREADS), 0, s, (const unsigned*)bits, h, w, g);
  const DtRing ring{dev_mask1, match1, lo, hi, (unsigned)out_value};
  hipLaunchKernelGGL(dt_row_kernel, dim3((unsigned)h, (unsigned)batch), dim3(DT_THREADS), lds, s, (const uint16_t*)g, (const int*)flag, h, w, hv,
                     diag, start, dev_dist, ring, dev_ring);
  return launched(e);
}

int unetpp_components_best_cable(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats, int batch, int h,
                                 int w, int capacity, double min_area, int min_h, int max_w, double min_aspect, uint8_t out_value,
                                 uint8_t* dev_out, void* dev_workspace, void* stream) {
  REQUIRE_ROBUST(e, dev_labels && dev_num && dev_stats && dev_out && dev_workspace);
  CcWorkspace ws;
  if (capacity < 2 || !cc_layout(batch, h, w, capacity, &ws))
    return fail(e, UNETPP_E_UNSUPPORTED, "bad shape %dx%dx%d or capacity %d", batch, h, w, capacity);
  if (std::isnan(min_area) || std::isnan(min_aspect)) return fail(e, UNETPP_E_UNSUPPORTED, "best cable: NaN parameter");
  if (out_value == 0) return fail(e, UNETPP_E_UNSUPPORTED, "out_value must not be 0");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  uint8_t* keep = (uint8_t*)dev_workspace + ws.keep;
  const BestCableRule r{min_area, min_aspect, min_h, max_w, h, w};
  hipLaunchKernelGGL(best_cable_select_kernel, dim3((unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_num, (const int*)dev_stats, capacity, r,
                     keep);
  hipLaunchKernelGGL(cc_apply_kernel, dim3((unsigned)ws.nchunk, (unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_labels,
                     (const uint8_t*)keep, hw, capacity, vec16(hw, dev_labels, dev_out), (unsigned)out_value, dev_out);
  return launched(e);
}

size_t unetpp_roi_limit_workspace_bytes(int batch) {
  return batch >= 1 && batch <= MAX_DIM ? align_up((size_t)batch * 4 * sizeof(int), 256) : 0;
}

int unetpp_roi_limit_u8(unetpp_engine* e, const uint8_t* dev_mask, const uint8_t* dev_cable, int batch, int h, int w, int pad,
                        uint8_t* dev_out, void* dev_workspace, void* stream) {
  REQUIRE_ROBUST(e, dev_mask && dev_cable && dev_out && dev_workspace);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  if (pad < 0) return fail(e, UNETPP_E_UNSUPPORTED, "pad %d: must not be negative", pad);
  if ((uintptr_t)dev_workspace % 4) return fail(e, UNETPP_E_UNSUPPORTED, "dev_workspace must be 4-byte aligned");
  const size_t n = (size_t)batch * h * w;
  if (dev_out != dev_mask && overlaps(dev_mask, n, dev_out, n)) return fail(e, UNETPP_E_UNSUPPORTED, "dev_out overlaps dev_mask: in place means the same pointer");
  if (overlaps(dev_cable, n, dev_out, n)) return fail(e, UNETPP_E_UNSUPPORTED, "dev_out aliases dev_cable");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  int* box = (int*)dev_workspace;
  HIP_TRY(e, hipMemsetAsync(box, 0xff, (size_t)batch * 4 * sizeof(int), s));
  hipLaunchKernelGGL(roi_box_kernel, dim3((unsigned)((h + 3) / 4), (unsigned)batch), dim3(DT_THREADS), 0, s, dev_cable, h, w, box);
  const int vec = w % 4 == 0 && ((uintptr_t)dev_mask | (uintptr_t)dev_out) % 4 == 0;
  hipLaunchKernelGGL(roi_apply_kernel, dim3((unsigned)((w + 4 * DT_THREADS - 1) / (4 * DT_THREADS)), (unsigned)h, (unsigned)batch), dim3(DT_THREADS), 0,
                     s, dev_mask, (const int*)box, h, w, std::min(pad, MAX_DIM), vec, dev_out);
  return launched(e);
}

int unetpp_row_width_median(unetpp_engine* e, const float* dev_widths, int batch, int h, double* dev_median, void* stream) {
  REQUIRE_ROBUST(e, dev_widths && dev_median);
  if (batch < 1 || batch > MAX_DIM || h < 1 || h > MAX_DIM) return fail(e, UNETPP_E_UNSUPPORTED, "bad shape %dx%d", batch, h);
  if ((uintptr_t)dev_median % 8) return fail(e, UNETPP_E_UNSUPPORTED, "dev_median must be 8-byte aligned");
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(row_median_kernel, dim3(2u, (unsigned)batch), dim3(DT_THREADS), 0, (hipStream_t)stream, dev_widths, h, dev_median);
  return launched(e);
}

// ---- grey-frame enhancement: decision, CLAHE, gamma, bilateral filter (enhance.h) ---------------------------------------
struct EnhWorkspace { size_t gray, hist, sums, luts, decisions, total; };

// CLAHE_Impl::apply's geometry (enhance.clahe_geometry); false outside 1 <= tiles <= 16, h > tiles_y, w > tiles_x
static bool enh_grid(int h, int w, int tiles_x, int tiles_y, EnhGrid* g) {
  if (tiles_x < 1 || tiles_y < 1 || tiles_x > EN_MAX_GRID || tiles_y > EN_MAX_GRID || h <= tiles_y || w <= tiles_x) return false;
  const bool divides = w % tiles_x == 0 && h % tiles_y == 0;
  g->tiles_x = tiles_x; g->tiles_y = tiles_y;
  g->ext_w = divides ? w : w + tiles_x - w % tiles_x;
  g->ext_h = divides ? h : h + tiles_y - h % tiles_y;
  g->tw = g->ext_w / tiles_x; g->th = g->ext_h / tiles_y;
  return true;
}
static bool enh_layout(int batch, int h, int w, int tiles_x, int tiles_y, EnhWorkspace* ws) {
  EnhGrid g;
  if (!shape_ok(batch, h, w, MASK_SHAPE) || !enh_grid(h, w, tiles_x, tiles_y, &g)) return false;
  const size_t tiles = (size_t)tiles_x * tiles_y;
  Carve c;
  ws->gray = c.take((size_t)batch * h * w);
  ws->hist = c.take((size_t)batch * tiles * 256 * sizeof(unsigned));
  ws->sums = c.take((size_t)batch * 3 * sizeof(unsigned long long));          // directly behind hist (whole KiB): one memset clears both
  ws->luts = c.take((size_t)batch * tiles * 256);
  ws->decisions = c.take((size_t)batch);
  ws->total = c.end;
  return true;
}
// Everything the apply kernel indexes its LDS with is checked here.  tables == NULL: no filter.
static int enh_tables(unetpp_engine* e, const uint8_t* gamma_table, const unetpp_bilateral_tables* tables, int h, int w, EnhTables* T) {
  std::memset(T, 0, sizeof *T);
  if (gamma_table) { std::memcpy(T->gamma, gamma_table, 256); T->has_gamma = 1; }
  if (!tables) return UNETPP_OK;
  if (!tables->color_w || !tables->space_w || !tables->dy || !tables->dx) return fail(e, UNETPP_E_INVALID, "bilateral tables: null array");
  const int r = tables->radius, n = tables->n_taps;
  if (r < 1 || r > EN_MAX_R) return fail(e, UNETPP_E_UNSUPPORTED, "bilateral radius %d: 1..%d", r, EN_MAX_R);
  if (h <= r || w <= r) return fail(e, UNETPP_E_UNSUPPORTED, "image %dx%d: needs h, w > radius %d", h, w, r);
  if (n < 1 || n > (2 * r + 1) * (2 * r + 1)) return fail(e, UNETPP_E_INVALID, "bilateral n_taps %d: 1..%d", n, (2 * r + 1) * (2 * r + 1));
  for (int k = 0; k < n; ++k) {
    if (std::abs(tables->dy[k]) > r || std::abs(tables->dx[k]) > r) return fail(e, UNETPP_E_INVALID, "bilateral tap %d lies outside the radius %d", k, r);
    if (!std::isfinite(tables->space_w[k]) || tables->space_w[k] < 0) return fail(e, UNETPP_E_INVALID, "bilateral space weight %d is not finite and non-negative", k);
    T->space_w[k] = tables->space_w[k]; T->dy[k] = (signed char)tables->dy[k]; T->dx[k] = (signed char)tables->dx[k];
  }
  for (int i = 0; i < 256; ++i) {
    if (!std::isfinite(tables->color_w[i]) || tables->color_w[i] < 0) return fail(e, UNETPP_E_INVALID, "bilateral colour weight %d is not finite and non-negative", i);
    T->color_w[i] = tables->color_w[i];
  }
  T->n_taps = n; T->radius = r;
  return UNETPP_OK;
}
static void enh_launch_stats(hipStream_t s, const uint8_t* src, int batch, int h, int w, int cin, const EnhGrid& g, uint8_t* gray, unsigned* hist,
                             unsigned long long* sums) {
  const int area = g.tw * g.th;
  const dim3 grid((unsigned)((area + EN_CHUNK - 1) / EN_CHUNK), (unsigned)(g.tiles_x * g.tiles_y), (unsigned)batch);
  hipLaunchKernelGGL(enhance_stats_kernel, grid, dim3(EN_THREADS), 0, s, src, h, w, cin, g, gray, hist, sums);
}
// clip_limit * tileArea / 256 in double, truncated, at least 1; 0 = no clipping.  A clip of tileArea or more clips nothing.
static int enh_clip(double clip_limit, int area) {
  if (!(clip_limit > 0)) return 0;
  const double c = clip_limit * area / 256;
  return c >= (double)area ? area : std::max((int)c, 1);
}
static int enh_launch_apply(unetpp_engine* e, hipStream_t s, const uint8_t* gray, const uint8_t* luts, const uint8_t* decisions, const uint8_t* frames,
                            int batch, int h, int w, const EnhGrid* g, int cin, int cout, const EnhTables& T, uint8_t* out) {
  EnhApplyArgs A;
  std::memset(&A, 0, sizeof A);
  size_t lds = 0;
  if (g) {
    A.g = *g; A.do_clahe = 1;
    // tiles a window of EN_TH + 2 r rows can touch: ceil(span / th) + 2 (enhance.h), never more than the grid has
    A.lut_rows = std::min(g->tiles_y, (EN_TH + 2 * T.radius + g->th - 1) / g->th + 2);
    A.lut_cols = std::min(g->tiles_x, (EN_TW + 2 * T.radius + g->tw - 1) / g->tw + 2);
    lds = (size_t)A.lut_rows * A.lut_cols * 256;
  } else {
    A.g.tiles_x = A.g.tiles_y = A.g.tw = A.g.th = 1;
  }
  A.cin = cin; A.cout = cout;
  A.vec = w % 4 == 0 && (uintptr_t)out % 4 == 0;
  // the kernel has static LDS too, so the limit asked for is the largest dynamic part (the whole 16 x 16 grid), not all 160 KiB
  if (lds > 32 * 1024) HIP_TRY(e, allow_full_lds((const void*)enhance_apply_kernel, unetpp_common(e)->cfg.device, EN_MAX_GRID * EN_MAX_GRID * 256));
  hipLaunchKernelGGL(enhance_apply_kernel, tile_grid(w, h, EN_TW, EN_TH, batch), dim3(EN_THREADS), lds, s, gray, luts, decisions, frames, h, w, A, T, out);
  return UNETPP_OK;
}

size_t unetpp_enhance_workspace_bytes(int batch, int h, int w, int tiles_x, int tiles_y) {
  EnhWorkspace ws;
  return enh_layout(batch, h, w, tiles_x, tiles_y, &ws) ? ws.total : 0;
}

int unetpp_enhance_layout(int* tile_rows, int* tile_cols) {
  if (!tile_rows || !tile_cols) return fail(nullptr, UNETPP_E_INVALID, "null argument");
  *tile_rows = EN_TH;
  *tile_cols = EN_TW;
  return UNETPP_OK;
}

int unetpp_gray_decision(unetpp_engine* e, const uint8_t* dev_frames, int batch, int h, int w, double threshold, uint8_t* dev_decisions,
                         uint64_t* dev_sums, void* stream) {
  REQUIRE_ARGS(e, dev_frames && dev_decisions && dev_sums);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  if ((uintptr_t)dev_sums % 8) return fail(e, UNETPP_E_INVALID, "dev_sums must be 8-byte aligned");
  if (threshold != threshold) return fail(e, UNETPP_E_INVALID, "threshold is not a number");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  EnhGrid g{1, 1, w, h, h, w};                               // one tile: the image
  HIP_TRY(e, hipMemsetAsync(dev_sums, 0, (size_t)batch * 3 * sizeof(uint64_t), s));
  enh_launch_stats(s, dev_frames, batch, h, w, 3, g, nullptr, nullptr, (unsigned long long*)dev_sums);
  hipLaunchKernelGGL(enhance_decide_kernel, dim3((unsigned)((batch + EN_THREADS - 1) / EN_THREADS)), dim3(EN_THREADS), 0, s,
                     (const unsigned long long*)dev_sums, batch, (double)h * (double)w, threshold, dev_decisions);
  return launched(e);
}

int unetpp_bilateral_u8(unetpp_engine* e, const uint8_t* dev_gray, int batch, int h, int w, const unetpp_bilateral_tables* tables,
                        uint8_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_gray && dev_out && tables);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  EnhTables T;
  if (const int rc = enh_tables(e, nullptr, tables, h, w, &T)) return rc;
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_gray, n, dev_out, n)) return fail(e, UNETPP_E_INVALID, "dev_out aliases dev_gray: workgroups read halo pixels their neighbours write");
  ENTER_DEVICE(e);
  const int lrc = enh_launch_apply(e, (hipStream_t)stream, dev_gray, nullptr, nullptr, nullptr, batch, h, w, nullptr, 1, 1, T, dev_out);
  return lrc != UNETPP_OK ? lrc : launched(e);
}

int unetpp_enhance_u8(unetpp_engine* e, const uint8_t* dev_frames, int batch, int h, int w, int channels_in, int channels_out, int mode,
                      double threshold, double clip_limit, int tiles_x, int tiles_y, const uint8_t* gamma_table,
                      const unetpp_bilateral_tables* tables, uint8_t* dev_out, uint8_t* dev_luts, uint8_t* dev_decisions, void* dev_workspace,
                      void* stream) {
  REQUIRE_ARGS(e, dev_frames && dev_out && dev_workspace);
  if ((channels_in != 1 && channels_in != 3) || (channels_out != 1 && channels_out != 3))
    return fail(e, UNETPP_E_INVALID, "channels %d -> %d: each 1 or 3", channels_in, channels_out);
  if (mode != UNETPP_ENHANCE_ALWAYS && mode != UNETPP_ENHANCE_IF_GREY) return fail(e, UNETPP_E_INVALID, "unknown mode %d", mode);
  if (mode == UNETPP_ENHANCE_IF_GREY && channels_in == 3 && channels_out != 3)
    return fail(e, UNETPP_E_INVALID, "UNETPP_ENHANCE_IF_GREY copies colour frames through: channels_out must be 3");
  if (threshold != threshold || clip_limit != clip_limit) return fail(e, UNETPP_E_INVALID, "threshold or clip_limit is not a number");
  EnhWorkspace ws;
  if (!enh_layout(batch, h, w, tiles_x, tiles_y, &ws))
    return fail(e, UNETPP_E_UNSUPPORTED, "shape %dx%dx%d with a %dx%d grid outside 1 <= tiles <= 16, h > tiles_y, w > tiles_x, h, w <= 65535, h * w <= 2^30",
                batch, h, w, tiles_x, tiles_y);
  if ((uintptr_t)dev_workspace % 16) return fail(e, UNETPP_E_INVALID, "dev_workspace must be 16-byte aligned");
  if (dev_luts && (uintptr_t)dev_luts % 4) return fail(e, UNETPP_E_INVALID, "dev_luts must be 4-byte aligned");
  EnhGrid g;
  enh_grid(h, w, tiles_x, tiles_y, &g);
  EnhTables T;
  if (const int rc = enh_tables(e, gamma_table, tables, h, w, &T)) return rc;
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_frames, n * channels_in, dev_out, n * channels_out))
    return fail(e, UNETPP_E_INVALID, "dev_out aliases dev_frames: workgroups read halo pixels their neighbours write");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  char* wsp = (char*)dev_workspace;
  unsigned* hist = (unsigned*)(wsp + ws.hist);
  unsigned long long* sums = (unsigned long long*)(wsp + ws.sums);
  uint8_t* luts = dev_luts ? dev_luts : (uint8_t*)(wsp + ws.luts);
  uint8_t* decisions = dev_decisions ? dev_decisions : (uint8_t*)(wsp + ws.decisions);
  const bool decide = mode == UNETPP_ENHANCE_IF_GREY && channels_in == 3;      // a one-channel frame is grey by definition
  const uint8_t* gray = channels_in == 3 ? (const uint8_t*)(wsp + ws.gray) : dev_frames;
  const int area = g.tw * g.th;
  HIP_TRY(e, hipMemsetAsync(hist, 0, ws.luts - ws.hist, s));
  enh_launch_stats(s, dev_frames, batch, h, w, channels_in, g, channels_in == 3 ? (uint8_t*)(wsp + ws.gray) : nullptr, hist,
                   channels_in == 3 ? sums : nullptr);
  hipLaunchKernelGGL(clahe_lut_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)batch), dim3(EN_THREADS), 0, s, (const unsigned*)hist,
                     enh_clip(clip_limit, area), 255.0f / (float)area, luts, (const unsigned long long*)sums, (double)h * (double)w, threshold,
                     decide ? 0 : 1, (decide || dev_decisions) ? decisions : (uint8_t*)nullptr);
  const int lrc = enh_launch_apply(e, s, gray, luts, decide ? decisions : nullptr, dev_frames, batch, h, w, &g, channels_in, channels_out, T, dev_out);
  return lrc != UNETPP_OK ? lrc : launched(e);
}

int unetpp_clahe_u8(unetpp_engine* e, const uint8_t* dev_gray, int batch, int h, int w, double clip_limit, int tiles_x, int tiles_y,
                    uint8_t* dev_out, uint8_t* dev_luts, void* dev_workspace, void* stream) {
  return unetpp_enhance_u8(e, dev_gray, batch, h, w, 1, 1, UNETPP_ENHANCE_ALWAYS, 0.0, clip_limit, tiles_x, tiles_y, nullptr, nullptr, dev_out,
                           dev_luts, nullptr, dev_workspace, stream);
}

// ---- non-local-means denoising: cv2.fastNlMeansDenoising(img, None, h, 7, 21) (nlmeans.h) ----------------------------------
int unetpp_nlmeans_layout(int* tile_rows, int* tile_cols) {
  if (!tile_rows || !tile_cols) return fail(nullptr, UNETPP_E_INVALID, "null argument");
  *tile_rows = NLM_TILE_H;
  *tile_cols = NLM_TILE_W;
  return UNETPP_OK;
}

int unetpp_nlmeans_u8(unetpp_engine* e, const uint8_t* dev_src, int batch, int h, int w, int channels_in, int channels_out,
                      const uint8_t* dev_decisions, const uint16_t* dev_weights_u16, int n_weights, uint8_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_src && dev_weights_u16 && dev_out);
  if ((channels_in != 1 && channels_in != 3) || (channels_out != 1 && channels_out != 3))
    return fail(e, UNETPP_E_INVALID, "channels %d -> %d: each 1 or 3", channels_in, channels_out);
  if (dev_decisions && channels_in != channels_out)
    return fail(e, UNETPP_E_INVALID, "dev_decisions copies frames through: channels_out must equal channels_in");
  if (!shape_ok(batch, h, w, NLM_SHAPE))
    return fail(e, UNETPP_E_UNSUPPORTED, "shape %dx%dx%d outside %d <= h, w <= 65535, h * w <= 2^30", batch, h, w, NLM_MIN_SIDE);
  if (n_weights < 1 || n_weights > NLM_MAX_WEIGHTS)
    return fail(e, UNETPP_E_UNSUPPORTED, "n_weights %d: the non-zero prefix of the weight table must have 1..%d entries", n_weights, NLM_MAX_WEIGHTS);
  if ((uintptr_t)dev_weights_u16 % 2) return fail(e, UNETPP_E_INVALID, "dev_weights_u16 must be 2-byte aligned");
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_src, n * channels_in, dev_out, n * channels_out))
    return fail(e, UNETPP_E_INVALID, "dev_out aliases dev_src: workgroups read halo pixels their neighbours write");
  ENTER_DEVICE(e);
  const int vec = w % 4 == 0 && (uintptr_t)dev_out % 4 == 0;
  hipLaunchKernelGGL(nlmeans_kernel, tile_grid(w, h, NLM_TILE_W, NLM_TILE_H, batch), dim3(NLM_THREADS), 0, (hipStream_t)stream, dev_src, h, w,
                     channels_in, channels_out, dev_decisions, dev_weights_u16, n_weights, vec, dev_out);
  return launched(e);
}

// ---- segmentation evaluation: joint histogram of two masks, mask disagreement (evaluation.h) --------------------------------
int unetpp_evaluation_layout(int* span_pixels) {
  if (!span_pixels) return fail(nullptr, UNETPP_E_INVALID, "null argument");
  *span_pixels = EV_SPAN;
  return UNETPP_OK;
}

// any h, w >= 1 below `pixel_limit` pixels; batch is a grid dimension
static int eval_shape_check(unetpp_engine* e, int batch, int h, int w, uint64_t pixel_limit) {
  if (batch < 1 || batch > MAX_DIM || h < 1 || w < 1 || (uint64_t)h * (uint64_t)w >= pixel_limit)
    return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d: 1 <= batch <= 65535, h, w >= 1, h * w < 2^%d", batch, h, w, pixel_limit >> 32 ? 32 : 31);
  return UNETPP_OK;
}

// 16-byte loads need the two masks to sit at the same offset from a 16-byte boundary; frames then share their heads
static int eval_vec(const void* p, const void* q) { return (((uintptr_t)p ^ (uintptr_t)q) & 15u) == 0; }

static dim3 eval_grid(uint64_t hw, int batch) { return dim3((unsigned)((hw + 15 + EV_SPAN - 1) / EV_SPAN), (unsigned)batch); }

int unetpp_confusion_u8(unetpp_engine* e, const uint8_t* dev_pred, const uint8_t* dev_target, int batch, int h, int w, int num_classes,
                        int ignore_value, uint32_t* dev_counts, uint32_t* dev_outside, uint64_t* dev_total, void* stream) {
  REQUIRE_ARGS(e, dev_pred && dev_target && dev_counts && dev_outside);
  if (int rc = eval_shape_check(e, batch, h, w, 1ull << 32)) return rc;
  if (num_classes < 2 || num_classes > EV_MAX_CLASSES) return fail(e, UNETPP_E_INVALID, "num_classes %d: 2..%d", num_classes, EV_MAX_CLASSES);
  if (ignore_value < -1 || ignore_value > 255) return fail(e, UNETPP_E_INVALID, "ignore_value %d: 0..255, or -1 for none", ignore_value);
  if ((uintptr_t)dev_total % 8) return fail(e, UNETPP_E_INVALID, "dev_total must be 8-byte aligned");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const uint64_t hw = (uint64_t)h * (uint64_t)w;
  HIP_TRY(e, hipMemsetAsync(dev_counts, 0, (size_t)batch * num_classes * num_classes * sizeof(uint32_t), s));
  HIP_TRY(e, hipMemsetAsync(dev_outside, 0, (size_t)batch * 2 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(confusion_kernel, eval_grid(hw, batch), dim3(EV_THREADS), 0, s, dev_pred, dev_target, (unsigned)hw, num_classes, ignore_value,
                     eval_vec(dev_pred, dev_target), (unsigned*)dev_counts, (unsigned*)dev_outside, (unsigned long long*)dev_total);
  return launched(e);
}

int unetpp_mask_disagreement(unetpp_engine* e, const uint8_t* dev_a, const uint8_t* dev_b, int batch, int h, int w, const float* dev_logits,
                             int num_classes, uint32_t* dev_n_diff, int32_t* dev_first, float* dev_max_margin, uint32_t* dev_n_nan, void* stream) {
  REQUIRE_ARGS(e, dev_a && dev_b && dev_n_diff && dev_first && (!dev_logits || (dev_max_margin && dev_n_nan)));
  if (int rc = eval_shape_check(e, batch, h, w, 1ull << 31)) return rc;
  if (dev_logits && (num_classes < 1 || num_classes > 256)) return fail(e, UNETPP_E_INVALID, "num_classes %d: 1..256 with logits", num_classes);
  if ((uintptr_t)dev_logits % 4) return fail(e, UNETPP_E_INVALID, "dev_logits must be 4-byte aligned");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const uint64_t hw = (uint64_t)h * (uint64_t)w;
  HIP_TRY(e, hipMemsetAsync(dev_n_diff, 0, (size_t)batch * sizeof(uint32_t), s));
  HIP_TRY(e, hipMemsetAsync(dev_first, 0xff, (size_t)batch * sizeof(int32_t), s));
  if (dev_max_margin) HIP_TRY(e, hipMemsetAsync(dev_max_margin, 0, (size_t)batch * sizeof(float), s));
  if (dev_n_nan) HIP_TRY(e, hipMemsetAsync(dev_n_nan, 0, (size_t)batch * sizeof(uint32_t), s));
  hipLaunchKernelGGL(mask_disagreement_kernel, eval_grid(hw, batch), dim3(EV_THREADS), 0, s, dev_a, dev_b, (unsigned)hw, dev_logits, num_classes,
                     eval_vec(dev_a, dev_b), (unsigned*)dev_n_diff, (unsigned*)dev_first, (unsigned*)dev_max_margin, (unsigned*)dev_n_nan);
  return launched(e);
}

// ---- rules on a float32 probability plane: levels, the one-pass threshold scan, mean probability per component (probmap.h) ----
int unetpp_probmap_layout(int* span_pixels) {
  if (!span_pixels) return fail(nullptr, UNETPP_E_INVALID, "null argument");
  *span_pixels = PM_SPAN;
  return UNETPP_OK;
}

// channel `channel` of float32 [B,h,w,pixel_stride]; the array holds fewer than 2^40 floats, far above any device's memory
static int plane_check(unetpp_engine* e, const float* dev_prob, int pixel_stride, int channel) {
  if ((uintptr_t)dev_prob % 4) return fail(e, UNETPP_E_INVALID, "dev_prob must be 4-byte aligned");
  if (pixel_stride < 1 || pixel_stride > 256 || channel < 0 || channel >= pixel_stride)
    return fail(e, UNETPP_E_INVALID, "pixel_stride %d, channel %d: 1 <= pixel_stride <= 256, 0 <= channel < pixel_stride", pixel_stride, channel);
  return UNETPP_OK;
}

static dim3 plane_grid(uint64_t hw, int batch) { return dim3((unsigned)((hw + PM_SPAN - 1) / PM_SPAN), (unsigned)batch); }

int unetpp_prob_levels_f32(unetpp_engine* e, const float* dev_prob, int pixel_stride, int channel, int batch, int h, int w, float t_low,
                           float t_high, uint8_t* dev_codes, void* stream) {
  REQUIRE_ARGS(e, dev_prob && dev_codes);
  if (int rc = eval_shape_check(e, batch, h, w, 1ull << 32)) return rc;
  if (int rc = plane_check(e, dev_prob, pixel_stride, channel)) return rc;
  if (!(t_low <= t_high)) return fail(e, UNETPP_E_INVALID, "thresholds %g, %g: need t_low <= t_high, neither NaN", (double)t_low, (double)t_high);
  ENTER_DEVICE(e);
  const uint64_t hw = (uint64_t)h * (uint64_t)w;
  hipLaunchKernelGGL(prob_levels_kernel, plane_grid(hw, batch), dim3(PM_THREADS), 0, (hipStream_t)stream, dev_prob, pixel_stride, channel,
                     (unsigned)hw, t_low, t_high, dev_codes);
  return launched(e);
}

int unetpp_prob_threshold_hist_f32(unetpp_engine* e, const float* dev_prob, int pixel_stride, int channel, const uint8_t* dev_target, int batch,
                                   int h, int w, const float* thresholds, int n_thresholds, int target_class, int ignore_value,
                                   uint32_t* dev_counts, uint32_t* dev_outside, uint64_t* dev_total, void* stream) {
  REQUIRE_ARGS(e, dev_prob && dev_target && thresholds && dev_counts && dev_outside);
  if (int rc = eval_shape_check(e, batch, h, w, 1ull << 32)) return rc;
  if (int rc = plane_check(e, dev_prob, pixel_stride, channel)) return rc;
  if (n_thresholds < 1 || n_thresholds > PM_MAX_THRESHOLDS) return fail(e, UNETPP_E_INVALID, "n_thresholds %d: 1..%d", n_thresholds, PM_MAX_THRESHOLDS);
  PmThresholds th{};
  for (int j = 0; j < n_thresholds; ++j) {
    if (std::isnan(thresholds[j]) || (j && !(thresholds[j - 1] < thresholds[j])))
      return fail(e, UNETPP_E_INVALID, "thresholds must be strictly ascending numbers (entry %d)", j);
    th.t[j] = thresholds[j];
  }
  if (target_class < -1 || target_class > 255) return fail(e, UNETPP_E_INVALID, "target_class %d: 0..255, or -1 for non-zero", target_class);
  if (ignore_value < -1 || ignore_value > 255) return fail(e, UNETPP_E_INVALID, "ignore_value %d: 0..255, or -1 for none", ignore_value);
  if ((uintptr_t)dev_total % 8) return fail(e, UNETPP_E_INVALID, "dev_total must be 8-byte aligned");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const uint64_t hw = (uint64_t)h * (uint64_t)w;
  HIP_TRY(e, hipMemsetAsync(dev_counts, 0, (size_t)batch * 2 * (n_thresholds + 1) * sizeof(uint32_t), s));
  HIP_TRY(e, hipMemsetAsync(dev_outside, 0, (size_t)batch * sizeof(uint32_t), s));
  hipLaunchKernelGGL(prob_threshold_hist_kernel, plane_grid(hw, batch), dim3(PM_THREADS), 0, s, dev_prob, pixel_stride, channel, dev_target,
                     (unsigned)hw, th, n_thresholds, target_class, ignore_value, (unsigned*)dev_counts, (unsigned*)dev_outside,
                     (unsigned long long*)dev_total);
  return launched(e);
}

int unetpp_components_prob_sum_f32(unetpp_engine* e, const int32_t* dev_labels, const float* dev_prob, int pixel_stride, int channel, int batch,
                                   int h, int w, int capacity, uint64_t* dev_sums, void* stream) {
  REQUIRE_ARGS(e, dev_labels && dev_prob && dev_sums);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  if (capacity < 2) return fail(e, UNETPP_E_INVALID, "capacity %d: at least 2 rows (background + one component)", capacity);
  if (int rc = plane_check(e, dev_prob, pixel_stride, channel)) return rc;
  if ((uintptr_t)dev_labels % 4 || (uintptr_t)dev_sums % 8) return fail(e, UNETPP_E_INVALID, "dev_labels must be 4-byte, dev_sums 8-byte aligned");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  HIP_TRY(e, hipMemsetAsync(dev_sums, 0, (size_t)batch * ((size_t)capacity + 1) * sizeof(uint64_t), s));
  hipLaunchKernelGGL(components_prob_sum_kernel, plane_grid((uint64_t)hw, batch), dim3(PM_THREADS), 0, s, (const int*)dev_labels, dev_prob,
                     pixel_stride, channel, hw, capacity, (unsigned long long*)dev_sums);
  return launched(e);
}

int unetpp_components_filter_mean(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats,
                                  const uint64_t* dev_prob_sums, int batch, int h, int w, int capacity, int64_t min_area, uint64_t thr_q,
                                  uint8_t out_value, uint8_t* dev_out, void* dev_workspace, void* stream) {
  REQUIRE_ARGS(e, dev_labels && dev_num && dev_stats && dev_prob_sums && dev_out && dev_workspace);
  if (capacity < 2) return fail(e, UNETPP_E_INVALID, "capacity %d: at least 2 rows (background + one component)", capacity);
  CcWorkspace ws;
  if (!cc_layout(batch, h, w, capacity, &ws)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  uint8_t* keep = (uint8_t*)dev_workspace + ws.keep;
  hipLaunchKernelGGL(cc_select_mean_kernel, dim3((unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_num, (const int*)dev_stats,
                     (const unsigned long long*)dev_prob_sums, capacity, (long long)min_area, (unsigned long long)thr_q, keep);
  hipLaunchKernelGGL(cc_apply_kernel, dim3((unsigned)ws.nchunk, (unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_labels,
                     (const uint8_t*)keep, hw, capacity, vec16(hw, dev_labels, dev_out), (unsigned)out_value, dev_out);
  return launched(e);
}

// ---- binary morphology programs (morphology.h) ------------------------------------------------------------------
struct MorphPlan {
  MorphArgs args;
  dim3 grid;
  size_t lds_bytes = 0;
};

// Checks the elements and turns them into the kernels' sorted row runs; ax / ay receive the resolved anchors.
static int morph_elements(unetpp_engine* e, const unetpp_morph_element* elements, int n_elements, MorphElem* out, int* ax, int* ay) {
  for (int k = 0; k < n_elements; ++k) {
    const unetpp_morph_element& el = elements[k];
    if (el.kw < 1 || el.kh < 1 || !el.host_data) return fail(e, UNETPP_E_INVALID, "element %d: bad size %dx%d or NULL data", k, el.kw, el.kh);
    if (el.kw > MORPH_MAX_K || el.kh > MORPH_MAX_K)
      return fail(e, UNETPP_E_UNSUPPORTED, "element %d is %dx%d: too large, at most %dx%d", k, el.kw, el.kh, MORPH_MAX_K, MORPH_MAX_K);
    ax[k] = el.ax < 0 ? el.kw / 2 : el.ax;
    ay[k] = el.ay < 0 ? el.kh / 2 : el.ay;
    if (ax[k] >= el.kw || ay[k] >= el.kh) return fail(e, UNETPP_E_INVALID, "element %d: anchor (%d,%d) outside %dx%d", k, el.ax, el.ay, el.kw, el.kh);
    MorphElem& E = out[k];
    for (int i = 0; i < el.kh; ++i) {
      const uint8_t* r = el.host_data + (size_t)i * el.kw;
      int first = -1, last = -1, count = 0;
      for (int j = 0; j < el.kw; ++j)
        if (r[j]) { if (first < 0) first = j; last = j; ++count; }
      if (!count) continue;
      if (count != last - first + 1)
        return fail(e, UNETPP_E_UNSUPPORTED, "element %d is not row-convex: the non-zeros of row %d are not one run", k, i);
      E.row[E.nrows++] = MorphRow{(signed char)(i - ay[k]), (signed char)(first - ax[k]), (signed char)(last - ax[k]), 0};
    }
    if (!E.nrows) return fail(e, UNETPP_E_INVALID, "element %d is empty (all zero)", k);
    std::sort(E.row, E.row + E.nrows, [](const MorphRow& p, const MorphRow& q) {
      return std::make_tuple(p.lo, p.hi, p.dy) < std::make_tuple(q.lo, q.hi, q.dy);
    });
  }
  return UNETPP_OK;
}

// Lays the tiles of a bit-plane program out for planes of at most plane_words 64-bit words: bands of full-width rows while a
// row and its halo fit, else tiles with a halo on all four sides.  *band_out stays 0 when nothing fits.
static void morph_tiles(int plane_words, int batch, int h, int wpr, int halo, int left, int right, int* band_out, int* cw, int* hl, int* tw) {
  *band_out = 0;
  int band_max;
  if (wpr * (halo + 1) <= plane_words) {            // bands of full-width rows: no horizontal halo
    *cw = wpr; *hl = 0; *tw = wpr;
    band_max = plane_words / wpr - halo;
    // enough workgroups to fill the device before the bands grow: at most as much halo as core, never below 16 rows
    int band = std::min(std::max(halo, 16), band_max);
    while ((long long)batch * ((h + band - 1) / band) > 2048 && band * 2 <= band_max) band *= 2;
    band = std::min(band, h);
    // one thread per word and pass: grow the band until the window's words fill whole passes of the workgroup
    int unit = MORPH_THREADS;
    for (int a = MORPH_THREADS, b = wpr; b;) { const int r = a % b; a = b; b = r; unit = MORPH_THREADS / a; }
    const int rows_up = (band + halo + unit - 1) / unit * unit;
    if (rows_up - halo <= std::min(band_max, h)) band = rows_up - halo;
    *band_out = band;
  } else {                                                  // tiles with a halo on all four sides: the best core share
    const int wl = (left + 63) / 64, wr = (right + 63) / 64;
    double best = -1.0;
    *cw = 0;
    for (int c = 1; c <= std::min(wpr, 64); ++c) {
      const int bm = std::min(plane_words / (c + wl + wr) - halo, h);
      if (bm < 1) break;
      const double share = (double)c * bm / ((double)(c + wl + wr) * (bm + halo));
      if (share > best) { best = share; *cw = c; *band_out = bm; }
    }
    *hl = wl; *tw = *cw + wl + wr;
  }
}

// Checks a program and lays its tiles out.  Everything the kernel indexes with is validated here.
static int morph_plan(unetpp_engine* e, int batch, int h, int w, const unetpp_morph_element* elements, int n_elements,
                      const unetpp_morph_step* steps, int n_steps, int result_plane, MorphPlan* plan) {
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  if (n_elements < 0 || n_elements > MORPH_MAX_ELEMENTS || (n_elements > 0 && !elements))
    return fail(e, UNETPP_E_INVALID, "n_elements %d not in [0,%d]", n_elements, MORPH_MAX_ELEMENTS);
  if (n_steps < 0 || n_steps > MORPH_MAX_STEPS || (n_steps > 0 && !steps))
    return fail(e, UNETPP_E_INVALID, "n_steps %d not in [0,%d]", n_steps, MORPH_MAX_STEPS);
  MorphArgs& A = plan->args;
  std::memset(&A, 0, sizeof A);
  int ax[MORPH_MAX_ELEMENTS], ay[MORPH_MAX_ELEMENTS];
  if (const int rc = morph_elements(e, elements, n_elements, A.elem, ax, ay)) return rc;
  bool written[MORPH_USER_PLANES] = {true, true, false, false};     // plane 1 is all zero without a second mask
  auto plane_ok = [](int p) { return p >= 0 && p < MORPH_USER_PLANES; };
  int up = 0, down = 0, left = 0, right = 0;
  for (int s = 0; s < n_steps; ++s) {
    const unetpp_morph_step& st = steps[s];
    if (st.op < UNETPP_MORPH_DILATE || st.op > UNETPP_MORPH_COPY) return fail(e, UNETPP_E_INVALID, "step %d: unknown op %d", s, st.op);
    const bool morph = st.op == UNETPP_MORPH_DILATE || st.op == UNETPP_MORPH_ERODE;
    const bool binary = st.op == UNETPP_MORPH_AND || st.op == UNETPP_MORPH_ANDNOT || st.op == UNETPP_MORPH_OR;
    if (!plane_ok(st.dst) || !plane_ok(st.a) || (binary && !plane_ok(st.b)))
      return fail(e, UNETPP_E_INVALID, "step %d: plane index out of range [0,%d)", s, MORPH_USER_PLANES);
    if (!written[st.a] || (binary && !written[st.b]))
      return fail(e, UNETPP_E_INVALID, "step %d reads scratch plane %d before any step has written it", s, !written[st.a] ? st.a : st.b);
    MorphStep& D = A.step[s];
    D.op = st.op; D.dst = st.dst; D.a = st.a; D.b = binary ? st.b : st.a; D.elem = 0; D.iters = 1;
    if (morph) {
      if (st.element < 0 || st.element >= n_elements) return fail(e, UNETPP_E_INVALID, "step %d: element index %d not in [0,%d)", s, st.element, n_elements);
      if (st.iterations < 1) return fail(e, UNETPP_E_INVALID, "step %d: iterations must be at least 1, got %d", s, st.iterations);
      if (st.iterations > MORPH_MAX_REACH) return fail(e, UNETPP_E_UNSUPPORTED, "step %d: iterations %d beyond %d", s, st.iterations, MORPH_MAX_REACH);
      D.elem = st.element; D.iters = st.iterations;
      const unetpp_morph_element& el = elements[st.element];
      up += st.iterations * ay[st.element]; down += st.iterations * (el.kh - 1 - ay[st.element]);
      left += st.iterations * ax[st.element]; right += st.iterations * (el.kw - 1 - ax[st.element]);
      if (up + down > MORPH_MAX_REACH || left + right > MORPH_MAX_REACH)
        return fail(e, UNETPP_E_UNSUPPORTED, "the program's reach (sum of iterations * (k - 1) over its dilates and erodes) exceeds %d pixels "
                    "(vertical %d, horizontal %d)", MORPH_MAX_REACH, up + down, left + right);
    }
    written[st.dst] = true;
  }
  if (!plane_ok(result_plane) || !written[result_plane])
    return fail(e, UNETPP_E_INVALID, "result_plane %d is out of range or never written", result_plane);
  A.n_steps = n_steps; A.result = result_plane;
  A.H = h; A.W = w; A.wpr = (w + 63) / 64;
  const int halo = up + down;
  morph_tiles(MORPH_PLANE_WORDS, batch, h, A.wpr, halo, left, right, &A.band, &A.cw, &A.hl, &A.tw);
  A.up = up; A.rows = A.band + halo;
  plan->grid = tile_grid(A.wpr, h, A.cw, A.band, batch);
  plan->lds_bytes = (size_t)MORPH_PLANES * A.rows * A.tw * sizeof(unsigned long long);
  if (A.band < 1 || A.rows * A.tw > MORPH_PLANE_WORDS) return fail(e, UNETPP_E_STATE, "internal: morphology tile layout");
  return UNETPP_OK;
}

int unetpp_morphology_layout(int batch, int h, int w, const unetpp_morph_element* elements, int n_elements,
                             const unetpp_morph_step* steps, int n_steps, int* band_rows, int* tile_cols) {
  if (!band_rows || !tile_cols) return fail(nullptr, UNETPP_E_INVALID, "null argument");
  MorphPlan plan;
  if (const int rc = morph_plan(nullptr, batch, h, w, elements, n_elements, steps, n_steps, n_steps > 0 ? steps[n_steps - 1].dst : 0, &plan)) return rc;
  *band_rows = plan.args.band;
  *tile_cols = plan.args.cw * 64;
  return UNETPP_OK;
}

int unetpp_morphology(unetpp_engine* e, const uint8_t* dev_mask0, int match0, const uint8_t* dev_mask1, int match1, int batch,
                      int h, int w, const unetpp_morph_element* elements, int n_elements, const unetpp_morph_step* steps,
                      int n_steps, int result_plane, uint8_t out_value, uint8_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_mask0 && dev_out);
  if (match0 > 255 || match1 > 255) return fail(e, UNETPP_E_INVALID, "match_class %d out of range", match0 > 255 ? match0 : match1);
  MorphPlan plan;
  if (const int rc = morph_plan(e, batch, h, w, elements, n_elements, steps, n_steps, result_plane, &plan)) return rc;
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_mask0, n, dev_out, n) || (dev_mask1 && overlaps(dev_mask1, n, dev_out, n)))
    return fail(e, UNETPP_E_INVALID, "dev_out aliases an input mask: every workgroup reads the halo rows its neighbours write");
  ENTER_DEVICE(e);
  MorphArgs& A = plan.args;
  A.match0 = match0; A.match1 = match1; A.out_value = out_value;
  A.vec0 = vec16(w, dev_mask0); A.vec1 = vec16(w, dev_mask1); A.vec_out = vec16(w, dev_out);
  hipLaunchKernelGGL(morph_program_kernel, plan.grid, dim3(MORPH_THREADS), plan.lds_bytes, (hipStream_t)stream, dev_mask0, dev_mask1,
                     dev_out, A);
  return launched(e);
}

// ---- frame glue: cv2.resize either side of the model ----------------------------------
// resizeGeneric_'s INTER_LINEAR index/coefficient tables (OpenCV imgproc/src/resize.cpp): double index math, float
// fraction.  Entry = {s0, s1, a0, a1} with a = saturate_cast<short>(c * 2048), round-half-even, for the uint8 resize; with
// as_f32 the same indices and the bits of the float coefficients 1 - fx and fx of the float32 resize (tiling.h).
static void linear_table(int n_src, int n_dst, bool as_f32, std::vector<int>& t) {
#pragma clang fp contract(off)
  t.resize((size_t)n_dst * 4);
  const double inv_scale = (double)n_dst / (double)n_src;
  const double scale = 1.0 / inv_scale;
  for (int d = 0; d < n_dst; ++d) {
    float fx = (float)((d + 0.5) * scale - 0.5);
    int s0 = (int)floorf(fx);
    fx -= (float)s0;
    if (s0 < 0) { fx = 0.f; s0 = 0; }
    if (s0 >= n_src - 1) { fx = 0.f; s0 = n_src - 1; }
    const float c0 = 1.f - fx;
    int a0, a1;
    if (as_f32) {
      std::memcpy(&a0, &c0, sizeof a0);
      std::memcpy(&a1, &fx, sizeof a1);
    } else {
      a0 = (int)std::min(32767L, std::max(-32768L, lrintf(c0 * 2048.f)));
      a1 = (int)std::min(32767L, std::max(-32768L, lrintf(fx * 2048.f)));
    }
    t[4 * d + 0] = s0; t[4 * d + 1] = std::min(s0 + 1, n_src - 1); t[4 * d + 2] = a0; t[4 * d + 3] = a1;
  }
}
// resizeNN's index table: min(floor(d * (1 / (n_dst / n_src))), n_src - 1) in double.
static void nearest_table(int n_src, int n_dst, std::vector<int>& t) {
#pragma clang fp contract(off)
  t.resize((size_t)n_dst);
  const double inv = (double)n_dst / (double)n_src;
  const double ifx = 1.0 / inv;
  for (int d = 0; d < n_dst; ++d) t[d] = std::min((int)floor(d * ifx), n_src - 1);
}
// Device copy of a table, built on first use (that first call synchronises: a blocking hipMemcpy).
static int resize_table(unetpp_engine* e, int kind, int n_src, int n_dst, void** out) {
  auto& tabs = unetpp_common(e)->resize_tabs;
  auto key = std::make_tuple(kind, n_src, n_dst);
  auto it = tabs.find(key);
  if (it == tabs.end()) {
    std::vector<int> t;
    if (kind == 1) nearest_table(n_src, n_dst, t); else linear_table(n_src, n_dst, kind == 2, t);
    void* d = nullptr;
    HIP_TRY(e, hipMalloc(&d, t.size() * sizeof(int)));
    hipError_t r = hipMemcpy(d, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice);
    if (r != hipSuccess) { (void)hipFree(d); return fail(e, UNETPP_E_HIP, "hipMemcpy(resize table): %s", hipGetErrorString(r)); }
    it = tabs.emplace(key, d).first;
  }
  *out = it->second;
  return UNETPP_OK;
}

int unetpp_resize_linear_u8(unetpp_engine* e, const uint8_t* dev_src, int batch, int src_h, int src_w, int channels,
                            uint8_t* dev_dst, int dst_h, int dst_w, void* stream) {
  REQUIRE_ARGS(e, dev_src && dev_dst);
  if (batch < 1 || src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || channels < 1 || channels > 4)
    return fail(e, UNETPP_E_INVALID, "bad resize shape %dx%dx%dx%d -> %dx%d", batch, src_h, src_w, channels, dst_h, dst_w);
  if (batch > 65535 || dst_h > 65535 || (size_t)src_h * src_w * channels > 0x7fffffffULL)
    return fail(e, UNETPP_E_INVALID, "resize shape too large");
  ENTER_DEVICE(e);
  void *xt = nullptr, *yt = nullptr;
  if (const int rc = resize_table(e, 0, src_w, dst_w, &xt)) return rc;
  if (const int rc = resize_table(e, 0, src_h, dst_h, &yt)) return rc;
  const unsigned gx = (unsigned)((dst_w * channels + 1023) / 1024);
  hipLaunchKernelGGL(resize_linear_u8_kernel, dim3(gx, (unsigned)dst_h, (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                     dev_src, src_h, src_w, channels, dev_dst, dst_h, dst_w, (const int4*)xt, (const int4*)yt);
  return launched(e);
}

int unetpp_resize_nearest_roi_u8(unetpp_engine* e, const uint8_t* dev_src, int batch, int src_h, int src_w, int match_class,
                                 uint8_t* dev_dst, int dst_h, int dst_w, int x1, int y1, int x2, int y2, void* stream) {
  REQUIRE_ARGS(e, dev_src && dev_dst);
  if (batch < 1 || src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1)
    return fail(e, UNETPP_E_INVALID, "bad resize shape %dx%dx%d -> %dx%d", batch, src_h, src_w, dst_h, dst_w);
  if (batch > 65535 || dst_h > 65535) return fail(e, UNETPP_E_INVALID, "resize shape too large");
  if (x1 < 0 || y1 < 0 || x2 < 0 || y2 < 0) return fail(e, UNETPP_E_INVALID, "negative ROI bound (%d, %d, %d, %d)", x1, y1, x2, y2);
  if (match_class > 255) return fail(e, UNETPP_E_INVALID, "match_class %d out of range", match_class);
  ENTER_DEVICE(e);
  void *xo = nullptr, *yo = nullptr;
  if (const int rc = resize_table(e, 1, src_w, dst_w, &xo)) return rc;
  if (const int rc = resize_table(e, 1, src_h, dst_h, &yo)) return rc;
  const unsigned gx = (unsigned)((dst_w + 1023) / 1024);
  hipLaunchKernelGGL(resize_nearest_roi_u8_kernel, dim3(gx, (unsigned)dst_h, (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                     dev_src, src_h, src_w, dev_dst, dst_h, dst_w, (const int*)xo, (const int*)yo, match_class, x1, y1, x2, y2);
  return launched(e);
}

// ---- sliding-window inference: gather tiles, gate, blend (tiling.h) ------------------------------------------
// Checks a separable plan against the frame and copies it.  Everything the kernels index with is validated here.
static int tile_plan_check(unetpp_engine* e, int h, int w, const int32_t* oy, int n_y, const int32_t* ox, int n_x, int patch_size,
                           bool reflect, TilePlan* plan) {
  if (!oy || !ox) return fail(e, UNETPP_E_INVALID, "null argument");
  if (!shape_ok(1, h, w, ROWS_SHAPE) || patch_size < 1 || patch_size > 65535)
    return fail(e, UNETPP_E_INVALID, "bad shape %dx%d, patch_size %d", h, w, patch_size);
  if (n_y < 1 || n_x < 1) return fail(e, UNETPP_E_INVALID, "empty plan %dx%d", n_y, n_x);
  if (n_y > TILE_MAX_AXIS || n_x > TILE_MAX_AXIS)
    return fail(e, UNETPP_E_UNSUPPORTED, "plan of %dx%d patches: at most %d per axis", n_y, n_x, TILE_MAX_AXIS);
  plan->ny = n_y; plan->nx = n_x;
  for (int a = 0; a < 2; ++a) {
    const int n = a ? w : h, cnt = a ? n_x : n_y;
    const int32_t* o = a ? ox : oy;
    for (int i = 0; i < cnt; ++i) {
      if (o[i] < 0 || o[i] >= n) return fail(e, UNETPP_E_INVALID, "origin %d outside an axis of %d", o[i], n);
      if (reflect && o[i] + patch_size - 1 > 2 * (n - 1))
        return fail(e, UNETPP_E_UNSUPPORTED, "patch of %d at %d on an axis of %d: reflect padding of the axis length or more", patch_size, o[i], n);
      (a ? plan->ox : plan->oy)[i] = o[i];
    }
  }
  return UNETPP_OK;
}

int unetpp_tile_gather_u8(unetpp_engine* e, const uint8_t* dev_frames, int batch, int h, int w, const int32_t* origins_y, int n_y,
                          const int32_t* origins_x, int n_x, int patch_size, int t, int channel_order, uint8_t* dev_patches,
                          void* stream) {
  REQUIRE_ARGS(e, dev_frames && dev_patches);
  if (batch < 1 || t < 4 || t % 4 || t > 16384) return fail(e, UNETPP_E_INVALID, "bad batch %d or patch size %d (a multiple of 4)", batch, t);
  if (channel_order != UNETPP_TILE_BGR && channel_order != UNETPP_TILE_RGB) return fail(e, UNETPP_E_INVALID, "channel_order %d", channel_order);
  TilePlan plan;
  if (const int rc = tile_plan_check(e, h, w, origins_y, n_y, origins_x, n_x, patch_size, true, &plan)) return rc;
  if ((long long)batch * n_y * n_x > 65535) return fail(e, UNETPP_E_INVALID, "%d x %d x %d patches: at most 65535 per call", batch, n_y, n_x);
  if ((size_t)h * w * 3 > 0x7fffffffULL) return fail(e, UNETPP_E_INVALID, "frame too large");
  ENTER_DEVICE(e);
  void* tab = nullptr;
  if (const int rc = resize_table(e, 0, patch_size, t, &tab)) return rc;
  hipLaunchKernelGGL(tile_gather_u8_kernel, dim3((unsigned)((t * 3 + 1023) / 1024), (unsigned)t, (unsigned)(batch * n_y * n_x)),
                     dim3(TILE_THREADS), 0, (hipStream_t)stream, dev_frames, h, w, plan, t, (int)(channel_order == UNETPP_TILE_RGB),
                     (const int4*)tab, (const int4*)tab, dev_patches);
  return launched(e);
}

int unetpp_tile_gate_f32(unetpp_engine* e, const float* dev_maps, int n, int classes, int t, int gate_class, float gate_thr,
                         float* dev_scores, uint8_t* dev_include, void* stream) {
  REQUIRE_ARGS(e, dev_maps && dev_scores && dev_include);
  if (n < 1 || classes < 1 || t < 2 || t % 2 || t > 16384) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%dx%d", n, classes, t, t);
  if (gate_class < 0 || gate_class >= classes) return fail(e, UNETPP_E_INVALID, "gate_class %d not in [0,%d)", gate_class, classes);
  if ((uintptr_t)dev_maps % 16) return fail(e, UNETPP_E_INVALID, "dev_maps must be 16-byte aligned");
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(tile_gate_f32_kernel, dim3((unsigned)n), dim3(TILE_THREADS), 0, (hipStream_t)stream, dev_maps, classes, t, gate_class,
                     gate_thr, dev_scores, dev_include);
  return launched(e);
}

int unetpp_tile_blend_f32(unetpp_engine* e, const float* dev_maps, int batch, int classes, int t, const int32_t* origins_y, int n_y,
                          const int32_t* origins_x, int n_x, int patch_size, const uint8_t* dev_include, int h, int w,
                          uint8_t* dev_mask, float* dev_output, void* stream) {
  REQUIRE_ARGS(e, dev_maps && dev_mask);
  if (batch < 1 || batch > 65535 || classes < 1 || t < 1 || t > 16384) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%dx%d", batch, classes, t, t);
  if (classes > TILE_MAX_CLASSES) return fail(e, UNETPP_E_UNSUPPORTED, "%d classes: at most %d", classes, TILE_MAX_CLASSES);
  TilePlan plan;
  if (const int rc = tile_plan_check(e, h, w, origins_y, n_y, origins_x, n_x, patch_size, false, &plan)) return rc;
  ENTER_DEVICE(e);
  void* tab = nullptr;
  if (const int rc = resize_table(e, 2, t, patch_size, &tab)) return rc;
  const dim3 grid = tile_grid(w, h, TILE_WAVE, TILE_BLEND_ROWS, batch);
#define TILE_BLEND_CASE(C)                                                                                                       \
  case C:                                                                                                                        \
    hipLaunchKernelGGL(tile_blend_f32_kernel<C>, grid, dim3(TILE_THREADS), 0, (hipStream_t)stream, dev_maps, plan, patch_size, t, \
                       (const int4*)tab, (const int4*)tab, dev_include, h, w, dev_mask, dev_output);                             \
    break
  switch (classes) {
    TILE_BLEND_CASE(1); TILE_BLEND_CASE(2); TILE_BLEND_CASE(3); TILE_BLEND_CASE(4);
    TILE_BLEND_CASE(5); TILE_BLEND_CASE(6); TILE_BLEND_CASE(7); TILE_BLEND_CASE(8);
  }
#undef TILE_BLEND_CASE
  return launched(e);
}

// ---- the 6- and 7-class video loops: quality gate, class bits, class merge with its table, overlay (multiclass.h) -----------
size_t unetpp_quality_gate_workspace_bytes(int batch) {
  return batch >= 1 && batch <= MAX_DIM ? align_up((size_t)batch * QG_SUMS * sizeof(uint64_t), 256) : 0;
}

int unetpp_quality_gate_u8(unetpp_engine* e, const uint8_t* dev_bgr, const uint8_t* dev_prev_gray, int batch, int h, int w, int enable,
                           double blur_th, double flat_th, double motion_th, double glitch_flat_th, uint8_t* dev_gray, uint8_t* dev_is_bad,
                           uint8_t* dev_reason, double* dev_lap_var, double* dev_gray_std, double* dev_mad, void* dev_workspace, void* stream) {
  REQUIRE_ARGS(e, dev_bgr && dev_gray && dev_is_bad && dev_reason && dev_lap_var && dev_gray_std && dev_mad && dev_workspace);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  if (blur_th != blur_th || flat_th != flat_th || motion_th != motion_th || glitch_flat_th != glitch_flat_th)
    return fail(e, UNETPP_E_INVALID, "a threshold is NaN");
  if ((uintptr_t)dev_workspace % 8 || (uintptr_t)dev_lap_var % 8 || (uintptr_t)dev_gray_std % 8 || (uintptr_t)dev_mad % 8)
    return fail(e, UNETPP_E_INVALID, "dev_workspace and the float64 outputs must be 8-byte aligned");
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_bgr, 3 * n, dev_gray, n) || (dev_prev_gray && overlaps(dev_prev_gray, (size_t)h * w, dev_gray, n)))
    return fail(e, UNETPP_E_INVALID, "dev_gray aliases an input: workgroups read pixels that others write");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(e, hipMemsetAsync(dev_workspace, 0, (size_t)batch * QG_SUMS * sizeof(uint64_t), s));
  hipLaunchKernelGGL(quality_sums_kernel, tile_grid(w, h, QG_TW, QG_TH, batch), dim3(MC_THREADS), 0, s, dev_bgr, dev_prev_gray, h, w,
                     (int)(w % 8 == 0 && (uintptr_t)dev_gray % 8 == 0), dev_gray, (unsigned long long*)dev_workspace);
  hipLaunchKernelGGL(quality_finish_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, (const unsigned long long*)dev_workspace, batch,
                     (unsigned long long)h * (unsigned long long)w, enable ? 1 : 0, blur_th, flat_th, motion_th, glitch_flat_th, dev_is_bad,
                     dev_reason, dev_lap_var, dev_gray_std, dev_mad);
  return launched(e);
}

int unetpp_threshold_classes_f32(unetpp_engine* e, const float* dev_prob, int64_t frame_stride, int pixel_stride, const int64_t* plane_offsets,
                                 int batch, int src_h, int src_w, const float* thresholds, float ratio, int dst_h, int dst_w,
                                 uint8_t* dev_bits, void* stream) {
  REQUIRE_ARGS(e, dev_prob && plane_offsets && thresholds && dev_bits);
  if (int rc = eval_shape_check(e, batch, src_h, src_w, 1ull << 31)) return rc;
  if (int rc = eval_shape_check(e, batch, dst_h, dst_w, 1ull << 31)) return rc;
  if (dst_h > MAX_DIM) return fail(e, UNETPP_E_INVALID, "dst_h %d: at most %d rows (a grid dimension)", dst_h, MAX_DIM);
  if ((uintptr_t)dev_prob % 4) return fail(e, UNETPP_E_INVALID, "dev_prob must be 4-byte aligned");
  const int64_t hw = (int64_t)src_h * src_w;
  if (pixel_stride < 1 || pixel_stride > 256 || frame_stride < hw * pixel_stride || frame_stride >= (1ll << 40))
    return fail(e, UNETPP_E_INVALID, "pixel_stride %d, frame_stride %lld: 1 <= pixel_stride <= 256, frame_stride >= src_h * src_w * pixel_stride",
                pixel_stride, (long long)frame_stride);
  ThresholdArgs A{};
  for (int k = 0; k < TC_PLANES; ++k) {
    // the last float of plane k lies inside the frame's frame_stride floats
    if (plane_offsets[k] < 0 || plane_offsets[k] + (hw - 1) * pixel_stride >= frame_stride)
      return fail(e, UNETPP_E_INVALID, "plane %d at offset %lld does not lie inside a frame of %lld floats", k, (long long)plane_offsets[k],
                  (long long)frame_stride);
    if (thresholds[k] != thresholds[k]) return fail(e, UNETPP_E_INVALID, "threshold %d is NaN", k);
    A.chan_off[k] = plane_offsets[k];
    A.thr[k] = thresholds[k];
  }
  if (ratio != ratio) return fail(e, UNETPP_E_INVALID, "ratio is NaN");
  A.frame_stride = frame_stride; A.pixel_stride = pixel_stride; A.ratio = ratio;
  A.sh = src_h; A.sw = src_w; A.H = dst_h; A.W = dst_w; A.resize = src_h != dst_h || src_w != dst_w;
  ENTER_DEVICE(e);
  void *xt = nullptr, *yt = nullptr;
  if (A.resize) {
    if (const int rc = resize_table(e, 2, src_w, dst_w, &xt)) return rc;
    if (const int rc = resize_table(e, 2, src_h, dst_h, &yt)) return rc;
  }
  const dim3 grid((unsigned)((dst_w + TC_PX * MC_THREADS - 1) / (TC_PX * MC_THREADS)), (unsigned)dst_h, (unsigned)batch);
  hipLaunchKernelGGL(threshold_classes_kernel, grid, dim3(MC_THREADS), 0, (hipStream_t)stream, dev_prob, A, (const int4*)xt, (const int4*)yt,
                     (int)(dst_w % 4 == 0 && (uintptr_t)dev_bits % 4 == 0), dev_bits);
  return launched(e);
}

struct MergePlan {
  MergeArgs args;
  dim3 grid;
  size_t lds_bytes = 0;
};

// Checks the planes and their programs and lays the tiles out.  Everything the kernel indexes with is validated here.
static int merge_plan(unetpp_engine* e, int batch, int h, int w, int n_planes, const unetpp_morph_element* elements, int n_elements,
                      const unetpp_merge_step* steps, int n_steps, MergePlan* plan) {
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_INVALID, "bad shape %dx%dx%d", batch, h, w);
  if (n_planes < 1) return fail(e, UNETPP_E_INVALID, "n_planes %d: at least 1", n_planes);
  if (n_planes > MC_MAX_PLANES) return fail(e, UNETPP_E_UNSUPPORTED, "n_planes %d: at most %d", n_planes, MC_MAX_PLANES);
  if (n_elements < 0 || (n_elements > 0 && !elements)) return fail(e, UNETPP_E_INVALID, "n_elements %d with NULL elements", n_elements);
  if (n_steps < 0 || (n_steps > 0 && !steps)) return fail(e, UNETPP_E_INVALID, "n_steps %d with NULL steps", n_steps);
  if (n_elements > MORPH_MAX_ELEMENTS) return fail(e, UNETPP_E_UNSUPPORTED, "n_elements %d: at most %d over all planes", n_elements, MORPH_MAX_ELEMENTS);
  if (n_steps > MORPH_MAX_STEPS) return fail(e, UNETPP_E_UNSUPPORTED, "n_steps %d: at most %d over all planes", n_steps, MORPH_MAX_STEPS);
  MergeArgs& A = plan->args;
  std::memset(&A, 0, sizeof A);
  int ax[MORPH_MAX_ELEMENTS], ay[MORPH_MAX_ELEMENTS];
  if (const int rc = morph_elements(e, elements, n_elements, A.elem, ax, ay)) return rc;
  int up[MC_MAX_PLANES] = {}, down[MC_MAX_PLANES] = {}, left[MC_MAX_PLANES] = {}, right[MC_MAX_PLANES] = {};
  int reach_v = 0, reach_h = 0;
  for (int s = 0; s < n_steps; ++s) {
    const unetpp_merge_step& st = steps[s];
    if (st.plane < 0 || st.plane >= n_planes) return fail(e, UNETPP_E_INVALID, "step %d: plane %d not in [0,%d)", s, st.plane, n_planes);
    if (st.op != UNETPP_MORPH_DILATE && st.op != UNETPP_MORPH_ERODE && st.op != UNETPP_MERGE_OPEN && st.op != UNETPP_MERGE_CLOSE)
      return fail(e, UNETPP_E_INVALID, "step %d: op %d is not dilate, erode, open or close", s, st.op);
    if (st.element < 0 || st.element >= n_elements) return fail(e, UNETPP_E_INVALID, "step %d: element index %d not in [0,%d)", s, st.element, n_elements);
    if (st.iterations < 1) return fail(e, UNETPP_E_INVALID, "step %d: iterations must be at least 1, got %d", s, st.iterations);
    if (st.iterations > MORPH_MAX_REACH) return fail(e, UNETPP_E_UNSUPPORTED, "step %d: iterations %d beyond %d", s, st.iterations, MORPH_MAX_REACH);
    const unetpp_morph_element& el = elements[st.element];
    const int passes = (st.op == UNETPP_MERGE_OPEN || st.op == UNETPP_MERGE_CLOSE ? 2 : 1) * st.iterations;
    up[st.plane] += passes * ay[st.element]; down[st.plane] += passes * (el.kh - 1 - ay[st.element]);
    left[st.plane] += passes * ax[st.element]; right[st.plane] += passes * (el.kw - 1 - ax[st.element]);
    reach_v += passes * (el.kh - 1); reach_h += passes * (el.kw - 1);
    if (reach_v > MORPH_MAX_REACH || reach_h > MORPH_MAX_REACH)
      return fail(e, UNETPP_E_UNSUPPORTED, "the programs' reach (sum of iterations * (k - 1) over the dilates and erodes of all planes) exceeds %d "
                  "pixels (vertical %d, horizontal %d)", MORPH_MAX_REACH, reach_v, reach_h);
    A.step[s] = MergeStep{st.plane, st.op, st.element, st.iterations};
  }
  A.n_steps = n_steps; A.n_planes = n_planes;
  A.H = h; A.W = w; A.wpr = (w + 63) / 64;
  // the window must hold the widest halo of any plane; a plane with a smaller one recomputes a little more than it needs
  const int hu = *std::max_element(up, up + n_planes), hd = *std::max_element(down, down + n_planes);
  const int hl = *std::max_element(left, left + n_planes), hr = *std::max_element(right, right + n_planes);
  const int halo = hu + hd, plane_words = std::min(MORPH_PLANE_WORDS, MC_LDS_WORDS / (n_planes + 2));
  morph_tiles(plane_words, batch, h, A.wpr, halo, hl, hr, &A.band, &A.cw, &A.hl, &A.tw);
  A.up = hu; A.rows = A.band + halo;
  if (A.band < 1 || A.cw < 1 || A.rows * A.tw > plane_words) return fail(e, UNETPP_E_STATE, "internal: merge tile layout");
  plan->grid = tile_grid(A.wpr, h, A.cw, A.band, batch);
  plan->lds_bytes = (size_t)(n_planes + 2) * A.rows * A.tw * sizeof(unsigned long long);
  return UNETPP_OK;
}

int unetpp_merge_classes_layout(int batch, int h, int w, int n_planes, const unetpp_morph_element* elements, int n_elements,
                                const unetpp_merge_step* steps, int n_steps, int* band_rows, int* tile_cols) {
  if (!band_rows || !tile_cols) return fail(nullptr, UNETPP_E_INVALID, "null argument");
  MergePlan plan;
  if (const int rc = merge_plan(nullptr, batch, h, w, n_planes, elements, n_elements, steps, n_steps, &plan)) return rc;
  *band_rows = plan.args.band;
  *tile_cols = plan.args.cw * 64;
  return UNETPP_OK;
}

int unetpp_merge_classes(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, const uint8_t* lut, int n_planes,
                         const int32_t* out_values, const unetpp_morph_element* elements, int n_elements, const unetpp_merge_step* steps,
                         int n_steps, uint8_t* dev_out, int32_t* dev_table, int table_classes, void* stream) {
  REQUIRE_ARGS(e, dev_mask && lut && out_values && (dev_out || dev_table));
  MergePlan plan;
  if (const int rc = merge_plan(e, batch, h, w, n_planes, elements, n_elements, steps, n_steps, &plan)) return rc;
  MergeArgs& A = plan.args;
  for (int k = 0; k < n_planes; ++k) {
    if (out_values[k] != -1 && (out_values[k] < 1 || out_values[k] > 255))
      return fail(e, UNETPP_E_INVALID, "out_values[%d] = %d: 1..255, or -1 for the input pixel's own value", k, out_values[k]);
    A.out_value[k] = out_values[k];
  }
  for (int v = 0; v < 256; ++v) {
    if (lut[v] >> n_planes) return fail(e, UNETPP_E_INVALID, "lut[%d] = %d names a plane beyond the %d given", v, lut[v], n_planes);
    A.lut[v] = lut[v];
  }
  if (dev_table && (table_classes < 1 || table_classes > 256)) return fail(e, UNETPP_E_INVALID, "table_classes %d: 1..256", table_classes);
  if ((uintptr_t)dev_table % 4) return fail(e, UNETPP_E_INVALID, "dev_table must be 4-byte aligned");
  const size_t n = (size_t)batch * h * w, tb = dev_table ? (size_t)batch * table_classes * MC_TABLE_COLS * sizeof(int32_t) : 0;
  if (dev_out && overlaps(dev_mask, n, dev_out, n))
    return fail(e, UNETPP_E_INVALID, "dev_out aliases dev_mask: every workgroup reads the halo rows its neighbours write");
  if (dev_table && (overlaps(dev_mask, n, dev_table, tb) || (dev_out && overlaps(dev_out, n, dev_table, tb))))
    return fail(e, UNETPP_E_INVALID, "dev_table overlaps a mask");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  A.vec_in = vec16(w, dev_mask); A.vec_out = dev_out ? vec16(w, dev_out) : 0;
  A.table_classes = dev_table ? table_classes : 0;
  if (dev_table) {
    const int rows = batch * table_classes;
    hipLaunchKernelGGL(merge_table_init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (int*)dev_table, rows);
  }
  hipLaunchKernelGGL(merge_classes_kernel, plan.grid, dim3(MORPH_THREADS), plan.lds_bytes, s, dev_mask, dev_out, (int*)dev_table, A);
  return launched(e);
}

int unetpp_overlay_u8(unetpp_engine* e, const uint8_t* dev_frames, const uint8_t* dev_mask, int batch, int h, int w, const uint8_t* colors,
                      const uint8_t* has_color, float w_frame, float w_color, int mode, uint8_t* dev_out, void* stream) {
  REQUIRE_ARGS(e, dev_frames && dev_mask && colors && has_color && dev_out);
  if (int rc = eval_shape_check(e, batch, h, w, 1ull << 31)) return rc;
  if (mode != UNETPP_OVERLAY_REGION && mode != UNETPP_OVERLAY_WEIGHTED) return fail(e, UNETPP_E_INVALID, "mode %d: 0 (region) or 1 (weighted)", mode);
  if (!(w_frame >= 0.f && w_frame <= 1.f && w_color >= 0.f && w_color <= 1.f))
    return fail(e, UNETPP_E_INVALID, "weights %g, %g: both in [0,1]", (double)w_frame, (double)w_color);
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_out, 3 * n, dev_frames, 3 * n) || overlaps(dev_out, 3 * n, dev_mask, n))
    return fail(e, UNETPP_E_INVALID, "dev_out aliases an input");
  const size_t items = (n + OV_PX - 1) / OV_PX;
  if ((items + MC_THREADS - 1) / MC_THREADS > 0x7fffffffull) return fail(e, UNETPP_E_UNSUPPORTED, "batch %d of %dx%d: too many pixels for one launch", batch, h, w);
  OverlayColors C;
  for (int v = 0; v < 256; ++v)
    C.c[v] = (uint32_t)colors[3 * v] | (uint32_t)colors[3 * v + 1] << 8 | (uint32_t)colors[3 * v + 2] << 16 | (has_color[v] ? 1u << 24 : 0u);
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)((items + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, dev_frames,
                     dev_mask, n, C, w_frame, w_color, mode, vec16(16, dev_frames, dev_mask, dev_out), dev_out);
  return launched(e);
}

// ---- the ROI and full-frame 3-class loops (roi_loop.h; include/unetpp_roi.h) ---------------------------------------------------
struct RoiStatsWorkspace { size_t sums = 0, maxbits = 0, total = 0; };
static bool roi_stats_layout(int batch, RoiStatsWorkspace* ws) {
  if (batch < 1 || batch > MAX_DIM) return false;
  Carve c;
  ws->sums = c.take((size_t)batch * 3 * sizeof(unsigned long long));
  ws->maxbits = c.take((size_t)batch * 3 * sizeof(unsigned));              // directly behind sums: one memset clears both
  ws->total = c.end;
  return true;
}
static bool roi_table_ok(const void* dev_roi) { return (uintptr_t)dev_roi % 4 == 0; }

size_t unetpp_roi_projection_workspace_bytes(int batch, int w) {
  return batch >= 1 && batch <= MAX_DIM && w >= 1 && w <= MAX_DIM ? align_up((size_t)batch * w * sizeof(int), 256) : 0;
}

size_t unetpp_roi_stats_workspace_bytes(int batch) {
  RoiStatsWorkspace ws;
  return roi_stats_layout(batch, &ws) ? ws.total : 0;
}

int unetpp_roi_from_edges_u8(unetpp_engine* e, const uint8_t* dev_edges, int batch, int h, int w, int32_t* dev_roi, void* dev_workspace,
                             void* stream) {
  REQUIRE_ROBUST(e, dev_edges && dev_roi && dev_workspace);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  if ((uintptr_t)dev_workspace % 4 || !roi_table_ok(dev_roi)) return fail(e, UNETPP_E_UNSUPPORTED, "dev_workspace and dev_roi must be 4-byte aligned");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  int* counts = (int*)dev_workspace;
  HIP_TRY(e, hipMemsetAsync(counts, 0, (size_t)batch * w * sizeof(int), s));
  hipLaunchKernelGGL(roi_column_count_kernel, dim3((unsigned)((w + ROI_THREADS - 1) / ROI_THREADS), (unsigned)((h + ROI_BAND - 1) / ROI_BAND), (unsigned)batch),
                     dim3(ROI_THREADS), 0, s, dev_edges, h, w, counts);
  hipLaunchKernelGGL(roi_decide_kernel, dim3((unsigned)batch), dim3(ROI_THREADS), 0, s, (const int*)counts, w, (int*)dev_roi);
  return launched(e);
}

int unetpp_roi_crop_resize_u8(unetpp_engine* e, const uint8_t* dev_frames, int batch, int h, int w, int channels, const int32_t* dev_roi,
                              uint8_t* dev_out, int out_h, int out_w, void* stream) {
  REQUIRE_ROBUST(e, dev_frames && dev_roi && dev_out);
  if (!shape_ok(batch, h, w, MASK_SHAPE) || !shape_ok(batch, out_h, out_w, MASK_SHAPE) || channels < 1 || channels > 4)
    return fail(e, UNETPP_E_UNSUPPORTED, "crop_resize: bad shape %dx%dx%dx%d -> %dx%d", batch, h, w, channels, out_h, out_w);
  if (!roi_table_ok(dev_roi)) return fail(e, UNETPP_E_UNSUPPORTED, "dev_roi must be 4-byte aligned");
  if (overlaps(dev_frames, (size_t)batch * h * w * channels, dev_out, (size_t)batch * out_h * out_w * channels))
    return fail(e, UNETPP_E_UNSUPPORTED, "dev_out aliases dev_frames");
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(roi_crop_resize_kernel, dim3((unsigned)((out_w + ROI_THREADS - 1) / ROI_THREADS), (unsigned)out_h, (unsigned)batch), dim3(ROI_THREADS), 0,
                     (hipStream_t)stream, dev_frames, h, w, channels, (const int*)dev_roi, out_h, out_w, dev_out);
  return launched(e);
}

static int roi_probs_check(unetpp_engine* e, const float* dev_probs, int batch, int channels, int h, int w) {
  if (!shape_ok(batch, h, w, MASK_SHAPE) || channels < 3 || channels > MAX_DIM)
    return fail(e, UNETPP_E_UNSUPPORTED, "probabilities %dx%dx%dx%d: 3 <= channels, 1 <= h, w <= 65535, h * w <= 2^30", batch, channels, h, w);
  if ((uintptr_t)dev_probs % 4) return fail(e, UNETPP_E_UNSUPPORTED, "dev_probs must be 4-byte aligned");
  return UNETPP_OK;
}

int unetpp_roi_adaptive_thresholds_f32(unetpp_engine* e, const float* dev_probs, int batch, int channels, int h, int w, float* dev_thresholds,
                                       float* dev_means, float* dev_maxima, void* dev_workspace, void* stream) {
  REQUIRE_ROBUST(e, dev_probs && dev_thresholds && dev_means && dev_maxima && dev_workspace);
  if (int rc = roi_probs_check(e, dev_probs, batch, channels, h, w)) return rc;
  RoiStatsWorkspace ws;
  roi_stats_layout(batch, &ws);
  if ((uintptr_t)dev_workspace % 8 || ((uintptr_t)dev_thresholds | (uintptr_t)dev_means | (uintptr_t)dev_maxima) % 4)
    return fail(e, UNETPP_E_UNSUPPORTED, "dev_workspace must be 8-byte aligned, the tables 4-byte aligned");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const unsigned hw = (unsigned)h * (unsigned)w;
  unsigned long long* sums = (unsigned long long*)((char*)dev_workspace + ws.sums);
  unsigned* maxbits = (unsigned*)((char*)dev_workspace + ws.maxbits);
  HIP_TRY(e, hipMemsetAsync(dev_workspace, 0, ws.total, s));
  hipLaunchKernelGGL(roi_plane_sums_kernel, dim3((hw + PM_SPAN - 1) / PM_SPAN, 3u, (unsigned)batch), dim3(ROI_THREADS), 0, s, dev_probs, channels, hw, sums,
                     maxbits);
  hipLaunchKernelGGL(roi_thresholds_kernel, dim3((unsigned)((batch + ROI_THREADS - 1) / ROI_THREADS)), dim3(ROI_THREADS), 0, s,
                     (const unsigned long long*)sums, (const unsigned*)maxbits, batch, hw, dev_thresholds, dev_means, dev_maxima);
  return launched(e);
}

int unetpp_roi_ultra_strict_f32(unetpp_engine* e, const float* dev_probs, int batch, int channels, int h, int w, const float* dev_thresholds,
                                uint8_t* dev_cable, uint8_t* dev_tape, void* stream) {
  REQUIRE_ROBUST(e, dev_probs && dev_thresholds && dev_cable && dev_tape);
  if (int rc = roi_probs_check(e, dev_probs, batch, channels, h, w)) return rc;
  if ((uintptr_t)dev_thresholds % 4) return fail(e, UNETPP_E_UNSUPPORTED, "dev_thresholds must be 4-byte aligned");
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_cable, n, dev_tape, n) || overlaps(dev_probs, n * channels * sizeof(float), dev_cable, n) ||
      overlaps(dev_probs, n * channels * sizeof(float), dev_tape, n))
    return fail(e, UNETPP_E_UNSUPPORTED, "the masks overlap each other or dev_probs");
  ENTER_DEVICE(e);
  const unsigned hw = (unsigned)h * (unsigned)w;
  hipLaunchKernelGGL(roi_ultra_strict_kernel, dim3((hw + PM_SPAN - 1) / PM_SPAN, (unsigned)batch), dim3(ROI_THREADS), 0, (hipStream_t)stream, dev_probs,
                     channels, hw, dev_thresholds, dev_cable, dev_tape);
  return launched(e);
}

int unetpp_roi_components_select(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats, const uint64_t* dev_sums,
                                 int batch, int h, int w, int capacity, int rule, const unetpp_roi_cc_rule* params, uint8_t out_value, uint8_t* dev_out,
                                 void* dev_workspace, void* stream) {
  REQUIRE_ROBUST(e, dev_labels && dev_num && dev_stats && dev_sums && params && dev_out && dev_workspace);
  CcWorkspace ws;
  if (capacity < 2 || !cc_layout(batch, h, w, capacity, &ws))
    return fail(e, UNETPP_E_UNSUPPORTED, "bad shape %dx%dx%d or capacity %d", batch, h, w, capacity);
  if (rule != UNETPP_ROI_RULE_GEOMETRY && rule != UNETPP_ROI_RULE_PRIMARY) return fail(e, UNETPP_E_UNSUPPORTED, "unknown rule %d", rule);
  const RoiCcRule r{params->min_area, params->min_aspect, params->wide_width, params->edge_lo, params->edge_hi, params->large_area};
  if (std::isnan(r.min_area) || std::isnan(r.min_aspect) || std::isnan(r.wide_width) || std::isnan(r.edge_lo) || std::isnan(r.edge_hi) ||
      std::isnan(r.large_area))
    return fail(e, UNETPP_E_UNSUPPORTED, "component rule: NaN parameter");
  if (out_value == 0) return fail(e, UNETPP_E_UNSUPPORTED, "out_value must not be 0");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  uint8_t* keep = (uint8_t*)dev_workspace + ws.keep;
  hipLaunchKernelGGL(roi_cc_select_kernel, dim3((unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_num, (const int*)dev_stats,
                     (const unsigned long long*)dev_sums, w, capacity, rule, r, keep);
  hipLaunchKernelGGL(cc_apply_kernel, dim3((unsigned)ws.nchunk, (unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_labels,
                     (const uint8_t*)keep, hw, capacity, vec16(hw, dev_labels, dev_out), (unsigned)out_value, dev_out);
  return launched(e);
}

int unetpp_roi_paste_masks_u8(unetpp_engine* e, const uint8_t* dev_mask0, const uint8_t* dev_mask1, int batch, int h, int w, const int32_t* dev_roi,
                              uint8_t* dev_out0, uint8_t* dev_out1, int out_h, int out_w, void* stream) {
  REQUIRE_ROBUST(e, dev_mask0 && dev_mask1 && dev_roi && dev_out0 && dev_out1);
  if (!shape_ok(batch, h, w, MASK_SHAPE) || !shape_ok(batch, out_h, out_w, MASK_SHAPE))
    return fail(e, UNETPP_E_UNSUPPORTED, "paste_masks: bad shape %dx%dx%d -> %dx%d", batch, h, w, out_h, out_w);
  if (!roi_table_ok(dev_roi)) return fail(e, UNETPP_E_UNSUPPORTED, "dev_roi must be 4-byte aligned");
  const size_t n_in = (size_t)batch * h * w, n_out = (size_t)batch * out_h * out_w;
  if (overlaps(dev_out0, n_out, dev_out1, n_out) || overlaps(dev_out0, n_out, dev_mask0, n_in) || overlaps(dev_out0, n_out, dev_mask1, n_in) ||
      overlaps(dev_out1, n_out, dev_mask0, n_in) || overlaps(dev_out1, n_out, dev_mask1, n_in))
    return fail(e, UNETPP_E_UNSUPPORTED, "an output overlaps the other output or an input");
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(roi_paste_kernel, dim3((unsigned)((out_w + ROI_THREADS - 1) / ROI_THREADS), (unsigned)out_h, (unsigned)batch), dim3(ROI_THREADS), 0,
                     (hipStream_t)stream, dev_mask0, dev_mask1, h, w, (const int*)dev_roi, out_h, out_w, dev_out0, dev_out1);
  return launched(e);
}

// ---- validation losses: the five sums per frame and class (loss.h; include/unetpp_loss.h) ---------------------------------------
int unetpp_loss_layout(int* span_pixels) {
  if (!span_pixels) return UNETPP_E_UNSUPPORTED;
  *span_pixels = LS_SPAN;
  return UNETPP_OK;
}

int unetpp_loss_sums_f32(unetpp_engine* e, const float* dev_logits, const uint8_t* dev_target, int batch, int classes, int h, int w, int gamma,
                         uint64_t* dev_table, uint32_t* dev_outside, void* stream) {
  REQUIRE_ROBUST(e, dev_logits && dev_target && dev_table && dev_outside);
  if (batch < 1 || batch > MAX_DIM || h < 1 || w < 1 || (size_t)h * (size_t)w > LS_MAX_PIXELS)
    return fail(e, UNETPP_E_UNSUPPORTED, "loss sums: shape %dx%dx%d outside 1 <= batch <= 65535, h, w >= 1, h * w <= 2^22", batch, h, w);
  if (classes < 2 || classes > LS_MAX_CLASSES || gamma < 0 || gamma > LS_MAX_GAMMA)
    return fail(e, UNETPP_E_UNSUPPORTED, "loss sums: classes %d outside 2..8 or gamma %d outside 0..4", classes, gamma);
  if ((uintptr_t)dev_logits % 4 || (uintptr_t)dev_table % 8 || (uintptr_t)dev_outside % 4)
    return fail(e, UNETPP_E_UNSUPPORTED, "dev_logits and dev_outside must be 4-byte aligned, dev_table 8-byte aligned");
  const size_t hw = (size_t)h * w, n_logits = (size_t)batch * classes * hw * sizeof(float), n_target = (size_t)batch * hw;
  const size_t n_table = (size_t)batch * classes * LS_COLUMNS * sizeof(unsigned long long), n_outside = (size_t)batch * 2 * sizeof(unsigned);
  if (overlaps(dev_table, n_table, dev_outside, n_outside) || overlaps(dev_table, n_table, dev_logits, n_logits) ||
      overlaps(dev_table, n_table, dev_target, n_target) || overlaps(dev_outside, n_outside, dev_logits, n_logits) ||
      overlaps(dev_outside, n_outside, dev_target, n_target))
    return fail(e, UNETPP_E_UNSUPPORTED, "loss sums: an output overlaps the other output or an input");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  if ((const char*)dev_outside == (const char*)dev_table + n_table) {
    HIP_TRY(e, hipMemsetAsync(dev_table, 0, n_table + n_outside, s));
  } else {
    HIP_TRY(e, hipMemsetAsync(dev_table, 0, n_table, s));
    HIP_TRY(e, hipMemsetAsync(dev_outside, 0, n_outside, s));
  }
  const dim3 grid((unsigned)((hw + LS_GROUP - 1 + LS_SPAN - 1) / LS_SPAN), (unsigned)batch);
#define LOSS_SUMS_CASE(C)                                                                                                   \
  case C:                                                                                                                   \
    hipLaunchKernelGGL(loss_sums_kernel<C>, grid, dim3(LS_THREADS), 0, s, dev_logits, dev_target, (unsigned)hw, gamma,       \
                       (unsigned long long*)dev_table, (unsigned*)dev_outside);                                              \
    break
  switch (classes) {
    LOSS_SUMS_CASE(2); LOSS_SUMS_CASE(3); LOSS_SUMS_CASE(4); LOSS_SUMS_CASE(5); LOSS_SUMS_CASE(6); LOSS_SUMS_CASE(7); LOSS_SUMS_CASE(8);
  }
#undef LOSS_SUMS_CASE
  return launched(e);
}

// ---- loss gradients: one pass from logits, target and the coefficient table (loss_grad.h; include/unetpp_loss_grad.h) ------------
int unetpp_loss_grad_layout(int* span_pixels) {
  if (!span_pixels) return UNETPP_E_UNSUPPORTED;
  *span_pixels = LS_SPAN;
  return UNETPP_OK;
}

int unetpp_loss_grad_f32(unetpp_engine* e, const float* dev_logits, const uint8_t* dev_target, int batch, int classes, int h, int w, int gamma,
                         const float* dev_coef, const float* dev_scale, float* dev_grad, void* stream) {
  REQUIRE_ROBUST(e, dev_logits && dev_target && dev_coef && dev_grad);
  if (batch < 1 || batch > MAX_DIM || h < 1 || w < 1 || (size_t)h * (size_t)w > LS_MAX_PIXELS)
    return fail(e, UNETPP_E_UNSUPPORTED, "loss grad: shape %dx%dx%d outside 1 <= batch <= 65535, h, w >= 1, h * w <= 2^22", batch, h, w);
  if (classes < 2 || classes > LS_MAX_CLASSES || gamma < 0 || gamma > LS_MAX_GAMMA)
    return fail(e, UNETPP_E_UNSUPPORTED, "loss grad: classes %d outside 2..8 or gamma %d outside 0..4", classes, gamma);
  if ((uintptr_t)dev_logits % 4 || (uintptr_t)dev_grad % 4 || (uintptr_t)dev_coef % 4 || (uintptr_t)dev_scale % 4)
    return fail(e, UNETPP_E_UNSUPPORTED, "dev_logits, dev_grad, dev_coef and dev_scale must be 4-byte aligned");
  const size_t hw = (size_t)h * w, n_logits = (size_t)batch * classes * hw * sizeof(float), n_target = (size_t)batch * hw;
  const size_t n_coef = (size_t)batch * classes * LG_COEF * sizeof(float);
  if (((const void*)dev_grad != (const void*)dev_logits && overlaps(dev_grad, n_logits, dev_logits, n_logits)) ||
      overlaps(dev_grad, n_logits, dev_target, n_target) || overlaps(dev_grad, n_logits, dev_coef, n_coef) ||
      (dev_scale && overlaps(dev_grad, n_logits, dev_scale, sizeof(float))))
    return fail(e, UNETPP_E_UNSUPPORTED, "loss grad: dev_grad overlaps an input (only dev_grad == dev_logits is allowed)");
  ENTER_DEVICE(e);
  const dim3 grid((unsigned)((hw + LS_GROUP - 1 + LS_SPAN - 1) / LS_SPAN), (unsigned)batch);
#define LOSS_GRAD_CASE(C)                                                                                                   \
  case C:                                                                                                                   \
    hipLaunchKernelGGL(loss_grad_kernel<C>, grid, dim3(LS_THREADS), 0, (hipStream_t)stream, dev_logits, dev_target,          \
                       (unsigned)hw, gamma, dev_coef, dev_scale, dev_grad);                                                  \
    break
  switch (classes) {
    LOSS_GRAD_CASE(2); LOSS_GRAD_CASE(3); LOSS_GRAD_CASE(4); LOSS_GRAD_CASE(5); LOSS_GRAD_CASE(6); LOSS_GRAD_CASE(7); LOSS_GRAD_CASE(8);
  }
#undef LOSS_GRAD_CASE
  return launched(e);
}

int unetpp_loss_narrow_target_i64(unetpp_engine* e, const int64_t* dev_target_i64, int64_t n, uint8_t* dev_target_u8, void* stream) {
  REQUIRE_ROBUST(e, dev_target_i64 && dev_target_u8);
  if (n < 1 || n > (int64_t)MAX_DIM * LS_MAX_PIXELS)
    return fail(e, UNETPP_E_UNSUPPORTED, "narrow target: n %lld outside 1 .. 65535 * 2^22", (long long)n);
  if ((uintptr_t)dev_target_i64 % 8) return fail(e, UNETPP_E_UNSUPPORTED, "dev_target_i64 must be 8-byte aligned");
  if (overlaps(dev_target_u8, (size_t)n, dev_target_i64, (size_t)n * sizeof(int64_t)))
    return fail(e, UNETPP_E_UNSUPPORTED, "narrow target: the output overlaps the input");
  ENTER_DEVICE(e);
  const size_t groups = ((size_t)n + ((uintptr_t)dev_target_u8 & 15u) + LN_GROUP - 1) / LN_GROUP;
  hipLaunchKernelGGL(loss_narrow_kernel, dim3((unsigned)((groups + LN_THREADS - 1) / LN_THREADS)), dim3(LN_THREADS), 0, (hipStream_t)stream,
                     (const long long*)dev_target_i64, (long long)n, dev_target_u8);
  return launched(e);
}

// ---- training batches: the data-dependent crop and the assembly (train_batch.h; include/unetpp_train_batch.h) -----------------------
int unetpp_train_batch_layout(int* tile_w, int* tile_h, int* pass_bytes, int* plan_columns) {
  if (!tile_w || !tile_h || !pass_bytes || !plan_columns) return UNETPP_E_UNSUPPORTED;
  *tile_w = TB_TW; *tile_h = TB_TH; *pass_bytes = TB_THREADS * TB_SEG; *plan_columns = TB_PLAN;
  return UNETPP_OK;
}

int unetpp_train_crop_rects(unetpp_engine* e, const uint8_t* dev_masks, int64_t masks_bytes, const int64_t* dev_items, int n_items,
                            const int32_t* dev_requests, int batch, int32_t* dev_rects, void* stream) {
  REQUIRE_ROBUST(e, dev_masks && dev_items && dev_requests && dev_rects);
  if (batch < 1 || batch > MAX_DIM || n_items < 1 || masks_bytes < 1)
    return fail(e, UNETPP_E_UNSUPPORTED, "crop rects: batch %d outside 1..65535, n_items %d or masks_bytes %lld below 1", batch, n_items,
                (long long)masks_bytes);
  if ((uintptr_t)dev_items % 8 || (uintptr_t)dev_requests % 4 || (uintptr_t)dev_rects % 4)
    return fail(e, UNETPP_E_UNSUPPORTED, "dev_items must be 8-byte, dev_requests and dev_rects 4-byte aligned");
  const size_t n_rects = (size_t)batch * TB_RECT * sizeof(int32_t);
  if (overlaps(dev_rects, n_rects, dev_masks, (size_t)masks_bytes) || overlaps(dev_rects, n_rects, dev_items, (size_t)n_items * TB_ITEM * 8) ||
      overlaps(dev_rects, n_rects, dev_requests, (size_t)batch * TB_REQUEST * sizeof(int32_t)))
    return fail(e, UNETPP_E_UNSUPPORTED, "crop rects: dev_rects overlaps an input");
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(tb_crop_rects_kernel, dim3((unsigned)batch), dim3(TB_THREADS), 0, (hipStream_t)stream, dev_masks, (long long)masks_bytes,
                     (const long long*)dev_items, n_items, dev_requests, dev_rects);
  return launched(e);
}

int unetpp_train_batch_u8(unetpp_engine* e, const uint8_t* dev_images, int64_t images_bytes, const uint8_t* dev_masks, int64_t masks_bytes,
                          const int64_t* dev_items, int n_items, const int32_t* dev_plan, int batch, const int32_t* dev_rects, int n_rects,
                          const uint8_t* dev_luts, int n_luts, const uint8_t* dev_class_lut, int out_h, int out_w, int image_format,
                          void* dev_image_out, uint8_t* dev_target_out, void* stream) {
  REQUIRE_ROBUST(e, dev_images && dev_masks && dev_items && dev_plan && dev_image_out && dev_target_out);
  if (batch < 1 || batch > MAX_DIM || out_h < 1 || out_h > MAX_DIM || out_w < 1 || out_w > MAX_DIM)
    return fail(e, UNETPP_E_UNSUPPORTED, "train batch: shape %dx%dx%d outside 1..65535", batch, out_h, out_w);
  if (n_items < 1 || images_bytes < 3 || masks_bytes < 1 || n_rects < 0 || n_luts < 0 || (n_rects > 0) != (dev_rects != nullptr) ||
      (n_luts > 0) != (dev_luts != nullptr))
    return fail(e, UNETPP_E_UNSUPPORTED, "train batch: n_items %d, arenas of %lld and %lld bytes, %d rects, %d look-ups: a count below its "
                "minimum, or a table without its count", n_items, (long long)images_bytes, (long long)masks_bytes, n_rects, n_luts);
  if (image_format != UNETPP_TRAIN_CHW_F32 && image_format != UNETPP_TRAIN_HWC_RGB && image_format != UNETPP_TRAIN_HWC_BGR)
    return fail(e, UNETPP_E_UNSUPPORTED, "train batch: image_format %d is none of UNETPP_TRAIN_*", image_format);
  if ((uintptr_t)dev_items % 8 || (uintptr_t)dev_plan % 4 || (uintptr_t)dev_rects % 4 ||
      (image_format == UNETPP_TRAIN_CHW_F32 && (uintptr_t)dev_image_out % 4))
    return fail(e, UNETPP_E_UNSUPPORTED, "dev_items must be 8-byte, dev_plan, dev_rects and a float32 dev_image_out 4-byte aligned");
  const size_t px = (size_t)batch * out_h * out_w, n_image = px * (image_format == UNETPP_TRAIN_CHW_F32 ? 12 : 3);
  const struct { const void* p; size_t n; } in[] = {{dev_images, (size_t)images_bytes}, {dev_masks, (size_t)masks_bytes},
      {dev_items, (size_t)n_items * TB_ITEM * 8}, {dev_plan, (size_t)batch * TB_PLAN * sizeof(int32_t)},
      {dev_rects, (size_t)n_rects * TB_RECT * sizeof(int32_t)}, {dev_luts, (size_t)n_luts * 256}, {dev_class_lut, dev_class_lut ? 256u : 0u}};
  for (const auto& a : in)
    if (a.p && a.n && (overlaps(dev_image_out, n_image, a.p, a.n) || overlaps(dev_target_out, px, a.p, a.n)))
      return fail(e, UNETPP_E_UNSUPPORTED, "train batch: an output overlaps an input");
  if (overlaps(dev_image_out, n_image, dev_target_out, px)) return fail(e, UNETPP_E_UNSUPPORTED, "train batch: the two outputs overlap");
  ENTER_DEVICE(e);
  const dim3 grid((unsigned)((out_w + TB_TW - 1) / TB_TW), (unsigned)((out_h + TB_TH - 1) / TB_TH), (unsigned)batch);
  hipLaunchKernelGGL(tb_batch_kernel, grid, dim3(TB_THREADS), 0, (hipStream_t)stream, dev_images, (long long)images_bytes, dev_masks,
                     (long long)masks_bytes, (const long long*)dev_items, n_items, dev_plan, dev_rects, n_rects, dev_luts, n_luts,
                     dev_class_lut, out_h, out_w, image_format, dev_image_out, dev_target_out);
  return launched(e);
}

// ---- external contours, the enclosing circle, paste and the chained overlay (contours.h; include/unetpp_contours.h) ---------------
struct CtWorkspace { size_t plane = 0, inside = 0, bg_labels = 0, bg_num = 0, flags = 0, rows = 0, cc = 0, total = 0; };
static bool ct_layout(int batch, int h, int w, int capacity, CtWorkspace* ws) {
  if (batch < 1 || batch > MAX_DIM || h < 1 || w < 1 || h > CT_MAX_SIDE || w > CT_MAX_SIDE || capacity < 2) return false;
  CcWorkspace cc;
  if (!cc_layout(batch, h, w, capacity, &cc)) return false;
  const size_t hw = (size_t)h * w;
  Carve c;
  ws->plane = c.take(hw * batch);
  ws->inside = c.take(hw * batch);
  ws->bg_labels = c.take(hw * batch * sizeof(int));
  ws->bg_num = c.take((size_t)batch * sizeof(int));
  ws->flags = c.take((hw + 1) * batch);
  ws->rows = c.take((size_t)h * batch * sizeof(unsigned));
  ws->cc = c.take(cc.total);
  ws->total = c.end;
  return true;
}
static const char* const CT_SHAPE_TEXT = "outside 1 <= batch <= 65535, 1 <= h, w <= 4095, capacity >= 2";

size_t unetpp_contours_workspace_bytes(int batch, int h, int w, int capacity) {
  CtWorkspace ws;
  return ct_layout(batch, h, w, capacity, &ws) ? ws.total : 0;
}

int unetpp_contour_areas_u8(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, int match_class, int capacity, int32_t* dev_labels,
                            int32_t* dev_num, uint64_t* dev_area2, uint8_t* dev_border, void* dev_workspace, void* stream) {
  REQUIRE_ROBUST(e, dev_mask && dev_labels && dev_num && dev_area2 && dev_workspace);
  CtWorkspace ws;
  if (!ct_layout(batch, h, w, capacity, &ws)) return fail(e, UNETPP_E_UNSUPPORTED, "contour areas: %dx%dx%d, capacity %d %s", batch, h, w, capacity, CT_SHAPE_TEXT);
  if (match_class > 255) return fail(e, UNETPP_E_UNSUPPORTED, "match_class %d out of range", match_class);
  if ((uintptr_t)dev_workspace % 16 || (uintptr_t)dev_labels % 4 || (uintptr_t)dev_num % 4 || (uintptr_t)dev_area2 % 8)
    return fail(e, UNETPP_E_UNSUPPORTED, "dev_workspace must be 16-byte aligned, dev_labels and dev_num 4-byte, dev_area2 8-byte");
  const size_t hw = (size_t)h * w, n = hw * batch, n_area = (size_t)batch * capacity * sizeof(unsigned long long);
  const void* outs[] = {dev_labels, dev_num, dev_area2, dev_border, dev_workspace};
  const size_t sizes[] = {n * sizeof(int), (size_t)batch * sizeof(int), n_area, dev_border ? n : 0, ws.total};
  for (int i = 0; i < 5; ++i) {
    if (!sizes[i]) continue;
    if (overlaps(outs[i], sizes[i], dev_mask, n)) return fail(e, UNETPP_E_UNSUPPORTED, "contour areas: an output or the workspace overlaps the mask");
    for (int j = i + 1; j < 5; ++j)
      if (sizes[j] && overlaps(outs[i], sizes[i], outs[j], sizes[j])) return fail(e, UNETPP_E_UNSUPPORTED, "contour areas: two outputs overlap");
  }
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)dev_workspace;
  uint8_t* plane = (uint8_t*)(base + ws.plane);
  uint8_t* inside = (uint8_t*)(base + ws.inside);
  int* bg_labels = (int*)(base + ws.bg_labels);
  uint8_t* flags = (uint8_t*)(base + ws.flags);
  const unsigned flat_blocks = (unsigned)((n + (size_t)CT_THREADS * CT_PX - 1) / ((size_t)CT_THREADS * CT_PX));
  const dim3 blk(CT_THREADS);
  HIP_TRY(e, hipMemsetAsync(flags, 0, (hw + 1) * batch, s));
  HIP_TRY(e, hipMemsetAsync(dev_area2, 0, n_area, s));
  hipLaunchKernelGGL(ct_background_kernel, dim3(flat_blocks), blk, 0, s, dev_mask, n, match_class, (int)((uintptr_t)dev_mask % 16 == 0), plane);
  if (int rc = unetpp_components(e, plane, batch, h, w, 1, 4, capacity, bg_labels, (int32_t*)(base + ws.bg_num), nullptr, nullptr, base + ws.cc, stream))
    return rc;
  hipLaunchKernelGGL(ct_edge_flags_kernel, dim3((unsigned)((2 * w + 2 * h + CT_THREADS - 1) / CT_THREADS), (unsigned)batch), blk, 0, s,
                     (const int*)bg_labels, h, w, flags);
  hipLaunchKernelGGL(ct_inside_kernel, dim3(flat_blocks), blk, 0, s, (const int*)bg_labels, (const uint8_t*)flags, batch, h, w,
                     (int)((uintptr_t)dev_border % 16 == 0), inside, dev_border);
  if (int rc = unetpp_components(e, inside, batch, h, w, 1, 8, capacity, dev_labels, dev_num, nullptr, nullptr, base + ws.cc, stream)) return rc;
  hipLaunchKernelGGL(ct_area_kernel, dim3((unsigned)((w + 1 + CT_THREADS * CT_WIN - 1) / (CT_THREADS * CT_WIN)), (unsigned)(h + 1), (unsigned)batch), blk,
                     0, s, (const int*)dev_labels, h, w, capacity, (unsigned long long*)dev_area2);
  return launched(e);
}

int unetpp_contour_circle(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const uint64_t* dev_area2, int batch, int h, int w,
                          int capacity, int32_t* dev_support, void* dev_workspace, void* stream) {
  REQUIRE_ROBUST(e, dev_labels && dev_num && dev_area2 && dev_support && dev_workspace);
  CtWorkspace ws;
  if (!ct_layout(batch, h, w, capacity, &ws)) return fail(e, UNETPP_E_UNSUPPORTED, "contour circle: %dx%dx%d, capacity %d %s", batch, h, w, capacity, CT_SHAPE_TEXT);
  if ((uintptr_t)dev_workspace % 16 || (uintptr_t)dev_labels % 4 || (uintptr_t)dev_num % 4 || (uintptr_t)dev_area2 % 8 || (uintptr_t)dev_support % 4)
    return fail(e, UNETPP_E_UNSUPPORTED, "dev_workspace must be 16-byte aligned, dev_labels, dev_num and dev_support 4-byte, dev_area2 8-byte");
  const size_t n_support = (size_t)batch * 8 * sizeof(int);
  if (overlaps(dev_support, n_support, dev_labels, (size_t)batch * h * w * sizeof(int)) || overlaps(dev_support, n_support, dev_num, (size_t)batch * sizeof(int)) ||
      overlaps(dev_support, n_support, dev_area2, (size_t)batch * capacity * sizeof(unsigned long long)) ||
      overlaps(dev_support, n_support, dev_workspace, ws.total))
    return fail(e, UNETPP_E_UNSUPPORTED, "contour circle: dev_support overlaps an input or the workspace");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  unsigned* rows = (unsigned*)((char*)dev_workspace + ws.rows);
  hipLaunchKernelGGL(ct_choose_kernel, dim3((unsigned)batch), dim3(CT_THREADS), 0, s, (const int*)dev_num, (const unsigned long long*)dev_area2, capacity,
                     (int*)dev_support);
  hipLaunchKernelGGL(ct_row_extremes_kernel, dim3((unsigned)h, (unsigned)batch), dim3(64), 0, s, (const int*)dev_labels, (const int*)dev_support, h, w, rows);
  hipLaunchKernelGGL(ct_circle_kernel, dim3((unsigned)batch), dim3(CT_THREADS), 0, s, (const unsigned*)rows, h, (int*)dev_support);
  return launched(e);
}

int unetpp_paste_roi_u8(unetpp_engine* e, const uint8_t* dev_masks, int batch, int h, int w, int roi_x, int roi_y, int roi_w, int roi_h, int out_h,
                        int out_w, uint8_t* dev_out, void* stream) {
  REQUIRE_ROBUST(e, dev_masks && dev_out);
  if (!shape_ok(batch, h, w, MASK_SHAPE) || !shape_ok(batch, out_h, out_w, MASK_SHAPE) || (size_t)batch * out_h * out_w > (1ull << 40))
    return fail(e, UNETPP_E_UNSUPPORTED, "paste_roi: bad shape %dx%dx%d -> %dx%d", batch, h, w, out_h, out_w);
  const long long x1 = std::max(0, roi_x), y1 = std::max(0, roi_y);
  const long long x2 = std::min<long long>(out_w, (long long)roi_x + roi_w), y2 = std::min<long long>(out_h, (long long)roi_y + roi_h);
  const long long pw = std::min<long long>(w, x2 - x1), ph = std::min<long long>(h, y2 - y1);
  if (pw < 1 || ph < 1) return fail(e, UNETPP_E_UNSUPPORTED, "paste_roi: roi (%d, %d, %d, %d) misses the %dx%d frame", roi_x, roi_y, roi_w, roi_h, out_h, out_w);
  const size_t n_in = (size_t)batch * h * w, n_out = (size_t)batch * out_h * out_w;
  if (overlaps(dev_out, n_out, dev_masks, n_in)) return fail(e, UNETPP_E_UNSUPPORTED, "paste_roi: dev_out overlaps dev_masks");
  const int pad = (int)((uintptr_t)dev_out % 16);
  const size_t blocks = (n_out + pad + (size_t)CT_THREADS * CT_PX - 1) / ((size_t)CT_THREADS * CT_PX);
  if (blocks > 0x7fffffffull) return fail(e, UNETPP_E_UNSUPPORTED, "paste_roi: too many pixels for one launch");
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(ct_paste_kernel, dim3((unsigned)blocks), dim3(CT_THREADS), 0, (hipStream_t)stream, dev_masks, batch, h, w, (int)x1, (int)y1, (int)pw,
                     (int)ph, out_h, out_w, pad, dev_out);
  return launched(e);
}

int unetpp_overlay_chain_u8(unetpp_engine* e, const uint8_t* dev_frames, const uint8_t* dev_cable, const uint8_t* dev_tape, const uint8_t* dev_burr,
                            int batch, int h, int w, const uint8_t* host_table, uint8_t* dev_out, void* stream) {
  REQUIRE_ROBUST(e, dev_frames && dev_cable && dev_tape && dev_burr && host_table && dev_out);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "overlay chain: bad shape %dx%dx%d", batch, h, w);
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_out, 3 * n, dev_frames, 3 * n) || overlaps(dev_out, 3 * n, dev_cable, n) || overlaps(dev_out, 3 * n, dev_tape, n) ||
      overlaps(dev_out, 3 * n, dev_burr, n))
    return fail(e, UNETPP_E_UNSUPPORTED, "overlay chain: dev_out overlaps an input");
  const int pad = (int)((uintptr_t)dev_out % 16);
  const size_t blocks = (3 * n + pad + (size_t)CT_THREADS * CT_PX - 1) / ((size_t)CT_THREADS * CT_PX);
  if (blocks > 0x7fffffffull) return fail(e, UNETPP_E_UNSUPPORTED, "overlay chain: too many pixels for one launch");
  CtOverlayTable T;
  std::memcpy(T.w, host_table, sizeof(T.w));
  ENTER_DEVICE(e);
  hipLaunchKernelGGL(ct_overlay_kernel, dim3((unsigned)blocks), dim3(CT_THREADS), 0, (hipStream_t)stream, dev_frames, dev_cable, dev_tape, dev_burr,
                     (long long)(3 * n), T, pad, (int)((uintptr_t)dev_frames % 16 == (uintptr_t)pad), dev_out);
  return launched(e);
}

// ---- the pixel and component rules of the spatial, fixed and simple loops (simple_loops.h, include/unetpp_simple_loops.h) ------------
int unetpp_pixel_rules_f32(unetpp_engine* e, const float* dev_probs, int64_t frame_stride, int64_t plane_stride, int64_t pixel_stride, int batch, int h,
                           int w, int rule, float a, float b, uint8_t* dev_cable, uint8_t* dev_tape, void* stream) {
  REQUIRE_ROBUST(e, dev_probs && dev_cable && dev_tape);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "pixel rules: shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  if (rule != UNETPP_PIXEL_RELATIVE && rule != UNETPP_PIXEL_CONFIDENCE) return fail(e, UNETPP_E_UNSUPPORTED, "pixel rules: unknown rule %d", rule);
  if (std::isnan(a) || std::isnan(b)) return fail(e, UNETPP_E_UNSUPPORTED, "pixel rules: NaN parameter");
  const long long hw = (long long)h * w;
  const long long lim = 1ll << 40;                           // keeps every product below inside int64
  if (frame_stride < 1 || plane_stride < 1 || pixel_stride < 1 || frame_stride > lim || plane_stride > lim || pixel_stride > (1 << 20) ||
      2 * plane_stride + (hw - 1) * pixel_stride + 1 > frame_stride)
    return fail(e, UNETPP_E_UNSUPPORTED, "pixel rules: strides (%lld, %lld, %lld) do not hold three planes of %lld pixels in one frame",
                (long long)frame_stride, (long long)plane_stride, (long long)pixel_stride, hw);
  if ((uintptr_t)dev_probs % 4) return fail(e, UNETPP_E_UNSUPPORTED, "pixel rules: dev_probs must be 4-byte aligned");
  const size_t n = (size_t)batch * hw, np_ = (size_t)batch * (size_t)frame_stride * sizeof(float);
  if (overlaps(dev_cable, n, dev_tape, n) || overlaps(dev_probs, np_, dev_cable, n) || overlaps(dev_probs, np_, dev_tape, n))
    return fail(e, UNETPP_E_UNSUPPORTED, "pixel rules: the masks overlap each other or dev_probs");
  ENTER_DEVICE(e);
  const long long span = (long long)SL_THREADS * SL_PX;
  hipLaunchKernelGGL(sl_pixel_rules_kernel, dim3((unsigned)((hw + span - 1) / span), (unsigned)batch), dim3(SL_THREADS), 0, (hipStream_t)stream, dev_probs,
                     (long long)frame_stride, (long long)plane_stride, (long long)pixel_stride, hw, rule, a, b, dev_cable, dev_tape);
  return launched(e);
}

int unetpp_components_keep(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats, int batch, int h, int w,
                           int capacity, int min_area, int max_area, int min_width, uint8_t out_value, uint8_t* dev_out, void* dev_workspace,
                           void* stream) {
  REQUIRE_ROBUST(e, dev_labels && dev_num && dev_stats && dev_out && dev_workspace);
  CcWorkspace ws;
  if (capacity < 2 || !cc_layout(batch, h, w, capacity, &ws))
    return fail(e, UNETPP_E_UNSUPPORTED, "components keep: bad shape %dx%dx%d or capacity %d", batch, h, w, capacity);
  if (out_value == 0) return fail(e, UNETPP_E_UNSUPPORTED, "out_value must not be 0");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  uint8_t* keep = (uint8_t*)dev_workspace + ws.keep;
  hipLaunchKernelGGL(sl_keep_select_kernel, dim3((unsigned)batch), dim3(SL_THREADS), 0, s, (const int*)dev_num, (const int*)dev_stats, capacity, min_area,
                     max_area, min_width, keep);
  hipLaunchKernelGGL(cc_apply_kernel, dim3((unsigned)ws.nchunk, (unsigned)batch), dim3(CC_THREADS), 0, s, (const int*)dev_labels,
                     (const uint8_t*)keep, hw, capacity, vec16(hw, dev_labels, dev_out), (unsigned)out_value, dev_out);
  return launched(e);
}

int unetpp_tape_position_filter_u8(unetpp_engine* e, const uint8_t* dev_tape, int tape_match, const uint8_t* dev_cable, int cable_match, int batch,
                                   int h, int w, uint8_t* dev_out, int32_t* dev_table, void* stream) {
  REQUIRE_ROBUST(e, dev_tape && dev_cable && dev_out && dev_table);
  if (tape_match > 255 || cable_match > 255) return fail(e, UNETPP_E_UNSUPPORTED, "tape filter: match value out of range");
  if (!shape_ok(batch, h, w, MASK_SHAPE) || (size_t)h * w > (size_t)UNETPP_TAPE_MAX_PIXELS)
    return fail(e, UNETPP_E_UNSUPPORTED, "tape filter: shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^23", batch, h, w);
  if ((uintptr_t)dev_table % 4) return fail(e, UNETPP_E_UNSUPPORTED, "tape filter: dev_table must be 4-byte aligned");
  const size_t n = (size_t)batch * h * w, nt = (size_t)batch * SL_TABLE * sizeof(int32_t);
  if (overlaps(dev_out, n, dev_tape, n) || (dev_cable != dev_tape && overlaps(dev_out, n, dev_cable, n)) || overlaps(dev_table, nt, dev_out, n) ||
      overlaps(dev_table, nt, dev_tape, n) || overlaps(dev_table, nt, dev_cable, n))
    return fail(e, UNETPP_E_UNSUPPORTED, "tape filter: dev_out or dev_table overlaps another buffer");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  int* table = (int*)dev_table;
  HIP_TRY(e, hipMemsetAsync(table, 0, nt, s));
  const dim3 rows((unsigned)((h + SL_THREADS / SL_WAVE - 1) / (SL_THREADS / SL_WAVE)), (unsigned)batch);
  hipLaunchKernelGGL(sl_tape_sums_kernel, rows, dim3(SL_THREADS), 0, s, dev_tape, tape_match, dev_cable, cable_match, h, w, table);
  hipLaunchKernelGGL(sl_tape_filtered_kernel, rows, dim3(SL_THREADS), 0, s, dev_tape, tape_match, h, w, table);
  hipLaunchKernelGGL(sl_tape_finish_kernel, dim3((unsigned)((batch + SL_THREADS - 1) / SL_THREADS)), dim3(SL_THREADS), 0, s, batch, w, table);
  const int vec = w % 4 == 0 && ((uintptr_t)dev_tape | (uintptr_t)dev_out) % 4 == 0;
  hipLaunchKernelGGL(sl_tape_apply_kernel, dim3((unsigned)((w + 4 * SL_THREADS - 1) / (4 * SL_THREADS)), (unsigned)h, (unsigned)batch), dim3(SL_THREADS), 0,
                     s, dev_tape, tape_match, (const int*)table, h, w, vec, dev_out);
  return launched(e);
}

int unetpp_column_band_u8(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, int x_start, int x_end, uint8_t* dev_out, void* stream) {
  REQUIRE_ROBUST(e, dev_mask && dev_out);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "column band: shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  if (x_start < 0 || x_start > w || x_end < 0 || x_end > w) return fail(e, UNETPP_E_UNSUPPORTED, "column band: columns [%d, %d) outside 0..%d", x_start, x_end, w);
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_mask, n, dev_out, n)) return fail(e, UNETPP_E_UNSUPPORTED, "column band: dev_out overlaps dev_mask");
  ENTER_DEVICE(e);
  const int vec = w % 4 == 0 && ((uintptr_t)dev_mask | (uintptr_t)dev_out) % 4 == 0;
  hipLaunchKernelGGL(sl_column_band_kernel, dim3((unsigned)((w + 4 * SL_THREADS - 1) / (4 * SL_THREADS)), (unsigned)h, (unsigned)batch), dim3(SL_THREADS), 0,
                     (hipStream_t)stream, dev_mask, h, w, x_start, x_end, vec, dev_out);
  return launched(e);
}

int unetpp_mask_join_u8(unetpp_engine* e, const uint8_t* dev_a, int and_a, const uint8_t* dev_b, int or_b, const uint8_t* dev_c, int or_c, int batch,
                        int h, int w, uint8_t* dev_out, void* stream) {
  REQUIRE_ROBUST(e, dev_a && dev_out);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "mask join: shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  if (and_a < 0 || and_a > 255 || or_b < 0 || or_b > 255 || or_c < 0 || or_c > 255) return fail(e, UNETPP_E_UNSUPPORTED, "mask join: a bit mask outside 0..255");
  const size_t n = (size_t)batch * h * w;
  if (overlaps(dev_out, n, dev_a, n) || (dev_b && overlaps(dev_out, n, dev_b, n)) || (dev_c && overlaps(dev_out, n, dev_c, n)))
    return fail(e, UNETPP_E_UNSUPPORTED, "mask join: dev_out overlaps an input");
  const size_t blocks = (n + 4 * (size_t)SL_THREADS - 1) / (4 * (size_t)SL_THREADS);
  if (blocks > 0x7fffffffull) return fail(e, UNETPP_E_UNSUPPORTED, "mask join: too many pixels for one launch");
  ENTER_DEVICE(e);
  const int vec = n % 4 == 0 && ((uintptr_t)dev_a | (uintptr_t)dev_b | (uintptr_t)dev_c | (uintptr_t)dev_out) % 4 == 0;
  hipLaunchKernelGGL(sl_join_kernel, dim3((unsigned)blocks), dim3(SL_THREADS), 0, (hipStream_t)stream, dev_a, (unsigned)and_a, dev_b, (unsigned)or_b, dev_c,
                     (unsigned)or_c, (long long)n, vec, dev_out);
  return launched(e);
}

// ---- raw camera frames: the demosaic alone and fused into the resize (raw_frames.h, include/unetpp_raw.h) -----------------------------
static int raw_check(unetpp_engine* e, const char* what, int64_t row_stride, int64_t frame_stride, int batch, int h, int w, int pattern,
                     size_t* extent) {
  if (pattern < UNETPP_RAW_BG || pattern > UNETPP_RAW_MONO) return fail(e, UNETPP_E_UNSUPPORTED, "%s: unknown pattern %d", what, pattern);
  const ShapeLimits lim{pattern == UNETPP_RAW_MONO ? 1 : 3, MAX_DIM, true};
  if (!shape_ok(batch, h, w, lim))
    return fail(e, UNETPP_E_UNSUPPORTED, "%s: shape %dx%dx%d outside %d <= h, w <= 65535, h * w <= 2^30", what, batch, h, w, lim.min_side);
  const long long cap = 1ll << 40;                           // keeps every product below inside int64
  if (row_stride < w || row_stride > cap || frame_stride > cap || frame_stride < (long long)(h - 1) * row_stride + w)
    return fail(e, UNETPP_E_UNSUPPORTED, "%s: strides (%lld, %lld) do not hold rows of %d bytes and frames of %d rows", what, (long long)row_stride,
                (long long)frame_stride, w, h);
  *extent = (size_t)(batch - 1) * (size_t)frame_stride + (size_t)(h - 1) * (size_t)row_stride + (size_t)w;
  return UNETPP_OK;
}

int unetpp_raw_to_bgr_u8(unetpp_engine* e, const uint8_t* dev_raw, int64_t row_stride, int64_t frame_stride, int batch, int h, int w, int pattern,
                         uint8_t* dev_bgr, uint8_t* dev_gray, void* stream) {
  REQUIRE_ROBUST(e, dev_raw && (dev_bgr || dev_gray));
  size_t n_in = 0;
  if (int rc = raw_check(e, "raw to bgr", row_stride, frame_stride, batch, h, w, pattern, &n_in)) return rc;
  const size_t n = (size_t)batch * h * w;
  if ((dev_bgr && overlaps(dev_raw, n_in, dev_bgr, 3 * n)) || (dev_gray && overlaps(dev_raw, n_in, dev_gray, n)) ||
      (dev_bgr && dev_gray && overlaps(dev_bgr, 3 * n, dev_gray, n)))
    return fail(e, UNETPP_E_UNSUPPORTED, "raw to bgr: an output overlaps dev_raw or the other output");
  ENTER_DEVICE(e);
  const bool mono = pattern == UNETPP_RAW_MONO;
  const dim3 grid = tile_grid(mono ? w : w - 1, mono ? h : h - 1, RF_TW, RF_TH, batch);      // raw_frames.h: a Bayer frame's last tile takes the last column and row
  const int vec_in = (uintptr_t)dev_raw % 16 == 0 && row_stride % 16 == 0 && frame_stride % 16 == 0;
#define RF_LAUNCH(RY, RX, MONO)                                                                                                            \
  hipLaunchKernelGGL((rf_to_bgr_kernel<RY, RX, MONO>), grid, dim3(RF_THREADS), 0, (hipStream_t)stream, dev_raw, (long long)row_stride, \
                     (long long)frame_stride, h, w, vec_in, dev_bgr, dev_gray)
  switch (pattern) {
    case UNETPP_RAW_BG: RF_LAUNCH(0, 0, false); break;
    case UNETPP_RAW_GB: RF_LAUNCH(0, 1, false); break;
    case UNETPP_RAW_RG: RF_LAUNCH(1, 1, false); break;
    case UNETPP_RAW_GR: RF_LAUNCH(1, 0, false); break;
    default: RF_LAUNCH(0, 0, true); break;
  }
#undef RF_LAUNCH
  return launched(e);
}

int unetpp_raw_resize_u8(unetpp_engine* e, const uint8_t* dev_raw, int64_t row_stride, int64_t frame_stride, int batch, int h, int w, int pattern,
                         int x0, int y0, int cw, int ch, uint8_t* dev_out, int oh, int ow, void* stream) {
  REQUIRE_ROBUST(e, dev_raw && dev_out);
  size_t n_in = 0;
  if (int rc = raw_check(e, "raw resize", row_stride, frame_stride, batch, h, w, pattern, &n_in)) return rc;
  if (!shape_ok(batch, oh, ow, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "raw resize: output %dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", oh, ow);
  if (x0 < 0 || y0 < 0 || cw < 1 || ch < 1 || x0 > w - cw || y0 > h - ch)
    return fail(e, UNETPP_E_UNSUPPORTED, "raw resize: the crop (x %d, y %d, %d x %d) does not lie inside the %dx%d frame", x0, y0, cw, ch, h, w);
  if (overlaps(dev_raw, n_in, dev_out, (size_t)batch * oh * ow * 3)) return fail(e, UNETPP_E_UNSUPPORTED, "raw resize: dev_out overlaps dev_raw");
  ENTER_DEVICE(e);
  static const int red_site[5][2] = {{0, 0}, {0, 1}, {1, 1}, {1, 0}, {0, 0}};      // (row parity, column parity) by UNETPP_RAW_*
  hipLaunchKernelGGL(rf_resize_kernel, tile_grid(ow, oh, RF_OTW, RF_OTH, batch), dim3(RF_THREADS), 0, (hipStream_t)stream, dev_raw,
                     (long long)row_stride, (long long)frame_stride, h, w, red_site[pattern][0], red_site[pattern][1],
                     (int)(pattern == UNETPP_RAW_MONO), x0, y0, cw, ch, oh, ow, dev_out);
  return launched(e);
}

// ---- the two-stage loop's own steps: class masks with their sums, the overlay, the rotation (two_stage.h, include/unetpp_two_stage.h) --
int unetpp_two_stage_masks_u8(unetpp_engine* e, const uint8_t* dev_pred, int batch, int th, int tw, uint8_t* dev_cable, uint8_t* dev_tape, int fh,
                              int fw, int x1, int y1, int x2, int y2, int64_t* dev_counts, void* stream) {
#pragma clang fp contract(off)
  REQUIRE_ROBUST(e, dev_pred && dev_cable && dev_tape && dev_counts);
  if (!shape_ok(batch, th, tw, MASK_SHAPE) || !shape_ok(batch, fh, fw, MASK_SHAPE))
    return fail(e, UNETPP_E_UNSUPPORTED, "two-stage masks: shape %dx%dx%d -> %dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, th, tw, fh, fw);
  if (x1 < 0 || y1 < 0 || x2 < 0 || y2 < 0) return fail(e, UNETPP_E_UNSUPPORTED, "two-stage masks: negative ROI bound (%d, %d, %d, %d)", x1, y1, x2, y2);
  if ((uintptr_t)dev_counts % 8) return fail(e, UNETPP_E_UNSUPPORTED, "two-stage masks: dev_counts must be 8-byte aligned");
  const size_t n_in = (size_t)batch * th * tw, n = (size_t)batch * fh * fw, nc = (size_t)batch * 2 * sizeof(int64_t);
  if (overlaps(dev_cable, n, dev_tape, n) || overlaps(dev_pred, n_in, dev_cable, n) || overlaps(dev_pred, n_in, dev_tape, n) ||
      overlaps(dev_counts, nc, dev_pred, n_in) || overlaps(dev_counts, nc, dev_cable, n) || overlaps(dev_counts, nc, dev_tape, n))
    return fail(e, UNETPP_E_UNSUPPORTED, "two-stage masks: an output overlaps dev_pred or another output");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(e, hipMemsetAsync(dev_counts, 0, nc, s));
  const double ifx = 1.0 / ((double)fw / (double)tw), ify = 1.0 / ((double)fh / (double)th);      // resizeNN's inverse scales (nearest_table)
  hipLaunchKernelGGL(ts_masks_kernel, tile_grid(fw, fh, TS_MW, TS_MH, batch), dim3(TS_THREADS), 0, s, dev_pred, th, tw, fh, fw, ifx, ify, x1, y1,
                     x2, y2, dev_cable, dev_tape, (unsigned long long*)dev_counts);
  return launched(e);
}

int unetpp_two_stage_overlay_u8(unetpp_engine* e, const uint8_t* dev_frames, const uint8_t* dev_cable, const uint8_t* dev_tape,
                                const uint8_t* dev_burr, int batch, int h, int w, int x1, int y1, int x2, int y2, const uint8_t* dev_table,
                                uint8_t* dev_out, int64_t* dev_burr_count, void* stream) {
  REQUIRE_ROBUST(e, dev_frames && dev_cable && dev_tape && dev_burr && dev_table && dev_out && dev_burr_count);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "two-stage overlay: shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  if (x1 < 0 || y1 < 0 || x2 < 0 || y2 < 0) return fail(e, UNETPP_E_UNSUPPORTED, "two-stage overlay: negative ROI bound (%d, %d, %d, %d)", x1, y1, x2, y2);
  if ((uintptr_t)dev_burr_count % 8) return fail(e, UNETPP_E_UNSUPPORTED, "two-stage overlay: dev_burr_count must be 8-byte aligned");
  const size_t n = (size_t)batch * h * w, nc = (size_t)batch * sizeof(int64_t);
  const void* ins[5] = {dev_frames, dev_cable, dev_tape, dev_burr, dev_table};
  const size_t in_bytes[5] = {3 * n, n, n, n, (size_t)TS_OV_TABLE};
  for (int i = 0; i < 5; ++i)
    if (overlaps(dev_out, 3 * n, ins[i], in_bytes[i]) || overlaps(dev_burr_count, nc, ins[i], in_bytes[i]))
      return fail(e, UNETPP_E_UNSUPPORTED, "two-stage overlay: an output overlaps an input");
  if (overlaps(dev_out, 3 * n, dev_burr_count, nc)) return fail(e, UNETPP_E_UNSUPPORTED, "two-stage overlay: the outputs overlap");
  ENTER_DEVICE(e);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(e, hipMemsetAsync(dev_burr_count, 0, nc, s));
  const size_t spans = (3 * (size_t)h * w + 47 + 47) / 48;                   // the first span starts up to 47 bytes before the frame
  hipLaunchKernelGGL(ts_overlay_kernel, dim3((unsigned)((spans + TS_THREADS - 1) / TS_THREADS), (unsigned)batch), dim3(TS_THREADS), 0, s, dev_frames,
                     dev_cable, dev_tape, dev_burr, h, w, x1, y1, x2, y2, dev_table, dev_out, (unsigned long long*)dev_burr_count);
  return launched(e);
}

int unetpp_rotate_u8(unetpp_engine* e, const uint8_t* dev_in, int batch, int h, int w, int channels, int code, uint8_t* dev_out, void* stream) {
  REQUIRE_ROBUST(e, dev_in && dev_out);
  if (!shape_ok(batch, h, w, MASK_SHAPE)) return fail(e, UNETPP_E_UNSUPPORTED, "rotate: shape %dx%dx%d outside 1 <= h, w <= 65535, h * w <= 2^30", batch, h, w);
  if (channels != 1 && channels != 3) return fail(e, UNETPP_E_UNSUPPORTED, "rotate: %d channels, 1 or 3 are supported", channels);
  if (code < UNETPP_ROTATE_90_CW || code > UNETPP_ROTATE_90_CCW) return fail(e, UNETPP_E_UNSUPPORTED, "rotate: unknown code %d", code);
  const size_t n = (size_t)batch * h * w * channels;
  if (overlaps(dev_in, n, dev_out, n)) return fail(e, UNETPP_E_UNSUPPORTED, "rotate: dev_out overlaps dev_in");
  ENTER_DEVICE(e);
  const int oh = code == UNETPP_ROTATE_180 ? h : w, ow = code == UNETPP_ROTATE_180 ? w : h;
  const dim3 grid = tile_grid(ow, oh, TS_RT, TS_RT, batch);
  if (channels == 3) hipLaunchKernelGGL(ts_rotate_kernel<3>, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, dev_in, h, w, code, dev_out);
  else hipLaunchKernelGGL(ts_rotate_kernel<1>, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, dev_in, h, w, code, dev_out);
  return launched(e);
}

}  // extern "C"
