// unetpp_abi.hip — the engine and the model entry points of the C ABI (include/unetpp.h) of the MI355X-native U-Net
// inference paths: create / load_weights / forward* / status / profile / debug.  The post-processing entry points (mask
// statistics, components, edges, measurements, enhancement, morphology, resizes, tiling) live in unetpp_postproc.hip;
// abi_common.h is what the two files share.
//
// arch 0, NestedUNet (reference src/models/unetpp.py:104-119, eval mode):
//   x0_0 = CB(3,32)(x)            x1_0 = CB(32,64)(pool x0_0)     x2_0 = CB(64,128)(pool x1_0)
//   x3_0 = CB(128,256)(pool x2_0) x4_0 = CB(256,512)(pool x3_0)
//   x3_1 = CB(768,256)(cat[x3_0, up x4_0])   x2_2 = CB(384,128)(cat[x2_0, up x3_1])
//   x1_3 = CB(192,64)(cat[x1_0, up x2_2])    x0_4 = CB(96,32)(cat[x0_0, up x1_3])
//   out  = Conv1x1(32,C)(x0_4)  -> argmax / class masks (infer_two_stage_burr.py:299-304)
// arch 1, SimpleUNet (reference src/models/simple_unet.py:94-128):
//   enc1 = CR(3,64) CR(64,64)(x)        enc2 = CR CR(pool enc1) [128]   enc3 [256]   enc4 [512]
//   dec3 = CR CR(cat[ConvT(512,256)(enc4), enc3])   dec2 = CR CR(cat[ConvT(256,128)(dec3), enc2])
//   dec1 = CR CR(cat[ConvT(128,64)(dec2), enc1])    out = Conv1x1(64,C)(dec1)
// Both are executed from one op list (convert, conv3x3, upsample, convT, head) built in unetpp_create.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

#include "abi_common.h"
#include "aux_kernels.h"
#include "conv3x3_mfma.h"
#include "conv3x3_ws.h"
#include "convt2x2_mfma.h"
#include "tapmm_ws.h"
#include "ws_dbg_host.h"

using namespace unetpp;

namespace {

thread_local std::string g_create_error;

constexpr uint32_t BLOB_MAGIC = 0x50504e55u;  // 'UNPP'
constexpr uint32_t DS_BLOB_MAGIC = 0x53444e55u;  // 'UNDS': the deep-supervision heads (unetpp_load_ds_heads)
constexpr int BLOB_VERSION = 1;
const int NB[5] = {32, 64, 128, 256, 512};    // nb_filter, reference unetpp.py:49
const int SB[4] = {64, 128, 256, 512};        // SimpleUNet widths, simple_unet.py:32-57

struct Tensor {
  std::string name;
  size_t off = 0;   // byte offset inside one activation slot
  int C = 0;        // channels of an activation tensor; 0 = raw bytes (fp32 side tensors, split-K buffers)
  int lvl = 0;
  bool virt = false;   // named in the graph but never written (fused away): no storage
};

struct ConvLayer {
  std::string name;
  int cin_real = 0;   // channels the canonical weight has
  int cout = 0;
  int lvl = 0;
  int in = -1, in2 = -1, out = -1, pool = -1;   // tensor ids; in2: second source of the virtual concat
  bool do_pool = false;
  int zt = -1;                  // tensor id of the fp32 accumulator start values (tapmm_ws.h): K = skip channels only
  int y_t = -1, low_t = -1;     // tapmm: fp32 Y tensor and the low-res input it is computed from
  bool c0f = false;             // conv0_0.conv2 computing conv0_0.conv1 itself from the caller's input (conv3x3_ws.h, C0F)
  bool upf = false;             // in2 is the LOW-resolution tensor: the loader does the bilinear x2 itself (no `up` tensor)
  bool ws = false;              // runs in the wave-specialised kernel (conv3x3_ws.h), else the lock-step one: fixes the weight layout too
  bool uprows = false;          // fused upsample on low-resolution rows (conv3x3_ws_uprows_kernel): 32-channel weight tiles (NW = 1)
  size_t w_off = 0, b_off = 0;  // float offsets inside the canonical blob payload
  int KC = 16, NW = 1, MW = 2, WAVES = 8;
  int nchunks = 1;
  size_t wpk_bytes = 0;         // packed weights: Cout / BN channel tiles x nchunks slabs in the layout of the layer's kernel
  size_t wpk_at = 0, scale_at = 0, mult_at = 0, tapw_at = 0;   // byte offsets inside the arena (unetpp_engine::at)
};

struct ConvTLayer {
  std::string name;
  int cin = 0, cout = 0, lvl = 0;   // lvl = level of the INPUT (the output is one level up)
  int in = -1, out = -1;
  size_t w_off = 0, b_off = 0;
  size_t wpk_at = 0, scale_at = 0, mult_at = 0;   // byte offsets inside the arena
};

enum OpKind { OP_CONVERT, OP_CONV, OP_UP, OP_CONVT, OP_HEAD, OP_TAPMM, OP_UPSUM, OP_DS };
struct Op {
  OpKind kind;
  int idx = -1;            // conv / convT index, (OP_UP) source tensor id, or (OP_DS) deep-supervision output k = level
  int out = -1;            // OP_UP: destination tensor id; OP_HEAD, OP_DS: input tensor id
  bool fuse_head = false;  // OP_CONV: run the 1x1 head in this conv's epilogue when allowed
};

struct ProfRec {
  std::string name;
  double flops = 0, bytes = 0;
  int ev0 = -1, ev1 = -1;   // indices into the engine's event pool: launches on one stream are back to
                            // back, so a launch's start event is the previous launch's end event
  int plan[4] = {0, 0, 0, 0};   // persistent launches: grid, tiles (split shares counted), ksplit, rows per wave (unetpp_profile_plan)
};

}  // namespace

struct unetpp_engine : unetpp_engine_common {
  int P = 2;
  bool x8 = false;                // UNETPP_PREC_EXACT8: P = 2 records with 8-bit cross-term planes (conv3x3_ws.h)
  int mb = 1;
  int num_cus = 256;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  template <class T> T* at(size_t byte_off) const { return (T*)(arena + byte_off); }
  float* blob = nullptr;  // canonical fp32 blob payload on device (weights + biases)
  size_t blob_floats = 0;
  bool weights_loaded = false;
  std::vector<Tensor> tensors;
  std::vector<ConvLayer> convs;
  std::vector<ConvTLayer> convts;
  std::vector<Op> ops;
  int n_blob_layers = 0;          // header[4] of a matching blob
  int t_in8 = -1, t_head_in = -1;
  int head_cx = 32;
  size_t head_w_off = 0, head_b_off = 0;
  // profiling
  bool prof_on = false;
  std::vector<ProfRec> prof;
  int prof_used = 0;
  std::vector<hipEvent_t> evpool;
  int ev_used = 0;
  int prof_prev_ev = -1;          // end event of the previous launch on the same stream, -1 = none
  hipStream_t prof_prev_stream = nullptr;
  int last_b = 0, last_h = 0, last_w = 0;
  bool keep_all = false;   // debug: materialise the head's input and run the head as its own kernel
  // concurrent micro-batches: `nstreams` copies of the activation area, one internal stream each
  int nstreams = 1;
  size_t act_bytes = 0;          // size of one activation area (slot)
  size_t last_slot_off = 0;
  hipStream_t streams[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_start = nullptr, ev_done[4] = {nullptr, nullptr, nullptr, nullptr};
  half_t* c1w = nullptr;          // fused first block: conv0_0.conv1 as MFMA A fragments (conv0_pack_kernel)
  int c0f_conv1 = -1;             // index of conv0_0.conv1 in `convs` when the first block is fused, else -1
  unsigned* d_status = nullptr;   // sticky range flags (UNETPP_STATUS_*), one word inside the arena
  int ksplit_max = 16, ksplit_min_chunks = 4, ksplit_gate = 4;      // split-K of small launches (UNETPP_KSPLIT=max[,min chunks]; 1 = off)
  int t_kpart = -1, t_kcnt = -1;  // per slot: partial sums and arrival counters of the split tiles
  bool kcnt_dirty = false;        // a forward returned early: its split launches may have left counters behind
  // deep-supervision heads (unetpp_load_ds_heads): their own allocations, outside the arena
  float* ds_w = nullptr;          // the UNDS blob payload: ds3_1 weight + bias, ds2_2, ds1_3
  size_t ds_w_off[4] = {0, 0, 0, 0};      // float offset of output k's weight [C][NB[k]] (its bias follows)
  float* ds_scratch[4] = {nullptr, nullptr, nullptr, nullptr};   // per slot: fp32 low-res logits of outputs 1..3
  size_t ds_scr_off[4] = {0, 0, 0, 0};    // float offset of output k's [mb][C][max_h >> k][max_w >> k] in a slot's scratch
  bool ds_loaded = false;
};

namespace unetpp {

unetpp_engine_common* unetpp_common(unetpp_engine* e) { return e; }

int fail(unetpp_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e) e->err = buf; else g_create_error = buf;
  return code;
}

// The attribute is process-wide state of the HIP runtime and engines may be driven from several threads, so the
// bookkeeping is locked and the value is the same constant for everybody.
hipError_t allow_full_lds(const void* kernel, int device, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({device, kernel})) return hipSuccess;
  hipError_t st = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (st == hipSuccess) done.insert({device, kernel});
  return st;
}

}  // namespace unetpp

namespace {

// payload floats of the canonical blob and number of layers in it
size_t blob_payload_floats(int arch, int C, int cin, int* n_layers = nullptr) {
  size_t n = 0;
  int layers = 0;
  if (arch == UNETPP_ARCH_NESTED) {
    int ci[9] = {cin, NB[0], NB[1], NB[2], NB[3], NB[3] + NB[4], NB[2] + NB[3], NB[1] + NB[2], NB[0] + NB[1]};
    int co[9] = {NB[0], NB[1], NB[2], NB[3], NB[4], NB[3], NB[2], NB[1], NB[0]};
    for (int b = 0; b < 9; ++b) {
      n += (size_t)co[b] * ci[b] * 9 + co[b];
      n += (size_t)co[b] * co[b] * 9 + co[b];
      layers += 2;
    }
    n += (size_t)C * NB[0] + C;
    layers += 1;
  } else {
    for (int l = 0; l < 4; ++l) {          // enc1..enc4
      int ci = l == 0 ? cin : SB[l - 1];
      n += (size_t)SB[l] * ci * 9 + SB[l] + (size_t)SB[l] * SB[l] * 9 + SB[l];
      layers += 2;
    }
    for (int l = 2; l >= 0; --l) { n += (size_t)SB[l + 1] * SB[l] * 4 + SB[l]; layers += 1; }   // up3, up2, up1
    for (int l = 2; l >= 0; --l) {         // dec3, dec2, dec1
      n += (size_t)SB[l] * (2 * SB[l]) * 9 + SB[l] + (size_t)SB[l] * SB[l] * 9 + SB[l];
      layers += 2;
    }
    n += (size_t)C * SB[0] + C;
    layers += 1;
  }
  if (n_layers) *n_layers = layers;
  return n;
}

// ---- conv dispatch ---------------------------------------------------------------------------
struct LaunchCtx {      // per engine: one process may drive engines on several devices
  int device; int num_cus; int ksplit_max = 1, ksplit_min_chunks = 4, ksplit_gate = 4;
  int* plan = nullptr;      // profiling on: the launch's ProfRec::plan, else null
  void report(int grid, int tiles, int ks, int rows) const { if (plan) { plan[0] = grid; plan[1] = tiles; plan[2] = ks; plan[3] = rows; } }
};

template <int P, int KC, int NW, int MW, int WAVES, bool POOL, bool HEAD, bool UPF = false>
hipError_t launch_conv_k(const LaunchCtx& cx, const ConvArgs& a, hipStream_t s) {
  using C = ConvCfg<P, KC, NW, MW, WAVES, UPF>;
  const int lds = C::LDS_BYTES + lds_tail(a.Cout, HEAD ? a.head_C : 0).bytes;
  // persistent workgroups: as many as are resident at once, each walks tiles blockIdx, +grid, ...
  const int total = a.N * a.tiles_x * a.tiles_y * a.nct;
  const int per_cu = std::max(1, std::min(2, (160 * 1024) / lds));
  dim3 grid((unsigned)std::min(total, cx.num_cus * per_cu));
  cx.report((int)grid.x, total, 1, MW);
  auto k = conv3x3_bias_relu_kernel<P, KC, NW, MW, WAVES, POOL, HEAD, UPF>;
  hipError_t st = allow_full_lds((const void*)k, cx.device);
  if (st != hipSuccess) return st;
  hipLaunchKernelGGL(k, grid, dim3(C::NT), lds, s, a);
  return hipGetLastError();
}

// wave-specialised kernel (conv3x3_ws.h): 16-row tiles (Cout = 32) or 8-row tiles (Cout % 64 == 0), one persistent workgroup per CU
template <int P, bool POOL, bool HEAD, bool UPF, bool C0F = false, int NW = 1, int MW = 4, bool X8 = false, bool CAT2 = false>
hipError_t launch_ws_k(const LaunchCtx& cx, ConvArgs a, hipStream_t s, bool uprows = false) {
  using C = WsCfg<P, UPF, C0F, NW, MW, X8>;
  a.tiles_x = (a.W + C::TW - 1) / C::TW; a.tiles_y = (a.H + C::TH - 1) / C::TH; a.nct = a.Cout / C::BN;
  const int lds = C::LDS_BYTES + C::tail(a.Cout, HEAD ? a.head_C : 0, uprows).bytes;
  // Split-K plan (small batches): a layer with fewer tiles than a quarter of the CUs shares each tile's K-chunks among
  // `ksplit` workgroups -- the largest divisor of the chunk count that still leaves every workgroup four chunks and fits
  // the chip (measured at batch 1, 512x512: levels 3-4 gain 10-35 us per layer; two-way splits and two-chunk shares gain nothing:
  // a split launch costs its partials' round trip, ~10 us).
  // The plan depends on (batch, H, W) only; results of different plans differ in summation order (1e-7-class).
  const int tiles = a.N * a.tiles_x * a.tiles_y * a.nct;
  int ks = 1;
  if (!UPF && !C0F && !HEAD && a.kpart && a.kcnt && cx.ksplit_max > 1 && tiles * cx.ksplit_gate <= cx.num_cus)
    for (int d = 2; d <= cx.ksplit_max && tiles * d <= cx.num_cus && a.nchunks / d >= cx.ksplit_min_chunks; ++d)
      if (a.nchunks % d == 0 && !(a.pair9 && (a.nchunks / d) % 2)) ks = d;      // (pair9: whole chunk pairs per workgroup)
  a.ksplit = ks;
  const int total = tiles * ks;
  dim3 grid((unsigned)std::min(total, cx.num_cus));
  cx.report((int)grid.x, total, ks, MW);
  {      // the grid size in the kernel's tile-number radix (its workgroups step through the tiles by G)
    int t = (int)grid.x;
    a.gdec[0] = t % ks; t /= ks;
    a.gdec[1] = t % a.nct; t /= a.nct;
    a.gdec[2] = t % a.tiles_x; t /= a.tiles_x;
    a.gdec[3] = t % a.tiles_y;
    a.gdec[4] = t / a.tiles_y;
  }
  // split launches have a kernel of their own: everywhere else the share arithmetic, the partials and the counters are not
  // compiled (conv3x3_ws.h).  The plan above decides, nothing else: ks > 1 exactly when it did before.
  void (*k)(ConvArgs) = conv3x3_ws_kernel<P, POOL, HEAD, UPF, C0F, NW, MW, X8, CAT2>;
  if constexpr (!UPF && !C0F && !HEAD) {
    if (ks > 1) k = conv3x3_ws_splitk_kernel<P, POOL, NW, MW, X8, CAT2>;
  }
  // `exact`, fused upsample, 32 channels per workgroup: the up chunks on low-resolution rows (conv3x3_ws.h, UR); same tiles, same LDS,
  // same weights as the plain 1 x 4 kernel (a.nct = Cout / 32 channel tiles per pixel tile)
  if constexpr (P == 2 && UPF && !POOL && !HEAD && !C0F && NW == 1 && MW == 4 && !X8) {
    if (uprows) k = conv3x3_ws_uprows_kernel;
  }
  hipError_t st = allow_full_lds((const void*)k, cx.device);
  if (st != hipSuccess) return st;
  hipLaunchKernelGGL(k, grid, dim3(C::NT), lds, s, a);
  return hipGetLastError();
}

// The wave-specialised kernel of one launch, worked out once from the layer and the pass (ws_variant): the profile label is
// printed from it, launch_ws instantiates from it, and unetpp_create asks it whether every EXACT8 layer has a kernel.
struct WsVariant {
  bool pool, head, upf, c0f;
  bool cat2;        // two full-resolution sources
  bool uprows;      // conv3x3_ws_uprows_kernel: Cout / 32 channel tiles per 16-row pixel tile, weights packed to match (unetpp_create)
  int NW, MW;       // 1 x 4: 16-row tiles (Cout = 32, low rows); 2 x 2: 8-row tiles, two 32-channel blocks per consumer wave, Cout / 64 channel tiles
  bool valid;       // conv3x3_ws.h has this combination
};

// `head`: the 1x1 head runs in this launch's epilogue.  debug_keep_intermediates keeps the plain fused-upsample kernel reachable
// for conv0_4.conv1 (Cout = 32: one weight layout for both kernels), and for that layer only.
WsVariant ws_variant(int P, bool x8, const ConvLayer& L, bool head, bool keep_all) {
  const bool two = L.in2 >= 0, wide = L.cout >= 64 && L.cout % 64 == 0;
  WsVariant v{L.do_pool, head, L.upf, L.c0f, two && !L.upf, L.uprows && !(keep_all && L.cout == 32), wide ? 2 : 1, wide ? 2 : 4, false};
  if (P != 2 || (v.upf && (v.pool || head)) || (v.pool && head)) return v;
  if (v.uprows) {
    v.NW = 1; v.MW = 4;
    v.valid = !x8 && v.upf && !v.c0f && (L.cout == 32 || L.cout == 64);
  } else if (wide) {
    v.valid = !head && !v.c0f && !(v.pool && v.cat2);
  } else if (L.cout == 32 && !v.cat2) {
    v.valid = !v.c0f || (v.pool && !head && !v.upf && L.nchunks == 2);
  }
  return v;
}

// "<layer and what is fused into it>|<kernel and its full template argument list>", as rocprofv3 prints it (bench.py matches on
// it).  A split-K launch (conv3x3_ws_splitk_kernel, chosen in launch_ws_k) keeps the label of the unsplit kernel it stands for.
std::string ws_label(int P, bool x8, const ConvLayer& L, const WsVariant& v) {
  char lbl[160];
  auto tf = [](bool b) { return b ? "true" : "false"; };
  if (v.uprows) snprintf(lbl, sizeof lbl, "%s+up|conv3x3_ws_uprows_kernel", L.name.c_str());
  else snprintf(lbl, sizeof lbl, "%s%s%s%s|conv3x3_ws_kernel<%d, %s, %s, %s, %s, %d, %d, %s, %s>", v.c0f ? "input+conv0_0.conv1+" : "", L.name.c_str(),
                v.upf ? "+up" : "", v.head ? "+final+argmax" : "", P, tf(v.pool), tf(v.head), tf(v.upf), tf(v.c0f), v.NW, v.MW, tf(x8), tf(v.cat2));
  return lbl;
}

template <bool X8>
hipError_t launch_ws_x(const LaunchCtx& cx, const WsVariant& v, const ConvArgs& a, hipStream_t s) {
  if (!v.valid) return hipErrorInvalidValue;
#define CASE(pool_, head_, upf_, c0f_, nw, cat2_) \
  if (v.pool == pool_ && v.head == head_ && v.upf == upf_ && v.c0f == c0f_ && v.NW == nw && v.cat2 == cat2_) \
    return launch_ws_k<2, pool_, head_, upf_, c0f_, nw, 4 / nw, X8, cat2_>(cx, a, s, v.uprows);
  CASE(false, false, true, false, 2, false)
  CASE(true, false, false, false, 2, false)
  CASE(false, false, false, false, 2, true)
  CASE(false, false, false, false, 2, false)
  CASE(true, false, false, true, 1, false)
  CASE(false, false, true, false, 1, false)      // and, with v.uprows, its low-row sibling
  CASE(false, true, false, false, 1, false)
  CASE(true, false, false, false, 1, false)
  CASE(false, false, false, false, 1, false)
#undef CASE
  return hipErrorInvalidValue;
}

hipError_t launch_ws(const LaunchCtx& cx, bool x8, const WsVariant& v, const ConvArgs& a, hipStream_t s) {
  return x8 ? launch_ws_x<true>(cx, v, a, s) : launch_ws_x<false>(cx, v, a, s);
}

template <int P, int KC, int NW, int MW, int WAVES>
hipError_t launch_conv_cfg(const LaunchCtx& cx, const ConvArgs& a, bool pool, bool head, bool upf, hipStream_t s) {
  if (a.zinit) return hipErrorInvalidValue;     // accumulator start values (tapmm_ws.h): the wave-specialised kernel only
  if constexpr (P == 2) {      // exact: only SimpleUNet's two-source decoder convs run here, with nothing fused
    if (pool || head || upf) return hipErrorInvalidValue;
  } else {
    if constexpr (NW == 1 && MW == 2 && KC == 16) {      // fused upsample: built for the narrow full-resolution tiles
      if (upf) return (pool || head) ? hipErrorInvalidValue : launch_conv_k<P, KC, NW, MW, WAVES, false, false, true>(cx, a, s);
    }
    if (upf) return hipErrorInvalidValue;
    if constexpr (NW == 1) {
      if (head) return launch_conv_k<P, KC, NW, MW, WAVES, false, true>(cx, a, s);
    }
    if constexpr (MW == 2) {     // the fused 2x2 pool needs both rows of a window in one wave
      if (pool) return launch_conv_k<P, KC, NW, MW, WAVES, true, false>(cx, a, s);
    }
    if (pool) return hipErrorInvalidValue;
  }
  return launch_conv_k<P, KC, NW, MW, WAVES, false, false>(cx, a, s);
}

// `mw` = rows per wave: the layer's own (2: 16-row tiles) or 1 (8-row tiles, see small_grid_rows)
hipError_t launch_conv(const LaunchCtx& cx, int P, const ConvLayer& L, int mw, const ConvArgs& a, bool head, hipStream_t s) {
#define CASE(p, kc, nw, mw_, wv) \
  if (P == p && L.KC == kc && L.NW == nw && mw == mw_ && L.WAVES == wv) return launch_conv_cfg<p, kc, nw, mw_, wv>(cx, a, L.do_pool, head, L.upf, s);
  CASE(1, 16, 1, 2, 8)
  CASE(1, 32, 2, 2, 8)
  CASE(1, 16, 2, 2, 8)
  CASE(1, 16, 4, 2, 8)
  CASE(2, 16, 2, 2, 8)
  CASE(1, 16, 2, 1, 8)
  CASE(1, 32, 2, 1, 8)
  CASE(1, 16, 4, 1, 8)
  CASE(2, 16, 2, 1, 8)
#undef CASE
  return hipErrorInvalidValue;
}

// Small batches leave the deep layers with fewer 16x32-pixel tiles than the chip has CUs (B=1: 16 tiles at 32x32).
// Layers without a fused pool (its 2x2 window needs both rows in one wave) then run 8-row tiles: twice the
// workgroups, each with half the matrix work per K-chunk.  Every output is still accumulated chunk by chunk, tap by
// tap in the same order, so the result is bitwise the same whichever tile height ran (tested).
int small_grid_rows(const ConvLayer& L, int num_cus, int nb, int H, int W, bool head) {
  if (L.do_pool || head || L.upf || L.zt >= 0 || L.NW == 1 || L.MW != 2) return L.MW;
  const int tiles = nb * ((W + 31) / 32) * ((H + 15) / 16) * (L.cout / (32 * L.NW));
  return tiles < num_cus ? 1 : L.MW;
}

void choose_cfg(int P, int cin_tensor, ConvLayer& L) {
  L.MW = 2; L.WAVES = 8;
  if (P == 1) {
    if (L.cout == 32) { L.NW = 1; L.KC = 16; }     // 2 workgroups of 8 waves per CU (58 KB LDS each): measured best
    else if (L.cout == 64) { L.NW = 2; L.KC = (cin_tensor <= 16) ? 16 : 32; }
    else { L.NW = 4; L.KC = 16; }
  } else {
    L.KC = 16;
    L.NW = (L.cout == 32) ? 1 : 2;
  }
}

// Bytes of one K-chunk's weight slab as the layer's kernel reads it (0: no such kernel)
size_t slab_bytes(int P, bool x8, const ConvLayer& L) {
  if (L.ws && x8) return L.NW == 1 ? WsCfg<2, false, false, 1, 4, true>::SLAB_BYTES : WsCfg<2, false, false, 2, 2, true>::SLAB_BYTES;
  if (L.ws) return L.NW == 1 ? WsCfg<2, false, false, 1, 4>::SLAB_BYTES : WsCfg<2, false, false, 2, 2>::SLAB_BYTES;
#define CASE(p, kc, nw) \
  if (P == p && L.KC == kc && L.NW == nw) return ConvCfg<p, kc, nw, 2, 8>::SLAB_BYTES;
  CASE(1, 16, 1)
  CASE(1, 32, 2)
  CASE(1, 16, 2)
  CASE(1, 16, 4)
  CASE(2, 16, 2)
#undef CASE
  return 0;
}

struct Launcher {
  unetpp_engine* e;
  hipStream_t s;
  int rc = UNETPP_OK;
  int* plan = nullptr;      // inside run(), profiling on: where the launch writes its plan (LaunchCtx::plan)
  template <class F>
  void run(const std::string& name, double flops, double bytes, F&& f) {
    if (rc) return;
    ProfRec* r = nullptr;
    auto new_event = [&]() {
      if ((size_t)e->ev_used >= e->evpool.size()) {
        hipEvent_t ev = nullptr;
        hipError_t es = hipEventCreate(&ev);
        if (es != hipSuccess) { rc = fail(e, UNETPP_E_HIP, "hipEventCreate: %s", hipGetErrorString(es)); return -1; }
        e->evpool.push_back(ev);
      }
      return e->ev_used++;
    };
    if (e->prof_on) {
      if ((size_t)e->prof_used >= e->prof.size()) e->prof.push_back(ProfRec());
      r = &e->prof[e->prof_used++];
      r->name = name; r->flops = flops; r->bytes = bytes;
      std::fill(r->plan, r->plan + 4, 0);
      if (e->prof_prev_ev >= 0 && e->prof_prev_stream == s) {
        r->ev0 = e->prof_prev_ev;
      } else {
        r->ev0 = new_event();
        if (r->ev0 < 0) { --e->prof_used; return; }
        (void)hipEventRecord(e->evpool[r->ev0], s);
      }
    }
    plan = r ? r->plan : nullptr;
    hipError_t st = f();
    plan = nullptr;
    if (st == hipSuccess) st = hipGetLastError();
    if (r) {
      r->ev1 = new_event();
      if (r->ev1 < 0) { --e->prof_used; e->prof_prev_ev = -1; return; }
      (void)hipEventRecord(e->evpool[r->ev1], s);
      e->prof_prev_ev = r->ev1; e->prof_prev_stream = s;
    }
    if (st != hipSuccess) rc = fail(e, UNETPP_E_HIP, "launch %s: %s", name.c_str(), hipGetErrorString(st));
  }
};

// ---- graph construction ------------------------------------------------------------------------
struct Builder {
  unetpp_engine* e;
  size_t act = 0;     // bytes of one activation slot so far
  size_t off = 0;     // floats of the blob payload so far
  int tensor(const std::string& name, int C, int lvl, bool virt = false) {
    Tensor t;
    t.name = name; t.C = C; t.lvl = lvl; t.off = act; t.virt = virt;
    const unetpp_config& c = e->cfg;
    size_t px = (size_t)e->mb * (c.max_h >> lvl) * (c.max_w >> lvl);
    if (!virt) act += align_up(px * e->P * C * sizeof(half_t), 256);
    e->tensors.push_back(t);
    return (int)e->tensors.size() - 1;
  }
  int tensor_raw(const std::string& name, size_t bytes_per_px, int lvl) {      // e.g. an fp32 tensor
    Tensor t;
    t.name = name; t.C = 0; t.lvl = lvl; t.off = act;
    const unetpp_config& c = e->cfg;
    size_t px = (size_t)e->mb * (c.max_h >> lvl) * (c.max_w >> lvl);
    act += align_up(px * bytes_per_px, 256);
    e->tensors.push_back(t);
    return (int)e->tensors.size() - 1;
  }
  int conv(const std::string& name, int cin_real, int in, int in2, int out, bool pool_to = false, int pool = -1, bool emit_op = true) {
    ConvLayer L;
    L.name = name; L.cin_real = cin_real; L.in = in; L.in2 = in2; L.out = out; L.pool = pool; L.do_pool = pool_to;
    L.cout = e->tensors[out].C; L.lvl = e->tensors[out].lvl;
    L.w_off = off; off += (size_t)L.cout * cin_real * 9;
    L.b_off = off; off += L.cout;
    const int c0 = e->tensors[in].C, c1 = in2 >= 0 ? e->tensors[in2].C : 0;
    choose_cfg(e->P, c0 + c1, L);
    L.nchunks = (c0 + L.KC - 1) / L.KC + c1 / L.KC;
    e->convs.push_back(L);
    Op op; op.kind = OP_CONV; op.idx = (int)e->convs.size() - 1;
    if (emit_op) e->ops.push_back(op);
    return op.idx;
  }
  void convt(const std::string& name, int in, int out) {
    ConvTLayer T;
    T.name = name; T.in = in; T.out = out; T.cin = e->tensors[in].C; T.cout = e->tensors[out].C; T.lvl = e->tensors[in].lvl;
    T.w_off = off; off += (size_t)T.cin * T.cout * 4;
    T.b_off = off; off += T.cout;
    e->convts.push_back(T);
    Op op; op.kind = OP_CONVT; op.idx = (int)e->convts.size() - 1;
    e->ops.push_back(op);
  }
  void up(int src, int dst) { Op op; op.kind = OP_UP; op.idx = src; op.out = dst; e->ops.push_back(op); }
  // deep-supervision output k right after the op that completes its node: launches only when unetpp_forward_ds asks for it
  void ds(int k, int node) { Op op; op.kind = OP_DS; op.idx = k; op.out = node; e->ops.push_back(op); }
  void head(int in, int cx) {
    e->t_head_in = in; e->head_cx = cx;
    e->head_w_off = off; off += (size_t)e->cfg.num_classes * cx;
    e->head_b_off = off; off += e->cfg.num_classes;
    Op op; op.kind = OP_HEAD; op.out = in; e->ops.push_back(op);
  }
};

// The plan switches of the environment (include/unetpp.h), read once per unetpp_create.
struct PlanSwitches {
  int plan_cus = 0;                 // UNETPP_PLAN_CUS=n: plan every launch for n compute units instead of the device's own count; 0 = unset
  int ksplit_max = 16, ksplit_min_chunks = 4, ksplit_gate = 4;      // UNETPP_KSPLIT=max[,min chunks[,gate]]: split-K of small launches (unetpp_engine)
  const char* tapmm = "23";         // UNETPP_TAPMM=levels whose up channels are multiplied at low resolution, e.g. "" (off) or "123"
  const char* uprows = "01";        // UNETPP_UPROWS=levels of the low-row fused upsample, e.g. "0" (level 0 only) or "none"
};

int read_plan_switches(PlanSwitches* sw) {
  if (const char* pc = getenv("UNETPP_PLAN_CUS")) {
    char* end = nullptr;
    errno = 0;
    const long v = strtol(pc, &end, 10);
    if (end == pc || *end != '\0' || errno != 0 || v < 1 || v > (1 << 20))
      return fail(nullptr, UNETPP_E_INVALID, "UNETPP_PLAN_CUS='%s': a whole number of compute units >= 1 required", pc);
    sw->plan_cus = (int)v;
  }
  if (const char* k = getenv("UNETPP_KSPLIT")) {
    sw->ksplit_max = std::max(1, atoi(k));
    if (const char* c = strchr(k, ',')) {
      sw->ksplit_min_chunks = std::max(1, atoi(c + 1));
      if (const char* g2 = strchr(c + 1, ',')) sw->ksplit_gate = std::max(1, atoi(g2 + 1));      // split when tiles * gate <= CUs
    }
  }
  if (const char* tl = getenv("UNETPP_TAPMM")) sw->tapmm = tl;
  if (const char* ul = getenv("UNETPP_UPROWS")) sw->uprows = ul;
  return UNETPP_OK;
}

void build_nested(unetpp_engine* e, Builder& b, const PlanSwitches& sw) {
  // exact modes: the first ConvBlock runs as ONE launch from the caller's tensor (no input copy, no conv0_0.conv1 launch,
  // no x0_0a tensor): conv3x3_ws.h, C0F.
  const bool c0f = e->P == 2;
  if (!c0f) { Op cv; cv.kind = OP_CONVERT; e->ops.push_back(cv); }
  e->t_in8 = b.tensor("in8", 8, 0, c0f);            // fused first block: neither the fp16 input copy nor x0_0a exists
  int x[5], xa[5], pooled[4], up[4], d[4], da[4];
  for (int l = 0; l < 5; ++l) {
    char nm[32];
    snprintf(nm, sizeof nm, "x%d_0", l);
    xa[l] = b.tensor(std::string(nm) + "a", NB[l], l, c0f && l == 0);
    x[l] = b.tensor(nm, NB[l], l);
    if (l < 4) pooled[l] = b.tensor(std::string(nm) + "p", NB[l], l + 1);
    snprintf(nm, sizeof nm, "conv%d_0", l);
    const int c1 = b.conv(std::string(nm) + ".conv1", l == 0 ? 3 : NB[l - 1], l == 0 ? e->t_in8 : pooled[l - 1], -1, xa[l], false, -1,
                          !(c0f && l == 0));
    const int c2 = b.conv(std::string(nm) + ".conv2", NB[l], xa[l], -1, x[l], l < 4, l < 4 ? pooled[l] : -1);
    if (c0f && l == 0) { e->convs[c2].c0f = true; e->c0f_conv1 = c1; }
  }
  for (int l = 3; l >= 0; --l) {
    char nm[32], tn[32];
    snprintf(tn, sizeof tn, "x%d_%d", l, 4 - l);
    const int low = l == 3 ? x[4] : d[l + 1];
    // Levels 2-3 (exact modes): the up channels are multiplied at LOW resolution and interpolated afterwards
    // (tapmm_ws.h: half the flops of the layer); UNETPP_TAPMM=levels overrides (PlanSwitches).
    // (the GEMM's 128-wide virtual-channel tiles need 9 * Cout % 128 == 0: levels 2 and 3; at level 1 the fp32
    // side tensors would be 0.9 GB per step and the path measured slower anyway)
    const bool tapmm = e->P == 2 && l >= 1 && (9 * NB[l]) % TapmmCfg::TN == 0 && strchr(sw.tapmm, '0' + l) != nullptr;
    if (tapmm) {
      snprintf(nm, sizeof nm, "conv%d_%d", l, 4 - l);
      const int yt = b.tensor_raw(std::string(tn) + "y", (size_t)9 * NB[l] * 4, l + 1);
      const int zt = b.tensor_raw(std::string(tn) + "z", (size_t)NB[l] * 4, l);
      da[l] = b.tensor(std::string(tn) + "a", NB[l], l);
      d[l] = b.tensor(tn, NB[l], l);
      { Op op; op.kind = OP_TAPMM; op.idx = (int)e->convs.size(); e->ops.push_back(op); }     // the conv pushed next
      { Op op; op.kind = OP_UPSUM; op.idx = (int)e->convs.size(); e->ops.push_back(op); }
      const int ci = b.conv(std::string(nm) + ".conv1", NB[l] + NB[l + 1], x[l], -1, da[l]);
      ConvLayer& L = e->convs[ci];
      L.zt = zt; L.y_t = yt; L.low_t = low;
      L.nchunks = NB[l] / L.KC;                         // K over the skip channels only
      b.conv(std::string(nm) + ".conv2", NB[l], da[l], -1, d[l]);
      b.ds(l, d[l]);
      continue;
    }
    // Every other level of the exact modes, and level 0 of fast (Cout = 32: narrow tiles, HBM co-bound): the decoder
    // conv interpolates its `up` channels itself from the low-res tensor (conv3x3_ws.h / conv3x3_mfma.h, UPF) -- no
    // upsample launch, no `up` tensor.  Levels 1-3 of fast keep the separate upsample kernel.
    const bool upf = e->P == 2 || l == 0;
    if (!upf) up[l] = b.tensor(std::string(tn) + "u", NB[l + 1], l);
    da[l] = b.tensor(std::string(tn) + "a", NB[l], l);
    d[l] = b.tensor(tn, NB[l], l);
    if (!upf) b.up(low, up[l]);
    snprintf(nm, sizeof nm, "conv%d_%d", l, 4 - l);
    const int ci = b.conv(std::string(nm) + ".conv1", NB[l] + NB[l + 1], x[l], upf ? low : up[l], da[l]);     // cat([skip, up]) (unetpp.py:112-116)
    e->convs[ci].upf = upf;
    b.conv(std::string(nm) + ".conv2", NB[l], da[l], -1, d[l]);
    if (l == 0) e->ops.back().fuse_head = true;
    else b.ds(l, d[l]);
  }
  b.head(d[0], NB[0]);
}

void build_simple(unetpp_engine* e, Builder& b) {
  Op cv; cv.kind = OP_CONVERT; e->ops.push_back(cv);
  e->t_in8 = b.tensor("in8", 8, 0);
  int enc[4], enca[4], pooled[3];
  for (int l = 0; l < 4; ++l) {
    char nm[32];
    snprintf(nm, sizeof nm, "enc%d", l + 1);
    enca[l] = b.tensor(std::string(nm) + "a", SB[l], l);
    enc[l] = b.tensor(nm, SB[l], l);
    if (l < 3) pooled[l] = b.tensor(std::string(nm) + "p", SB[l], l + 1);
    b.conv(std::string(nm) + ".0", l == 0 ? 3 : SB[l - 1], l == 0 ? e->t_in8 : pooled[l - 1], -1, enca[l]);
    b.conv(std::string(nm) + ".2", SB[l], enca[l], -1, enc[l], l < 3, l < 3 ? pooled[l] : -1);
  }
  // The canonical blob follows the module DEFINITION order (enc*, up3, up2, up1, dec3, dec2, dec1, final) while
  // the forward interleaves up/dec: blob offsets are assigned here in definition order, ops in forward order.
  size_t up_w[3], up_b[3], dec_w[3][2], dec_b[3][2];
  size_t off = b.off;
  for (int l = 2; l >= 0; --l) { up_w[l] = off; off += (size_t)SB[l + 1] * SB[l] * 4; up_b[l] = off; off += SB[l]; }
  for (int l = 2; l >= 0; --l) {
    dec_w[l][0] = off; off += (size_t)SB[l] * 2 * SB[l] * 9; dec_b[l][0] = off; off += SB[l];
    dec_w[l][1] = off; off += (size_t)SB[l] * SB[l] * 9; dec_b[l][1] = off; off += SB[l];
  }
  int prev = enc[3];
  for (int l = 2; l >= 0; --l) {
    char nm[32];
    snprintf(nm, sizeof nm, "up%d", l + 1);
    int u = b.tensor(std::string(nm) + "t", SB[l], l);
    b.convt(nm, prev, u);
    e->convts.back().w_off = up_w[l]; e->convts.back().b_off = up_b[l];
    snprintf(nm, sizeof nm, "dec%d", l + 1);
    int da = b.tensor(std::string(nm) + "a", SB[l], l);
    int d = b.tensor(nm, SB[l], l);
    int c1 = b.conv(std::string(nm) + ".0", 2 * SB[l], u, enc[l], da);        // cat([up, enc]) (simple_unet.py:112,117,122)
    e->convs[c1].w_off = dec_w[l][0]; e->convs[c1].b_off = dec_b[l][0];
    int c2 = b.conv(std::string(nm) + ".2", SB[l], da, -1, d);
    e->convs[c2].w_off = dec_w[l][1]; e->convs[c2].b_off = dec_b[l][1];
    prev = d;
  }
  b.off = off;
  b.head(prev, SB[0]);
}

// ---- forward: one function per op kind ----------------------------------------------------------
// The engine's activation format as its kernels' template arguments: fast <1>, exact <2>, exact8 <2, true>; the heads count 1, 2, 3.
struct Prec {
  int P; bool x8;
  template <class K> K pick(K fast, K exact, K exact8) const { return x8 ? exact8 : P == 2 ? exact : fast; }
  const char* args() const { return pick("1", "2", "2, true"); }
  const char* head_args() const { return pick("1", "2", "3"); }
};

// One pass's share of the caller's input: where frame b0 starts, and what a launch that reads it loads per pixel.
struct InSlice { const char* raw; int format; double bytes_per_px; };
InSlice in_slice(const void* dev_input, int in_format, int b0, size_t hw) {
  const int bpp = in_format == UNETPP_IN_F32_NCHW ? 12 : 3;      // three fp32 planes, or one BGR byte triple
  return {(const char*)dev_input + (size_t)b0 * hw * bpp, in_format, (double)bpp};
}

// One pass's share of one unetpp_outputs: its five pointers moved to frame b0 (NULL stays NULL), and what the launch that
// writes them stores per pixel.  o == NULL: this output was not requested.
struct OutSlice {
  const unetpp_outputs* o = nullptr;      // rule and thresholds
  float* logits = nullptr; float* probs = nullptr;
  uint8_t* mask = nullptr; uint8_t* cable = nullptr; uint8_t* tape = nullptr;
  double bytes_per_px = 0;
};
OutSlice out_slice(const unetpp_outputs* o, int b0, int C, size_t hw) {
  OutSlice r;
  if (!o) return r;
  r.o = o;
  if (o->dev_logits) r.logits = o->dev_logits + (size_t)b0 * C * hw;
  if (o->dev_probs) r.probs = o->dev_probs + (size_t)b0 * C * hw;
  if (o->dev_mask) r.mask = o->dev_mask + (size_t)b0 * hw;
  if (o->dev_cable) r.cable = o->dev_cable + (size_t)b0 * hw;
  if (o->dev_tape) r.tape = o->dev_tape + (size_t)b0 * hw;
  r.bytes_per_px = (r.logits ? 4.0 * C : 0) + (r.probs ? 4.0 * C : 0) + (r.mask ? 1 : 0) + (r.cable ? 1 : 0) + (r.tape ? 1 : 0);
  return r;
}

// One micro-batch pass of forward_impl: frames b0 .. b0 + nb of the caller's batch, on stream s, in activation slot `slot`.
struct Pass {
  unetpp_engine* e;
  hipStream_t s;
  Launcher& lx;
  int nb, b0, h, w;
  int slot;
  size_t slot_off;
  InSlice in;
  OutSlice out[4];      // unetpp_forward_ds's outs[k]; out[0] is the final head's
  bool head_done = false;      // the head ran in the last conv's epilogue
#ifdef UNETPP_WS_DBG
  WsDbgPass dbg;
#endif
  half_t* tp(int id) const { return (half_t*)(e->arena + slot_off + e->tensors[id].off); }
};

// EXACT8: layers whose chunk count is even pair the ninth taps of consecutive chunks (conv3x3_ws.h); the split-K plan then
// only makes shares with an even number of chunks (launch_ws_k)
bool x8_pair9(const unetpp_engine* e, const ConvLayer& L) { return e->x8 && L.nchunks % 2 == 0; }

void run_convert(Pass& c) {
  unetpp_engine* e = c.e;
  const Prec prec{e->P, e->x8};
  const size_t total = (size_t)c.nb * c.h * c.w;
  const double bytes = (double)total * c.in.bytes_per_px + (double)total * e->P * 16;
  c.lx.run(std::string("convert_input|convert_input_kernel<") + prec.args() + ">", 0, bytes, [&] {
    hipLaunchKernelGGL(prec.pick(convert_input_kernel<1>, convert_input_kernel<2>, convert_input_kernel<2, true>), dim3((unsigned)((total + 255) / 256)),
                       dim3(256), 0, c.s, (const void*)c.in.raw, c.in.format, c.nb, c.h, c.w, c.tp(e->t_in8), e->d_status);
    return hipSuccess;
  });
}

void run_conv(Pass& c, const Op& op) {
  unetpp_engine* e = c.e;
  const ConvLayer& L = e->convs[op.idx];
  const int P = e->P, C = e->cfg.num_classes;
  const bool head = op.fuse_head && !e->keep_all && L.cout == 32;
  const OutSlice& o = c.out[0];
  ConvArgs a{};
  const int H = c.h >> L.lvl, W = c.w >> L.lvl;
  const Tensor& t0 = e->tensors[L.in];
  const int c1 = L.in2 >= 0 ? e->tensors[L.in2].C : 0;
  a.in0 = c.tp(L.in); a.in1 = L.in2 >= 0 ? c.tp(L.in2) : nullptr; a.C0 = t0.C; a.C1 = c1;
  a.wpk = e->at<half_t>(L.wpk_at); a.scale = e->at<float>(L.scale_at); a.bias = e->blob + L.b_off; a.out = c.tp(L.out);
  a.pool_out = L.do_pool ? c.tp(L.pool) : nullptr;
  a.N = c.nb; a.H = H; a.W = W; a.Cout = L.cout;
  a.status = e->d_status;
  a.zinit = L.zt >= 0 ? (const float*)c.tp(L.zt) : nullptr;
  if (e->t_kpart >= 0) { a.kpart = (float*)c.tp(e->t_kpart); a.kcnt = (unsigned*)c.tp(e->t_kcnt); }
  a.ksplit = 1;
  a.pair9 = x8_pair9(e, L) ? 1 : 0;
  if (L.c0f) {     // the first block reads the caller's tensor itself
    const ConvLayer& L1 = e->convs[e->c0f_conv1];
    a.raw_in = c.in.raw;
    a.raw_fmt = c.in.format == UNETPP_IN_F32_NCHW ? 0 : 1;
    a.c1w = e->c1w; a.c1_scale = e->at<float>(L1.scale_at); a.c1_bias = e->blob + L1.b_off;
  }
  const int mw = small_grid_rows(L, e->num_cus, c.nb, H, W, head);
  const int TH = L.WAVES * mw;
  a.tiles_x = (W + 31) / 32; a.tiles_y = (H + TH - 1) / TH;
  a.nct = L.cout / (32 * L.NW); a.nchunks = L.nchunks;
  double px = (double)c.nb * H * W;
  double flops = 2.0 * px * L.cout * (L.zt >= 0 ? t0.C : L.cin_real) * 9;
  double bytes = px * P * 2.0 * (t0.C + (L.upf ? c1 / 4.0 : c1) + (head ? 0 : L.cout)) + (L.do_pool ? px / 4 * P * 2.0 * L.cout : 0.0) + (double)L.cout * L.cin_real * 9 * 2.0 * P;
  if (L.zt >= 0) bytes += px * L.cout * 4.0 - (double)L.cout * (L.cin_real - t0.C) * 9 * 2.0 * P;
  if (L.c0f) {     // conv0_0.conv1 rides along: its flops, the raw input instead of x0_0a
    flops += 2.0 * px * 32 * 3 * 9;
    bytes += px * c.in.bytes_per_px - px * P * 2.0 * t0.C;
  }
  if (head) {
    a.head_w = e->blob + e->head_w_off; a.head_b = e->blob + e->head_b_off; a.head_C = C;
    a.logits = o.logits; a.mask = o.mask; a.cable = o.cable; a.tape = o.tape;
    a.probs = o.probs; a.rule = o.o->rule;
    a.t_cable = o.o->t_cable; a.t_tape = o.o->t_tape; a.bg_margin = o.o->bg_margin; a.ct_margin = o.o->ct_margin;
    flops += 2.0 * px * 32 * C;
    bytes += px * o.bytes_per_px;
    c.head_done = true;
  }
  const WsVariant v = ws_variant(P, e->x8, L, head, e->keep_all);
  std::string lbl;
  if (L.ws) {
    lbl = ws_label(P, e->x8, L, v);
  } else {
    char buf[160];
    auto tf = [](bool b) { return b ? "true" : "false"; };
    snprintf(buf, sizeof buf, "%s%s%s|conv3x3_bias_relu_kernel<%d, %d, %d, %d, %d, %s, %s, %s>", L.name.c_str(), L.upf ? "+up" : "", head ? "+final+argmax" : "",
             P, L.KC, L.NW, mw, L.WAVES, tf(L.do_pool), tf(head), tf(L.upf));
    lbl = buf;
  }
#ifdef UNETPP_WS_DBG
  ws_dbg_before_launch(c.dbg, a, L.name, c.s);
#endif
  c.lx.run(lbl, flops, bytes, [&] {
    return L.ws ? launch_ws(LaunchCtx{e->cfg.device, e->num_cus, e->ksplit_max, e->ksplit_min_chunks, e->ksplit_gate, c.lx.plan}, e->x8, v, a, c.s)
                : launch_conv(LaunchCtx{e->cfg.device, e->num_cus, 1, 4, 4, c.lx.plan}, P, L, mw, a, head, c.s);
  });
#ifdef UNETPP_WS_DBG
  ws_dbg_after_launch(c.dbg, a, L.name, L.ws, c.s);
#endif
}

void run_tapmm(Pass& c, const Op& op) {
  unetpp_engine* e = c.e;
  const ConvLayer& L = e->convs[op.idx];
  const int P = e->P, H = c.h >> L.lvl, W = c.w >> L.lvl;
  const int cup = L.cin_real - e->tensors[L.in].C;
  TapmmArgs t{};
  t.low = c.tp(L.low_t); t.wpk = e->at<half_t>(L.tapw_at); t.y = (float*)c.tp(L.y_t);
  t.N = c.nb; t.hw = (H >> 1) * (W >> 1); t.K = cup; t.Nv = 9 * L.cout;
#ifdef UNETPP_WS_DBG
  { const char* d = getenv("UNETPP_TAPMM_DBG"); t.dbg = d ? atoi(d) : 0; }
#endif
  const int tiles = c.nb * ((t.hw + TapmmCfg::TM - 1) / TapmmCfg::TM) * (t.Nv / TapmmCfg::TN);
  const double M = (double)c.nb * t.hw;
  char lbl[96];
  snprintf(lbl, sizeof lbl, "%s.up-gemm|tapmm_ws_kernel<%s>", L.name.c_str(), e->x8 ? "true" : "false");
  c.lx.run(lbl, 2.0 * M * cup * t.Nv, M * cup * 2.0 * P + M * t.Nv * 4.0 + (double)t.Nv * cup * 2.0 * P, [&] {
    auto k = e->x8 ? tapmm_ws_kernel<true> : tapmm_ws_kernel<false>;
    hipError_t st = allow_full_lds((const void*)k, e->cfg.device);
    if (st != hipSuccess) return st;
    const int grid = std::min(tiles, e->num_cus);
    if (c.lx.plan) { c.lx.plan[0] = grid; c.lx.plan[1] = tiles; c.lx.plan[2] = 1; c.lx.plan[3] = 0; }      // (a GEMM tile has no rows per wave)
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(TapmmCfg::NT), TapmmCfg::LDS_BYTES, c.s, t);
    return hipSuccess;
  });
}

void run_upsum(Pass& c, const Op& op) {
  unetpp_engine* e = c.e;
  const ConvLayer& L = e->convs[op.idx];
  const int H = c.h >> L.lvl, W = c.w >> L.lvl;
  UpsumArgs u{};
  u.y = (const float*)c.tp(L.y_t); u.z = (float*)c.tp(L.zt); u.N = c.nb; u.H = H; u.W = W; u.Cout = L.cout;
  unsigned blocks = (unsigned)(((W + UpsumCfg::TW - 1) / UpsumCfg::TW) * ((H + UpsumCfg::TH - 1) / UpsumCfg::TH) * (L.cout / 32) * c.nb);
  const double px = (double)c.nb * H * W;
  char lbl[96];
  const bool small = blocks <= (unsigned)e->num_cus;      // too few 16-row tiles for the chip: 4-row tiles
  if (small) blocks = (unsigned)(((W + 31) / 32) * ((H + 3) / 4) * (L.cout / 32) * c.nb);
  snprintf(lbl, sizeof lbl, "%s.up-sum|upsum_kernel<1, %d>", L.name.c_str(), small ? 4 : 16);
  c.lx.run(lbl, px * L.cout * 9 * 8.0, px / 4 * 9 * L.cout * 4.0 + px * L.cout * 4.0, [&] {
    if (small) hipLaunchKernelGGL((upsum_kernel<1, 4>), dim3(blocks), dim3(256), UpsumCfgT<4>::LDS_BYTES, c.s, u);
    else hipLaunchKernelGGL((upsum_kernel<1, 16>), dim3(blocks), dim3(256), UpsumCfg::LDS_BYTES, c.s, u);
    return hipSuccess;
  });
}

// fast only: the exact modes interpolate in the decoder conv's loader (UPF)
void run_up(Pass& c, const Op& op) {
  unetpp_engine* e = c.e;
  const Tensor& low = e->tensors[op.idx];
  const Tensor& dst = e->tensors[op.out];
  const int P = e->P, H = c.h >> dst.lvl, W = c.w >> dst.lvl;
  double px = (double)c.nb * H * W;
  double bytes = px * P * 2.0 * low.C + px / 4 * P * 2.0 * low.C;
  const int nseg = (W + UP_SEG - 1) / UP_SEG;
  const int seg_w = std::min(W, UP_SEG);
  const size_t up_lds = (size_t)3 * (seg_w / 2 + 2) * P * 32;      // staged low-res rows of one segment
  const int up_threads = seg_w * 2 * P >= 1024 ? 512 : (seg_w * 2 * P >= 256 ? 256 : 128);   // one item = both rows of a piece
  char nm[64];
  snprintf(nm, sizeof nm, "up%d|upsample2x_kernel<1>", dst.lvl);
  c.lx.run(nm, px * low.C * 8, bytes, [&] {
    if (P != 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsample2x_kernel<1>, dim3((unsigned)((H / 2) * nseg), (unsigned)(c.nb * (low.C / 16))), dim3(up_threads), up_lds, c.s, c.tp(op.idx), H, W, c.tp(op.out));
    return hipSuccess;
  });
}

void run_convt(Pass& c, const Op& op) {
  unetpp_engine* e = c.e;
  const ConvTLayer& T = e->convts[op.idx];
  const Prec prec{e->P, e->x8};
  const int P = e->P, H = c.h >> T.lvl, W = c.w >> T.lvl;
  ConvTArgs a{};
  a.in = c.tp(T.in); a.wpk = e->at<half_t>(T.wpk_at); a.scale = e->at<float>(T.scale_at); a.bias = e->blob + T.b_off; a.out = c.tp(T.out);
  a.N = c.nb; a.H = H; a.W = W; a.Cin = T.cin; a.Cout = T.cout;
  a.status = e->d_status;
  double px = (double)c.nb * H * W;
  double flops = 2.0 * px * T.cin * T.cout * 4;
  double bytes = px * P * 2.0 * (T.cin + 4.0 * T.cout) + 4.0 * T.cin * T.cout * 2.0 * P;
  dim3 grid((unsigned)(((H * W + 511) / 512) * (4 * T.cout / 64) * c.nb));
  c.lx.run(T.name + "|convt2x2_kernel<" + prec.args() + ">", flops, bytes, [&] {
    hipLaunchKernelGGL(prec.pick(convt2x2_kernel<1>, convt2x2_kernel<2>, convt2x2_kernel<2, true>), grid, dim3(256), 0, c.s, a);
    return hipSuccess;
  });
}

// unetpp_forward_ds: output k of this node, when requested
void run_ds(Pass& c, const Op& op) {
  unetpp_engine* e = c.e;
  const Prec prec{e->P, e->x8};
  const int k = op.idx, C = e->cfg.num_classes, P = e->P, h = c.h, w = c.w;
  const OutSlice& o = c.out[k];
  if (!o.o) return;
  const int cx = e->tensors[op.out].C, hk = h >> k, wk = w >> k;
  const double lowpx = (double)c.nb * hk * wk, px = (double)c.nb * h * w;
  const float* dsw = e->ds_w + e->ds_w_off[k];
  const char* nm = k == 3 ? "ds3_1" : k == 2 ? "ds2_2" : "ds1_3";
  // 1. the 1x1 conv at the node's resolution, fp32 logits only, into the slot's scratch
  float* low = e->ds_scratch[c.slot] + e->ds_scr_off[k];
  const dim3 hgrid((unsigned)((hk * wk + 255) / 256), (unsigned)c.nb);
  const size_t lds = (size_t)(C * cx + C) * sizeof(float);
  c.lx.run(std::string(nm) + "|head_generic_kernel<" + prec.head_args() + ">", 2.0 * lowpx * cx * C, lowpx * (P * 2.0 * cx + 4.0 * C), [&] {
    uint8_t* none = nullptr;
    hipLaunchKernelGGL(prec.pick(head_generic_kernel<1>, head_generic_kernel<2>, head_generic_kernel<3>), hgrid, dim3(256), lds, c.s, c.tp(op.out), cx, dsw,
                       dsw + (size_t)C * cx, C, hk, wk, low, (float*)nullptr, none, none, none, 0, 0.f, 0.f, 0.f, 0.f);
    return hipSuccess;
  });
  // 2. one bilinear step to (h, w) + the head epilogue; ATen's scale, float(in - 1) / float(out - 1)
  const float sy = (float)(hk - 1) / (float)(h - 1), sx = (float)(wk - 1) / (float)(w - 1);
  const size_t items = (size_t)c.nb * h * (w / 4);
  c.lx.run(std::string(nm) + "+up|ds_upsample_kernel", px * C * 9.0, lowpx * 4.0 * C + px * o.bytes_per_px, [&] {
    hipLaunchKernelGGL(ds_upsample_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, c.s, (const float*)low, C, hk, wk, c.nb, h, w, sy, sx,
                       o.logits, o.probs, o.mask, o.cable, o.tape, o.o->rule, o.o->t_cable, o.o->t_tape, o.o->bg_margin, o.o->ct_margin);
    return hipSuccess;
  });
}

void run_head(Pass& c, const Op& op) {
  if (c.head_done) return;     // ran in the last conv's epilogue
  unetpp_engine* e = c.e;
  const Prec prec{e->P, e->x8};
  const OutSlice& o = c.out[0];
  const int cx = e->head_cx, C = e->cfg.num_classes;
  const size_t hw = (size_t)c.h * c.w, total = c.nb * hw;
  const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)c.nb);
  const size_t lds = (size_t)(C * cx + C) * sizeof(float);
  c.lx.run(std::string("final+argmax|head_generic_kernel<") + prec.head_args() + ">", 2.0 * total * cx * C, (double)total * (e->P * 2.0 * cx + o.bytes_per_px), [&] {
    hipLaunchKernelGGL(prec.pick(head_generic_kernel<1>, head_generic_kernel<2>, head_generic_kernel<3>), grid, dim3(256), lds, c.s, c.tp(op.out), cx,
                       e->blob + e->head_w_off, e->blob + e->head_b_off, C, c.h, c.w, o.logits, o.probs, o.mask, o.cable, o.tape, o.o->rule, o.o->t_cable,
                       o.o->t_tape, o.o->bg_margin, o.o->ct_margin);
    return hipSuccess;
  });
}

}  // namespace

extern "C" {

#ifndef UNETPP_SRC_HASH
#define UNETPP_SRC_HASH "unknown"
#endif
// "src:<hash>" = digest of the sources this binary was built from (unet-_amd/_lib.py compares it with the tree)
#ifdef UNETPP_WS_DBG
#define UNETPP_BUILD_TAG " +wsdbg"      /* measurement build (phase ablations): unet-_amd/_lib.py refuses it unless asked */
#else
#define UNETPP_BUILD_TAG ""
#endif
const char* unetpp_version(void) { return "unetpp-hip 0.3.0 (gfx950) src:" UNETPP_SRC_HASH UNETPP_BUILD_TAG; }

const char* unetpp_last_error(const unetpp_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

size_t unetpp_weights_blob_bytes(int num_classes, int in_channels) {
  return 32 + 4 * blob_payload_floats(UNETPP_ARCH_NESTED, num_classes, in_channels);
}

size_t unetpp_weights_blob_bytes_arch(int arch, int num_classes, int in_channels) {
  if (arch != UNETPP_ARCH_NESTED && arch != UNETPP_ARCH_SIMPLE) return 0;
  return 32 + 4 * blob_payload_floats(arch, num_classes, in_channels);
}

int unetpp_create(const unetpp_config* cfg, unetpp_engine** out) {
  if (!cfg || !out) return fail(nullptr, UNETPP_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->arch != UNETPP_ARCH_NESTED && cfg->arch != UNETPP_ARCH_SIMPLE) return fail(nullptr, UNETPP_E_INVALID, "arch=%d unknown", cfg->arch);
  if (cfg->in_channels != 3) return fail(nullptr, UNETPP_E_UNSUPPORTED, "input_channels=%d unsupported (only 3)", cfg->in_channels);
  if (cfg->num_classes < 1 || cfg->num_classes > HEAD_FUSED_MAX_CLASSES)
    return fail(nullptr, UNETPP_E_INVALID, "num_classes=%d out of range [1,%d]", cfg->num_classes, HEAD_FUSED_MAX_CLASSES);
  const int mult = cfg->arch == UNETPP_ARCH_NESTED ? 16 : 8;      // 4 resp. 3 poolings
  if (cfg->max_batch < 1 || cfg->max_h < mult || cfg->max_w < mult || cfg->max_h % mult || cfg->max_w % mult)
    return fail(nullptr, UNETPP_E_INVALID, "max shape (%d,%d,%d): batch>=1 and H,W positive multiples of %d required",
                cfg->max_batch, cfg->max_h, cfg->max_w, mult);
  if (cfg->precision != UNETPP_PREC_EXACT && cfg->precision != UNETPP_PREC_FAST && cfg->precision != UNETPP_PREC_EXACT8)
    return fail(nullptr, UNETPP_E_INVALID, "precision=%d unknown", cfg->precision);
  // the conv loader addresses one image of one tensor with 32-bit byte offsets (buffer loads): the largest
  // full-resolution tensor has 64 channels x (1 or 2) fp16 planes
  if ((double)cfg->max_h * cfg->max_w * 64 * 2 * (cfg->precision == UNETPP_PREC_FAST ? 1 : 2) >= 2147483648.0)
    return fail(nullptr, UNETPP_E_UNSUPPORTED, "max shape %dx%d too large for 32-bit tensor offsets", cfg->max_h, cfg->max_w);
  PlanSwitches sw;
  if (const int rc = read_plan_switches(&sw)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, UNETPP_E_HIP, "no HIP device available: this engine has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, UNETPP_E_INVALID, "device %d not in [0,%d)", cfg->device, ndev);
  DeviceScope dev_scope(cfg->device);
  if (dev_scope.st != hipSuccess) return fail(nullptr, UNETPP_E_HIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(dev_scope.st));

  // the one owner of the engine until it is handed to the caller: every early return below frees whatever exists by then
  struct Destroy { void operator()(unetpp_engine* p) const { unetpp_destroy(p); } };
  std::unique_ptr<unetpp_engine, Destroy> owner(new unetpp_engine());
  unetpp_engine* e = owner.get();
  e->cfg = *cfg;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) e->num_cus = prop.multiProcessorCount;
  }
  if (sw.plan_cus > 0) {      // only ever smaller launches than the device's own plan: never a grid that is not resident at once
    if (sw.plan_cus > e->num_cus)
      return fail(nullptr, UNETPP_E_INVALID, "UNETPP_PLAN_CUS=%d exceeds the device's %d compute units", sw.plan_cus, e->num_cus);
    e->num_cus = sw.plan_cus;
  }
  e->ksplit_max = sw.ksplit_max; e->ksplit_min_chunks = sw.ksplit_min_chunks; e->ksplit_gate = sw.ksplit_gate;
  e->P = cfg->precision == UNETPP_PREC_FAST ? 1 : 2;
  e->x8 = cfg->precision == UNETPP_PREC_EXACT8;
  e->mb = (cfg->micro_batch > 0 && cfg->micro_batch < cfg->max_batch) ? cfg->micro_batch : cfg->max_batch;
  e->nstreams = std::max(1, std::min(4, cfg->streams));
  if (e->mb >= cfg->max_batch) e->nstreams = 1;      // a single pass has nothing to overlap with
  const int P = e->P;

  Builder b{e};
  if (cfg->arch == UNETPP_ARCH_NESTED) build_nested(e, b, sw); else build_simple(e, b);
  // The kernel of every conv, fixed here for the engine's lifetime (it also decides the weight layout, see repack): in the
  // exact modes the wave-specialised one, except SimpleUNet's two-source decoder convs in exact, which stay on the
  // lock-step kernel (same speed, and results that do not depend on a split-K plan: DESIGN.md 5.6); fast: lock-step.
  for (ConvLayer& L : e->convs) L.ws = P == 2 && (L.in2 < 0 || L.upf || e->x8);
  // `exact`, fused upsample with at least two skip chunks, Cout = 32 or 64 (conv0_4.conv1, conv1_3.conv1): the kernel that multiplies
  // the up chunks on low-resolution rows, 32 output channels per workgroup -- Cout = 64 runs as two channel tiles per pixel tile, so
  // its weights are packed in 32-channel slabs (NW = 1; L.MW x L.WAVES stays the 16-row tile).  Cout >= 128 would repeat halo and
  // interpolation four to eight times per pixel tile and stays on the 2 x 2 kernel.  UNETPP_UPROWS=levels overrides (PlanSwitches).
  for (ConvLayer& L : e->convs) {
    if (!L.ws || !L.upf || P != 2 || e->x8 || (L.cout != 32 && L.cout != 64) || L.lvl > 9) continue;
    const int c0 = e->tensors[L.in].C, c1 = e->tensors[L.in2].C;
    if (c0 < 32 || c0 % 16 || c1 < 16 || c1 % 16 || strchr(sw.uprows, '0' + L.lvl) == nullptr) continue;
    L.uprows = true;
    L.NW = 1;
  }
  if (e->x8)      // EXACT8 exists in the wave-specialised kernel only: every conv must have a variant there (ws_variant)
    for (const ConvLayer& L : e->convs)
      if (!L.ws || !ws_variant(P, true, L, false, false).valid)
        return fail(nullptr, UNETPP_E_UNSUPPORTED, "internal: %s has no EXACT8 kernel", L.name.c_str());
  if (P == 2 && e->ksplit_max > 1) {
    // at most num_cus workgroups take part in a split launch, each with 4 consumer waves x 16 KB of raw accumulators
    e->t_kpart = (int)e->tensors.size();
    { Tensor t; t.name = "ksplit.partials"; t.off = b.act; e->tensors.push_back(t); b.act += align_up((size_t)e->num_cus * 4 * 16384, 256); }
    e->t_kcnt = (int)e->tensors.size();
    { Tensor t; t.name = "ksplit.counters"; t.off = b.act; e->tensors.push_back(t); b.act += align_up((size_t)e->num_cus * 4 * sizeof(unsigned), 256); }
  }
  e->blob_floats = b.off;
  if (b.off != blob_payload_floats(cfg->arch, cfg->num_classes, 3, &e->n_blob_layers))
    return fail(nullptr, UNETPP_E_STATE, "internal: blob size mismatch");
  e->act_bytes = align_up(b.act, 4096);

  // ---- behind the activation slots, in the same arena: blob, packed weights and scales, each offset kept with its layer
  Carve arena{e->act_bytes * e->nstreams};
  const size_t blob_at = arena.take(b.off * sizeof(float));
  for (ConvLayer& L : e->convs) {
    L.wpk_bytes = (size_t)(L.cout / (32 * L.NW)) * L.nchunks * slab_bytes(P, e->x8, L);
    L.wpk_at = arena.take(L.wpk_bytes);
    L.scale_at = arena.take(L.cout * sizeof(float));
    L.mult_at = arena.take(L.cout * sizeof(float));
  }
  for (ConvLayer& L : e->convs)
    if (L.zt >= 0) L.tapw_at = arena.take((size_t)9 * L.cout * (L.cin_real - e->tensors[L.in].C) * P * sizeof(half_t));
  for (ConvTLayer& T : e->convts) {
    T.wpk_at = arena.take((size_t)4 * T.cout * T.cin * P * sizeof(half_t));
    T.scale_at = arena.take(T.cout * sizeof(float));
    T.mult_at = arena.take(T.cout * sizeof(float));
  }
  const size_t c1w_at = arena.take(4096);
  const size_t status_at = arena.take(256);
  const size_t total = arena.end;
  hipError_t st = hipMalloc((void**)&e->arena, total);
  if (st == hipSuccess) st = hipMemset(e->arena + status_at, 0, 256);
  if (st != hipSuccess) return fail(nullptr, UNETPP_E_HIP, "hipMalloc(%zu bytes): %s", total, hipGetErrorString(st));
  e->arena_bytes = total;
  if (e->t_kcnt >= 0)
    for (int i = 0; i < e->nstreams; ++i)
      (void)hipMemset(e->arena + (size_t)i * e->act_bytes + e->tensors[e->t_kcnt].off, 0, (size_t)e->num_cus * 4 * sizeof(unsigned));
  e->d_status = e->at<unsigned>(status_at);
  e->c1w = e->at<half_t>(c1w_at);
  e->blob = e->at<float>(blob_at);
  if (e->nstreams > 1) {
    hipError_t se = hipSuccess;
    for (int i = 0; i < e->nstreams && se == hipSuccess; ++i) {
      se = hipStreamCreateWithFlags(&e->streams[i], hipStreamNonBlocking);
      if (se == hipSuccess) se = hipEventCreateWithFlags(&e->ev_done[i], hipEventDisableTiming);
    }
    if (se == hipSuccess) se = hipEventCreateWithFlags(&e->ev_start, hipEventDisableTiming);
    if (se != hipSuccess) return fail(nullptr, UNETPP_E_HIP, "stream/event creation: %s", hipGetErrorString(se));
  }
  *out = owner.release();
  return UNETPP_OK;
}

void unetpp_destroy(unetpp_engine* e) {
  if (!e) return;
  DeviceScope dev_scope(e->cfg.device);
  for (auto ev : e->evpool) (void)hipEventDestroy(ev);
  for (int i = 0; i < 4; ++i) { if (e->streams[i]) (void)hipStreamDestroy(e->streams[i]); if (e->ev_done[i]) (void)hipEventDestroy(e->ev_done[i]); }
  if (e->ev_start) (void)hipEventDestroy(e->ev_start);
  if (e->arena) (void)hipFree(e->arena);
  for (auto& kv : e->resize_tabs) (void)hipFree(kv.second);
  if (e->ds_w) (void)hipFree(e->ds_w);
  for (float* p : e->ds_scratch) if (p) (void)hipFree(p);
  delete e;
}

size_t unetpp_workspace_bytes(const unetpp_engine* e) { return e ? e->arena_bytes : 0; }

static int repack(unetpp_engine* e, hipStream_t s) {
  const int P = e->P;
  for (auto& L : e->convs) {
    const float* w = e->blob + L.w_off;
    float* mult = e->at<float>(L.mult_at);
    hipLaunchKernelGGL(weight_scale_kernel, dim3(L.cout), dim3(256), 0, s, w, L.cin_real * 9, e->blob + L.b_off, mult, e->at<float>(L.scale_at), e->d_status);
    const int BN = 32 * L.NW;
    const long long units = (long long)(L.wpk_bytes / 16);      // one thread per 16 bytes of packed weights
    if (e->x8) {
      if ((int)(&L - &e->convs[0]) == e->c0f_conv1) continue;      // conv0_0.conv1 runs in the producers (conv0_pack_kernel below)
      hipLaunchKernelGGL(weight_pack_x8_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, w, mult, L.cin_real, L.cout, BN,
                         L.nchunks, e->at<char>(L.wpk_at), units, x8_pair9(e, L) ? 1 : 0);
      continue;
    }
    hipLaunchKernelGGL(weight_pack_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, w, mult, L.cin_real,
                       L.cout, P, L.KC, BN, L.nchunks, e->at<half_t>(L.wpk_at), units, L.ws ? 1 : 0);
  }
  for (auto& L : e->convs) {
    if (L.zt < 0) continue;
    const int cs = e->tensors[L.in].C, cup = L.cin_real - cs;
    const long long units = (long long)9 * L.cout * cup * P / 8;
    hipLaunchKernelGGL(tapw_pack_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, e->blob + L.w_off, e->at<float>(L.mult_at), L.cout, cs,
                       cup, e->at<half_t>(L.tapw_at), units, e->x8 ? 1 : 0);
  }
  if (e->c0f_conv1 >= 0) {
    const ConvLayer& L1 = e->convs[e->c0f_conv1];
    hipLaunchKernelGGL(conv0_pack_kernel, dim3(1), dim3(256), 0, s, e->blob + L1.w_off, e->at<float>(L1.mult_at), e->c1w);
  }
  for (auto& T : e->convts) {
    const float* w = e->blob + T.w_off;
    float* mult = e->at<float>(T.mult_at);
    hipLaunchKernelGGL(convt_scale_kernel, dim3(T.cout), dim3(256), 0, s, w, T.cin, T.cout, e->blob + T.b_off, mult, e->at<float>(T.scale_at), e->d_status);
    long long units = (long long)(4 * T.cout / 32) * (T.cin / 16) * P * 64;
    hipLaunchKernelGGL(convt_pack_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, w, mult, T.cin, T.cout, P,
                       e->at<half_t>(T.wpk_at), units);
  }
  HIP_TRY(e, hipGetLastError());
  e->weights_loaded = true;
  return UNETPP_OK;
}

static int check_header(unetpp_engine* e, const uint32_t* h, size_t bytes) {
  const size_t want = unetpp_weights_blob_bytes_arch(e->cfg.arch, e->cfg.num_classes, e->cfg.in_channels);
  if (bytes != want)
    return fail(e, UNETPP_E_INVALID, "weight blob is %zu bytes, expected %zu for arch=%d num_classes=%d", bytes, want, e->cfg.arch,
                e->cfg.num_classes);
  if (h[0] != BLOB_MAGIC || (int)h[1] != BLOB_VERSION) return fail(e, UNETPP_E_INVALID, "bad weight blob magic/version");
  if ((int)h[2] != e->cfg.num_classes || (int)h[3] != e->cfg.in_channels || (int)h[4] != e->n_blob_layers || (int)h[5] != e->cfg.arch)
    return fail(e, UNETPP_E_INVALID, "weight blob is for num_classes=%u in_channels=%u layers=%u arch=%u", h[2], h[3], h[4], h[5]);
  return UNETPP_OK;
}

int unetpp_load_weights(unetpp_engine* e, const void* host_blob, size_t bytes) {
  if (!e || !host_blob) return fail(e, UNETPP_E_INVALID, "null argument");
  ENTER_DEVICE(e);
  if (bytes < 32) return fail(e, UNETPP_E_INVALID, "weight blob too small");
  int rc = check_header(e, (const uint32_t*)host_blob, bytes);
  if (rc) return rc;
  e->ds_loaded = false;      // the deep-supervision heads belong to the previous checkpoint: load them again
  HIP_TRY(e, hipMemcpy(e->blob, (const char*)host_blob + 32, bytes - 32, hipMemcpyHostToDevice));
  rc = repack(e, nullptr);
  if (rc) return rc;
  HIP_TRY(e, hipDeviceSynchronize());
  return UNETPP_OK;
}

int unetpp_load_weights_device(unetpp_engine* e, const void* dev_blob, size_t bytes, void* stream) {
  if (!e || !dev_blob) return fail(e, UNETPP_E_INVALID, "null argument");
  ENTER_DEVICE(e);
  if (bytes < 32) return fail(e, UNETPP_E_INVALID, "weight blob too small");
  uint32_t h[8];
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(e, hipMemcpyAsync(h, dev_blob, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  int rc = check_header(e, h, bytes);
  if (rc) return rc;
  e->ds_loaded = false;      // as in unetpp_load_weights
  HIP_TRY(e, hipMemcpyAsync(e->blob, (const char*)dev_blob + 32, bytes - 32, hipMemcpyDeviceToDevice, s));
  return repack(e, s);
}

// ---- forward -------------------------------------------------------------------------------------
int unetpp_forward(unetpp_engine* e, const void* dev_input, int in_format, int batch, int h, int w, float* dev_logits,
                   uint8_t* dev_mask, uint8_t* dev_cable, uint8_t* dev_tape, void* stream) {
  unetpp_outputs o{};
  o.dev_logits = dev_logits; o.dev_mask = dev_mask; o.dev_cable = dev_cable; o.dev_tape = dev_tape;
  o.rule = UNETPP_RULE_ARGMAX;
  return unetpp_forward_ex(e, dev_input, in_format, batch, h, w, &o, stream);
}

static int check_rule(unetpp_engine* e, const unetpp_outputs* o) {
  if (o->rule < UNETPP_RULE_ARGMAX || o->rule > UNETPP_RULE_EXCLUSIVE) return fail(e, UNETPP_E_INVALID, "unknown rule %d", o->rule);
  if (o->rule != UNETPP_RULE_ARGMAX && e->cfg.num_classes < 3)
    return fail(e, UNETPP_E_INVALID, "class rules need num_classes >= 3 (bg, cable, tape)");
  return UNETPP_OK;
}

// One forward of unetpp_forward_ex (outs = {out, NULL, NULL, NULL}: every op, the same launches) or unetpp_forward_ds.
// outs[k != 0] launches output k's head and interpolation at its OP_DS; without outs[0] the op list is cut after the
// last requested OP_DS (the shallowest requested level), so deeper decoder levels never run.
static int forward_impl(unetpp_engine* e, const void* dev_input, int in_format, int batch, int h, int w,
                        const unetpp_outputs* const outs[4], void* stream) {
  static const unetpp_outputs no_outputs{};      // out[0] of a pass that was asked for deep-supervision outputs only
  size_t n_ops = e->ops.size();
  if (!outs[0])
    for (size_t i = 0; i < e->ops.size(); ++i)
      if (e->ops[i].kind == OP_DS && outs[e->ops[i].idx]) n_ops = i + 1;
  if (!dev_input) return fail(e, UNETPP_E_INVALID, "input is NULL");
  if (!e->weights_loaded) return fail(e, UNETPP_E_STATE, "forward before load_weights");
  if (in_format != UNETPP_IN_F32_NCHW && in_format != UNETPP_IN_U8_NHWC_BGR) return fail(e, UNETPP_E_INVALID, "unknown input format %d", in_format);
  if (batch < 1 || batch > e->cfg.max_batch) return fail(e, UNETPP_E_INVALID, "batch %d not in [1,%d]", batch, e->cfg.max_batch);
  const int mult = e->cfg.arch == UNETPP_ARCH_NESTED ? 16 : 8;
  if (h < mult || w < mult || h % mult || w % mult)
    return fail(e, UNETPP_E_INVALID, "Sizes of tensors must match: H=%d W=%d must be positive multiples of %d", h, w, mult);
  if (h > e->cfg.max_h || w > e->cfg.max_w) return fail(e, UNETPP_E_INVALID, "shape %dx%d exceeds engine maximum %dx%d", h, w, e->cfg.max_h, e->cfg.max_w);
  ENTER_DEVICE(e);
  hipStream_t user_stream = (hipStream_t)stream;
  const bool multi = e->nstreams > 1 && batch > e->mb;
  // join: the caller's stream continues after every internal stream has drained.  It runs on EVERY exit after the
  // fork, failures included: the caller may free or reuse its output buffers on its stream right after an error
  // return, and kernels already queued on the internal streams still write to them.
  struct Join {
    unetpp_engine* e; hipStream_t user; bool armed = false;
    hipError_t run() {
      if (!armed) return hipSuccess;
      armed = false;
      hipError_t first = hipSuccess;
      for (int i = 0; i < e->nstreams; ++i) {
        hipError_t r = hipEventRecord(e->ev_done[i], e->streams[i]);
        if (r == hipSuccess) r = hipStreamWaitEvent(user, e->ev_done[i], 0);
        if (r != hipSuccess) { (void)hipStreamSynchronize(e->streams[i]); if (first == hipSuccess) first = r; }
      }
      return first;
    }
    ~Join() { (void)run(); }
  } join{e, user_stream};
  if (multi) {   // fork: the internal streams start after everything already queued on the caller's stream
    HIP_TRY(e, hipEventRecord(e->ev_start, user_stream));
    join.armed = true;
    for (int i = 0; i < e->nstreams; ++i) HIP_TRY(e, hipStreamWaitEvent(e->streams[i], e->ev_start, 0));
  }
  e->last_b = batch; e->last_h = h; e->last_w = w;
  // The last arriver of every split tile puts its counter back to zero, so a completed forward leaves them clean; after a
  // forward that failed half-way they are cleared here (stream-ordered, before the first launch).
  if (e->t_kcnt >= 0 && e->kcnt_dirty)
    for (int i = 0; i < e->nstreams; ++i)
      HIP_TRY(e, hipMemsetAsync(e->arena + (size_t)i * e->act_bytes + e->tensors[e->t_kcnt].off, 0, (size_t)e->num_cus * 4 * sizeof(unsigned),
                                multi ? e->streams[i] : user_stream));
  e->kcnt_dirty = true;
  Launcher Lx{e, user_stream};
  int pass = 0;
  e->prof_prev_ev = -1;     // other work may sit between two forwards: start a fresh event chain
  const size_t hw = (size_t)h * w;

  for (int b0 = 0; b0 < batch; b0 += e->mb, ++pass) {
    const int slot = multi ? pass % e->nstreams : 0;
    if (multi) Lx.s = e->streams[slot];
    Pass c{e, Lx.s, Lx, std::min(e->mb, batch - b0), b0, h, w, slot, (size_t)slot * e->act_bytes, in_slice(dev_input, in_format, b0, hw)};
    c.out[0] = out_slice(outs[0] ? outs[0] : &no_outputs, b0, e->cfg.num_classes, hw);
    for (int k = 1; k < 4; ++k) c.out[k] = out_slice(outs[k], b0, e->cfg.num_classes, hw);
    e->last_slot_off = c.slot_off;
    for (size_t oi = 0; oi < n_ops; ++oi) {
      const Op& op = e->ops[oi];
      switch (op.kind) {
        case OP_CONVERT: run_convert(c); break;
        case OP_CONV: run_conv(c, op); break;
        case OP_TAPMM: run_tapmm(c, op); break;
        case OP_UPSUM: run_upsum(c, op); break;
        case OP_UP: run_up(c, op); break;
        case OP_CONVT: run_convt(c, op); break;
        case OP_DS: run_ds(c, op); break;
        case OP_HEAD: run_head(c, op); break;
      }
    }
    if (Lx.rc) return Lx.rc;
#ifdef UNETPP_WS_DBG
    ws_dbg_end_of_pass(c.dbg, c.s);
#endif
  }
  HIP_TRY(e, join.run());
  e->kcnt_dirty = Lx.rc != UNETPP_OK;
  return Lx.rc;
}

int unetpp_forward_ex(unetpp_engine* e, const void* dev_input, int in_format, int batch, int h, int w,
                      const unetpp_outputs* outp, void* stream) {
  if (!e) return UNETPP_E_INVALID;
  if (!outp) return fail(e, UNETPP_E_INVALID, "outputs is NULL");
  const int rc = check_rule(e, outp);
  if (rc) return rc;
  const unetpp_outputs* const outs[4] = {outp, nullptr, nullptr, nullptr};
  return forward_impl(e, dev_input, in_format, batch, h, w, outs, stream);
}

// ---- deep-supervision outputs -------------------------------------------------------------------------
static size_t ds_payload_floats(int C) { return (size_t)C * (NB[3] + NB[2] + NB[1]) + 3 * (size_t)C; }

size_t unetpp_ds_blob_bytes(int num_classes) { return num_classes < 1 ? 0 : 32 + 4 * ds_payload_floats(num_classes); }

int unetpp_load_ds_heads(unetpp_engine* e, const void* host_blob, size_t bytes) {
  if (!e || !host_blob) return fail(e, UNETPP_E_INVALID, "null argument");
  if (e->cfg.arch != UNETPP_ARCH_NESTED) return fail(e, UNETPP_E_UNSUPPORTED, "deep-supervision heads exist for NestedUNet only");
  const int C = e->cfg.num_classes;
  const size_t want = unetpp_ds_blob_bytes(C);
  if (bytes != want) return fail(e, UNETPP_E_INVALID, "ds blob is %zu bytes, expected %zu for num_classes=%d", bytes, want, C);
  const uint32_t* hd = (const uint32_t*)host_blob;
  if (hd[0] != DS_BLOB_MAGIC || (int)hd[1] != BLOB_VERSION) return fail(e, UNETPP_E_INVALID, "bad ds blob magic/version");
  if ((int)hd[2] != C || (int)hd[3] != e->cfg.in_channels)
    return fail(e, UNETPP_E_INVALID, "ds blob is for num_classes=%u in_channels=%u", hd[2], hd[3]);
  ENTER_DEVICE(e);
  size_t off = 0, per_slot = 0;
  for (int k = 3; k >= 1; --k) { e->ds_w_off[k] = off; off += (size_t)C * NB[k] + C; }        // definition order: ds3_1, ds2_2, ds1_3
  for (int k = 1; k <= 3; ++k) { e->ds_scr_off[k] = per_slot; per_slot += (size_t)e->mb * C * (e->cfg.max_h >> k) * (e->cfg.max_w >> k); }
  for (int i = 0; i < e->nstreams; ++i)
    if (!e->ds_scratch[i]) HIP_TRY(e, hipMalloc((void**)&e->ds_scratch[i], per_slot * sizeof(float)));
  const size_t nf = ds_payload_floats(C);
  if (!e->ds_w) HIP_TRY(e, hipMalloc((void**)&e->ds_w, nf * sizeof(float)));
  e->ds_loaded = false;
  HIP_TRY(e, hipMemcpy(e->ds_w, (const char*)host_blob + 32, nf * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(nonfinite_flag_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, nullptr, (const float*)e->ds_w, (int)nf, e->d_status);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipDeviceSynchronize());
  e->ds_loaded = true;
  return UNETPP_OK;
}

int unetpp_forward_ds(unetpp_engine* e, const void* dev_input, int in_format, int batch, int h, int w,
                      const unetpp_outputs* const outs[4], void* stream) {
  if (!e) return UNETPP_E_INVALID;
  if (e->cfg.arch != UNETPP_ARCH_NESTED) return fail(e, UNETPP_E_UNSUPPORTED, "deep-supervision outputs exist for NestedUNet only");
  if (!outs || (!outs[0] && !outs[1] && !outs[2] && !outs[3])) return fail(e, UNETPP_E_INVALID, "no output requested");
  for (int k = 0; k < 4; ++k)
    if (outs[k]) { const int rc = check_rule(e, outs[k]); if (rc) return rc; }
  for (int k = 1; k < 4; ++k) {      // ds_upsample_kernel stores 4 pixels at once: 16 bytes of fp32, 4 bytes of a mask
    if (!outs[k]) continue;
    const unetpp_outputs& o = *outs[k];
    if (((uintptr_t)o.dev_logits | (uintptr_t)o.dev_probs) % 16 || ((uintptr_t)o.dev_mask | (uintptr_t)o.dev_cable | (uintptr_t)o.dev_tape) % 4)
      return fail(e, UNETPP_E_INVALID, "outs[%d]: logits / probs must be 16-byte aligned, masks 4-byte aligned", k);
  }
  if (!e->ds_loaded && (outs[1] || outs[2] || outs[3]))
    return fail(e, UNETPP_E_STATE, "deep-supervision output requested before unetpp_load_ds_heads");
  return forward_impl(e, dev_input, in_format, batch, h, w, outs, stream);
}

int unetpp_status(unetpp_engine* e, uint32_t* flags, int clear) {
  if (!e) return UNETPP_E_INVALID;
  if (!flags) return fail(e, UNETPP_E_INVALID, "flags is NULL");
  ENTER_DEVICE(e);
  HIP_TRY(e, hipDeviceSynchronize());      // every forward queued so far has set its bits
  unsigned v = 0;
  HIP_TRY(e, hipMemcpy(&v, e->d_status, sizeof v, hipMemcpyDeviceToHost));
  if (clear && v) HIP_TRY(e, hipMemset(e->d_status, 0, sizeof v));
  *flags = v;
  return UNETPP_OK;
}

// ---- profiling -------------------------------------------------------------------------------------
int unetpp_profile_enable(unetpp_engine* e, int on) {
  if (!e) return UNETPP_E_INVALID;
  e->prof_on = on != 0;
  e->prof_used = 0;
  e->ev_used = 0;
  e->prof_prev_ev = -1;
  return UNETPP_OK;
}
int unetpp_profile_count(const unetpp_engine* e) { return e ? e->prof_used : 0; }
int unetpp_profile_read(unetpp_engine* e, float* ms_out, int n) {
  if (!e || !ms_out) return UNETPP_E_INVALID;
  ENTER_DEVICE(e);
  int m = std::min(n, e->prof_used);
  for (int i = 0; i < m; ++i) {
    HIP_TRY(e, hipEventSynchronize(e->evpool[e->prof[i].ev1]));
    HIP_TRY(e, hipEventElapsedTime(&ms_out[i], e->evpool[e->prof[i].ev0], e->evpool[e->prof[i].ev1]));
  }
  return m;
}
const char* unetpp_profile_name(const unetpp_engine* e, int i) {
  if (!e || i < 0 || i >= e->prof_used) return "";
  return e->prof[i].name.c_str();
}
int unetpp_profile_work(const unetpp_engine* e, int i, double* flops, double* bytes) {
  if (!e || i < 0 || i >= e->prof_used) return UNETPP_E_INVALID;
  if (flops) *flops = e->prof[i].flops;
  if (bytes) *bytes = e->prof[i].bytes;
  return UNETPP_OK;
}
int unetpp_profile_plan(const unetpp_engine* e, int i, int out[4]) {
  if (!e || !out || i < 0 || i >= e->prof_used) return UNETPP_E_INVALID;
  std::copy(e->prof[i].plan, e->prof[i].plan + 4, out);
  return UNETPP_OK;
}

// ---- debug -------------------------------------------------------------------------------------
int unetpp_debug_keep_intermediates(unetpp_engine* e, int on) {
  if (!e) return UNETPP_E_INVALID;
  e->keep_all = on != 0;
  return UNETPP_OK;
}

long long unetpp_debug_read(unetpp_engine* e, const char* name, float* host_out, size_t max_floats) {
  if (!e || !name || !host_out) return UNETPP_E_INVALID;
  if (e->last_b == 0) return fail(e, UNETPP_E_STATE, "debug_read before forward");
  const Tensor* t = nullptr;
  int tid = -1;
  // "name#hi", "name#lo", "name#x8": one stored plane instead of the reconstructed value (see unpack_nchw_kernel)
  std::string base(name);
  int plane = 0;
  if (size_t hash = base.find('#'); hash != std::string::npos) {
    const std::string sel = base.substr(hash + 1);
    base.resize(hash);
    plane = sel == "hi" ? 1 : sel == "lo" ? 2 : sel == "x8" ? 3 : -1;
    if (plane < 0 || (plane == 3 && !e->x8) || (plane == 2 && e->P != 2))
      return fail(e, UNETPP_E_INVALID, "plane '%s' does not exist in this engine's activation format", sel.c_str());
  }
  for (size_t i = 0; i < e->tensors.size(); ++i)
    if (e->tensors[i].name == base) { t = &e->tensors[i]; tid = (int)i; }
  if (!t) return fail(e, UNETPP_E_INVALID, "unknown tensor '%s'", base.c_str());
  if (t->virt) return fail(e, UNETPP_E_STATE, "'%s' is never materialised on this engine (fused into its consumer)", name);
  if (t->C == 0) return fail(e, UNETPP_E_STATE, "'%s' is not an activation tensor (raw fp32 / bookkeeping buffer)", name);
  if (e->cfg.arch == UNETPP_ARCH_NESTED && tid == e->t_head_in && !e->keep_all)
    return fail(e, UNETPP_E_STATE, "x0_4 is not materialised (head fused): call unetpp_debug_keep_intermediates(e, 1) before forward");
  ENTER_DEVICE(e);
  int nb = e->last_b % e->mb == 0 ? std::min(e->mb, e->last_b) : e->last_b % e->mb;
  const int H = e->last_h >> t->lvl, W = e->last_w >> t->lvl;
  size_t total = (size_t)nb * t->C * H * W;
  if (total > max_floats) return fail(e, UNETPP_E_INVALID, "buffer too small: need %zu floats", total);
  float* tmp = nullptr;
  HIP_TRY(e, hipDeviceSynchronize());
  HIP_TRY(e, hipMalloc((void**)&tmp, total * sizeof(float)));
  const half_t* src = (const half_t*)(e->arena + e->last_slot_off + t->off);
  if (e->x8) hipLaunchKernelGGL(unpack_nchw_kernel<3>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, src, nb, t->C, H, W, tmp, plane);
  else if (e->P == 2) hipLaunchKernelGGL(unpack_nchw_kernel<2>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, src, nb, t->C, H, W, tmp, plane);
  else hipLaunchKernelGGL(unpack_nchw_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, src, nb, t->C, H, W, tmp, plane);
  hipError_t st = hipMemcpy(host_out, tmp, total * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(tmp);
  if (st != hipSuccess) return fail(e, UNETPP_E_HIP, "debug copy: %s", hipGetErrorString(st));
  return (long long)total;
}

}  // extern "C"
