// abi_common.h — host only: what the library's two translation units share.  unetpp_abi.hip holds the engine and the model
// entry points and defines the functions declared here; unetpp_postproc.hip holds the post-processing entry points and sees
// no more of an engine than unetpp_engine_common.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <map>
#include <string>
#include <tuple>

#include "../../include/unetpp.h"

// shared between the two files, not with the world: the dynamic symbol table holds the C ABI and nothing else
#define UNETPP_HIDDEN __attribute__((visibility("hidden")))

struct unetpp_engine_common {
  unetpp_config cfg{};
  std::string err;
  // frame glue: per-axis resize tables on the device, keyed by (kind, n_src, n_dst); kind 0 = linear, 1 = nearest,
  // 2 = linear with float coefficients.  unetpp_destroy frees them.
  std::map<std::tuple<int, int, int>, void*> resize_tabs;
};

namespace unetpp {

UNETPP_HIDDEN unetpp_engine_common* unetpp_common(unetpp_engine* e);      // e is not NULL
// Records the message in the engine, with e == NULL as the calling thread's create error, and returns `code`.
UNETPP_HIDDEN int fail(unetpp_engine* e, int code, const char* fmt, ...);
// For kernels that take more dynamic LDS than the 64 KiB default: raises the limit once per (device, kernel).
UNETPP_HIDDEN hipError_t allow_full_lds(const void* kernel, int device, int bytes = 160 * 1024);

#define HIP_TRY(e, call)                                                                       \
  do {                                                                                         \
    hipError_t _s = (call);                                                                    \
    if (_s != hipSuccess) return fail(e, UNETPP_E_HIP, "%s: %s", #call, hipGetErrorString(_s)); \
  } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Hands out the byte offsets of a workspace's parts in order, each on a 256-byte boundary; `end` is the total so far.
struct Carve {
  size_t end = 0;
  size_t take(size_t bytes) { const size_t at = end; end = align_up(end + bytes, 256); return at; }
};

// Every entry point runs with the engine's device current and puts the caller's device back on return, so that a
// single-process multi-GPU program (torch, another engine) is not redirected by a call into this library.
struct UNETPP_HIDDEN DeviceScope {
  int prev = -1;
  bool switched = false;
  hipError_t st = hipSuccess;
  explicit DeviceScope(int dev) {
    st = hipGetDevice(&prev);
    if (st == hipSuccess && prev != dev) { st = hipSetDevice(dev); switched = st == hipSuccess; }
  }
  ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};
#define ENTER_DEVICE(e)                                    \
  DeviceScope _dev_scope(unetpp_common(e)->cfg.device);    \
  if (_dev_scope.st != hipSuccess)                         \
    return fail(e, UNETPP_E_HIP, "hipSetDevice(%d): %s", unetpp_common(e)->cfg.device, hipGetErrorString(_dev_scope.st))

}  // namespace unetpp
