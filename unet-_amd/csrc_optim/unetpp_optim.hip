// libunetpp_optim_hip.so: the entry points of include/optim/unetpp_optim.h.  Host side only: argument checks, the chunk
// plan (a function of n alone) and the two launches; the kernels are in optim_kernels.h.
#include "optim_kernels.h"

#ifndef UNETPP_OPTIM_SRC_HASH
#define UNETPP_OPTIM_SRC_HASH "unknown"
#endif

namespace {

enum { E_INVALID = -1, E_UNSUPPORTED = -2, E_HIP = -3 };           // the values of UNETPP_E_*

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int launched() { return hipGetLastError() == hipSuccess ? 0 : E_HIP; }

// the groups and arguments of a step as the kernels may rely on them
int check_step(int64_t n, const unetpp_optim_groups& G, const unetpp_optim_step_args& A, const float* m, const float* v) {
  if (n < 1 || n > optim::MAX_N) return E_UNSUPPORTED;
  if (G.n_groups < 1 || G.n_groups > UNETPP_OPTIM_MAX_GROUPS) return E_UNSUPPORTED;
  if (G.kind != UNETPP_OPTIM_ADAM && G.kind != UNETPP_OPTIM_ADAMW && G.kind != UNETPP_OPTIM_SGD) return E_UNSUPPORTED;
  int64_t prev = 0;
  for (int k = 0; k < G.n_groups; ++k) {
    if (G.end[k] <= prev) return E_UNSUPPORTED;
    prev = G.end[k];
    if (G.kind == UNETPP_OPTIM_SGD && (float)G.momentum[k] != 0.0f && !m) return E_INVALID;
  }
  if (prev != n) return E_UNSUPPORTED;
  if (G.kind != UNETPP_OPTIM_SGD && (!m || !v)) return E_INVALID;
  if ((A.parity != 0 && A.parity != 1) || (A.scaler_parity != 0 && A.scaler_parity != 1)) return E_UNSUPPORTED;
  return 0;
}

template <int KIND>
void launch_step(bool vec, dim3 grid, hipStream_t s, float* p, float* g, float* m, float* v, int64_t n, long long chunk, int parts,
                 const double* partial, const uint32_t* flag, const unetpp_optim_groups& G, const unetpp_optim_step_args& A,
                 uint32_t* state, uint32_t* scaler) {
  if (vec)
    hipLaunchKernelGGL((optim::step_kernel<KIND, true>), grid, dim3(optim::THREADS), 0, s, p, g, m, v, (long long)n, chunk, parts,
                       partial, flag, G, A, state, scaler);
  else
    hipLaunchKernelGGL((optim::step_kernel<KIND, false>), grid, dim3(optim::THREADS), 0, s, p, g, m, v, (long long)n, chunk, parts,
                       partial, flag, G, A, state, scaler);
}

}  // namespace

extern "C" {

int unetpp_optim_layout(int* granule, int* max_partials, int* state_slot_words, int* max_groups) {
  if (!granule || !max_partials || !state_slot_words || !max_groups) return E_INVALID;
  *granule = optim::GRANULE;
  *max_partials = optim::MAX_PARTIALS;
  *state_slot_words = optim::SLOT_WORDS;
  *max_groups = UNETPP_OPTIM_MAX_GROUPS;
  return 0;
}

size_t unetpp_optim_workspace_bytes(int64_t n) {
  if (n < 1 || n > optim::MAX_N) return 0;
  return (size_t)optim::parts_of(n) * (sizeof(double) + sizeof(uint32_t));
}

const char* unetpp_optim_version(void) { return "unetpp-optim-hip 0.1.0 (gfx950) osrc:" UNETPP_OPTIM_SRC_HASH; }

int unetpp_optim_grad_norm_f32(const float* dev_grad, int64_t n, void* dev_workspace, void* stream) {
  if (!dev_grad || !dev_workspace) return E_INVALID;
  if (n < 1 || n > optim::MAX_N || !aligned(dev_grad, 4) || !aligned(dev_workspace, 8)) return E_UNSUPPORTED;
  const long long chunk = optim::chunk_of(n);
  const int parts = optim::parts_of(n);
  double* partial = static_cast<double*>(dev_workspace);
  uint32_t* flag = reinterpret_cast<uint32_t*>(partial + parts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (aligned(dev_grad, 16))
    hipLaunchKernelGGL((optim::grad_norm_kernel<true>), dim3(parts), dim3(optim::THREADS), 0, s, dev_grad, (long long)n, chunk, partial, flag);
  else
    hipLaunchKernelGGL((optim::grad_norm_kernel<false>), dim3(parts), dim3(optim::THREADS), 0, s, dev_grad, (long long)n, chunk, partial, flag);
  return launched();
}

int unetpp_optim_step_f32(float* dev_param, float* dev_grad, float* dev_m, float* dev_v, int64_t n, const unetpp_optim_groups* groups,
                          const unetpp_optim_step_args* args, const void* dev_workspace, uint32_t* dev_state, uint32_t* dev_scaler_state,
                          void* stream) {
  if (!dev_param || !dev_grad || !groups || !args || !dev_workspace || !dev_state) return E_INVALID;
  if (const int bad = check_step(n, *groups, *args, dev_m, dev_v)) return bad;
  if (!aligned(dev_param, 4) || !aligned(dev_grad, 4) || !aligned(dev_m, 4) || !aligned(dev_v, 4) || !aligned(dev_workspace, 8) ||
      !aligned(dev_state, 4) || !aligned(dev_scaler_state, 4) || (dev_scaler_state && args->growth_interval < 1))
    return E_UNSUPPORTED;
  const long long chunk = optim::chunk_of(n);
  const int parts = optim::parts_of(n);
  const double* partial = static_cast<const double*>(dev_workspace);
  const uint32_t* flag = reinterpret_cast<const uint32_t*>(partial + parts);
  const bool vec = aligned(dev_param, 16) && aligned(dev_grad, 16) && aligned(dev_m, 16) && aligned(dev_v, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(parts);
  switch (groups->kind) {
    case UNETPP_OPTIM_ADAM:
      launch_step<UNETPP_OPTIM_ADAM>(vec, grid, s, dev_param, dev_grad, dev_m, dev_v, n, chunk, parts, partial, flag, *groups, *args, dev_state,
                                     dev_scaler_state);
      break;
    case UNETPP_OPTIM_ADAMW:
      launch_step<UNETPP_OPTIM_ADAMW>(vec, grid, s, dev_param, dev_grad, dev_m, dev_v, n, chunk, parts, partial, flag, *groups, *args, dev_state,
                                     dev_scaler_state);
      break;
    default:
      launch_step<UNETPP_OPTIM_SGD>(vec, grid, s, dev_param, dev_grad, dev_m, dev_v, n, chunk, parts, partial, flag, *groups, *args, dev_state,
                                     dev_scaler_state);
  }
  return launched();
}

}  // extern "C"
