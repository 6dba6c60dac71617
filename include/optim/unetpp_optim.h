/* unetpp_optim.h — C ABI of the optimiser step: the three lines every training loop of the reference runs after backward(),
 *   torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm);  optimizer.step();  optimizer.zero_grad()
 * with Adam, AdamW or SGD(momentum), optionally inside GradScaler.unscale_ / step / update, as two launches over one flat
 * float32 buffer.  The library (libunetpp_optim_hip.so, built from unet-_amd/csrc_optim/) is separate from the engine's: its
 * entries take no engine, the last parameter of a launching entry is the stream.  They return 0 or a negative code with the
 * values of UNETPP_E_* (-1 invalid: a NULL pointer; -2 unsupported: every other bad argument; -3 a HIP call failed), are
 * asynchronous on `stream`, allocate nothing, never synchronise and read nothing back.  unet_amd/optim.py holds the NumPy
 * form (grad_norm_np, scalars_np, step_np, scaler_update_np: bit for bit) and the torch classes.
 *
 * Layout (unetpp_optim_layout).  The n elements are cut into chunks of
 *   chunk(n) = granule * ceil(n / (granule * max_partials))        elements, 1 <= n <= 2^27,
 * one workgroup of 256 threads per chunk, parts(n) = ceil(n / chunk(n)) <= max_partials of them.  Chunk and grid follow from n
 * alone, never from the device.  Inside a chunk, 4-element vector j (elements 4j .. 4j+3 of the chunk) belongs to thread
 * j mod 256; ownership is by element index, not by address.  Every buffer may be 4-byte aligned at any phase; when all of
 * a launch's buffers are 16-byte aligned the accesses are 16 bytes wide, otherwise 4, with the same results bit for bit.
 *
 * Workspace (unetpp_optim_workspace_bytes(n) bytes, 8-byte aligned): float64 partial[parts], then uint32 flag[parts].
 *
 * unetpp_optim_grad_norm_f32 (launch A).  Thread: four float64 accumulators a_k, one per vector component, a_k += (double)x *
 * (double)x over its vectors in index order (elements past n count as +0); lane value (a_0 + a_1) + (a_2 + a_3).  Wave: v[l] +=
 * v[l + off] for off = 32, 16, 8, 4, 2, 1.  Workgroup: ((w_0 + w_1) + w_2) + w_3.  partial[chunk] = that sum, flag[chunk] = 1 when
 * it is not finite (the float64 square of a float32 is exact and cannot overflow, so that is: when an element is not finite).
 *
 * unetpp_optim_step_f32 (launch B).  State: dev_state (the optimiser's) and dev_scaler_state (the loss scaler's, or NULL: no
 * scaler) each hold two slots of `state_slot_words` uint32, 4-byte aligned.  A launch touches the words
 *   dev_state:         [0] step count (int32)   [3] total_norm of this step (float32)   [4] found_inf of this step (int32)
 *   dev_scaler_state:  [1] loss scale (float32)   [2] growth tracker (int32)
 * and no other.  It reads slot args->parity (args->scaler_parity) and writes the other slot; the host alternates each parity
 * with every launch that uses the buffer, so no workgroup reads what another writes.  "use_scaler" below means
 * dev_scaler_state != NULL.  Every workgroup derives, from the workspace of launch A on the same gradients:
 *   S = partial[0] + partial[1] + ... in index order (float64);  found_inf = any flag
 *   inv_scale = 1 / scale (float32) with use_scaler, else 1;  total_norm = (float)sqrt(S) * inv_scale
 *   coef = max_norm / (total_norm + 1e-6f), replaced by 1 when it is > 1 (a NaN stays), or 1 without use_clip
 *   mult = inv_scale * coef;  t = step + 1;  bc_i = 1 - pow(beta_i, t) in float64, pow by square-and-multiply:
 *     r = 1, b = beta, e = t;  while e: { if (e & 1) r = r * b;  e >>= 1;  if (e) b = b * b; }
 * and per group (float64 arithmetic on the doubles of unetpp_optim_groups, each result rounded once to float32):
 *   lr, wd, eps, mu, beta2, decay = 1 - lr * wd, omb1 = 1 - beta1, omb2 = 1 - beta2, ss = lr / bc_1, rbc2 = sqrt(bc_2).
 * Per element of group k (elements end[k-1] .. end[k]-1; end[n_groups-1] == n), in float32, every operation rounded on its
 * own (no fused multiply-add), correctly rounded division and square root, subnormals kept:
 *   g = g * mult
 *   ADAM, SGD:  if wd != 0: g = g + wd * p              ADAMW:  if wd != 0: p = p * decay
 *   ADAM, ADAMW:  m = m + (g - m) * omb1;  v = v * beta2 + (g * g) * omb2;  d = sqrt(v) / rbc2 + eps;  p = p - (ss * m) / d
 *   SGD:  if mu != 0: { m = g when t == 1, else m * mu + g;  g = m; }   p = p - lr * g          (v is not touched, may be NULL)
 * With use_scaler and found_inf nothing is written to p, m, v.  With zero_grads every element of g is set to +0, else g is
 * not written (the scaled gradient lives in a register only).  Workgroup 0 writes the other slot:
 *   step' = step when (use_scaler and found_inf), else t;  [3], [4] as above
 *   use_scaler (torch's _amp_update_scale_):  found_inf: scale' = scale * backoff_factor, tracker' = 0
 *     else: k = tracker + 1;  k == growth_interval: scale' = scale * growth_factor if that is finite, else scale; tracker' = 0
 *           otherwise scale' = scale, tracker' = k
 * Without use_scaler a non-finite gradient does what the arithmetic does (NaN or 0 * inf through g * mult), as in torch. */
#ifndef UNETPP_OPTIM_H
#define UNETPP_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_OPTIM_ADAM = 0, UNETPP_OPTIM_ADAMW = 1, UNETPP_OPTIM_SGD = 2 };
enum { UNETPP_OPTIM_MAX_GROUPS = 8 };

typedef struct unetpp_optim_groups {
  int32_t n_groups;                             /* 1 .. UNETPP_OPTIM_MAX_GROUPS */
  int32_t kind;                                 /* UNETPP_OPTIM_* */
  int64_t end[UNETPP_OPTIM_MAX_GROUPS];         /* ascending; end[n_groups - 1] == n */
  double lr[UNETPP_OPTIM_MAX_GROUPS], beta1[UNETPP_OPTIM_MAX_GROUPS], beta2[UNETPP_OPTIM_MAX_GROUPS], eps[UNETPP_OPTIM_MAX_GROUPS],
      weight_decay[UNETPP_OPTIM_MAX_GROUPS], momentum[UNETPP_OPTIM_MAX_GROUPS];
} unetpp_optim_groups;

typedef struct unetpp_optim_step_args {
  int32_t use_clip;
  float max_norm;
  float growth_factor, backoff_factor;
  int32_t growth_interval;
  int32_t zero_grads;
  int32_t parity, scaler_parity;                /* 0 or 1: the slot of dev_state / dev_scaler_state this launch reads */
} unetpp_optim_step_args;

int unetpp_optim_layout(int* granule, int* max_partials, int* state_slot_words, int* max_groups);
size_t unetpp_optim_workspace_bytes(int64_t n);
const char* unetpp_optim_version(void);
int unetpp_optim_grad_norm_f32(const float* dev_grad, int64_t n, void* dev_workspace, void* stream);
int unetpp_optim_step_f32(float* dev_param, float* dev_grad, float* dev_m, float* dev_v, int64_t n, const unetpp_optim_groups* groups,
                          const unetpp_optim_step_args* args, const void* dev_workspace, uint32_t* dev_state, uint32_t* dev_scaler_state,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_OPTIM_H */
