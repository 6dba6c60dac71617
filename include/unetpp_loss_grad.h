/* unetpp_loss_grad.h — C ABI of the loss gradients: d loss / d logits of the reference's CombinedLoss (cross-entropy + Dice)
 * and AdvancedCombinedLoss (Focal + Tversky + Dice) of src/models/losses.py, in one pass that reads the logits and the target
 * once and writes the gradient once.  The conventions are those of unetpp_loss.h: the engine first, the stream last, 0 or a
 * negative UNETPP_E_* code; the launching entries are asynchronous on `stream`, allocate nothing and never synchronise.  A
 * NULL engine is answered with -1 (UNETPP_E_INVALID), every other bad argument with UNETPP_E_UNSUPPORTED.
 * unet_amd/loss_grad.py holds the NumPy form (loss_grad_np, bit for bit), the coefficients and the torch modules;
 * csrc/loss_grad.h the kernels.
 *
 * Coefficients.  Everything that couples the pixels of a batch is a function of the table of unetpp_loss_sums_f32.  The host
 * computes, in float64, from the columns T, P, I of that table as real numbers (P, I in units of 2^-32), s = smooth = 1e-5:
 *   Dice (losses.py:55-83).  valid depends on T only (ignore_bg drops class 0, skip_empty drops T = 0, nothing left: all but
 *     the background again).  w_bc = 1 / |valid| without class weights, w_c / (sum over valid of w + 1e-6) with them, 0
 *     outside valid.  U = P + T + s:      A_dice = -2 w / U                G_dice = w (2 I + s) / U^2
 *   Tversky (losses.py:189-200).  w = 1 / (B C'), C' = C - 1 with ignore_bg (and 0 for class 0), else C.
 *     D = I + alpha (T - I) + beta (P - I) + s:
 *                                         A_tv = -w [1 / D - (I + s)(1 - alpha - beta) / D^2]      G_tv = w beta (I + s) / D^2
 *   A = weight_dice A_dice + weight_tversky A_tv, G likewise: G is d loss / d P_bc, A is d loss / d I_bc.
 *   K_ce[., c]  = weight_ce w_c / sum over (b, c') of w_c' T_bc'     (torch's weighted mean; w = 1 without weights)
 *   K_foc[., c] = weight_focal alpha_c / (B h w)                     (the reference's Focal mean runs over every pixel)
 * and rounds them once to float32: dev_coef float32 [batch,classes,4] = (A, G, K_ce, K_foc), 4-byte aligned.  CombinedLoss
 * has weight_tversky = 0 and K_foc = 0, AdvancedCombinedLoss K_ce = 0.
 *
 * unetpp_loss_grad_f32.  dev_logits float32 [batch,classes,h,w], 4-byte aligned, 2 <= classes <= 8; dev_target uint8
 * [batch,h,w], any alignment; gamma an integer in 0..4; 1 <= batch <= 65535, h, w >= 1, h * w <= 2^22 (the limits of
 * unetpp_loss_sums_f32).  dev_scale NULL or one float32 on the device (the incoming gradient of the loss), 4-byte aligned.
 * dev_grad float32 [batch,classes,h,w], 4-byte aligned at any phase of its own: every element is written exactly once, no
 * atomics and no memset, so the result does not depend on the order in which threads arrive.  dev_grad == dev_logits (the
 * gradient in place) is allowed; any other overlap of dev_grad with an input is UNETPP_E_UNSUPPORTED.
 *
 * Per pixel, in float32, every operation rounded on its own (no fused multiply-add), IEEE division, in this order (x_c the
 * logits, t the target; exp32, log32 and the first line are those of unetpp_loss.h):
 *   m = max_c x_c;  d_c = x_c - m;  e_c = exp32(d_c);  s = e_0 + e_1 + ... in class order;  p_c = e_c / s
 *   nll = min(max(0, log32(s) - d_t), 131072)         the forward's clamp: it keeps 0 * nll finite
 *   om  = 1 - p_t;  w1 = om^(gamma - 1) by repeated multiplication from 1 (w1 = 1 for gamma <= 1);
 *   w   = w1 om for gamma >= 1, else 1
 *   phi = w + ((gamma p_t) w1) nll,  and phi = 1 for gamma = 0            d [(1 - p_t)^gamma nll] / d x_c = phi y_c
 *   u_c = G_c + A_c for c = t, G_c otherwise;  dot = p_0 u_0 + p_1 u_1 + ... in class order;  r_c = p_c (u_c - dot)
 *   k   = K_ce[t] + K_foc[t] phi;  y_c = p_c - 1 for c = t, p_c otherwise;  g_c = k y_c + r_c
 *   g_c = g_c * (*dev_scale) when dev_scale is given
 * A pixel the forward leaves out of every sum (target >= classes, or a logit that is not finite) gets g_c = +0 for every c.
 *
 * unetpp_loss_narrow_target_i64.  dev_target_i64 int64 [n], 8-byte aligned (the reference's targets, dataset.py:100-101);
 * dev_target_u8 uint8 [n], any alignment, not overlapping the input; 1 <= n <= 65535 * 2^22.  Values 0..254 are copied,
 * every other value (ignore_index -100 included) becomes 255, which both loss kernels count as outside the classes. */
#ifndef UNETPP_LOSS_GRAD_H
#define UNETPP_LOSS_GRAD_H

#include "unetpp_loss.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_LOSS_GRAD_COEFFICIENTS = 4 };

/* *span_pixels = the consecutive pixels of a frame one workgroup owns (that of unetpp_loss_layout). */
int unetpp_loss_grad_layout(int* span_pixels);
int unetpp_loss_grad_f32(unetpp_engine* e, const float* dev_logits, const uint8_t* dev_target, int batch, int classes, int h,
                         int w, int gamma, const float* dev_coef, const float* dev_scale, float* dev_grad, void* stream);
int unetpp_loss_narrow_target_i64(unetpp_engine* e, const int64_t* dev_target_i64, int64_t n, uint8_t* dev_target_u8, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_LOSS_GRAD_H */
