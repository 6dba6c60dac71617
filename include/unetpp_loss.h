/* unetpp_loss.h — C ABI of the validation losses: the five sums per frame and class that every loss of the reference's
 * src/models/losses.py (cross-entropy, DiceLoss, FocalLoss, TverskyLoss, CombinedLoss, AdvancedCombinedLoss) is a function
 * of, from one pass over the logits and the target.  The conventions are those of unetpp_roi.h: the engine first, the stream
 * last, 0 or a negative UNETPP_E_* code; the launching entry is asynchronous on `stream`, allocates nothing and never
 * synchronises.  A NULL engine is answered with -1 (UNETPP_E_INVALID), every other bad argument with UNETPP_E_UNSUPPORTED.
 * unet_amd/loss.py holds the NumPy form (loss_sums_np, bit for bit) and the losses as float64 algebra on the table;
 * csrc/loss.h the kernel.
 *
 * Inputs.  dev_logits float32 [batch,classes,h,w], 4-byte aligned, 2 <= classes <= 8; dev_target uint8 [batch,h,w], any
 * alignment; gamma an integer in 0..4 (the reference uses 2.0); 1 <= batch <= 65535, h, w >= 1, h * w <= 2^22.
 *
 * Outputs, both cleared by the entry (memset on the stream) before its one launch:
 *   dev_table    uint64 [batch,classes,5], 8-byte aligned; columns, with p = softmax over the classes and
 *                nll = -log p[target] per pixel:
 *                  0  T    pixels with target c
 *                  1  P    sum over all pixels of p_c                                   units of 2^-32
 *                  2  I    sum over the pixels with target c of p_c                     units of 2^-32
 *                  3  NLL  sum over the pixels with target c of nll                     units of 2^-24
 *                  4  FOC  sum over the pixels with target c of (1 - p_c)^gamma nll     units of 2^-24
 *   dev_outside  uint32 [batch,2], 4-byte aligned: the pixels with target >= classes; the remaining pixels with a logit
 *                that is not finite.  Both kinds stay out of every sum; T summed over the classes plus the two counters
 *                is h * w for every frame.
 * When dev_outside lies directly behind dev_table one memset clears both.  Neither output may overlap an input.
 *
 * Per pixel, in float32, every operation rounded on its own (no fused multiply-add), IEEE division, in this order
 * (x_c the logits, t the target):
 *   m   = max_c x_c                          d_c = x_c - m               e_c = exp32(d_c)
 *   s   = e_0 + e_1 + ...  in class order    p_c = e_c / s
 *   nll = max(0, log32(s) - d_t)             foc = (1 - p_t)^gamma nll,  the power by repeated multiplication from 1
 *   P, I add floor(p_c 2^32);  NLL, FOC add rint(min(v, 131072) 2^24), round-to-nearest-even (truncation would be a bias of
 *   2^-25 per pixel, which on a cross-entropy of 0.24 is larger than the float32 noise of the reference itself).
 * The clamp is unreachable for logits in the fp16 range the engine produces (nll <= 131008 + ln 8).  Sums are integers, so
 * no result depends on the order in which threads arrive and a frame's row is the same in any batch.  With h * w <= 2^22:
 * P, I < 2^54 and NLL, FOC <= 2^63.
 *
 * exp32(d), d <= 0: 0 for d < -87; else with x = d, n = rint(x L), L = 0x1.715476p+0 (log2 e), r = (x - n C1) - n C2,
 *   C1 = 0.693359375, C2 = -0x1.bd0106p-13 (-2.12194440e-4), q = (((((a0 r + a1) r + a2) r + a3) r + a4) r + a5 with
 *   a0..a5 = 0x1.a0d2cep-13, 0x1.6e879cp-10, 0x1.111210p-7, 0x1.555382p-5, 0x1.555554p-3, 0.5:
 *   exp32 = ldexp((q (r r) + r) + 1, n).  The result is a normal number, ldexp is exact.
 * log32(s), s >= 1: s = f 2^e, f in [0.5, 1) (frexp); if f < 0x1.6a09e6p-1 (sqrt 1/2): e = e - 1, x = (f + f) - 1, else
 *   x = f - 1; z = x x; q = b0, then q = q x + b_k for b0..b8 = 0x1.204376p-4, -0x1.d7a370p-4, 0x1.de4a34p-4,
 *   -0x1.fcba9ep-4, 0x1.23d37ep-3, -0x1.555ca0p-3, 0x1.999d58p-3, -0x1.fffff8p-3, 0x1.555554p-2;
 *   y = (q x) z; y = y + C2 e; y = y + (-0.5 z); log32 = (x + y) + C1 e.  log32(1) = 0.
 * These are the Cephes single-precision forms; measured against float64: 0.97 ulp for exp32 on [-87, 0], 0.82 ulp for
 * log32 on (1, 8] (tests/golden/README_loss.txt). */
#ifndef UNETPP_LOSS_H
#define UNETPP_LOSS_H

#include "unetpp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_LOSS_COLUMNS = 5, UNETPP_LOSS_MAX_CLASSES = 8, UNETPP_LOSS_MAX_GAMMA = 4 };

/* *span_pixels = the consecutive pixels of a frame one workgroup owns (a frame of more pixels takes several). */
int unetpp_loss_layout(int* span_pixels);
int unetpp_loss_sums_f32(unetpp_engine* e, const float* dev_logits, const uint8_t* dev_target, int batch, int classes, int h,
                         int w, int gamma, uint64_t* dev_table, uint32_t* dev_outside, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_LOSS_H */
