/* unetpp_train_batch.h — C ABI of the training batches: what the reference's dataset classes (src/data/dataset.py,
 * src/data/patch_dataset.py, the tape-focused crop of src/data/advanced_dataset.py and the class maps of the trainers) do per
 * sample and per pixel on the host, in one launch per batch over a dataset that stays resident on the device as uint8.  The
 * conventions are those of unetpp_loss_grad.h: the engine first, the stream last, 0 or a negative UNETPP_E_* code; the launching
 * entries are asynchronous on `stream`, allocate nothing and never synchronise.  A NULL engine is answered with -1
 * (UNETPP_E_INVALID), every other bad argument with UNETPP_E_UNSUPPORTED.  unet_amd/train_batch.py holds the NumPy forms
 * (assemble_np, tape_crop_rect_np, hsv_value_scale_np: bit for bit), csrc/train_batch.h the kernels and the arithmetic.
 *
 * The resident set.  dev_images uint8, images_bytes long: decoded RGB images [h,w,3] one behind the other; dev_masks uint8,
 * masks_bytes long: their masks [h,w]; both at any alignment.  dev_items int64 [n_items,4] = (image offset, mask offset, h, w),
 * offsets in bytes from the arenas' starts, 8-byte aligned, 1 <= h, w <= 65535, h * w <= 2^31 - 1.  The kernels check every
 * row they use against images_bytes and masks_bytes; an item that does not fit is not read.
 *
 * unetpp_train_crop_rects.  dev_requests int32 [batch,5] = (item, k, crop_h, crop_w, class), dev_rects int32 [batch,6] = (x1,
 * y1, x2, y2, n_found, valid), both 4-byte aligned; 1 <= batch <= 65535.  One workgroup per sample finds the k-th (0-based)
 * pixel of `class` in raster order and builds the rectangle of advanced_dataset.py:165-180 around it: y1 = max(0, cy - crop_h /
 * 2), y2 = min(h, cy + crop_h / 2); when y2 - y1 < crop_h: y2 = min(h, y1 + crop_h) if y1 == 0, else y1 = max(0, y2 - crop_h);
 * x likewise.  n_found is the class's pixel count.  n_found == 0: the whole item, valid 1 (the reference returns the original).
 * k outside 0 .. n_found - 1 (a stale count) or a crop size below 1: the whole item, valid 0.  An item that does not fit the
 * arena: six zeros.
 *
 * unetpp_train_batch_u8.  dev_plan int32 [batch,16], 4-byte aligned, one row per output sample:
 *   0 item   1 rect row, or -1 for the inline rectangle   2..5 x1, y1, x2, y2 (inline)   6 flip_h   7 flip_v   8 rot90 k (0..3)
 *   9 row of the byte look-up, or -1   10 post_flip_h   11 post_flip_v   12 row of the value look-up, or -1   13..15 unused
 * dev_rects NULL or the int32 [n_rects,6] table of unetpp_train_crop_rects (a later launch on the same stream sees it: nothing
 * is read back); dev_luts NULL or uint8 [n_luts,256]; dev_class_lut NULL (identity) or uint8 [256].  Stages, in this order:
 *   1 crop   2 fliplr, flipud, np.rot90(., k)   3 the byte look-up on every source tap   4 cv2's 11-bit INTER_LINEAR to out_w x
 *   out_h with coefficients from the sample's own size after stage 2   5 flips of the result   6 the brightness step: 8-bit
 *   RGB -> HSV (hue range 180), V through the value look-up, HSV -> RGB   7 i / 255.0f by IEEE division, or the byte
 * The mask takes 1, 2, INTER_NEAREST, 5 and dev_class_lut.  Equal source and destination size give the source bytes.
 * image_format UNETPP_TRAIN_CHW_F32: dev_image_out float32 [batch,3,out_h,out_w], 4-byte aligned; UNETPP_TRAIN_HWC_RGB /
 * UNETPP_TRAIN_HWC_BGR: uint8 [batch,out_h,out_w,3] at any alignment.  dev_target_out uint8 [batch,out_h,out_w] at any
 * alignment.  1 <= batch, out_h, out_w <= 65535.  Every output byte is written exactly once, in 16-byte stores wherever 16
 * bytes of a tile row lie between two 16-byte boundaries of the destination; no atomics.  A sample whose plan row does not fit
 * (item, rectangle row, look-up row out of range; an empty rectangle after clamping to the item) is written as zeros. */
#ifndef UNETPP_TRAIN_BATCH_H
#define UNETPP_TRAIN_BATCH_H

#include "unetpp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_TRAIN_PLAN_COLUMNS = 16, UNETPP_TRAIN_RECT_COLUMNS = 6, UNETPP_TRAIN_REQUEST_COLUMNS = 5, UNETPP_TRAIN_ITEM_COLUMNS = 4 };
enum { UNETPP_TRAIN_CHW_F32 = 0, UNETPP_TRAIN_HWC_RGB = 1, UNETPP_TRAIN_HWC_BGR = 2 };

/* the output tile of a workgroup, the mask bytes a workgroup of unetpp_train_crop_rects compares per pass, the plan's columns */
int unetpp_train_batch_layout(int* tile_w, int* tile_h, int* pass_bytes, int* plan_columns);
int unetpp_train_crop_rects(unetpp_engine* e, const uint8_t* dev_masks, int64_t masks_bytes, const int64_t* dev_items, int n_items,
                            const int32_t* dev_requests, int batch, int32_t* dev_rects, void* stream);
int unetpp_train_batch_u8(unetpp_engine* e, const uint8_t* dev_images, int64_t images_bytes, const uint8_t* dev_masks,
                          int64_t masks_bytes, const int64_t* dev_items, int n_items, const int32_t* dev_plan, int batch,
                          const int32_t* dev_rects, int n_rects, const uint8_t* dev_luts, int n_luts, const uint8_t* dev_class_lut,
                          int out_h, int out_w, int image_format, void* dev_image_out, uint8_t* dev_target_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_TRAIN_BATCH_H */
