/* unetpp_two_stage.h — C ABI of the two-stage loop's own steps (infer_two_stage_burr.py): the two class masks at frame size with
 * their sums (:303-314, :333-334), the four chained blends of visualize_two_stage with the burr count (:132-153, :321) and
 * cv2.rotate (:276).  The conventions are those of unetpp_raw.h: the engine first, the stream last, 0 or a negative UNETPP_E_* code;
 * an entry is asynchronous on `stream`, allocates nothing and never synchronises.  A NULL engine is answered with -1
 * (UNETPP_E_INVALID), every other bad argument with UNETPP_E_UNSUPPORTED.  unet_amd/two_stage.py holds the NumPy forms,
 * csrc/two_stage.h the kernels.
 *
 * Shapes: 1 <= batch <= 65535, 1 <= h, w <= 65535, h * w <= 2^30 for every image.  Every uint8 pointer is valid at any byte
 * alignment; the int64 count tables must be 8-byte aligned (they are added to with 64-bit atomics).  No output may overlap an
 * input or another output.  A ROI is (x1, y1, x2, y2) in pixels of the frame, the slice [y1:y2, x1:x2] of NumPy for
 * non-negative bounds: a bound past the frame is the frame's edge, x2 <= x1 or y2 <= y1 is the empty ROI.  Negative bounds are
 * refused.
 *
 * unetpp_two_stage_masks_u8: dev_cable, dev_tape uint8 [batch,fh,fw] = (pred == 1), (pred == 2) of dev_pred uint8 [batch,th,tw],
 *   cv2.resize(INTER_NEAREST) to fw x fh (source index min(floor(d * (1 / (n_dst / n_src))), n_src - 1) in double, as
 *   unetpp_resize_nearest_roi_u8), zero outside the ROI; values 0 / 1.  dev_counts int64 [batch,2] = the set pixels of the two
 *   masks; the entry zeroes it first.  One launch; dev_pred is read once.
 * unetpp_two_stage_overlay_u8: dev_out uint8 [batch,h,w,3] = dev_table[state][channel][frame byte] per byte of dev_frames uint8
 *   [batch,h,w,3], state = 8 * (the pixel lies inside the ROI) + 4 * (cable != 0) + 2 * (tape != 0) + (burr != 0) of the three
 *   masks uint8 [batch,h,w]; dev_table is uint8 [16,3,256] in DEVICE memory.  dev_burr_count int64 [batch] = the non-zero
 *   pixels of dev_burr; the entry zeroes it first.  One launch.
 * unetpp_rotate_u8: cv2.rotate(frame, code) for dev_in uint8 [batch,h,w,channels], channels 1 or 3.  UNETPP_ROTATE_90_CW:
 *   dev_out [batch,w,h,channels], out[y, x] = in[h - 1 - x, y]; UNETPP_ROTATE_180: [batch,h,w,channels], out[y, x] =
 *   in[h - 1 - y, w - 1 - x]; UNETPP_ROTATE_90_CCW: [batch,w,h,channels], out[y, x] = in[x, w - 1 - y]. */
#ifndef UNETPP_TWO_STAGE_H
#define UNETPP_TWO_STAGE_H

#include "unetpp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_ROTATE_90_CW = 0, UNETPP_ROTATE_180 = 1, UNETPP_ROTATE_90_CCW = 2 };

int unetpp_two_stage_masks_u8(unetpp_engine* e, const uint8_t* dev_pred, int batch, int th, int tw, uint8_t* dev_cable, uint8_t* dev_tape, int fh,
                              int fw, int x1, int y1, int x2, int y2, int64_t* dev_counts, void* stream);
int unetpp_two_stage_overlay_u8(unetpp_engine* e, const uint8_t* dev_frames, const uint8_t* dev_cable, const uint8_t* dev_tape,
                                const uint8_t* dev_burr, int batch, int h, int w, int x1, int y1, int x2, int y2, const uint8_t* dev_table,
                                uint8_t* dev_out, int64_t* dev_burr_count, void* stream);
int unetpp_rotate_u8(unetpp_engine* e, const uint8_t* dev_in, int batch, int h, int w, int channels, int code, uint8_t* dev_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_TWO_STAGE_H */
