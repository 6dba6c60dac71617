/* unetpp_simple_loops.h — C ABI of the pixel and component rules of the spatial, fixed and simple video loops (the reference's
 * infer_video_spatial.py, infer_video_fixed.py, infer_video_simple_v2.py and infer_video_simple_optimized.py).  The conventions
 * are those of unetpp_roi.h and unetpp_contours.h: the engine first, the stream last, 0 or a negative UNETPP_E_* code; an entry
 * is asynchronous on `stream`, allocates nothing and never synchronises.  A NULL engine is answered with -1 (UNETPP_E_INVALID),
 * every other bad argument with UNETPP_E_UNSUPPORTED.  unet_amd/simple_loops.py holds the NumPy forms, csrc/simple_loops.h
 * the kernels.
 *
 * Shapes: 1 <= batch <= 65535, 1 <= h, w <= 65535, h * w <= 2^30 (2^23 for the tape filter, whose sums of uint8 values are
 * int32).  Masks are uint8 at any alignment; int32 tables are 4-byte aligned, float planes 4-byte aligned.
 *
 * unetpp_pixel_rules_f32: two rules on three float32 probabilities per pixel -> dev_cable, dev_tape uint8 0/1 [batch,h,w].
 *   Channel c (0 background, 1 cable, 2 tape) of pixel i = y * w + x of frame f is read in place at
 *   dev_probs[f * frame_stride + c * plane_stride + i * pixel_stride] (strides in elements, all positive, one frame's reads
 *   inside frame_stride): [B,C,H,W] is (C h w, h w, 1), [B,H,W,C] is (h w C, 1, C).  Arithmetic is float32, no contraction.
 *   UNETPP_PIXEL_RELATIVE    relative_threshold (infer_video_spatial.py:71-98) with a = cable_bg_ratio, b = tape_bg_ratio:
 *                            c = cable > bg * a, t = tape > bg * b; where both hold c = cable >= tape and t = !c.
 *   UNETPP_PIXEL_CONFIDENCE  simple_threshold (infer_video_simple_v2.py:36-58) with a = b = conf_threshold: the winner is the
 *                            first maximum of the three (the first NaN when there is one, as np.argmax answers);
 *                            c = winner == 1 && cable >= a, t = winner == 2 && tape >= b.
 *   A comparison with a NaN is false.  a and b must not be NaN.
 * unetpp_components_keep: from the label, num and stats tables of unetpp_components (capacity rows; dev_workspace is the
 *   one of that call), dev_out uint8 [batch,h,w] = out_value on EVERY component with min_area <= area <= max_area and
 *   bounding-box width >= min_width, else 0: filter_by_size_and_shape (infer_video_fixed.py:85-105), the tape filter
 *   area >= 500 and width >= 20 (infer_video_simple_optimized.py:194-208) and the burr filter area >= 100 (:213-226,
 *   infer_video_simple.py:137-146).  A frame with more than `capacity` labels comes out all zero.
 * unetpp_tape_position_filter_u8: spatial_filter_tape (infer_video_simple_optimized.py:88-137) per frame.  A mask is read as its
 *   bytes for match < 0, else as 1 where a byte equals match and 0 elsewhere (two classes of one map: the same pointer twice).
 *   With x_min, x_max the first and last column holding a non-zero cable pixel and cw = x_max - x_min, the valid columns are
 *   [max(0, x_min - cw / 2), x_min + cw / 3) and [max(x_min + 2 * cw / 3, x_max - cw / 3), min(w, x_max + cw / 2)) (integer
 *   division; an empty range stays empty).  original_area = the sum of the tape's values, filtered_area = the sum of tape & 1
 *   over the valid columns.  dev_out uint8 [batch,h,w] = tape & 1 in the valid columns and 0 in the others, or the tape itself
 *   when the cable is empty, original_area is 0 or 2 * filtered_area < original_area.
 *   dev_table int32 [batch,6] = {x_min, x_max, original_area, filtered_area, verdict, 0}: -1 extents for an empty cable,
 *   filtered_area 0 when the cable or the tape is empty, verdict 1 where the filtered tape was written.  The table carries the
 *   decision from launch to launch; nothing is read back.  dev_out must not overlap an input.
 * unetpp_column_band_u8: dev_out uint8 [batch,h,w] = dev_mask & 1 in columns [x_start, x_end), 0 in the others: the AND with
 *   create_vertical_focus_region (infer_video_spatial.py:56-68, :155-156), x_start = int(w * 0.25), x_end = int(w * 0.75)
 *   there.  0 <= x_start, x_end <= w; dev_out must not overlap dev_mask.
 * unetpp_mask_join_u8: dev_out uint8 [batch,h,w] = (dev_a & and_a) | (dev_b != 0 ? or_b : 0) | (dev_c != 0 ? or_c : 0); dev_b
 *   and dev_c may be NULL.  It joins separately filtered masks into the one map of bits that unetpp_merge_classes turns into
 *   the merged class map and its table (infer_video_simple.py:148-152, infer_video_simple_optimized.py:228-232). */
#ifndef UNETPP_SIMPLE_LOOPS_H
#define UNETPP_SIMPLE_LOOPS_H

#include "unetpp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_PIXEL_RELATIVE = 0, UNETPP_PIXEL_CONFIDENCE = 1 };
enum { UNETPP_TAPE_TABLE_COLUMNS = 6, UNETPP_TAPE_MAX_PIXELS = 1 << 23 };

int unetpp_pixel_rules_f32(unetpp_engine* e, const float* dev_probs, int64_t frame_stride, int64_t plane_stride, int64_t pixel_stride,
                           int batch, int h, int w, int rule, float a, float b, uint8_t* dev_cable, uint8_t* dev_tape, void* stream);
int unetpp_components_keep(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats, int batch,
                           int h, int w, int capacity, int min_area, int max_area, int min_width, uint8_t out_value, uint8_t* dev_out,
                           void* dev_workspace, void* stream);
int unetpp_tape_position_filter_u8(unetpp_engine* e, const uint8_t* dev_tape, int tape_match, const uint8_t* dev_cable, int cable_match,
                                   int batch, int h, int w, uint8_t* dev_out, int32_t* dev_table, void* stream);
int unetpp_column_band_u8(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, int x_start, int x_end, uint8_t* dev_out,
                          void* stream);
int unetpp_mask_join_u8(unetpp_engine* e, const uint8_t* dev_a, int and_a, const uint8_t* dev_b, int or_b, const uint8_t* dev_c, int or_c,
                        int batch, int h, int w, uint8_t* dev_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_SIMPLE_LOOPS_H */
