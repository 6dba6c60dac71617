/* unetpp_roi.h — C ABI of the two 3-class frame loops that decide things per frame from the frame itself:
 * infer_video_roi.py (the cable's column range from an edge projection, crop and resize, thresholds from the frame's own
 * probability means, ultra_strict_threshold, refine_mask_by_geometry, resize back and paste) and
 * infer_video_3class_full.py (select_primary_component).  The conventions are those of unetpp.h: the engine first, the
 * stream last, 0 or a negative UNETPP_E_* code; every launching entry is asynchronous on `stream`, allocates nothing and
 * never synchronises.  Every bad argument except a NULL engine is answered with UNETPP_E_UNSUPPORTED.  unet_amd/roi_loop.py
 * is the NumPy form of every entry; csrc/roi_loop.h states the arithmetic.
 *
 * Two small device tables carry a frame's decisions from one entry to the next, so that no value is read back:
 *   dev_roi         int32   [B,4]  (x_min, x_max, found, valid); valid = x_max > x_min
 *   dev_thresholds  float32 [B,3]  (t_cable, t_tape, bg_margin)
 *
 * Column range (detect_roi_by_projection after its Canny, :34-57).  dev_edges uint8 [B,h,w], non-zero = edge.  Per-column
 * counts of non-zero pixels, the window-30 box sum in np.convolve's mode='same' alignment (max(w, 30) entries), a column
 * is significant when 10 S > 3 max S; first and last significant column scaled as int(col * (w / 512)), widened by
 * int((x_max - x_min) * 0.1) and clipped to [0, w], in float64; a frame without an edge gets (int(w * 0.25), int(w * 0.75))
 * and found = 0.  1 <= h, w <= 65535, h * w <= 2^30.  dev_workspace: the projection's size query below, 4-byte aligned.
 *
 * Crop and resize.  dev_frames uint8 [B,h,w,channels], 1 <= channels <= 4; dev_out uint8 [B,out_h,out_w,channels] =
 * cv2.resize(frame[:, x_min:x_max], (out_w, out_h)) with OpenCV's 11-bit fixed-point INTER_LINEAR, the source width read
 * from dev_roi on the device; zeros for a frame that is not valid.
 *
 * Thresholds (adaptive_thresholding, :60-97).  dev_probs float32 [B,channels,h,w], channels >= 3, 4-byte aligned; planes
 * 0..2 are summed per frame as floor(clamp(p, 0, 1) * 2^32) in 64 bits, mean = (float)((double)sum / ((double)(h * w) * 2^32)),
 * and in float32 t_cable = mean1 > 0.3 ? min(0.85, mean1 + 0.4) : 0.5, t_tape = mean2 > 0.15 ? min(0.85, mean2 + 0.5) : 0.55,
 * bg_margin = max(0.2, 1 - mean0).  dev_means and dev_maxima float32 [B,3] hold the means and the largest max(p, 0) of the
 * three planes.  dev_workspace: the statistics' size query below, 8-byte aligned.
 *
 * Ultra strict (ultra_strict_threshold, :100-125).  dev_cable, dev_tape uint8 [B,h,w], 1 where the class is the first
 * maximum of planes 0..2 and p >= t and p > bg * 2 and p >= bg + bg_margin (float32), thresholds read from dev_thresholds.
 * Any alignment of the masks; 16-byte accesses where an address allows.
 *
 * Component rules, on the labels, num, stats and sums that the components entry of unetpp.h writes, with that call's
 * dev_workspace:
 *   UNETPP_ROI_RULE_GEOMETRY  refine_mask_by_geometry (:128-167): every component stays unless area < min_area, or
 *       h / w < min_aspect and w > wide_width, or int(sum_x / area) < edge_lo * w_frame or > edge_hi * w_frame while
 *       area < large_area; float64 comparisons
 *   UNETPP_ROI_RULE_PRIMARY   select_primary_component (infer_video_3class_full.py:85-114): among the components with
 *       area >= min_area and aspect = h / max(1, w) >= min_aspect the first with the strictly greatest
 *       score = area * aspect * (1 - |sum_x / area - w_frame / 2| / max(1, w_frame)), float64 without contraction
 * dev_out uint8 [B,h,w] = out_value on the kept components, 0 elsewhere and everywhere when num > capacity.
 *
 * Paste.  dev_out0, dev_out1 uint8 [B,out_h,out_w]: columns [x_min, x_max) hold cv2.resize(mask, (x_max - x_min, out_h),
 * INTER_NEAREST) of dev_mask0, dev_mask1 uint8 [B,h,w], everything else 0; all 0 for a frame that is not valid. */
#ifndef UNETPP_ROI_H
#define UNETPP_ROI_H

#include "unetpp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_ROI_RULE_GEOMETRY = 0, UNETPP_ROI_RULE_PRIMARY = 1 };

typedef struct unetpp_roi_cc_rule {
  double min_area;    /* 2000 (geometry), 1000 (primary) */
  double min_aspect;  /* 2.0 (geometry), 1.6 (primary) */
  double wide_width;  /* 100; geometry only, as are the three below */
  double edge_lo;     /* 0.1 */
  double edge_hi;     /* 0.9 */
  double large_area;  /* 10000 */
} unetpp_roi_cc_rule;

size_t unetpp_roi_projection_workspace_bytes(int batch, int w);
size_t unetpp_roi_stats_workspace_bytes(int batch);
int unetpp_roi_from_edges_u8(unetpp_engine* e, const uint8_t* dev_edges, int batch, int h, int w, int32_t* dev_roi,
                             void* dev_workspace, void* stream);
int unetpp_roi_crop_resize_u8(unetpp_engine* e, const uint8_t* dev_frames, int batch, int h, int w, int channels,
                              const int32_t* dev_roi, uint8_t* dev_out, int out_h, int out_w, void* stream);
int unetpp_roi_adaptive_thresholds_f32(unetpp_engine* e, const float* dev_probs, int batch, int channels, int h, int w,
                                       float* dev_thresholds, float* dev_means, float* dev_maxima, void* dev_workspace,
                                       void* stream);
int unetpp_roi_ultra_strict_f32(unetpp_engine* e, const float* dev_probs, int batch, int channels, int h, int w,
                                const float* dev_thresholds, uint8_t* dev_cable, uint8_t* dev_tape, void* stream);
int unetpp_roi_components_select(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats,
                                 const uint64_t* dev_sums, int batch, int h, int w, int capacity, int rule,
                                 const unetpp_roi_cc_rule* params, uint8_t out_value, uint8_t* dev_out, void* dev_workspace,
                                 void* stream);
int unetpp_roi_paste_masks_u8(unetpp_engine* e, const uint8_t* dev_mask0, const uint8_t* dev_mask1, int batch, int h, int w,
                              const int32_t* dev_roi, uint8_t* dev_out0, uint8_t* dev_out1, int out_h, int out_w, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_ROI_H */
