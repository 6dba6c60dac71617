/* unetpp_contours.h — C ABI of the tail of the refactored frame loop (the reference's infer_video_refactored.py:366-405):
 * the external contours of a mask and their areas, the smallest circle around the largest one (measure_diameter),
 * paste_roi_mask and the three chained blends of create_overlay.  The conventions are those of unetpp_roi.h: the engine
 * first, the stream last, 0 or a negative UNETPP_E_* code; a launching entry is asynchronous on `stream`, allocates nothing
 * and never synchronises.  A NULL engine is answered with -1 (UNETPP_E_INVALID), every other bad argument with
 * UNETPP_E_UNSUPPORTED.  unet_amd/contours.py holds the NumPy forms, csrc/contours.h the kernels.
 *
 * No border is followed on the device.  With the frame zero-padded, `outside` is the background (pixels that are not
 * foreground) 4-connected to the padding and `inside` everything else: the foreground, its holes and what lies in them.
 * One 8-connected component of `inside` is one contour of findContours(RETR_EXTERNAL); labels are numbered in raster order
 * of first pixels, as unetpp_components numbers them.  Foreground is mask == match_class, or mask != 0 for match_class < 0.
 *
 * Shapes: 1 <= batch <= 65535, 1 <= h, w <= 4095 (coordinates below 2^12 keep the circle's integer predicates inside
 * int64).  Masks and frames are uint8 at any alignment; int32 tables 4-byte aligned, uint64 tables 8-byte aligned, the
 * workspace 16-byte aligned.
 *
 * unetpp_contour_areas_u8:
 *   dev_labels  int32 [batch,h,w]       the label of every inside pixel, 0 outside
 *   dev_num     int32 [batch]           labels of the frame, the background included (exact even beyond capacity)
 *   dev_area2   uint64 [batch,capacity] twice the contourArea of the contour of each label < capacity, row 0 = 0: the sum
 *               over every 2 x 2 window of pixel centres (those hanging over the frame edge included) of 2 where all four
 *               pixels are inside, 1 where exactly three are.  Integer sums: independent of the order of arrival.
 *   dev_border  uint8 [batch,h,w] or NULL: 1 on the foreground pixels with a 4-neighbour that is outside or beyond the frame
 *               (the pixels of the external contours), else 0.
 * unetpp_contour_circle: from the three tables above, per frame the label of the largest area2 (the lowest label on ties,
 *   among labels < capacity) and a support set of the smallest circle around its pixels:
 *   dev_support int32 [batch,8] = {count, x0, y0, x1, y1, x2, y2, label}; count = 0 and label = 0 for a frame without
 *               foreground, unused coordinates 0.  The circle is the one through the points (1: the point; 2: their
 *               diameter; 3: their circumcircle); when more points lie on it, which of them are reported is not part of
 *               the contract, the circle is.  The caller computes centre and radius (circle_from_points).
 * unetpp_paste_roi_u8: dev_out uint8 [batch,out_h,out_w] = zeros with dev_masks [batch,h,w] pasted as the reference's
 *   paste_roi_mask does for roi = (x, y, w, h): x1 = max(0, roi_x), x2 = min(out_w, roi_x + roi_w), the first
 *   min(w, x2 - x1) columns of the mask at x1, and the same for rows.  A ROI that misses the frame is refused.
 * unetpp_overlay_chain_u8: dev_out uint8 [batch,h,w,3]: every byte of dev_frames sent through table[0], table[1], table[2]
 *   in this order, each only where dev_cable, dev_tape, dev_burr [batch,h,w] is non-zero; host_table uint8 [3,3,256] is
 *   indexed [mask][channel][value] and read on the host before the entry returns.  No float arithmetic on the device. */
#ifndef UNETPP_CONTOURS_H
#define UNETPP_CONTOURS_H

#include "unetpp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_CONTOURS_MAX_SIDE = 4095, UNETPP_CONTOURS_SUPPORT_COLUMNS = 8 };

/* 0 for a shape or capacity the entries refuse */
size_t unetpp_contours_workspace_bytes(int batch, int h, int w, int capacity);
int unetpp_contour_areas_u8(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, int match_class, int capacity,
                            int32_t* dev_labels, int32_t* dev_num, uint64_t* dev_area2, uint8_t* dev_border, void* dev_workspace,
                            void* stream);
int unetpp_contour_circle(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const uint64_t* dev_area2, int batch,
                          int h, int w, int capacity, int32_t* dev_support, void* dev_workspace, void* stream);
int unetpp_paste_roi_u8(unetpp_engine* e, const uint8_t* dev_masks, int batch, int h, int w, int roi_x, int roi_y, int roi_w,
                        int roi_h, int out_h, int out_w, uint8_t* dev_out, void* stream);
int unetpp_overlay_chain_u8(unetpp_engine* e, const uint8_t* dev_frames, const uint8_t* dev_cable, const uint8_t* dev_tape,
                            const uint8_t* dev_burr, int batch, int h, int w, const uint8_t* host_table, uint8_t* dev_out,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_CONTOURS_H */
