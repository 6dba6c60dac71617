/* unetpp_raw.h — C ABI of the raw camera frames: the Bayer demosaic of the reference's GigECameraHarvester._to_bgr
 * (src/camera/gige_harvester.py:101-114), alone and fused into the resize of preprocess_image (infer_two_stage_burr.py:122-127).
 * The conventions are those of unetpp_simple_loops.h: the engine first, the stream last, 0 or a negative UNETPP_E_* code; an
 * entry is asynchronous on `stream`, allocates nothing and never synchronises.  A NULL engine is answered with -1
 * (UNETPP_E_INVALID), every other bad argument with UNETPP_E_UNSUPPORTED.  unet_amd/raw_frames.py holds the NumPy forms,
 * csrc/raw_frames.h the kernels.
 *
 * Shapes: 1 <= batch <= 65535, 3 <= h, w <= 65535 (1 <= h, w for UNETPP_RAW_MONO), h * w <= 2^30.  Every pointer is valid at any
 * byte alignment.  Raw byte (f, y, x) is read at dev_raw[f * frame_stride + y * row_stride + x]; the strides are in bytes,
 * row_stride >= w and frame_stride >= (h - 1) * row_stride + w, so a padded GenTL line is read in place.  No output may overlap
 * the input or another output.
 *
 * The arithmetic is OpenCV's bilinear Bayer2RGB_<uchar>, integer and exact.  Interior pixels (1 <= y <= h - 2, 1 <= x <= w - 2):
 * a channel measured at the pixel is the raw byte; at a red or blue site green is (N + S + W + E + 2) >> 2 and the opposite colour
 * (NW + NE + SW + SE + 2) >> 2; at a green site red and blue are (a + b + 1) >> 1 of their two neighbours, horizontal for the
 * colour that shares the row, vertical for the other.  Border: out[y, x] = interior[clamp(y, 1, h - 2), clamp(x, 1, w - 2)].
 * A pattern carries OpenCV's name (the components in the second row, second and third columns).  Red and blue sites by
 * (row parity, column parity): BG red (0,0) blue (1,1); GB red (0,1) blue (1,0); RG red (1,1) blue (0,0); GR red (1,0) blue (0,1).
 * UNETPP_RAW_MONO gives (v, v, v) and has no border rule.
 *
 * unetpp_raw_to_bgr_u8: dev_bgr uint8 [batch,h,w,3] BGR = the demosaiced frame, dev_gray uint8 [batch,h,w] =
 *   (3735 B + 19235 G + 9798 R + 16384) >> 15 of it (cv2's COLOR_BGR2GRAY).  Either may be NULL, not both; with dev_bgr NULL the
 *   BGR frame is never written.
 * unetpp_raw_resize_u8: dev_out uint8 [batch,oh,ow,3] BGR = cv2.resize(INTER_LINEAR) to ow x oh (the 11-bit fixed-point form of
 *   unetpp_resize_linear_u8) of the crop [y0, y0 + ch) x [x0, x0 + cw) of the demosaiced frame, which is never written: only
 *   the taps the resize reads are demosaiced.  The demosaic's phase comes from the frame's coordinates, so x0 and y0 may be odd.
 *   0 <= x0, x0 + cw <= w, cw >= 1, the same for y; 1 <= oh, ow <= 65535, oh * ow <= 2^30. */
#ifndef UNETPP_RAW_H
#define UNETPP_RAW_H

#include "unetpp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { UNETPP_RAW_BG = 0, UNETPP_RAW_GB = 1, UNETPP_RAW_RG = 2, UNETPP_RAW_GR = 3, UNETPP_RAW_MONO = 4 };

int unetpp_raw_to_bgr_u8(unetpp_engine* e, const uint8_t* dev_raw, int64_t row_stride, int64_t frame_stride, int batch, int h, int w,
                         int pattern, uint8_t* dev_bgr, uint8_t* dev_gray, void* stream);
int unetpp_raw_resize_u8(unetpp_engine* e, const uint8_t* dev_raw, int64_t row_stride, int64_t frame_stride, int batch, int h, int w,
                         int pattern, int x0, int y0, int cw, int ch, uint8_t* dev_out, int oh, int ow, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNETPP_RAW_H */
