/* unetpp.h — C ABI of the MI355X-native UNet++ (NestedUNet) inference engine.
 *
 * The reference (Chenxu1103/UNET-) is pure Python and has no FFI of its own; the boundary this
 * library replaces is the nn.Module protocol exercised by its frame loops.  Each entry point cites
 * the reference interface it stands in for (paths relative to the reference root).  The Python
 * drop-in (unet-_amd/nested_unet.py) binds exactly these symbols with ctypes; INTEGRATION.md shows
 * the stub a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success or a negative UNETPP_E_* code; the message is
 * available from unetpp_last_error().  All pointers named dev_* are HIP device pointers on the
 * engine's device; `stream` is a hipStream_t passed as void* (NULL = the default stream).
 * unetpp_forward() is asynchronous on `stream` and never synchronises.  One engine per device;
 * an engine is not thread-safe, independent engines are.  The caller owns all I/O buffers; the
 * library owns packed weights and the activation workspace and never keeps a caller pointer.
 * Every call runs with the engine's device current and restores the calling thread's previous HIP device before
 * it returns.  One thread at a time per engine: the engine keeps per-call state (event pools, resize tables).
 *
 * Value range.  Activations live in HBM as fp16 planes (hi, or hi + lo in EXACT mode), so an activation (or a
 * float32 input value) beyond +-65504 is clamped and a NaN does not propagate the way it does in the fp32
 * reference (src/models/unetpp.py:23-26, src/models/simple_unet.py:94-128).  Neither happens silently: the
 * kernel that narrows such a value sets a sticky flag, see unetpp_status().
 *
 * The BOTTOM of the fp16 window is not flagged.  EXACT's lo plane is an fp16 subnormal (quantum 2^-24) for every
 * |x| < 0.25, so a stored tensor whose LARGEST value is far below 1 is kept with fewer bits.  Measured on the device
 * (tests/test_gpu_value_range.py, one tensor of the network moved at a time, logits of +-1): largest value
 * >= 0.04: logit error <= 6e-6 as at the usual scale; 0.01: <= 2e-5; 2e-3 ... 5e-3 (2^-10 of the usual scale):
 * 2e-5 ... 8e-5; 1.5e-4 ... 3e-4 (2^-14): 3e-4 ... 1.3e-3, i.e. beyond the 1e-3 parity bar.  A checkpoint can be
 * checked with unetpp_debug_read (largest value of every tensor).  EXACT8 keeps its usual error down to 0.01 at
 * least; its error is RELATIVE to the logits (about 1e-4 of the largest |logit|), so it meets 1e-3 absolute only
 * for logits within about +-6, where EXACT stays below 5e-4 up to +-400.  DESIGN.md section 3, "Range".
 */
#ifndef UNETPP_H
#define UNETPP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct unetpp_engine unetpp_engine;

enum {
  UNETPP_OK = 0,
  UNETPP_E_INVALID = -1,     /* bad argument (shape not a multiple of 16, batch too large, ...) */
  UNETPP_E_UNSUPPORTED = -2, /* e.g. pretrained_encoder=True (src/models/unetpp.py:52-65) */
  UNETPP_E_HIP = -3,         /* a HIP runtime call failed */
  UNETPP_E_STATE = -4        /* forward before weights were loaded, ... */
};

/* precision of the 3x3-conv stacks (the 1x1 head always runs in fp32):
 *   EXACT  fp16 MFMA with split operands (x = hi + lo for activations and weights, three MFMAs per
 *          product, fp32 accumulate): fp32-class accuracy; this is the parity-gated mode.
 *   FAST   plain fp16 operands, fp32 accumulate: single MFMA per product.
 *   EXACT8 the main term hi * hi of EXACT in fp16, its two small cross terms lo * w and x * w_lo from 8-bit
 *          operands (e5m2 activations, e4m3 weights) in ONE block-scaled K = 64 MFMA per tap pair
 *          (v_mfma_scale_f32_32x32x64_f8f6f4): 2/3 of EXACT's matrix-pipe cycles, logits within 1e-3 of
 *          the fp32 reference (measured <= 5e-4; EXACT: 1e-5, FAST: 5e-3).  Both architectures.   */
enum { UNETPP_PREC_EXACT = 0, UNETPP_PREC_FAST = 1, UNETPP_PREC_EXACT8 = 2 };

/* network architecture of an engine */
enum {
  UNETPP_ARCH_NESTED = 0,    /* NestedUNet, src/models/unetpp.py:28-135 (the north-star path) */
  UNETPP_ARCH_SIMPLE = 1     /* SimpleUNet, src/models/simple_unet.py:20-128: plain 4-level U-Net,
                                no BatchNorm, ConvTranspose2d(k=2,s=2) upsampling, cat([up, skip]); H, W multiples of 8 */
};

/* input formats accepted by unetpp_forward */
enum {
  UNETPP_IN_F32_NCHW = 0,    /* float32 [B,3,H,W] RGB: the tensor model(img_tensor) receives,
                                infer_two_stage_burr.py:292-295.  Any float32 value: k/255 in [0,1] as that loop feeds, signed
                                normalised inputs (src/infer/preprocess.py:10-15), anything up to +-65504; subnormals and -0.0
                                count as 0.  Beyond +-65504 a value is clamped there and UNETPP_STATUS_OVERFLOW is set; a NaN
                                sets UNETPP_STATUS_NAN and reaches no output (tests/test_gpu_input_domain.py,
                                tests/test_range_status.py) */
  UNETPP_IN_U8_NHWC_BGR = 1  /* uint8 [B,H,W,3] BGR frame at model resolution: fuses the resize-free
                                part of preprocess_image (BGR->RGB, /255, HWC->CHW),
                                infer_two_stage_burr.py:122-127 */
};

typedef struct unetpp_config {
  int num_classes;   /* NestedUNet(num_classes=...)            src/models/unetpp.py:42 */
  int in_channels;   /* NestedUNet(input_channels=3)           src/models/unetpp.py:43 (only 3 supported) */
  int max_batch;     /* largest B passed to unetpp_forward */
  int max_h;         /* largest H (multiple of 16) */
  int max_w;         /* largest W (multiple of 16) */
  int precision;     /* UNETPP_PREC_* */
  int device;        /* HIP device ordinal: model.to(device)   infer_two_stage_burr.py:214 */
  int micro_batch;   /* frames pushed through the network per pass (0 = max_batch) */
  int streams;       /* passes in flight at once (1..4): each gets its own activation area and an internal
                        HIP stream, forked from / joined to the caller's stream with events, so HBM-bound
                        and MFMA-bound kernels of different passes overlap; 0 or 1 = serial */
  int arch;          /* UNETPP_ARCH_* */
} unetpp_config;

/* NestedUNet.__init__ + .to(device) (src/models/unetpp.py:40-91, infer_two_stage_burr.py:214):
 * allocates the activation workspace for (micro_batch, max_h, max_w) on cfg->device.
 *
 * Environment switches, read once here (an engine keeps the plan it was created with):
 *   UNETPP_KSPLIT=max[,min chunks[,gate]]  split-K of small launches (default 16,4,4; 1 = off)
 *   UNETPP_TAPMM=levels                    decoder levels that take the low-resolution GEMM (default "23"; "none" = off)
 *   UNETPP_UPROWS=levels                   decoder levels whose up chunks run on low-resolution rows (default "01")
 *   UNETPP_PLAN_CUS=n                      plan every launch (grid sizes, split-K, tile heights, up-sum tiles) for n compute
 *                                          units instead of the device's own count: a test and diagnosis aid that makes the
 *                                          persistent workgroups walk several tiles each at small shapes.  Results depend on
 *                                          it only through the split-K summation order.  n must be a whole number with
 *                                          1 <= n <= the device's count (launches only ever get smaller), else
 *                                          UNETPP_E_INVALID; a malformed value is refused before the device is looked at. */
int unetpp_create(const unetpp_config* cfg, unetpp_engine** out);

/* del model */
void unetpp_destroy(unetpp_engine* e);

/* Text of the last error on this engine (or, with e == NULL, of the last failed unetpp_create). */
const char* unetpp_last_error(const unetpp_engine* e);

const char* unetpp_version(void);

/* Size in bytes of the canonical weight blob for a (num_classes, in_channels) network:
 * 32-byte header {magic 'UNPP', version, num_classes, in_channels, n_layers, arch, 0,0} followed, for
 * each of the 18 3x3 convs in forward order (conv0_0.conv1, conv0_0.conv2, conv1_0.conv1, ...,
 * conv0_4.conv2) and then the 1x1 head, by the BN-folded fp32 weight in OIHW order and the
 * folded fp32 bias.  The host side (unet-_amd/packing.py) builds it from a state_dict. */
size_t unetpp_weights_blob_bytes(int num_classes, int in_channels);

/* Same for any architecture (header word 5 = arch).  SimpleUNet: the 8 encoder convs enc1.0 ... enc4.2, then
 * up3, up2, up1 (ConvTranspose2d weight in its native [Cin][Cout][2][2] order + bias), then dec3.0 ... dec1.2,
 * then the 1x1 head — the module's definition order (simple_unet.py:30-92); no BatchNorm to fold. */
size_t unetpp_weights_blob_bytes_arch(int arch, int num_classes, int in_channels);

/* model.load_state_dict(checkpoint['model'], strict=True) (infer_two_stage_burr.py:215-216):
 * takes the canonical blob from host memory, uploads it and repacks it on the device into the
 * kernels' layouts (per-channel power-of-two scaling, fp16 hi/lo planes, tile order). Synchronous. */
int unetpp_load_weights(unetpp_engine* e, const void* host_blob, size_t bytes);

/* Same, from a blob already in device memory (e.g. after the RCCL broadcast from rank 0);
 * asynchronous on `stream`. */
int unetpp_load_weights_device(unetpp_engine* e, const void* dev_blob, size_t bytes, void* stream);

/* outputs = model(img_tensor); probs = softmax(outputs,1); pred = argmax(probs,0).astype(uint8);
 * mask_cable = (pred==1); mask_tape = (pred==2)        (infer_two_stage_burr.py:294-304).
 *   dev_input   B frames in `in_format`
 *   dev_logits  float32 [B,num_classes,H,W] or NULL      (NestedUNet.forward return, unetpp.py:119,135)
 *   dev_mask    uint8 [B,H,W] class index (first maximal class) or NULL
 *   dev_cable / dev_tape  uint8 [B,H,W] 0/1 masks of class 1 / class 2, or NULL
 * H and W must be multiples of 16 (the reference raises in torch.cat otherwise), B <= max_batch. */
int unetpp_forward(unetpp_engine* e, const void* dev_input, int in_format, int batch, int h, int w,
                   float* dev_logits, uint8_t* dev_mask, uint8_t* dev_cable, uint8_t* dev_tape,
                   void* stream);

/* ---- value-range status -------------------------------------------------------------------------
 * Sticky flags set by the kernels of any forward since creation (or since the last clearing read):
 *   UNETPP_STATUS_OVERFLOW  a conv / transposed-conv output or a float32 input value exceeded the fp16
 *                           range and was clamped to +-65504: results differ from the fp32 reference
 *   UNETPP_STATUS_NAN       a NaN in a float32 input, or a non-finite weight / bias in a loaded blob (the only ways
 *                           a NaN can reach an accumulator: fp16 operands cannot overflow fp32 sums); the reference
 *                           would carry it to its logits, this engine replaces it (clamp -> +-65504, ReLU -> 0)
 * unetpp_status synchronises the device (hipDeviceSynchronize), copies the flags to *flags and, with
 * clear != 0, resets them.  0 = every value since the last clear was representable. */
enum { UNETPP_STATUS_OVERFLOW = 1, UNETPP_STATUS_NAN = 2 };
int unetpp_status(unetpp_engine* e, uint32_t* flags, int clear);

/* ---- probability outputs and thresholded class rules -------------------------
 * Half of the reference's frame loops do not take a plain argmax: they compute
 * probs = softmax_np(outputs[0].transpose(1,2,0)) on the host and derive the cable / tape masks with
 * a thresholded rule.  unetpp_forward_ex runs the softmax (fp32) and the rule in the same epilogue as
 * the 1x1 head, so neither logits nor probabilities need to leave the GPU. */
enum {
  UNETPP_RULE_ARGMAX = 0,        /* (pred==1), (pred==2)                infer_two_stage_burr.py:303-304 */
  UNETPP_RULE_THRESHOLDED = 1,   /* thresholded_argmax(probs, t_cable, t_tape, bg_margin)
                                    infer_video_3class_best.py:56-83, infer_video_strict.py:36-63 */
  UNETPP_RULE_STRICT_BG = 2,     /* strict_threshold_with_bg_check(probs, t_cable, t_tape, bg_margin)
                                    infer_video_fixed.py:35-83 */
  UNETPP_RULE_EXCLUSIVE = 3      /* exclusive_threshold(probs, t_cable, t_tape, bg_margin, ct_margin)
                                    infer_video_robust.py:70-99 */
};

typedef struct unetpp_outputs {
  float* dev_logits;     /* float32 [B,C,H,W] or NULL */
  float* dev_probs;      /* float32 [B,C,H,W] softmax over C, or NULL (the reference builds HxWxC on the host) */
  uint8_t* dev_mask;     /* uint8 [B,H,W] plain argmax class index, or NULL */
  uint8_t* dev_cable;    /* uint8 [B,H,W] 0/1 under `rule`, or NULL */
  uint8_t* dev_tape;     /* uint8 [B,H,W] 0/1 under `rule`, or NULL */
  int rule;              /* UNETPP_RULE_* (rules 1-3 need num_classes >= 3: bg, cable, tape = classes 0,1,2) */
  float t_cable, t_tape, bg_margin, ct_margin;
} unetpp_outputs;

int unetpp_forward_ex(unetpp_engine* e, const void* dev_input, int in_format, int batch, int h, int w,
                      const unetpp_outputs* out, void* stream);

/* ---- deep-supervision outputs and pruned inference (NestedUNet(deep_supervision=True)) ------------------
 * The list [out, out1, out2, out3] that the reference's forward builds with deep supervision
 * (src/models/unetpp.py:121-133, BatchNorm with its eval statistics):
 *   out_k = F.interpolate(dsK(x_k), size=(H, W), mode='bilinear', align_corners=True)
 *   k = 1: ds1_3 on x1_3 (64 channels)   k = 2: ds2_2 on x2_2 (128)   k = 3: ds3_1 on x3_1 (256)
 * computed as the 1x1 conv in fp32 at (H >> k, W >> k) and ONE bilinear interpolation to (H, W) with ATen's fp32 index rule,
 * followed by the same epilogue as the main head (logits, softmax probabilities, first-max argmax, class masks and
 * rules of unetpp_outputs).  NestedUNet engines only.
 *
 * unetpp_ds_blob_bytes: size of the heads' blob, a 32-byte header {magic 'UNDS', version 1, num_classes, 3, 0,0,0,0}
 * followed by fp32 ds3_1.weight [C][256], ds3_1.bias [C], ds2_2.weight [C][128], ds2_2.bias [C], ds1_3.weight [C][64],
 * ds1_3.bias [C] (the module's definition order, src/models/unetpp.py:87-91).  0 for num_classes < 1.
 *
 * unetpp_load_ds_heads: uploads that blob from host memory.  Synchronous, like unetpp_load_weights.  Allocates the
 * heads and, per internal stream, a float32 scratch of micro_batch * sum_k C (max_h >> k) (max_w >> k) low-resolution
 * logits outside the workspace that unetpp_workspace_bytes reports; unetpp_destroy frees them.  A non-finite value in
 * the blob sets UNETPP_STATUS_NAN.  UNETPP_E_INVALID on a bad magic, size or class count.  The heads belong to the
 * checkpoint of the main weights: a later unetpp_load_weights or unetpp_load_weights_device drops them, and outs[1..3]
 * get UNETPP_E_STATE until they are loaded again.
 *
 * unetpp_forward_ds: one pass computing outs[k] (k = 0..3, the list [out, out1, out2, out3]); outs[k] == NULL skips
 * output k.  outs[0] is exactly unetpp_forward_ex's output (bitwise the same results).  The network runs only as deep
 * as the requested outputs need: with outs[0] == NULL it stops after the node of the smallest requested k, so
 * decoder levels below it are never launched (pruned UNet++ inference).  The logits and probabilities of outs[1..3]
 * must be 16-byte aligned and their masks 4-byte aligned (the kernel stores four pixels at once).
 * Errors: UNETPP_E_UNSUPPORTED for UNETPP_ARCH_SIMPLE; UNETPP_E_INVALID when all four are NULL, a rule is bad or a
 * buffer of outs[1..3] is misaligned;
 * UNETPP_E_STATE when outs[1..3] is requested before unetpp_load_ds_heads (e.g. on an engine loaded with
 * unetpp_load_weights_device only).  Asynchronous on `stream`, like unetpp_forward_ex. */
size_t unetpp_ds_blob_bytes(int num_classes);
int unetpp_load_ds_heads(unetpp_engine* e, const void* host_blob, size_t bytes);
int unetpp_forward_ds(unetpp_engine* e, const void* dev_input, int in_format, int batch, int h, int w,
                      const unetpp_outputs* const outs[4], void* stream);

/* ---- mask statistics on the device -------------------------------------------
 * From a uint8 class-index mask [B,H,W] (e.g. the dev_mask of a forward): per-frame class pixel counts
 * (np.sum(mask_cable) / coverage, infer_two_stage_burr.py:333-340, src/utils/geometry_enhanced.py:151-152) and,
 * per class and row, the first and last column of that class — the operands of _compute_width_per_row
 * (geometry_enhanced.py:45-74: width = xs.max() - xs.min() + 1).  The reference's Gaussian smoothing of these widths
 * is unetpp_width_profile, its connected-component filtering unetpp_components_filter, both below.
 *   dev_counts   uint32 [B,num_classes]      (zeroed by this call)
 *   dev_row_min  int32  [B,num_classes,H]    W  when the row has no pixel of the class
 *   dev_row_max  int32  [B,num_classes,H]    -1 when the row has no pixel of the class
 * Asynchronous on `stream`. */
int unetpp_mask_stats(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, uint32_t* dev_counts,
                      int32_t* dev_row_min, int32_t* dev_row_max, void* stream);

/* ---- connected components and the reference's component filters on the device ---------------------------------
 * What every frame loop of the reference does next with a class mask is cv2.connectedComponentsWithStats(mask,
 * connectivity=8) followed by a choice among the components (src/utils/geometry_enhanced.py:81-110 and :275-311,
 * src/refactor/postprocess.py:12-76 and :106-116, infer_video_spatial.py:24-53).
 *
 * unetpp_components labels B frames.  dev_mask is uint8 [B,h,w] (any h, w >= 1, h * w <= 2^30, h, w <= 65535);
 * foreground = (mask == match_class), or (mask != 0) for match_class < 0; connectivity is 4 or 8.
 *   dev_labels  int32 [B,h,w]         0 = background, components 1..n NUMBERED IN RASTER ORDER OF THEIR FIRST PIXEL
 *                                     (row-major, per frame): scipy.ndimage.label's order.  cv2's own numbering is an
 *                                     artefact of its block-based algorithm and is not reproduced; the reference depends
 *                                     on it only to break ties between components of equal area / score, which here go
 *                                     to the lower label.
 *   dev_num     int32 [B]             n + 1 like cv2's num_labels (the background counts); exact whatever `capacity`
 *   dev_stats   int32 [B,capacity,5]  cv2's columns LEFT, TOP, WIDTH, HEIGHT, AREA; row = label, row 0 = background;
 *                                     rows >= num (and a background without pixels) are zero
 *   dev_sums    uint64 [B,capacity,2] sum of x, sum of y over the label's pixels: cv2's double centroids are
 *                                     sums / area in one correctly rounded division
 * dev_stats and dev_sums may both be NULL (labels and num only).  `capacity` (>= 2) is the number of rows: labels and
 * num are exact for any number of components, stats and sums hold labels 0 .. capacity - 1.  The worst case is
 * h * w / 2 components (a checkerboard at connectivity 4), real masks stay in the low thousands.
 * All results are integers and every component is rooted at its smallest pixel index, so they are bitwise the same
 * from run to run.  dev_workspace: unetpp_components_workspace_bytes(batch, h, w, capacity) bytes (0 for bad
 * arguments), 16-byte aligned, owned by the caller; nothing is allocated per call and the engine's activation
 * workspace is not touched.  Asynchronous on `stream`.
 *
 * unetpp_components_filter writes dev_out uint8 [B,h,w] = out_value where the pixel's component is kept, else 0,
 * from the outputs of unetpp_components (same batch, h, w, capacity and workspace).  All arithmetic in fp64 without
 * contraction, as the reference's NumPy / Python expressions evaluate:
 *   UNETPP_CC_LARGEST      _largest_connected_component(mask, min_area), geometry_enhanced.py:81-110: the first
 *                          (lowest label) of the largest components with area >= min_area, nothing if there is none;
 *                          min_area = 0 is the tail of constrain_tape_to_ring, postprocess.py:106-116
 *   UNETPP_CC_SPATIAL      spatial_filter, infer_video_spatial.py:24-53: every component with area > min_area and
 *                          min_width <= width <= max_width and height >= h * min_height_ratio
 *   UNETPP_CC_CABLE_SHAPE  filter_cable_by_shape, postprocess.py:12-76: area >= min_area,
 *                          aspect = max(w,h) / (min(w,h) + 1e-6) >= min_aspect,
 *                          offset = |cx - roi_width / 2| / roi_width <= max_center_offset; the first of the highest
 *                          score = area * aspect * (1 - offset) is kept (out_value 255 in the reference)
 * A frame with num > capacity cannot be decided from truncated stats: its output is all zero; callers compare
 * dev_num with capacity.  Errors: UNETPP_E_INVALID for connectivity other than 4 / 8, capacity < 2, a bad shape or
 * rule, NULL where not allowed, exactly one of dev_stats / dev_sums NULL. */
enum { UNETPP_CC_LARGEST = 0, UNETPP_CC_SPATIAL = 1, UNETPP_CC_CABLE_SHAPE = 2 };

typedef struct unetpp_cc_rule {
  double min_area;           /* all rules (reference defaults: 100 / 1000 / 1000) */
  double min_width;          /* SPATIAL (50) */
  double max_width;          /* SPATIAL (300) */
  double min_height_ratio;   /* SPATIAL (0.3) */
  double min_aspect;         /* CABLE_SHAPE (1.6) */
  double max_center_offset;  /* CABLE_SHAPE (0.3) */
  double roi_width;          /* CABLE_SHAPE: the ROI's width in pixels, > 0 */
} unetpp_cc_rule;

size_t unetpp_components_workspace_bytes(int batch, int h, int w, int capacity);
int unetpp_components(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, int match_class,
                      int connectivity, int capacity, int32_t* dev_labels, int32_t* dev_num, int32_t* dev_stats,
                      uint64_t* dev_sums, void* dev_workspace, void* stream);
int unetpp_components_filter(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num,
                             const int32_t* dev_stats, const uint64_t* dev_sums, int batch, int h, int w,
                             int capacity, int rule, const unetpp_cc_rule* params, uint8_t out_value,
                             uint8_t* dev_out, void* dev_workspace, void* stream);

/* ---- stage-2 burr detection on the device: grey, blur, Canny, Laplacian band, box rule -----------------------------
 * What the reference's frame loop does after every segmentation: detect_burrs_on_cable(frame_gray, mask_cable, cfg)
 * (infer_two_stage_burr.py:50-119 and :317-318, infer_high_res_custom_roi.py:50-93) and its Laplacian variant
 * get_burr_mask_rulebased (src/refactor/burr_detector.py:11-66).  Their band, close / open and component steps are
 * unetpp_morphology and unetpp_components above; the entries here are the grey-level steps and the final choice.
 * All arithmetic is integer and restated from OpenCV's published algorithms (unet_amd/edges.py is the NumPy form);
 * cv2 itself is not available to the tests, so its own output stays unpinned.  Everything is asynchronous on `stream`.
 *
 * Shapes: uint8 [B,h,w] images on the device.  unetpp_gaussian_blur_u8 and unetpp_canny_u8 need 8 <= h, w <= 65535 and
 * h * w <= 2^30 (UNETPP_E_UNSUPPORTED beyond, UNETPP_E_INVALID for a shape below 1), any size in between.
 *
 * unetpp_gray_u8: cv2.cvtColor(frame, COLOR_BGR2GRAY) (burr_detector.py:27-28) for uint8 [B,h,w,3]:
 *   (3735 B + 19235 G + 9798 R + 16384) >> 15, OpenCV 4's 15-bit constants (3.x used a 14-bit set).
 *
 * unetpp_gaussian_blur_u8: cv2.GaussianBlur(gray, (k, k), sigma) (infer_two_stage_burr.py:85) with the kernel given as
 * `taps`: n_taps (odd, <= 7: UNETPP_E_UNSUPPORTED above) integers with 8 fractional bits that sum to 256
 * (UNETPP_E_INVALID otherwise), read from HOST memory during the call.  Horizontal pass into a 16-bit 8.8 value,
 * vertical pass into 32 bits, (acc + 32768) >> 16; BORDER_REFLECT_101 on both axes.  A caller holding cv2's own
 * fixed-point kernel passes it here.  dev_out must not overlap dev_gray.
 *
 * unetpp_canny_u8: cv2.Canny(blurred, low, high) (infer_two_stage_burr.py:86; L2gradient off, aperture 3), with the
 * blur fused when taps != NULL (taps == NULL: dev_gray is used as it is).  3x3 Sobel with BORDER_REPLICATE of the
 * blurred image, mag = |dx| + |dy|, 0 outside the image; candidate if mag > floor(low) and it passes the non-maximum
 * test along its direction (TG22 = 13573 in 15 bits: with x = |dx|, y = |dy| << 15: y < x TG22 horizontal,
 * m > left && m >= right; y > x TG22 + (x << 16) vertical, m > up && m >= down; otherwise the diagonal chosen by the
 * sign of dx ^ dy, strict on both sides); strong if mag > floor(high).  dev_out uint8 [B,h,w] = 255 on every candidate
 * that is 8-connected to a strong pixel through candidates, else 0.  low > high swaps them, as cv2 does.  The
 * hysteresis is not iterated: the candidates are labelled with the launches of unetpp_components and a flag per root
 * pixel decides, so the result is the same bits from run to run and no component count limits it.
 * dev_workspace: unetpp_canny_workspace_bytes(batch, h, w) bytes (0 for bad arguments), 16-byte aligned, the
 * caller's; nothing is allocated per call.  unetpp_canny_layout reports the core rows x columns of one workgroup's
 * tile (no engine, no device needed); tests aim at these seams, callers need not care.
 *
 * unetpp_laplacian_band_u8: burr_detector.py:44-51 in one launch: dev_out = 255 where dev_band != 0 and
 * (|L| & 255) > threshold, else 0, with L = cv2.Laplacian(gray, CV_64F) = 4 neighbours - 4 centre under
 * BORDER_REFLECT_101.  `& 255` is what the reference's np.abs(L).astype(np.uint8) does to the values above 255
 * (300 -> 44); it is the reference's behaviour and is reproduced.  h, w >= 2.  dev_out must not overlap dev_gray.
 *
 * unetpp_components_filter_box: the loop of infer_two_stage_burr.py:100-117 (and burr_detector.py:53-64 with
 * max_aspect = infinity, min_side = 0) from the outputs of unetpp_components (same batch, h, w, capacity,
 * workspace): keeps EVERY component with min_area <= area <= max_area and
 * max(w,h) / (min(w,h) + 1e-6) < max_aspect (fp64, no contraction) and w > min_side and h > min_side.
 * As for unetpp_components_filter, a frame with num > capacity gives all zero. */
typedef struct unetpp_cc_box_rule {
  double min_area;           /* 30 */
  double max_area;           /* 800 */
  double max_aspect;         /* 5.0 */
  double min_side;           /* 3 */
} unetpp_cc_box_rule;

int unetpp_gray_u8(unetpp_engine* e, const uint8_t* dev_bgr, int batch, int h, int w, uint8_t* dev_gray, void* stream);
int unetpp_gaussian_blur_u8(unetpp_engine* e, const uint8_t* dev_gray, int batch, int h, int w, const int32_t* taps,
                            int n_taps, uint8_t* dev_out, void* stream);
size_t unetpp_canny_workspace_bytes(int batch, int h, int w);
int unetpp_canny_layout(int h, int w, int* tile_rows, int* tile_cols);
int unetpp_canny_u8(unetpp_engine* e, const uint8_t* dev_gray, int batch, int h, int w, const int32_t* taps, int n_taps,
                    double low, double high, uint8_t* dev_out, void* dev_workspace, void* stream);
int unetpp_laplacian_band_u8(unetpp_engine* e, const uint8_t* dev_gray, const uint8_t* dev_band, int batch, int h, int w,
                             int threshold, uint8_t* dev_out, void* stream);
int unetpp_components_filter_box(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num,
                                 const int32_t* dev_stats, int batch, int h, int w, int capacity,
                                 const unetpp_cc_box_rule* params, uint8_t out_value, uint8_t* dev_out,
                                 void* dev_workspace, void* stream);

/* ---- binary morphology programs on the device ------------------------------------------------------------------
 * cv2.dilate / cv2.erode / cv2.morphologyEx (OPEN, CLOSE) with a structuring element on class masks, and the short
 * programs the reference builds from them (src/refactor/postprocess.py:79-118 and :144-166,
 * src/utils/geometry_enhanced.py:281-289, src/refactor/burr_detector.py:37-41, infer_two_stage_burr.py:78-79), each
 * program in ONE kernel launch.  Everything is boolean: results are exact.
 *
 * Masks are uint8 [B,h,w] on the device, any h, w >= 1 (h, w <= 65535, h * w <= 2^30).  Foreground of dev_mask0 is
 * (mask == match0), or (mask != 0) for match0 < 0; likewise dev_mask1 / match1.  dev_mask1 may be NULL.
 *
 * Semantics (OpenCV's published definition; cv2 itself is not available to the tests, so its own output stays
 * unpinned).  An element is uint8 [kh,kw], row-major in HOST memory (read during the call), with anchor (ax, ay);
 * ax = -1 / ay = -1 mean kw / 2 and kh / 2.
 *   dilate: dst(x,y) = OR  over (i,j) with elem[i][j] != 0 of src(x + j - ax, y + i - ay)
 *   erode:  dst(x,y) = AND over (i,j) with elem[i][j] != 0 of src(x + j - ax, y + i - ay)
 * The element is NOT reflected (this differs from scipy.ndimage.binary_dilation for an asymmetric element such as
 * cv2's ELLIPSE (8,8)).  Pixels outside the image do not contribute: they count as 0 for a dilate and as 1 for an
 * erode, at every step and every iteration (BORDER_CONSTANT with morphologyDefaultBorderValue).  iterations = n
 * repeats the step n times.  cv2 replaces n iterations of a RECT element by one pass with an enlarged element and a
 * scaled anchor, which differs for an anchor off the centre: that shortcut is not imitated and stays unpinned.
 *
 * Planes: P0 = fg(dev_mask0), P1 = fg(dev_mask1) (all zero for NULL), P2 and P3 scratch.  A program is at most 8
 * steps {op, dst, a, b, element, iterations}:
 *   UNETPP_MORPH_DILATE / _ERODE   P[dst] = op^iterations(P[a]) with elements[element]   (b unused)
 *   UNETPP_MORPH_AND / _ANDNOT / _OR   P[dst] = P[a] & P[b] / P[a] & ~P[b] / P[a] | P[b]  (element, iterations unused)
 *   UNETPP_MORPH_COPY                  P[dst] = P[a]
 * dst may be any plane, a or b included.  dev_out uint8 [B,h,w] = out_value where P[result_plane] is set, else 0.
 * open = ERODE then DILATE, close = DILATE then ERODE (cv2.morphologyEx, each with the same iterations).
 *
 * Limits: at most 4 elements, each at most 63 x 63 and ROW-CONVEX (the non-zeros of every row form one run: rect,
 * cross and every ellipse are); the sum of iterations * (kh - 1) over the program's dilates and erodes at most 126,
 * and the same for kw (a close with one 63 x 63 element, or close(E5, iterations=2) then dilate(E3), fit).
 * Beyond these: UNETPP_E_UNSUPPORTED, never a wrong result.  UNETPP_E_INVALID for NULL dev_mask0 / dev_out, a bad
 * shape, op, plane or element index, a step or result_plane reading a scratch plane no earlier step wrote,
 * iterations < 1, an empty element, an anchor outside the element, and dev_out overlapping an input mask
 * (workgroups read halo rows their neighbours write).  After an error dev_out is untouched.
 * No allocation, no device workspace; program and elements travel as kernel arguments.  Asynchronous on `stream`.
 *
 * unetpp_morphology_layout reports how the kernel tiles a program (no engine, no device needed): band_rows = rows
 * of a frame one workgroup owns, tile_cols = its columns (a multiple of 64, >= w when rows are not split).  Tests
 * aim at these boundaries; callers need not care. */
enum { UNETPP_MORPH_DILATE = 0, UNETPP_MORPH_ERODE = 1, UNETPP_MORPH_AND = 2, UNETPP_MORPH_ANDNOT = 3,
       UNETPP_MORPH_OR = 4, UNETPP_MORPH_COPY = 5 };

typedef struct unetpp_morph_element {
  int kw, kh;                /* 1..63 each */
  int ax, ay;                /* anchor, 0 <= ax < kw, 0 <= ay < kh; -1 = centre (k / 2) */
  const uint8_t* host_data;  /* [kh,kw], row-major, non-zero = member */
} unetpp_morph_element;

typedef struct unetpp_morph_step {
  int op, dst, a, b, element, iterations;
} unetpp_morph_step;

int unetpp_morphology(unetpp_engine* e, const uint8_t* dev_mask0, int match0, const uint8_t* dev_mask1, int match1,
                      int batch, int h, int w, const unetpp_morph_element* elements, int n_elements,
                      const unetpp_morph_step* steps, int n_steps, int result_plane, uint8_t out_value,
                      uint8_t* dev_out, void* stream);
int unetpp_morphology_layout(int batch, int h, int w, const unetpp_morph_element* elements, int n_elements,
                             const unetpp_morph_step* steps, int n_steps, int* band_rows, int* tile_cols);

/* ---- frame glue either side of the model --------------------------------
 * unetpp_resize_linear_u8 replaces `cv2.resize(frame_rgb, target_size, interpolation=cv2.INTER_LINEAR)`
 * of preprocess_image (infer_two_stage_burr.py:124; also the --normalize-resolution resize, :281):
 *   dev_src uint8 [B,src_h,src_w,channels] interleaved (channels 1..4)  ->  dev_dst uint8 [B,dst_h,dst_w,channels]
 * OpenCV's published fixed-point algorithm (11-bit coefficients; see oracle/unetpp_oracle.py
 * cv2_resize_linear_u8_np — parity unpinned: cv2 is not installable in the build environment).
 * The result feeds unetpp_forward(_ex) with UNETPP_IN_U8_NHWC_BGR, which does BGR->RGB, /255 and the layout change.
 *
 * unetpp_resize_nearest_roi_u8 replaces infer_two_stage_burr.py:303-314 for one class:
 *   (pred == match_class).astype(uint8)  [match_class < 0: the mask itself]
 *   -> cv2.resize(mask, (dst_w, dst_h), interpolation=cv2.INTER_NEAREST)
 *   -> zeros outside rows [y1, y2) x columns [x1, x2) (Python slice semantics for non-negative bounds; pass
 *      0, 0, dst_w, dst_h for "no ROI").
 *   dev_src uint8 [B,src_h,src_w]  ->  dev_dst uint8 [B,dst_h,dst_w]
 * Both are asynchronous on `stream`, except that the first call for a new (source, destination) extent builds
 * the index tables on the host and uploads them with a blocking copy. */
int unetpp_resize_linear_u8(unetpp_engine* e, const uint8_t* dev_src, int batch, int src_h, int src_w, int channels,
                            uint8_t* dev_dst, int dst_h, int dst_w, void* stream);
int unetpp_resize_nearest_roi_u8(unetpp_engine* e, const uint8_t* dev_src, int batch, int src_h, int src_w,
                                 int match_class, uint8_t* dev_dst, int dst_h, int dst_w, int x1, int y1, int x2,
                                 int y2, void* stream);

/* Bytes of device memory held by the engine (workspace + packed weights). */
size_t unetpp_workspace_bytes(const unetpp_engine* e);

/* ---- measurement hooks (bench.py roofline leg) ------------------------------------------------
 * With profiling on, every kernel launch of the next forward is bracketed by HIP events recorded
 * on the launch stream.  unetpp_profile_read synchronises those events and returns, per launch in
 * issue order, its duration in milliseconds; unetpp_profile_name gives the launch's label. */
int unetpp_profile_enable(unetpp_engine* e, int on);
int unetpp_profile_count(const unetpp_engine* e);
int unetpp_profile_read(unetpp_engine* e, float* ms_out, int n);
const char* unetpp_profile_name(const unetpp_engine* e, int i);
/* algorithmic FLOPs and minimum HBM bytes (read+write) of launch i for the last forward's shape */
int unetpp_profile_work(const unetpp_engine* e, int i, double* flops, double* bytes);
/* the launch plan of launch i: out = {grid (workgroups), tiles (split-K shares counted), ksplit, rows per wave}; all 0 for a
 * launch that is not persistent (one workgroup per tile), rows per wave 0 for the low-resolution GEMM */
int unetpp_profile_plan(const unetpp_engine* e, int i, int out[4]);

/* ---- debug (layer-by-layer parity tests) -------------------------------------------------------
 * Copies the named activation of the LAST micro-batch processed ("x0_0", "x1_0", ..., "x0_4"; also a block's first conv
 * "x1_0a" and a pooled tensor "x1_0p" [b,C,h/2,w/2]) to host memory as float32 [b,C,h,w]; returns the number of floats
 * written or a negative error.  "name#hi", "name#lo", "name#x8" give one stored plane instead of the reconstructed value
 * (fp16 hi; fp16 lo, or EXACT8's decoded e5m2(2^8 lo); EXACT8's decoded e5m2(2^-3 v)). */
long long unetpp_debug_read(unetpp_engine* e, const char* name, float* host_out, size_t max_floats);

/* x0_4 is normally never written to HBM (the 1x1 head + argmax run in the epilogue of conv0_4.conv2).
 * With on != 0 the next forwards materialise it and run the head as a separate kernel, so that
 * unetpp_debug_read("x0_4") works. */
int unetpp_debug_keep_intermediates(unetpp_engine* e, int on);

/* ---- the multi-scale and the DoG burr detectors, has_burr ---------------------------------------------------------
 * The grey-level steps of detect_burrs_enhanced (infer_enhanced_burr.py:87-106), get_burr_mask_dog
 * (src/refactor/burr_detector.py:93-103) and has_burr (:121-133); their mask-side steps are unetpp_morphology,
 * unetpp_components and unetpp_components_filter_box.  All integer, exact; images uint8 [B,h,w] on the device with the
 * shape limits and status codes of unetpp_canny_u8 (8 <= h, w <= 65535, h * w <= 2^30: UNETPP_E_UNSUPPORTED beyond).
 * Asynchronous on `stream`; nothing is allocated.
 *
 * unetpp_edges_union_u8: dev_out = dev_canny | sobel | laplacian, bytewise, where
 *   sobel     = 255 where uint8(sqrt(s) / sqrt(max s over the frame) * 255) > sobel_threshold (float64, truncating),
 *               s = dx^2 + dy^2 of cv2.Sobel(ksize = 3) on the raw grey image with BORDER_REFLECT_101.  A constant frame
 *               (max s = 0; 0 / 0 in the reference) has no Sobel edges.
 *   laplacian = 255 where (|cv2.Laplacian(ksize = 1)| & 255) > laplacian_threshold (the reference's uint8 cast wraps).
 *   dev_workspace: unetpp_edges_union_workspace_bytes(batch) bytes (0 for a bad batch), 16-byte aligned; it holds the
 *   per-frame maximum between the two launches.  dev_out may be dev_canny itself (in place), not dev_gray.
 *   Thresholds are those of cv2.threshold on uint8: below 0 everything passes, from 255 on nothing.
 *
 * unetpp_dog_band_u8: dev_out = 255 where dev_band != 0 and cv2.subtract(blur1, blur2) > threshold, else 0; blur1 and
 *   blur2 are unetpp_gaussian_blur_u8 with taps1[n1] and taps2[n2] (host memory; odd, at most 7, in [0,256], sum 256).
 *   The subtraction saturates at 0.  dev_out may alias neither input.
 *
 * unetpp_count_nonzero_u8: dev_counts uint32 [B] = number of non-zero bytes of each frame (any h, w >= 1). */
size_t unetpp_edges_union_workspace_bytes(int batch);
int unetpp_edges_union_u8(unetpp_engine* e, const uint8_t* dev_gray, const uint8_t* dev_canny, int batch, int h, int w,
                          int sobel_threshold, int laplacian_threshold, void* dev_workspace, uint8_t* dev_out,
                          void* stream);
int unetpp_dog_band_u8(unetpp_engine* e, const uint8_t* dev_gray, const uint8_t* dev_band, int batch, int h, int w,
                       const int32_t* taps1, int n1, const int32_t* taps2, int n2, int threshold, uint8_t* dev_out,
                       void* stream);
int unetpp_count_nonzero_u8(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, uint32_t* dev_counts,
                            void* stream);

/* ---- measurements on the device: diameters, thickness profile, defect summary ---------------------------------------
 * The step the reference's production loop ends in (infer_video_production.py:198-226): compute_diameter_metrics,
 * compute_thickness_profile and analyze_defects (src/utils/geometry_enhanced.py:113-330) and
 * diameter_profile_from_masks (src/utils/geometry.py:28-64).  Their component filters, hole mask and labelling are
 * unetpp_components(_filter) and unetpp_morphology above; the entries here are what is left: widths per row, their
 * smoothing, the valid rows and medians, and the reduction of a statistics table.  unet_amd/geometry.py is the NumPy
 * form.  All three are asynchronous on `stream` and allocate nothing.
 *
 * unetpp_row_widths: _compute_width_per_row(smooth=False) (geometry_enhanced.py:61-67; _width_per_row, geometry.py:7-18)
 * of two binary planes, and the mask.sum() behind the coverages (geometry_enhanced.py:152-153, :271).  Planes as for
 * unetpp_morphology: foreground of dev_mask0 is (mask == match0), or (mask != 0) for match0 < 0; likewise dev_mask1 /
 * match1.  The two pointers may be the same tensor (cable and tape of one class mask); dev_mask1 may be NULL (plane 1
 * is then empty).  Masks uint8 [B,h,w], any 1 <= h, w <= 65535.
 *   dev_widths float32 [B,2,h] = last - first + 1 over the foreground columns of the row, 0 for an empty row
 *                               (integers <= 65535: exact)
 *   dev_area   uint32  [B,2]   = foreground pixels of each plane (zeroed by the call on the same stream)
 *
 * unetpp_width_profile: the rest of compute_diameter_metrics / compute_thickness_profile (geometry_enhanced.py:144-168,
 * :211-219) for dev_widths float32 [B,2,h], h <= 4096 (UNETPP_E_INVALID above: one workgroup holds a frame's widths).
 *   smoothing  cv2.GaussianBlur(widths.reshape(-1, 1), (1, k), sigmaX=0) with the kernel given as `taps`: n_taps (odd,
 *              1..127) float32 values in HOST memory (read during the call), finite and symmetric.  BORDER_REFLECT_101
 *              (cv2.borderInterpolate, with its loop for h <= n_taps / 2).  OpenCV's symmetric column filter, every
 *              operation rounded to float32, no contraction, r = n_taps / 2:
 *                s = taps[r] * w[y];  for j = 1 .. r ascending:  s = s + taps[r + j] * (w[y + j] + w[y - j])
 *              n_taps = 1 with taps[0] = 1 is the identity.  cv2's own kernel values and the summation order of its
 *              SIMD paths are not pinned by this project's tests.
 *   dev_smoothed float32 [B,2,h]  the smoothed widths
 *   dev_valid    uint8   [B,h]    smoothed plane 0 > 0 && smoothed plane 1 > 0
 *   dev_delta    float32 [B,h]    smoothed plane 1 - smoothed plane 0; may be NULL
 *   dev_out      [B] records      valid_rows = the number of valid rows; when valid_rows >= min_valid_rows, dc_px / dt_px =
 *                                 np.median of smoothed plane 0 / 1 over the valid rows as a float32 array forms it (the
 *                                 middle element; for an even count (a + b) rounded to float32, then halved); otherwise
 *                                 both are 0, the reference's early return.  min_valid_rows >= 1 (UNETPP_E_INVALID for
 *                                 0: the reference would take the median of nothing).
 *
 * unetpp_components_summary: the reductions analyze_defects makes of a statistics table (geometry_enhanced.py:291-294,
 * :302-309) from dev_num [B] and dev_stats [B,capacity,5] of unetpp_components.  dev_out int64 [B,4]:
 *   [0] max(0, num - 1), the component count; exact even when num > capacity
 *   [1] the number of labels 1 .. min(num, capacity) - 1 with area >= min_area
 *   [2] the sum of those areas
 *   [3] the largest area of any of these labels (0 when there is none)
 * dev_stats may be NULL (unetpp_components run without stats): [1..3] are then 0.
 *
 * Errors: UNETPP_E_INVALID for a bad shape, an even n_taps, n_taps > 127, taps that are not finite or not symmetric,
 * min_valid_rows < 1, capacity < 2, NULL where not allowed. */
typedef struct unetpp_width_profile_out {
  float dc_px, dt_px;
  int32_t valid_rows;
} unetpp_width_profile_out;

int unetpp_row_widths(unetpp_engine* e, const uint8_t* dev_mask0, int match0, const uint8_t* dev_mask1, int match1,
                      int batch, int h, int w, float* dev_widths, uint32_t* dev_area, void* stream);
int unetpp_width_profile(unetpp_engine* e, const float* dev_widths, int batch, int h, const float* taps, int n_taps,
                         int min_valid_rows, float* dev_smoothed, uint8_t* dev_valid, float* dev_delta,
                         unetpp_width_profile_out* dev_out, void* stream);
int unetpp_components_summary(unetpp_engine* e, const int32_t* dev_num, const int32_t* dev_stats, int batch, int capacity,
                              int64_t min_area, int64_t* dev_out, void* stream);

/* ---- the robust loop's mask rules on the device: distance transform + ring, best cable, ROI limit, row median ----------
 * What infer_video_robust.py does with its two masks after exclusive_threshold (:102-216, :325-387).  unet_amd/robust.py
 * is the NumPy form.  Every launching entry is asynchronous on `stream` and allocates nothing.  Every bad argument except
 * a NULL engine is answered with UNETPP_E_UNSUPPORTED.
 *
 * unetpp_distance_transform_u8: cv2.distanceTransform(img, DIST_L2 | DIST_L1 | DIST_C, 3) (OpenCV's published
 * distanceTransform_3x3), bit for bit.  A pixel of img is non-zero where dev_src is foreground (== match_class, or != 0
 * for match_class < 0), or with invert != 0 where it is NOT -- so `(mask_cable == 0)` needs no launch of its own.
 * Arithmetic: t = the smallest chamfer path length to a zero pixel in 16.16 fixed point with the weights (HV, DIAG) =
 * (62587, 89738) for UNETPP_DIST_L2, (65536, 131072) for _L1, (65536, 65536) for _C; t = min(t, INT_MAX >> 2);
 * distance = (float)t * (1.f / 65536).  A frame without a zero pixel is 8192.0 everywhere.  Any 1 <= h, w <= 65535 with
 * h * w <= 2^30, any alignment of the masks.
 *   dev_dist   float32 [B,h,w]  the distance map; may be NULL
 *   dev_ring   uint8   [B,h,w]  out_value where lo <= distance <= hi (float32 comparisons) and the pixel of img is
 *                               non-zero and dev_mask1 is foreground (match1 as above; dev_mask1 NULL: no such
 *                               condition), 0 elsewhere; may be NULL, but not together with dev_dist.  With dev_dist
 *                               NULL the search is cut off just beyond hi, so its cost follows the band's width.
 *   dev_workspace  unetpp_distance_workspace_bytes(batch, h, w) bytes (0 for a shape outside the limits), 16-byte aligned
 *
 * unetpp_components_best_cable: keep_best_cable_cc (:102-160) on the labels, num and stats of unetpp_components.  In
 * label order a component is rejected when area < min_area, then h < min_h, then w > max_w, then
 * aspect = h / (w + 1e-6) < min_aspect; score = (h / H) * 3.0 + min(aspect, 12.0) * 0.5 + (area / (H * W)) * 0.5 in
 * float64 without contraction; the first component with the strictly greatest score is written as out_value into dev_out
 * uint8 [B,h,w], everything else 0 (all 0 when none qualifies or num > capacity).  min_h / max_w are the reference's
 * int(min_h_ratio * H) / int(max_w_ratio * W), formed by the caller.  dev_workspace: the one of unetpp_components.
 *
 * unetpp_roi_limit_u8: apply_roi_limit (:201-216).  The bounding box of the non-zero pixels of dev_cable per frame, padded
 * by pad >= 0 and clipped to the frame; dev_out = dev_mask inside it and 0 outside, all 0 when the cable is empty.
 * dev_out may be dev_mask itself.  dev_workspace: unetpp_roi_limit_workspace_bytes(batch) bytes, 4-byte aligned.
 *
 * unetpp_row_width_median: calc_width of _measure_diameters (:372-387) from dev_widths float32 [B,2,h] of
 * unetpp_row_widths: dev_median float64 [B,2] = np.median of the widths above 1 (a row has more than one foreground pixel
 * exactly when last - first + 1 > 1): the middle value, the mean of the two middle ones for an even count, 0 for none. */
enum { UNETPP_DIST_L1 = 1, UNETPP_DIST_L2 = 2, UNETPP_DIST_C = 3 };   /* cv2.DIST_L1, DIST_L2, DIST_C */

size_t unetpp_distance_workspace_bytes(int batch, int h, int w);
int unetpp_distance_transform_u8(unetpp_engine* e, const uint8_t* dev_src, int match_class, int invert, int batch, int h, int w,
                                 int metric, float* dev_dist, const uint8_t* dev_mask1, int match1, float lo, float hi,
                                 uint8_t out_value, uint8_t* dev_ring, void* dev_workspace, void* stream);
int unetpp_components_best_cable(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num, const int32_t* dev_stats,
                                 int batch, int h, int w, int capacity, double min_area, int min_h, int max_w, double min_aspect,
                                 uint8_t out_value, uint8_t* dev_out, void* dev_workspace, void* stream);
size_t unetpp_roi_limit_workspace_bytes(int batch);
int unetpp_roi_limit_u8(unetpp_engine* e, const uint8_t* dev_mask, const uint8_t* dev_cable, int batch, int h, int w, int pad,
                        uint8_t* dev_out, void* dev_workspace, void* stream);
int unetpp_row_width_median(unetpp_engine* e, const float* dev_widths, int batch, int h, double* dev_median, void* stream);

/* ---- sliding-window inference on the device: gather tiles, gate, blend -------------------------------------------------
 * SlidingWindowInference.predict (tools/inference_binary_patch.py:19-115) and OptimizedSlidingWindowInference.predict
 * (tools/inference_binary_optimized.py:21-113) around the network: cut frames into overlapping patch_size squares,
 * resize each to the network's size t, and fold the network's per-patch maps back into one image.  unet_amd/tiling.py
 * is the NumPy form and builds the plan.  The plan is separable: patch (i, j) has its top-left corner at
 * (origins_y[i], origins_x[j]) and index i * n_x + j inside its frame (the reference's loop order); both arrays are in
 * HOST memory, read during the call, 1 <= n_y, n_x <= 64 (UNETPP_E_UNSUPPORTED above).  All three calls are asynchronous
 * on `stream`; the first call with a new (patch_size, t) pair builds two small device tables and synchronises once.
 *
 * unetpp_tile_gather_u8: dev_frames uint8 [B,h,w,3] -> dev_patches uint8 [B * n_y * n_x, t, t, 3] in one launch:
 *   crop    source index s of a patch maps to image coordinate origin + s;
 *   pad     np.pad(mode="reflect") at the bottom and right: a coordinate k >= h reads 2 (h - 1) - k.  Every origin must
 *           satisfy 0 <= origin < h and origin + patch_size - 1 <= 2 (h - 1) (likewise for w): padding of h or more is
 *           UNETPP_E_UNSUPPORTED;
 *   resize  cv2.resize(patch, (t, t), INTER_LINEAR) for uint8, the arithmetic of unetpp_resize_linear_u8; t ==
 *           patch_size is the identity; t a multiple of 4;
 *   channel_order  UNETPP_TILE_BGR copies the channels, UNETPP_TILE_RGB reverses them, so that either way the patches
 *           are BGR, which UNETPP_IN_U8_NHWC_BGR expects.
 *
 * unetpp_tile_gate_f32: the window gate (inference_binary_optimized.py:91-98) for dev_maps float32 [n, classes, t, t]:
 *   dev_scores float32 [n] = the maximum over the patch of class gate_class; dev_include uint8 [n] = score >= gate_thr
 *   (both float32).  t a multiple of 2, dev_maps 16-byte aligned.
 *
 * unetpp_tile_blend_f32: dev_maps float32 [B * n_y * n_x, classes, t, t] -> dev_mask uint8 [B,h,w] and, unless NULL,
 *   dev_output float32 [B,h,w,classes].  Per pixel, for every patch that covers it (and whose dev_include byte is
 *   non-zero; dev_include may be NULL), in plan order: the sample of cv2.resize(map, (patch_size, patch_size),
 *   INTER_LINEAR) at the patch-local coordinate, with float coefficients 1 - fx and fx: horizontal S[s0] * a0 + S[s1] *
 *   a1 on the two source rows, then the vertical pass, every product and sum rounded to float32; added to a float32
 *   accumulator per class.  Then acc / (count + 1e-8f) (IEEE division; count is the number of patches added) and the
 *   first maximum over the classes.  A pixel no included patch covers gives 0 and class 0.  The order is fixed per pixel,
 *   so there are no atomics and the bits do not depend on scheduling.  1 <= classes <= 8 (UNETPP_E_UNSUPPORTED above).
 *
 * Errors: UNETPP_E_INVALID for NULL where not allowed, a bad shape, an origin outside the frame, a bad gate_class or
 * channel_order.  No kernel is launched when an error is returned. */
enum { UNETPP_TILE_BGR = 0, UNETPP_TILE_RGB = 1 };

int unetpp_tile_gather_u8(unetpp_engine* e, const uint8_t* dev_frames, int batch, int h, int w, const int32_t* origins_y,
                          int n_y, const int32_t* origins_x, int n_x, int patch_size, int t, int channel_order,
                          uint8_t* dev_patches, void* stream);
int unetpp_tile_gate_f32(unetpp_engine* e, const float* dev_maps, int n, int classes, int t, int gate_class, float gate_thr,
                         float* dev_scores, uint8_t* dev_include, void* stream);
int unetpp_tile_blend_f32(unetpp_engine* e, const float* dev_maps, int batch, int classes, int t, const int32_t* origins_y,
                          int n_y, const int32_t* origins_x, int n_x, int patch_size, const uint8_t* dev_include, int h, int w,
                          uint8_t* dev_mask, float* dev_output, void* stream);

/* ---- grey-frame enhancement in front of the network: decision, CLAHE, gamma, bilateral filter --------------------------
 * preprocess_frame of the refactored loop (src/refactor/preprocess.py:12-91, infer_video_refactored.py:346) with
 * PreprocessConfig's defaults (src/refactor/config.py:44-52): is_grayscale_frame, then for a grey frame
 * cv2.cvtColor(BGR2GRAY), cv2.createCLAHE(clip, (tiles, tiles)).apply, a 256-entry gamma table, cv2.bilateralFilter(d, 75,
 * 75) and GRAY2BGR; a colour frame is copied.  unet_amd/enhance.py is the NumPy form, restated from OpenCV's published
 * algorithms, and every result equals it bit for bit; cv2's own results are not pinned by this project's tests.
 * Images uint8 on the device, 1 <= h, w <= 65535, h * w <= 2^30.  Everything is asynchronous on `stream`, allocates
 * nothing and never synchronises with the host: the grey / colour decision stays on the device.
 *
 * unetpp_gray_decision: dev_frames uint8 [B,h,w,3] -> dev_sums uint64 [B,3] = the sums of |b - g|, |g - r|, |r - b|
 *   (8-byte aligned; zeroed by the call) and dev_decisions uint8 [B] = (max(sums) / (h w) < threshold), one double
 *   division of exact integers: what np.abs(...).mean() < threshold yields.
 *
 * unetpp_clahe_u8: OpenCV's CLAHE_Impl::apply for dev_gray uint8 [B,h,w] -> dev_out.  1 <= tiles_x, tiles_y <= 16,
 *   h > tiles_y, w > tiles_x.  When the grid does not divide BOTH extents the histograms come from the image extended
 *   with BORDER_REFLECT_101 by tiles_y - h % tiles_y rows and tiles_x - w % tiles_x columns (a whole extra `tiles` in
 *   an extent that does divide: OpenCV's quirk, kept).  Per tile: clip = max((int)(clip_limit * tileArea / 256), 1)
 *   (clip_limit <= 0: none), the excess redistributed as OpenCV does, lut[i] = saturate(rint(float(cumsum_i) * (255.f /
 *   tileArea))).  Per pixel: the bilinear blend of the four surrounding tiles' tables in float32, no contraction.
 *   dev_luts: NULL, or uint8 [B, tiles_y * tiles_x, 256] (4-byte aligned) that receives the tables.
 *
 * unetpp_bilateral_u8: cv2.bilateralFilter's scalar 8-bit loop for dev_gray uint8 [B,h,w] -> dev_out (may not alias),
 *   BORDER_REFLECT_101, h, w > radius.  `tables` (HOST memory, read during the call): radius 1..4, n_taps offsets
 *   (dy[k], dx[k]) within the radius, their space weights, 256 colour weights.  Per pixel, over the taps in table order,
 *   float32 without contraction: w = space_w[k] * color_w[|val - val0|]; sum += val * w; wsum += w; out = rint(sum /
 *   wsum) with IEEE division.
 *
 * unetpp_enhance_u8: the fused sequence, three launches and one memset.  dev_frames uint8 [B,h,w,channels_in]
 *   (3: BGR, converted with unetpp_gray_u8's constants; 1: grey) -> dev_out uint8 [B,h,w,channels_out] (3: the grey value
 *   replicated).  mode UNETPP_ENHANCE_ALWAYS enhances every frame (enhance_grayscale_frame); UNETPP_ENHANCE_IF_GREY
 *   enhances the frames whose decision (as unetpp_gray_decision, `threshold`) is 1 and copies the others
 *   (preprocess_frame; channels_out must be 3 for 3-channel input; a 1-channel frame always counts as grey).
 *   gamma_table: NULL, or 256 bytes in HOST memory applied after CLAHE.  tables: NULL (no filter), or as above.
 *   dev_luts as for unetpp_clahe_u8; dev_decisions: NULL, or uint8 [B] that receives the decisions (1 for every frame
 *   in UNETPP_ENHANCE_ALWAYS).  dev_workspace: unetpp_enhance_workspace_bytes(batch, h, w, tiles_x, tiles_y) bytes (0
 *   for a shape or grid outside the limits), 16-byte aligned; also needed by unetpp_clahe_u8.  dev_out may not overlap
 *   dev_frames.
 *
 * unetpp_enhance_layout: the core rows and columns of one workgroup of the last launch (tests place seams with it).
 *
 * Errors: UNETPP_E_UNSUPPORTED for a shape, grid or radius outside the limits; UNETPP_E_INVALID for NULL where not
 * allowed, bad channels or mode, a tap outside the radius, a weight that is negative or not finite, misalignment,
 * overlap.  No kernel is launched when an error is returned. */
typedef struct unetpp_bilateral_tables {
  int32_t radius, n_taps;
  const float* color_w;      /* [256] */
  const float* space_w;      /* [n_taps] */
  const int32_t* dy;         /* [n_taps] */
  const int32_t* dx;         /* [n_taps] */
} unetpp_bilateral_tables;

enum { UNETPP_ENHANCE_ALWAYS = 0, UNETPP_ENHANCE_IF_GREY = 1 };

size_t unetpp_enhance_workspace_bytes(int batch, int h, int w, int tiles_x, int tiles_y);
int unetpp_enhance_layout(int* tile_rows, int* tile_cols);
int unetpp_gray_decision(unetpp_engine* e, const uint8_t* dev_frames, int batch, int h, int w, double threshold,
                         uint8_t* dev_decisions, uint64_t* dev_sums, void* stream);
int unetpp_clahe_u8(unetpp_engine* e, const uint8_t* dev_gray, int batch, int h, int w, double clip_limit, int tiles_x,
                    int tiles_y, uint8_t* dev_out, uint8_t* dev_luts, void* dev_workspace, void* stream);
int unetpp_bilateral_u8(unetpp_engine* e, const uint8_t* dev_gray, int batch, int h, int w,
                        const unetpp_bilateral_tables* tables, uint8_t* dev_out, void* stream);
int unetpp_enhance_u8(unetpp_engine* e, const uint8_t* dev_frames, int batch, int h, int w, int channels_in, int channels_out,
                      int mode, double threshold, double clip_limit, int tiles_x, int tiles_y, const uint8_t* gamma_table,
                      const unetpp_bilateral_tables* tables, uint8_t* dev_out, uint8_t* dev_luts, uint8_t* dev_decisions,
                      void* dev_workspace, void* stream);

/* ---- non-local-means denoising: the 'fastNlMeans' denoiser of enhance_grayscale_frame ------------------------------------
 * cv2.fastNlMeansDenoising(img, None, h, 7, 21) (src/refactor/preprocess.py:68-69) for one 8-bit channel, as OpenCV's
 * published FastNlMeansDenoisingInvoker<uchar, int, unsigned, DistSquared, int> computes it: the image extended by 13
 * pixels with BORDER_REFLECT_101; per pixel and per offset (dy, dx) in [-10, 10]^2, D = the sum over the 7 x 7 window of
 * the squared differences, w = table[D >> 6], est += w * value at the offset, wsum += w; out = (est + wsum / 2) / wsum,
 * unsigned.  unet_amd/nlmeans.py is the NumPy form and builds the table (nlm_weights); every result equals it bit for bit,
 * the arithmetic being integer throughout; cv2's own result is not pinned by this project's tests.
 *
 * unetpp_nlmeans_u8: dev_src uint8 [B,h,w,channels_in] (channel 0 is filtered) -> dev_out uint8 [B,h,w,channels_out] (the
 *   result replicated); channels 1 or 3; 14 <= h, w <= 65535, h * w <= 2^30.  Template 7 and search window 21 are compile-time
 *   constants.  dev_weights_u16: the first n_weights entries of the table as uint16 on the DEVICE, owned by the caller
 *   (no engine state, no copy inside the call); every later entry counts as 0; 1 <= n_weights <= 8192; entry 0 must be
 *   positive (it divides) and no entry above 19096 (the sums are 32-bit).  dev_decisions: NULL, or uint8 [B] on the device
 *   (e.g. from the enhancement call above): a frame with 0 is copied through unchanged, every channel
 *   (channels_out == channels_in then), with nothing read back.  dev_out may not overlap dev_src.  One launch,
 *   asynchronous on `stream`.
 *
 * unetpp_nlmeans_layout: the rows and columns of output one workgroup owns (tests place seams with it).
 *
 * Errors: UNETPP_E_UNSUPPORTED for a shape or n_weights outside the limits; UNETPP_E_INVALID for NULL where not allowed,
 * bad channels, misalignment, overlap.  No kernel is launched when an error is returned. */
int unetpp_nlmeans_layout(int* tile_rows, int* tile_cols);
int unetpp_nlmeans_u8(unetpp_engine* e, const uint8_t* dev_src, int batch, int h, int w, int channels_in, int channels_out,
                      const uint8_t* dev_decisions, const uint16_t* dev_weights_u16, int n_weights, uint8_t* dev_out,
                      void* stream);

/* ---- segmentation evaluation on the device: confusion matrix and mask disagreement ---------------------------------------
 * What the reference's compute_metrics / compute_confusion_matrix (src/utils/metrics.py:9-127) and iou_per_class
 * (tools/eval.py:25-34) are functions of, and the comparison of two masks of the same frames.  unet_amd/evaluation.py is
 * the NumPy form and derives the metrics from the table; every result equals it exactly: integer sums, a minimum, and a
 * maximum of float32 values, none of which depends on the order of arrival.
 *
 * unetpp_confusion_u8: dev_pred, dev_target uint8 [B,h,w] (any h, w >= 1 with h * w < 2^32; any byte alignment: frames
 *   are read with 16-byte loads when the two pointers agree modulo 16, byte by byte otherwise and at each frame's head
 *   and tail; nothing outside a frame is read).  2 <= num_classes <= 16 is an argument, not the engine's class count.
 *   ignore_value: 0..255, or -1 for none.
 *   dev_counts  uint32 [B,C,C]: [b,t,p] = pixels of frame b with target t and pred p, both < C, target not ignored
 *   dev_outside uint32 [B,2]:   [b,0] = pixels whose target equals ignore_value; [b,1] = the other pixels with
 *               target >= C or pred >= C.  Neither kind enters dev_counts; the three sum to h * w per frame.
 *   dev_total   NULL, or uint64 [C*C + 2] (8-byte aligned): the kernel ADDS the counts and then the two outside counters
 *               of all frames to it and never clears it, so a loop over a whole set needs no synchronisation.
 *   dev_counts and dev_outside are cleared on `stream` inside the call.  One launch.
 *
 * unetpp_mask_disagreement: dev_a, dev_b uint8 [B,h,w] (h * w < 2^31).  Per frame over the pixels with a != b:
 *   dev_n_diff uint32 [B] their number; dev_first int32 [B] the smallest linear index y * w + x, -1 for none.
 *   dev_logits: NULL, or float32 [B,num_classes,h,w] (1 <= num_classes <= 256); then, over the differing pixels with
 *   both values < num_classes: dev_max_margin float32 [B] = max |logits[a] - logits[b]| (0.0 for none) and dev_n_nan
 *   uint32 [B] = those whose margin is NaN (they stay out of the maximum).  Logits are read at differing pixels only.
 *   Without logits dev_max_margin and dev_n_nan may be NULL (num_classes is ignored); given, they are cleared.
 *
 * unetpp_evaluation_layout: the pixels of a frame one workgroup of either kernel owns (tests place seams with it).
 *
 * Errors: UNETPP_E_INVALID for NULL where not allowed, a bad shape, num_classes or ignore_value, a misaligned
 * dev_total.  No kernel is launched when an error is returned. */
int unetpp_evaluation_layout(int* span_pixels);
int unetpp_confusion_u8(unetpp_engine* e, const uint8_t* dev_pred, const uint8_t* dev_target, int batch, int h, int w,
                        int num_classes, int ignore_value, uint32_t* dev_counts, uint32_t* dev_outside,
                        uint64_t* dev_total, void* stream);
int unetpp_mask_disagreement(unetpp_engine* e, const uint8_t* dev_a, const uint8_t* dev_b, int batch, int h, int w,
                             const float* dev_logits, int num_classes, uint32_t* dev_n_diff, int32_t* dev_first,
                             float* dev_max_margin, uint32_t* dev_n_nan, void* stream);

/* ---- rules on a probability map: threshold levels, the one-pass threshold scan, mean probability per component -------------
 * What tools/inference_binary_optimized.py does with the softmax map of its sliding-window predict: apply_hysteresis
 * (:116-136), apply_morphological_and_filtering (:139-176) and scan_thresholds (:179-270).  unet_amd/probmap.py is the
 * NumPy form and holds the compositions; every result equals it exactly: float32 comparisons and integer sums.
 *
 * A probability plane is (dev_prob, pixel_stride, channel): channel `channel` of an array float32
 * [B,h,w,pixel_stride] that starts at dev_prob (4-byte aligned), so pixel i of frame b is
 * dev_prob[(b*h*w + i)*pixel_stride + channel]; 1 <= pixel_stride <= 256.  Class 1 of the [B,h,w,C] output of
 * unetpp_tile_blend_f32 is read in place with pixel_stride = C, channel = 1; a dense [B,h,w] plane has pixel_stride 1.
 * With pixel_stride 1 or 2 the plane is read with 16-byte loads wherever 16 pixels start on a 16-byte boundary, one float
 * at a time elsewhere; nothing outside the array is read.  All entries queue their work on `stream` and allocate nothing.
 *
 * unetpp_prob_levels_f32: dev_codes uint8 [B,h,w] = 0 for p < t_low, 1 for t_low <= p < t_high, 2 for p >= t_high
 *   (t_low <= t_high; NaN gives 0); h * w < 2^32.  The codes feed unetpp_morphology with mask0 = codes, match0 = 2 (the
 *   seeds) and mask1 = codes, match1 = -1 (the low region).
 *
 * unetpp_prob_threshold_hist_f32: thresholds is a HOST array of n_thresholds float32 values, strictly ascending,
 *   1 <= n_thresholds = T <= 256.  Per pixel k = the number of thresholds <= p, 0..T (NaN: 0).  dev_target uint8 [B,h,w];
 *   g = 1 where the target equals target_class (0..255; -1: is non-zero), else 0.
 *   dev_counts  uint32 [B,2,T+1]: [b,g,k] = pixels of frame b with that g and k whose target is not ignore_value
 *   dev_outside uint32 [B]:       pixels whose target equals ignore_value (0..255, or -1 for none)
 *   dev_total   NULL, or uint64 [2*(T+1) + 1] (8-byte aligned): the kernel ADDS the counts and then the outside counter
 *               of all frames to it and never clears it.
 *   dev_counts and dev_outside are cleared on `stream` inside the call.  One launch.  The confusion table of threshold j
 *   (pred = p >= thresholds[j]) is a suffix sum: pred 1 is k > j.
 *
 * unetpp_components_prob_sum_f32: dev_labels int32 [B,h,w] of unetpp_components (h * w <= 2^30).  dev_sums uint64
 *   [B,capacity+1] (8-byte aligned, cleared inside the call): [b,l] = the sum over the pixels with label l,
 *   1 <= l <= capacity, of q(p) = floor(clamp(p, 0, 1) * 2^32), formed from the float's bits (q(1) = 2^32, q(NaN) = 0);
 *   row 0 stays 0.  Integer adds only: the same bits whatever order they land in.
 *
 * unetpp_components_filter_mean: dev_out uint8 [B,h,w] = out_value where the pixel's component l has
 *   stats AREA >= min_area and dev_prob_sums[b,l] >= thr_q * AREA (the product formed in 128 bits), i.e. a mean probability
 *   >= thr_q / 2^32.  dev_num, dev_stats [B,capacity,5], capacity, dev_workspace (that of unetpp_components, same
 *   arguments) and the overflow rule are those of unetpp_components_filter: a frame with num > capacity gives all zero.
 *
 * unetpp_probmap_layout: the pixels of a frame one workgroup of the first three kernels owns.
 *
 * Errors: UNETPP_E_INVALID for NULL where not allowed, a bad shape, plane, threshold list, class or capacity, a
 * misaligned pointer.  No kernel is launched when an error is returned. */
int unetpp_probmap_layout(int* span_pixels);
int unetpp_prob_levels_f32(unetpp_engine* e, const float* dev_prob, int pixel_stride, int channel, int batch, int h, int w,
                           float t_low, float t_high, uint8_t* dev_codes, void* stream);
int unetpp_prob_threshold_hist_f32(unetpp_engine* e, const float* dev_prob, int pixel_stride, int channel,
                                   const uint8_t* dev_target, int batch, int h, int w, const float* thresholds,
                                   int n_thresholds, int target_class, int ignore_value, uint32_t* dev_counts,
                                   uint32_t* dev_outside, uint64_t* dev_total, void* stream);
int unetpp_components_prob_sum_f32(unetpp_engine* e, const int32_t* dev_labels, const float* dev_prob, int pixel_stride,
                                   int channel, int batch, int h, int w, int capacity, uint64_t* dev_sums, void* stream);
int unetpp_components_filter_mean(unetpp_engine* e, const int32_t* dev_labels, const int32_t* dev_num,
                                  const int32_t* dev_stats, const uint64_t* dev_prob_sums, int batch, int h, int w,
                                  int capacity, int64_t min_area, uint64_t thr_q, uint8_t out_value, uint8_t* dev_out,
                                  void* dev_workspace, void* stream);

/* ---- the 6- and 7-class video loops: quality gate, class bits, class merge with its table, overlay --------------------------
 * What infer_video.py, infer_video_v3_high_quality.py and infer_video_optimized.py do per frame around the network:
 * FrameQualityGate.check (infer_video.py:73-118), the class clean-up with its priority merge (VideoInference.predict,
 * infer_video.py:194-216; NestedUNetInference.predict, infer_video_v3_high_quality.py:105-173), per-class pixel counts and
 * bounding boxes (infer_video.py:398, :421-445; validate_detection, infer_video_optimized.py:294-360) and overlay_mask
 * (infer_video.py:220-243; infer_video_optimized.py:282-292).  unet_amd/multiclass.py is the NumPy form and holds the
 * compositions; every result equals it exactly.  All entries queue their work on `stream` and allocate nothing (the resize
 * tables of the threshold entry are built once per size pair, on first use, which synchronises).  No kernel is launched when an
 * error is returned, and the outputs are untouched.
 *
 * Quality gate: dev_bgr uint8 [B,h,w,3], h, w >= 1, h * w <= 2^30.  dev_gray uint8 [B,h,w] = cvtColor(BGR2GRAY), the
 *   arithmetic of the grey entry above.  Per frame, from five 64-bit integer sums (sum g, sum g^2, sum L, sum L^2, sum |g - g_prev|,
 *   L the ksize-1 Laplacian [[0,1,0],[1,-4,1],[0,1,0]] with BORDER_REFLECT_101, accumulated with one integer atomic per sum
 *   and workgroup: the same bits in any order of arrival), in float64:
 *     dev_gray_std = sqrt((n S2 - S1^2) / n^2), dev_lap_var = (n SL2 - SL1^2) / n^2, dev_mad = S / n, n = h * w,
 *   each quotient the correctly rounded quotient of the two exact integers.  The previous frame of frame i > 0 is frame i - 1 of the
 *   batch (bad or not, as in the reference); that of frame 0 is dev_prev_gray uint8 [h,w], or NULL: mad = 0 for frame 0.
 *   dev_reason uint8 [B], in the reference's order of tests: 1 gray_std < glitch_flat_th; 2 lap_var < blur_th and mad >
 *   motion_th; 3 gray_std < flat_th; 4 ok; dev_is_bad uint8 [B] = reason != 4.  enable = 0 is the reference's first branch:
 *   reason 0, not bad, lap_var = mad = 0, gray_std computed.  dev_workspace: unetpp_quality_gate_workspace_bytes bytes, 8-byte
 *   aligned, cleared inside the call.  Two launches.  UNETPP_E_INVALID for NULL where not allowed, a bad shape, a NaN threshold,
 *   a misaligned float64 output or workspace, dev_gray overlapping an input.
 *
 * Class bits: five probability planes float32 [src_h,src_w] per frame; plane k of frame b starts at dev_prob + b * frame_stride +
 *   plane_offsets[k] (floats; plane_offsets is a HOST array of 5) and its pixels lie pixel_stride floats apart, so both
 *   [B,C,h,w] (frame_stride C h w, pixel_stride 1, offsets k h w) and [B,h,w,C] (frame_stride h w C, pixel_stride C, offsets k)
 *   are read in place.  dev_bits uint8 [B,dst_h,dst_w]; with p0..p4 the planes at that pixel, in float32 without contraction:
 *     bit 0: p0 >= thresholds[0] and p0 > p1 * ratio      bit 1: p1 >= thresholds[1] and p1 > p0 * ratio
 *     bits 2..4: pk >= thresholds[k]                      (thresholds: HOST array of 5; NaN sets no bit)
 *   With (dst_h, dst_w) != (src_h, src_w) each plane is first sampled at the bit map's resolution as OpenCV's published
 *   float32 INTER_LINEAR resize does: source coordinate (x + 0.5) scale - 0.5, clamped; S[sx] a0 + S[sx+1] a1 on two rows, then
 *   r0 b0 + r1 b1, four taps per output pixel and no full-size float plane (cv2's own output is unpinned).  One launch.
 *   h * w < 2^31 for both sizes, dst_h <= 65535.  UNETPP_E_INVALID for NULL, a bad shape, stride or offset, a NaN threshold.
 *
 * Class merge: dev_mask uint8 [B,h,w] (shape limits of the morphology entry).  One launch:
 *   1. plane k (0 <= k < n_planes <= 6) = the pixels whose value v has bit k set in lut[v] (HOST array of 256; bits >= n_planes
 *      must be clear).  For a label map plane k is "v in set k"; for a bit map from the entry above lut is the identity.
 *   2. the steps that name plane k run on it in order, in LDS: UNETPP_MORPH_DILATE / UNETPP_MORPH_ERODE / UNETPP_MERGE_OPEN / UNETPP_MERGE_CLOSE with
 *      elements[element], `iterations` times (open = erode^n then dilate^n, close = dilate^n then erode^n); semantics, elements and
 *      the border rule are those of the morphology entry.  Opening or closing an empty plane gives an empty plane.
 *   3. dev_out uint8 [B,h,w] (may be NULL with a table) = 0, then per plane in the order given, a later plane overwriting an
 *      earlier one: out_values[k] (HOST array; 1..255), or for -1 the input pixel's own value.
 *   4. dev_table (may be NULL) int32 [B,table_classes,5], 1 <= table_classes <= 256: per output value v < table_classes
 *      {count, x0, y0, x1, y1}, x1 and y1 inclusive, all four -1 for count 0.  Accumulated per workgroup in LDS, then one atomic
 *      add / min / max per non-empty value and workgroup; initialised inside the call.
 *   Limits: those of the morphology entry applied to all planes together: at most 4 elements (63 x 63, row-convex), at most 8
 *   steps, and the sum over every step of passes * (k - 1) at most 126 per axis (passes = iterations, twice that for open and
 *   close).  Beyond them, and for n_planes > 6: UNETPP_E_UNSUPPORTED, never a wrong result.  UNETPP_E_INVALID for NULL where
 *   not allowed, a bad shape, plane, op, element index, out value or lut entry, and dev_out overlapping dev_mask.
 *   unetpp_merge_classes_layout reports the tiling (no engine, no device needed) as the morphology layout entry does.
 *
 * Overlay: dev_frames, dev_out uint8 [B,h,w,3]; dev_mask uint8 [B,h,w]; colors HOST uint8 [256,3] in the frames' channel order,
 *   has_color HOST uint8 [256].  float32 without contraction:
 *     UNETPP_OVERLAY_REGION    where mask > 0: uint8(w_frame * f + w_color * c), truncated, c the value's colour (0 without
 *                              one); elsewhere the frame
 *     UNETPP_OVERLAY_WEIGHTED  cv2.addWeighted(frame, w_frame, painted, w_color, 0) per OpenCV's published scalar loop:
 *                              saturate_cast<uchar>(f * w_frame + p * w_color), round to nearest even; painted = the colour
 *                              where the value is non-zero and has one, else the frame (cv2's own output is unpinned)
 *   16-byte loads and stores when the three pointers are 16-byte aligned, bytes otherwise and for the tail.  0 <= weights <= 1.
 *   UNETPP_E_INVALID for NULL, a bad shape, mode or weight, dev_out overlapping an input.  One launch. */
enum { UNETPP_MERGE_OPEN = 6, UNETPP_MERGE_CLOSE = 7 };
enum { UNETPP_OVERLAY_REGION = 0, UNETPP_OVERLAY_WEIGHTED = 1 };

typedef struct unetpp_merge_step {
  int plane, op, element, iterations;
} unetpp_merge_step;

size_t unetpp_quality_gate_workspace_bytes(int batch);
int unetpp_quality_gate_u8(unetpp_engine* e, const uint8_t* dev_bgr, const uint8_t* dev_prev_gray, int batch, int h, int w,
                           int enable, double blur_th, double flat_th, double motion_th, double glitch_flat_th,
                           uint8_t* dev_gray, uint8_t* dev_is_bad, uint8_t* dev_reason, double* dev_lap_var,
                           double* dev_gray_std, double* dev_mad, void* dev_workspace, void* stream);
int unetpp_threshold_classes_f32(unetpp_engine* e, const float* dev_prob, int64_t frame_stride, int pixel_stride,
                                 const int64_t* plane_offsets, int batch, int src_h, int src_w, const float* thresholds,
                                 float ratio, int dst_h, int dst_w, uint8_t* dev_bits, void* stream);
int unetpp_merge_classes(unetpp_engine* e, const uint8_t* dev_mask, int batch, int h, int w, const uint8_t* lut, int n_planes,
                         const int32_t* out_values, const unetpp_morph_element* elements, int n_elements,
                         const unetpp_merge_step* steps, int n_steps, uint8_t* dev_out, int32_t* dev_table,
                         int table_classes, void* stream);
int unetpp_merge_classes_layout(int batch, int h, int w, int n_planes, const unetpp_morph_element* elements, int n_elements,
                                const unetpp_merge_step* steps, int n_steps, int* band_rows, int* tile_cols);
int unetpp_overlay_u8(unetpp_engine* e, const uint8_t* dev_frames, const uint8_t* dev_mask, int batch, int h, int w,
                      const uint8_t* colors, const uint8_t* has_color, float w_frame, float w_color, int mode,
                      uint8_t* dev_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNETPP_H */
