"""The model-adjacent lines of the reference frame loop (infer_two_stage_burr.py:37-47, 122-127, 292-314):
everything between "a BGR video frame" and "uint8 class masks at frame size, clipped to the ROI".
`process_frames_refactored` is the head of the refactored loop (infer_video_refactored.py:346-352): the grey-frame
enhancement and the ROI crop in front of the same steps.  `segment_frames` starts from frames already at model resolution; `process_frames` also runs the two
cv2.resize steps either side on the device (those two restate OpenCV's published
algorithm and are parity-unpinned, see oracle/unetpp_oracle.py).  `measure_frames` is the tail of the production loop
(infer_video_production.py:198-226): the diameter metrics and the defect analysis of every frame of a batch.
`process_frames_multiclass` is the frame loop of the 6- and 7-class scripts (infer_video.py:359-464,
infer_video_v3_high_quality.py, infer_video_optimized.py): quality gate, model, class clean-up, class table, overlay.
`process_frames_roi` and `process_frames_3class_full` are infer_frame of infer_video_roi.py (:193-259) and of
infer_video_3class_full.py (:193-261): the two 3-class loops that decide things per frame from the frame itself (roi_loop.py).
`process_frames_refactored_full` is the whole body of the refactored loop (infer_video_refactored.py:346-405): the head above,
postprocess_masks, the paste, the two contour diameters, the burr mask, the coverages and the overlay (contours.py).
`process_frames_spatial`, `process_frames_fixed`, `process_frames_confidence` and `process_frames_simple` are infer_frame of
infer_video_spatial.py, infer_video_fixed.py, infer_video_simple_v2.py and predict of infer_video_simple.py,
infer_video_simple_optimized.py and infer_video_simple_backup.py (simple_loops.py holds their steps and NumPy forms).
`process_raw_frames` is `process_frames` from the camera's one-byte-per-pixel buffer (GigECameraHarvester.read,
src/camera/gige_harvester.py:116-129): the demosaic of _to_bgr runs inside the resize launch (raw_frames.py).
`process_frames_two_stage` is the whole body of the two-stage loop (infer_two_stage_burr.py:274-343): rotate, normalise, the
model, the class masks with their sums, stage 2 and the overlay (two_stage.py); `process_raw_frames_two_stage` is the same from
the camera's raw bytes.  stream.FrameStream runs any of these double-buffered.
"""
from __future__ import annotations

import collections

import numpy as np


def preprocess_frames(frames_bgr_u8: np.ndarray) -> np.ndarray:
    """Resize-free part of preprocess_image (infer_two_stage_burr.py:122-127) for a batch of frames:
    uint8 [B,H,W,3] BGR -> float32 [B,3,H,W] RGB in [0,1]."""
    rgb = frames_bgr_u8[..., ::-1]
    return np.ascontiguousarray(np.transpose(rgb.astype(np.float32) / np.float32(255.0), (0, 3, 1, 2)))


def segment_frames(model, frames_bgr_u8, device=None):
    """infer_two_stage_burr.py:292-304 for B frames at once.

    `frames_bgr_u8` is a uint8 [B,H,W,3] BGR array/tensor already at model resolution.  Returns
    (pred, mask_cable, mask_tape) as uint8 CUDA tensors [B,H,W]; the BGR->RGB swap, /255, layout
    change, forward, softmax/argmax and the class-equality masks all run inside one engine call."""
    import torch
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    pred, cable, tape = model.segment(x, return_class_masks=True)
    return pred, cable, tape


FIXED_ROI_512 = {"x1": 140, "y1": 0, "x2": 270, "y2": 512}      # infer_two_stage_burr.py:29-34


def map_roi_to_original(original_size, target_size=(512, 512), roi=None):
    """infer_two_stage_burr.py:37-47: the fixed 512x512 ROI scaled to the frame size (width, height)."""
    orig_w, orig_h = original_size
    target_w, target_h = target_size
    scale_x = orig_w / target_w
    scale_y = orig_h / target_h
    roi = FIXED_ROI_512 if roi is None else roi
    return (int(roi["x1"] * scale_x), int(roi["y1"] * scale_y), int(roi["x2"] * scale_x), int(roi["y2"] * scale_y))


def process_frames(model, frames_bgr_u8, target_size=(512, 512), roi="fixed", device=None):
    """infer_two_stage_burr.py:292-314 for B raw frames at once, every step on the device:
    preprocess_image (BGR->RGB, cv2.resize INTER_LINEAR to `target_size` = (width, height), /255, CHW), the
    model, softmax/argmax, `(pred == 1)`, `(pred == 2)`, cv2.resize INTER_NEAREST back to the frame size and the
    ROI clip.  `roi`: "fixed" (map_roi_to_original of the frame size), None, or (x1, y1, x2, y2) in frame pixels.
    Returns (pred uint8 [B,H,W] at model resolution, mask_cable, mask_tape uint8 [B,frame_h,frame_w])."""
    import torch
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    fh, fw = int(x.shape[1]), int(x.shape[2])
    tw, th = int(target_size[0]), int(target_size[1])
    resized = x if (fh, fw) == (th, tw) else model.resize_frames(x, (th, tw))
    pred = model.segment(resized)
    if roi == "fixed":
        roi = map_roi_to_original((fw, fh), (tw, th))
    cable = model.resize_masks(pred, (fw, fh), match_class=1, roi=roi)
    tape = model.resize_masks(pred, (fw, fh), match_class=2, roi=roi)
    return pred, cable, tape


def process_raw_frames(model, raw_u8, pixel_format, target_size=(512, 512), roi="fixed", want_gray=False, device=None):
    """GigECameraHarvester.read (src/camera/gige_harvester.py:116-129) followed by process_frames, for B raw frames uint8 [B,H,W]
    in the camera's `pixel_format` ("BayerRG8", "BayerBG8", "Mono8", ...; raw_frames.pattern_of reads it as _to_bgr does): one
    launch takes the raw bytes to the network's uint8 input (raw_frames.resize), the full-size BGR frame is never written, and
    the tail is process_frames' own.  Returns what process_frames(model, raw_frames.to_bgr(model, raw_u8, pixel_format), ...)
    returns, bit for bit; with want_gray also the full-size grey frame uint8 [B,H,W] that model.detect_burrs reads."""
    from . import raw_frames as rf
    x = _device_frames(model, raw_u8, device)
    pattern = rf.pattern_of(pixel_format)
    fh, fw = int(x.shape[1]), int(x.shape[2])
    tw, th = int(target_size[0]), int(target_size[1])
    pred = model.segment(rf.resize(model, x, pattern, (th, tw)))
    if roi == "fixed":
        roi = map_roi_to_original((fw, fh), (tw, th))
    cable = model.resize_masks(pred, (fw, fh), match_class=1, roi=roi)
    tape = model.resize_masks(pred, (fw, fh), match_class=2, roi=roi)
    if want_gray:
        return pred, cable, tape, rf.to_gray(model, x, pattern=pattern)
    return pred, cable, tape


def process_frames_refactored(model, frames_bgr_u8, roi_xywh, input_size=512, *, enable=True, threshold=10.0, device=None, **cfg):
    """infer_video_refactored.py:346-352 for B raw frames at once, every step on the device and nothing read back:
    preprocess_frame (src/refactor/preprocess.py:77-91: grey frames enhanced with CLAHE, gamma and the bilateral filter --
    or, with denoise_method="fastNlMeans", non-local means (nlmeans.preprocess_frames_nlm) -- colour frames copied, decided
    per frame on the device), crop_roi (:94-113, the slice of roi = (x, y, w, h) clamped to
    the frame), then process_frames on the crop with target_size = (input_size, input_size) and no ROI clip.  `cfg`:
    PreprocessConfig's fields as NestedUNet.preprocess_frames takes them (clip_limit, tile_grid, gamma, denoise_method,
    denoise_strength); `enable` is enable_grayscale_enhance.  Returns (pred uint8 [B,input_size,input_size], mask_cable,
    mask_tape uint8 [B,crop_h,crop_w])."""
    import torch
    from . import enhance as en
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    x1, y1, x2, y2 = en.roi_bounds(int(x.shape[1]), int(x.shape[2]), roi_xywh)
    if x2 <= x1 or y2 <= y1:
        raise ValueError(f"roi {tuple(roi_xywh)} does not meet the {int(x.shape[1])}x{int(x.shape[2])} frame")
    if cfg.get("denoise_method") == "fastNlMeans":          # NestedUNet.preprocess_frames refuses it by name (its tests pin that)
        from . import nlmeans
        pre = nlmeans.preprocess_frames_nlm(model, x, enable, threshold, **{k: v for k, v in cfg.items() if k != "denoise_method"})
    else:
        pre = model.preprocess_frames(x, enable, threshold, **cfg)
    crop = pre[:, y1:y2, x1:x2].contiguous()
    return process_frames(model, crop, (int(input_size), int(input_size)), roi=None)


_DIAMETER_FIELDS = ("dc_px", "dt_px", "delta_d_px", "dc_mm", "dt_mm", "delta_d_mm", "valid_rows", "cable_coverage", "tape_coverage")
_DEFECT_FIELDS = ("tape_hole_ratio", "tape_num_holes", "tape_coverage", "cable_num_components", "tape_num_components",
                  "tape_largest_area_ratio", "total_defect_area")
_INT_FIELDS = {"valid_rows", "tape_num_holes", "cable_num_components", "tape_num_components", "total_defect_area"}


def measure_frames(model, pred, mm_per_px=0.05, defect_classes=(3, 4, 5, 6), max_components=8192):
    """The tail of process_frame (infer_video_production.py:198-226) for a uint8 CUDA class mask [B,H,W] (e.g. from
    segment()): compute_diameter_metrics(pred, 1, 2, mm_per_px), `None` where valid_rows < 20, else analyze_defects(pred,
    1, 2, defect_classes).  Everything is computed on the device for the whole batch; ONE read-back brings the scalars.
    Returns a list of B records, each None or
      {"diameter": {DiameterMetrics' fields}, "defect_analysis": {DefectAnalysis' fields, defect_areas a {class: area}
       dict}, "delta_d_mm": diameter.delta_d_mm, "wrap_diameter_mm": diameter.dt_mm}
    as plain Python numbers: what FrameResult carries besides timestamp_ns and frame_id, ready for the window
    aggregator.  RuntimeError for a frame with more than max_components - 1 components in one of its labellings."""
    import torch
    k = int(max_components)
    defect_classes = [int(c) for c in defect_classes]
    dia, over_d = model._diameter_metrics(pred, 1, 2, mm_per_px, 20, 31, 50, None, k)
    dfa, over_a = model._analyze_defects(pred, 1, 2, defect_classes, 10, k)
    cols = [dia[f] for f in _DIAMETER_FIELDS] + [dfa[f] for f in _DEFECT_FIELDS]
    cols += [dfa["defect_areas"][:, i] for i in range(len(defect_classes))] + [over_d | over_a]
    table = torch.stack([c.to(torch.float64) for c in cols], dim=1).cpu().tolist()     # integers here are far below 2^53: exact
    out = []
    for i, row in enumerate(table):
        if row[-1]:
            raise RuntimeError(f"measure_frames: frame {i} has more than max_components - 1 = {k - 1} components in one of its "
                               f"labellings: raise max_components")
        conv = lambda f, v: int(v) if f in _INT_FIELDS else v
        d = {f: conv(f, v) for f, v in zip(_DIAMETER_FIELDS, row)}
        if d["valid_rows"] < 20:
            out.append(None)
            continue
        a = {f: conv(f, v) for f, v in zip(_DEFECT_FIELDS, row[len(_DIAMETER_FIELDS):])}
        base = len(_DIAMETER_FIELDS) + len(_DEFECT_FIELDS)
        a["defect_areas"] = {c: int(row[base + j]) for j, c in enumerate(defect_classes)}
        out.append({"diameter": d, "defect_analysis": a, "delta_d_mm": d["delta_d_mm"], "wrap_diameter_mm": d["dt_mm"]})
    return out


def process_frames_robust(model, frames_bgr_u8, new_size=512, *, t_cable=0.50, t_tape=0.42, bg_margin=0.15, ct_margin=0.10, device=None, **post):
    """infer_frame of infer_video_robust.py (:284-370) for B raw frames of one size at once, every step on the device:
    letterbox to new_size, the model and exclusive_threshold with the call site's thresholds (segment_thresholded,
    rule="exclusive"), unletterbox, steps 7-9 (robust.postprocess_robust, which takes `post`: close_ksize, min_area,
    min_h_ratio, min_aspect, max_w_ratio, band_out, band_in, tape_min_area, pad, max_components, check) and steps 10-11.
    Returns (mask_cable, mask_tape uint8 0/1 [B,frame_h,frame_w] on the device, metrics: a list of B dicts of
    robust.MEASURE_FIELDS); the metrics are the one read-back.  create_overlay / putText and EventGate stay on the host."""
    import torch
    from . import robust
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    canvas, plan = robust.letterbox(model, x, new_size)
    cable_s, tape_s = model.segment_thresholded(canvas, "exclusive", t_cable, t_tape, bg_margin, ct_margin)
    cable = robust.unletterbox_masks(model, cable_s, plan)
    tape = robust.unletterbox_masks(model, tape_s, plan)
    cable, tape = robust.postprocess_robust(model, cable, tape, **post)
    return cable, tape, robust.measure_robust(model, cable, tape)


def process_frames_optimized(model, frames_bgr_u8, *, patch_size=384, stride=192, target_size=256, gate_thr=0.70, gate_class=1,
                             channel_order="bgr", device=None, **post):
    """The frame loop of tools/inference_binary_optimized.py's main() (:381-408) for B raw frames of one size, the map
    never leaving the device: predict_tiled(blend="probs", gate_thr) (OptimizedSlidingWindowInference.predict with the
    window gate), then probmap.postprocess_probmap on class `gate_class` of its output, read in place (apply_hysteresis,
    apply_morphological_and_filtering; `post` takes its thr_high, thr_low, ksize, iterations, min_area, mean_prob_thr,
    kernel_size, max_components, out_value, check).  Frames are BGR as cv2.imread returns them (channel_order="rgb" for
    frames already converted).  Returns (pred_final uint8 [B,H,W], output float32 [B,H,W,C]) on the device."""
    import torch
    from . import probmap
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    _, output = model.predict_tiled(x, patch_size, stride, target_size, blend="probs", gate_thr=gate_thr, gate_class=gate_class,
                                    channel_order=channel_order)
    _, pred_final = probmap.postprocess_probmap(model, output, channel=int(gate_class), **post)
    return pred_final, output


def process_frames_multiclass(model, frames_bgr_u8, prev_gray=None, *, input_size, variant="video", colors, alpha=0.6, overlay_mode="region",
                              num_classes=None, gate=None, thresholds=None, min_area_px=50, validate=None, device=None):
    """The per-frame body of the 6- and 7-class video loops for B raw BGR frames of one size at once, the frames never leaving
    the device (multiclass.py holds every step and its NumPy form):
      1. FrameQualityGate.check on every frame (multiclass.quality_gate; `gate`: its thresholds and `enable`), prev_gray = the
         grey frame before the batch or None; ONE read-back of the B flags
      2. resize_frames of the good frames to input_size (an int or (h, w))
      3. variant="video" (infer_video.py): segment(); variant="v3" (infer_video_v3_high_quality.py): predict_proba()
      4. video: resize_masks to the frame size, then clean_classes_video; v3: predict_v3 (`thresholds`: its cable_thr, tape_thr,
         defect_thr, ratio, channels)
      5. the class table, written by the same launch as the cleaned mask
      6. the overlay (`colors`, alpha, overlay_mode, classes >= the model's num_classes dropped from the colours)
      7. ONE read-back of the tables (with the gate's three statistics)
    Returns (records, overlays uint8 [B,H,W,3], gray uint8 [H,W] of the last frame: the next call's prev_gray), both tensors on
    the device.  records[i] is None for a gated frame (its overlay is the frame), else {"reason", "lap_var", "gray_std", "mad",
    "table" int32 [C,5] (count, x0, y0, x1, y1 per class), "events" (multiclass.defect_events with min_area_px)} and, with
    `validate` (the keyword arguments of multiclass.validate_detection), "valid" and "defects".  Contours, rectangles, text,
    cool-down counters and the window aggregator stay with the caller."""
    import torch
    from . import multiclass as mc
    if variant not in ("video", "v3"):
        raise ValueError(f"variant must be 'video' or 'v3', got {variant!r}")
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    is_bad, reason, lap_var, gray_std, mad, gray = mc.quality_gate(model, x, prev_gray, **(gate or {}))
    flags = torch.stack((is_bad.to(torch.uint8), reason)).cpu().numpy()                      # read-back 1: 2 B bytes
    b, fh, fw = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    good = [i for i in range(b) if not flags[0, i]]
    records = [None] * b
    if not good:
        return records, x.clone(), gray[-1]
    xg = x if len(good) == b else x.index_select(0, torch.tensor(good, dtype=torch.int64, device=x.device))
    th, tw = (int(input_size), int(input_size)) if isinstance(input_size, (int, np.integer)) else (int(input_size[0]), int(input_size[1]))
    resized = xg if (fh, fw) == (th, tw) else model.resize_frames(xg, (th, tw))
    c = model.num_classes if num_classes is None else int(num_classes)
    if variant == "video":
        mask, table = mc.clean_classes_video(model, model.resize_masks(model.segment(resized), (fw, fh)), num_classes=c)
    else:
        mask, table = mc.predict_v3(model, model.predict_proba(resized), (fh, fw), num_classes=c, **(thresholds or {}))
    over = mc.overlay(model, xg, mask, colors, alpha, overlay_mode, model.num_classes)
    if len(good) == b:
        overlays = over
    else:
        overlays = x.clone()
        overlays.index_copy_(0, torch.tensor(good, dtype=torch.int64, device=x.device), over)
    stats = torch.stack((lap_var, gray_std, mad)).view(torch.int32).reshape(-1)               # float64 bits as int32 pairs
    packed = torch.cat((table.reshape(-1), stats)).cpu().numpy()                               # read-back 2
    tables = packed[:table.numel()].reshape(len(good), c, 5)
    st = np.ascontiguousarray(packed[table.numel():]).view(np.float64).reshape(3, b)
    for k, i in enumerate(good):
        rec = {"reason": mc.REASONS[int(flags[1, i])], "lap_var": float(st[0, i]), "gray_std": float(st[1, i]), "mad": float(st[2, i]),
               "table": tables[k].copy(), "events": mc.defect_events(tables[k], min_area_px=min_area_px)}
        if validate is not None:
            rec["valid"], rec["defects"] = mc.validate_detection(tables[k], (fh, fw), **validate)
        records[i] = rec
    return records, overlays, gray[-1]


def _raise_loop_overflow(what, nums, k):
    for name, col in nums:
        for i, v in enumerate(col):
            if v > k:
                raise RuntimeError(f"{what}: frame {i} has num = {v} labels in its {name} labelling (background included), more than "
                                   f"max_components = {k}: raise max_components")


def process_frames_roi(model, frames_bgr_u8, *, use_roi=True, input_size=512, max_components=8192, device=None, **geometry):
    """infer_frame of infer_video_roi.py (:193-259) for B raw BGR frames of one size at once, every step on the device
    (roi_loop.py holds every step and its NumPy form):
      1. detect_roi_by_projection (roi_loop.detect_roi; use_roi=False: the whole frame)
      2. the crop and cv2.resize to input_size, the source width read from the device table
      3. the model's probabilities (predict_proba)
      4. adaptive_thresholding and ultra_strict_threshold with that frame's own thresholds
      5. refine_mask_by_geometry on both masks (`geometry`: its min_area, min_aspect, wide_width, edge_lo, edge_hi, large_area)
      6. cv2.resize INTER_NEAREST back and the paste into the full frame
      7. ONE read-back: the two coverages, the ROI table and the labellings' num
    Returns (mask_cable, mask_tape uint8 0/1 [B,H,W] on the device, metrics: a list of B dicts with cable_coverage,
    tape_coverage and roi = (x_min, x_max), roi int32 [B,4] on the device).  A frame whose ROI is empty (valid = 0; the
    reference's cv2.resize raises there) gets zero masks and zero coverages.  Overlay, text and events stay on the host."""
    import torch
    from . import roi_loop as rl
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    b, fh, fw = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    k, size = int(max_components), int(input_size)
    roi = rl.detect_roi(model, x) if use_roi else rl.full_roi(model, x)
    probs = model.predict_proba(rl.crop_resize(model, x, roi, size))
    cable, tape, counts, _ = rl.postprocess_roi(model, probs, roi, (fh, fw), max_components=k, **geometry)
    table = torch.cat((counts, roi), dim=1).cpu().tolist()                                    # the read-back: 8 B integers
    _raise_loop_overflow("process_frames_roi", (("cable", [r[2] for r in table]), ("tape", [r[3] for r in table])), k)
    metrics = [{"cable_coverage": r[0] / (size * size), "tape_coverage": r[1] / (size * size), "roi": (r[4], r[5])} for r in table]
    return cable, tape, metrics, roi


def process_frames_3class_full(model, frames_bgr_u8, *, input_size=512, t_cable=0.45, t_tape=0.50, bg_margin=0.15, use_cc_filter=True,
                               cc_min_area_cable=1000, cc_min_area_tape=500, cable_min_aspect=1.6, tape_dilate_px=15, max_components=8192,
                               device=None):
    """infer_frame of infer_video_3class_full.py (:193-261) for B raw BGR frames of one size at once, every step on the device:
    resize_frames to input_size, segment_thresholded(rule="thresholded_argmax"), select_primary_component on the cable,
    tape & dilate(cable, ELLIPSE 2 tape_dilate_px + 1) for the frames whose cable is not empty (one morphology program),
    keep_largest_cc on the tape (filter_components, rule="largest"), resize_masks to the frame size,
    measure_diameters_simple and the coverages at model size.  Returns (mask_cable, mask_tape uint8 0/1 [B,H,W], metrics: a
    list of B dicts of robust.MEASURE_FIELDS, pred uint8 [B,input_size,input_size] with cable 1 and tape 2); the metrics and
    the labellings' num are the one read-back."""
    import torch
    from . import robust
    from . import roi_loop as rl
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    fh, fw = int(x.shape[1]), int(x.shape[2])
    k, size = int(max_components), int(input_size)
    resized = x if (fh, fw) == (size, size) else model.resize_frames(x, (size, size))
    cable_s, tape_s = model.segment_thresholded(resized, "thresholded_argmax", t_cable, t_tape, bg_margin)
    n = size * size
    if use_cc_filter:
        cable, tape, cable_s, tape_s, table = rl.postprocess_3class_full(
            model, cable_s, tape_s, (fh, fw), cc_min_area_cable=cc_min_area_cable, cc_min_area_tape=cc_min_area_tape,
            cable_min_aspect=cable_min_aspect, tape_dilate_px=tape_dilate_px, max_components=k)
    else:
        cable, tape = model.resize_masks(cable_s, (fw, fh)), model.resize_masks(tape_s, (fw, fh))
        table = robust._measure_table(model, cable_s, tape_s)
    pred = torch.where(tape_s > 0, torch.full_like(tape_s, 2), cable_s)   # pred_mask[cable > 0] = 1, then [tape > 0] = 2
    rows = table.cpu().tolist()                                            # the read-back
    if use_cc_filter:
        _raise_loop_overflow("process_frames_3class_full", (("cable", [int(r[5]) for r in rows]), ("tape", [int(r[6]) for r in rows])), k)
    metrics = [dict(zip(robust.MEASURE_FIELDS, r[:3] + [int(r[3]) / n, int(r[4]) / n])) for r in rows]
    return cable, tape, metrics, pred


_REFACTORED_POST = ("min_area", "min_aspect", "max_center_offset", "ring_dilate", "ring_erode")
_REFACTORED_BURR = ("band_out", "laplacian_threshold", "burr_min_area", "burr_max_area")


def process_frames_refactored_full(model, frames_bgr_u8, roi_xywh, input_size=512, *, max_components=8192, device=None, **cfg):
    """The per-frame body of infer_video_refactored.py (:346-405) for B raw BGR frames of one size at once, every step on the
    device (contours.py holds the new steps and their NumPy forms):
      1. process_frames_refactored: preprocess_frame, crop_roi, model_inference (:346-352)
      2. the class map at the crop's size and postprocess_masks (:355-364; `cfg`: PostprocessConfig's min_area, min_aspect,
         max_center_offset, ring_dilate, ring_erode; roi_width is the ROI's w)
      3. paste_roi_mask of both masks into the full frame (:367-371)
      4. measure_diameter of both: the smallest circle around the largest external contour (:374-375)
      5. get_burr_mask_rulebased on cvtColor(frame, BGR2GRAY) and the full-frame cable mask (:380-381; `cfg`: BurrConfig's
         band_out, laplacian_threshold, burr_min_area, burr_max_area)
      6. the three counts behind has_burr and the two coverages (:382-386)
      7. the three blends of create_overlay (:191-201)
      8. ONE read-back: the two support tables, the labellings' num and the three counts per frame
    Every other keyword of `cfg` goes to process_frames_refactored (enable, threshold, PreprocessConfig's fields).  Returns
    (metrics: a list of B dicts with FrameMetrics' fields dc_px, dt_px, delta_d_px, ratio (None when dc_px == 0), has_burr,
    cable_coverage, tape_coverage; overlays uint8 [B,H,W,3]; (mask_cable, mask_tape, mask_burr) uint8 0/255 [B,H,W]), the
    tensors on the device.  ValueError for a frame with more than max_components labels in a labelling, frames of 4096 or
    more pixels a side, or a ROI that misses the frame.  The component filters inside steps 2 and 5 run with check=False: a
    frame with more than max_components - 1 components there gets an empty mask from them, as they document, and no
    read-back of their own.  EventDetector, putText and the CSV stay on the host."""
    import torch
    from . import contours as ct
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    if x.dim() != 4:
        raise ValueError("frames must be uint8 [B,H,W,3]")
    b, fh, fw = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    ct.check_frame_shape(fh, fw)
    k = ct.check_max_components(max_components)
    rx, ry, rw, rh = (int(v) for v in roi_xywh)
    post = {n: cfg.pop(n) for n in _REFACTORED_POST if n in cfg}
    burr = {n[5:] if n.startswith("burr_") else n: cfg.pop(n) for n in _REFACTORED_BURR if n in cfg}
    from . import enhance as en
    x1, y1, x2, y2 = en.roi_bounds(fh, fw, roi_xywh)
    if x2 <= x1 or y2 <= y1:
        raise ValueError(f"roi {(rx, ry, rw, rh)} does not meet the {fh}x{fw} frame")
    pred, _, _ = process_frames_refactored(model, x, roi_xywh, input_size, **cfg)
    pred_roi = model.resize_masks(pred, (x2 - x1, y2 - y1))
    cable_roi, tape_roi = model.postprocess_masks(pred_roi, 1, 2, roi_width=rw, max_components=k, check=False, **post)
    return _refactored_tail(model, x, cable_roi, tape_roi, roi_xywh, k, burr)


def _refactored_tail(model, x, cable_roi, tape_roi, roi_xywh, k, burr):
    """Lines :366-405 for frames uint8 [B,H,W,3] and the two post-processed ROI masks, all on the device: steps 3-8 of
    process_frames_refactored_full (scripts/contours_bench.py times exactly this)."""
    import torch
    from . import contours as ct
    fh, fw = int(x.shape[1]), int(x.shape[2])
    cable = ct.paste_roi_masks(model, cable_roi, roi_xywh, (fh, fw))
    tape = ct.paste_roi_masks(model, tape_roi, roi_xywh, (fh, fw))
    sup_c, num_c, _ = ct._support(model, cable, -1, k)
    sup_t, num_t, _ = ct._support(model, tape, -1, k)
    mask_burr = model.burr_mask_rulebased(model.bgr_to_gray(x), cable, -1, max_components=k, check=False, **burr)
    counts = torch.stack((model.count_nonzero(cable), model.count_nonzero(tape), model.count_nonzero(mask_burr), num_c, num_t), dim=1)
    overlays = ct.create_overlay_masks(model, x, cable, tape, mask_burr)
    rows = torch.cat((sup_c, sup_t, counts), dim=1).cpu().numpy()                              # the read-back: 21 B integers
    ct._raise_contour_overflow("process_frames_refactored_full", (("cable", rows[:, 19].tolist()), ("tape", rows[:, 20].tolist())), k)
    metrics = []
    for (_, rc), (_, rt), r in zip(ct.circle_from_support(rows[:, 0:8]), ct.circle_from_support(rows[:, 8:16]), rows):
        dc, dt = 2.0 * rc, 2.0 * rt
        metrics.append({"dc_px": dc, "dt_px": dt, "delta_d_px": dt - dc, "ratio": dt / dc if dc > 0 else None, "has_burr": bool(r[18] > 0),
                        "cable_coverage": int(r[16]) / (fw * fh), "tape_coverage": int(r[17]) / (fw * fh)})
    return metrics, overlays, (cable, tape, mask_burr)


def _device_frames(model, frames_bgr_u8, device):
    import torch
    x = frames_bgr_u8
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        x = x.to(device if device is not None else f"cuda:{model._device_index or 0}", non_blocking=True)
    return x


def _resized(model, x, size):
    return x if (int(x.shape[1]), int(x.shape[2])) == (size, size) else model.resize_frames(x, (size, size))


def process_frames_spatial(model, frames_bgr_u8, *, input_size=512, cable_bg_ratio=2.0, tape_bg_ratio=2.5, max_components=8192, device=None):
    """infer_frame of infer_video_spatial.py (:123-171) for B raw BGR frames of one size at once, every step on the device
    (simple_loops.py holds the new steps and their NumPy forms): resize_frames to input_size, predict_proba,
    relative_threshold, spatial_filter with 30 / 200 on the cable and 20 / 150 on the tape (filter_components,
    rule="spatial"), the focus band (column_band), resize_masks to the frame size, the coverages of the masks at model size.
    Returns (mask_cable, mask_tape uint8 0/1 [B,H,W], metrics: a list of B dicts with cable_coverage and tape_coverage, probs
    float32 [B,C,input_size,input_size]), the tensors on the device; the two counts and the labellings' num are the one
    read-back."""
    import torch
    from . import simple_loops as sl
    x = _device_frames(model, frames_bgr_u8, device)
    fh, fw = int(x.shape[1]), int(x.shape[2])
    k, size = int(max_components), int(input_size)
    probs = model.predict_proba(_resized(model, x, size))
    cable_s, tape_s = sl.relative_threshold(model, probs, cable_bg_ratio, tape_bg_ratio)
    cable_s, num_c = sl._filter_spatial(model, cable_s, 30, 200, k)
    tape_s, num_t = sl._filter_spatial(model, tape_s, 20, 150, k)
    cable_s, tape_s = sl.column_band(model, cable_s), sl.column_band(model, tape_s)
    cable, tape = model.resize_masks(cable_s, (fw, fh)), model.resize_masks(tape_s, (fw, fh))
    rows = torch.stack((model.count_nonzero(cable_s), model.count_nonzero(tape_s), num_c, num_t), dim=1).cpu().tolist()   # the read-back
    _raise_loop_overflow("process_frames_spatial", (("cable", [r[2] for r in rows]), ("tape", [r[3] for r in rows])), k)
    metrics = [{"cable_coverage": r[0] / (size * size), "tape_coverage": r[1] / (size * size)} for r in rows]
    return cable, tape, metrics, probs


def _measured_tail(model, what, cable_s, tape_s, frame_hw, nums, k):
    """The common end of infer_frame in infer_video_fixed.py (:210-234) and infer_video_simple_v2.py (:135-159): the masks
    resized to the frame, measure_diameters_simple and the coverages at model size, pred_mask; one read-back."""
    import torch
    from . import robust
    fh, fw = frame_hw
    n = int(cable_s.shape[1]) * int(cable_s.shape[2])
    cable, tape = model.resize_masks(cable_s, (fw, fh)), model.resize_masks(tape_s, (fw, fh))
    table = robust._measure_table(model, cable_s, tape_s)
    pred = torch.where(tape_s > 0, torch.full_like(tape_s, 2), cable_s)   # pred_mask[cable > 0] = 1, then [tape > 0] = 2
    if nums:
        table = torch.cat((table, torch.stack(nums, dim=1).to(torch.float64)), dim=1)
    rows = table.cpu().tolist()                                            # the read-back
    if nums:
        _raise_loop_overflow(what, (("cable", [int(r[5]) for r in rows]), ("tape", [int(r[6]) for r in rows])), k)
    metrics = [dict(zip(robust.MEASURE_FIELDS, r[:3] + [int(r[3]) / n, int(r[4]) / n])) for r in rows]
    return cable, tape, metrics, pred


def process_frames_fixed(model, frames_bgr_u8, *, input_size=512, conf_cable=0.6, conf_tape=0.65, bg_margin=0.4, min_area_cable=3000,
                         min_area_tape=1500, max_area_cable=100000, max_area_tape=80000, max_components=8192, device=None):
    """infer_frame of infer_video_fixed.py (:168-234) for B raw BGR frames of one size at once, every step on the device:
    resize_frames to input_size, segment_thresholded(rule="strict_bg_check"), filter_by_size_and_shape on both masks
    (simple_loops.keep_components), resize_masks to the frame size, measure_diameters_simple and the coverages at model size.
    Returns (mask_cable, mask_tape uint8 0/1 [B,H,W], metrics: a list of B dicts of robust.MEASURE_FIELDS, pred uint8
    [B,input_size,input_size] with cable 1 and tape 2); the metrics and the labellings' num are the one read-back."""
    from . import simple_loops as sl
    x = _device_frames(model, frames_bgr_u8, device)
    k, size = int(max_components), int(input_size)
    cable_s, tape_s = model.segment_thresholded(_resized(model, x, size), "strict_bg_check", conf_cable, conf_tape, bg_margin)
    cable_s, num_c, _ = sl._keep(model, cable_s, min_area_cable, max_area_cable, 0, -1, 1, k)
    tape_s, num_t, _ = sl._keep(model, tape_s, min_area_tape, max_area_tape, 0, -1, 1, k)
    return _measured_tail(model, "process_frames_fixed", cable_s, tape_s, (int(x.shape[1]), int(x.shape[2])), [num_c, num_t], k)


def process_frames_confidence(model, frames_bgr_u8, *, input_size=512, conf_threshold=0.3, device=None):
    """infer_frame of infer_video_simple_v2.py (:110-159) for B raw BGR frames of one size at once, every step on the device:
    resize_frames to input_size, predict_proba, simple_threshold (simple_loops.confidence_threshold), no filter, then the tail
    of process_frames_fixed.  Returns (mask_cable, mask_tape, metrics, pred, probs float32 [B,C,input_size,input_size])."""
    from . import simple_loops as sl
    x = _device_frames(model, frames_bgr_u8, device)
    probs = model.predict_proba(_resized(model, x, int(input_size)))
    cable_s, tape_s = sl.confidence_threshold(model, probs, conf_threshold)
    return _measured_tail(model, "process_frames_confidence", cable_s, tape_s, (int(x.shape[1]), int(x.shape[2])), [], 0) + (probs,)


def process_frames_simple(model, frames_bgr_u8, variant="simple", input_size=256, colors=None, alpha=0.5, *, want_table=True, max_components=8192,
                          device=None, **tape):
    """SimpleInference.predict of infer_video_simple.py (variant "simple", :81-154), infer_video_simple_optimized.py
    ("optimized", :139-234) and infer_video_simple_backup.py ("backup", :61-88) for B raw BGR frames of one size at once on a
    SimpleUNet (or any 7-class model), every step on the device: resize_frames to input_size (256 in the first two scripts),
    then predict_proba and simple_loops.predict_simple (`tape`: its min_tape_area, min_tape_width, min_burr_area), or for
    "backup" segment, resize_masks and simple_loops.predict_simple_backup.  With `colors` ({class: (b, g, r)}) the region blend
    of overlay_mask follows (multiclass.overlay, mode="region"); its drawContours stays on the host.  Returns (map uint8 [B,H,W]
    at frame size, table int32 [B,256,5] or None, overlays uint8 [B,H,W,3] or None), all on the device; the only
    synchronisation is the overflow check of the labellings' num after the last launch ("backup" labels nothing and
    never synchronises)."""
    from . import multiclass as mc
    from . import simple_loops as sl
    if variant not in ("simple", "optimized", "backup"):
        raise ValueError(f"variant must be 'simple', 'optimized' or 'backup', got {variant!r}")
    x = _device_frames(model, frames_bgr_u8, device)
    fh, fw = int(x.shape[1]), int(x.shape[2])
    resized = _resized(model, x, int(input_size))
    num = None
    if variant == "backup":
        if tape:
            raise ValueError(f"variant 'backup' takes no filter constants, got {sorted(tape)}")
        res = sl.predict_simple_backup(model, model.resize_masks(model.segment(resized), (fw, fh)), want_table=want_table)
        out, table = res if want_table else (res, None)
    else:
        kw = dict(min_tape_area=500, min_tape_width=20, min_burr_area=100)
        if set(tape) - set(kw):
            raise ValueError(f"unknown filter constants {sorted(set(tape) - set(kw))}")
        kw.update(tape)
        out, table, _, num, k = sl._predict_simple(model, model.predict_proba(resized), (fh, fw), variant, kw["min_tape_area"], kw["min_tape_width"],
                                                   kw["min_burr_area"], want_table, max_components)
    over = None if colors is None else mc.overlay(model, x, out, colors, alpha, "region", model.num_classes)
    if num is not None:
        model._raise_num_overflow(num, k)                                     # the read-back, after the last launch
    return out, table, over


# ---- the two-stage loop, end to end (infer_two_stage_burr.py:274-343) -----------------------------------------------------------------
TwoStageResult = collections.namedtuple("TwoStageResult", "pred mask_cable mask_tape mask_burr result counts roi roi_area")
_UNUSED_BURR_KEYS = ("band_out", "laplacian_threshold", "morph_kernel")      # in the reference's presets, never read by detect_burrs_on_cable


def _two_stage_tail(model, gray, pred, target_wh, roi, want_overlay, frames_of, burr_config):
    """:303-343 for the class map `pred`, the grey frames and (when an overlay is wanted) the BGR frames frames_of() gives."""
    import torch
    from . import two_stage as ts
    fh, fw = int(gray.shape[1]), int(gray.shape[2])
    if isinstance(roi, str):
        if roi != "fixed":
            raise ValueError(f"roi must be 'fixed', None or (x1, y1, x2, y2), got {roi!r}")
        roi = map_roi_to_original((fw, fh), target_wh)
    roi = (0, 0, fw, fh) if roi is None else tuple(int(v) for v in roi)
    cfg = {k: v for k, v in burr_config.items() if k not in _UNUSED_BURR_KEYS}
    cable, tape, counts = ts.class_masks(model, pred, (fw, fh), roi)
    burr = model.detect_burrs(gray, cable, **cfg)
    if want_overlay:
        result, n_burr = ts.overlay(model, frames_of(), cable, tape, burr, roi)
    else:
        result, n_burr = None, model.count_nonzero(burr).to(torch.int64)
    counts = torch.cat((counts, n_burr[:, None]), dim=1)
    return TwoStageResult(pred, cable, tape, burr, result, counts, roi, ts.roi_area(roi))


def process_frames_two_stage(model, frames_bgr_u8, *, target_size=(512, 512), roi="fixed", rotate=False, normalize_resolution=None,
                             want_overlay=True, device=None, **burr_config):
    """The body of the two-stage loop (infer_two_stage_burr.py:274-343) for B BGR frames of one size at once, every step on the
    device (two_stage.py holds the new steps and their NumPy forms):
      1. rotate=True: cv2.rotate(frame, ROTATE_90_COUNTERCLOCKWISE) (:276; two_stage.rotate)
      2. normalize_resolution=(width, height): cv2.resize to it (:280; resize_frames)
      3. preprocess_image and the model (:292-300; resize_frames to target_size = (width, height), segment)
      4. the two class masks at frame size, clipped to the ROI, and their sums (:303-314, :333-334; two_stage.class_masks)
      5. cv2.cvtColor(frame, COLOR_BGR2GRAY) (:317; bgr_to_gray)
      6. detect_burrs_on_cable (:318; detect_burrs, which takes `burr_config`: min_area, max_area and its other keywords; the
         keys of the reference's presets that its function never reads are dropped, so **edges.PRESETS[name] works)
      7. want_overlay: the four blends of visualize_two_stage and the burr count (:132-153, :321; two_stage.overlay)
    `roi`: "fixed" (map_roi_to_original of the frame size), None (the whole frame) or (x1, y1, x2, y2) in frame pixels.  Returns a
    TwoStageResult: pred uint8 [B,th,tw], mask_cable, mask_tape, mask_burr uint8 0/1 [B,H,W], result uint8 [B,H,W,3] or None,
    counts int64 [B,3] (cable, tape, burr pixels), all on the device, and roi, roi_area as Python numbers;
    two_stage.ratios(counts.cpu(), roi_area) gives the percentages and the [BURR!] flag of :338-342.  Nothing is read back apart
    from detect_burrs' own overflow check (check=False drops it).  The ROI box, the text and the contour outlines (:155-168,
    :345-348) stay on the host."""
    from . import two_stage as ts
    x = _device_frames(model, frames_bgr_u8, device)
    if x.dim() != 4 or int(x.shape[3]) != 3:
        raise ValueError("frames must be uint8 [B,H,W,3]")
    if rotate:
        x = ts.rotate(model, x, ts.ROTATE_CODES["90_ccw"])
    if normalize_resolution is not None:
        nw, nh = int(normalize_resolution[0]), int(normalize_resolution[1])
        if (int(x.shape[1]), int(x.shape[2])) != (nh, nw):
            x = model.resize_frames(x, (nh, nw))
    fh, fw = int(x.shape[1]), int(x.shape[2])
    tw, th = int(target_size[0]), int(target_size[1])
    pred = model.segment(x if (fh, fw) == (th, tw) else model.resize_frames(x, (th, tw)))
    return _two_stage_tail(model, model.bgr_to_gray(x), pred, (tw, th), roi, want_overlay, lambda: x, burr_config)


def process_raw_frames_two_stage(model, raw_u8, pixel_format, *, target_size=(512, 512), roi="fixed", want_overlay=True, device=None,
                                 **burr_config):
    """process_frames_two_stage from the camera's one-byte-per-pixel buffer, B raw frames uint8 [B,H,W] in `pixel_format`
    (process_raw_frames): raw_frames.resize feeds the model, raw_frames.to_gray stage 2, and raw_frames.to_bgr runs only when an
    overlay is wanted.  Returns what process_frames_two_stage(model, raw_frames.to_bgr(model, raw_u8, pixel_format), ...) returns,
    bit for bit.  A Bayer mosaic cannot be rotated or resized before its demosaic, so there is no rotate or normalize_resolution."""
    from . import raw_frames as rf
    x = _device_frames(model, raw_u8, device)
    pattern = rf.pattern_of(pixel_format)
    tw, th = int(target_size[0]), int(target_size[1])
    pred = model.segment(rf.resize(model, x, pattern, (th, tw)))
    gray = rf.to_gray(model, x, pattern=pattern)
    return _two_stage_tail(model, gray, pred, (tw, th), roi, want_overlay, lambda: rf.to_bgr(model, x, pattern=pattern), burr_config)
