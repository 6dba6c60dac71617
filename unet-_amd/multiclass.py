"""What the 6- and 7-class video loops do around the network, in NumPy (torch-free) and on the device (include/unetpp.h,
unetpp_quality_gate_u8, unetpp_threshold_classes_f32, unetpp_merge_classes, unetpp_overlay_u8; csrc/multiclass.h).  The loops
are infer_video.py, infer_video_v3_high_quality.py and infer_video_optimized.py; per frame they run
  1  FrameQualityGate.check (infer_video.py:73-118, used at :359-392)                               -> quality_gate
  2  the class clean-up with a priority merge: VideoInference.predict (infer_video.py:194-216)       -> clean_classes_video
     and NestedUNetInference.predict (infer_video_v3_high_quality.py:105-173)                        -> predict_v3
  3  per-class pixel counts and bounding boxes (infer_video.py:398, :421-445) and validate_detection -> class_table,
     (infer_video_optimized.py:294-360)                                                                 defect_events, validate_detection
  4  overlay_mask: the region blend (infer_video.py:220-243) and cv2.addWeighted (_optimized.py:282-292) -> overlay
Every device function takes the model and has its NumPy form here (<name>_np); the device results equal them bit for bit.

How the reference computes, and what follows for the restatement (NumPy 2.2.6, checked on its own expressions):
  `prob >= 0.60`, `prob_tape * 1.2`   a float32 array against a Python float: the scalar is rounded to float32 first and the
                        comparison / product is made in float32.  threshold_classes converts its scalars with np.float32.
  `(1 - alpha) * frame.astype(np.float32) + alpha * color_mask.astype(np.float32)`   1 - alpha is formed in float64, then both
                        scalars are rounded to float32; products and sum are float32; .astype(np.uint8) truncates.
  gray.std(), Laplacian(gray).var()   float64, two passes with pairwise summation.  The device (and quality_gate_np) form the
                        correctly rounded closed form of the exact integer sums instead: (n S2 - S1^2) / n^2.  The two differ by a
                        few ulps, which is why the fixtures keep every statistic away from its threshold.
Pinned on the restatement only (cv2 is not installed where this project is built; cv2's own output is unpinned, like the other
cv2 primitives here): the float32 INTER_LINEAR resize of the probability planes at a scale other than 1, and cv2.addWeighted.

Left on the host: findContours / drawContours(..., 2), cv2.rectangle and putText of the overlays, the cool-down counters,
event names, logging and the window aggregator of the event rule (bookkeeping across frames), and video I/O.
"""
from __future__ import annotations

import ctypes
import hashlib
import math

import numpy as np

from . import edges as ed
from . import evaluation as ev
from . import morphology as mo
from . import tiling as tl

REASONS = ("disabled", "revealed_glitch_frame(std<glitch_flat_th)", "motion_blur(lap<th & mad>th)", "too_flat(std<flat_th)", "ok")
REASON_DISABLED, REASON_GLITCH, REASON_MOTION_BLUR, REASON_TOO_FLAT, REASON_OK = range(5)
MAX_PLANES = 6
TABLE_COLS = ("count", "x0", "y0", "x1", "y1")
MERGE_OPS = {"dilate": 0, "erode": 1, "open": 6, "close": 7}


# ---- 1. the frame quality gate ----------------------------------------------------------------------------------------------------
def _check_frames(frames, prev_gray):
    if ev._dtype_name(frames) != "uint8" or len(frames.shape) != 4 or frames.shape[3] != 3 or min(frames.shape[:3]) < 1:
        raise ValueError(f"frames must be uint8 [B,H,W,3], got {ev._dtype_name(frames)} {list(frames.shape)}")
    b, h, w = (int(v) for v in frames.shape[:3])
    if prev_gray is not None and (ev._dtype_name(prev_gray) != "uint8" or tuple(prev_gray.shape) != (h, w)):
        raise ValueError(f"prev_gray must be uint8 [{h},{w}] like a frame, got {ev._dtype_name(prev_gray)} {list(prev_gray.shape)}")
    return b, h, w


def _check_gate(blur_th, flat_th, motion_th, glitch_flat_th):
    th = tuple(float(v) for v in (blur_th, flat_th, motion_th, glitch_flat_th))
    if any(v != v for v in th):
        raise ValueError("a threshold is NaN")
    return th


def _reflect101(i, n):
    i = np.abs(i)
    i = np.where(i >= n, 2 * n - 2 - i, i)
    return np.clip(i, 0, n - 1)


def laplacian_np(gray):
    """cv2.Laplacian(gray, CV_64F) with the default ksize = 1 and BORDER_REFLECT_101 as int64 [..,H,W]: the four neighbours
    minus four times the centre (exact integers, |L| <= 1020)."""
    g = np.asarray(gray).astype(np.int64)
    h, w = g.shape[-2:]
    ys, xs = np.arange(h), np.arange(w)
    up, down = g[..., _reflect101(ys - 1, h), :], g[..., _reflect101(ys + 1, h), :]
    left, right = g[..., :, _reflect101(xs - 1, w)], g[..., :, _reflect101(xs + 1, w)]
    return up + down + left + right - 4 * g


def quality_sums_np(frames, prev_gray=None):
    """(gray uint8 [B,H,W], sums): sums[b] = (sum g, sum g^2, sum L, sum L^2, sum |g - g_prev|) of frame b as Python ints.  The
    previous frame of frame b > 0 is frame b - 1; that of frame 0 is prev_gray, and None gives 0."""
    frames = np.asarray(frames)
    _check_frames(frames, prev_gray)
    gray = ed.bgr_to_gray_np(frames)
    sums = []
    for b in range(len(gray)):
        g = gray[b].astype(np.int64)
        lap = laplacian_np(gray[b])
        prev = gray[b - 1] if b else prev_gray
        diff = 0 if prev is None else int(np.abs(g - np.asarray(prev).astype(np.int64)).sum())
        sums.append((int(g.sum()), int((g * g).sum()), int(lap.sum()), int((lap * lap).sum()), diff))
    return gray, sums


def variance_from_sums(n, s1, s2):
    """(n s2 - s1^2) / n^2 for Python ints: one correctly rounded division of exact integers."""
    return (n * s2 - s1 * s1) / (n * n)


def gate_decision(lap_var, gray_std, mad, blur_th=80.0, flat_th=8.0, motion_th=10.0, glitch_flat_th=3.0):
    """The reason code of FrameQualityGate.check's tests, in its order."""
    if gray_std < glitch_flat_th:
        return REASON_GLITCH
    if lap_var < blur_th and mad > motion_th:
        return REASON_MOTION_BLUR
    if gray_std < flat_th:
        return REASON_TOO_FLAT
    return REASON_OK


def quality_gate_np(frames, prev_gray=None, *, enable=True, blur_th=80.0, flat_th=8.0, motion_th=10.0, glitch_flat_th=3.0):
    """FrameQualityGate(enable, ...).check over a batch: (is_bad bool [B], reason uint8 [B] (REASONS), lap_var, gray_std, mad
    float64 [B], gray uint8 [B,H,W]).  A bad frame still is the next frame's previous frame, as in the reference's loop."""
    th = _check_gate(blur_th, flat_th, motion_th, glitch_flat_th)
    gray, sums = quality_sums_np(frames, prev_gray)
    n = gray.shape[1] * gray.shape[2]
    bsz = len(gray)
    is_bad, reason = np.zeros(bsz, bool), np.zeros(bsz, np.uint8)
    lap_var, gray_std, mad = np.zeros(bsz), np.zeros(bsz), np.zeros(bsz)
    for b, (s1, s2, l1, l2, d) in enumerate(sums):
        gray_std[b] = math.sqrt(variance_from_sums(n, s1, s2))
        if not enable:
            continue
        lap_var[b], mad[b] = variance_from_sums(n, l1, l2), d / n
        reason[b] = gate_decision(lap_var[b], gray_std[b], mad[b], *th)
        is_bad[b] = reason[b] != REASON_OK
    return is_bad, reason, lap_var, gray_std, mad, gray


# ---- 2. class planes, their programs, the priority merge and the class table -----------------------------------------------------
def _element_of(el):
    if isinstance(el, (int, np.integer)):
        return mo.structuring_element("ellipse", int(el)), None
    if isinstance(el, tuple) and len(el) == 2 and isinstance(el[0], str):
        return mo.structuring_element(el[0], el[1]), None
    return (el if isinstance(el, tuple) else (el, None))


def check_planes(planes, lut=None):
    """Normalise planes = [(select, program, out_value)] -> (lut uint8 [256], out_values, elements [(array, (ax, ay))], steps
    [(plane, op code, element, iterations)]).  select: the input values of the plane (ignored with lut=); program: a list of
    (op, element[, iterations]) with op in dilate | erode | open | close and element an int k (ELLIPSE (k, k)), a
    (shape, ksize) pair, an array or an (array, anchor) pair; out_value: 1..255, or -1 for the input pixel's own value.
    lut: uint8 [256], bit k of lut[v] = "value v belongs to plane k".  ValueError for everything unetpp_merge_classes
    refuses: its limits are unetpp_morphology's, applied to all planes together."""
    planes = list(planes)
    if not 1 <= len(planes) <= MAX_PLANES:
        raise ValueError(f"1..{MAX_PLANES} planes, got {len(planes)}")
    if lut is None:
        table = np.zeros(256, np.uint8)
        for k, (select, _, _) in enumerate(planes):
            if select is None:
                raise ValueError(f"plane {k} names no input values and no lut= is given")
            for v in select:
                if not 0 <= int(v) <= 255:
                    raise ValueError(f"plane {k}: value {v!r} is not in 0..255")
                table[int(v)] |= 1 << k
    else:
        table = np.ascontiguousarray(np.asarray(lut), dtype=np.uint8)
        if np.asarray(lut).shape != (256,) or (table >> len(planes)).any():
            raise ValueError(f"lut must be uint8 [256] naming planes 0..{len(planes) - 1} only")
    elements, steps, out_values = [], [], []
    reach_v = reach_h = 0
    for k, (_, program, out_value) in enumerate(planes):
        ov = int(out_value)
        if ov != -1 and not 1 <= ov <= 255:
            raise ValueError(f"plane {k}: out_value must be 1..255 or -1 (the input pixel's own value), got {out_value!r}")
        out_values.append(ov)
        for st in program:
            op, el = st[0], st[1]
            it = int(st[2]) if len(st) > 2 else 1
            if op not in MERGE_OPS:
                raise ValueError(f"plane {k}: op must be one of {sorted(MERGE_OPS)}, got {op!r}")
            if it < 1:
                raise ValueError(f"plane {k}: iterations must be at least 1, got {it}")
            arr, anchor = mo.check_element(*_element_of(el))
            for i, (a, an) in enumerate(elements):
                if an == anchor and a.shape == arr.shape and np.array_equal(a, arr):
                    idx = i
                    break
            else:
                elements.append((arr, anchor))
                idx = len(elements) - 1
            passes = it * (2 if op in ("open", "close") else 1)
            reach_v += passes * (arr.shape[0] - 1)
            reach_h += passes * (arr.shape[1] - 1)
            steps.append((k, MERGE_OPS[op], idx, it))
    if len(elements) > mo.MAX_ELEMENTS:
        raise ValueError(f"at most {mo.MAX_ELEMENTS} distinct elements over all planes, got {len(elements)}")
    if len(steps) > mo.MAX_STEPS:
        raise ValueError(f"at most {mo.MAX_STEPS} steps over all planes, got {len(steps)}")
    if reach_v > mo.MAX_REACH or reach_h > mo.MAX_REACH:
        raise ValueError(f"the programs' reach (sum of iterations * (k - 1) over the dilates and erodes of all planes) exceeds "
                         f"{mo.MAX_REACH} pixels (vertical {reach_v}, horizontal {reach_h})")
    return table, out_values, elements, steps


def class_table_np(mask, num_classes=256):
    """int32 [B,num_classes,5] of a uint8 map [B,H,W]: per value v < num_classes count, x0, y0, x1, y1 (x1, y1 inclusive; -1 for
    count 0)."""
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 or mask.ndim != 3:
        raise ValueError(f"mask must be uint8 [B,H,W], got {mask.dtype} {list(mask.shape)}")
    c = _check_classes(num_classes)
    out = np.full((len(mask), c, 5), -1, np.int32)
    out[:, :, 0] = 0
    for b, m in enumerate(mask):
        for v in np.unique(m):
            if v < c:
                ys, xs = np.nonzero(m == v)
                out[b, v] = (len(ys), xs.min(), ys.min(), xs.max(), ys.max())
    return out


def _check_classes(num_classes):
    c = int(num_classes)
    if not 1 <= c <= 256:
        raise ValueError(f"num_classes must be 1..256, got {num_classes!r}")
    return c


def merge_classes_np(mask, planes, *, lut=None, want_table=True, num_classes=256):
    """What unetpp_merge_classes computes for a uint8 map [B,H,W]: plane k = the pixels whose value has bit k of the table set, its
    program run on it (cv2.morphologyEx semantics, unet_amd/morphology.py), then the planes merged in the order given, a later one
    overwriting an earlier one, as out_value or (for -1) the input pixel's own value.  Returns the merged map, and with
    want_table class_table_np of it."""
    table, out_values, elements, steps = check_planes(planes, lut)
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 or mask.ndim != 3:
        raise ValueError(f"mask must be uint8 [B,H,W], got {mask.dtype} {list(mask.shape)}")
    out = np.zeros_like(mask)
    sets = table[mask]
    for b in range(len(mask)):
        for k, ov in enumerate(out_values):
            x = ((sets[b] >> k) & 1).astype(bool)
            for plane, op, el, it in steps:
                if plane != k:
                    continue
                arr, anchor = elements[el]
                if op == MERGE_OPS["dilate"]:
                    x = mo.dilate_np(x, arr, anchor, it)
                elif op == MERGE_OPS["erode"]:
                    x = mo.erode_np(x, arr, anchor, it)
                elif op == MERGE_OPS["open"]:
                    x = mo.dilate_np(mo.erode_np(x, arr, anchor, it), arr, anchor, it)
                else:
                    x = mo.erode_np(mo.dilate_np(x, arr, anchor, it), arr, anchor, it)
            out[b][x] = mask[b][x] if ov < 0 else ov
    return (out, class_table_np(out, num_classes)) if want_table else out


# VideoInference.predict (infer_video.py:194-216) after its resize: the untrained class 4 belongs to no plane and becomes 0, cable
# and tape are closed with ELLIPSE (3,3), the defects {3, 5, 6} pass raw; cable < tape < defect
PLANES_VIDEO = (((1,), (("close", 3),), 1), ((2,), (("close", 3),), 2), ((3, 5, 6), (), -1))
# NestedUNetInference.predict (infer_video_v3_high_quality.py:143-171) on the bit map of threshold_classes: cable and tape close E3,
# the three defects open E3 then close E5; labels 1, 2, 4, 5, 6.  Its `if np.sum(mask) > 0` guards are no-ops (opening or
# closing an empty plane gives an empty plane), so there is no device-side branch for them.
_DEFECT = (("open", 3), ("close", 5))
PLANES_V3 = ((None, (("close", 3),), 1), (None, (("close", 3),), 2), (None, _DEFECT, 4), (None, _DEFECT, 5), (None, _DEFECT, 6))
LUT_BITS = (np.arange(256) & 31).astype(np.uint8)                # a bit map is its own plane table
PLANES_TABLE = ((range(1, 256), (), -1),)                          # every non-zero value passes as itself


def clean_classes_video_np(pred, want_table=True, num_classes=256):
    """infer_video.py:198-216 for a uint8 class map [B,H,W] already at frame size."""
    return merge_classes_np(pred, PLANES_VIDEO, want_table=want_table, num_classes=num_classes)


# ---- 3. probability planes -> class bits ---------------------------------------------------------------------------------------------
def _check_probs(probs, channels, layout):
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw' or 'nhwc', got {layout!r}")
    if ev._dtype_name(probs) != "float32" or len(probs.shape) != 4:
        raise ValueError(f"probs must be float32 [B,C,H,W] (or [B,H,W,C] with layout='nhwc'), got {ev._dtype_name(probs)} {list(probs.shape)}")
    shape = tuple(int(v) for v in probs.shape)
    b, c, h, w = shape if layout == "nchw" else (shape[0], shape[3], shape[1], shape[2])
    channels = tuple(int(k) for k in channels)
    if len(channels) != 5 or any(not 0 <= k < c for k in channels):
        raise ValueError(f"channels must be five indices in [0,{c}), got {channels!r}")
    if min(b, h, w) < 1 or c > 256:
        raise ValueError(f"probs is {list(shape)}: needs B, H, W >= 1 and C <= 256")
    return b, c, h, w, channels


def _thresholds(cable_thr, tape_thr, defect_thr, ratio):
    thr = np.array([cable_thr, tape_thr, defect_thr, defect_thr, defect_thr], np.float32)
    r = np.float32(ratio)
    if np.isnan(thr).any() or np.isnan(r):
        raise ValueError("a threshold or the ratio is NaN")
    return thr, r


def _frame_hw(frame_hw, h, w):
    if frame_hw is None:
        return h, w
    fh, fw = int(frame_hw[0]), int(frame_hw[1])
    if fh < 1 or fw < 1:
        raise ValueError(f"frame_hw must be positive, got {frame_hw!r}")
    return fh, fw


def threshold_classes_np(probs, frame_hw=None, *, cable_thr=0.60, tape_thr=0.60, defect_thr=0.70, ratio=1.2, channels=(1, 2, 3, 4, 5),
                         layout="nchw"):
    """infer_video_v3_high_quality.py:118-141: uint8 [B,frame_h,frame_w], bit 0 cable >= thr and cable > tape * ratio, bit 1 tape
    likewise, bits 2..4 the three defects >= defect_thr; planes `channels` of float32 probs.  Scalars are rounded to float32 and
    everything is float32 (module docstring); NaN sets no bit.  With frame_hw != the planes' size each plane is first resized as
    tiling.resize_linear_f32_np states the float32 INTER_LINEAR resize (at equal size it is the identity)."""
    probs = np.asarray(probs)
    b, c, h, w, channels = _check_probs(probs, channels, layout)
    thr, r = _thresholds(cable_thr, tape_thr, defect_thr, ratio)
    fh, fw = _frame_hw(frame_hw, h, w)
    out = np.zeros((b, fh, fw), np.uint8)
    for i in range(b):
        p = [np.ascontiguousarray(probs[i, k] if layout == "nchw" else probs[i, :, :, k]) for k in channels]
        if (fh, fw) != (h, w):
            p = [tl.resize_linear_f32_np(x, (fw, fh)) for x in p]
        with np.errstate(invalid="ignore"):
            bits = ((p[0] >= thr[0]) & (p[0] > p[1] * r)).astype(np.uint8)
            bits |= ((p[1] >= thr[1]) & (p[1] > p[0] * r)).astype(np.uint8) << 1
            for k in (2, 3, 4):
                bits |= (p[k] >= thr[k]).astype(np.uint8) << k
        out[i] = bits
    return out


def predict_v3_np(probs, frame_hw=None, *, want_table=True, num_classes=256, **thresholds):
    """NestedUNetInference.predict (infer_video_v3_high_quality.py:105-173) from the softmax planes on: threshold_classes_np, then
    merge_classes_np with PLANES_V3."""
    bits = threshold_classes_np(probs, frame_hw, **thresholds)
    return merge_classes_np(bits, PLANES_V3, lut=LUT_BITS, want_table=want_table, num_classes=num_classes)


# ---- 4. the overlay -----------------------------------------------------------------------------------------------------------------
def color_table(colors, num_classes=None):
    """(uint8 [256,3], uint8 [256]) from a dict {class_id: (b, g, r)} like the reference's CLASS_COLORS: the
    colours and the "has a colour" flags.  Class 0 and, with num_classes, every class_id >= num_classes are dropped, as the
    reference's loops drop them; a (table, flags) pair is treated the same way."""
    if isinstance(colors, tuple) and len(colors) == 2 and not isinstance(colors[0], (int, np.integer)):
        table, has = np.array(colors[0], dtype=np.uint8), np.array(np.asarray(colors[1]) != 0, dtype=np.uint8)
        if table.shape != (256, 3) or has.shape != (256,):
            raise ValueError("a colour table is (uint8 [256,3], flags [256])")
        has[0] = 0
        if num_classes is not None:
            has[max(int(num_classes), 0):] = 0
        return np.ascontiguousarray(table), has
    if not isinstance(colors, dict):
        raise ValueError("colors must be a dict {class_id: (b, g, r)} or a (table, flags) pair")
    table, has = np.zeros((256, 3), np.uint8), np.zeros(256, np.uint8)
    for cid, col in colors.items():
        cid = int(cid)
        if not 0 <= cid <= 255 or len(col) != 3 or any(not 0 <= int(v) <= 255 for v in col):
            raise ValueError(f"colour {cid!r}: {col!r} is not a class 0..255 with three values 0..255")
        if cid == 0 or (num_classes is not None and cid >= int(num_classes)):
            continue
        table[cid], has[cid] = col, 1
    return table, has


def _weights(alpha, mode):
    if mode not in ("region", "weighted"):
        raise ValueError(f"mode must be 'region' or 'weighted', got {mode!r}")
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"alpha must be in [0,1], got {alpha!r}")
    return np.float32(1 - a), np.float32(a)


def _check_overlay(frames, mask):
    if ev._dtype_name(frames) != "uint8" or len(frames.shape) != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be uint8 [B,H,W,3], got {ev._dtype_name(frames)} {list(frames.shape)}")
    if ev._dtype_name(mask) != "uint8" or tuple(mask.shape) != tuple(frames.shape[:3]):
        raise ValueError(f"mask must be uint8 {list(frames.shape[:3])} like the frames, got {ev._dtype_name(mask)} {list(mask.shape)}")


def overlay_np(frames, mask, colors, alpha=0.5, mode="region", num_classes=None):
    """overlay_mask without its contours.  mode="region" (infer_video.py:220-243): where mask > 0
    uint8(fl32(1 - alpha) f + fl32(alpha) c), truncated, c the value's colour, black for a value without one; elsewhere the frame.
    mode="weighted" (infer_video_optimized.py:282-292): cv2.addWeighted(frame, 1 - alpha, painted, alpha, 0) per OpenCV's
    published scalar loop, saturate_cast<uchar>(f w0 + p w1) in float32, rounded to nearest even; painted = the frame with the
    colour where the value has one."""
    frames, mask = np.asarray(frames), np.asarray(mask)
    _check_overlay(frames, mask)
    table, has = color_table(colors, num_classes)
    w0, w1 = _weights(alpha, mode)
    f32 = frames.astype(np.float32)
    colored = (mask > 0) & (has[mask] != 0)
    if mode == "region":
        color_mask = np.where(colored[..., None], table[mask], 0).astype(np.uint8)
        blended = (w0 * f32 + w1 * color_mask.astype(np.float32)).astype(np.uint8)
        return np.where((mask > 0)[..., None], blended, frames)
    painted = np.where(colored[..., None], table[mask], frames).astype(np.float32)
    return np.clip(np.rint(f32 * w0 + painted * w1), 0, 255).astype(np.uint8)


# ---- 5. host rules on the class table -----------------------------------------------------------------------------------------------
def _table_rows(table):
    t = table.cpu().numpy() if hasattr(table, "cpu") else np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 5 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"table must be the integer [C,5] table of one frame, got {t.dtype} {list(t.shape)}")
    return [[int(v) for v in row] for row in t]


def validate_detection(table, hw, *, min_cable_area, cable_coverage_threshold, min_defect_area, edge_margin, defect_classes=(3, 4, 5, 6)):
    """validate_detection (infer_video_optimized.py:294-360) on the class table [C,5] of one frame of size hw = (h, w):
    (is_valid, [{class_id, bbox (x0, y0, x1, y1), area}]), in Python integers as the reference computes.  The reference divides by
    (x1 - x0) * (y1 - y0): a defect one pixel wide or high that touches the edge margin raises its ZeroDivisionError here too."""
    rows = _table_rows(table)
    h, w = int(hw[0]), int(hw[1])
    cable_area = rows[1][0] if len(rows) > 1 else 0
    cable_coverage = cable_area / (h * w)
    if cable_area < min_cable_area:
        return False, []
    if cable_coverage < cable_coverage_threshold:
        return False, []
    defects = []
    for class_id in defect_classes:
        area, x0, y0, x1, y1 = rows[class_id] if class_id < len(rows) else (0, -1, -1, -1, -1)
        if area < min_defect_area:
            continue
        if area == 0:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")      # ys.min() of the reference
        if x0 < edge_margin or x1 > w - edge_margin or y0 < edge_margin or y1 > h - edge_margin:
            edge_pixels = 0
            total_pixels = (x1 - x0) * (y1 - y0)
            if x0 < edge_margin:
                edge_pixels += (edge_margin - x0) * (y1 - y0)
            if x1 > w - edge_margin:
                edge_pixels += (x1 - (w - edge_margin)) * (y1 - y0)
            if y0 < edge_margin:
                edge_pixels += (edge_margin - y0) * (x1 - x0)
            if y1 > h - edge_margin:
                edge_pixels += (y1 - (h - edge_margin)) * (x1 - x0)
            if edge_pixels / total_pixels > 0.5:
                continue
        defects.append({"class_id": class_id, "bbox": (x0, y0, x1, y1), "area": area})
    return True, defects


def defect_events(table, *, classes=(3, 5, 6), min_area_px):
    """The area and box part of the event rule (infer_video.py:421-464) on the class table [C,5] of one frame: per class present
    with area >= min(min_area_px, 10) a dict {class_id, bbox (x0, y0, x1, y1), area}.  Cool-down, names and logging stay with the
    caller."""
    rows = _table_rows(table)
    events = []
    for class_id in classes:
        area, x0, y0, x1, y1 = rows[class_id] if class_id < len(rows) else (0, -1, -1, -1, -1)
        if area > 0 and area >= min(min_area_px, 10):
            events.append({"class_id": class_id, "bbox": (x0, y0, x1, y1), "area": area})
    return events


# ---- scenes for tests, fixtures and the bench (seeded; the fixtures store only results and the inputs' SHA-256) ---------------------
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _colour(gray, r):
    """A BGR frame whose channels are the grey image plus a small seeded offset each."""
    off = r.integers(-6, 7, 3)
    return np.clip(gray[..., None].astype(np.int64) + off, 0, 255).astype(np.uint8)


def make_gate_sequence(H, W, seed, kind="reasons"):
    """uint8 [B,H,W,3] for the quality gate.  "reasons": a textured frame (ok), a nearly constant one (glitch), a smooth ramp far
    from it (motion blur), a textured frame of low contrast (too flat), a textured frame (ok).  "moving": a textured frame, then
    a smooth ramp, which is bad only because of what precedes it.  "still": two smooth ramps a grey level apart (both ok)."""
    r = np.random.default_rng(7300 + 31 * int(seed))
    x = np.arange(W)[None, :] * np.ones((H, 1))
    ramp = (40 + 170 * x / max(W - 1, 1)).astype(np.int64)
    textured = lambda: r.integers(0, 256, (H, W))
    if kind == "reasons":
        grays = [textured(), 127 + r.integers(0, 3, (H, W)), ramp, r.integers(118, 138, (H, W)), textured()]
    elif kind == "moving":
        grays = [textured(), ramp]
    elif kind == "still":
        grays = [ramp + 1, ramp]
    else:
        raise ValueError(f"unknown kind {kind!r}")
    return np.stack([_colour(g, r) for g in grays])


def make_class_scene(H, W, seed):
    """(pred uint8 [H,W] with classes 0..6, frame uint8 [H,W,3]) for the class clean-up, H >= 48, W >= 64: a cable band and a tape
    band side by side with one-pixel gap rows (a close bridges them), a row of cable inside the tape, a patch of alternating cable
    and tape columns (both closes fill it: tape overwrites closed cable) with a 2 x 2 class-3 block on it (a raw defect overwrites
    both) and a larger one on the cable, a class-4 block (it disappears), a class-5 block inside the left edge margin, a class-6 block that only touches it, and
    sparse noise of classes 0, 1, 2 and 4."""
    r = np.random.default_rng(8100 + 17 * int(seed))
    pred = np.zeros((H, W), np.uint8)
    c0, c1, c2 = W // 4, W // 2, 3 * W // 4
    pred[:, c0:c1] = 1
    pred[:, c1:c2] = 2
    pred[H // 3, c0:c2] = 0
    pred[H // 2, c1:c2] = 1
    py, px = 4, c2 + 2
    patch = pred[py:py + 12, px:px + 12]
    patch[:, 0::2] = 1
    patch[:, 1::2] = 2
    pred[py + 4:py + 6, px + 4:px + 6] = 3
    pred[H // 2 + 6:H // 2 + 11, c0 + 4:c0 + 9] = 3
    pred[H - 12:H - 6, c1 + 2:c1 + 8] = 4
    pred[H // 2 + 4:H // 2 + 12, 0:5] = 5
    pred[H // 4:H // 4 + 7, 5:c0 - 2] = 6
    noise = r.random((H, W)) < 0.01
    noise[H // 2 + 4:H // 2 + 12, 0:5] = False
    pred[noise] = r.choice(np.array([0, 1, 2, 4], np.uint8), int(noise.sum()))
    return pred, r.integers(0, 256, (H, W, 3), dtype=np.uint8)


def make_v3_logits(S, seed):
    """float32 [1,6,S,S] piecewise-constant logits for NestedUNetInference.predict, S >= 48: a cable and a tape region with
    one-pixel gaps (closed), blocks of the three defect channels (kept), single defect pixels (an open removes them), and regions
    whose probability lies on either side of the thresholds."""
    r = np.random.default_rng(8700 + 13 * int(seed))
    z = np.zeros((6, S, S), np.float32)
    z[0] = 1.0
    a, b, c = S // 6, S // 2, 5 * S // 6
    z[1, :, a:b] = 3.0
    z[2, :, b:c] = 3.0
    z[1, S // 3, a:b] = 0.0                                   # gaps
    z[2, 2 * S // 3, b:c] = 0.0
    z[1, :S // 8, a:b] = 2.0                                   # p = 0.54: below the cable threshold
    z[2, -S // 8:, b:c] = 2.3                                  # p = 0.62: just above the tape threshold
    for ch, (y, x) in zip((3, 4, 5), ((S // 4, a + 3), (S // 2, b + 3), (3 * S // 4, a + 10))):
        z[ch, y:y + 6, x:x + 7] = 5.5
        z[ch, y + 1, x + 2] = 1.0                              # a hole in the block: the close fills it
    for ch in (3, 4, 5):
        for _ in range(4):
            z[ch, int(r.integers(2, S - 2)), int(r.integers(2, S - 2))] = 6.0
    z[4, 2:5, c + 2:c + 4] = 3.3                               # p = 0.70 +: a 3 x 2 block, too thin for the open
    return z[None]


PLANE_LEVELS = [0.0, 0.05, 0.3, 0.5, 0.55, 0.6, 0.65, 0.7, 0.72, 0.75, 0.9, 1.0]


def make_prob_planes(B, h, w, seed):
    """float32 [B,5,h,w]: per plane blocks of 4 x 4 pixels at levels around the default thresholds with single-pixel specks, and
    the float32 values of 0.6, 0.7, 0.6 * 1.2 and their neighbours planted."""
    r = np.random.default_rng(9400 + 7 * int(seed))
    levels = np.array(PLANE_LEVELS, np.float32)
    blocks = r.integers(0, len(levels), (B, 5, (h + 3) // 4, (w + 3) // 4))
    p = levels[blocks].repeat(4, 2).repeat(4, 3)[:, :, :h, :w].copy()
    p += (r.random((B, 5, h, w)) < 0.3) * r.uniform(-0.02, 0.02, (B, 5, h, w)).astype(np.float32)
    base = [np.float32(0.6), np.float32(0.7), np.float32(0.6) * np.float32(1.2)]
    vals = [v for t in base for v in (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)))]
    flat = p.reshape(-1)
    flat[r.choice(flat.size, size=min(4 * len(vals), flat.size), replace=False)] = np.resize(np.array(vals, np.float32), min(4 * len(vals), flat.size))
    return np.clip(p, 0, 1).astype(np.float32)


def fixture_facts(g, margin=1e-9):
    """What tests/golden/multiclass_scenes.npz must show, asserted by its generator and by the host test (g: the file or the
    generator's payload).  Returns the counts it looked at."""
    seen, facts = set(), {}
    for name, kind, H, W, seed, _ in g["gate"]:
        std, lap, mad = (np.asarray(g[f"{name}_{f}"]) for f in ("gray_std", "lap_var", "mad"))
        for values, ths in ((std, (3.0, 8.0)), (lap, (80.0,)), (mad, (10.0,))):
            for th in ths:
                assert (np.abs(values - th) >= margin * th).all(), (name, values, th)       # no statistic within 1e-9 of a threshold
        seen |= set(np.asarray(g[name + "_reason"]).tolist())
        assert len(g[name + "_disabled_std"]) == len(std)
        if kind == "moving":                                        # the second frame is bad only because of the first
            assert np.asarray(g[name + "_is_bad"]).tolist() == [False, True] and not bool(g[name + "_alone_bad"])
            assert int(g[name + "_reason"][1]) == REASON_MOTION_BLUR
            facts["moving"] = name
    assert seen == {REASON_GLITCH, REASON_MOTION_BLUR, REASON_TOO_FLAT, REASON_OK}, seen      # REASON_DISABLED: the _disabled_std runs
    e3 = mo.structuring_element("ellipse", 3)
    close = lambda x, e: mo.erode_np(mo.dilate_np(x, e), e)
    min_cable, coverage, min_defect, edge = (float(v) for v in g["validate"])
    skipped = kept = 0
    for name, H, W, seed, _, _ in g["video"]:
        H, W = int(H), int(W)
        pred, _ = make_class_scene(H, W, int(seed))
        out = np.asarray(g[name + "_video"])
        cable, tape, defect = pred == 1, pred == 2, np.isin(pred, (3, 5, 6))
        cc, ct = close(cable, e3), close(tape, e3)
        facts[name] = (int((cc & ~cable).sum()), int((cc & (out == 2)).sum()), int((defect & cc & ct).sum()), int((pred == 4).sum()))
        assert all(v > 0 for v in facts[name]) and not (out == 4).any(), (name, facts[name])
        assert (out == 6).any()                                     # without a colour when num_classes = 6
        table = class_table_np(out[None], 7)[0]
        listed = set(np.asarray(g[name + "_defects"])[:, 0].tolist())
        for cid in (3, 4, 5, 6):
            n, x0, y0, x1, y1 = (int(v) for v in table[cid])
            if cid != 4:
                assert n == 0 or (x1 > x0 and y1 > y0), (name, cid)        # no defect box is one pixel wide
            if n >= min_defect and (x0 < edge or x1 > W - edge or y0 < edge or y1 > H - edge):
                skipped += cid not in listed
                kept += cid in listed
        assert bool(g[name + "_valid"])
        for tag in ("region_a50", "region_a60", "weighted_a50", "weighted_a60", "region6_a60"):
            assert len(str(g[f"{name}_{tag}"])) == 64
    assert skipped > 0 and kept > 0, (skipped, kept)                # both sides of validate_detection's edge rule
    facts["edge_rule"] = (skipped, kept)
    e5 = mo.structuring_element("ellipse", 5)
    for name, S, seed, _ in g["v3"]:
        planes = np.asarray(g[name + "_planes"])
        bits = threshold_classes_np(planes[None], channels=(0, 1, 2, 3, 4))[0]
        raw_c = (bits & 1) != 0
        bridged = int((close(raw_c, e3) & ~raw_c).sum())
        specks = 0
        for k in (2, 3, 4):
            x = ((bits >> k) & 1) != 0
            opened = mo.dilate_np(mo.erode_np(x, e3), e3)
            specks += int((x & ~close(opened, e5)).sum())
        assert bridged > 0 and specks > 0, (name, bridged, specks)
        facts[name] = (bridged, specks)
    return facts


# ---- the device path (torch imported lazily, as in evaluation.py) -----------------------------------------------------------------
def quality_gate(model, frames, prev_gray=None, *, enable=True, blur_th=80.0, flat_th=8.0, motion_th=10.0, glitch_flat_th=3.0):
    """quality_gate_np on the device for uint8 CUDA frames [B,H,W,3] (BGR) and prev_gray uint8 [H,W] or None: device tensors
    (is_bad bool [B], reason uint8 [B], lap_var, gray_std, mad float64 [B], gray uint8 [B,H,W]).  Two launches on the current
    stream (the sums with the grey frames, the statistics), nothing read back; gray[-1] is the next batch's prev_gray."""
    import torch
    from . import _lib
    th = _check_gate(blur_th, flat_th, motion_th, glitch_flat_th)
    frames = model._input(frames, "frames", "[B,H,W,3]")
    if prev_gray is not None:
        prev_gray = model._input(prev_gray, "prev_gray", "[H,W]")
    b, h, w = _check_frames(frames, prev_gray)
    dev = frames.device
    gray = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    flags = torch.empty((2, b), dtype=torch.uint8, device=dev)
    stats = torch.empty((3, b), dtype=torch.float64, device=dev)
    ws = model._workspace(("quality_gate", b), lambda: _lib.load().unetpp_quality_gate_workspace_bytes(b), dev, f"quality_gate: unsupported batch {b}")
    model._call("unetpp_quality_gate_u8", frames, prev_gray, b, h, w, 1 if enable else 0, *th, gray, flags[0], flags[1], stats[0], stats[1],
                stats[2], ws, stream_of=frames)
    return flags[0].view(torch.bool), flags[1], stats[0], stats[1], stats[2], gray


def _merge_compiled(model, planes, lut):
    """The ctypes form of checked planes, cached in the model's program cache.  The arrays stay referenced from the entry."""
    from . import _lib

    def freeze(el):
        if isinstance(el, np.ndarray):
            return ("array", el.shape, el.tobytes())
        if isinstance(el, tuple):
            return tuple(freeze(v) for v in el)
        return el
    key = ("merge", tuple((None if s is None else tuple(int(v) for v in s), tuple(tuple(freeze(v) for v in st) for st in p), int(o))
                          for s, p, o in planes), None if lut is None else np.asarray(lut, np.uint8).tobytes())
    if key in model._morph_programs:
        return model._morph_programs[key]
    table, out_values, elements, steps = check_planes(planes, lut)
    c_el = (_lib.MorphElement * max(len(elements), 1))()
    for i, (arr, (ax, ay)) in enumerate(elements):
        c_el[i] = _lib.MorphElement(arr.shape[1], arr.shape[0], ax, ay, arr.ctypes.data)
    c_st = (_lib.MergeStep * max(len(steps), 1))()
    for i, st in enumerate(steps):
        c_st[i] = _lib.MergeStep(*st)
    c_ov = (ctypes.c_int32 * len(out_values))(*out_values)
    entry = (elements, table, table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(out_values), c_ov, c_el, len(elements), c_st, len(steps))
    model._morph_programs[key] = entry
    return entry


def merge_layout(shape, planes, lut=None):
    """(band_rows, tile_cols) of unetpp_merge_classes for a [B,H,W] shape: the rows and columns of a frame one workgroup owns."""
    from . import _lib
    _, _, elements, steps = check_planes(planes, lut)
    c_el = (_lib.MorphElement * max(len(elements), 1))()
    for i, (arr, (ax, ay)) in enumerate(elements):
        c_el[i] = _lib.MorphElement(arr.shape[1], arr.shape[0], ax, ay, arr.ctypes.data)
    c_st = (_lib.MergeStep * max(len(steps), 1))(*[_lib.MergeStep(*st) for st in steps])
    band, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.load().unetpp_merge_classes_layout(int(shape[0]), int(shape[1]), int(shape[2]), len(list(planes)), c_el, len(elements), c_st, len(steps),
                                                 ctypes.byref(band), ctypes.byref(cols))
    if rc != 0:
        raise ValueError(f"unetpp_merge_classes_layout refused {tuple(shape)} (code {rc})")
    return band.value, cols.value


def merge_classes(model, mask, planes, *, lut=None, want_table=True, num_classes=256, want_mask=True):
    """merge_classes_np on the device for a uint8 CUDA map [B,H,W], in ONE launch (plus the table's initialisation): the planes
    are cut from one read of the map, every plane's program runs in LDS, and the merged map and its class table int32
    [B,num_classes,5] (count, x0, y0, x1, y1) are written.  Returns (out, table), or out alone without want_table, or (with
    want_mask=False) the table alone.  ValueError for what the kernel does not support (check_planes)."""
    import torch
    compiled = _merge_compiled(model, planes, lut)
    c = _check_classes(num_classes)
    if not (want_table or want_mask):
        raise ValueError("nothing to compute: want_table and want_mask are both off")
    mask = model._input(mask, "mask")
    b, h, w = mask.shape
    _, _, c_lut, n_planes, c_ov, c_el, n_el, c_st, n_st = compiled
    out = torch.empty((b, h, w), dtype=torch.uint8, device=mask.device) if want_mask else None
    table = torch.empty((b, c, 5), dtype=torch.int32, device=mask.device) if want_table else None
    model._call("unetpp_merge_classes", mask, b, h, w, c_lut, n_planes, c_ov, c_el, n_el, c_st, n_st, out, table, c, stream_of=mask)
    return (out, table) if want_table and want_mask else out if want_mask else table


def clean_classes_video(model, pred, want_table=True, num_classes=256):
    """infer_video.py:198-216 on the device for a uint8 CUDA class map [B,H,W] at frame size (resize_masks' output): class 4
    becomes 0, cable and tape are closed with E3, the defects {3, 5, 6} pass raw, defect > tape > cable.  One launch; returns
    (mask, table) or the mask."""
    return merge_classes(model, pred, PLANES_VIDEO, want_table=want_table, num_classes=num_classes)


def class_table(model, mask, num_classes=256):
    """class_table_np on the device: int32 [B,num_classes,5].  The merge kernel with one plane "value != 0" that passes as
    itself, no program and no map written: one read of the mask."""
    return merge_classes(model, mask, PLANES_TABLE, want_table=True, num_classes=num_classes, want_mask=False)


def threshold_classes(model, probs, frame_hw=None, *, cable_thr=0.60, tape_thr=0.60, defect_thr=0.70, ratio=1.2, channels=(1, 2, 3, 4, 5),
                      layout="nchw"):
    """threshold_classes_np on the device for a float32 CUDA tensor [B,C,h,w] (predict_proba's output) or, with layout="nhwc",
    [B,h,w,C] (predict_tiled(blend="probs")'s): the five planes are read in place, resized to frame_hw inside the kernel (four
    taps per output pixel, no full-size float plane), and one uint8 bit map [B,frame_h,frame_w] is written.  One launch."""
    import torch
    probs = model._input(probs, "probs", "[B,C,H,W]", "float32")
    b, c, h, w, channels = _check_probs(probs, channels, layout)
    thr, r = _thresholds(cable_thr, tape_thr, defect_thr, ratio)
    fh, fw = _frame_hw(frame_hw, h, w)
    if layout == "nchw":
        frame_stride, pixel_stride, offsets = c * h * w, 1, [k * h * w for k in channels]
    else:
        frame_stride, pixel_stride, offsets = h * w * c, c, list(channels)
    bits = torch.empty((b, fh, fw), dtype=torch.uint8, device=probs.device)
    model._call("unetpp_threshold_classes_f32", probs, frame_stride, pixel_stride, (ctypes.c_int64 * 5)(*offsets), b, h, w,
                thr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float(r), fh, fw, bits, stream_of=probs)
    return bits


def predict_v3(model, probs, frame_hw=None, *, want_table=True, num_classes=256, **thresholds):
    """predict_v3_np on the device: threshold_classes, then merge_classes with PLANES_V3.  Two launches; (mask, table) or the mask."""
    bits = threshold_classes(model, probs, frame_hw, **thresholds)
    return merge_classes(model, bits, PLANES_V3, lut=LUT_BITS, want_table=want_table, num_classes=num_classes)


def overlay(model, frames, mask, colors, alpha=0.5, mode="region", num_classes=None):
    """overlay_np on the device for uint8 CUDA frames [B,H,W,3] and a uint8 CUDA map [B,H,W]: uint8 [B,H,W,3], one launch.
    findContours / drawContours(..., 2), cv2.rectangle and putText stay on the host."""
    import torch
    from . import _lib
    table, has = color_table(colors, num_classes)
    w0, w1 = _weights(alpha, mode)
    frames = model._input(frames, "frames", "[B,H,W,3]")
    mask = model._input(mask, "mask")
    _check_overlay(frames, mask)
    b, h, w = mask.shape
    out = torch.empty_like(frames)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    model._call("unetpp_overlay_u8", frames, mask, b, h, w, table.ctypes.data_as(u8p), has.ctypes.data_as(u8p), float(w0), float(w1),
                _lib.OVERLAY_MODES[mode], out, stream_of=frames)
    return out
