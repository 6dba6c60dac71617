"""The pixel rules, component rules and class clean-ups of the spatial, fixed and simple video loops, in NumPy (torch-free) and on
the device (include/unetpp_simple_loops.h; csrc/simple_loops.h).  Per reference script:
  infer_video_spatial.py            relative_threshold :71-98                     -> relative_threshold
                                    create_vertical_focus_region :56-68, :155-156 -> column_band
  infer_video_simple_v2.py          simple_threshold :36-58                       -> confidence_threshold
  infer_video_fixed.py              filter_by_size_and_shape :85-105              -> keep_components
  infer_video_simple_optimized.py   spatial_filter_tape :88-137                   -> tape_position_filter
                                    predict from the softmax planes on :156-234   -> predict_simple(variant="optimized")
  infer_video_simple.py             predict from the softmax planes on :98-154    -> predict_simple(variant="simple")
  infer_video_simple_backup.py      the clean-up of predict :81-88                -> predict_simple_backup
Every device function takes the model and has its NumPy form here (<name>_np); the device results equal them bit for bit.  The
whole loops are frame_loop.process_frames_spatial, _fixed, _confidence and _simple.

How the reference computes (NumPy 2, see multiclass.py's docstring): `cable > bg * 2.0`, `cable >= 0.3` on float32 arrays round
the Python scalar to float32 and multiply and compare in float32.  np.argmax answers the first maximum, and the first NaN where
there is one; a comparison with a NaN is false.  The forms below are the reference's own expressions, so whatever they give for
NaN and infinite values is the definition.

The reference's `if np.sum(mask) > 0` guards in front of morphologyEx and connectedComponentsWithStats are no-ops (an empty mask
stays empty), so there is no branch for them; the guards inside spatial_filter_tape are its exits and live in a device table.
"""
from __future__ import annotations

import hashlib
import math

import numpy as np

from . import components as cc
from . import evaluation as ev
from . import morphology as mo
from . import multiclass as mc
from . import tiling as tl

TABLE_COLS = ("x_min", "x_max", "original_area", "filtered_area", "verdict", "reserved")
MAX_TAPE_PIXELS = 1 << 23                           # sums of uint8 values stay inside int32 (csrc/simple_loops.h)
INT_MAX = 2 ** 31 - 1
BIT_CABLE, BIT_TAPE, BIT_BURR, BIT_KEPT_BURR = 4, 8, 16, 32          # threshold_planes' bits; the burr after its component filter
VARIANTS = {
    # thresholds of planes 1, 2, 5; the programs of the cable and the tape (multiclass.check_planes' notation)
    "simple": dict(thresholds=(0.35, 0.35, 0.70), cable=(("close", 5, 2), ("dilate", 3)), tape=(("close", 5, 2), ("dilate", 3))),
    "optimized": dict(thresholds=(0.30, 0.55, 0.70), cable=(("close", 5, 2),), tape=(("close", 5),)),
}
BURR_PROGRAM = (("open", 3),)
PLANE_CHANNELS = (1, 2, 5)                          # cable, tape, burr of the 7-class SimpleUNet


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _check_probs(probs, layout):
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw' or 'nhwc', got {layout!r}")
    if ev._dtype_name(probs) != "float32" or len(probs.shape) != 4:
        raise ValueError(f"probs must be float32 [B,C,H,W] (or [B,H,W,C] with layout='nhwc'), got {ev._dtype_name(probs)} {list(probs.shape)}")
    shape = tuple(int(v) for v in probs.shape)
    b, c, h, w = shape if layout == "nchw" else (shape[0], shape[3], shape[1], shape[2])
    if min(b, h, w) < 1 or c < 3:
        raise ValueError(f"probs is {list(shape)}: needs B, H, W >= 1 and C >= 3")
    return b, c, h, w


def _f32(value, what):
    v = np.float32(value)
    if np.isnan(v):
        raise ValueError(f"{what} is NaN")
    return v


def _check_masks(*masks):
    first = masks[0]
    for m in masks:
        if ev._dtype_name(m) != "uint8" or len(m.shape) != 3 or min(m.shape) < 1 or tuple(m.shape) != tuple(first.shape):
            raise ValueError(f"masks must be uint8 [B,H,W] of one shape, got {ev._dtype_name(m)} {list(m.shape)}")
    return tuple(int(v) for v in first.shape)


def component_bounds(min_area, max_area=None, min_width=0):
    """(min_area, max_area, min_width) as the int32 the device compares with: an area is an integer, so area >= x is
    area >= ceil(x) and area <= x is area <= floor(x).  max_area=None: no upper bound.  ValueError for a NaN."""
    vals = [min_area, INT_MAX if max_area is None else max_area, min_width]
    if any(isinstance(v, float) and v != v for v in vals):
        raise ValueError("min_area, max_area and min_width must be numbers, got a NaN")
    lo, hi, wd = math.ceil(vals[0]), math.floor(vals[1]), math.ceil(vals[2])
    clamp = lambda v: int(max(-INT_MAX - 1, min(INT_MAX, v)))
    return clamp(lo), clamp(hi), clamp(wd)


def band_columns(w, lo=0.25, hi=0.75):
    """(x_start, x_end) of create_vertical_focus_region for width w: int(w * 0.25), int(w * 0.75)."""
    lo, hi = float(lo), float(hi)
    if not (0.0 <= lo <= 1.0 and 0.0 <= hi <= 1.0):
        raise ValueError(f"the band's fractions must lie in [0, 1], got {lo!r}, {hi!r}")
    return int(w * lo), int(w * hi)


def _check_variant(variant):
    if variant not in VARIANTS:
        raise ValueError(f"variant must be one of {sorted(VARIANTS)}, got {variant!r}")
    return VARIANTS[variant]


# ---- 1. the two pixel rules --------------------------------------------------------------------------------------------------------
def _hwc(probs, layout):
    p = np.asarray(probs)
    return p.transpose(0, 2, 3, 1) if layout == "nchw" else p


def relative_threshold_np(probs, cable_bg_ratio=2.0, tape_bg_ratio=2.5, layout="nchw"):
    """relative_threshold (infer_video_spatial.py:71-98) per frame of float32 probs [B,C,H,W] (C >= 3): (mask_cable, mask_tape)
    uint8 0/1 [B,H,W]."""
    _check_probs(probs, layout)
    rc, rt = _f32(cable_bg_ratio, "cable_bg_ratio"), _f32(tape_bg_ratio, "tape_bg_ratio")
    p = _hwc(probs, layout)
    bg, cable, tape = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        mask_cable = (cable > bg * rc).astype(np.uint8)
        mask_tape = (tape > bg * rt).astype(np.uint8)
        overlap = (mask_cable & mask_tape).astype(bool)
        if overlap.any():
            cable_wins = cable[overlap] >= tape[overlap]
            mask_cable[overlap] = cable_wins.astype(np.uint8)
            mask_tape[overlap] = (~cable_wins).astype(np.uint8)
    return mask_cable, mask_tape


def confidence_threshold_np(probs, conf_threshold=0.3, layout="nchw"):
    """simple_threshold (infer_video_simple_v2.py:36-58) per frame of float32 probs [B,C,H,W] (C >= 3): (mask_cable, mask_tape)
    uint8 0/1 [B,H,W]."""
    _check_probs(probs, layout)
    thr = _f32(conf_threshold, "conf_threshold")
    p = _hwc(probs, layout)
    cable, tape = p[..., 1], p[..., 2]
    winner = np.argmax(p[..., :3], axis=-1)
    with np.errstate(invalid="ignore"):
        mask_cable = (winner == 1) & (cable >= thr)
        mask_tape = (winner == 2) & (tape >= thr)
    return mask_cable.astype(np.uint8), mask_tape.astype(np.uint8)


# ---- 2. the area / box-width rule ---------------------------------------------------------------------------------------------------
def keep_components_np(mask, min_area, max_area=None, min_width=0, *, match_class=-1, out_value=1):
    """uint8 [B,H,W]: out_value on EVERY 8-connected component of (mask == match_class; != 0 for match_class < 0) with
    min_area <= area (<= max_area when given) and bounding-box width >= min_width.  filter_by_size_and_shape
    (infer_video_fixed.py:85-105) is (min_area, max_area); the tape filter of infer_video_simple_optimized.py:194-208 is
    (500, min_width=20); the burr filter (:213-226, infer_video_simple.py:137-146) is (100,)."""
    b, h, w = _check_masks(mask)
    lo, hi, wd = component_bounds(min_area, max_area, min_width)
    out = np.zeros((b, h, w), np.uint8)
    for i, m in enumerate(np.asarray(mask)):
        labels, stats, _ = cc.components_np(m, 8, match_class)
        area, width = stats[:, cc.CC_STAT_AREA].astype(np.int64), stats[:, cc.CC_STAT_WIDTH].astype(np.int64)
        keep = (area >= lo) & (area <= hi) & (width >= wd)
        keep[0] = False
        out[i] = keep[labels] * np.uint8(out_value)
    return out


# ---- 3. spatial_filter_tape ----------------------------------------------------------------------------------------------------------
def valid_ranges(x_min, x_max, w):
    """The two column ranges of spatial_filter_tape (:116-121) as Python slices' bounds: (l0, l1, r0, r1)."""
    x_min, x_max, w = int(x_min), int(x_max), int(w)
    cw = x_max - x_min
    return max(0, x_min - cw // 2), x_min + cw // 3, max(x_min + 2 * cw // 3, x_max - cw // 3), min(w, x_max + cw // 2)


def tape_position_filter_np(tape, cable):
    """spatial_filter_tape (infer_video_simple_optimized.py:88-137) per frame of uint8 masks [B,H,W]: (filtered uint8 [B,H,W],
    table int32 [B,6] = x_min, x_max, original_area, filtered_area, verdict, 0).  The areas are np.sum of the values, as in the
    reference (pixel counts for its 0/1 masks); verdict 1 = the filtered tape is the result, 0 = the tape came back unchanged
    (no cable: extents -1; no tape; or 2 * filtered_area < original_area).  filtered_area is 0 where no filter was tried."""
    b, h, w = _check_masks(tape, cable)
    if h * w > MAX_TAPE_PIXELS:
        raise ValueError(f"frames of {h}x{w}: the tape filter takes H * W <= {MAX_TAPE_PIXELS}")
    tape, cable = np.asarray(tape), np.asarray(cable)
    out = tape.copy()
    table = np.zeros((b, 6), np.int32)
    for i in range(b):
        xs = np.where(cable[i] > 0)[1]
        x_min, x_max = (int(xs.min()), int(xs.max())) if xs.size else (-1, -1)
        original = int(np.sum(tape[i], dtype=np.int64))
        table[i, :3] = (x_min, x_max, original)
        if xs.size == 0 or original == 0:
            continue
        l0, l1, r0, r1 = valid_ranges(x_min, x_max, w)
        valid = np.zeros_like(tape[i])
        valid[:, l0:l1] = 1
        valid[:, r0:r1] = 1
        filtered = tape[i] & valid
        area = int(np.sum(filtered, dtype=np.int64))
        table[i, 3] = area
        if not area < original * 0.5:
            out[i] = filtered
            table[i, 4] = 1
    return out, table


# ---- 4. the focus band ---------------------------------------------------------------------------------------------------------------
def column_band_np(mask, lo=0.25, hi=0.75):
    """mask & create_vertical_focus_region (infer_video_spatial.py:56-68, :155-156) for uint8 masks [B,H,W]: mask & 1 in the
    columns [int(w * lo), int(w * hi)), 0 in the others."""
    b, h, w = _check_masks(mask)
    x0, x1 = band_columns(w, lo, hi)
    focus = np.zeros((h, w), np.uint8)
    focus[:, x0:x1] = 1
    return np.asarray(mask) & focus


# ---- the three NestedUNet loops after the network, composed as infer_frame composes them ----------------------------------------------
def _resize_back(mask, frame_hw):
    from . import robust as rb
    return np.stack([rb.resize_nearest_np(m, (int(frame_hw[1]), int(frame_hw[0]))) for m in mask])


def postprocess_spatial_np(probs, frame_hw, cable_bg_ratio=2.0, tape_bg_ratio=2.5):
    """infer_video_spatial.py:145-171 for float32 probs [B,C,S,S]: (mask_cable, mask_tape uint8 [B,fh,fw], metrics: a list of
    dicts with cable_coverage and tape_coverage)."""
    c, t = relative_threshold_np(probs, cable_bg_ratio, tape_bg_ratio)
    c = np.stack([cc.filter_components_np(m, -1, "spatial", min_width=30, max_width=200) for m in c])
    t = np.stack([cc.filter_components_np(m, -1, "spatial", min_width=20, max_width=150) for m in t])
    c, t = column_band_np(c), column_band_np(t)
    metrics = [{"cable_coverage": int(a.sum()) / a.size, "tape_coverage": int(b_.sum()) / b_.size} for a, b_ in zip(c, t)]
    return _resize_back(c, frame_hw), _resize_back(t, frame_hw), metrics


def measured_tail_np(cable_s, tape_s, frame_hw):
    """infer_video_fixed.py:210-234 (= infer_video_simple_v2.py:135-159) for uint8 0/1 masks [B,S,S]: (mask_cable, mask_tape
    at frame size, metrics: a list of dicts of robust.MEASURE_FIELDS, pred_mask uint8 [B,S,S])."""
    from . import robust as rb
    metrics = [rb.measure_diameters_np(a, b_) for a, b_ in zip(cable_s, tape_s)]
    pred = np.zeros_like(cable_s)
    pred[cable_s > 0] = 1
    pred[tape_s > 0] = 2
    return _resize_back(cable_s, frame_hw), _resize_back(tape_s, frame_hw), metrics, pred


def postprocess_fixed_np(cable_s, tape_s, frame_hw, min_area_cable=3000, min_area_tape=1500, max_area_cable=100000, max_area_tape=80000):
    """infer_video_fixed.py:198-234 after strict_threshold_with_bg_check for uint8 0/1 masks [B,S,S]."""
    return measured_tail_np(keep_components_np(cable_s, min_area_cable, max_area_cable), keep_components_np(tape_s, min_area_tape, max_area_tape),
                            frame_hw)


# ---- 5. the clean-up of the SimpleUNet loops -------------------------------------------------------------------------------------------
def _frame_hw(frame_hw):
    fh, fw = int(frame_hw[0]), int(frame_hw[1])
    if fh < 1 or fw < 1:
        raise ValueError(f"frame_hw must be positive, got {frame_hw!r}")
    return fh, fw


def _check_planes(probs, channels):
    if ev._dtype_name(probs) != "float32" or len(probs.shape) != 4 or min(probs.shape) < 1:
        raise ValueError(f"probs must be float32 [B,C,h,w], got {ev._dtype_name(probs)} {list(probs.shape)}")
    channels = tuple(int(k) for k in channels)
    if len(channels) != 3 or any(not 0 <= k < probs.shape[1] for k in channels):
        raise ValueError(f"channels must be three indices in [0,{probs.shape[1]}), got {channels!r}")
    return channels


def threshold_planes_np(probs, frame_hw, thresholds, channels=PLANE_CHANNELS):
    """The head of the three predict bodies (infer_video_simple.py:98-115): planes `channels` (cable, tape, burr) of float32 probs
    [B,C,h,w] resized to frame_hw as tiling.resize_linear_f32_np states the float32 INTER_LINEAR resize, then `plane >= thr` with
    the scalar rounded to float32.  uint8 [B,fh,fw] with BIT_CABLE, BIT_TAPE, BIT_BURR (4, 8, 16); NaN sets no bit."""
    channels = _check_planes(probs, channels)
    thr = [_f32(t, "a threshold") for t in thresholds]
    if len(thr) != 3:
        raise ValueError("three thresholds: cable, tape, burr")
    fh, fw = _frame_hw(frame_hw)
    probs = np.asarray(probs)
    out = np.zeros((len(probs), fh, fw), np.uint8)
    for i in range(len(probs)):
        for k, t, bit in zip(channels, thr, (BIT_CABLE, BIT_TAPE, BIT_BURR)):
            plane = np.ascontiguousarray(probs[i, k])
            with np.errstate(invalid="ignore"):                           # 0 * inf in the resize, comparisons with NaN
                if plane.shape != (fh, fw):
                    plane = tl.resize_linear_f32_np(plane, (fw, fh))
                out[i] |= (plane >= t).astype(np.uint8) * np.uint8(bit)
    return out


def _run_program(x, program):
    """A plane program of multiclass.check_planes' notation on a boolean image, with cv2.morphologyEx's semantics."""
    x = np.asarray(x) != 0
    for st in program:
        el, it = mo.structuring_element("ellipse", int(st[1])), (int(st[2]) if len(st) > 2 else 1)
        if st[0] == "dilate":
            x = mo.dilate_np(x, el, None, it)
        elif st[0] == "erode":
            x = mo.erode_np(x, el, None, it)
        elif st[0] == "open":
            x = mo.dilate_np(mo.erode_np(x, el, None, it), el, None, it)
        else:
            x = mo.erode_np(mo.dilate_np(x, el, None, it), el, None, it)
    return x


def predict_simple_np(probs, frame_hw, variant="simple", *, min_tape_area=500, min_tape_width=20, min_burr_area=100, want_table=True,
                      return_tape_table=False):
    """SimpleInference.predict from the softmax planes on (variant "simple": infer_video_simple.py:98-154; "optimized":
    infer_video_simple_optimized.py:156-234) for float32 probs [B,7,h,w]: the merged map uint8 [B,fh,fw] with cable 1, tape 2,
    burr 5 (a later one over an earlier one), and with want_table multiclass.class_table_np of it.  return_tape_table adds the
    table of tape_position_filter_np (variant "optimized" only), so that a test sees which exit a frame took."""
    v = _check_variant(variant)
    bits = threshold_planes_np(probs, frame_hw, v["thresholds"])
    out = np.zeros_like(bits)
    tape_table = None
    cable = np.stack([_run_program(m & BIT_CABLE, v["cable"]) for m in bits]).astype(np.uint8)
    tape = np.stack([_run_program(m & BIT_TAPE, v["tape"]) for m in bits]).astype(np.uint8)
    if variant == "optimized":
        tape = tape & ~cable
        tape, tape_table = tape_position_filter_np(tape, cable)
        tape = keep_components_np(tape, min_tape_area, None, min_tape_width)
    burr = np.stack([_run_program(m & BIT_BURR, BURR_PROGRAM) for m in bits]).astype(np.uint8)
    burr = keep_components_np(burr, min_burr_area)
    out[cable > 0] = 1
    out[tape > 0] = 2
    out[burr > 0] = 5
    res = (out, mc.class_table_np(out)) if want_table else (out,)
    if return_tape_table:
        res = res + (tape_table,)
    return res if len(res) > 1 else res[0]


def predict_simple_backup_np(pred, want_table=True):
    """The clean-up of infer_video_simple_backup.py:81-88 on a uint8 class map [B,H,W] already at frame size: close(pred == 1, E3)
    is written as 1, THEN the tape plane is taken from the updated map (tape pixels the cable's closing overwrote are gone),
    closed and written as 2; every other value stays where neither wrote."""
    _check_masks(pred)
    out = np.array(pred, np.uint8, copy=True)
    el = mo.structuring_element("ellipse", 3)
    for m in out:
        for cid in (1, 2):
            x = m == cid
            m[mo.erode_np(mo.dilate_np(x, el), el)] = cid
    return (out, mc.class_table_np(out)) if want_table else out


# the planes of multiclass.merge_classes that express the steps above (select None: a bit map through multiclass.LUT_BITS' kin)
def _lut(bit_of_plane):
    t = np.zeros(256, np.uint8)
    v = np.arange(256)
    for k, bit in enumerate(bit_of_plane):
        t[(v & bit) != 0] |= 1 << k
    return t


PLANES_BURR = ((None, BURR_PROGRAM, 1),)
LUT_BURR = _lut((BIT_BURR,))
LUT_SIMPLE = _lut((BIT_CABLE, BIT_TAPE, BIT_KEPT_BURR))
LUT_TAPE_CABLE = _lut((BIT_TAPE, BIT_CABLE))
LUT_JOINED = _lut((1, 2, 4))
PLANES_JOINED = ((None, (), 1), (None, (), 2), (None, (), 5))
# backup: everything passes as itself, then the closed plane is written over it -- twice, the second launch on the first's map
PLANES_BACKUP = tuple(((range(1, 256), (), -1), ((cid,), (("close", 3),), cid)) for cid in (1, 2))


# ---- seeded inputs of the fixtures and tests ------------------------------------------------------------------------------------------
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return np.packbits(np.asarray(a) != 0)


def unbits(packed, shape):
    n = int(np.prod(shape))
    return np.unpackbits(packed)[:n].reshape(shape)


def make_random_probs(b, c, h, w, seed, specials=False, layout="nchw"):
    """float32 softmax planes [b,c,h,w] of smooth random logits with a low-background cable / tape region, so that both ratios of
    relative_threshold hold on many pixels at once.  specials=True plants NaN and +-inf in every channel, two NaNs in one pixel
    and a tie at +inf.  For the device tests; the reference's relative_threshold cannot be run on it (make_probs says why)."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    logits = r.normal(0, 0.6, (b, c, h, w))
    for i in range(b):
        cx = w * (0.35 + 0.3 * r.random())
        logits[i, 0] += 2.0 * (np.abs(x - cx) > w * 0.22)
        logits[i, 1] += 2.2 * (np.abs(x - cx) <= w * 0.12) + 1.0 * (np.abs(x - cx) <= w * 0.22)
        logits[i, 2] += 2.2 * ((np.abs(x - cx) > w * 0.10) & (np.abs(x - cx) <= w * 0.22)) + 1.0 * (np.abs(x - cx) <= w * 0.22)
    e = np.exp(logits - logits.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(np.float32)
    p[0, :3, 0, 0] = (0.1, 0.45, 0.45)                                    # cable == tape, both above their ratios
    if specials:
        flat = p.reshape(b, c, -1)
        n = flat.shape[2]
        for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
            flat[k % b, k % 3, (7 * k + 5) % n] = v                       # one special per pixel, every channel with every value
        flat[b - 1, 0, n - 1] = flat[b - 1, 1, n - 1] = np.nan            # two NaNs in one pixel: the first wins the argmax
        flat[b - 1, 1, n - 2] = flat[b - 1, 2, n - 2] = np.inf            # a tie at +inf
    return p if layout == "nchw" else np.ascontiguousarray(p.transpose(0, 2, 3, 1))


def make_probs(b, c, h, w, seed, specials=False):
    """float32 planes [b,c,h,w] on which the reference's relative_threshold computes the rule it documents.  Its lines :88-96
    index with a uint8 array, which NumPy reads as ROW NUMBERS: once a frame has an overlap pixel they rewrite rows 0 and 1 of
    both masks as `cable >= tape` / its negation and leave every overlap in the other rows standing.  So here a frame's
    overlaps lie in row 0 only, and rows 0 and 1 of such a frame hold no background pixel (there the rewrite and the rule
    agree).  Frame 0: rows 0 and 1 cable on the left half, tape on the right, and three overlap pixels with a background of
    0.1: (0,0) cable == tape, (0,1) tape above cable, (0,2) cable above tape.  The other frames have no overlap.  Everywhere
    else: a cable strip, tape on both sides of it, background outside, each value within 10 % of (0.8, 0.1, 0.1).
    specials=True plants NaN and +-inf in the frames without an overlap, in places where no overlap arises from them."""
    r = np.random.default_rng(seed)
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    p = np.zeros((b, c, h, w), np.float32)
    zones = []
    for i in range(b):
        cx = w * (0.4 + 0.2 * r.random())
        zone = np.where(np.abs(x - cx) <= w * 0.15, 1, np.where(np.abs(x - cx) <= w * 0.28, 2, 0))
        if i == 0:
            zone[:2] = np.where(x[:2] < w // 2, 1, 2)
        zones.append(zone)
        for k in range(c):
            p[i, k] = np.where(zone == k, 0.8, 0.1 if k < 3 else 0.02) * (0.9 + 0.2 * r.random((h, w)))
    p[0, :3, 0, 0] = (0.1, 0.45, 0.45)
    p[0, :3, 0, 1] = (0.1, 0.4, 0.5)
    p[0, :3, 0, 2] = (0.1, 0.5, 0.4)
    if specials and b > 1:
        flat = p.reshape(b, c, -1)
        n = flat.shape[2]
        for k, (ch, v) in enumerate(((0, np.nan), (0, np.inf), (1, np.nan), (1, np.inf), (1, -np.inf), (2, np.nan), (2, np.inf), (2, -np.inf))):
            f = 1 + k % (b - 1)
            ok = np.flatnonzero((zones[f] != 3 - ch).reshape(-1)) if v == np.inf and ch else np.arange(n)    # +inf never beside the other class
            flat[f, ch, ok[(11 * k + 3 * w + 5) % len(ok)]] = v
        flat[b - 1, 0, n - 1] = flat[b - 1, 1, n - 1] = np.nan            # two NaNs in one pixel: the first wins the argmax
    return p


TAPE_SCENES = ("no_cable", "no_tape", "fallback", "filtered", "one_column_cable")


def make_tape_scene(kind, h=64, w=96):
    """(tape, cable) uint8 0/1 [h,w] for one exit of spatial_filter_tape each."""
    tape, cable = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    c0, c1 = w // 2 - w // 8, w // 2 + w // 8
    if kind != "no_cable":
        cable[h // 8:h - h // 8, c0:c1] = 1
    if kind == "one_column_cable":
        cable[:] = 0
        cable[h // 4:h // 2, w // 3] = 1                                  # cw = 0: both ranges are empty, the filtered area is 0
    if kind in ("no_cable", "filtered", "one_column_cable"):
        tape[h // 4:h - h // 4, c0 - w // 12:c0] = 1                      # hugs the cable on both sides
        tape[h // 4:h - h // 4, c1:c1 + w // 12] = 1
        tape[2:6, 1:5] = 1                                                # and a far blob the filter removes
    if kind == "fallback":
        tape[h // 4:h - h // 4, 0:w // 8] = 1                             # most of the tape far from the cable
        tape[h // 4:h // 2, c1:c1 + 3] = 1
    return tape, cable


def make_component_scene(h=96, w=128):
    """uint8 0/1 [h,w]: components on either side of every bound the reference's filters use: areas 99 and 100 (a burr on either
    side of 100), 40 x 12 = 480 (below 500 at width 40: rejected by area only), 10 x 60 = 600 (width 10: rejected by width
    only), 40 x 20 = 800 (kept by every rule), a diagonal pair and a single pixel."""
    m = np.zeros((h, w), np.uint8)
    m[2:13, 2:11] = 1                     # 11 rows x 9 columns = 99
    m[2:12, 14:24] = 1                    # 100
    m[16:28, 2:42] = 1                    # 480, width 40
    m[32:92, 2:12] = 1                    # 600, width 10
    m[40:60, 50:90] = 1                   # 800, width 40
    m[90, 120] = m[91, 121] = 1           # touching diagonally: one component of area 2
    m[5, 100] = 1
    return m


def make_backup_map(h=48, w=64, seed=0):
    """uint8 class map [h,w] with values 0..6: two cable blocks with a one-pixel gap that holds tape pixels (the cable's closing
    overwrites them), a tape region with holes, and speckle of the other classes."""
    r = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    m[4:h - 4, w // 2 - 8:w // 2] = 1
    m[4:h - 4, w // 2 + 1:w // 2 + 9] = 1
    m[4:h - 4, w // 2] = 2                                                 # the gap: tape that the closed cable swallows
    m[8:h - 8, w // 2 + 9:w // 2 + 16] = 2
    m[10:h - 10:4, w // 2 + 11] = 0                                        # holes the tape's closing fills
    m[6:h - 6:5, w // 2 - 4] = 3                                           # a defect inside the cable: closed over
    s = r.random((h, w)) < 0.02
    m[s] = r.integers(3, 7, int(s.sum()), dtype=np.uint8)
    return m


PLANE_SCENES = ("filtered", "fallback", "no_cable", "no_tape")


def make_simple_planes(kind, h=32, w=32, seed=0):
    """float32 [7,h,w] in [0,1] as predict reads them (planes 1, 2, 5).  "filtered": a cable over the middle half with the tape
    on both sides of it, inside the columns spatial_filter_tape accepts; "fallback": a narrow cable and a wide tape far from it,
    so that less than half survives and the tape comes back whole; "no_cable", "no_tape".  Holes and noise give the closings
    and the opening something to do; one burr blob is large enough at frame size, one is not."""
    r = np.random.default_rng(seed + 17 * PLANE_SCENES.index(kind))
    y, x = np.mgrid[0:h, 0:w]
    p = (0.05 + 0.1 * r.random((7, h, w))).astype(np.float32)
    box = lambda x0, x1, y0, y1: (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    narrow = kind == "fallback"
    c0, c1 = (7 * w // 16, 9 * w // 16) if narrow else (w // 4, 3 * w // 4)
    if kind != "no_cable":
        cable = box(c0, c1, h // 8, h - h // 8)
        p[1][cable] = 0.8
        p[1][cable & (r.random((h, w)) < 0.08)] = 0.1                       # holes
    if kind != "no_tape":
        tape = box(0, 5 * w // 16, h // 4, 3 * h // 4) if narrow else (box(0, c0 + 2, h // 4, 3 * h // 4) | box(c1, w, h // 4, 3 * h // 4))
        p[2][tape] = 0.85                                                   # two columns overlap the cable: the exclusion removes them
        p[2][tape & (r.random((h, w)) < 0.05)] = 0.2
    p[5][box(w - 7, w - 2, 0, 5)] = 0.9                                     # 5 x 5 at plane size
    p[5][box(1, 3, 0, 2)] = 0.9                                             # 2 x 2
    p[5][(r.random((h, w)) < 0.01) & (y >= h - 3)] = 0.95
    return p


def make_simple_batch(kinds=PLANE_SCENES, h=32, w=32, seed=0):
    return np.stack([make_simple_planes(k, h, w, seed) for k in kinds])


# what the fixture file holds: scripts/make_golden_simple_loops.py writes it, the tests read it
FIXTURE_PROBS = (("probs_a", 2, 3, 24, 40, 0, False), ("probs_b", 2, 7, 17, 23, 1, True))
FIXTURE_LOOP_PROBS = ("probs_loop", 2, 3, 128, 128, 2, False)          # large enough for spatial_filter's area > 1000
FIXTURE_LOOP_FRAME = (72, 100)
FIXTURE_FRAME, FIXTURE_PLANE = (64, 96), (32, 32)
FIXTURE_COMPONENTS = (("burr", 100, None, 0), ("tape", 500, None, 20), ("band", 100, 600, 0))
SCALED_TAPE = dict(min_tape_area=60, min_tape_width=6, min_burr_area=20)      # the constants scaled down, for the device tests


def fixture_facts(g):
    """The conditions the fixtures must meet (asserted by the generator and by tests/test_simple_loops_host.py), from the stored
    results and the regenerated inputs; returns a dict of the figures."""
    facts = {}
    # relative_threshold: an overlap pixel decided each way and one with cable == tape
    name, b, c_, h, w, seed, specials = FIXTURE_PROBS[0]
    p = make_probs(b, c_, h, w, seed, specials)
    bg, cable, tape = p[0, 0], p[0, 1], p[0, 2]
    both = (cable > bg * np.float32(2.0)) & (tape > bg * np.float32(2.5))
    c, t = unbits(g[name + "_rel_cable"], (b, h, w))[0], unbits(g[name + "_rel_tape"], (b, h, w))[0]
    assert both[0, 0] and cable[0, 0] == tape[0, 0] and c[0, 0] == 1 and t[0, 0] == 0
    assert both[0, 1] and cable[0, 1] < tape[0, 1] and c[0, 1] == 0 and t[0, 1] == 1
    assert both[0, 2] and cable[0, 2] > tape[0, 2] and c[0, 2] == 1 and t[0, 2] == 0
    assert not (c & t).any() and c.any() and t.any()
    facts["overlap_pixels"] = int(both.sum())
    # every exit of spatial_filter_tape
    exits = {}
    for kind in TAPE_SCENES:
        tp, _ = make_tape_scene(kind)
        exits[kind] = tuple(int(v) for v in g[f"tape_{kind}_table"])
        changed = bool((unbits(g[f"tape_{kind}_out"], tp.shape) != tp).any())
        assert changed == (exits[kind][4] == 1 and exits[kind][3] < exits[kind][2]), kind
    assert exits["no_cable"][:2] == (-1, -1) and exits["no_cable"][4] == 0 and exits["no_cable"][2] > 0
    assert exits["no_tape"][2] == 0 and exits["no_tape"][0] >= 0 and exits["no_tape"][4] == 0
    assert exits["fallback"][4] == 0 and 0 < 2 * exits["fallback"][3] < exits["fallback"][2]
    assert exits["filtered"][4] == 1 and exits["filtered"][3] < exits["filtered"][2] <= 2 * exits["filtered"][3]
    assert exits["one_column_cable"][0] == exits["one_column_cable"][1] >= 0 and exits["one_column_cable"][3:5] == (0, 0)
    facts["tape_exits"] = exits
    # components on either side of every bound
    m = make_component_scene()
    _, stats, _ = cc.components_np(m, 8, -1)
    comps = list(zip(stats[1:, cc.CC_STAT_AREA].tolist(), stats[1:, cc.CC_STAT_WIDTH].tolist()))
    assert any(a == 99 for a, _ in comps) and any(a == 100 for a, _ in comps)                  # a burr on either side of 100
    assert any(a < 500 and wd >= 20 for a, wd in comps) and any(a >= 500 and wd < 20 for a, wd in comps)   # area only, width only
    kept = {n: int(unbits(g["components_" + n], m.shape).sum()) for n, *_ in FIXTURE_COMPONENTS}
    assert kept["burr"] == sum(a for a, _ in comps if a >= 100) and kept["tape"] == sum(a for a, wd in comps if a >= 500 and wd >= 20) > 0
    assert kept["band"] == sum(a for a, _ in comps if 100 <= a <= 600) and kept["band"] < kept["burr"]
    facts["components_kept"] = kept
    # the backup clean-up: the cable's closing overwrites tape pixels
    bm, out = make_backup_map(), g["backup_map"]
    facts["backup_tape_overwritten"] = int(((bm == 2) & (out == 1)).sum())
    assert facts["backup_tape_overwritten"] > 0 and ((bm == 0) & (out == 2)).any() and ((bm >= 3) & (out == bm)).any()
    # the predict scenes at the reference's constants: both verdicts, a tape that survives, a burr that does and one that does not
    verdicts = {kind: int(row[4]) for kind, row in zip(PLANE_SCENES, g["predict_optimized_tape_table"])}
    assert verdicts == {"filtered": 1, "fallback": 0, "no_cable": 0, "no_tape": 0}
    facts["predict_verdicts"] = verdicts
    for variant in ("simple", "optimized"):
        for kind, mp in zip(PLANE_SCENES, g[f"predict_{variant}_map"]):
            want = {0, 5} | ({1} if kind != "no_cable" else set()) | ({2} if kind != "no_tape" else set())
            assert set(np.unique(mp).tolist()) == want, (variant, kind, np.unique(mp).tolist())
        assert (g[f"predict_{variant}_map"][:, :12, :12] != 5).all()                           # the small burr blob is gone
    return facts


# ---- the device path (torch imported lazily, as in contours.py) -------------------------------------------------------------------------
def _probs(model, probs, layout):
    probs = model._input(probs, "probs", "[B,C,H,W]", "float32")
    b, c, h, w = _check_probs(probs, layout)
    strides = (c * h * w, h * w, 1) if layout == "nchw" else (h * w * c, 1, c)
    return probs, b, h, w, strides


def _pixel_rule(model, probs, layout, rule, a, b_):
    import torch
    from . import _lib
    probs, b, h, w, strides = _probs(model, probs, layout)
    cable, tape = (torch.empty((b, h, w), dtype=torch.uint8, device=probs.device) for _ in range(2))
    model._call("unetpp_pixel_rules_f32", probs, *strides, b, h, w, _lib.PIXEL_RULES[rule], float(a), float(b_), cable, tape, stream_of=probs)
    return cable, tape


def relative_threshold(model, probs, cable_bg_ratio=2.0, tape_bg_ratio=2.5, layout="nchw"):
    """relative_threshold_np on the device for float32 CUDA probabilities [B,C,H,W] (predict_proba's output) or, with
    layout="nhwc", [B,H,W,C], read in place: (mask_cable, mask_tape) uint8 0/1 [B,H,W], one launch."""
    return _pixel_rule(model, probs, layout, "relative", _f32(cable_bg_ratio, "cable_bg_ratio"), _f32(tape_bg_ratio, "tape_bg_ratio"))


def confidence_threshold(model, probs, conf_threshold=0.3, layout="nchw"):
    """confidence_threshold_np on the device: (mask_cable, mask_tape) uint8 0/1 [B,H,W], one launch."""
    thr = _f32(conf_threshold, "conf_threshold")
    return _pixel_rule(model, probs, layout, "confidence", thr, thr)


def _keep(model, mask, min_area, max_area, min_width, match_class, out_value, max_components):
    import torch
    out_value = model._check_out_value(out_value)
    lo, hi, wd = component_bounds(min_area, max_area, min_width)
    labels, num, stats, _, ws, _ = model._components(mask, match_class, 8, max_components, True)
    b, h, w = labels.shape
    k = int(max_components)
    out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
    model._call("unetpp_components_keep", labels, num, stats, b, h, w, k, lo, hi, wd, out_value, out, ws, stream_of=labels)
    return out, num, k


def keep_components(model, mask, min_area, max_area=None, min_width=0, *, match_class=-1, out_value=1, max_components=8192, check=True):
    """keep_components_np on the device for a uint8 CUDA mask [B,H,W].  max_components and check as for
    NestedUNet.filter_components: a frame with more components raises RuntimeError (check=True, one B-int read-back) or comes
    out all zero."""
    out, num, k = _keep(model, mask, min_area, max_area, min_width, match_class, out_value, max_components)
    if check:
        model._raise_num_overflow(num, k)
    return out


def _filter_spatial(model, mask, min_width, max_width, max_components):
    """NestedUNet.filter_components(mask, rule="spatial", check=False) that also hands back num, so that a loop checks the
    overflow of all its labellings in its one read-back."""
    import ctypes
    import torch
    from . import _lib
    labels, num, stats, sums, ws, _ = model._components(mask, -1, 8, max_components, True)
    b, h, w = labels.shape
    params = _lib.CcRule(1000.0, float(min_width), float(max_width), 0.3, 1.6, 0.3, float(w))
    out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
    model._call("unetpp_components_filter", labels, num, stats, sums, b, h, w, int(max_components), _lib.CC_RULES["spatial"], ctypes.byref(params),
                1, out, ws, stream_of=labels, invalid=RuntimeError)
    return out, num


def _tape_filter(model, tape, tape_match, cable, cable_match):
    import torch
    b, h, w = tape.shape
    if h * w > MAX_TAPE_PIXELS:
        raise ValueError(f"frames of {h}x{w}: the tape filter takes H * W <= {MAX_TAPE_PIXELS}")
    out = torch.empty((b, h, w), dtype=torch.uint8, device=tape.device)
    table = torch.empty((b, 6), dtype=torch.int32, device=tape.device)
    model._call("unetpp_tape_position_filter_u8", tape, int(tape_match), cable, int(cable_match), b, h, w, out, table, stream_of=tape)
    return out, table


def tape_position_filter(model, tape, cable):
    """tape_position_filter_np on the device for uint8 CUDA masks [B,H,W]: (filtered uint8 [B,H,W], table int32 [B,6]), both on
    the device.  The extents, the two areas and the verdict stay in the table between the launches; nothing is read back."""
    tape, cable = model._input(tape, "tape"), model._input(cable, "cable")
    _check_masks(tape, cable)
    return _tape_filter(model, tape, -1, cable, -1)


def column_band(model, mask, lo=0.25, hi=0.75):
    """column_band_np on the device for a uint8 CUDA mask [B,H,W]: one launch."""
    import torch
    mask = model._input(mask, "mask")
    b, h, w = _check_masks(mask)
    x0, x1 = band_columns(w, lo, hi)
    out = torch.empty((b, h, w), dtype=torch.uint8, device=mask.device)
    model._call("unetpp_column_band_u8", mask, b, h, w, x0, x1, out, stream_of=mask)
    return out


def _join(model, a, and_a, b_=None, or_b=0, c=None, or_c=0):
    import torch
    b, h, w = a.shape
    out = torch.empty((b, h, w), dtype=torch.uint8, device=a.device)
    model._call("unetpp_mask_join_u8", a, int(and_a), b_, int(or_b), c, int(or_c), b, h, w, out, stream_of=a)
    return out


def threshold_planes(model, probs, frame_hw, thresholds, channels=PLANE_CHANNELS):
    """threshold_planes_np on the device for float32 CUDA probs [B,C,h,w]: one launch of unetpp_threshold_classes_f32, whose
    bits 2..4 are the plain `plane >= threshold` of the planes handed to them.  Its bits 0 and 1 carry the v3 loop's ratio
    rule `p >= thr and p > q * ratio`; they get the same plane twice, threshold +inf and ratio +inf, under which no value sets
    them (inf > inf is false), so the map holds BIT_CABLE, BIT_TAPE and BIT_BURR only."""
    import ctypes
    import torch
    probs = model._input(probs, "probs", "[B,C,H,W]", "float32")
    channels = _check_planes(probs, channels)
    thr = np.array([np.inf, np.inf] + [_f32(t, "a threshold") for t in thresholds], np.float32)
    if len(thr) != 5:
        raise ValueError("three thresholds: cable, tape, burr")
    fh, fw = _frame_hw(frame_hw)
    b, c, h, w = (int(v) for v in probs.shape)
    offsets = [k * h * w for k in (channels[0], channels[0]) + channels]
    out = torch.empty((b, fh, fw), dtype=torch.uint8, device=probs.device)
    model._call("unetpp_threshold_classes_f32", probs, c * h * w, 1, (ctypes.c_int64 * 5)(*offsets), b, h, w,
                thr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float("inf"), fh, fw, out, stream_of=probs)
    return out


def _predict_simple(model, probs, frame_hw, variant, min_tape_area, min_tape_width, min_burr_area, want_table, max_components):
    """predict_simple without its check: (map, table or None, tape table or None, num int32 [B]: the largest num of the frame's
    labellings, max_components)."""
    import torch
    v = _check_variant(variant)
    bits_map = threshold_planes(model, probs, frame_hw, v["thresholds"])
    k = int(max_components)
    burr_open = mc.merge_classes(model, bits_map, PLANES_BURR, lut=LUT_BURR, want_table=False)
    burr, num, _ = _keep(model, burr_open, min_burr_area, None, 0, -1, 1, k)
    tape_table = None
    if variant == "simple":
        joined = _join(model, bits_map, BIT_CABLE | BIT_TAPE, burr, BIT_KEPT_BURR)
        planes = ((None, v["cable"], 1), (None, v["tape"], 2), (None, (), 5))
        res = mc.merge_classes(model, joined, planes, lut=LUT_SIMPLE, want_table=want_table)
    else:
        # one launch closes both planes; the cable, merged last, overwrites the tape: value 2 is tape & ~cable
        both = mc.merge_classes(model, bits_map, ((None, v["tape"], 2), (None, v["cable"], 1)), lut=LUT_TAPE_CABLE, want_table=False)
        tape, tape_table = _tape_filter(model, both, 2, both, 1)
        tape, num_t, _ = _keep(model, tape, min_tape_area, None, min_tape_width, -1, 1, k)
        num = torch.maximum(num, num_t)
        joined = _join(model, both, 1, tape, 2, burr, 4)
        res = mc.merge_classes(model, joined, PLANES_JOINED, lut=LUT_JOINED, want_table=want_table)
    out, table = res if want_table else (res, None)
    return out, table, tape_table, num, k


def predict_simple(model, probs, frame_hw, variant="simple", *, min_tape_area=500, min_tape_width=20, min_burr_area=100, want_table=True,
                   max_components=8192, check=True, return_tape_table=False):
    """predict_simple_np on the device for float32 CUDA probs [B,7,h,w] (predict_proba's output): the merged map uint8
    [B,fh,fw] and, with want_table, its class table int32 [B,256,5], both on the device.  The planes are resized inside the
    threshold launch; every closing, opening and dilation runs in the LDS bit planes of unetpp_merge_classes; the last launch
    writes the merged map and its table.  Nothing is read back between probs and the map: the tape filter's decision stays in
    its device table.  check=True ends with one read-back of the labellings' num (synchronises) and raises RuntimeError for a
    frame with more than max_components labels; with check=False such a frame loses the filtered class."""
    out, table, tape_table, num, k = _predict_simple(model, probs, frame_hw, variant, min_tape_area, min_tape_width, min_burr_area, want_table,
                                                     max_components)
    if check:
        model._raise_num_overflow(num, k)
    res = (out,) + ((table,) if want_table else ()) + ((tape_table,) if return_tape_table else ())
    return res if len(res) > 1 else res[0]


def predict_simple_backup(model, pred, want_table=True):
    """predict_simple_backup_np on the device for a uint8 CUDA class map [B,H,W] at frame size: two launches of
    unetpp_merge_classes, the second on the first's map (so the tape plane is cut after the cable's closing was written); the
    second writes the table."""
    pred = model._input(pred, "pred")
    first = mc.merge_classes(model, pred, PLANES_BACKUP[0], want_table=False)
    return mc.merge_classes(model, first, PLANES_BACKUP[1], want_table=want_table)
