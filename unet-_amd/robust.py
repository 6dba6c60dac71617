"""The mask rules of the reference's robust 3-class frame loop (infer_video_robust.py) in NumPy (torch-free) and on the
device (include/unetpp.h: unetpp_distance_transform_u8, unetpp_components_best_cable, unetpp_roi_limit_u8,
unetpp_row_width_median; csrc/distance.h):
  letterbox_rgb / unletterbox_mask           :40-61     letterbox_plan, letterbox, unletterbox_masks
  keep_best_cable_cc                         :102-160   keep_best_cable
  restrict_tape_to_cable_ring                :169-198   restrict_tape_to_ring (cv2.distanceTransform: distance_transform)
  apply_roi_limit                            :201-216   roi_limit
  infer_frame steps 7-9 / 10-11              :325-363   postprocess_robust / measure_robust
The network call and exclusive_threshold are NestedUNet.segment_thresholded(rule="exclusive"); the whole loop is
frame_loop.process_frames_robust.  create_overlay / putText and EventGate stay on the host.

The distance transform restates OpenCV's published distanceTransform_3x3: a chamfer distance in 16.16 fixed point with
the weights (HV, DIAG) of METRICS, capped at DIST_CAP = INT_MAX >> 2 and converted as float32(t) * 2^-16 (t rounded to
float32 first; a frame without a zero pixel is 8192.0 everywhere).  distance_fixed_np is its two raster scans,
distance_fixed_closed_np the closed form min over the zero pixels q of DIAG min(|dx|, |dy|) + HV (max - min); both give
the same integers, and the device computes a third exact form (csrc/distance.h).  cv2 is not installed where this project
is built and tested, so cv2's own transform (its IPP path may differ) and its label order stay unpinned.

The functions take the model, as evaluation.py and nlmeans.py do.
"""
from __future__ import annotations

import numpy as np

from . import components as cc
from . import geometry as ge
from . import morphology as mo
from . import tiling as tl

DIST_SHIFT = 16
DIST_CAP = (2 ** 31 - 1) >> 2                   # 536,870,911 = 8192 * 65536 - 1
# cvRound(0.955f * 65536), cvRound(1.3693f * 65536) for DIST_L2 with a 3 x 3 mask; (1, 2) and (1, 1) for DIST_L1, DIST_C
METRICS = {"l2": (62587, 89738), "l1": (65536, 131072), "c": (65536, 65536)}
MAX_PAD = 65535                                 # a pad no frame outgrows: roi_limit then only empties frames without a cable


def _weights(metric):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    return METRICS[metric]


def _plane(mask, what="mask"):
    m = np.asarray(mask)
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"{what} must be [H,W], got {list(m.shape)}")
    return m


# ---- the distance transform ----------------------------------------------------------------------------------------------
def distance_fixed_np(mask, metric="l2"):
    """The integer result t (int64 [H,W]) of distanceTransform_3x3 for a plane whose zero pixels are the targets: its
    forward and backward raster scans, one row at a time.  Within a row the scan tmp[j] = min(v[j], tmp[j-1] + HV) is
    formed as a running minimum of v[j] - HV j (integers: exact); the cap, which OpenCV applies at every pixel, is
    applied per row (adding a weight and taking minima commute with it); OpenCV's `if t0 > HV` in the backward scan only
    skips neighbours that cannot lower t0."""
    hv, diag = _weights(metric)
    nz = _plane(mask) != 0
    H, W = nz.shape
    ramp = hv * np.arange(W, dtype=np.int64)
    tmp = np.empty((H, W), np.int64)
    prev = np.full(W + 2, DIST_CAP, np.int64)                    # the border row and columns hold the cap
    for i in range(H):
        v = np.minimum(np.minimum(prev[:-2] + diag, prev[1:-1] + hv), prev[2:] + diag)
        v[~nz[i]] = 0
        tmp[i] = np.minimum(np.minimum.accumulate(v - ramp) + ramp, DIST_CAP)
        prev[1:-1] = tmp[i]
    prev[:] = DIST_CAP
    for i in range(H - 1, -1, -1):
        v = np.minimum(np.minimum(np.minimum(prev[2:] + diag, prev[1:-1] + hv), prev[:-2] + diag), tmp[i])
        rv = v[::-1]
        tmp[i] = np.minimum((np.minimum.accumulate(rv - ramp) + ramp)[::-1], DIST_CAP)
        prev[1:-1] = tmp[i]
    return tmp


def distance_fixed_literal_np(mask, metric="l2"):
    """distance_fixed_np pixel by pixel, as OpenCV's two loops run (slow: for small planes in tests)."""
    hv, diag = _weights(metric)
    nz = _plane(mask) != 0
    H, W = nz.shape
    t = [[DIST_CAP] * (W + 2) for _ in range(H + 2)]
    for i in range(1, H + 1):
        for j in range(1, W + 1):
            if not nz[i - 1, j - 1]:
                t[i][j] = 0
            else:
                t0 = min(t[i - 1][j - 1] + diag, t[i - 1][j] + hv, t[i - 1][j + 1] + diag, t[i][j - 1] + hv)
                t[i][j] = min(t0, DIST_CAP)
    out = np.empty((H, W), np.int64)
    for i in range(H, 0, -1):
        for j in range(W, 0, -1):
            t0 = t[i][j]
            if t0 > hv:
                t0 = min(t0, t[i + 1][j + 1] + diag, t[i + 1][j] + hv, t[i + 1][j - 1] + diag, t[i][j + 1] + hv)
                t[i][j] = t0
            out[i - 1, j - 1] = min(t0, DIST_CAP)
    return out


def distance_fixed_closed_all_np(mask, metrics=tuple(METRICS)):
    """{metric: t} from the closed form: min over the zero pixels q of DIAG min(|dx|, |dy|) + HV (max - min), capped.  The
    offsets are formed once for all the metrics asked for."""
    weights = {m: _weights(m) for m in metrics}
    nz = _plane(mask) != 0
    H, W = nz.shape
    zy, zx = np.nonzero(~nz)
    out = {m: np.full(H * W, DIST_CAP, np.int64) for m in weights}
    if len(zy):
        it = np.int32 if 131072 * max(H, W) < 2 ** 31 else np.int64     # the largest cost fits
        py, px = np.divmod(np.arange(H * W, dtype=it), it(W))
        zy, zx = zy.astype(it), zx.astype(it)
        step = max(1, (1 << 21) // len(zy))
        for s in range(0, H * W, step):
            dy = np.abs(py[s:s + step, None] - zy[None, :])
            dx = np.abs(px[s:s + step, None] - zx[None, :])
            lo, hi = np.minimum(dx, dy), np.maximum(dx, dy)
            for m, (hv, diag) in weights.items():
                out[m][s:s + step] = np.minimum((it(diag - hv) * lo + it(hv) * hi).min(axis=1), DIST_CAP)
    return {m: t.reshape(H, W) for m, t in out.items()}


def distance_fixed_closed_np(mask, metric="l2"):
    return distance_fixed_closed_all_np(mask, (metric,))[metric]


def fixed_to_float(t):
    """OpenCV's `(float)(t0 * scale)` with scale = 1.f / 65536: t rounded to float32, then scaled (exact)."""
    return np.asarray(t).astype(np.float32) * np.float32(1.0 / (1 << DIST_SHIFT))


def distance_transform_np(mask, metric="l2"):
    """cv2.distanceTransform(mask, DIST_L2 | DIST_L1 | DIST_C, 3) of one plane [H,W] (non-zero: mask != 0): float32 [H,W]."""
    return fixed_to_float(distance_fixed_np(mask, metric))


def distance_transform_closed_np(mask, metric="l2"):
    return fixed_to_float(distance_fixed_closed_np(mask, metric))


def ring_np(src_nonzero, mask1, lo, hi, metric="l2", out_value=1):
    """What unetpp_distance_transform_u8's ring output holds for one frame: out_value where the plane is non-zero, mask1
    (None: no condition) is non-zero and float32(lo) <= distance <= float32(hi)."""
    nz = _plane(src_nonzero) != 0
    d = distance_transform_np(nz, metric)
    with np.errstate(over="ignore"):
        keep = nz & (d >= np.float32(lo)) & (d <= np.float32(hi))
    if mask1 is not None:
        keep &= np.asarray(mask1) != 0
    return (keep * np.uint8(out_value)).astype(np.uint8)


# ---- the three mask rules -------------------------------------------------------------------------------------------------
def best_cable_label(stats, H, W, min_area=2000, min_h_ratio=0.35, min_aspect=3.0, max_w_ratio=0.20, return_trace=False):
    """The label keep_best_cable_cc (:113-149) keeps, from a statistics table [n,5] (row 0 = background), or -1: the four
    rejections in the reference's order, its float64 score, the first strictly greatest.  return_trace: also
    (the rejection of every label: 'area', 'height', 'width', 'aspect' or None; {label: score} of the candidates)."""
    best_i, best_score = -1, -1e9
    why, scores = {}, {}
    min_h, max_w = int(min_h_ratio * H), int(max_w_ratio * W)
    for i in range(1, len(stats)):
        w, h, area = int(stats[i, cc.CC_STAT_WIDTH]), int(stats[i, cc.CC_STAT_HEIGHT]), int(stats[i, cc.CC_STAT_AREA])
        aspect = h / (w + 1e-6)
        why[i] = "area" if area < min_area else "height" if h < min_h else "width" if w > max_w else "aspect" if aspect < min_aspect else None
        if why[i]:
            continue
        score = (h / H) * 3.0 + min(aspect, 12.0) * 0.5 + (area / (H * W)) * 0.5
        scores[i] = score
        if score > best_score:
            best_score, best_i = score, i
    return (best_i, why, scores) if return_trace else best_i


def keep_best_cable_np(mask, min_area=2000, min_h_ratio=0.35, min_aspect=3.0, max_w_ratio=0.20, out_value=1):
    """keep_best_cable_cc for one frame [H,W]: uint8, out_value on the kept component (labels in raster order of first
    pixels: it only matters between equal scores)."""
    m = _plane(mask)
    labels, stats, _ = cc.components_np(m, 8, -1)
    best = best_cable_label(stats, m.shape[0], m.shape[1], min_area, min_h_ratio, min_aspect, max_w_ratio)
    return ((labels == best) & (best > 0)).astype(np.uint8) * np.uint8(out_value)


def roi_limit_np(mask, cable, pad=80):
    """apply_roi_limit for one frame: mask inside the cable's bounding box padded by `pad` and clipped, 0 outside; all 0
    for an empty cable."""
    m, c = _plane(mask), _plane(cable, "cable")
    out = np.zeros_like(m)
    ys, xs = np.nonzero(c)
    if len(ys):
        H, W = m.shape
        y1, y2 = max(0, int(ys.min()) - pad), min(H - 1, int(ys.max()) + pad)
        x1, x2 = max(0, int(xs.min()) - pad), min(W - 1, int(xs.max()) + pad)
        out[y1:y2 + 1, x1:x2 + 1] = m[y1:y2 + 1, x1:x2 + 1]
    return out


def restrict_tape_to_ring_np(mask_tape, mask_cable, band_out=26, band_in=2, min_area=500, roi_pad=None):
    """restrict_tape_to_cable_ring for one frame: uint8 0/1.  Tape where band_in <= distance to the cable <= band_out and
    the cable is 0; components of at least min_area; close with ELLIPSE (3, 3); all 0 for an empty cable.  roi_pad: also
    apply_roi_limit(result, mask_cable, roi_pad), step 9 of infer_frame."""
    tape, cable = _plane(mask_tape, "mask_tape"), _plane(mask_cable, "mask_cable")
    ring = ring_np(cable == 0, tape, band_in, band_out)
    labels, stats, _ = cc.components_np(ring, 8, -1)
    keep = stats[:, cc.CC_STAT_AREA] >= min_area
    keep[0] = False
    e3 = mo.structuring_element("ellipse", 3)
    out = mo.erode_np(mo.dilate_np(keep[labels], e3), e3).astype(np.uint8)
    return roi_limit_np(out, cable, MAX_PAD if roi_pad is None else roi_pad)


def postprocess_robust_np(mask_cable, mask_tape, close_ksize=5, min_area=2000, min_h_ratio=0.35, min_aspect=3.0, max_w_ratio=0.20,
                          band_out=20, band_in=2, tape_min_area=500, pad=80):
    """Steps 7-9 of infer_frame for one frame: (cable, tape) uint8 0/1."""
    e = mo.structuring_element("ellipse", close_ksize)
    closed = mo.erode_np(mo.dilate_np(_plane(mask_cable) != 0, e), e).astype(np.uint8)
    cable = keep_best_cable_np(closed, min_area, min_h_ratio, min_aspect, max_w_ratio)
    tape = restrict_tape_to_ring_np(mask_tape, cable, band_out, band_in, tape_min_area, roi_pad=pad)
    return roi_limit_np(cable, cable, pad), tape


def row_width_median_np(mask):
    """calc_width of _measure_diameters: np.median of xs.max() - xs.min() + 1 over the rows with more than one non-zero
    pixel, as float64; 0.0 when no row qualifies."""
    widths, _ = ge.row_widths_np(_plane(mask))
    w = widths[0][widths[0] > 1].astype(np.int64)
    return float(np.median(w)) if len(w) else 0.0


def measure_diameters_np(mask_cable, mask_tape):
    """Steps 10-11 of infer_frame for one frame: dict of dc_px, dt_px, delta_d_px, cable_coverage, tape_coverage (float64;
    the coverages count the non-zero pixels, which is mask.sum() for the reference's 0/1 masks)."""
    c, t = _plane(mask_cable), _plane(mask_tape)
    dc, dt = row_width_median_np(c), row_width_median_np(t)
    return {"dc_px": dc, "dt_px": dt, "delta_d_px": dt - dc if dc > 0 else 0.0,
            "cable_coverage": int(np.count_nonzero(c)) / c.size, "tape_coverage": int(np.count_nonzero(t)) / t.size}


MEASURE_FIELDS = ("dc_px", "dt_px", "delta_d_px", "cable_coverage", "tape_coverage")


# ---- letterbox -------------------------------------------------------------------------------------------------------------
def letterbox_plan(h, w, new_size=512):
    """The `meta` of letterbox_rgb (:43-52) with its Python arithmetic: (scale, top, left, nh, nw, h, w)."""
    h, w, new_size = int(h), int(w), int(new_size)
    if h < 1 or w < 1 or new_size < 1:
        raise ValueError(f"letterbox_plan: bad sizes {h}x{w} -> {new_size}")
    scale = new_size / max(h, w)
    nh, nw = int(h * scale), int(w * scale)
    if nh < 1 or nw < 1:
        raise ValueError(f"letterbox_plan: a {h}x{w} frame leaves no pixel at size {new_size}")
    return (scale, (new_size - nh) // 2, (new_size - nw) // 2, nh, nw, h, w)


def resize_nearest_np(img, dsize):
    """cv2.resize(img, (w, h), interpolation=INTER_NEAREST) restated (unetpp_resize_nearest_roi_u8's table): source index
    min(floor(d * (1 / (n_dst / n_src))), n_src - 1) in double."""
    x = np.asarray(img)
    idx = [np.minimum(np.floor(np.arange(n, dtype=np.float64) * (np.float64(1.0) / (np.float64(n) / np.float64(s)))).astype(np.int64), s - 1)
           for n, s in ((int(dsize[1]), x.shape[0]), (int(dsize[0]), x.shape[1]))]
    return x[idx[0]][:, idx[1]]


def letterbox_np(frame, new_size=512):
    """letterbox_rgb without the channel swap (the engine swaps): (canvas uint8 [new_size,new_size,C], plan)."""
    f = np.asarray(frame)
    plan = letterbox_plan(f.shape[0], f.shape[1], new_size)
    _, top, left, nh, nw, _, _ = plan
    canvas = np.zeros((new_size, new_size) + f.shape[2:], np.uint8)
    canvas[top:top + nh, left:left + nw] = tl.resize_linear_u8_np(f, (nw, nh))
    return canvas, plan


def unletterbox_mask_np(mask, plan):
    """unletterbox_mask (:56-61) for one mask at the letterbox size."""
    _, top, left, nh, nw, h, w = plan
    return resize_nearest_np(np.asarray(mask)[top:top + nh, left:left + nw].astype(np.uint8), (w, h))


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def make_robust_scene(H, W, seed, noise=0.02, cable=True, wide=False, squat=False, second=None, overlap=0, **wrap):
    """(mask_cable, mask_tape) uint8 0/1 [H,W] as exclusive_threshold hands them to steps 7-9, from
    geometry.make_wrap_scene(H, W, seed, noise, cable=cable, **wrap): the cable from row 0 (it touches the frame's edge)
    with the tape's flanks beside it, a short cable blob, a tape blob and speckle of both classes.  Options, all of the
    cable class, for the four rejections of keep_best_cable_cc:
      wide     a tall block 0.22 W wide at the left edge          squat    a block 0.37 H x 0.18 W at the right edge
      second   (height, width) as fractions of H, W: a second upright bar at 0.78 W
      overlap  so many rows of tape laid over the cable below the tape's start (the masks then overlap)"""
    m = ge.make_wrap_scene(H, W, seed, noise=noise, cable=cable, **wrap)
    c, t = (m == 1).astype(np.uint8), (m == 2).astype(np.uint8)
    if wide:
        c[0:H // 2, 1:1 + max(int(0.22 * W), 2)] = 1
    if squat:
        x0 = W - 1 - max(int(0.18 * W), 2)
        c[H // 2:H // 2 + max(int(0.37 * H), 2), x0:W - 1] = 1
    if second is not None:
        x0 = int(0.78 * W)
        c[1:1 + max(int(second[0] * H), 2), x0:x0 + max(int(second[1] * W), 1)] = 1
    t[c != 0] = 0                                                # exclusive, as exclusive_threshold leaves them
    if overlap:
        rows = np.nonzero(t.any(axis=1))[0]
        if len(rows):
            y0 = int(rows[len(rows) // 3])
            t[y0:y0 + int(overlap)] |= c[y0:y0 + int(overlap)]
    return c, t


# ---- the device path (torch imported lazily, as in frame_loop.py) ---------------------------------------------------------
def _mask_pair(model, a, b, na, nb):
    a, b = model._input(a, na), model._input(b, nb)
    if a.shape != b.shape:
        raise RuntimeError(f"{nb} {tuple(b.shape)} does not match {na} {tuple(a.shape)}")
    return a, b


def _distance(model, src, match_class, invert, metric, want_dist, mask1, match1, lo, hi, out_value):
    import torch
    from . import _lib
    if metric not in _lib.DIST_METRICS:
        raise ValueError(f"metric must be one of {sorted(_lib.DIST_METRICS)}, got {metric!r}")
    b, h, w = src.shape
    ws = model._workspace(("distance", b, h, w), lambda: _lib.load().unetpp_distance_workspace_bytes(b, h, w), src.device,
                          f"distance_transform: unsupported shape {tuple(src.shape)}")
    dist = torch.empty((b, h, w), dtype=torch.float32, device=src.device) if want_dist else None
    ring = torch.empty((b, h, w), dtype=torch.uint8, device=src.device) if out_value else None
    model._call("unetpp_distance_transform_u8", src, int(match_class), 1 if invert else 0, b, h, w, _lib.DIST_METRICS[metric], dist, mask1,
                int(match1), float(lo), float(hi), int(out_value), ring, ws, stream_of=src)
    return dist, ring


def distance_transform(model, mask, match_class=-1, invert=False, metric="l2"):
    """distance_transform_np on the device for a uint8 CUDA mask [B,H,W] (any H, W, any alignment): float32 [B,H,W], bit for
    bit.  A pixel is non-zero where mask == match_class (match_class < 0: mask != 0), with invert=True where it is not,
    so distance_transform(model, cable, invert=True) is cv2.distanceTransform((cable == 0).astype(np.uint8), DIST_L2, 3).
    metric: 'l2', 'l1' or 'c'.  Three launches on the current stream, nothing read back."""
    mask = model._input(mask, "mask")
    return _distance(model, mask, match_class, invert, metric, True, None, -1, 0.0, 0.0, 0)[0]


def distance_ring(model, mask, mask1=None, lo=2, hi=26, match_class=-1, invert=True, match1=-1, metric="l2", out_value=1, return_distance=False):
    """ring_np on the device: uint8 [B,H,W] = out_value where the plane of distance_transform is non-zero, mask1 (None: no
    condition) is foreground and float32(lo) <= distance <= float32(hi); the distance map is neither written nor read
    unless return_distance=True (then (ring, distance))."""
    out_value = model._check_out_value(out_value)
    if mask1 is None:
        mask = model._input(mask, "mask")
    else:
        mask, mask1 = _mask_pair(model, mask, mask1, "mask", "mask1")
    dist, ring = _distance(model, mask, match_class, invert, metric, return_distance, mask1, match1, lo, hi, out_value)
    return (ring, dist) if return_distance else ring


def keep_best_cable(model, mask, min_area=2000, min_h_ratio=0.35, min_aspect=3.0, max_w_ratio=0.20, *, match_class=-1, out_value=1,
                    max_components=8192, check=True):
    """keep_best_cable_np on the device for a uint8 CUDA mask [B,H,W].  max_components and check as for
    NestedUNet.filter_components: a frame with more components raises RuntimeError (check=True, one B-int read-back) or
    comes out all zero."""
    import torch
    out_value = model._check_out_value(out_value)
    if any(v != v for v in (float(min_area), float(min_h_ratio), float(min_aspect), float(max_w_ratio))):
        raise ValueError("min_area, min_h_ratio, min_aspect and max_w_ratio must be numbers, got a NaN")
    labels, num, stats, _, ws, _ = model._components(mask, match_class, 8, max_components, True)
    b, h, w = labels.shape
    k = int(max_components)
    out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
    model._call("unetpp_components_best_cable", labels, num, stats, b, h, w, k, float(min_area), int(min_h_ratio * h), int(max_w_ratio * w),
                float(min_aspect), out_value, out, ws, stream_of=labels)
    if check:
        model._raise_num_overflow(num, k)
    return out


def roi_limit(model, mask, cable, pad=80):
    """roi_limit_np on the device for uint8 CUDA masks [B,H,W]; the box never leaves the device."""
    import torch
    from . import _lib
    mask, cable = _mask_pair(model, mask, cable, "mask", "cable")
    if int(pad) < 0:
        raise ValueError(f"pad must not be negative, got {pad!r}")
    b, h, w = mask.shape
    ws = model._workspace(("roi", b), lambda: _lib.load().unetpp_roi_limit_workspace_bytes(b), mask.device, f"roi_limit: unsupported batch {b}")
    out = torch.empty_like(mask)
    model._call("unetpp_roi_limit_u8", mask, cable, b, h, w, min(int(pad), MAX_PAD), out, ws, stream_of=mask)
    return out


def restrict_tape_to_ring(model, mask_tape, mask_cable, band_out=26, band_in=2, min_area=500, *, roi_pad=None, max_components=8192, check=True):
    """restrict_tape_to_ring_np on the device, uint8 0/1 [B,H,W]: the fused ring launch, the component area filter
    (filter_components_box with min_area and no upper bounds), close with ELLIPSE (3, 3) (one morphology launch) and
    unetpp_roi_limit_u8, which empties the frames whose cable is empty (the reference's early return) and, with roi_pad,
    is step 9 of infer_frame as well."""
    tape, cable = _mask_pair(model, mask_tape, mask_cable, "mask", "mask_cable")
    ring = distance_ring(model, cable, tape, band_in, band_out)
    kept = model.filter_components_box(ring, -1, min_area, float("inf"), float("inf"), -1, max_components=max_components, check=check)
    closed = model.morphology(kept, -1, "close", 3, "ellipse")
    return roi_limit(model, closed, cable, MAX_PAD if roi_pad is None else roi_pad)


def postprocess_robust(model, mask_cable, mask_tape, *, close_ksize=5, min_area=2000, min_h_ratio=0.35, min_aspect=3.0, max_w_ratio=0.20,
                       band_out=20, band_in=2, tape_min_area=500, pad=80, max_components=8192, check=True):
    """Steps 7-9 of infer_frame (:325-348) with its call-site constants, for uint8 CUDA masks [B,H,W]: (cable, tape) uint8
    0/1, nothing read back but the two overflow checks.  The cable's own ROI cut (:347) changes nothing -- the box of a
    mask holds the mask -- and is not launched."""
    cable, tape = _mask_pair(model, mask_cable, mask_tape, "mask", "mask_tape")
    closed = model.morphology(cable, -1, "close", close_ksize, "ellipse")
    best = keep_best_cable(model, closed, min_area, min_h_ratio, min_aspect, max_w_ratio, max_components=max_components, check=check)
    ring = restrict_tape_to_ring(model, tape, best, band_out, band_in, tape_min_area, roi_pad=pad, max_components=max_components, check=check)
    return best, ring


def _measure_table(model, mask_cable, mask_tape):
    """float64 [B,5] on the device: dc_px, dt_px, delta_d_px, then the non-zero pixels of the cable and of the tape (integers
    far below 2^53: exact)."""
    import torch
    cable, tape = _mask_pair(model, mask_cable, mask_tape, "mask", "mask_tape")
    b, h, w = cable.shape
    widths, area = model.row_widths(cable, -1, tape, -1)
    med = torch.empty((b, 2), dtype=torch.float64, device=cable.device)
    model._call("unetpp_row_width_median", widths, b, h, med, stream_of=cable)
    dc, dt = med[:, 0], med[:, 1]
    delta = torch.where(dc > 0, dt - dc, torch.zeros_like(dc))
    count = area.to(torch.float64)
    return torch.stack([dc, dt, delta, count[:, 0], count[:, 1]], dim=1)


def measure_robust(model, mask_cable, mask_tape):
    """Steps 10-11 of infer_frame (:350-363) for uint8 CUDA masks [B,H,W]: a list of B dicts with dc_px, dt_px, delta_d_px,
    cable_coverage and tape_coverage as Python floats, from ONE read-back per batch (two launches before it)."""
    table = _measure_table(model, mask_cable, mask_tape).cpu().tolist()
    size = mask_cable.shape[1] * mask_cable.shape[2]              # the coverages are divided here: count / size as Python does
    return [dict(zip(MEASURE_FIELDS, row[:3] + [int(row[3]) / size, int(row[4]) / size])) for row in table]


def letterbox(model, frames, new_size=512):
    """letterbox_rgb (:40-53) for uint8 CUDA frames [B,H,W,C] without the channel swap (segment() swaps): resize_frames
    into a zero canvas -> (canvas uint8 [B,new_size,new_size,C], plan)."""
    import torch
    frames = model._input(frames, "frames", "[B,H,W,C]")
    plan = letterbox_plan(frames.shape[1], frames.shape[2], new_size)
    _, top, left, nh, nw, _, _ = plan
    canvas = torch.zeros((frames.shape[0], int(new_size), int(new_size), frames.shape[3]), dtype=torch.uint8, device=frames.device)
    canvas[:, top:top + nh, left:left + nw] = model.resize_frames(frames, (nh, nw))
    return canvas, plan


def unletterbox_masks(model, masks, plan):
    """unletterbox_mask (:56-61) for uint8 CUDA masks [B,S,S]: the plan's slice, then resize_masks to the frame size."""
    masks = model._input(masks, "mask")
    _, top, left, nh, nw, h, w = plan
    if top + nh > masks.shape[1] or left + nw > masks.shape[2]:
        raise ValueError(f"plan {plan} does not fit masks {tuple(masks.shape)}")
    return model.resize_masks(masks[:, top:top + nh, left:left + nw].contiguous(), (w, h))
