"""CPU restatement (NumPy only) of the device's measurement step (include/unetpp.h, unetpp_row_widths,
unetpp_width_profile, unetpp_components_summary) and of the reference functions the NestedUNet methods restate:
  compute_diameter_metrics, compute_thickness_profile, analyze_defects   src/utils/geometry_enhanced.py:113-330
  diameter_profile_from_masks                                            src/utils/geometry.py:28-64
plus the wrap-scene generator the tests and fixtures share.

The one floating-point primitive is cv2.GaussianBlur of a float32 H x 1 image with ksize (1, k), sigmaX = 0 and the
default BORDER_REFLECT_101.  It is restated from OpenCV's published code: the kernel of cv2.getGaussianKernel(k, 0,
CV_32F) (gaussian_taps_f32) and the symmetric column filter, every product and sum rounded to float32, in this order:
  s = t[r] * w[y];  for j = 1 .. r ascending:  s = s + t[r + j] * (w[y + j] + w[y - j])
cv2 is not installed where this project is built and tested, so cv2's own taps and the summation order of its SIMD
paths stay unpinned; every entry point takes `taps=` for cv2's own kernel.
"""
from __future__ import annotations

import numpy as np

from . import components as cc
from . import morphology as mo

MAX_TAPS = 127          # the device kernel's limit (r = 63)
MAX_ROWS = 4096         # rows of a frame unetpp_width_profile takes
# OpenCV's fixed kernels for k = 1, 3, 5, 7 when sigma <= 0 (small_gaussian_tab)
_SMALL_TAPS = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
               7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def odd_kernel_size(kernel_size):
    """The reference's `k if k % 2 == 1 else k + 1`; k <= 1 means no smoothing (1)."""
    k = int(kernel_size)
    if k <= 1:
        return 1
    return k if k % 2 == 1 else k + 1


def gaussian_taps_f32(kernel_size):
    """cv2.getGaussianKernel(k, 0, CV_32F) as float32 [k] (a derived reading, unpinned: see the module docstring).
    sigma = 0.3 ((k - 1) / 2 - 1) + 0.8; t_i = exp(-0.5 / sigma^2 (i - (k - 1) / 2)^2) in double; c_i = float32(t_i);
    S = sum of the c_i in double; tap = float32(c_i * (1 / S)).  k = 3, 5, 7 are OpenCV's fixed tables; an even k
    becomes k + 1 as in the reference; k <= 1 is the identity [1]."""
    k = odd_kernel_size(kernel_size)
    if k in _SMALL_TAPS:
        return np.asarray(_SMALL_TAPS[k], np.float32)
    sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8
    scale2x = -0.5 / (sigma * sigma)
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    c = np.exp(scale2x * x * x).astype(np.float32)
    total = 0.0
    for v in c.tolist():                               # double accumulation over the float32 values, in index order
        total += v
    return (c.astype(np.float64) * (1.0 / total)).astype(np.float32)


def check_taps(taps):
    """float32 [n] C-contiguous, or ValueError for what unetpp_width_profile refuses: an even or empty length, more
    than 127 taps, a value that is not finite, a kernel that is not symmetric (the column filter reads one half)."""
    t = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
    if len(t) < 1 or len(t) % 2 == 0 or len(t) > MAX_TAPS:
        raise ValueError(f"taps must be an odd number of values, 1..{MAX_TAPS}, got {len(t)}")
    if not np.isfinite(t).all():
        raise ValueError("taps must be finite")
    if not np.array_equal(t, t[::-1]):
        raise ValueError("taps must be symmetric")
    return t


def resolve_taps(kernel_size=31, taps=None):
    """The float32 kernel a method smooths with: `taps` when given, else gaussian_taps_f32(kernel_size)."""
    return check_taps(gaussian_taps_f32(kernel_size) if taps is None else taps)


def reflect101(p, n):
    """cv2.borderInterpolate(p, n, BORDER_REFLECT_101) for an int or an int array: 0 for n == 1; otherwise, while p is
    out of range, p = -p below 0 and p = 2 (n - 1) - p from n on."""
    if n < 1:
        raise ValueError(f"n must be positive, got {n!r}")
    q = np.array(p, dtype=np.int64, copy=True)
    if n == 1:
        q[...] = 0
    else:
        while True:
            lo, hi = q < 0, q >= n
            if not (lo.any() or hi.any()):
                break
            q[lo] = -q[lo]
            q[hi] = 2 * (n - 1) - q[hi]
    return int(q) if q.ndim == 0 else q


def smooth_widths_np(w, taps):
    """The column filter of the module docstring along the last axis of a float32 array [..., H]: float32, same shape."""
    t = check_taps(taps)
    w = np.asarray(w, dtype=np.float32)
    H = w.shape[-1]
    r = len(t) // 2
    wp = w[..., reflect101(np.arange(-r, H + r), H)]
    s = t[r] * wp[..., r:r + H]
    for j in range(1, r + 1):
        s = s + t[r + j] * (wp[..., r + j:r + j + H] + wp[..., r - j:r - j + H])
    return s.astype(np.float32, copy=False)


def median_f32(v):
    """np.median of a non-empty float32 vector: the middle element, or (a + b) rounded to float32, then halved."""
    v = np.sort(np.asarray(v, dtype=np.float32).reshape(-1))
    n = len(v)
    if n == 0:
        raise ValueError("median of nothing")
    if n % 2:
        return np.float32(v[n // 2])
    return np.float32(np.float32(v[n // 2 - 1] + v[n // 2]) * np.float32(0.5))


def row_widths_np(mask0, match0=-1, mask1=None, match1=-1):
    """What unetpp_row_widths computes for one frame [H,W] or a batch [B,H,W]: (widths float32 [.,2,H], area uint32
    [.,2]); widths = last - first + 1 over the foreground columns of a row, 0 for an empty row
    (_compute_width_per_row(smooth=False), geometry_enhanced.py:61-67); plane 1 is empty without mask1."""
    mask0 = np.asarray(mask0)
    if mask0.ndim == 3:
        m1 = [None] * len(mask0) if mask1 is None else mask1
        out = [row_widths_np(a, match0, b, match1) for a, b in zip(mask0, m1)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    H, W = mask0.shape
    planes = [cc.foreground(mask0, match0), np.zeros((H, W), bool) if mask1 is None else cc.foreground(mask1, match1)]
    widths = np.zeros((2, H), np.float32)
    area = np.zeros(2, np.uint32)
    cols = np.arange(W)
    for p, fg in enumerate(planes):
        has = fg.any(axis=1)
        first = np.where(fg, cols, W).min(axis=1)
        last = np.where(fg, cols, -1).max(axis=1)
        widths[p] = np.where(has, last - first + 1, 0).astype(np.float32)
        area[p] = fg.sum()
    return widths, area


def width_profile_np(widths, taps, min_valid_rows=20):
    """What unetpp_width_profile computes for raw widths float32 [2,H]: (smoothed float32 [2,H], valid bool [H],
    dc_px, dt_px as float32, valid_rows)."""
    if int(min_valid_rows) < 1:
        raise ValueError(f"min_valid_rows must be at least 1, got {min_valid_rows!r}")
    ws = smooth_widths_np(widths, taps)
    valid = (ws[0] > 0) & (ws[1] > 0)
    n = int(valid.sum())
    if n < int(min_valid_rows):
        return ws, valid, np.float32(0), np.float32(0), n
    return ws, valid, median_f32(ws[0][valid]), median_f32(ws[1][valid]), n


def diameter_metrics_np(pred2d, cable_cls=1, tape_cls=2, mm_per_px=0.05, min_valid_rows=20, kernel_size=31, min_area=50, taps=None):
    """compute_diameter_metrics (geometry_enhanced.py:113-185) for one frame: a dict with DiameterMetrics' fields."""
    t = resolve_taps(kernel_size, taps)
    pred2d = np.asarray(pred2d)
    H, W = pred2d.shape
    cable = cc.filter_components_np(pred2d, cable_cls, "largest", min_area=min_area)
    tape = cc.filter_components_np(pred2d, tape_cls, "largest", min_area=min_area)
    widths, area = row_widths_np(cable, -1, tape, -1)
    _, _, dc, dt, n = width_profile_np(widths, t, min_valid_rows)
    dc_px, dt_px = float(dc), float(dt)
    dc_mm, dt_mm = dc_px * mm_per_px, dt_px * mm_per_px
    return {"dc_px": dc_px, "dt_px": dt_px, "delta_d_px": dt_px - dc_px, "dc_mm": dc_mm, "dt_mm": dt_mm,
            "delta_d_mm": dt_mm - dc_mm, "valid_rows": n, "cable_coverage": int(area[0]) / (H * W),
            "tape_coverage": int(area[1]) / (H * W)}


def thickness_profile_np(pred2d, cable_cls=1, tape_cls=2, mm_per_px=0.05, kernel_size=31, taps=None):
    """compute_thickness_profile (geometry_enhanced.py:188-225) for one frame, no component filter:
    (delta_d_mm float32 [H] = (tape - cable) * float32(mm_per_px), valid_mask bool [H])."""
    t = resolve_taps(kernel_size, taps)
    widths, _ = row_widths_np(pred2d, cable_cls, pred2d, tape_cls)
    ws = smooth_widths_np(widths, t)
    return (ws[1] - ws[0]) * np.float32(mm_per_px), (ws[0] > 0) & (ws[1] > 0)


def diameter_profile_np(pred2d, cable_cls, wrap_cls, kernel_size=31, taps=None):
    """diameter_profile_from_masks (src/utils/geometry.py:28-64) for one frame: the largest component of each class with
    no area floor -> (w_cable_px, w_wrap_px float32 [H], valid uint8 [H])."""
    t = resolve_taps(kernel_size, taps)
    cable = cc.filter_components_np(pred2d, cable_cls, "largest", min_area=0)
    wrap = cc.filter_components_np(pred2d, wrap_cls, "largest", min_area=0)
    widths, _ = row_widths_np(cable, -1, wrap, -1)
    ws = smooth_widths_np(widths, t)
    return ws[0], ws[1], ((ws[0] > 0) & (ws[1] > 0)).astype(np.uint8)


def components_summary_np(num, stats, min_area):
    """What unetpp_components_summary computes for one frame from unetpp_components' num and stats [capacity,5]:
    int64 [4] = (max(0, num - 1), labels 1..min(num, capacity)-1 with area >= min_area, the sum of those areas, the
    largest area of any label)."""
    stats = np.asarray(stats)
    n = min(int(num), len(stats))
    area = stats[1:max(n, 1), cc.CC_STAT_AREA].astype(np.int64)
    ok = area >= int(min_area)
    return np.array([max(0, int(num) - 1), int(ok.sum()), int(area[ok].sum()), int(area.max()) if len(area) else 0], np.int64)


def analyze_defects_np(pred2d, cable_cls=1, tape_cls=2, defect_classes=(3, 4, 5, 6), hole_min_size=10):
    """analyze_defects (geometry_enhanced.py:246-330) for one frame: a dict with DefectAnalysis' fields (defect_areas
    as a list in the order of defect_classes)."""
    pred2d = np.asarray(pred2d)
    H, W = pred2d.shape
    tape_area = int((pred2d == tape_cls).sum())
    num_holes, hole_area, _ = mo.tape_holes_np(pred2d, tape_cls, hole_min_size)
    _, tstats, _ = cc.components_np(pred2d, 8, tape_cls)
    _, cstats, _ = cc.components_np(pred2d, 8, cable_cls)
    tape_n = len(tstats) - 1
    largest = int(tstats[1:, cc.CC_STAT_AREA].max()) / tape_area if tape_n > 0 else 0.0
    areas = [int((pred2d == c).sum()) for c in defect_classes]
    return {"tape_hole_ratio": hole_area / max(tape_area, 1), "tape_num_holes": num_holes, "tape_coverage": tape_area / (H * W),
            "cable_num_components": len(cstats) - 1, "tape_num_components": tape_n, "tape_largest_area_ratio": largest,
            "defect_areas": areas, "total_defect_area": int(sum(areas))}


def make_wrap_scene(H, W, seed, noise=0.02, tape_start=None, cable_end=None, tape_end=None, cable=True, holes=14, classes7=False, sway=0.03):
    """A wrapping frame as compute_diameter_metrics wants it, uint8 [H,W] of classes 0..2 (0..6 with classes7):
      cable   class 1, rows [0, cable_end), half width about 0.08 W varying slowly, centre swaying slowly by `sway` W
      tape    class 2, a sleeve 1.8 times as wide over rows [tape_start, tape_end): two flanks beside the cable where
              the cable runs, the full width below its end, so that the sleeve is one component and the cable another
      distractors  a class-2 blob in rows above the sleeve and a class-1 blob in rows below the cable's end (each with
              area >= 50): they change the widths unless the largest-component filter removes them
      pinholes     `holes` discs of radius 0.8 .. 3.2 px punched out of the tape (areas below and above 10 px)
      speckle      `noise` of the pixels redrawn from classes 0..2
      classes7     one small blob of each class 3..6 beside the cable
    Defaults: tape_start in [0.30 H, 0.45 H), cable_end = H - H // 8, tape_end = H - H // 16.  cable=False leaves out
    the cable and its distractor (the speckle stays)."""
    r = np.random.default_rng(seed)
    y = np.arange(H)[:, None]; x = np.arange(W)[None, :]
    cx = W / 2 + (W * sway) * np.sin(y / H * 6.28 * r.uniform(0.5, 2)) + r.uniform(-W * 0.05, W * 0.05)
    t0 = int(H * r.uniform(0.30, 0.45))
    tape_start = t0 if tape_start is None else int(tape_start)
    cable_end = H - H // 8 if cable_end is None else int(cable_end)
    tape_end = H - H // 16 if tape_end is None else int(tape_end)
    hw_c = W * 0.08 * (1 + 0.08 * np.sin(y / H * 6.28 * 3)); hw_t = hw_c * 1.8
    d = np.abs(x - cx)
    m = np.zeros((H, W), np.uint8)
    m[(d < hw_t) & (y >= tape_start) & (y < tape_end)] = 2
    if cable:
        m[(d < hw_c) & (y < cable_end)] = 1
    bh, bw = max(H // 12, 2), max(W // 10, 2)
    while bh * bw < 50:                                                          # small frames: still 50 px
        bw += 1
    m[max(tape_start - 2 * bh, 0):max(tape_start - 2 * bh, 0) + bh, W - bw - 1:W - 1] = 2     # above the sleeve
    if cable:
        m[cable_end + 1:cable_end + 1 + bh, 1:1 + bw] = 1                        # below the cable's end
    if classes7:
        for k, c in enumerate((3, 4, 5, 6)):
            y0 = (k + 1) * H // 6
            m[y0:y0 + max(H // 40, 2), 2 + bw:2 + bw + max(W // 30, 2) + k] = c
    ys, xs = np.nonzero(m == 2)
    if holes and len(ys):
        for k in r.integers(0, len(ys), holes):
            rad = r.uniform(0.8, 3.2)
            m[(((y - ys[k]) ** 2 + (x - xs[k]) ** 2) <= rad * rad) & (m == 2)] = 0
    if noise > 0:
        n = r.random((H, W)); k = n < noise
        m[k] = r.integers(0, 3, (H, W), dtype=np.uint8)[k]
    return m
