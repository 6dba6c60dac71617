"""The per-frame decisions of the reference's ROI loop (infer_video_roi.py) and of its full-frame 3-class loop
(infer_video_3class_full.py) in NumPy (torch-free) and on the device (include/unetpp_roi.h; csrc/roi_loop.h):
  detect_roi_by_projection after its Canny   :34-57     roi_from_edges (detect_roi: grey conversion -> Canny -> this)
  frame[:, x_min:x_max] -> cv2.resize        :203-209   crop_resize
  adaptive_thresholding                      :60-97     adaptive_thresholds
  ultra_strict_threshold                     :100-125   ultra_strict
  refine_mask_by_geometry                    :128-167   refine_by_geometry
  cv2.resize(INTER_NEAREST) and the paste    :238-247   paste_masks
  select_primary_component (3class_full)     :85-114    select_primary
keep_largest_cc (3class_full :69-82) is filter_components(rule="largest", min_area=...): both keep the first component of
the greatest area when that area reaches min_area and nothing otherwise.  measure_diameters_simple (:119-134) is
calc_width of _measure_diameters, robust.row_width_median_np.  The whole loops are frame_loop.process_frames_roi and
frame_loop.process_frames_3class_full.

Two tables carry a frame's decisions between the device calls, so that nothing is read back: roi int32 [B,4] =
(x_min, x_max, found, valid) with valid = x_max > x_min, and thresholds float32 [B,3] = (t_cable, t_tape, bg_margin).
The reference's cv2.resize raises on an empty crop; here such a frame gets zero masks and valid = 0 reports it.

Every device function equals its `_np` form bit for bit.  Two of the forms restate the reference with other arithmetic:
  * the projection compares integers, 10 S_i > 3 S_max, where the reference compares float64 sums 255 / 30 times as large;
    they agree unless a column has 10 S_i == 3 S_max exactly (roi_condition_np), which the fixtures exclude;
  * the means are sums of floor(p * 2^32) in 64 bits, order-independent, where the reference's float32 .mean() of a strided
    view is a pairwise sum; the distance, a few float32 ulps, is measured by scripts/make_golden_roi.py.
cv2 is not installed where this project is built and tested: its resizes and its label order stay unpinned.

The functions take the model, as multiclass.py and robust.py do.
"""
from __future__ import annotations

import numpy as np

from . import components as cc
from . import edges as ed
from . import robust as rb
from . import tiling as tl

BOX = 30                                             # the reference's smoothing window
ROI_FIELDS = ("x_min", "x_max", "found", "valid")
GEOMETRY_DEFAULTS = dict(min_area=2000, min_aspect=2.0, wide_width=100, edge_lo=0.1, edge_hi=0.9, large_area=10000)
PRIMARY_DEFAULTS = dict(min_area=1000, min_aspect=1.6)


def _plane(mask, what="mask"):
    m = np.asarray(mask)
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"{what} must be [H,W], got {list(m.shape)}")
    return m


# ---- 1. the cable's column range ---------------------------------------------------------------------------------------------
def box_sums_np(counts):
    """np.convolve(counts, np.ones(30), mode='same') in integers: int64 [max(W, 30)], entry i = the sum of counts[k] over
    m - 29 <= k <= m with m = i + (n - 1 - n // 2), n = min(W, 30) (for W >= 30: columns i - 15 .. i + 14)."""
    c = np.asarray(counts, np.int64)
    W = len(c)
    n = min(W, BOX)
    cum = np.concatenate([[0], np.cumsum(c)])
    m = np.arange(max(W, BOX)) + (n - 1 - n // 2)
    lo, hi = np.maximum(m - (BOX - 1), 0), np.minimum(m, W - 1)
    return np.where(hi >= lo, cum[np.maximum(hi + 1, 0)] - cum[np.minimum(lo, W)], 0)


def roi_condition_np(edges):
    """The input condition of roi_from_edges for one frame: no column with 10 S_i == 3 S_max, unless the frame has no edge."""
    s = box_sums_np(np.count_nonzero(_plane(edges, "edges"), axis=0))
    return s.max() == 0 or not bool((10 * s == 3 * s.max()).any())


def roi_from_edges_np(edges):
    """detect_roi_by_projection (:34-57) from its Canny image uint8 [H,W] (non-zero = edge): int32 [4] = (x_min, x_max,
    found, valid).  The reference's arithmetic as written: int(col * (W / 512)), margin = int((x_max - x_min) * 0.1)."""
    e = _plane(edges, "edges")
    W = e.shape[1]
    s = box_sums_np(np.count_nonzero(e, axis=0))
    cols = np.nonzero(10 * s > 3 * s.max())[0]
    if len(cols):
        x_min = int(int(cols[0]) * (W / 512))
        x_max = int(int(cols[-1]) * (W / 512))
        margin = int((x_max - x_min) * 0.1)
        x_min, x_max = max(0, x_min - margin), min(W, x_max + margin)
    else:
        x_min, x_max = int(W * 0.25), int(W * 0.75)
    return np.array([x_min, x_max, 1 if len(cols) else 0, 1 if x_max > x_min else 0], np.int32)


def detect_roi_np(frame_bgr):
    """detect_roi_by_projection for one BGR frame uint8 [H,W,3] (RGB2GRAY of the swapped frame is BGR2GRAY of the frame)."""
    return roi_from_edges_np(ed.canny_np(ed.bgr_to_gray_np(np.asarray(frame_bgr)[None])[0], 50, 150))


def full_roi_np(batch, W):
    """The table of use_roi=False: every frame whole."""
    return np.tile(np.array([0, int(W), 0, 1], np.int32), (int(batch), 1))


# ---- 2. crop and resize ----------------------------------------------------------------------------------------------------------
def crop_resize_np(frame, roi, size=512):
    """cv2.resize(frame[:, x_min:x_max], (size, size)) for one frame uint8 [H,W,C] (tiling.resize_linear_u8_np, the
    oracle's cv2_resize_linear_u8_np); zeros when the range is empty."""
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.ndim != 3:
        raise ValueError("frame must be uint8 [H,W,C]")
    ow, oh = (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[1]), int(size[0]))
    x_min, x_max = int(roi[0]), int(roi[1])
    if not (int(roi[3]) and x_max > x_min):
        return np.zeros((oh, ow, f.shape[2]), np.uint8)
    return tl.resize_linear_u8_np(np.ascontiguousarray(f[:, x_min:x_max]), (ow, oh))


# ---- 3. the thresholds of a frame's own means ----------------------------------------------------------------------------------
def q32_np(p):
    """floor(clamp(p, 0, 1) * 2^32) of float32 values as uint64 (exact in float64; NaN and p <= 0 give 0)."""
    x = np.asarray(p, np.float32).astype(np.float64)
    x = np.where(x > 0, np.minimum(x, 1.0), 0.0)
    return np.floor(x * 4294967296.0).astype(np.uint64)


def plane_stats_np(probs):
    """(means, maxima) float32 [3] of planes 0..2 of float32 [C,H,W]: mean = (float)((double)sum q32 / ((double)n * 2^32)),
    max of max(p, 0)."""
    p = np.asarray(probs)
    if p.dtype != np.float32 or p.ndim != 3 or p.shape[0] < 3:
        raise ValueError("probs must be float32 [C,H,W] with C >= 3")
    n = p.shape[1] * p.shape[2]
    means = np.array([np.float32(float(int(q32_np(p[c]).sum(dtype=np.uint64))) / (float(n) * 4294967296.0)) for c in range(3)], np.float32)
    maxima = np.array([np.where(p[c] > 0, p[c], np.float32(0)).max() for c in range(3)], np.float32)
    return means, maxima


def thresholds_from_means_np(means):
    """adaptive_thresholding's three expressions (:80-94) in float32, as NumPy 2 evaluates them for float32 means:
    (t_cable, t_tape, bg_margin) float32 [3] from (bg_mean, cable_mean, tape_mean)."""
    f = np.float32
    bg, cable, tape = (f(v) for v in means)
    t_cable = (cable + f(0.4) if cable + f(0.4) < f(0.85) else f(0.85)) if cable > f(0.3) else f(0.5)
    t_tape = (tape + f(0.5) if tape + f(0.5) < f(0.85) else f(0.85)) if tape > f(0.15) else f(0.55)
    bm = f(1.0) - bg
    return np.array([t_cable, t_tape, bm if bm > f(0.2) else f(0.2)], np.float32)


def adaptive_thresholds_np(probs):
    """adaptive_thresholding (:60-97) for one frame float32 [C,H,W]: (thresholds, means, maxima), float32 [3] each."""
    means, maxima = plane_stats_np(probs)
    return thresholds_from_means_np(means), means, maxima


# ---- 4. ultra_strict_threshold ------------------------------------------------------------------------------------------------
def ultra_strict_np(probs, thresholds):
    """ultra_strict_threshold (:100-125) for one frame float32 [C,H,W] with thresholds (t_cable, t_tape, bg_margin):
    (mask_cable, mask_tape) uint8 0/1 [H,W]."""
    p = np.asarray(probs)
    if p.dtype != np.float32 or p.ndim != 3 or p.shape[0] < 3:
        raise ValueError("probs must be float32 [C,H,W] with C >= 3")
    t_cable, t_tape, margin = (np.float32(v) for v in thresholds)
    bg, cable, tape = p[0], p[1], p[2]
    winner = np.argmax(p[:3], axis=0)
    with np.errstate(invalid="ignore"):
        floor_ = bg + margin
        mc = (winner == 1) & (cable >= t_cable) & (cable > bg * np.float32(2)) & (cable >= floor_)
        mt = (winner == 2) & (tape >= t_tape) & (tape > bg * np.float32(2)) & (tape >= floor_)
    return mc.astype(np.uint8), mt.astype(np.uint8)


# ---- 5. the component rules ----------------------------------------------------------------------------------------------------
def geometry_keep(stats, sums, W, min_area=2000, min_aspect=2.0, wide_width=100, edge_lo=0.1, edge_hi=0.9, large_area=10000,
                  return_trace=False):
    """keep bool [n] of refine_mask_by_geometry's loop (:140-165) from the tables of components_np; return_trace: also the
    rejection of every label ('area', 'aspect', 'edge' or None)."""
    keep = np.zeros(len(stats), bool)
    why = {}
    for i in range(1, len(stats)):
        area, w, h = int(stats[i, cc.CC_STAT_AREA]), int(stats[i, cc.CC_STAT_WIDTH]), int(stats[i, cc.CC_STAT_HEIGHT])
        cx = int(float(sums[i, 0]) / float(area))
        why[i] = ("area" if area < min_area else "aspect" if w > 0 and h / w < min_aspect and w > wide_width else
                  "edge" if (cx < W * edge_lo or cx > W * edge_hi) and area < large_area else None)
        keep[i] = why[i] is None
    return (keep, why) if return_trace else keep


def refine_by_geometry_np(mask, out_value=1, **params):
    """refine_mask_by_geometry for one frame [H,W]: uint8, out_value on every kept component."""
    m = _plane(mask)
    labels, stats, sums = cc.components_np(m, 8, -1)
    return (geometry_keep(stats, sums, m.shape[1], **params)[labels] * np.uint8(out_value)).astype(np.uint8)


def primary_label(stats, sums, W, min_area=1000, min_aspect=1.6, return_trace=False):
    """The label select_primary_component (:95-110) keeps, or -1: float64 score, the first strictly greatest."""
    best_score, best, scores = -1.0, -1, {}
    for i in range(1, len(stats)):
        area = int(stats[i, cc.CC_STAT_AREA])
        if area < min_area:
            continue
        aspect = float(int(stats[i, cc.CC_STAT_HEIGHT])) / max(1.0, float(int(stats[i, cc.CC_STAT_WIDTH])))
        if aspect < min_aspect:
            continue
        cx = float(sums[i, 0]) / float(area)
        center_dist = abs(cx - (W * 0.5)) / max(1.0, float(W))
        score = area * aspect * (1.0 - center_dist)
        scores[i] = score
        if score > best_score:
            best_score, best = score, i
    return (best, scores) if return_trace else best


def select_primary_np(mask, min_area=1000, min_aspect=1.6, out_value=1):
    """select_primary_component for one frame [H,W]: uint8, out_value on the chosen component."""
    m = _plane(mask)
    labels, stats, sums = cc.components_np(m, 8, -1)
    best = primary_label(stats, sums, m.shape[1], min_area, min_aspect)
    return ((labels == best) & (best > 0)).astype(np.uint8) * np.uint8(out_value)


# ---- 6. paste ------------------------------------------------------------------------------------------------------------------
def paste_mask_np(mask, roi, frame_hw):
    """cv2.resize(mask, (x_max - x_min, H), INTER_NEAREST) in columns [x_min, x_max) of a zero uint8 [H,W] frame
    (robust.resize_nearest_np); all zero when the range is empty."""
    H, W = int(frame_hw[0]), int(frame_hw[1])
    out = np.zeros((H, W), np.uint8)
    x_min, x_max = int(roi[0]), int(roi[1])
    if int(roi[3]) and x_max > x_min:
        out[:, x_min:x_max] = rb.resize_nearest_np(_plane(mask).astype(np.uint8), (x_max - x_min, H))
    return out


# ---- the loops after the network, one frame --------------------------------------------------------------------------------------
def postprocess_roi_np(probs, roi, frame_hw, thresholds=None, **geometry):
    """infer_frame (:225-251) after the network for one frame's probabilities float32 [C,S,S]: (mask_cable, mask_tape uint8
    [H,W], cable_coverage, tape_coverage, thresholds); thresholds: a table to use in place of the frame's own."""
    if thresholds is None:
        thresholds = adaptive_thresholds_np(probs)[0]
    c, t = ultra_strict_np(probs, thresholds)
    c, t = refine_by_geometry_np(c, **geometry), refine_by_geometry_np(t, **geometry)
    if not int(roi[3]):
        c, t = np.zeros_like(c), np.zeros_like(t)
    return (paste_mask_np(c, roi, frame_hw), paste_mask_np(t, roi, frame_hw), int(np.count_nonzero(c)) / c.size, int(np.count_nonzero(t)) / t.size,
            thresholds)


def postprocess_3class_full_np(mask_cable, mask_tape, frame_hw, cc_min_area_cable=1000, cc_min_area_tape=500, cable_min_aspect=1.6,
                               tape_dilate_px=15):
    """infer_frame of infer_video_3class_full.py (:224-253) after thresholded_argmax for one frame: (mask_cable, mask_tape at
    frame size, mask_cable, mask_tape at model size, metrics dict of robust.MEASURE_FIELDS)."""
    from . import morphology as mo
    c = select_primary_np(_plane(mask_cable), cc_min_area_cable, cable_min_aspect)
    t = (_plane(mask_tape, "mask_tape") != 0).astype(np.uint8)
    if c.any() and tape_dilate_px > 0:
        t = (t & mo.dilate_np(c, mo.structuring_element("ellipse", 2 * int(tape_dilate_px) + 1))).astype(np.uint8)
    t = cc.filter_components_np(t, -1, "largest", 8, 1, min_area=cc_min_area_tape)
    H, W = int(frame_hw[0]), int(frame_hw[1])
    return rb.resize_nearest_np(c, (W, H)), rb.resize_nearest_np(t, (W, H)), c, t, rb.measure_diameters_np(c, t)


# ---- scenes (regenerated from seeds by the tests and by scripts/make_golden_roi.py) ---------------------------------------------
def make_projection_frame(H, W, seed, kind="cable"):
    """A BGR frame uint8 [H,W,3] for the projection: 'cable' a textured upright bar on a smooth background, 'flat' a constant
    frame (no edge: the fallback), 'line' one sharp vertical step (a single edge column)."""
    r = np.random.default_rng(seed)
    f = np.full((H, W, 3), 90, np.uint8)
    if kind == "flat":
        return f
    if kind == "line":
        f[:, W // 3:] = 200
        return f
    x0 = int(W * r.uniform(0.3, 0.45))
    x1 = min(W - 1, x0 + max(3, int(W * r.uniform(0.12, 0.25))))
    bar = r.integers(30, 230, (H, x1 - x0, 1), dtype=np.uint8)
    f[:, x0:x1] = np.repeat(np.repeat(bar[::4, ::3], 4, 0)[:H], 3, 1)[:, :x1 - x0]
    return f


def make_probs(H, W, seed, cable=0.02, tape=0.01, bar=1.0, C=3):
    """Probabilities float32 [C,H,W] (planes 0..2 sum to 1): an upright cable bar with a wider taped lower part, both at
    about 0.9 and `bar` times 0.16 W / 0.24 W wide, over a haze of the levels `cable` and `tape` with 30 % noise.  The haze
    moves the planes' means across the branches of adaptive_thresholding; classes above 2 are small noise."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    p1 = cable * r.uniform(0.7, 1.3, (H, W))
    p2 = tape * r.uniform(0.7, 1.3, (H, W))
    in_c = (np.abs(x - W * 0.5) < W * 0.08 * bar) & (y < H * 0.55)
    in_t = (np.abs(x - W * 0.5) < W * 0.12 * bar) & (y >= H * 0.55)
    p1[in_c] = r.uniform(0.86, 0.94, int(in_c.sum()))
    p2[in_c] = 0.02
    p2[in_t] = r.uniform(0.86, 0.94, int(in_t.sum()))
    p1[in_t] = 0.02
    p = np.zeros((C, H, W), np.float64)
    p[1], p[2] = p1, p2
    p[0] = 1.0 - p1 - p2
    if C > 3:
        p[3:] = r.uniform(0, 0.01, (C - 3, H, W))
    return p.astype(np.float32)


def make_component_scene(H=256, W=512, kind="all"):
    """A 0/1 mask uint8 [H,W] that meets every branch of both component rules at the reference's defaults:
      a tall central bar (kept by both), a small blob (area), a wide flat block (aspect and width), a tall bar at the left
      edge below 10000 pixels (edge), a tall bar at the right edge above 10000 pixels (kept by its area); 'ties': two equal
      bars mirrored about the centre column, whose scores are equal."""
    m = np.zeros((H, W), np.uint8)
    if kind == "ties":
        m[10:H - 10, W // 2 - 60:W // 2 - 40] = 1
        m[10:H - 10, W // 2 + 41:W // 2 + 61] = 1                # centroids W/2 - 50.5 and W/2 + 50.5
        return m
    m[5:H - 5, W // 2 - 20:W // 2 + 20] = 1                     # kept
    m[20:50, 150:180] = 1                                        # 900 pixels: area
    m[H - 60:H - 10, 300:300 + 140] = 1                          # 50 x 140: aspect < 2 and w > 100
    m[10:H - 10, 8:8 + 30] = 1                                   # at the left edge, 7080 pixels: edge
    m[2:H - 2, W - 50:W - 5] = 1                                 # at the right edge, 11340 pixels: stays
    m[H // 2:H // 2 + 2, 100:104] = 1                            # speckle
    return m


# ---- the fixtures: tests/golden/roi_scenes.npz (scripts/make_golden_roi.py writes it from the reference's own functions) ----
PROJECTION_SCENES = [("cable_96", "cable", 48, 96, 0), ("cable_512", "cable", 64, 512, 1), ("cable_640", "cable", 64, 640, 2),
                     ("flat_96", "flat", 48, 96, 3), ("line_640", "line", 64, 640, 4), ("cable_20", "cable", 40, 20, 5),
                     ("line_20", "line", 40, 20, 6)]
# (name, S, seed, make_probs' cable, tape, bar): both sides of each branch of adaptive_thresholding, and its two caps
PROB_SCENES = [("low", 192, 0, 0.02, 0.01, 1.0), ("cable_high", 192, 1, 0.4, 0.01, 1.0), ("tape_high", 192, 2, 0.02, 0.2, 1.0),
               ("both_high", 192, 3, 0.4, 0.2, 1.0), ("thin", 192, 4, 0.02, 0.01, 0.5), ("cable_cap", 192, 5, 0.5, 0.01, 1.0),
               ("tape_cap", 192, 6, 0.02, 0.45, 1.0)]
COMPONENT_SCENES = [("all", "all"), ("ties", "ties"), ("empty", "empty")]
LOOP_FRAME = (96, 240)                               # the frame the loop fixtures paste into
LOOP_ROIS = {"low": (60, 171, 1, 1), "cable_high": (0, 240, 0, 1), "tape_high": (100, 131, 1, 1), "both_high": (7, 8, 1, 1),
             "thin": (30, 200, 1, 1), "cable_cap": (120, 120, 1, 0), "tape_cap": (0, 33, 1, 1)}
THRESHOLDED = dict(t_cable=0.45, t_tape=0.50, bg_margin=0.15)


def component_scene(kind):
    return np.zeros((256, 512), np.uint8) if kind == "empty" else make_component_scene(kind=kind)


def sha256(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ulp_distance(a, b):
    """The largest distance of two float32 arrays of one sign in units in the last place."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def thresholded_argmax_np(probs, t_cable=0.45, t_tape=0.50, bg_margin=0.15):
    """thresholded_argmax of infer_video_3class_full.py (:40-66) for one frame float32 [C,H,W]: the input of its
    component steps in the fixtures (on the device it is segment_thresholded)."""
    p = np.asarray(probs)
    winner = np.argmax(p[:3], axis=0)
    f = np.float32
    c = (winner == 1) & (p[1] >= f(t_cable)) & ((p[1] - p[0]) >= f(bg_margin))
    t = (winner == 2) & (p[2] >= f(t_tape)) & ((p[2] - p[0]) >= f(bg_margin))
    return c.astype(np.uint8), t.astype(np.uint8)


def fixture_facts(g):
    """What both the generator and tests/test_roi_loop_host.py assert of the fixture `g` (the loaded .npz as a dict): the
    inputs are the regenerated scenes, the input conditions hold, and every `_np` form returns the reference's result."""
    seen = set()
    for name, kind, H, W, seed in PROJECTION_SCENES:
        frame = make_projection_frame(H, W, seed, kind)
        assert sha256(frame) == str(g[f"{name}_sha"]), name
        edges = ed.canny_np(ed.bgr_to_gray_np(frame[None])[0], 50, 150)
        assert roi_condition_np(edges), f"{name}: a column with 10 S == 3 S_max"
        roi = roi_from_edges_np(edges)
        assert np.array_equal(roi[:2], g[f"{name}_roi"]), (name, roi, g[f"{name}_roi"])
        cols = np.count_nonzero(np.count_nonzero(edges, axis=0))
        seen |= {("found", int(roi[2])), ("valid", int(roi[3])), ("W", W), ("columns", min(cols, 2))}
    assert seen >= {("found", 0), ("found", 1), ("valid", 0), ("valid", 1), ("W", 96), ("W", 512), ("W", 640), ("W", 20), ("columns", 1)}, seen
    sides = set()
    worst = 0
    for name, S, seed, cable, tape, bar in PROB_SCENES:
        probs = make_probs(S, S, seed, cable, tape, bar)
        assert sha256(probs) == str(g[f"{name}_sha"]), name
        thr, means, _ = adaptive_thresholds_np(probs)
        assert abs(float(means[1]) - 0.3) >= 1e-3 and abs(float(means[2]) - 0.15) >= 1e-3 and abs(float(means[0]) - 0.8) >= 1e-3, (name, means)
        assert thr.tobytes() == g[f"{name}_thr_np"].tobytes(), name
        ref = g[f"{name}_thr_ref"]
        worst = max(worst, ulp_distance(thr, ref))
        sides |= {("cable", bool(means[1] > 0.3)), ("tape", bool(means[2] > 0.15)), ("bg", bool(thr[2] > np.float32(0.2))),
                  ("cable_cap", bool(thr[0] == np.float32(0.85))), ("tape_cap", bool(thr[1] == np.float32(0.85)))}
        for table in (thr, ref):                                    # the condition under which the loops are compared with ==
            c, t = ultra_strict_np(probs, table)
            assert np.array_equal(c, np.unpackbits(g[f"{name}_cable"])[:S * S].reshape(S, S)), name
            assert np.array_equal(t, np.unpackbits(g[f"{name}_tape"])[:S * S].reshape(S, S)), name
        H, W = LOOP_FRAME
        fc, ft, cov_c, cov_t, _ = postprocess_roi_np(probs, LOOP_ROIS[name], LOOP_FRAME)
        assert np.array_equal(fc, np.unpackbits(g[f"{name}_full_cable"])[:H * W].reshape(H, W)), name
        assert np.array_equal(ft, np.unpackbits(g[f"{name}_full_tape"])[:H * W].reshape(H, W)), name
        assert [cov_c, cov_t] == g[f"{name}_coverage"].tolist(), name
        c0, t0 = thresholded_argmax_np(probs, **THRESHOLDED)
        assert np.array_equal(c0, np.unpackbits(g[f"{name}_ta_cable"])[:S * S].reshape(S, S)), name
        assert np.array_equal(t0, np.unpackbits(g[f"{name}_ta_tape"])[:S * S].reshape(S, S)), name
        fc, ft, c1, t1, m = postprocess_3class_full_np(c0, t0, LOOP_FRAME)
        assert np.array_equal(fc, np.unpackbits(g[f"{name}_f3_cable"])[:H * W].reshape(H, W)), name
        assert np.array_equal(ft, np.unpackbits(g[f"{name}_f3_tape"])[:H * W].reshape(H, W)), name
        assert [m[k] for k in rb.MEASURE_FIELDS] == g[f"{name}_f3_metrics"].tolist(), (name, m)
    assert sides == {(k, v) for k in ("cable", "tape", "bg", "cable_cap", "tape_cap") for v in (False, True)}, sides
    assert worst <= int(g["threshold_ulps"]), (worst, int(g["threshold_ulps"]))
    reasons = set()
    for name, kind in COMPONENT_SCENES:
        m = component_scene(kind)
        assert sha256(m) == str(g[f"{name}_sha"]), name
        assert np.array_equal(refine_by_geometry_np(m), np.unpackbits(g[f"{name}_geometry"]).reshape(m.shape)), name
        assert np.array_equal(select_primary_np(m), np.unpackbits(g[f"{name}_primary"]).reshape(m.shape)), name
        labels, stats, sums = cc.components_np(m, 8, -1)
        keep, why = geometry_keep(stats, sums, m.shape[1], return_trace=True)
        reasons |= set(why.values())
        large_at_edge = [i for i in why if why[i] is None and int(stats[i, cc.CC_STAT_AREA]) >= 10000]
        reasons |= {"large"} if large_at_edge else set()
        best, scores = primary_label(stats, sums, m.shape[1], return_trace=True)
        if kind == "ties":
            assert len(scores) == 2 and len(set(scores.values())) == 1 and best == 1, scores
    assert reasons == {None, "area", "aspect", "edge", "large"}, reasons
    return {"threshold_ulps": worst}


# ---- the device path (torch imported lazily, as in frame_loop.py) -------------------------------------------------------------
def _roi_table(model, roi, batch):
    return model._input(roi, "roi", f"[{int(batch)},4]", "int32")


def _probs(model, probs):
    import torch
    if isinstance(probs, torch.Tensor) and probs.dim() == 4 and probs.shape[1] < 3:
        raise ValueError(f"probs must have at least 3 classes, got {probs.shape[1]}")
    return model._input(probs, "probs", "[B,C,H,W]", "float32")


def roi_from_edges(model, edges):
    """roi_from_edges_np on the device for uint8 CUDA edge images [B,H,W], as model.canny(gray, 50, 150) returns them:
    int32 [B,4] on the device.  A memset and two launches on the current stream, nothing read back."""
    import torch
    from . import _lib
    edges = model._input(edges, "edges")
    b, h, w = edges.shape
    ws = model._workspace(("roi_projection", b, w), lambda: _lib.load().unetpp_roi_projection_workspace_bytes(b, w), edges.device,
                          f"roi_from_edges: unsupported shape {tuple(edges.shape)}")
    roi = torch.empty((b, 4), dtype=torch.int32, device=edges.device)
    model._call("unetpp_roi_from_edges_u8", edges, b, h, w, roi, ws, stream_of=edges)
    return roi


def detect_roi(model, frames_bgr):
    """detect_roi_np for uint8 CUDA frames [B,H,W,3] in BGR: grey conversion -> Canny(50, 150) -> roi_from_edges."""
    return roi_from_edges(model, model.canny(model.bgr_to_gray(frames_bgr), 50, 150))


def full_roi(model, frames):
    """full_roi_np on the device for frames [B,H,W,...]."""
    import torch
    return torch.from_numpy(full_roi_np(frames.shape[0], frames.shape[2])).to(frames.device)


def crop_resize(model, frames, roi, size=512):
    """crop_resize_np for every frame of uint8 CUDA frames [B,H,W,C] in one launch: uint8 [B,size,size,C]; the source width
    is read from roi on the device and the coefficients are formed in the kernel."""
    import torch
    frames = model._input(frames, "frames", "[B,H,W,C]")
    b, h, w, c = frames.shape
    roi = _roi_table(model, roi, b)
    oh, ow = (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))
    if oh < 1 or ow < 1:
        raise ValueError(f"size must be positive, got {size!r}")
    out = torch.empty((b, oh, ow, c), dtype=torch.uint8, device=frames.device)
    model._call("unetpp_roi_crop_resize_u8", frames, b, h, w, c, roi, out, oh, ow, stream_of=frames)
    return out


def adaptive_thresholds(model, probs):
    """adaptive_thresholds_np for float32 CUDA probabilities [B,C,H,W] (predict_proba), C >= 3: (thresholds, means, maxima)
    float32 [B,3] on the device.  A memset and two launches."""
    import torch
    from . import _lib
    probs = _probs(model, probs)
    b, c, h, w = probs.shape
    ws = model._workspace(("roi_stats", b), lambda: _lib.load().unetpp_roi_stats_workspace_bytes(b), probs.device,
                          f"adaptive_thresholds: unsupported batch {b}")
    thr, means, maxima = (torch.empty((b, 3), dtype=torch.float32, device=probs.device) for _ in range(3))
    model._call("unetpp_roi_adaptive_thresholds_f32", probs, b, c, h, w, thr, means, maxima, ws, stream_of=probs)
    return thr, means, maxima


def ultra_strict(model, probs, thresholds):
    """ultra_strict_np for float32 CUDA probabilities [B,C,H,W] with the device table thresholds float32 [B,3]:
    (mask_cable, mask_tape) uint8 0/1 [B,H,W], one launch."""
    import torch
    probs = _probs(model, probs)
    b, c, h, w = probs.shape
    thresholds = model._input(thresholds, "thresholds", f"[{b},3]", "float32")
    cable, tape = (torch.empty((b, h, w), dtype=torch.uint8, device=probs.device) for _ in range(2))
    model._call("unetpp_roi_ultra_strict_f32", probs, b, c, h, w, thresholds, cable, tape, stream_of=probs)
    return cable, tape


def _select(model, mask, rule, params, match_class, out_value, max_components, check, return_num=False):
    import ctypes
    import torch
    from . import _lib
    out_value = model._check_out_value(out_value)
    values = [float(params[n]) for n, _ in _lib.RoiCcRule._fields_]
    if any(v != v for v in values):
        raise ValueError(f"the parameters of the {rule} rule must be numbers, got a NaN")
    labels, num, stats, sums, ws, _ = model._components(mask, match_class, 8, max_components, True)
    b, h, w = labels.shape
    k = int(max_components)
    out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
    model._call("unetpp_roi_components_select", labels, num, stats, sums, b, h, w, k, _lib.ROI_RULES[rule], ctypes.byref(_lib.RoiCcRule(*values)),
                out_value, out, ws, stream_of=labels)
    if check:
        model._raise_num_overflow(num, k)
    return (out, num) if return_num else out


def refine_by_geometry(model, mask, min_area=2000, min_aspect=2.0, wide_width=100, edge_lo=0.1, edge_hi=0.9, large_area=10000, *,
                       match_class=-1, out_value=1, max_components=8192, check=True, return_num=False):
    """refine_by_geometry_np on the device for a uint8 CUDA mask [B,H,W].  max_components and check as for
    NestedUNet.filter_components; return_num: also num int32 [B] of the labelling, for a caller that checks it later."""
    params = dict(min_area=min_area, min_aspect=min_aspect, wide_width=wide_width, edge_lo=edge_lo, edge_hi=edge_hi, large_area=large_area)
    return _select(model, mask, "geometry", params, match_class, out_value, max_components, check, return_num)


def select_primary(model, mask, min_area=1000, min_aspect=1.6, *, match_class=-1, out_value=1, max_components=8192, check=True,
                   return_num=False):
    """select_primary_np on the device for a uint8 CUDA mask [B,H,W]; the keywords as for refine_by_geometry."""
    params = dict(GEOMETRY_DEFAULTS, min_area=min_area, min_aspect=min_aspect)
    return _select(model, mask, "primary", params, match_class, out_value, max_components, check, return_num)


def paste_masks(model, masks, roi, frame_hw):
    """paste_mask_np for a pair of uint8 CUDA masks (mask_cable, mask_tape), each [B,h,w], in one launch: two uint8
    [B,H,W] with frame_hw = (H, W); the ROI is read from the device table."""
    import torch
    m0, m1 = rb._mask_pair(model, masks[0], masks[1], "mask", "mask_tape")
    b, h, w = m0.shape
    roi = _roi_table(model, roi, b)
    H, W = int(frame_hw[0]), int(frame_hw[1])
    if H < 1 or W < 1:
        raise ValueError(f"frame_hw must be positive, got {frame_hw!r}")
    out0, out1 = (torch.empty((b, H, W), dtype=torch.uint8, device=m0.device) for _ in range(2))
    model._call("unetpp_roi_paste_masks_u8", m0, m1, b, h, w, roi, out0, out1, H, W, stream_of=m0)
    return out0, out1


# ---- the loops after the network, on the device ------------------------------------------------------------------------------------
def postprocess_roi(model, probs, roi, frame_hw, *, thresholds=None, max_components=8192, **geometry):
    """postprocess_roi_np for float32 CUDA probabilities [B,C,S,S] and the device table roi: (mask_cable, mask_tape uint8
    [B,H,W], counts int32 [B,4] = (cable pixels, tape pixels at model size, num of the cable's and of the tape's labelling),
    thresholds float32 [B,3]), all on the device and nothing read back.  `geometry`: refine_by_geometry's parameters.  A frame
    whose labelling has more than max_components labels comes out zero; its num says so."""
    import torch
    b = probs.shape[0]
    roi = _roi_table(model, roi, b)
    thr = adaptive_thresholds(model, probs)[0] if thresholds is None else thresholds
    cable_s, tape_s = ultra_strict(model, probs, thr)
    cable_s, num_c = refine_by_geometry(model, cable_s, max_components=max_components, check=False, return_num=True, **geometry)
    tape_s, num_t = refine_by_geometry(model, tape_s, max_components=max_components, check=False, return_num=True, **geometry)
    valid = roi[:, 3].to(torch.uint8)[:, None, None]
    cable_s, tape_s = cable_s * valid, tape_s * valid
    cable, tape = paste_masks(model, (cable_s, tape_s), roi, frame_hw)
    counts = torch.stack((model.count_nonzero(cable_s), model.count_nonzero(tape_s), num_c, num_t), dim=1)
    return cable, tape, counts, thr


def postprocess_3class_full(model, mask_cable, mask_tape, frame_hw, *, cc_min_area_cable=1000, cc_min_area_tape=500, cable_min_aspect=1.6,
                            tape_dilate_px=15, max_components=8192):
    """postprocess_3class_full_np for uint8 CUDA masks [B,S,S] as segment_thresholded returns them: (mask_cable, mask_tape at
    frame size, mask_cable, mask_tape at model size, table float64 [B,7] = robust's measure table (dc_px, dt_px, delta_d_px,
    cable pixels, tape pixels) and num of the two labellings), all on the device.  The reference dilates only where the cable
    is not empty: decided per frame on the device."""
    import ctypes
    import torch
    from . import _lib
    from . import morphology as mo
    k = int(max_components)
    cable_s, tape_s = rb._mask_pair(model, mask_cable, mask_tape, "mask", "mask_tape")
    cable_s, num_c = select_primary(model, cable_s, cc_min_area_cable, cable_min_aspect, max_components=k, check=False, return_num=True)
    if tape_dilate_px > 0:
        element = mo.structuring_element("ellipse", 2 * int(tape_dilate_px) + 1)
        near = model.morphology_program(cable_s, -1, [("dilate", 2, 0, 0, 0, 1), ("and", 2, 2, 1)], [element], tape_s, -1, 2, 1)
        some = model.count_nonzero(cable_s) > 0                          # `if mask_cable_small.sum() > 0`
        tape_s = torch.where(some[:, None, None], near, (tape_s != 0).to(torch.uint8))
    # keep_largest_cc: filter_components(rule="largest") with its num kept for the caller's one read-back
    labels, num_t, stats, sums, ws, _ = model._components(tape_s, -1, 8, k, True)
    b, h, w = labels.shape
    tape_s = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
    model._call("unetpp_components_filter", labels, num_t, stats, sums, b, h, w, k, _lib.CC_RULES["largest"],
                ctypes.byref(_lib.CcRule(float(cc_min_area_tape), 0.0, 0.0, 0.0, 0.0, 0.0, float(w))), 1, tape_s, ws, stream_of=labels,
                invalid=RuntimeError)
    H, W = int(frame_hw[0]), int(frame_hw[1])
    cable, tape = model.resize_masks(cable_s, (W, H)), model.resize_masks(tape_s, (W, H))
    table = torch.cat((rb._measure_table(model, cable_s, tape_s), torch.stack((num_c, num_t), dim=1).to(torch.float64)), dim=1)
    return cable, tape, cable_s, tape_s, table
