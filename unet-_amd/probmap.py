"""The rules the reference applies to a probability map, in NumPy (torch-free) and on the device (include/unetpp.h,
unetpp_prob_levels_f32, unetpp_prob_threshold_hist_f32, unetpp_components_prob_sum_f32, unetpp_components_filter_mean;
csrc/probmap.h).  tools/inference_binary_optimized.py takes the softmax map of its sliding-window predict
(predict_tiled(blend="probs")) through
  A2  apply_hysteresis (:116-136)                    seeds p >= 0.90, low region p >= 0.70, seeds dilated 3 x ELLIPSE (5,5);
                                                     seeds | (low & dilated)                              -> hysteresis
  A3  apply_morphological_and_filtering (:139-176)   open E3, close E3, 8-connected components; a component stays with
                                                     area >= min_area and mean probability >= 0.85        -> filter_by_mean_prob
  A1  scan_thresholds (:179-270)                     per threshold and image (p >= thr) and compute_metrics; the threshold
                                                     of the best mIoU, the best F1, the best precision at recall >= 0.90
                                                                                                          -> scan_thresholds
Here the map never leaves the device, and the scan reads it once: per pixel k = the number of thresholds <= p, and the
confusion table of every threshold is a suffix sum of the histogram of (target, k) (confusion_from_hist).

How the reference compares (NumPy 2.2.6, checked on its own expressions), and the two conversions that follow:
  `prob_map >= 0.90`    a float32 array against a Python float: the comparison is made in float32 against
                        np.float32(0.90).  Hysteresis and the mean rule convert a threshold with f32_nearest.
  `defect_prob >= thr`  thr = round(np.float64, 2) stays np.float64: the comparison is made in float64, and
                        np.float32(0.9) >= np.float64(0.9) is False.  p32 >= t64 is p32 >= f32_ceil(t64), the smallest
                        float32 not below t64: the scan converts float64 thresholds with f32_ceil.  A float32 threshold
                        array is used as it is.

Where the result may differ from the reference: the mean rule, and nothing else.  The reference decides on np.mean of
float32 values: float32 pairwise summation, a relative error of a few 1e-6 at most for n <= 2^22.  The device decides on
the exact mean of the values truncated at 2^-32 (q(p) = floor(clamp(p, 0, 1) 2^32), summed in 64-bit integers, compared
as sum >= thr_q area in integers: the same bits in any order of arrival).  The two can disagree only for a component whose
true mean lies within about 2e-6 of the threshold.  The fixtures (tests/golden/probmap_scenes.npz) therefore hold no
component with |float64 mean - 0.85| < 1e-5 (MEAN_MARGIN): 5 x the bound, which also covers |0.85 - float32(0.85)|.  That
is a condition on the inputs, not a tolerance on outputs: with it every mask is compared with ==.

`prob` is float32 [B,H,W], or [B,H,W,C] with channel= (read in place: predict_tiled's output with channel=1).  The device
functions take the model, as evaluation.py, nlmeans.py and robust.py do.
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction

import numpy as np

from . import components as cc
from . import evaluation as ev
from . import morphology as mo

MAX_THRESHOLDS = 256
MEAN_MARGIN = 1e-5
Q_ONE = 1 << 32


# ---- thresholds -----------------------------------------------------------------------------------------------------------------
def _number(t, what="threshold"):
    v = float(t)
    if v != v:
        raise ValueError(f"{what} must be a number, got {t!r}")
    return v


def f32_nearest(t):
    """np.float32(t): the float32 a float32 array is compared with when the other side is a Python float."""
    _number(t)
    return np.float32(t)


def f32_ceil(t):
    """The smallest float32 not below t (t as float64): p32 >= t in float64 is p32 >= f32_ceil(t)."""
    v = _number(t)
    x = np.float32(v)
    if float(x) < v:
        x = np.nextafter(x, np.float32(np.inf), dtype=np.float32)
    return np.float32(x)


def scan_values(thr_range=(0.50, 0.99, 0.01)):
    """The thresholds scan_thresholds walks: round(t, 2) of np.arange(*thr_range), np.float64 as in the reference."""
    return [round(t, 2) for t in np.arange(thr_range[0], thr_range[1], thr_range[2])]


def check_thresholds(thresholds):
    """float32 [T], strictly ascending, 1 <= T <= 256: a float32 array as it is, anything else through f32_ceil."""
    a = np.asarray(thresholds)
    if a.ndim != 1 or not 1 <= a.size <= MAX_THRESHOLDS:
        raise ValueError(f"thresholds must be a list of 1..{MAX_THRESHOLDS} values, got shape {a.shape}")
    if a.dtype.kind not in "fiu" or np.isnan(a.astype(np.float64)).any():
        raise ValueError(f"thresholds must be numbers, got {a.dtype} {a.tolist()!r}")
    t = a if a.dtype == np.float32 else np.array([f32_ceil(v) for v in a.tolist()], np.float32)
    if (np.diff(t) <= 0).any():
        raise ValueError("thresholds must be strictly ascending numbers (also after the conversion to float32)")
    return np.ascontiguousarray(t)


def thr_q_of(mean_prob_thr):
    """ceil(exact value of np.float32(mean_prob_thr) * 2^32) as a Python int, clamped to 0..2^64 - 1."""
    v = Fraction(float(f32_nearest(mean_prob_thr))) * Q_ONE
    return min(max(math.ceil(v), 0), (1 << 64) - 1)


# ---- argument checks shared by the NumPy and the device forms (they look only at .shape and .dtype) ---------------------------
def check_plane(prob, channel=None):
    """(B, H, W, pixel_stride, channel) of a float32 plane [B,H,W], or [B,H,W,C] with channel=."""
    if ev._dtype_name(prob) != "float32" or len(prob.shape) not in (3, 4):
        raise ValueError(f"prob must be float32 [B,H,W] or [B,H,W,C], got {ev._dtype_name(prob)} {list(prob.shape)}")
    if len(prob.shape) == 3:
        if channel not in (None, 0):
            raise ValueError(f"channel={channel!r} needs prob [B,H,W,C], got {list(prob.shape)}")
        s, c = 1, 0
    else:
        s = int(prob.shape[3])
        if channel is None or not 0 <= int(channel) < s or not 1 <= s <= 256:
            raise ValueError(f"prob is {list(prob.shape)}: channel= must be given, in [0,{s}), and C <= 256; got {channel!r}")
        c = int(channel)
    b, h, w = (int(v) for v in prob.shape[:3])
    if min(b, h, w) < 1 or b > 65535 or h * w >= 2 ** 32:
        raise ValueError(f"prob is {list(prob.shape)}: needs 1 <= B <= 65535, H, W >= 1 and H W < 2^32")
    return b, h, w, s, c


def _same_frames(other, shape, what, dtype):
    if ev._dtype_name(other) != dtype or tuple(other.shape) != tuple(shape):
        raise ValueError(f"{what} must be {dtype} {list(shape)} like prob, got {ev._dtype_name(other)} {list(other.shape)}")


def _plane_np(prob, channel):
    prob = np.asarray(prob)
    b, h, w, s, c = check_plane(prob, channel)
    return prob if s == 1 and prob.ndim == 3 else prob[..., c]


def _levels_thresholds(t_low, t_high):
    lo = f32_nearest(t_low)
    hi = lo if t_high is None else f32_nearest(t_high)
    if lo > hi:
        raise ValueError(f"t_low {t_low!r} is above t_high {t_high!r}")
    return lo, hi


def _check_class(target_class, ignore_value):
    tc = int(target_class)
    if not -1 <= tc <= 255:
        raise ValueError(f"target_class must be 0..255, or -1 for non-zero, got {target_class!r}")
    ign = -1 if ignore_value is None else int(ignore_value)
    if ignore_value is not None and not 0 <= ign <= 255:
        raise ValueError(f"ignore_value must be 0..255 or None, got {ignore_value!r}")
    return tc, ign


def _check_total(total, t):
    if total is not None and (ev._dtype_name(total) != "int64" or tuple(total.shape) != (2 * (t + 1) + 1,)):
        raise ValueError(f"total must be int64 [{2 * (t + 1) + 1}] (2 (T + 1) counts, then the ignored pixels), got "
                         f"{ev._dtype_name(total)} {list(total.shape)}")


def _check_hysteresis(thr_high, thr_low, ksize, iterations):
    lo, hi = f32_nearest(thr_low), f32_nearest(thr_high)
    if lo > hi:
        raise ValueError(f"thr_low {thr_low!r} is above thr_high {thr_high!r}")
    if int(iterations) < 1:
        raise ValueError(f"iterations must be at least 1, got {iterations!r}")
    return lo, hi


# ---- NumPy forms --------------------------------------------------------------------------------------------------------------
def levels_np(prob, t_low, t_high=None, channel=None):
    """uint8 [B,H,W]: 0 for p < t_low, 1 for t_low <= p < t_high, 2 for p >= t_high, compared in float32 against
    f32_nearest of each threshold; NaN gives 0.  t_high=None: t_high = t_low (codes 0 and 2)."""
    p = _plane_np(prob, channel)
    lo, hi = _levels_thresholds(t_low, t_high)
    return ((p >= lo).astype(np.uint8) + (p >= hi).astype(np.uint8)).astype(np.uint8)


def program_hysteresis(ksize=5, iterations=3):
    """apply_hysteresis as a morphology program over plane 0 = seeds, plane 1 = low region: dilate, and, or."""
    el = [mo.structuring_element("ellipse", ksize)]
    return el, [("dilate", 2, 0, 0, 0, int(iterations)), ("and", 2, 2, 1), ("or", 2, 2, 0)], 2


def hysteresis_np(prob, thr_high=0.90, thr_low=0.70, ksize=5, iterations=3, channel=None, out_value=1):
    """apply_hysteresis(prob_map, thr_high, thr_low) (:116-136) per frame: uint8 [B,H,W], out_value where set."""
    _check_hysteresis(thr_high, thr_low, ksize, iterations)
    codes = levels_np(prob, thr_low, thr_high, channel)
    el, steps, res = program_hysteresis(ksize, iterations)
    return mo.run_program_np(codes, codes, el, steps, 2, -1, res, out_value)


def q32_np(p):
    """q(p) = floor(clamp(p, 0, 1) 2^32) as uint64; exact: a float32 times 2^32 is a float64, and so is its floor."""
    p = np.asarray(p, np.float32).astype(np.float64)
    p = np.where(np.isnan(p), 0.0, np.clip(p, 0.0, 1.0))
    return np.floor(p * float(Q_ONE)).astype(np.uint64)


def prob_sums_np(labels, prob, capacity, channel=None):
    """uint64 [B, capacity + 1]: [b, l] = the sum of q(p) over the pixels of frame b with label l, 1 <= l <= capacity; row
    0 (the background) stays 0."""
    p = _plane_np(prob, channel)
    labels = np.asarray(labels)
    _same_frames(labels, p.shape, "labels", "int32")
    k = int(capacity)
    out = np.zeros((p.shape[0], k + 1), np.uint64)
    for b in range(p.shape[0]):
        l = labels[b].ravel().astype(np.int64)
        sel = (l >= 1) & (l <= k)
        np.add.at(out[b], l[sel], q32_np(p[b].ravel()[sel]))
    return out


def means_from_sums(sums, stats):
    """float64 [..., K]: sums / 2^32 / area for the K rows of `stats` (NaN for an empty row): the mean of the truncated
    values, within 2^-32 below the true mean."""
    sums, stats = np.asarray(sums), np.asarray(stats)
    k = stats.shape[-2]
    area = stats[..., cc.CC_STAT_AREA].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums[..., :k].astype(np.float64) / float(Q_ONE) / area


def keep_mean_prob(stats, sums, min_area=50, mean_prob_thr=0.85):
    """bool [n]: label l >= 1 stays with area >= min_area and sum >= thr_q area, in Python integers."""
    tq = thr_q_of(mean_prob_thr)
    keep = np.zeros(len(stats), bool)
    for l in range(1, len(stats)):
        area = int(stats[l, cc.CC_STAT_AREA])
        keep[l] = area >= min_area and int(sums[l]) >= tq * area
    return keep


def filter_mean_prob_np(mask, prob, min_area=50, mean_prob_thr=0.85, kernel_size=3, channel=None, out_value=1):
    """apply_morphological_and_filtering(pred_mask, prob_map, min_area, mean_prob_thr) (:139-176) per frame for a uint8 mask
    [B,H,W] (non-zero = set): open and close with ELLIPSE (k, k), components, the two rules.  uint8 [B,H,W]."""
    p = _plane_np(prob, channel)
    mask = np.asarray(mask)
    _same_frames(mask, p.shape, "mask", "uint8")
    out = np.zeros(p.shape, np.uint8)
    for b in range(p.shape[0]):
        cleaned = mo.cleanup_np(mask[b], -1, kernel_size, 1)
        labels, stats, _ = cc.components_np(cleaned, 8, -1)
        sums = prob_sums_np(labels[None], p[b:b + 1], len(stats))[0]
        out[b] = keep_mean_prob(stats, sums, min_area, mean_prob_thr)[labels] * np.uint8(out_value)
    return out


def postprocess_probmap_np(prob, thr_high=0.90, thr_low=0.70, ksize=5, iterations=3, min_area=50, mean_prob_thr=0.85, kernel_size=3,
                           channel=None, out_value=1):
    """A2 then A3 as main() chains them (:400-408): (pred_hyst, pred_final), uint8 [B,H,W]."""
    hyst = hysteresis_np(prob, thr_high, thr_low, ksize, iterations, channel, out_value)
    return hyst, filter_mean_prob_np(hyst, prob, min_area, mean_prob_thr, kernel_size, channel, out_value)


def threshold_hist_np(prob, target, thresholds, target_class=-1, ignore_value=None, total=None, channel=None, return_outside=False):
    """int64 [B,2,T+1]: [b,g,k] = the pixels of frame b with k thresholds <= p (NaN: 0) whose target (uint8 [B,H,W]) is not
    ignore_value, g = 1 where the target equals target_class (-1: is non-zero).  total: an int64 [2 (T + 1) + 1] array
    the counts and then the ignored pixels of all frames are ADDED to.  return_outside: also int64 [B], the ignored."""
    p = _plane_np(prob, channel)
    target = np.asarray(target)
    _same_frames(target, p.shape, "target", "uint8")
    thr = check_thresholds(thresholds)
    tc, ign = _check_class(target_class, ignore_value)
    t = len(thr)
    _check_total(total, t)
    b = p.shape[0]
    flat = p.reshape(b, -1)
    k = np.where(np.isnan(flat), 0, np.searchsorted(thr, flat, side="right")).astype(np.int64)
    tv = target.reshape(b, -1).astype(np.int64)
    g = (tv != 0) if tc < 0 else (tv == tc)
    key = np.where(tv == ign, 2 * (t + 1), g * (t + 1) + k)
    bins = np.stack([np.bincount(row, minlength=2 * (t + 1) + 1) for row in key]).astype(np.int64)
    if total is not None:
        total += bins.sum(0)
    hist = bins[:, :2 * (t + 1)].reshape(b, 2, t + 1)
    return (hist, bins[:, -1]) if return_outside else hist


def confusion_from_hist(hist):
    """int64 [B,T,2,2] from a histogram [B,2,T+1] (NumPy, or a tensor: read back): [b,j] is evaluation.confusion's
    counts[t, p] with C = 2 for pred = (p >= thresholds[j]), i.e. pred 1 where k > j."""
    if hasattr(hist, "cpu"):
        hist = hist.cpu().numpy()
    hist = np.asarray(hist)
    if hist.ndim != 3 or hist.shape[1] != 2 or hist.shape[2] < 2 or not np.issubdtype(hist.dtype, np.integer):
        raise ValueError(f"hist must be an integer table [B,2,T+1], got {hist.dtype} {list(hist.shape)}")
    hist = hist.astype(np.int64)
    below = np.cumsum(hist, axis=2)[:, :, :-1]                  # [b,g,j] = pixels with k <= j: pred 0
    above = hist.sum(2, keepdims=True) - below
    return np.stack([below, above], axis=-1).transpose(0, 2, 1, 3)


def _scan_pick(values, tables):
    """The tail of scan_thresholds for tables[i] = int64 [T,2,2] of image i: (thr_miou, thr_f1, thr_prec90, results)."""
    results = []
    for j, thr in enumerate(values):
        all_miou, all_precision, all_recall = [], [], []
        for tab in tables:
            miou, prec, rec, _ = ev.metrics_from_confusion(tab[j])
            all_miou.append(miou)
            all_precision.append(prec.get(1, 0.0))
            all_recall.append(rec.get(1, 0.0))
        avg_miou, avg_precision, avg_recall = np.mean(all_miou), np.mean(all_precision), np.mean(all_recall)
        f1 = 2 * avg_precision * avg_recall / (avg_precision + avg_recall + 1e-8)
        results.append({"thr": thr, "miou": avg_miou, "precision": avg_precision, "recall": avg_recall, "f1": f1})
    best_f1 = max(results, key=lambda x: x["f1"])
    valid = [r for r in results if r["recall"] >= 0.90]
    best_prec = max(valid, key=lambda x: x["precision"]) if valid else best_f1
    best_miou = max(results, key=lambda x: x["miou"])
    return best_miou["thr"], best_f1["thr"], best_prec["thr"], results


def _scan_values(thr_range, thresholds):
    """(the values `results` reports, the float32 thresholds the kernel compares with)."""
    values = scan_values(thr_range) if thresholds is None else list(thresholds)
    as_is = isinstance(thresholds, np.ndarray) and thresholds.dtype == np.float32
    return values, check_thresholds(thresholds if as_is else np.asarray(values, np.float64))


def _as_set(items, what):
    """A tensor / array [N,...] or a list of them -> a list of batches."""
    if isinstance(items, (list, tuple)):
        if not items:
            raise ValueError(f"{what} is empty")
        return [x if len(x.shape) >= 3 else x[None] for x in items]
    return [items]


def scan_thresholds_np(probs, targets, thr_range=(0.50, 0.99, 0.01), thresholds=None, channel=None):
    """scan_thresholds (:179-270) over a set: probs and targets are arrays [N,H,W] (targets uint8, non-zero = defect, the
    reference's gt_binary) or lists of them (images of several sizes, [H,W] or [B,H,W] each).  -> (thr_miou, thr_f1,
    thr_prec90, results), results the reference's list of dicts {thr, miou, precision, recall, f1}: per image
    evaluation.metrics_from_confusion, np.mean over the images in their order, f1 with the reference's 1e-8; the first
    maximum wins.  thresholds: the values to scan in place of round(np.arange(*thr_range), 2), ascending."""
    values, thr = _scan_values(thr_range, thresholds)
    tables = []
    for p, t in zip(_as_set(probs, "probs"), _as_set(targets, "targets")):
        tables.extend(confusion_from_hist(threshold_hist_np(p, t, thr, channel=channel)))
    return _scan_pick(values, tables)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
SCENE_KINDS = ("kept", "mean_low", "small", "low_only", "mid", "faint")


def make_prob_scene(H, W, seed, missed=False, specials=12):
    """A seeded (prob float32 [H,W], target uint8 [H,W] 0/1) pair for tests, fixtures and the bench.  Background noise
    below 0.45; one blob per 32 x 32 cell, its kind cycling through SCENE_KINDS from a seeded start:
      kept      a core of radius 7..9 at 0.93..0.98 inside a 2-pixel ring at 0.72..0.80: grows by its ring, mean above 0.85
      mean_low  a core of radius 3..4 at 0.93..0.98 inside a disc of radius 13 at 0.72..0.78: the ring within reach of the
                dilated seeds is kept and the rest dropped; area above 50, mean below 0.85
      small     a disc of radius 3 at 0.94..0.98: mean above 0.85, area below 50
      low_only  a disc of radius 6 at 0.72..0.80 without a seed: hysteresis drops it
      mid       a disc of radius 5 at 0.56..0.67: below the low threshold, seen by the scan alone
      faint     a disc of radius 6 at 0.51..0.58 that the target does not hold: a false positive of the low thresholds
    (the ranges include +-0.01 of noise per pixel); `specials` pixels inside blobs are set to exact threshold values
    (float32 of 0.9, 0.7, 0.85, 0.6, 0.75, 0.95 and their float32 neighbours).  The target is a disc one pixel smaller on
    every blob but low_only and faint, moved by up to a pixel; missed=True adds a large target disc where the map is
    background (recall stays below 0.9)."""
    r = np.random.default_rng(9100 + 17 * int(seed))
    prob = r.uniform(0.02, 0.45, (H, W))
    target = np.zeros((H, W), np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    start = int(r.integers(0, len(SCENE_KINDS)))
    cells = [(cy, cx) for cy in range(H // 32) for cx in range(W // 32)]
    blob = np.zeros((H, W), bool)
    for n, (cy, cx) in enumerate(cells):
        if missed and n == len(cells) - 1:
            target[(y - (cy * 32 + 16)) ** 2 + (x - (cx * 32 + 16)) ** 2 <= 13 ** 2] = 1
            continue
        kind = SCENE_KINDS[(start + n) % len(SCENE_KINDS)]
        py, px = cy * 32 + 16 + int(r.integers(-2, 3)), cx * 32 + 16 + int(r.integers(-2, 3))
        d2 = (y - py) ** 2 + (x - px) ** 2

        def paint(radius, lo, hi):
            sel = d2 <= radius * radius
            prob[sel] = r.uniform(lo, hi) + r.uniform(-0.01, 0.01, int(sel.sum()))
            blob[sel] = True

        if kind == "kept":
            rc = int(r.integers(7, 10))
            paint(rc + 2, 0.73, 0.79)
            paint(rc, 0.94, 0.97)
            outer = rc + 2
        elif kind == "mean_low":
            paint(13, 0.73, 0.77)
            paint(int(r.integers(3, 5)), 0.94, 0.97)
            outer = 13
        elif kind == "small":
            paint(3, 0.95, 0.97)
            outer = 3
        elif kind == "low_only":
            paint(6, 0.73, 0.79)
            outer = 0
        elif kind == "mid":
            paint(5, 0.57, 0.66)
            outer = 5
        else:
            paint(6, 0.52, 0.57)
            outer = 0
        if outer:
            oy, ox = int(r.integers(-1, 2)), int(r.integers(-1, 2))
            target[(y - py - oy) ** 2 + (x - px - ox) ** 2 <= (outer - 1) ** 2] = 1
    prob = prob.astype(np.float32)
    base = [np.float32(v) for v in (0.9, 0.7, 0.85, 0.6, 0.75, 0.95)]
    values = [v for t in base for v in (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)))]
    ys, xs = np.nonzero(blob)
    for n, k in enumerate(r.choice(len(ys), size=min(int(specials), len(ys)), replace=False)):
        prob[ys[k], xs[k]] = values[n % len(values)]
    return prob, target


def mean_rule_table_np(mask2d, prob2d, kernel_size=3):
    """(area int64 [n], float64 mean [n]) of the components the mean rule sees for one frame: the true means, in float64."""
    labels, stats, _ = cc.components_np(mo.cleanup_np(mask2d, -1, kernel_size, 1), 8, -1)
    area = stats[1:, cc.CC_STAT_AREA].astype(np.int64)
    return area, np.array([prob2d[labels == l].astype(np.float64).mean() for l in range(1, len(stats))])


def scene_facts(prob2d, hyst2d, min_area=50, mean_prob_thr=0.85, thr_high=0.90, thr_low=0.70):
    """What a fixture scene must show, for the generator and the host test: (the smallest |mean - threshold| over its
    components, the components rejected by area alone, by mean alone, kept, the low-region pixels hysteresis kept, those
    it dropped)."""
    area, mean = mean_rule_table_np(hyst2d, prob2d)
    low = (prob2d >= f32_nearest(thr_low)) & ~(prob2d >= f32_nearest(thr_high))
    margin = float(np.abs(mean - mean_prob_thr).min()) if len(mean) else 1.0
    big, sure = area >= min_area, mean >= mean_prob_thr
    return (margin, int((~big & sure).sum()), int((big & ~sure).sum()), int((big & sure).sum()),
            int((low & (hyst2d != 0)).sum()), int((low & (hyst2d == 0)).sum()))


# ---- the device path (torch imported lazily, as in evaluation.py) --------------------------------------------------------------
def layout():
    """The pixels of a frame one workgroup of the plane kernels owns (unetpp_probmap_layout)."""
    from . import _lib
    span = ctypes.c_int(-1)
    if _lib.load().unetpp_probmap_layout(ctypes.byref(span)) != 0:
        raise RuntimeError("unetpp_probmap_layout failed")
    return span.value


def _plane(model, prob, channel):
    prob = model._input(prob, "prob", "[B,H,W] or [B,H,W,C]", "float32")
    return (prob,) + check_plane(prob, channel)


def _frames_like(model, t, prob, what, dtype):
    t = model._input(t, what, "[B,H,W]", dtype)
    _same_frames(t, prob.shape[:3], what, dtype)
    return t


def threshold_levels(model, prob, t_low, t_high=None, channel=None):
    """levels_np on the device for a float32 CUDA plane: uint8 [B,H,W] codes 0 / 1 / 2; one launch on the current stream."""
    import torch
    lo, hi = _levels_thresholds(t_low, t_high)
    prob, b, h, w, s, c = _plane(model, prob, channel)
    codes = torch.empty((b, h, w), dtype=torch.uint8, device=prob.device)
    model._call("unetpp_prob_levels_f32", prob, s, c, b, h, w, float(lo), float(hi), codes, stream_of=prob)
    return codes


def hysteresis(model, prob, thr_high=0.90, thr_low=0.70, ksize=5, iterations=3, channel=None, out_value=1):
    """apply_hysteresis (:116-136) on the device: one levels launch, then ONE morphology program over the codes (seeds =
    codes == 2, low region = codes != 0): dilate, and, or.  uint8 [B,H,W], out_value where set.  ValueError for
    thr_low > thr_high."""
    lo, hi = _check_hysteresis(thr_high, thr_low, ksize, iterations)
    out_value = model._check_out_value(out_value)
    program = model._morph_named("hysteresis", (int(ksize), int(iterations)), program_hysteresis)
    codes = threshold_levels(model, prob, lo, hi, channel)
    return model._morph_launch(program, codes, 2, codes, -1, out_value)


def component_prob_sums(model, labels, num, prob, channel=None, max_components=8192):
    """prob_sums_np on the device for labels int32 [B,H,W] and num int32 [B] of model.components(...,
    max_components=max_components): int64 [B, max_components + 1] on the device holding the uint64 sums (below 2^63:
    H W <= 2^30).  `num` is not read here: rows above it are zero.  One launch."""
    import torch
    prob, b, h, w, s, c = _plane(model, prob, channel)
    labels = _frames_like(model, labels, prob, "labels", "int32")
    num = model._input(num, "num", "[B]", "int32")
    k = int(max_components)
    if k < 2:
        raise ValueError(f"max_components must be at least 2 (background + one component), got {max_components!r}")
    sums = torch.empty((b, k + 1), dtype=torch.int64, device=prob.device)
    model._call("unetpp_components_prob_sum_f32", labels, prob, s, c, b, h, w, k, sums, stream_of=prob)
    return sums


def filter_by_mean_prob(model, mask, prob, min_area=50, mean_prob_thr=0.85, kernel_size=3, channel=None, max_components=8192,
                        out_value=1, check=True):
    """apply_morphological_and_filtering (:139-176) on the device for a uint8 CUDA mask [B,H,W] (non-zero = set) and the
    plane it came from: open and close with ELLIPSE (k, k) in one morphology launch, the components, their probability
    sums, the rule area >= min_area and sum >= thr_q area with thr_q = thr_q_of(mean_prob_thr).  uint8 [B,H,W],
    out_value where kept.  max_components and check as for filter_components (check=True: one read-back)."""
    import torch
    out_value = model._check_out_value(out_value)
    tq, area_min = thr_q_of(mean_prob_thr), math.ceil(_number(min_area, "min_area"))
    prob, b, h, w, s, c = _plane(model, prob, channel)
    mask = _frames_like(model, mask, prob, "mask", "uint8")
    k = int(max_components)
    cleaned = model._morph_launch(model._morph_named("cleanup", (int(kernel_size),), mo.program_cleanup), mask, -1, None, -1, 1)
    labels, num, stats, _, ws, _ = model._components(cleaned, -1, 8, k, True)
    sums = component_prob_sums(model, labels, num, prob, channel, k)
    out = torch.empty((b, h, w), dtype=torch.uint8, device=prob.device)
    model._call("unetpp_components_filter_mean", labels, num, stats, sums, b, h, w, k, min(max(area_min, -2 ** 63), 2 ** 63 - 1), tq, out_value,
                out, ws, stream_of=prob, invalid=RuntimeError)
    if check:
        model._raise_num_overflow(num, k)
    return out


def postprocess_probmap(model, prob, thr_high=0.90, thr_low=0.70, ksize=5, iterations=3, min_area=50, mean_prob_thr=0.85, kernel_size=3,
                        channel=None, max_components=8192, out_value=1, check=True):
    """A2 then A3 (main(), :400-408) without the map leaving the device: (pred_hyst, pred_final), uint8 [B,H,W]."""
    hyst = hysteresis(model, prob, thr_high, thr_low, ksize, iterations, channel, out_value)
    return hyst, filter_by_mean_prob(model, hyst, prob, min_area, mean_prob_thr, kernel_size, channel, max_components, out_value, check)


def threshold_histogram(model, prob, target, thresholds, target_class=-1, ignore_value=None, total=None, channel=None, return_outside=False):
    """threshold_hist_np on the device: int64 [B,2,T+1] (and, with return_outside, int64 [B]) on the device; one launch on
    the current stream, the plane read once whatever T is.  total: an int64 [2 (T + 1) + 1] CUDA tensor the caller keeps
    across calls; the kernel adds to it."""
    import torch
    thr = check_thresholds(thresholds)
    tc, ign = _check_class(target_class, ignore_value)
    prob, b, h, w, s, c = _plane(model, prob, channel)
    target = _frames_like(model, target, prob, "target", "uint8")
    t = len(thr)
    _check_total(total, t)
    if total is not None:
        if not total.is_contiguous():
            raise ValueError("total must be contiguous: the kernel adds to it in place")
        total = model._input(total, "total", "[N]", "int64")
    n = b * 2 * (t + 1)
    raw = torch.empty((n + b,), dtype=torch.int32, device=prob.device)                 # uint32 bits: counts, then outside
    model._call("unetpp_prob_threshold_hist_f32", prob, s, c, target, b, h, w, thr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), t, tc, ign,
                raw[:n], raw[n:], total, stream_of=prob)
    wide = ev._u32(raw)
    hist = wide[:n].view(b, 2, t + 1)
    return (hist, wide[n:]) if return_outside else hist


def scan_thresholds(model, probs, targets, thr_range=(0.50, 0.99, 0.01), thresholds=None, channel=None):
    """scan_thresholds_np with the histograms made on the device: probs and targets are CUDA tensors [N,H,W] (or
    [N,H,W,C] with channel=) or lists of them; one launch per tensor, ONE read-back for the whole set."""
    import torch
    values, thr = _scan_values(thr_range, thresholds)
    hists = [threshold_histogram(model, p, t, thr, channel=channel)
             for p, t in zip(_as_set(probs, "probs"), _as_set(targets, "targets"))]
    got = torch.cat([h.reshape(-1, 2, len(thr) + 1) for h in hists]).cpu().numpy()      # the one read-back
    return _scan_pick(values, list(confusion_from_hist(got)))
