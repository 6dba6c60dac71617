"""Segmentation evaluation: the confusion matrix of two class masks and everything the reference derives from it, and the
disagreement of two masks of the same frames, in NumPy (torch-free) and on the device (include/unetpp.h,
unetpp_confusion_u8 and unetpp_mask_disagreement; csrc/evaluation.h).

The reference's compute_metrics (src/utils/metrics.py:9-99) makes 6 C boolean passes over the flattened set and its
compute_confusion_matrix (:102-127) is a Python loop over every pixel; tools/evaluate.py, the validation of every
tools/train_3class_*.py and tools/eval.py's iou_per_class are built on them.  Every number they produce is a function of
one small integer table, counts[t, p] = the pixels with target t and prediction p:
  target count of class c   T = counts[c, :].sum()        pred count   P = counts[:, c].sum()
  intersection              I = counts[c, c]              union        U = T + P - I
metrics_from_confusion restates compute_metrics on Python ints of those sums, with the reference's expressions and its
order of summation, and returns the same floats, not merely close ones (tests/golden/eval_scenes.npz, made by
scripts/make_golden_eval.py from the reference's own functions).  Only the table leaves the device: C C integers per
frame, or one running total per evaluation set.

Pixels outside the table are counted, never dropped silently: outside[:, 0] holds those whose target equals
`ignore_value`, outside[:, 1] the others with target >= C or pred >= C (where the reference's loop raises IndexError);
counts[b].sum() + outside[b].sum() == H W for every frame.

The functions take the model, as frame_loop.measure_frames and nlmeans.py do.
"""
from __future__ import annotations

import ctypes

import numpy as np

MIN_CLASSES, MAX_CLASSES = 2, 16                # the kernel's per-wave histogram holds 16 * 16 + 2 bins


# ---- argument checks shared by the NumPy and the device forms (they look only at .shape and .dtype) -------------------------
def _dtype_name(a):
    return str(a.dtype).rsplit(".", 1)[-1]


def check_args(pred, target, num_classes, ignore_value=None, total=None):
    """(C, ignore) with ignore = -1 for none.  ValueError for C outside 2..16, an ignore value outside 0..255, masks
    that are not uint8 [B,H,W] of one shape, and a `total` that is not int64 [C C + 2]."""
    c = int(num_classes)
    if not MIN_CLASSES <= c <= MAX_CLASSES:
        raise ValueError(f"num_classes must be {MIN_CLASSES}..{MAX_CLASSES}, got {num_classes!r}")
    ign = -1 if ignore_value is None else int(ignore_value)
    if ignore_value is not None and not 0 <= ign <= 255:
        raise ValueError(f"ignore_value must be 0..255 or None, got {ignore_value!r}")
    check_pair(pred, target, "pred", "target")
    if total is not None and (_dtype_name(total) != "int64" or tuple(total.shape) != (c * c + 2,)):
        raise ValueError(f"total must be int64 [{c * c + 2}] (C C counts, ignored, invalid), got {_dtype_name(total)} {list(total.shape)}")
    return c, ign


def check_pair(a, b, na="a", nb="b"):
    for name, m in ((na, a), (nb, b)):
        if _dtype_name(m) != "uint8" or len(m.shape) != 3:
            raise ValueError(f"{name} must be uint8 [B,H,W], got {_dtype_name(m)} {list(m.shape)}")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{na} is {list(a.shape)}, {nb} is {list(b.shape)}: the shapes must be equal")
    if min(a.shape) < 1 or a.shape[0] > 65535 or a.shape[1] * a.shape[2] >= 2 ** 31:
        raise ValueError(f"{na} is {list(a.shape)}: needs 1 <= B <= 65535, H, W >= 1 and H W < 2^31")


# ---- NumPy forms ----------------------------------------------------------------------------------------------------------
def confusion_np(pred, target, num_classes, ignore_value=None, total=None):
    """(counts int64 [B,C,C], outside int64 [B,2]) of uint8 masks [B,H,W] (module docstring), by np.bincount.  total:
    an int64 [C C + 2] array the counts and then the two outside counters of all frames are ADDED to."""
    pred, target = np.asarray(pred), np.asarray(target)
    c, ign = check_args(pred, target, num_classes, ignore_value, total)
    b = pred.shape[0]
    t = target.reshape(b, -1).astype(np.int64)
    p = pred.reshape(b, -1).astype(np.int64)
    key = np.where(t == ign, c * c, np.where((t >= c) | (p >= c), c * c + 1, t * c + p))
    bins = np.stack([np.bincount(k, minlength=c * c + 2) for k in key]).astype(np.int64)
    if total is not None:
        total += bins.sum(0)
    return bins[:, :c * c].reshape(b, c, c), bins[:, c * c:]


def _table(cm):
    cm = np.asarray(cm)
    if cm.ndim == 3:
        cm = cm.sum(0)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or not np.issubdtype(cm.dtype, np.integer):
        raise ValueError(f"cm must be an integer table [C,C] or [B,C,C], got {cm.dtype} {list(cm.shape)}")
    return [[int(v) for v in row] for row in cm]


def metrics_from_confusion(cm, ignore_index=-1):
    """compute_metrics(pred, target, C, ignore_index) (src/utils/metrics.py:9-99) for masks whose confusion table is cm
    ([C,C], or [B,C,C]: summed) -> (mIoU, precision, recall, iou), the last three dicts {class: float} as the reference
    returns them; the same floats.  Background (class 0) stays out of the mean; a class absent from the target has IoU
    and precision 1.0 when nothing was predicted as it and 0.0 otherwise, and recall 1.0; ignore_index skips a CLASS,
    not pixels; with no class left in the mean mIoU is 0.0."""
    rows = _table(cm)
    n = len(rows)
    ious, precision, recall, iou_d = [], {}, {}, {}
    for c in range(n):
        if c == ignore_index:
            continue
        t_n = sum(rows[c])
        p_n = sum(rows[r][c] for r in range(n))
        inter = rows[c][c]
        if t_n == 0:
            iou = 1.0 if p_n == 0 else 0.0
            iou_d[c], precision[c], recall[c] = iou, iou, 1.0
            if c != 0:
                ious.append(iou)
            continue
        iou = inter / float(t_n + p_n - inter)                  # the union is at least t_n > 0
        iou_d[c] = iou
        if c != 0:
            ious.append(iou)
        precision[c] = 0.0 if p_n == 0 else inter / float(p_n)
        recall[c] = inter / float(t_n)
    return (sum(ious) / len(ious) if ious else 0.0), precision, recall, iou_d


def iou_per_class_from_confusion(cm):
    """iou_per_class(pred, target, C) of tools/eval.py:25-34 as float64 [C]: intersection / union, 1.0 for an empty union."""
    rows = _table(cm)
    n = len(rows)
    out = np.zeros((n,))
    for c in range(n):
        inter = rows[c][c]
        union = sum(rows[c]) + sum(rows[r][c] for r in range(n)) - inter
        out[c] = inter / union if union > 0 else 1.0
    return out


def disagreement_np(a, b, logits=None):
    """Where uint8 masks a, b [B,H,W] differ -> dict of [B] arrays: n_diff (int64), first (int64: the smallest linear
    index y W + x of a differing pixel, -1 for none) and, with logits float32 [B,C,H,W], over the differing pixels with
    both values < C: max_margin (float32: max |logits[a] - logits[b]|, 0.0 for none) and n_nan (int64: those whose
    margin is NaN; they stay out of the maximum)."""
    a, b = np.asarray(a), np.asarray(b)
    check_pair(a, b)
    n = a.shape[0]
    diff = (a != b).reshape(n, -1)
    out = {"n_diff": diff.sum(1).astype(np.int64),
           "first": np.where(diff.any(1), diff.argmax(1), -1).astype(np.int64)}
    if logits is not None:
        lg = np.asarray(logits)
        if lg.dtype != np.float32 or lg.ndim != 4 or (lg.shape[0],) + lg.shape[2:] != a.shape or not 1 <= lg.shape[1] <= 256:
            raise ValueError(f"logits must be float32 [B,C,H,W] for masks {list(a.shape)}, got {lg.dtype} {list(lg.shape)}")
        c = lg.shape[1]
        lg = lg.reshape(n, c, -1)
        af, bf = a.reshape(n, -1), b.reshape(n, -1)
        mx, nn = np.zeros((n,), np.float32), np.zeros((n,), np.int64)
        for f in range(n):
            idx = np.flatnonzero(diff[f] & (af[f] < c) & (bf[f] < c))
            m = np.abs(lg[f, af[f, idx], idx] - lg[f, bf[f, idx], idx])
            nan = np.isnan(m)
            nn[f] = nan.sum()
            if (~nan).any():
                mx[f] = m[~nan].max()
        out["max_margin"], out["n_nan"] = mx, nn
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def make_eval_scene(H, W, seed, num_classes, flip=0.05, ignore=0.0):
    """A seeded (pred, target) pair of uint8 [H,W] masks for tests and the bench.  The target has piecewise-constant
    regions (the cells of 6..14 random sites; about half the sites are background); the pred is the target with its
    region boundaries moved by one pixel (a pixel whose right or lower neighbour has another label takes that label)
    and a share `flip` of the pixels relabelled at random.  A share `ignore` of the target's pixels is set to 255."""
    c = int(num_classes)
    r = np.random.default_rng(7700 + 131 * int(seed) + c)
    k = int(r.integers(6, 15))
    sy, sx = r.uniform(0, H, k), r.uniform(0, W, k)
    cls = np.where(r.random(k) < 0.5, 0, r.integers(0, c, k))
    cls[:min(k, c)] = np.arange(min(k, c))                      # the first sites cover the classes in turn
    y, x = np.mgrid[0:H, 0:W]
    d = (y[None] - sy[:, None, None]) ** 2 + (x[None] - sx[:, None, None]) ** 2
    target = cls[d.argmin(0)].astype(np.uint8)
    pred = target.copy()
    right = np.zeros((H, W), bool)
    right[:, :-1] = target[:, :-1] != target[:, 1:]
    pred[:, :-1][right[:, :-1]] = target[:, 1:][right[:, :-1]]
    below = np.zeros((H, W), bool)
    below[:-1] = target[:-1] != target[1:]
    pred[:-1][below[:-1]] = target[1:][below[:-1]]
    hit = r.random((H, W)) < flip
    pred[hit] = r.integers(0, c, int(hit.sum())).astype(np.uint8)
    if ignore > 0:
        target[r.random((H, W)) < ignore] = 255
    return pred, target


EVAL_VARIANTS = ("plain", "pred_missing", "target_missing", "both_missing", "background")


def make_eval_batch(B, H, W, seed, num_classes, variant="plain"):
    """(pred, target) uint8 [B,H,W]: make_eval_scene(H, W, seed + i, num_classes) for frame i, then by `variant`:
    pred_missing / target_missing / both_missing relabel the last class as background in the pred, the target or both
    (a class the model never predicts, one the set never shows, one absent altogether); background: all zeros."""
    if variant not in EVAL_VARIANTS:
        raise ValueError(f"variant must be one of {EVAL_VARIANTS}, got {variant!r}")
    pairs = [make_eval_scene(H, W, seed + i, num_classes) for i in range(B)]
    pred, target = np.stack([p for p, _ in pairs]), np.stack([t for _, t in pairs])
    last = num_classes - 1
    if variant in ("pred_missing", "both_missing"):
        pred[pred == last] = 0
    if variant in ("target_missing", "both_missing"):
        target[target == last] = 0
    if variant == "background":
        pred[:], target[:] = 0, 0
    return pred, target


# ---- the device path (torch imported lazily, as in frame_loop.py) ---------------------------------------------------------
def layout():
    """The pixels of a frame one workgroup of either kernel owns (unetpp_evaluation_layout)."""
    from . import _lib
    span = ctypes.c_int(-1)
    if _lib.load().unetpp_evaluation_layout(ctypes.byref(span)) != 0:
        raise RuntimeError("unetpp_evaluation_layout failed")
    return span.value


def _u32(t):
    """An int32 tensor holding uint32 bits -> int64."""
    return t.long() & 0xFFFFFFFF


def confusion(model, pred, target, num_classes=None, ignore_value=None, total=None, check=True):
    """confusion_np on the device for uint8 CUDA masks [B,H,W] (any H, W, any alignment) -> (counts int64 [B,C,C], outside
    int64 [B,2]) on the device; one launch on the current stream.  num_classes=None: model.num_classes.  total: an int64
    [C C + 2] CUDA tensor the caller keeps across calls; the kernel adds this call's counts and outside counters to it.
    check=True reads `outside` back (synchronises) and raises ValueError naming the first frame with a pixel whose
    target or pred is >= C and not ignored, where the reference's compute_confusion_matrix raises IndexError."""
    import torch
    pred, target = model._input(pred, "pred"), model._input(target, "target")
    c, ign = check_args(pred, target, model.num_classes if num_classes is None else num_classes, ignore_value, total)
    if total is not None:
        if not total.is_contiguous():
            raise ValueError("total must be contiguous: the kernel adds to it in place")
        total = model._input(total, "total", "[N]", "int64")
    b, h, w = pred.shape
    raw = torch.empty((b * (c * c + 2),), dtype=torch.int32, device=pred.device)      # uint32 bits: counts, then outside
    model._call("unetpp_confusion_u8", pred, target, b, h, w, c, ign, raw[:b * c * c], raw[b * c * c:], total, stream_of=pred)
    wide = _u32(raw)
    counts, outside = wide[:b * c * c].view(b, c, c), wide[b * c * c:].view(b, 2)
    if check:
        bad = outside[:, 1].nonzero().flatten().cpu().tolist()
        if bad:
            raise ValueError(f"frame {bad[0]}: {int(outside[bad[0], 1])} pixels have a target or pred value >= num_classes {c} "
                             f"(and the target is not ignore_value {ignore_value!r})")
    return counts, outside


def mask_disagreement(model, a, b, logits=None):
    """disagreement_np on the device for uint8 CUDA masks [B,H,W] and optional float32 CUDA logits [B,C,H,W] (the layout
    of segment(return_logits=True) and forward) -> dict of [B] device tensors: n_diff int64, first int32 and, with
    logits, max_margin float32 and n_nan int64.  One launch; the logits are read only where the masks differ."""
    import torch
    a, b = model._input(a, "a"), model._input(b, "b")
    check_pair(a, b)
    n, h, w = a.shape
    c = 0
    if logits is not None:
        logits = model._input(logits, "logits", "[B,C,H,W]", "float32")
        c = logits.shape[1]
        if (logits.shape[0],) + tuple(logits.shape[2:]) != tuple(a.shape) or not 1 <= c <= 256:
            raise ValueError(f"logits are {list(logits.shape)}, the masks {list(a.shape)}: need [B,C,H,W] with 1 <= C <= 256")
    raw = torch.empty((4, n), dtype=torch.int32, device=a.device)
    has = logits is not None
    model._call("unetpp_mask_disagreement", a, b, n, h, w, logits, c, raw[0], raw[1], raw[2] if has else None, raw[3] if has else None,
                stream_of=a)
    wide = _u32(raw)
    out = {"n_diff": wide[0], "first": raw[1]}
    if has:
        out["max_margin"], out["n_nan"] = raw[2].view(torch.float32), wide[3]
    return out


def evaluate_batches(model, batches, num_classes=None, ignore_value=None, per_image=False, output=0):
    """evaluate_model of tools/evaluate.py:22-79 over `batches`, an iterable of (x, target): x anything segment() accepts,
    target a uint8 CUDA tensor [B,H,W].  Per batch segment(x, output=output) and one confusion launch into a running
    total on the device; ONE synchronisation and read-back at the end.  Returns a dict: miou, precision, recall, iou
    (metrics_from_confusion of the whole set's table), confusion_matrix int64 [C,C], ignored and invalid (pixel counts;
    ValueError if invalid > 0); with per_image=True also iou_per_image float64 [N,C] (tools/eval.py's iou_per_class of
    every frame) and mean_iou_per_image float64 [C]."""
    import torch
    c = int(model.num_classes if num_classes is None else num_classes)
    total, frames = None, []
    for x, target in batches:
        mask = model.segment(x, output=output)
        if total is None:
            total = torch.zeros((c * c + 2,), dtype=torch.int64, device=mask.device)
        counts, _ = confusion(model, mask, target, c, ignore_value, total=total, check=False)
        if per_image:
            frames.append(counts.reshape(-1, c * c))
    if total is None:
        raise ValueError("evaluate_batches needs at least one batch")
    got = torch.cat([total] + [f.flatten() for f in frames]).cpu().numpy()               # the one read-back
    cm, ignored, invalid = got[:c * c].reshape(c, c), int(got[c * c]), int(got[c * c + 1])
    if invalid:
        raise ValueError(f"{invalid} pixels have a target or pred value >= num_classes {c} (and the target is not ignore_value {ignore_value!r})")
    miou, precision, recall, iou = metrics_from_confusion(cm)
    out = {"miou": miou, "precision": precision, "recall": recall, "iou": iou, "confusion_matrix": cm.copy(), "ignored": ignored,
           "invalid": invalid}
    if per_image:
        per = got[c * c + 2:].reshape(-1, c, c)
        out["iou_per_image"] = np.stack([iou_per_class_from_confusion(f) for f in per])
        out["mean_iou_per_image"] = out["iou_per_image"].mean(0)
    return out
