"""CPU restatement (NumPy only) of the device's binary morphology programs (include/unetpp.h, unetpp_morphology),
the program builders the NestedUNet methods launch, and the hole-scene generator the tests and fixtures share.

The contract is OpenCV's published definition of cv2.dilate / cv2.erode / cv2.morphologyEx on a binary mask:
  dilate: dst(x,y) = OR  over (i,j) with elem[i,j] != 0 of src(x + j - ax, y + i - ay)
  erode:  dst(x,y) = AND over the same offsets
with the element NOT reflected (scipy.ndimage reflects it, which shows for an asymmetric element such as ELLIPSE (8,8)),
anchor (ax, ay) = (kw // 2, kh // 2) by default, and pixels outside the image never contributing (0 for a dilate, 1 for
an erode, at every iteration: BORDER_CONSTANT with morphologyDefaultBorderValue).  cv2 is not installed where this
project is built and tested, so cv2's own output stays unpinned, like the resizes: every entry point
takes a caller-supplied `element=` array, so a user with cv2 can pass cv2.getStructuringElement's own kernel.
"""
from __future__ import annotations

import numpy as np

from . import components as cc

OPS = {"dilate": 0, "erode": 1, "and": 2, "andnot": 3, "or": 4, "copy": 5}
SHAPES = ("rect", "cross", "ellipse")
MAX_K = 63              # element side limit of the device kernel
MAX_REACH = 126         # sum of iterations * (k - 1) over a program's dilates and erodes, per axis
MAX_STEPS, MAX_ELEMENTS, PLANES = 8, 4, 4


def structuring_element(shape, ksize):
    """cv2.getStructuringElement(MORPH_RECT / MORPH_CROSS / MORPH_ELLIPSE, (kw, kh)) restated from OpenCV's published
    algorithm (its own output is unpinned here): uint8 [kh,kw].  ksize is (kw, kh) or one int for a square.
    Ellipse: r = kh // 2, c = kw // 2; row i (dy = i - r, |dy| <= r) holds ones in columns
    [max(c - dx, 0), min(c + dx + 1, kw)) with dx = round_half_even(c * sqrt((r^2 - dy^2) / r^2)); (1,1) is rect."""
    if shape not in SHAPES:
        raise ValueError(f"shape must be one of {SHAPES}, got {shape!r}")
    kw, kh = (ksize, ksize) if isinstance(ksize, (int, np.integer)) else (int(ksize[0]), int(ksize[1]))
    kw, kh = int(kw), int(kh)
    if kw < 1 or kh < 1:
        raise ValueError(f"ksize must be positive, got {ksize!r}")
    if shape == "rect" or (kw, kh) == (1, 1):
        return np.ones((kh, kw), np.uint8)
    e = np.zeros((kh, kw), np.uint8)
    r, c = kh // 2, kw // 2
    if shape == "cross":
        e[r, :] = 1
        e[:, c] = 1
        return e
    for i in range(kh):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) / float(r * r)))) if r else 0
            e[i, max(c - dx, 0):min(c + dx + 1, kw)] = 1
    return e


def check_element(element, anchor=None):
    """(uint8 [kh,kw] C-contiguous, (ax, ay)) or ValueError for what the device refuses: a side above 63, an element
    that is empty or not row-convex (the non-zeros of a row must form one run), an anchor outside it."""
    e = np.ascontiguousarray(np.asarray(element) != 0, dtype=np.uint8)
    if e.ndim != 2 or e.shape[0] < 1 or e.shape[1] < 1:
        raise ValueError(f"element must be a non-empty 2-D array, got shape {e.shape}")
    kh, kw = e.shape
    if kw > MAX_K or kh > MAX_K:
        raise ValueError(f"element is {kw}x{kh}: at most {MAX_K}x{MAX_K} is supported")
    if not e.any():
        raise ValueError("element is empty (all zero)")
    for i in range(kh):
        nz = np.nonzero(e[i])[0]
        if len(nz) and nz[-1] - nz[0] + 1 != len(nz):
            raise ValueError(f"element is not row-convex: the non-zeros of row {i} are not one run")
    ax, ay = (kw // 2, kh // 2) if anchor is None else (int(anchor[0]), int(anchor[1]))
    if ax < 0:
        ax = kw // 2
    if ay < 0:
        ay = kh // 2
    if ax >= kw or ay >= kh:
        raise ValueError(f"anchor {anchor!r} outside the {kw}x{kh} element")
    return e, (ax, ay)


def check_program(elements, steps, result_plane):
    """Normalise a program: elements -> [(uint8 array, (ax, ay))], steps -> [(op code, dst, a, b, element, iterations)].
    Raises ValueError for everything unetpp_morphology refuses."""
    elements = [check_element(*(el if isinstance(el, tuple) else (el, None))) for el in elements]
    if len(elements) > MAX_ELEMENTS:
        raise ValueError(f"at most {MAX_ELEMENTS} elements, got {len(elements)}")
    if len(steps) > MAX_STEPS:
        raise ValueError(f"at most {MAX_STEPS} steps, got {len(steps)}")
    written = [True, True, False, False]
    out = []
    reach_v = reach_h = 0
    for s, st in enumerate(steps):
        st = tuple(st)
        op, dst, a = st[0], int(st[1]), int(st[2])
        b = int(st[3]) if len(st) > 3 else 0
        el = int(st[4]) if len(st) > 4 else 0
        it = int(st[5]) if len(st) > 5 else 1
        if isinstance(op, str):
            if op not in OPS:
                raise ValueError(f"step {s}: op must be one of {sorted(OPS)}, got {op!r}")
            op = OPS[op]
        op = int(op)
        if op not in OPS.values():
            raise ValueError(f"step {s}: unknown op {op}")
        binary = op in (OPS["and"], OPS["andnot"], OPS["or"])
        used = [dst, a] + ([b] if binary else [])
        if any(not 0 <= p < PLANES for p in used):
            raise ValueError(f"step {s}: plane index out of range [0,{PLANES})")
        for p in used[1:]:
            if not written[p]:
                raise ValueError(f"step {s} reads scratch plane {p} before any step has written it")
        if op in (OPS["dilate"], OPS["erode"]):
            if not 0 <= el < len(elements):
                raise ValueError(f"step {s}: element index {el} not in [0,{len(elements)})")
            if it < 1:
                raise ValueError(f"step {s}: iterations must be at least 1, got {it}")
            kh, kw = elements[el][0].shape
            reach_v += it * (kh - 1)
            reach_h += it * (kw - 1)
            if reach_v > MAX_REACH or reach_h > MAX_REACH:
                raise ValueError(f"the program's reach (sum of iterations * (k - 1) over its dilates and erodes) exceeds "
                                 f"{MAX_REACH} pixels (vertical {reach_v}, horizontal {reach_h})")
        else:
            el, it = 0, 1
        if not binary:
            b = a
        written[dst] = True
        out.append((op, dst, a, b, el, it))
    if not 0 <= int(result_plane) < PLANES or not written[int(result_plane)]:
        raise ValueError(f"result_plane {result_plane!r} is out of range or never written")
    return elements, out


def _runs(row):
    nz = np.nonzero(row)[0]
    if not len(nz):
        return []
    cut = np.nonzero(np.diff(nz) > 1)[0]
    return list(zip(nz[np.r_[0, cut + 1]].tolist(), nz[np.r_[cut, len(nz) - 1]].tolist()))


def _dilate_once(x, e, ax, ay):
    H, W = x.shape
    kh, kw = e.shape
    pad = kw
    cs = np.zeros((H, W + 2 * pad + 1), np.int32)
    np.cumsum(x, axis=1, dtype=np.int32, out=cs[:, pad + 1:pad + 1 + W])
    cs[:, pad + 1 + W:] = cs[:, pad + W:pad + W + 1]
    out = np.zeros((H, W), bool)
    cols = np.arange(W) + pad
    for i in range(kh):
        dy = i - ay
        y0, y1 = max(0, -dy), min(H, H - dy)            # output rows whose source row y + dy lies inside the image
        if y1 <= y0:
            continue
        for first, last in _runs(e[i]):
            hor = cs[y0 + dy:y1 + dy][:, cols + (last - ax) + 1] > cs[y0 + dy:y1 + dy][:, cols + (first - ax)]
            out[y0:y1] |= hor
    return out


def dilate_np(fg, element, anchor=None, iterations=1):
    """cv2.dilate of a boolean image [H,W] (module docstring): bool [H,W].  Any element, row-convex or not."""
    e = np.asarray(element) != 0
    kh, kw = e.shape
    ax, ay = (kw // 2, kh // 2) if anchor is None else anchor
    x = np.asarray(fg) != 0
    if iterations < 1:
        raise ValueError(f"iterations must be at least 1, got {iterations!r}")
    for _ in range(int(iterations)):
        x = _dilate_once(x, e, ax, ay)
    return x


def erode_np(fg, element, anchor=None, iterations=1):
    """cv2.erode: the AND over the same offsets, i.e. ~dilate(~x) where ~x counts as 0 outside the image."""
    e = np.asarray(element) != 0
    kh, kw = e.shape
    ax, ay = (kw // 2, kh // 2) if anchor is None else anchor
    x = np.asarray(fg) != 0
    if iterations < 1:
        raise ValueError(f"iterations must be at least 1, got {iterations!r}")
    for _ in range(int(iterations)):
        x = ~_dilate_once(~x, e, ax, ay)
    return x


def run_program_np(mask0, mask1, elements, steps, match0=-1, match1=-1, result_plane=2, out_value=1):
    """What unetpp_morphology computes for one frame [H,W] or a batch [B,H,W]: uint8, out_value where the result plane
    is set.  elements: arrays or (array, (ax, ay)) tuples; steps: (op, dst, a, b, element, iterations) with op a name
    from OPS or its code."""
    elements, steps = check_program(elements, steps, result_plane)
    mask0 = np.asarray(mask0)
    if mask0.ndim == 3:
        m1 = [None] * len(mask0) if mask1 is None else mask1
        return np.stack([run_program_np(a, b, elements, steps, match0, match1, result_plane, out_value) for a, b in zip(mask0, m1)])
    planes = [cc.foreground(mask0, match0), np.zeros(mask0.shape, bool) if mask1 is None else cc.foreground(mask1, match1), None, None]
    for op, dst, a, b, el, it in steps:
        if op == OPS["dilate"]:
            planes[dst] = dilate_np(planes[a], elements[el][0], elements[el][1], it)
        elif op == OPS["erode"]:
            planes[dst] = erode_np(planes[a], elements[el][0], elements[el][1], it)
        elif op == OPS["and"]:
            planes[dst] = planes[a] & planes[b]
        elif op == OPS["andnot"]:
            planes[dst] = planes[a] & ~planes[b]
        elif op == OPS["or"]:
            planes[dst] = planes[a] | planes[b]
        else:
            planes[dst] = planes[a].copy()
    return (planes[result_plane] * np.uint8(out_value)).astype(np.uint8)


# ---- the programs the NestedUNet methods launch (one unetpp_morphology call each) ------------------------------------
def program_single(op, element, anchor=None, iterations=1):
    """dilate | erode | open | close of plane 0 -> (elements, steps, result_plane)."""
    if op not in ("dilate", "erode", "open", "close"):
        raise ValueError(f"op must be one of dilate, erode, open, close, got {op!r}")
    el = [(element, anchor)]
    if op in ("dilate", "erode"):
        return el, [(op, 2, 0, 0, 0, iterations)], 2
    first, second = ("erode", "dilate") if op == "open" else ("dilate", "erode")
    return el, [(first, 2, 0, 0, 0, iterations), (second, 2, 2, 0, 0, iterations)], 2


def program_cleanup(kernel_size):
    """apply_morphology_cleanup (src/refactor/postprocess.py:144-166): open then close with ELLIPSE (k, k)."""
    el = [structuring_element("ellipse", kernel_size)]
    return el, [("erode", 2, 0, 0, 0, 1), ("dilate", 2, 2, 0, 0, 1), ("dilate", 2, 2, 0, 0, 1), ("erode", 2, 2, 0, 0, 1)], 2


def program_band(band_out):
    """The boundary band of src/refactor/burr_detector.py:37-41: dilate(cable, ELLIPSE (2 band_out + 1)) - cable."""
    el = [structuring_element("ellipse", 2 * int(band_out) + 1)]
    return el, [("dilate", 2, 0, 0, 0, 1), ("andnot", 2, 2, 0)], 2


def program_ring(ring_dilate=15, ring_erode=5):
    """The ring of constrain_tape_to_ring (src/refactor/postprocess.py:94-104) with plane 0 = tape, plane 1 = cable:
    tape & (dilate(cable, E ring_dilate) - erode(cable, E ring_erode))."""
    el = [structuring_element("ellipse", ring_dilate), structuring_element("ellipse", ring_erode)]
    return el, [("dilate", 2, 1, 0, 0, 1), ("erode", 3, 1, 0, 1, 1), ("andnot", 2, 2, 3), ("and", 2, 2, 0)], 2


def program_holes():
    """The hole mask of analyze_defects (src/utils/geometry_enhanced.py:281-284): close(tape, ELLIPSE (5,5)) - tape."""
    el = [structuring_element("ellipse", 5)]
    return el, [("dilate", 2, 0, 0, 0, 1), ("erode", 2, 2, 0, 0, 1), ("andnot", 2, 2, 0)], 2


def make_hole_scene(H, W, seed, n=40, noise=0.02):
    """components.make_scene_mask(H, W, seed, noise) with n discs of radius 0.8 .. 3.2 px punched out of the tape class
    (set to background): the holes analyze_defects counts."""
    m = cc.make_scene_mask(H, W, seed, noise)
    r = np.random.default_rng(1000 + seed)
    ys, xs = np.nonzero(m == 2)
    y = np.arange(H)[:, None]; x = np.arange(W)[None, :]
    for k in r.integers(0, len(ys), n):
        rad = r.uniform(0.8, 3.2)
        m[((y - ys[k]) ** 2 + (x - xs[k]) ** 2) <= rad * rad] = 0
    return m


def tape_holes_np(pred2d, tape_class=2, hole_min_size=10):
    """(tape_num_holes, hole area, hole mask uint8) of analyze_defects for one frame, from the restatement."""
    el, steps, res = program_holes()
    holes = run_program_np(pred2d, None, el, steps, tape_class, -1, res, 1)
    _, stats, _ = cc.components_np(holes, 8, -1)
    areas = stats[1:, cc.CC_STAT_AREA].astype(np.int64)
    valid = areas[areas >= hole_min_size]
    return int(len(valid)), int(valid.sum()), holes


# ---- the reference's compositions, restated on the programs above and components.py ----------------------------------
def constrain_tape_to_ring_np(tape2d, cable2d, tape_class=-1, cable_class=-1, ring_dilate=15, ring_erode=5, out_value=255):
    """What NestedUNet.constrain_tape_to_ring computes for one frame."""
    el, steps, res = program_ring(ring_dilate, ring_erode)
    ring = run_program_np(tape2d, cable2d, el, steps, tape_class, cable_class, res, 1)
    return cc.filter_components_np(ring, 1, "largest", min_area=0, out_value=out_value)


def postprocess_masks_np(pred2d, cable_class=1, tape_class=2, roi_width=None, out_value=255, **cable_kw):
    """What NestedUNet.postprocess_masks computes for one frame: (filtered cable, constrained tape)."""
    cable = cc.filter_components_np(pred2d, cable_class, "cable_shape", out_value=out_value,
                                    roi_width=pred2d.shape[1] if roi_width is None else roi_width, **cable_kw)
    return cable, constrain_tape_to_ring_np(pred2d, cable, tape_class, -1, out_value=out_value)


def cleanup_np(mask2d, match_class=-1, kernel_size=3, out_value=1):
    """What NestedUNet.morphology_cleanup computes for one frame."""
    el, steps, res = program_cleanup(kernel_size)
    return run_program_np(mask2d, None, el, steps, match_class, -1, res, out_value)
