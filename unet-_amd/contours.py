"""The tail of the refactored frame loop (infer_video_refactored.py:366-405): paste_roi_mask, measure_diameter (the smallest
circle around the largest outer contour) and the three chained blends of create_overlay.  The NumPy forms below are the
definition; the device functions (csrc/contours.h behind include/unetpp_contours.h) are held to them with ==.

What the device computes, and why it equals the contour form:
  * `inside` = every pixel that is not 4-connected background reachable from beyond the zero-padded frame.  One 8-connected
    component of `inside` is one RETR_EXTERNAL contour with its holes and whatever lies in them; labels are numbered in
    raster order of first pixels, which is also the order in which findContours meets the contours.
  * twice the contourArea of a contour = the sum over every 2 x 2 window of pixel centres of (2 where all four pixels are
    inside and of its label, 1 where exactly three are).  tests/test_contours.py checks the identity on every 4 x 5 mask.
  * the smallest circle around a contour is the smallest circle around the row extremes of its label.  Its support set is
    found with integer predicates only; the floats come from exact rational arithmetic rounded once, so they do not depend
    on which of several equivalent support sets (a rectangle's four corners lie on one circle) an implementation ends on.
"""
from __future__ import annotations

import math

import numpy as np

from .components import components_np, foreground

MAX_SIDE = 4095                                      # coordinates below 2^12: the in-circle determinant stays below 2^52
OVERLAY_COLOURS = ((0, 255, 0), (255, 0, 0), (0, 0, 255))          # cable, tape, burr (create_overlay :195, :198, :201)

# the 8 directions of the border following, counter-clockwise on the screen from east: (dx, dy)
_DIRS = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))


# ---- findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) ---------------------------------------------------------------------------
def _trace_external(img, step, height, width):
    """Suzuki-Abe border following on the zero-padded image `img` (a flat list, 0/1, `step` columns, the frame in rows and
    columns 1..height / 1..width) as findContours runs it for RETR_EXTERNAL: holes are never followed, an outer border is
    followed only when the last marked pixel met in the row is a right-hand border pixel (negative) or none.  Border pixels
    are marked 2, or -2 where the search looked east of them and found background.  Returns [(points, ...)] with points a
    flat list x0, y0, x1, y1, ... in frame coordinates, CHAIN_APPROX_SIMPLE (a point where the direction changes)."""
    deltas = [dx + dy * step for dx, dy in _DIRS]
    contours = []
    for y in range(1, height + 1):
        row = y * step
        prev, lnbd = 0, row                                  # lnbd: index of the last marked pixel of this row (column 0: none)
        for x in range(1, width + 1):
            i0 = row + x
            p = img[i0]
            if p != prev:
                if prev == 0 and p == 1 and img[lnbd] <= 0:
                    # -- follow the outer border that starts here
                    pts = []
                    s = 4
                    while True:                              # clockwise from the west neighbour
                        s = (s - 1) & 7
                        if img[i0 + deltas[s]] != 0 or s == 4:
                            break
                    if s == 4:                               # an isolated pixel
                        img[i0] = -2
                        pts += (x - 1, y - 1)
                    else:
                        i1 = i0 + deltas[s]
                        i3, px, py = i0, x, y
                        prev_s = s ^ 4
                        while True:
                            s_end = s
                            while True:                      # counter-clockwise from the pixel we came from
                                s = (s + 1) & 7
                                i4 = i3 + deltas[s]
                                if img[i4] != 0:
                                    break
                            if 0 < s <= s_end:               # the sweep passed east and found it empty: a right-hand border pixel
                                img[i3] = -2
                            elif img[i3] == 1:
                                img[i3] = 2
                            if s != prev_s:
                                pts += (px - 1, py - 1)
                            prev_s = s
                            px += _DIRS[s][0]
                            py += _DIRS[s][1]
                            if i4 == i0 and i3 == i1:
                                break
                            i3 = i4
                            s = (s + 4) & 7
                    contours.append(pts)
                    p = img[i0]
            prev = p
            if p != 0 and p != 1:
                lnbd = i0
    return contours


def find_external_contours_np(mask):
    """cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)[0] for a 2-D mask (non-zero = foreground): the published
    Suzuki-Abe border following (CVGIP 30, 1985) as findContours applies it.  The frame is treated as zero-padded, foreground
    is 8-connected, only outermost borders are followed (a component inside a hole of another gives no contour), and only
    the end points of straight runs are kept.  Returns a list of int32 [n,1,2] arrays of (x, y), in the order the raster
    scan meets the contours' first pixels; each starts at that pixel."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask must be [H,W]")
    h, w = m.shape
    pad = np.zeros((h + 2, w + 2), np.int8)
    pad[1:-1, 1:-1] = m != 0
    return [np.asarray(p, np.int32).reshape(-1, 1, 2) for p in _trace_external(pad.reshape(-1).tolist(), w + 2, h, w)]


def _area2(pts):
    """Twice the signed area (Green's formula) of a flat list x0, y0, x1, y1, ...: an integer."""
    a, n = 0, len(pts)
    xp, yp = pts[n - 2], pts[n - 1]
    for i in range(0, n, 2):
        x, y = pts[i], pts[i + 1]
        a += xp * y - x * yp
        xp, yp = x, y
    return a


def contour_area_np(contour):
    """cv2.contourArea(contour): |sum(x[i-1] y[i] - x[i] y[i-1])| / 2 in float64.  Twice the area is an integer for integer
    points, so the value is exact."""
    pts = np.asarray(contour).reshape(-1).tolist()
    if not pts:
        return 0.0
    return abs(float(_area2(pts)) * 0.5)


# ---- the smallest enclosing circle ------------------------------------------------------------------------------------------------
def _outside(sup, p):
    """Is the integer point p strictly outside the circle the support tuple `sup` (1, 2 or 3 points) defines?  Integers only:
    1 point: p differs; 2 points (a diameter): (p - a).(p - b) > 0; 3 points: the in-circle determinant times the
    orientation, both relative to the first point."""
    if len(sup) == 1:
        return p != sup[0]
    if len(sup) == 2:
        (ax, ay), (bx, by) = sup
        return (p[0] - ax) * (p[0] - bx) + (p[1] - ay) * (p[1] - by) > 0
    (ax, ay), (bx, by), (cx, cy) = sup
    bx -= ax; by -= ay; cx -= ax; cy -= ay
    px, py = p[0] - ax, p[1] - ay
    b2, c2, p2 = bx * bx + by * by, cx * cx + cy * cy, px * px + py * py
    det = bx * (cy * p2 - c2 * py) - by * (cx * p2 - c2 * px) + b2 * (cx * py - cy * px)
    return det * (bx * cy - by * cx) > 0


def support_set_np(points):
    """A support set of the smallest enclosing circle of distinct integer points, in the order given: the incremental
    algorithm (a point outside the circle so far lies on the circle of the points up to it), three nested scans for "the
    first point outside".  Returns a tuple of 1, 2 or 3 (x, y) tuples; () for no points."""
    P = list(dict.fromkeys((int(x), int(y)) for x, y in points))
    n = len(P)
    if n == 0:
        return ()
    sup = (P[0],)
    for i in range(1, n):
        if not _outside(sup, P[i]):
            continue
        sup = (P[i], P[0])
        for j in range(1, i):
            if not _outside(sup, P[j]):
                continue
            sup = (P[i], P[j])
            for k in range(j):
                if _outside(sup, P[k]):
                    sup = (P[i], P[j], P[k])
    return sup


def circle_from_points(support):
    """((cx, cy), radius) in float64 of the circle 1, 2 or 3 integer points define.  The points are sorted by (y, x); then
      1 point   the point, radius 0
      2 points  the midpoint (exact), sqrt(dx^2 + dy^2) / 2
      3 points  the circumcircle: with b, c relative to a, D = 2 (bx cy - by cx), ux = cy |b|^2 - by |c|^2,
                uy = bx |c|^2 - cx |b|^2:  centre = ((ax D + ux) / D, (ay D + uy) / D), radius = sqrt((ux^2 + uy^2) / D^2)
    The numerators and denominators are exact integers and each quotient is rounded once (Python's int / int), the square root
    once more.  Three points of one circle give the same rationals whichever three they are, so the floats depend on the
    circle alone."""
    pts = sorted(((int(x), int(y)) for x, y in support), key=lambda p: (p[1], p[0]))
    if len(pts) == 0:
        return (0.0, 0.0), 0.0
    if len(pts) == 1:
        return (float(pts[0][0]), float(pts[0][1])), 0.0
    if len(pts) == 2:
        (ax, ay), (bx, by) = pts
        return ((ax + bx) / 2, (ay + by) / 2), math.sqrt(float((ax - bx) ** 2 + (ay - by) ** 2)) / 2
    (ax, ay), (bx, by), (cx, cy) = pts
    bx -= ax; by -= ay; cx -= ax; cy -= ay
    d = 2 * (bx * cy - by * cx)
    if d == 0:
        raise ValueError(f"the three points {pts} lie on one line")
    b2, c2 = bx * bx + by * by, cx * cx + cy * cy
    ux, uy = cy * b2 - by * c2, bx * c2 - cx * b2
    return ((ax * d + ux) / d, (ay * d + uy) / d), math.sqrt((ux * ux + uy * uy) / (d * d))


def min_enclosing_circle_np(points):
    """The exact smallest enclosing circle of integer points (any shape [..., 2] of (x, y)): ((cx, cy), radius) in float64.
    The support set of 1, 2 or 3 points is found with integer predicates only (support_set_np); centre and radius come from
    it by circle_from_points' fixed expression.  The result does not depend on the order of the points.  cv2's own
    minEnclosingCircle is a float32 iteration that pads the radius; its circle contains this one."""
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    if pts.size and (np.abs(pts).max() > MAX_SIDE):
        raise ValueError(f"coordinates must be at most {MAX_SIDE} in magnitude")
    return circle_from_points(support_set_np(pts.tolist()))


# ---- masks ---------------------------------------------------------------------------------------------------------------------
def _outside_background(fg):
    """bool [H,W]: the background pixels 4-connected to the zero padding around the frame."""
    h, w = fg.shape
    pad = np.ones((h + 2, w + 2), np.uint8)
    pad[1:-1, 1:-1] = ~fg
    lab, _, _ = components_np(pad, 4, -1)
    return (lab == lab[0, 0])[1:-1, 1:-1]


def inside_np(mask, match_class=-1):
    """uint8 0/1 [H,W]: everything but the outside background (the foreground, its holes and what lies in them)."""
    return (~_outside_background(foreground(mask, match_class))).astype(np.uint8)


def outer_border_np(mask, match_class=-1):
    """uint8 0/1 [H,W]: the pixels on any external contour = foreground pixels with a 4-neighbour in the outside background
    (the 4-connected background reachable from beyond the frame; the zero padding belongs to it)."""
    fg = foreground(mask, match_class)
    h, w = fg.shape
    out = np.ones((h + 2, w + 2), bool)
    out[1:-1, 1:-1] = _outside_background(fg)
    near = out[:-2, 1:-1] | out[2:, 1:-1] | out[1:-1, :-2] | out[1:-1, 2:]
    return (fg & near).astype(np.uint8)


def window_area2_np(labels, num):
    """int64 [num]: per label of an `inside` labelling, the sum over every 2 x 2 window of pixel centres (those hanging over
    the frame edge included) of 2 where all four pixels are inside, 1 where exactly three are.  The inside pixels of one
    window are 8-neighbours, so they share one label."""
    lab = np.asarray(labels)
    h, w = lab.shape
    pad = np.zeros((h + 2, w + 2), np.int64)
    pad[1:-1, 1:-1] = lab
    q = np.stack((pad[:-1, :-1], pad[:-1, 1:], pad[1:, :-1], pad[1:, 1:]))
    n = (q > 0).sum(0)
    out = np.zeros(max(int(num), 1), np.int64)
    np.add.at(out, q.max(0)[n >= 3], n[n >= 3] - 2)
    out[0] = 0
    return out


def external_contour_areas_np(mask, match_class=-1):
    """(labels int32 [H,W] of `inside` at connectivity 8, num (background included), area2 int64 [num]): label l is the l-th
    external contour find_external_contours_np meets, area2[l] twice its contourArea (area2[0] = 0)."""
    labels, stats, _ = components_np(inside_np(mask, match_class), 8, -1)
    return labels, len(stats), window_area2_np(labels, len(stats))


def measure_diameter_np(mask):
    """measure_diameter (infer_video_refactored.py:148-172) from the three functions above: 0.0 for an empty mask, else twice
    the radius of the smallest circle around the external contour of largest contourArea.  Among contours of equal area the
    one whose first raster pixel comes first wins (max() keeps the first; cv2's own contour order is not pinned)."""
    m = np.asarray(mask)
    if m.size == 0 or m.max() == 0:
        return 0.0
    contours = find_external_contours_np(m.astype(np.uint8))
    if len(contours) == 0:
        return 0.0
    largest = max(contours, key=contour_area_np)
    return min_enclosing_circle_np(largest)[1] * 2.0


def row_extremes_np(labels, chosen):
    """The points (x, y) the device's circle is built from: per row the first and last column of `labels == chosen`."""
    pts = []
    for y, row in enumerate(np.asarray(labels) == chosen):
        xs = np.flatnonzero(row)
        if xs.size:
            pts.append((int(xs[0]), y))
            if xs[-1] != xs[0]:
                pts.append((int(xs[-1]), y))
    return pts


def support_table_np(mask, match_class=-1):
    """The circle of the device's table for one frame, from the labelling: (chosen label, ((cx, cy), radius)); label 0 and a
    zero circle for a frame without foreground.  The chosen label has the largest area2, the lowest label on ties."""
    labels, num, area2 = external_contour_areas_np(mask, match_class)
    if num < 2:
        return 0, ((0.0, 0.0), 0.0)
    chosen = 1 + int(np.argmax(area2[1:]))
    return chosen, min_enclosing_circle_np(row_extremes_np(labels, chosen))


# ---- paste and overlay ------------------------------------------------------------------------------------------------------------
def roi_paste_bounds(frame_h, frame_w, roi_xywh, roi_h, roi_w):
    """paste_roi_mask's clamp (src/refactor/preprocess.py:128-139): (x1, y1, paste_w, paste_h), possibly empty."""
    x, y, w, h = (int(v) for v in roi_xywh)
    x1, y1 = max(0, x), max(0, y)
    x2, y2 = min(int(frame_w), x + w), min(int(frame_h), y + h)
    return x1, y1, min(int(roi_w), x2 - x1), min(int(roi_h), y2 - y1)


def paste_roi_masks_np(masks, roi_xywh, frame_hw):
    """paste_roi_mask into a zero frame for uint8 masks [..., h, w]: zeros outside the clamped ROI."""
    m = np.asarray(masks, np.uint8)
    fh, fw = int(frame_hw[0]), int(frame_hw[1])
    x1, y1, pw, ph = roi_paste_bounds(fh, fw, roi_xywh, m.shape[-2], m.shape[-1])
    out = np.zeros(m.shape[:-2] + (fh, fw), np.uint8)
    if pw > 0 and ph > 0:
        out[..., y1:y1 + ph, x1:x1 + pw] = m[..., :ph, :pw]
    return out


def overlay_table():
    """uint8 [3 masks, 3 channels, 256]: table[m, c, x] = uint8(x * 0.6 + colour[m][c] * 0.4), the reference's own float64
    expression, truncated as the assignment into a uint8 image does."""
    x = np.arange(256)
    return np.stack([np.stack([(x * 0.6 + np.array(col)[c] * 0.4).astype(np.uint8) for c in range(3)]) for col in OVERLAY_COLOURS])


def create_overlay_masks_np(frame, cable, tape, burr):
    """Lines :191-201 of create_overlay for one uint8 BGR frame [H,W,3] and three masks [H,W]: three sequential 0.6 / 0.4
    blends (green, blue, red in BGR order), each on the result of the one before, in float64 and assigned into uint8."""
    overlay = np.array(frame, np.uint8, copy=True)
    for m, col in zip((cable, tape, burr), OVERLAY_COLOURS):
        m = np.asarray(m)
        if m.max() > 0:
            overlay[m > 0] = overlay[m > 0] * 0.6 + np.array(col) * 0.4
    return overlay


# ---- argument checks (shared by the device functions; no torch) -------------------------------------------------------------------
def check_frame_shape(h, w):
    """The sides the circle's integer predicates are proved for: coordinates below 2^12, so that each of the six products of
    the in-circle determinant stays below 2^50 and the determinant inside int64."""
    if not (1 <= int(h) <= MAX_SIDE and 1 <= int(w) <= MAX_SIDE):
        raise ValueError(f"frames of {h}x{w}: the contour functions take 1 <= H, W <= {MAX_SIDE}")
    assert 6 * MAX_SIDE * MAX_SIDE * (2 * MAX_SIDE * MAX_SIDE) < 2 ** 63


def check_max_components(max_components):
    k = int(max_components)
    if k < 2:
        raise ValueError(f"max_components must be at least 2 (background + one contour), got {max_components!r}")
    return k


def check_paste(roi_h, roi_w, roi_xywh, frame_hw):
    """-> (x, y, w, h, frame_h, frame_w) as ints; ValueError for a ROI that misses the frame."""
    if len(tuple(roi_xywh)) != 4 or len(tuple(frame_hw)) != 2:
        raise ValueError("roi_xywh must be (x, y, w, h) and frame_hw (height, width)")
    fh, fw = int(frame_hw[0]), int(frame_hw[1])
    _, _, pw, ph = roi_paste_bounds(fh, fw, roi_xywh, roi_h, roi_w)
    if pw < 1 or ph < 1 or fh < 1 or fw < 1:
        raise ValueError(f"roi {tuple(int(v) for v in roi_xywh)} does not meet the {fh}x{fw} frame")
    return tuple(int(v) for v in roi_xywh) + (fh, fw)


def _raise_contour_overflow(what, nums, k):
    for name, col in nums:
        for i, v in enumerate(col):
            if v > k:
                raise ValueError(f"{what}: frame {i} has num = {v} labels in its {name} labelling (background included), more than "
                                 f"max_components = {k}: raise max_components")


# ---- the device path (torch imported lazily, as in loss.py) -----------------------------------------------------------------------
def _mask(model, mask, what="mask"):
    mask = model._input(mask, what)
    check_frame_shape(mask.shape[1], mask.shape[2])
    return mask


def _workspace(model, b, h, w, k, device):
    from . import _lib
    return model._workspace(("contours", b, h, w, k), lambda: _lib.load().unetpp_contours_workspace_bytes(b, h, w, k), device,
                            f"contours: unsupported shape {(b, h, w)}")


def _areas(model, mask, match_class, max_components, want_border):
    import torch
    k = check_max_components(max_components)
    mask = _mask(model, mask)
    b, h, w = mask.shape
    dev = mask.device
    ws = _workspace(model, b, h, w, k, dev)
    labels = torch.empty((b, h, w), dtype=torch.int32, device=dev)
    num = torch.empty((b,), dtype=torch.int32, device=dev)
    area2 = torch.empty((b, k), dtype=torch.int64, device=dev)               # uint64 bits; values below 2^25
    border = torch.empty((b, h, w), dtype=torch.uint8, device=dev) if want_border else None
    model._call("unetpp_contour_areas_u8", mask, b, h, w, int(match_class), k, labels, num, area2, border, ws, stream_of=mask)
    return labels, num, area2, border, ws, k


def outer_border(model, mask, match_class=-1, max_components=8192):
    """outer_border_np per frame of a uint8 CUDA mask [B,H,W] (H, W <= 4095): uint8 0/1 [B,H,W] on the device, the pixels of
    the external contours.  Nothing is read back (the border does not depend on max_components)."""
    return _areas(model, mask, match_class, max_components, True)[3]


def external_contour_areas(model, mask, match_class=-1, max_components=8192, check=True):
    """external_contour_areas_np per frame on the device -> (labels int32 [B,H,W], num int32 [B], area2 int64 [B,cap]): one
    label per external contour in raster order of first pixels, num counts the background, area2[b, l] is twice the
    contourArea of contour l (rows >= num zero).  check=True reads num back (synchronises) and raises ValueError for a frame
    with more than max_components labels; with check=False the labels >= max_components have no row."""
    labels, num, area2, _, _, k = _areas(model, mask, match_class, max_components, False)
    if check:
        _raise_contour_overflow("external_contour_areas", (("contour", num.cpu().tolist()),), k)
    return labels, num, area2


def _support(model, mask, match_class, max_components):
    import torch
    labels, num, area2, _, ws, k = _areas(model, mask, match_class, max_components, False)
    b, h, w = labels.shape
    table = torch.empty((b, 8), dtype=torch.int32, device=labels.device)
    model._call("unetpp_contour_circle", labels, num, area2, b, h, w, k, table, ws, stream_of=labels)
    return table, num, k


def enclosing_circle(model, mask, match_class=-1, max_components=8192, check=True):
    """The support table int32 [B,8] on the device: {count, x0, y0, x1, y1, x2, y2, label} of the smallest circle around the
    external contour of largest area (the lowest label on ties; count 0 for a frame without foreground).  circle_from_support
    turns it into floats on the host.  check as in external_contour_areas."""
    table, num, k = _support(model, mask, match_class, max_components)
    if check:
        _raise_contour_overflow("enclosing_circle", (("contour", num.cpu().tolist()),), k)
    return table


def circle_from_support(table):
    """[((cx, cy), radius)] per row of a support table (a host array or anything np.asarray takes), by circle_from_points."""
    out = []
    for row in np.asarray(table).reshape(-1, 8).tolist():
        out.append(circle_from_points([(row[1 + 2 * i], row[2 + 2 * i]) for i in range(row[0])]))
    return out


def measure_diameter(model, mask, match_class=-1, max_components=8192):
    """measure_diameter_np per frame of a uint8 CUDA mask [B,H,W]: float64 [B] (a host array) after one small read-back, the
    support table and num.  ValueError for a frame with more than max_components labels."""
    import torch
    table, num, k = _support(model, mask, match_class, max_components)
    got = torch.cat((table.reshape(-1), num)).cpu().numpy()
    _raise_contour_overflow("measure_diameter", (("contour", got[table.numel():].tolist()),), k)
    return np.array([2.0 * r for _, r in circle_from_support(got[:table.numel()])], np.float64)


def paste_roi_masks(model, masks, roi_xywh, frame_hw):
    """paste_roi_masks_np on the device for uint8 CUDA masks [B,h,w] (the ROI crop's size): uint8 [B,frame_h,frame_w], zeros
    outside the clamped ROI; one launch.  ValueError for a ROI that misses the frame."""
    import torch
    masks = model._input(masks, "masks")
    b, h, w = masks.shape
    x, y, rw, rh, fh, fw = check_paste(h, w, roi_xywh, frame_hw)
    out = torch.empty((b, fh, fw), dtype=torch.uint8, device=masks.device)
    model._call("unetpp_paste_roi_u8", masks, b, h, w, x, y, rw, rh, fh, fw, out, stream_of=masks)
    return out


_TABLE = None


def create_overlay_masks(model, frames, cable, tape, burr):
    """create_overlay_masks_np per frame on the device for uint8 CUDA frames [B,H,W,3] (BGR) and three uint8 masks [B,H,W]
    (non-zero = set): uint8 [B,H,W,3]; one launch of chained look-ups in overlay_table()."""
    import ctypes
    import torch
    global _TABLE
    frames = model._input(frames, "frames", "[B,H,W,3]")
    b, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    planes = []
    for t, what in ((cable, "cable"), (tape, "tape"), (burr, "burr")):
        t = model._input(t, what)
        if tuple(t.shape) != (b, h, w):
            raise RuntimeError(f"{what} {tuple(t.shape)} does not match the frames {(b, h, w)}")
        planes.append(t)
    if _TABLE is None:
        _TABLE = np.ascontiguousarray(overlay_table())
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=frames.device)
    model._call("unetpp_overlay_chain_u8", frames, planes[0], planes[1], planes[2], b, h, w,
                _TABLE.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out, stream_of=frames)
    return out
