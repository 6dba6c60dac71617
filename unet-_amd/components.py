"""CPU restatement (NumPy only) of the device's connected-component labelling and of the reference's three
component filters, plus the scene generator the component tests and fixtures share.

The contract (include/unetpp.h, unetpp_components): labels are int32, 0 = background, components 1..n numbered in
raster order of their first pixel (scipy.ndimage.label's order; cv2's own numbering is an artefact of its block
algorithm and is not reproduced -- it only decides ties between components of equal area / score, which here go to
the lower label).  stats rows are cv2's LEFT, TOP, WIDTH, HEIGHT, AREA with row 0 = background; sums = (sum x, sum y)
per label, so that cv2's double centroids are sums / area in one correctly rounded division.
"""
from __future__ import annotations

import numpy as np

CC_STAT_LEFT, CC_STAT_TOP, CC_STAT_WIDTH, CC_STAT_HEIGHT, CC_STAT_AREA = 0, 1, 2, 3, 4
RULES = {"largest": 0, "spatial": 1, "cable_shape": 2}


def make_scene_mask(H, W, seed, noise=0.02):
    """A cable frame as the reference's loops see it: bare cable above, wider taped part below, one distractor per
    class and 2 % speckle of every class."""
    r = np.random.default_rng(seed)
    y = np.arange(H)[:, None]; x = np.arange(W)[None, :]
    cx = W / 2 + (W * 0.03) * np.sin(y / H * 6.28 * r.uniform(0.5, 2)) + r.uniform(-W * 0.05, W * 0.05)
    split = int(H * r.uniform(0.45, 0.6))
    hw_c = W * 0.09 * (1 + 0.08 * np.sin(y / H * 6.28 * 3)); hw_t = hw_c * 1.55
    mask = np.zeros((H, W), np.uint8)
    mask[(np.abs(x - cx) < hw_c) & (y < split)] = 1                           # bare cable
    mask[(np.abs(x - cx) < hw_t) & (y >= split)] = 2                          # taped part, wider
    mask[H // 8:H // 8 + H // 3, W // 16:W // 16 + W // 8] = 1                # passes area + aspect, fails the centre gate
    mask[H // 2:H // 2 + H // 10, W - W // 5:W - W // 5 + W // 6] = 2         # too short for `spatial`
    n = r.random((H, W)); k = n < noise
    mask[k] = r.integers(0, 3, (H, W), dtype=np.uint8)[k]                     # 2 % speckle of every class
    return mask


def foreground(mask, match_class):
    """mask == match_class, or mask != 0 for match_class < 0."""
    mask = np.asarray(mask)
    return (mask != 0) if match_class < 0 else (mask == match_class)


def _runs(fg):
    """Horizontal runs of a boolean image in raster order: (row, first column, last column)."""
    H, W = fg.shape
    p = np.zeros((H, W + 2), np.int8)
    p[:, 1:-1] = fg
    d = np.diff(p, axis=1)
    ry, x0 = np.nonzero(d == 1)
    _, x1 = np.nonzero(d == -1)
    return ry.astype(np.int64), x0.astype(np.int64), x1.astype(np.int64) - 1


def components_np(mask2d, connectivity=8, match_class=-1):
    """labels int32 [H,W], stats int32 [n+1,5], sums uint64 [n+1,2] of one frame (row 0 = background)."""
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    fg = foreground(mask2d, match_class)
    if fg.ndim != 2:
        raise ValueError("mask2d must be [H,W]")
    H, W = fg.shape
    ry, x0, x1 = _runs(fg)
    n = len(ry)
    parent = list(range(n))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    d = 1 if connectivity == 8 else 0
    row_start = np.searchsorted(ry, np.arange(H + 1))
    X0, X1 = x0.tolist(), x1.tolist()
    for y in range(1, H):
        i, i_end = int(row_start[y]), int(row_start[y + 1])
        j, j_end = int(row_start[y - 1]), int(row_start[y])
        while i < i_end and j < j_end:
            if X1[j] + d < X0[i]:
                j += 1
            elif X1[i] + d < X0[j]:
                i += 1
            else:                                   # the runs touch: one component, rooted at the earlier run
                a, b = find(i), find(j)
                if a < b:
                    parent[b] = a
                elif b < a:
                    parent[a] = b
                if X1[j] < X1[i]:
                    j += 1
                else:
                    i += 1
    root = np.fromiter((find(a) for a in range(n)), np.int64, n)
    is_root = root == np.arange(n)
    dense = np.cumsum(is_root)                      # roots are each component's first run: raster order of first pixels
    lab = dense[root] if n else np.zeros(0, np.int64)
    ncomp = int(is_root.sum())

    flat = np.zeros(H * W + 1, np.int64)
    start = ry * W + x0
    np.add.at(flat, start, lab)
    np.add.at(flat, ry * W + x1 + 1, -lab)
    labels = np.cumsum(flat[:-1]).astype(np.int32).reshape(H, W)

    stats = np.zeros((ncomp + 1, 5), np.int32)
    sums = np.zeros((ncomp + 1, 2), np.uint64)
    ln = x1 - x0 + 1
    area = np.zeros(ncomp + 1, np.int64)
    np.add.at(area, lab, ln)
    sx = np.zeros(ncomp + 1, np.int64); sy = np.zeros(ncomp + 1, np.int64)
    np.add.at(sx, lab, ln * (x0 + x1) // 2)
    np.add.at(sy, lab, ln * ry)
    left = np.full(ncomp + 1, W, np.int64); right = np.full(ncomp + 1, -1, np.int64)
    top = np.full(ncomp + 1, H, np.int64); bot = np.full(ncomp + 1, -1, np.int64)
    np.minimum.at(left, lab, x0); np.maximum.at(right, lab, x1)
    np.minimum.at(top, lab, ry); np.maximum.at(bot, lab, ry)
    # background: everything the runs leave out
    bg = ~fg
    area[0] = int(bg.sum())
    if area[0]:
        ys, xs = np.nonzero(bg)
        left[0], right[0], top[0], bot[0] = xs.min(), xs.max(), ys.min(), ys.max()
        sx[0], sy[0] = int(xs.sum()), int(ys.sum())
    ok = area > 0
    stats[ok, CC_STAT_LEFT] = left[ok]; stats[ok, CC_STAT_TOP] = top[ok]
    stats[ok, CC_STAT_WIDTH] = (right - left + 1)[ok]; stats[ok, CC_STAT_HEIGHT] = (bot - top + 1)[ok]
    stats[:, CC_STAT_AREA] = area
    sums[:, 0] = sx.astype(np.uint64); sums[:, 1] = sy.astype(np.uint64)
    return labels, stats, sums


def centroids_np(stats, sums):
    """cv2's double centroids: one correctly rounded division per coordinate (NaN for an empty row)."""
    area = stats[..., CC_STAT_AREA].astype(np.float64)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums.astype(np.float64) / area


# ---- the reference's filters, decided from the stats --------------------------------------------------------
def keep_largest(stats, min_area=100):
    """_largest_connected_component (src/utils/geometry_enhanced.py:81-110): the first of the largest components with
    area >= min_area; min_area = 0 is the tail of constrain_tape_to_ring (src/refactor/postprocess.py:106-116)."""
    keep = np.zeros(len(stats), bool)
    area = stats[1:, CC_STAT_AREA].astype(np.int64)
    valid = np.nonzero(area >= min_area)[0]
    if len(valid):
        keep[1 + int(valid[np.argmax(area[valid])])] = True
    return keep


def keep_spatial(stats, frame_h, min_area=1000, min_width=50, max_width=300, min_height_ratio=0.3):
    """spatial_filter (infer_video_spatial.py:24-53): every component passing the area / width / height gates."""
    keep = np.zeros(len(stats), bool)
    for i in range(1, len(stats)):
        area, width, height = int(stats[i, CC_STAT_AREA]), int(stats[i, CC_STAT_WIDTH]), int(stats[i, CC_STAT_HEIGHT])
        keep[i] = area > min_area and min_width <= width <= max_width and height >= frame_h * min_height_ratio
    return keep


def keep_cable_shape(stats, sums, roi_width, min_area=1000, min_aspect=1.6, max_center_offset=0.3):
    """filter_cable_by_shape (src/refactor/postprocess.py:12-76), line for line in fp64."""
    keep = np.zeros(len(stats), bool)
    roi_center_x = float(roi_width) / 2.0
    best_score, best_label = -1.0, -1
    for label in range(1, len(stats)):
        area = int(stats[label, CC_STAT_AREA])
        w, h = int(stats[label, CC_STAT_WIDTH]), int(stats[label, CC_STAT_HEIGHT])
        if area < min_area:
            continue
        aspect = float(max(w, h)) / (float(min(w, h)) + 1e-6)
        if aspect < min_aspect:
            continue
        cx = float(sums[label, 0]) / float(area)
        center_offset = abs(cx - roi_center_x) / float(roi_width)
        if center_offset > max_center_offset:
            continue
        score = float(area) * aspect * (1.0 - center_offset)
        if score > best_score:
            best_score, best_label = score, label
    if best_label > 0:
        keep[best_label] = True
    return keep


def filter_components_np(mask2d, match_class=-1, rule="largest", connectivity=8, out_value=1, **params):
    """What NestedUNet.filter_components computes for one frame: uint8 [H,W], out_value where kept."""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {sorted(RULES)}")
    labels, stats, sums = components_np(mask2d, connectivity, match_class)
    if rule == "largest":
        keep = keep_largest(stats, params.get("min_area", 100))
    elif rule == "spatial":
        keep = keep_spatial(stats, labels.shape[0], params.get("min_area", 1000), params.get("min_width", 50),
                            params.get("max_width", 300), params.get("min_height_ratio", 0.3))
    else:
        keep = keep_cable_shape(stats, sums, params.get("roi_width", labels.shape[1]), params.get("min_area", 1000),
                                params.get("min_aspect", 1.6), params.get("max_center_offset", 0.3))
    return (keep[labels] * np.uint8(out_value)).astype(np.uint8)


def make_adversarial_masks(H=512, W=512, tile_h=32, tile_w=128):
    """Binary masks on which a wrong merge or a missed equivalence of a tiled labelling shows, as {name: uint8 [H,W]}
    (tile_h x tile_w is the device kernel's tile)."""
    y = np.arange(H)[:, None]; x = np.arange(W)[None, :]
    out = {"ones": np.ones((H, W), np.uint8), "zeros": np.zeros((H, W), np.uint8)}
    s = np.zeros((H, W), np.uint8)                      # one-pixel-wide serpentine over the whole frame: one component
    s[0::2, :] = 1
    s[1::4, W - 1] = 1
    s[3::4, 0] = 1
    out["serpentine"] = s
    c = np.zeros((H, W), np.uint8)                      # comb: the teeth join only in the last row
    c[:, 0::2] = 1
    c[H - 1, :] = 1
    out["comb"] = c
    out["diagonal"] = (x == y * W // H if H != W else x == y).astype(np.uint8) * np.ones((H, W), np.uint8)
    out["antidiagonal"] = np.ascontiguousarray(out["diagonal"][:, ::-1])
    out["tile_corners"] = (((y % tile_h == 0) | (y % tile_h == tile_h - 1)) &
                           ((x % tile_w == 0) | (x % tile_w == tile_w - 1))).astype(np.uint8)
    out["checkerboard"] = ((x + y) % 2).astype(np.uint8) * np.ones((H, W), np.uint8)
    return out
