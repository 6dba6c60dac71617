"""CPU restatement (NumPy only) of the grey-level steps of the reference's stage-2 burr detection and of its two
compositions, plus the scene generator the burr tests and fixtures share.

  detect_burrs_on_cable      infer_two_stage_burr.py:50-119 (also infer_high_res_custom_roi.py:50-93)
  get_burr_mask_rulebased    src/refactor/burr_detector.py:11-66

The device entries are declared in include/unetpp.h (unetpp_gray_u8, unetpp_gaussian_blur_u8, unetpp_canny_u8,
unetpp_laplacian_band_u8, unetpp_components_filter_box).  All arithmetic is integer, so every result is exact and the
tests compare for equality.  cv2 is not installed where this project is built and tested: the primitives below are
restated from OpenCV's published algorithms (8-bit fixed-point GaussianBlur, Canny with L2gradient off, Laplacian
with ksize 1, cvtColor's 15-bit constants) and cv2's own output stays UNPINNED, like the resizes and the morphology
(DESIGN.md §8).  Where a caller may hold cv2's own constants they are arguments: `taps=` everywhere a blur is used.
What the fixtures (scripts/make_golden_burr.py) pin on the reference's code is the composition: element sizes, the
`& ~mask_cable` arithmetic, close then open, 1 against 255, the clauses of the component loops.
"""
from __future__ import annotations

import math

import numpy as np

from . import components as cc
from . import morphology as mo

MAX_TAPS = 7            # the blur the device kernel fuses; more taps are refused there
MIN_SIDE = 8            # smallest image side of the device's blur and Canny
TG22 = 13573            # tan(22.5 deg) in 15 fractional bits (OpenCV's TG22)

# burr_configs of infer_two_stage_burr.py:194-198.  detect_burrs_on_cable reads min_area and max_area only: the band
# element (8), the blur, the Canny thresholds and the close / open elements are constants of the function, and
# band_out, laplacian_threshold and morph_kernel are never read by it.
PRESETS = {
    "low": {"band_out": 10, "laplacian_threshold": 35, "min_area": 50, "max_area": 800, "morph_kernel": 3},
    "medium": {"band_out": 15, "laplacian_threshold": 25, "min_area": 30, "max_area": 800, "morph_kernel": 3},
    "high": {"band_out": 20, "laplacian_threshold": 20, "min_area": 20, "max_area": 1000, "morph_kernel": 5},
}


def bgr_to_gray_np(frames):
    """cv2.cvtColor(frame, COLOR_BGR2GRAY) for uint8 [..,3]: (3735 B + 19235 G + 9798 R + 16384) >> 15.  These are
    OpenCV 4's 15-bit constants; OpenCV 3 used a 14-bit set (1868, 9617, 4899), which differs by one grey level on some
    colours.  The burr entry points take a grey frame, so the choice never reaches them."""
    f = np.asarray(frames)
    if f.dtype != np.uint8 or f.ndim < 1 or f.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 [..,3], got {f.dtype} {f.shape}")
    f = f.astype(np.int32)
    return ((3735 * f[..., 0] + 19235 * f[..., 1] + 9798 * f[..., 2] + 16384) >> 15).astype(np.uint8)


def gaussian_taps(ksize, sigma):
    """Integer taps with 8 fractional bits of cv2.getGaussianKernel(ksize, sigma): symmetric, summing to exactly 256.
    From the normalised exp(-x^2 / 2 sigma^2) kernel g, from the outside inwards: tap = round(256 g + carried error),
    the error of each rounding carried to the next tap, the centre taking what is left of 256.  (5, 1.0) gives
    [14, 62, 104, 62, 14].  sigma <= 0 means cv2's 0.3 ((ksize - 1) / 2 - 1) + 0.8.  This reading of OpenCV's
    fixed-point kernel is derived here and unpinned; pass cv2's own as `taps=` where it matters."""
    ksize = int(ksize)
    if ksize < 1 or ksize % 2 == 0:
        raise ValueError(f"ksize must be odd and positive, got {ksize!r}")
    sigma = float(sigma)
    if sigma <= 0:
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    r = ksize // 2
    g = [math.exp(-(x * x) / (2.0 * sigma * sigma)) for x in range(-r, r + 1)]
    total = sum(g)
    taps = [0] * ksize
    err = 0.0
    for i in range(r):
        want = 256.0 * g[i] / total + err
        taps[i] = taps[ksize - 1 - i] = int(math.floor(want + 0.5))
        err = want - taps[i]
    taps[r] = 256 - 2 * sum(taps[:r])
    return np.array(taps, np.int32)


def check_taps(taps):
    """int32 taps or ValueError for what the device refuses: an even or empty kernel, more than 7 taps, a tap outside
    [0,256], a sum other than 256."""
    t = np.asarray(taps)
    if t.ndim != 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"taps must be a 1-D integer array, got {t.dtype} {t.shape}")
    if len(t) < 1 or len(t) % 2 == 0:
        raise ValueError(f"the number of taps must be odd and positive, got {len(t)}")
    if len(t) > MAX_TAPS:
        raise ValueError(f"at most {MAX_TAPS} taps are supported, got {len(t)}")
    if (t < 0).any() or (t > 256).any():
        raise ValueError("every tap must lie in [0,256]")
    if int(t.sum()) != 256:
        raise ValueError(f"taps must sum to 256 (8 fractional bits), got {int(t.sum())}")
    return np.ascontiguousarray(t, np.int32)


def resolve_taps(ksize=5, sigma=1.0, taps=None):
    """The taps of a blur given as (ksize, sigma) or as `taps=`; None for ksize = 0 / None (no blur)."""
    if taps is not None:
        return check_taps(taps)
    if not ksize:
        return None
    return check_taps(gaussian_taps(ksize, sigma))


def _check_gray(gray):
    g = np.asarray(gray)
    if g.dtype != np.uint8 or g.ndim != 2:
        raise ValueError(f"expected a uint8 image [H,W], got {g.dtype} {g.shape}")
    return g


def gaussian_blur_np(gray, taps):
    """cv2.GaussianBlur's 8-bit path with the kernel `taps` (8 fractional bits) on both axes: horizontal pass into a
    16-bit 8.8 value, vertical pass into 32 bits, (acc + 32768) >> 16; BORDER_REFLECT_101."""
    g = _check_gray(gray)
    t = np.asarray(taps).astype(np.int64)
    r = len(t) // 2
    if len(t) % 2 == 0 or min(g.shape) <= r:
        raise ValueError(f"{len(t)} taps on a {g.shape} image: the kernel must be odd and shorter than twice the image side")
    p = np.pad(g.astype(np.int64), ((0, 0), (r, r)), mode="reflect") if r else g.astype(np.int64)
    W = g.shape[1]
    hor = sum(t[k] * p[:, k:k + W] for k in range(len(t)))
    assert hor.max(initial=0) < 65536
    p = np.pad(hor, ((r, r), (0, 0)), mode="reflect") if r else hor
    H = g.shape[0]
    acc = sum(t[k] * p[k:k + H] for k in range(len(t)))
    return ((acc + 32768) >> 16).astype(np.uint8)


def sobel_np(img):
    """(dx, dy) int32 of the 3x3 Sobel operator with BORDER_REPLICATE, as cv2.Canny computes them."""
    p = np.pad(_check_gray(img).astype(np.int32), 1, mode="edge")
    a, b, c = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    d, f = p[1:-1, :-2], p[1:-1, 2:]
    g, h, k = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    return (c + 2 * f + k) - (a + 2 * d + g), (g + 2 * h + k) - (a + 2 * b + c)


def canny_map_np(img, low, high):
    """The candidates of cv2.Canny(img, low, high) before hysteresis: uint8 [H,W], 0, 1 = weak candidate, 2 = strong.
    L2gradient off: mag = |dx| + |dy|, 0 outside the image; thresholds floored; low > high swaps them."""
    low, high = float(low), float(high)
    if not (low >= 0 and high >= 0):
        raise ValueError(f"thresholds must be non-negative, got {low!r}, {high!r}")
    if low > high:
        low, high = high, low
    ilow, ihigh = int(math.floor(min(low, 1e6))), int(math.floor(min(high, 1e6)))
    dx, dy = sobel_np(img)
    mag = np.abs(dx) + np.abs(dy)
    m = np.pad(mag, 1)                                     # magnitude 0 outside the image
    c = m[1:-1, 1:-1]
    left, right, up, down = m[1:-1, :-2], m[1:-1, 2:], m[:-2, 1:-1], m[2:, 1:-1]
    x = np.abs(dx)
    y = np.abs(dy) << 15
    tg22x = x * TG22
    horizontal = y < tg22x
    vertical = ~horizontal & (y > tg22x + (x << 16))
    diagonal = ~horizontal & ~vertical
    neg = (dx ^ dy) < 0                                    # s = -1: up-right and down-left; s = +1: up-left and down-right
    d_up = np.where(neg, m[:-2, 2:], m[:-2, :-2])
    d_down = np.where(neg, m[2:, :-2], m[2:, 2:])
    local_max = (horizontal & (c > left) & (c >= right)) | (vertical & (c > up) & (c >= down)) | (diagonal & (c > d_up) & (c > d_down))
    cand = (c > ilow) & local_max
    return (cand.astype(np.uint8) + (cand & (c > ihigh)).astype(np.uint8))


def hysteresis_np(cmap):
    """255 on every candidate (cmap != 0) that is 8-connected to a strong one (cmap == 2) through candidates."""
    cmap = np.asarray(cmap)
    labels, _, _ = cc.components_np(cmap, 8, -1)
    keep = np.zeros(int(labels.max()) + 1, bool)
    keep[np.unique(labels[cmap == 2])] = True
    keep[0] = False
    return (keep[labels] * np.uint8(255)).astype(np.uint8)


def canny_np(img, low, high):
    """cv2.Canny(img, low, high) (aperture 3, L2gradient off) for a uint8 image [H,W]: uint8, 0 or 255."""
    return hysteresis_np(canny_map_np(img, low, high))


def laplacian_np(gray):
    """cv2.Laplacian(gray, CV_64F) with ksize 1 as integers: 4 neighbours - 4 centre, BORDER_REFLECT_101."""
    p = np.pad(_check_gray(gray).astype(np.int32), 1, mode="reflect")
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * p[1:-1, 1:-1]


def laplacian_abs_u8_np(gray):
    """np.abs(cv2.Laplacian(gray, CV_64F)).astype(np.uint8) of src/refactor/burr_detector.py:44-45: |L| & 255.  The
    cast of a float64 above 255 wraps modulo 256 on the NumPy (x86-64) the fixtures were made with: 300 -> 44,
    1020 -> 252, 256 -> 0.  It is the reference's behaviour, so it is reproduced, not corrected."""
    return (np.abs(laplacian_np(gray)) & 255).astype(np.uint8)


def keep_box(stats, min_area=30, max_area=800, max_aspect=5.0, min_side=3):
    """The loop of detect_burrs_on_cable (infer_two_stage_burr.py:103-117): every component with
    min_area <= area <= max_area, max(w,h) / (min(w,h) + 1e-6) < max_aspect in fp64, w > min_side and h > min_side.
    max_aspect = inf and min_side = 0 leave the area clause of get_burr_mask_rulebased (burr_detector.py:60-64)."""
    keep = np.zeros(len(stats), bool)
    for i in range(1, len(stats)):
        area, w, h = int(stats[i, cc.CC_STAT_AREA]), int(stats[i, cc.CC_STAT_WIDTH]), int(stats[i, cc.CC_STAT_HEIGHT])
        aspect = float(max(w, h)) / (float(min(w, h)) + 1e-6)
        keep[i] = float(min_area) <= area <= float(max_area) and aspect < float(max_aspect) and w > float(min_side) and h > float(min_side)
    return keep


def filter_box_np(mask2d, match_class=-1, min_area=30, max_area=800, max_aspect=math.inf, min_side=0, out_value=1):
    """What NestedUNet.filter_components_box computes for one frame."""
    labels, stats, _ = cc.components_np(mask2d, 8, match_class)
    return (keep_box(stats, min_area, max_area, max_aspect, min_side)[labels] * np.uint8(out_value)).astype(np.uint8)


def program_burr(band_ksize=8, close_ksize=3, open_ksize=2):
    """Steps 2, 4, 5 and 6 of detect_burrs_on_cable (infer_two_stage_burr.py:78-97) as ONE morphology program with
    plane 0 = edges, plane 1 = cable: (dilate(cable, E band) & ~cable) & edges -> close with E close -> open with
    E open.  7 steps, 3 elements."""
    el = [mo.structuring_element("ellipse", band_ksize), mo.structuring_element("ellipse", close_ksize),
          mo.structuring_element("ellipse", open_ksize)]
    steps = [("dilate", 2, 1, 0, 0, 1), ("andnot", 2, 2, 1), ("and", 2, 2, 0),
             ("dilate", 2, 2, 0, 1, 1), ("erode", 2, 2, 0, 1, 1), ("erode", 2, 2, 0, 2, 1), ("dilate", 2, 2, 0, 2, 1)]
    return el, steps, 2


def burrs_from_edges_np(edges, mask_cable, match_class=-1, *, min_area=30, max_area=800, band_ksize=8, close_ksize=3, open_ksize=2,
                        max_aspect=5.0, min_side=3, out_value=1):
    """detect_burrs_on_cable after its cv2.Canny call (infer_two_stage_burr.py:78-117, without :85-86), for one frame:
    `edges` is the edge image (non-zero = edge).  What NestedUNet.burrs_from_edges computes."""
    el, steps, res = program_burr(band_ksize, close_ksize, open_ksize)
    cand = mo.run_program_np(edges, mask_cable, el, steps, -1, match_class, res, 1)
    return filter_box_np(cand, -1, min_area, max_area, max_aspect, min_side, out_value)


def detect_burrs_np(gray, mask_cable, match_class=-1, *, min_area=30, max_area=800, band_ksize=8, blur_ksize=5, blur_sigma=1.0,
                    taps=None, canny_low=50, canny_high=150, close_ksize=3, open_ksize=2, max_aspect=5.0, min_side=3, out_value=1):
    """What NestedUNet.detect_burrs computes for one frame: detect_burrs_on_cable(gray, mask_cable, config) with the
    function's constants as defaults.  An empty cable gives an empty band and so an empty result: the reference's two
    early returns."""
    t = resolve_taps(blur_ksize, blur_sigma, taps)
    blurred = _check_gray(gray) if t is None else gaussian_blur_np(gray, t)
    edges = canny_np(blurred, canny_low, canny_high)
    return burrs_from_edges_np(edges, mask_cable, match_class, min_area=min_area, max_area=max_area, band_ksize=band_ksize,
                               close_ksize=close_ksize, open_ksize=open_ksize, max_aspect=max_aspect, min_side=min_side,
                               out_value=out_value)


def burr_mask_rulebased_np(gray, mask_cable, match_class=-1, *, band_out=10, laplacian_threshold=30, min_area=20, max_area=500,
                           out_value=255):
    """What NestedUNet.burr_mask_rulebased computes for one frame: get_burr_mask_rulebased(gray, mask_cable,
    BurrConfig(band_out, laplacian_threshold, min_area, max_area))."""
    el, steps, res = mo.program_band(band_out)
    band = mo.run_program_np(mask_cable, None, el, steps, match_class, -1, res, 1)
    hot = ((band != 0) & (laplacian_abs_u8_np(gray) > int(math.floor(laplacian_threshold)))).astype(np.uint8)
    return filter_box_np(hot, -1, min_area, max_area, math.inf, 0, out_value)


def make_burr_scene(H, W, seed, noise_sigma=3.0):
    """(grey uint8 [H,W], cable uint8 0/1 [H,W]) for the burr tests: the cable class of components.make_scene_mask
    (distractor and speckle included, as a network's mask has them); a grey step one pixel inside the edge of the cable
    proper; max(60, H W / 1000) textured blobs of radius 2 .. 9 px centred on edge pixels of the mask (the burrs:
    stripes of period 4 in x or y with 15 % salt and pepper, so that the blur leaves dense edges and the Laplacian
    passes 255); sigma = 3 noise.  noise_sigma: another sigma for the same noise field (the multi-scale detector thresholds
    |Laplacian| at 15, which sigma = 3 noise alone passes on a quarter of all pixels, so its fixtures use 1)."""
    m = cc.make_scene_mask(H, W, seed)
    cable = (m == 1).astype(np.uint8)
    r = np.random.default_rng(5003 + seed)
    solid, _, _ = cc.components_np(cable, 8, -1)
    body = solid == (1 + int(np.argmax(np.bincount(solid.ravel())[1:])))     # the cable proper
    square = np.ones((3, 3), np.uint8)
    grey = np.where(mo.erode_np(body, square), 150.0, 70.0)
    ys, xs = np.nonzero((cable != 0) & ~mo.erode_np(cable, square))           # edge pixels of the mask
    y = np.arange(H)[:, None]; x = np.arange(W)[None, :]
    pepper = np.where(r.random((H, W)) < 0.15, r.integers(0, 2, (H, W)) * 255.0, -1.0)    # salt and pepper where >= 0
    n = max(60, (H * W) // 1000)
    for k, rad, vertical in zip(r.integers(0, len(ys), n), r.uniform(2.0, 9.0, n), r.random(n) < 0.5):
        y0, y1, x0, x1 = max(ys[k] - 9, 0), min(ys[k] + 10, H), max(xs[k] - 9, 0), min(xs[k] + 10, W)
        yy, xx = y[y0:y1], x[:, x0:x1]
        blob = ((yy - ys[k]) ** 2 + (xx - xs[k]) ** 2) <= rad * rad
        stripes = (((xx if vertical else yy) // 2) % 2) * 255.0 * np.ones(blob.shape)
        grey[y0:y1, x0:x1] = np.where(blob, np.where(pepper[y0:y1, x0:x1] >= 0, pepper[y0:y1, x0:x1], stripes), grey[y0:y1, x0:x1])
    grey = grey + r.normal(0.0, 3.0, (H, W)) * (noise_sigma / 3.0)
    return np.clip(np.rint(grey), 0, 255).astype(np.uint8), cable


# (height, width) of the rectangles of make_crafted_burr_case: families that straddle each clause of the component loop
# with the reference's default config (30 <= area <= 800, aspect < 5, sides > 3) after close E3 and open E2 (which
# keep a rectangle's box and cost it a pixel or a few).
CRAFTED_RECTS = [(12, 3), (12, 4), (12, 5), (3, 12), (4, 12), (5, 12),                            # side
                 (33, 7), (34, 7), (35, 7), (36, 7), (7, 34), (7, 35), (7, 36),                   # aspect
                 (4, 4), (4, 5), (5, 5), (5, 6), (6, 5), (4, 7), (4, 8), (5, 7), (6, 6),          # area, low end (20 and 30)
                 (28, 28), (28, 29), (29, 28), (29, 29), (20, 40), (20, 41), (32, 32), (33, 33)]  # area, high end (800 and 1000)


def make_crafted_burr_case(H=224, W=320, return_boxes=False):
    """(edges uint8 0/255 [H,W], cable uint8 0/1 [H,W]) for the tail of detect_burrs_on_cable: solid rectangles
    (CRAFTED_RECTS, laid out in rows with at least 6 px between them, each starting one column right of a stripe) in
    place of the Canny output, and a cable of 1-px vertical stripes every 8 px, whose band (dilate with ELLIPSE (8,8),
    minus the cable) covers everything between the stripes.  return_boxes adds the (y, x, h, w) of every rectangle."""
    boxes = []
    edges = np.zeros((H, W), np.uint8)
    cable = np.zeros((H, W), np.uint8)
    cable[:, 0::8] = 1
    x = 9; y = 6; row_h = 0
    for h, w in CRAFTED_RECTS:
        if x + w + 6 > W:
            x = 9; y += row_h + 6; row_h = 0
        assert y + h + 6 <= H, "make_crafted_burr_case: the rectangles do not fit"
        edges[y:y + h, x:x + w] = 255
        boxes.append((y, x, h, w))
        row_h = max(row_h, h)
        x += (w + 6 + 7) // 8 * 8
    return (edges, cable, boxes) if return_boxes else (edges, cable)


def make_hysteresis_adversaries(tile_h=32, tile_w=128):
    """Grey images for canny(low=50, high=150) without blur on which a wrong hysteresis of a tiled kernel shows, as
    {name: uint8 [H,W]} with H = 2 tile_h + 8, W = 3 tile_w + 16.  A step of 20 grey levels gives |dx| + |dy| = 80 (weak).
      serpentine_seeded    the outline of one serpentine-shaped region winding through every tile, weak everywhere but
                           for one bright pixel at its upper left end: all of it is an edge
      serpentine_unseeded  the same without the bright pixel: nothing is an edge
      diagonal_pair        two rectangles whose weak outlines come within one pixel of each other diagonally (not
                           8-connected); only the first is seeded"""
    H, W = 2 * tile_h + 8, 3 * tile_w + 16
    base = np.full((H, W), 100, np.uint8)
    region = np.zeros((H, W), bool)
    rows = list(range(4, H - 10, 12))
    for k, y in enumerate(rows):
        region[y:y + 6, 4:W - 4] = True                       # bars 6 px thick, 6 px apart
        if k + 1 < len(rows):                                  # joined alternately at the right and the left end
            x = W - 10 if k % 2 == 0 else 4
            region[y:y + 18, x:x + 6] = True
    out = {}
    s = base.copy(); s[region] = 120
    out["serpentine_unseeded"] = s
    s = s.copy(); s[rows[0] + 2, 5] = 255
    out["serpentine_seeded"] = s
    d = base.copy()
    d[tile_h - 21:tile_h - 1, tile_w - 31:tile_w - 1] = 120   # its outline ends at (tile_h - 2, tile_w - 2) ...
    d[tile_h:tile_h + 20, tile_w:tile_w + 30] = 120           # ... and this one's starts at (tile_h, tile_w), across the tile corner
    d[tile_h - 11, tile_w - 30] = 255
    out["diagonal_pair"] = d
    return out


def make_direction_cases(size=40):
    """uint8 [16,size,size]: one soft edge per frame whose gradient (dx, dy) lies on either side of tan 22.5 deg
    (|dy| / |dx| = 1/3 and 1/2) and of tan 67.5 deg (3 and 2), in all four sign combinations: the three branches of
    Canny's direction test and both diagonals."""
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    frames = []
    for a, b in ((3, 1), (2, 1), (1, 3), (1, 2)):
        for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            n = math.hypot(a, b)
            d = (sa * a * (x - size / 2) + sb * b * (y - size / 2)) / n          # signed distance from a line through the centre
            frames.append(np.clip(np.rint(128 + 100 * np.tanh(d / 2.5)), 0, 255).astype(np.uint8))
    return np.stack(frames)


# ---- the multi-scale and the DoG detector ----------------------------------------------------------------------------
#   detect_burrs_enhanced      infer_enhanced_burr.py:69-138
#   get_burr_mask_dog, has_burr   src/refactor/burr_detector.py:69-133
# Device entries: unetpp_edges_union_u8, unetpp_dog_band_u8, unetpp_count_nonzero_u8 (include/unetpp.h).  The fixtures
# (scripts/make_golden_burr_enhanced.py) pin the composition on the reference's code as above; cv2's own Sobel and blur
# stay unpinned.

SOBEL_S_MAX = 2 * 1020 * 1020   # the largest dx^2 + dy^2 of a uint8 image


def sobel_xy_np(gray):
    """(dx, dy) int32 of cv2.Sobel(gray, CV_64F, 1, 0, ksize=3) and cv2.Sobel(gray, CV_64F, 0, 1, ksize=3) on the RAW
    grey image with BORDER_REFLECT_101, OpenCV's default (infer_enhanced_burr.py:93-94).  Not sobel_np: that one is the
    Sobel inside cv2.Canny, which runs on the blurred image with BORDER_REPLICATE.  The two differ on the border
    rows and columns only, where reflect-101 makes the derivative across the border exactly 0."""
    p = np.pad(_check_gray(gray).astype(np.int32), 1, mode="reflect")
    a, b, c = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    d, f = p[1:-1, :-2], p[1:-1, 2:]
    g, h, k = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    return (c + 2 * f + k) - (a + 2 * d + g), (g + 2 * h + k) - (a + 2 * b + c)


def _u8_threshold(threshold):
    """cv2.threshold on a uint8 image compares against floor(thresh); below 0 everything passes, from 255 on nothing."""
    t = float(threshold)
    if t != t:
        raise ValueError("the threshold must be a number")
    return int(math.floor(min(max(t, -1.0), 255.0)))


def _sobel_level(s, root_max):
    """np.uint8(np.sqrt(s) / np.sqrt(s.max()) * 255) for one s, in float64, truncating (infer_enhanced_burr.py:95-96)."""
    return int(np.sqrt(np.float64(s)) / root_max * np.float64(255.0))


def sobel_s_threshold(smax, threshold=50):
    """The smallest integer s in [0, smax] with uint8(sqrt(s) / sqrt(smax) * 255) > threshold, smax + 1 where no s
    passes.  sqrt, the division and the product are monotone in float64, so `s >= sobel_s_threshold(smax, t)` is the
    per-pixel test of sobel_edges_np exactly.  Found as the device finds it: from the estimate ((t + 1) / 255)^2 smax,
    walking down while the value below still passes and up while the value itself fails, each probe evaluating the
    reference's own float64 expression.  smax == 0 (0 / 0 in the reference): 1, no s passes."""
    smax, thr = int(smax), _u8_threshold(threshold)
    if smax <= 0:
        return 1
    if thr < 0:
        return 0
    root_max = np.sqrt(np.float64(smax))
    passes = lambda s: _sobel_level(s, root_max) > thr
    k = np.float64(thr + 1) / np.float64(255.0)
    c = int(min(max(np.floor(k * k * np.float64(smax)), 0.0), float(smax)))
    if passes(c):
        while c > 0 and passes(c - 1):
            c -= 1
    else:
        while c <= smax and not passes(c):
            c += 1
    return c


def sobel_edges_np(gray, threshold=50):
    """edges_sobel of infer_enhanced_burr.py:93-97: s = dx^2 + dy^2 (an exact integer, <= 2 * 1020^2),
    v = np.uint8(np.sqrt(s) / np.sqrt(s.max()) * 255) in float64, truncating; 255 where v > threshold.
    The one stated departure: a frame with s.max() == 0 (a constant image) is 0 / 0 in the reference, whose uint8 cast
    of NaN is undefined; here it has no Sobel edges."""
    dx, dy = sobel_xy_np(gray)
    s = (dx.astype(np.int64) ** 2 + dy.astype(np.int64) ** 2).astype(np.float64)
    if s.max() == 0:
        return np.zeros(s.shape, np.uint8)
    v = (np.sqrt(s) / np.sqrt(s.max()) * 255).astype(np.uint8)
    return np.where(v > _u8_threshold(threshold), np.uint8(255), np.uint8(0)).astype(np.uint8)


def laplacian_edges_np(gray, threshold=15):
    """edges_laplacian of infer_enhanced_burr.py:100-102: laplacian_abs_u8_np (the `& 255` wrap of the reference's
    uint8 cast, reproduced and not corrected) above the threshold, 0 / 255."""
    return np.where(laplacian_abs_u8_np(gray) > _u8_threshold(threshold), np.uint8(255), np.uint8(0)).astype(np.uint8)


def edges_combined_np(gray, canny_edges, sobel_threshold=50, laplacian_threshold=15):
    """edges_combined of infer_enhanced_burr.py:105-106: canny_edges | Sobel edges | Laplacian edges, bytewise.  What
    NestedUNet.edges_combined computes for one frame given its Canny image."""
    c = _check_gray(canny_edges)
    if c.shape != np.asarray(gray).shape:
        raise ValueError(f"gray {np.asarray(gray).shape} and canny_edges {c.shape} differ in shape")
    return c | sobel_edges_np(gray, sobel_threshold) | laplacian_edges_np(gray, laplacian_threshold)


def detect_burrs_enhanced_np(gray, mask_cable, match_class=-1, *, min_area=50, max_area=500, band_ksize=25, blur_ksize=5,
                             blur_sigma=1.0, taps=None, canny_low=30, canny_high=100, sobel_threshold=50, laplacian_threshold=15,
                             close_ksize=5, open_ksize=3, max_aspect=6.0, min_side=4, out_value=1):
    """What NestedUNet.detect_burrs_enhanced computes for one frame: detect_burrs_enhanced(gray, mask_cable,
    {"min_area": .., "max_area": ..}) (infer_enhanced_burr.py:69-138) with the function's constants as defaults.  The
    reference's `width >= 5 and height >= 5` is keep_box's strict `> min_side` with min_side = 4: the same test on
    integers.  An empty cable gives an empty band: the two early returns."""
    t = resolve_taps(blur_ksize, blur_sigma, taps)
    blurred = _check_gray(gray) if t is None else gaussian_blur_np(gray, t)
    edges = edges_combined_np(gray, canny_np(blurred, canny_low, canny_high), sobel_threshold, laplacian_threshold)
    return burrs_from_edges_np(edges, mask_cable, match_class, min_area=min_area, max_area=max_area, band_ksize=band_ksize,
                               close_ksize=close_ksize, open_ksize=open_ksize, max_aspect=max_aspect, min_side=min_side,
                               out_value=out_value)


def resolve_dog_taps(taps1=None, taps2=None):
    """The two kernels of get_burr_mask_dog: gaussian_taps(3, 1.0) and gaussian_taps(7, 2.0) unless given."""
    return (check_taps(gaussian_taps(3, 1.0) if taps1 is None else taps1),
            check_taps(gaussian_taps(7, 2.0) if taps2 is None else taps2))


def dog_u8_np(gray, taps1=None, taps2=None):
    """cv2.subtract(blur1, blur2) of src/refactor/burr_detector.py:94-97 on uint8: the subtraction saturates at 0 and
    never wraps, so the reference's np.abs after it changes nothing and only the positive lobe of the difference of
    Gaussians survives.  Reproduced, not corrected."""
    t1, t2 = resolve_dog_taps(taps1, taps2)
    d = gaussian_blur_np(gray, t1).astype(np.int32) - gaussian_blur_np(gray, t2).astype(np.int32)
    return np.clip(d, 0, 255).astype(np.uint8)


def burr_mask_dog_np(gray, mask_cable, match_class=-1, *, band_out=10, threshold=30, min_area=20, max_area=500, taps1=None,
                     taps2=None, out_value=255):
    """What NestedUNet.burr_mask_dog computes for one frame: get_burr_mask_dog(gray, mask_cable, BurrConfig(band_out,
    laplacian_threshold=threshold, min_area, max_area)) (src/refactor/burr_detector.py:69-118)."""
    el, steps, res = mo.program_band(band_out)
    band = mo.run_program_np(mask_cable, None, el, steps, match_class, -1, res, 1)
    hot = ((band != 0) & (dog_u8_np(gray, taps1, taps2) > _u8_threshold(threshold))).astype(np.uint8)
    return filter_box_np(hot, -1, min_area, max_area, math.inf, 0, out_value)


def has_burr_np(mask, min_total_area=50):
    """has_burr of src/refactor/burr_detector.py:121-133: np.sum(mask > 0) >= min_total_area."""
    return bool(int(np.count_nonzero(np.asarray(mask))) >= min_total_area)


# (height, width) of the rectangles of make_crafted_enhanced_case: pairs that straddle each clause of
# infer_enhanced_burr.py:131-135 with the config 50 / 500 after close E5 (which leaves a rectangle alone) and open E3
# (a cross: it keeps the box and costs the four corner pixels, so the area is h w - 4).
CRAFTED_ENHANCED_RECTS = [(14, 4), (14, 5), (4, 14), (5, 14),                       # w < 5, h < 5
                          (6, 9), (6, 8), (7, 8), (7, 7), (9, 6),                   # area, low end: 50 kept, 44 and 45 not
                          (24, 21), (25, 21), (22, 22), (23, 22),                   # area, high end: 500 and 480 kept, 521 and 502 not
                          (30, 5), (31, 5), (36, 7), (43, 7)]                       # aspect: 5.999.. kept, 6.2 not; 5.14, 6.14


def make_crafted_enhanced_case(H=200, W=336, return_boxes=False):
    """(grey uint8 [H,W], edges uint8 0/255 [H,W], cable uint8 0/1 [H,W]) for the tail of detect_burrs_enhanced: solid
    rectangles (CRAFTED_ENHANCED_RECTS, one in every other 24-px cell, each starting one column right of a stripe) in
    place of the Canny output, and a cable of 1-px vertical stripes every 24 px over the columns below W - 48, whose band
    (dilate with ELLIPSE (25,25), minus the cable) covers everything between and 12 px beyond them.  The grey image is
    flat but for one bright square at least 14 px from every cable pixel: it is not constant (that is the 0 / 0 frame),
    and neither its Sobel nor its Laplacian response reaches the band."""
    boxes = []
    edges = np.zeros((H, W), np.uint8)
    cable = np.zeros((H, W), np.uint8)
    last = (W - 48) // 24 * 24
    cable[:, 0:last + 1:24] = 1
    x = 25; y = 6; row_h = 0                                # not the cell on the image border: a close grows into the border
    for h, w in CRAFTED_ENHANCED_RECTS:
        if x + w + 1 > last:
            x = 25; y += row_h + 6; row_h = 0
        assert y + h + 6 <= H and w <= 22, "make_crafted_enhanced_case: the rectangles do not fit"
        edges[y:y + h, x:x + w] = 255
        boxes.append((y, x, h, w))
        row_h = max(row_h, h)
        x += 48
    grey = np.full((H, W), 100, np.uint8)
    x0 = last + 12 + 14 + 2
    assert x0 + 6 <= W - 2
    grey[H // 2 - 3:H // 2 + 3, x0:x0 + 6] = 180
    return (grey, edges, cable, boxes) if return_boxes else (grey, edges, cable)
