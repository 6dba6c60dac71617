"""Raw camera frames: the Bayer demosaic of GigECameraHarvester._to_bgr (src/camera/gige_harvester.py:101-114), in NumPy
(torch-free) and on the device (include/unetpp_raw.h; csrc/raw_frames.h), and the same demosaic fused into the resize of
preprocess_image (infer_two_stage_burr.py:122-127), so that the full-size BGR frame is never written.
  _to_bgr :101-114                                   -> to_bgr_np / to_bgr
  cv2.cvtColor(img, COLOR_BAYER_xx2BGR)              -> demosaic_np
  stage 2's cv2.cvtColor(frame, COLOR_BGR2GRAY)      -> gray_np / to_gray
  read :116-129 followed by preprocess_image's resize -> raw_resize_np / resize
Every device function takes the model and has its NumPy form here; the device results equal them bit for bit (all integer).
The whole loop is frame_loop.process_raw_frames.

The arithmetic is OpenCV's published bilinear Bayer2RGB_<uchar>.  Interior pixels (1 <= y <= H - 2, 1 <= x <= W - 2): a channel
measured at the pixel is the raw byte; at a red or blue site green is (N + S + W + E + 2) >> 2 and the opposite colour
(NW + NE + SW + SE + 2) >> 2; at a green site red and blue are (a + b + 1) >> 1 of their two neighbours, which lie horizontally
for the colour that shares the row and vertically for the other.  Border: out[y, x] = interior[clamp(y, 1, H - 2),
clamp(x, 1, W - 2)] (OpenCV copies column 1 into column 0, column W - 2 into column W - 1, then rows likewise), so H, W >= 3.

Patterns carry OpenCV's names: a pattern is named by the components in the second row, second and third columns.  By
(row parity, column parity) of the red and the blue site: BG red (0,0) blue (1,1) [RGGB]; GB red (0,1) blue (1,0) [GRBG];
RG red (1,1) blue (0,0) [BGGR]; GR red (1,0) blue (0,1) [GBRG].  MONO gives (v, v, v) and has no border rule.

GenICam's BayerRG8 means R at (0,0), which is OpenCV's BG: the reference maps "BayerRG" to COLOR_BAYER_RG2BGR and so swaps red
and blue on such a camera.  pattern_of follows the reference for the string form; pattern= takes any of the five by name.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from . import edges as ed
from . import tiling as tl

PATTERNS = _lib.RAW_PATTERNS                                           # name -> UNETPP_RAW_*
RED_SITE = {"BG": (0, 0), "GB": (0, 1), "RG": (1, 1), "GR": (1, 0)}    # (row parity, column parity); blue is the opposite corner
MIN_SIDE = 3


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _check_pattern(pattern):
    if pattern not in PATTERNS:
        raise ValueError(f"pattern must be one of {sorted(PATTERNS)}, got {pattern!r}")
    return pattern


def _check_shape(h, w, pattern):
    low = 1 if pattern == "MONO" else MIN_SIDE
    if h < low or w < low:
        raise ValueError(f"raw frames of {h}x{w}: pattern {pattern} needs H, W >= {low}")


def pattern_of(pixel_format):
    """The dispatch of _to_bgr (:105-113) on the camera's PixelFormat string: "BayerRG" in it -> RG, else "BayerBG" -> BG, else
    grey -- BayerGR8, BayerGB8 and unknown names included, which the reference treats as mono."""
    if not isinstance(pixel_format, str):
        raise ValueError(f"pixel_format must be a string, got {pixel_format!r}")
    if "BayerRG" in pixel_format:
        return "RG"
    if "BayerBG" in pixel_format:
        return "BG"
    return "MONO"


def _pattern_arg(pixel_format, pattern):
    if (pixel_format is None) == (pattern is None):
        raise ValueError("give pixel_format (the camera's string) or pattern= (one of BG, GB, RG, GR, MONO), not both")
    return _check_pattern(pattern) if pattern is not None else pattern_of(pixel_format)


def _check_roi(roi_xywh, h, w):
    x0, y0, cw, ch = (0, 0, w, h) if roi_xywh is None else (int(v) for v in roi_xywh)
    if x0 < 0 or y0 < 0 or cw < 1 or ch < 1 or x0 + cw > w or y0 + ch > h:
        raise ValueError(f"roi (x, y, w, h) = {(x0, y0, cw, ch)} does not lie inside the {h}x{w} frame")
    return x0, y0, cw, ch


def _check_size(size_hw):
    oh, ow = int(size_hw[0]), int(size_hw[1])
    if oh < 1 or ow < 1:
        raise ValueError(f"size_hw must be positive, got {size_hw!r}")
    return oh, ow


# ---- the NumPy forms ---------------------------------------------------------------------------------------------------------------
def demosaic_np(raw, pattern):
    """cv2.cvtColor(raw, COLOR_BAYER_<pattern>2BGR) for uint8 [H,W] or [B,H,W]: uint8 [..,H,W,3] BGR (module docstring)."""
    _check_pattern(pattern)
    raw = np.asarray(raw)
    if raw.dtype != np.uint8 or raw.ndim not in (2, 3):
        raise ValueError(f"raw must be uint8 [H,W] or [B,H,W], got {raw.dtype} {list(raw.shape)}")
    h, w = raw.shape[-2:]
    _check_shape(h, w, pattern)
    if pattern == "MONO":
        return np.ascontiguousarray(np.repeat(raw[..., None], 3, axis=-1))
    v = raw.astype(np.int32)
    c = v[..., 1:-1, 1:-1]
    n, s, we, e = v[..., :-2, 1:-1], v[..., 2:, 1:-1], v[..., 1:-1, :-2], v[..., 1:-1, 2:]
    cross = (n + s + we + e + 2) >> 2
    diag = (v[..., :-2, :-2] + v[..., :-2, 2:] + v[..., 2:, :-2] + v[..., 2:, 2:] + 2) >> 2
    hor, ver = (we + e + 1) >> 1, (n + s + 1) >> 1
    ry, rx = RED_SITE[pattern]
    yy, xx = np.mgrid[1:h - 1, 1:w - 1]
    red_row, red_col = (yy & 1) == ry, (xx & 1) == rx                 # the row holds red sites; the column does
    site = red_row == red_col                                         # a red or a blue site, else a green one
    g = np.where(site, cross, c)
    r = np.where(site, np.where(red_row, c, diag), np.where(red_row, hor, ver))
    b = np.where(site, np.where(red_row, diag, c), np.where(red_row, ver, hor))
    inner = np.stack([b, g, r], axis=-1).astype(np.uint8)
    ys, xs = np.clip(np.arange(h), 1, h - 2) - 1, np.clip(np.arange(w), 1, w - 2) - 1
    return np.ascontiguousarray(inner[..., ys[:, None], xs[None, :], :])


def to_bgr_np(buffer, pixel_format, width, height):
    """_to_bgr (:101-114): the buffer reshaped to [height, width], then the demosaic pattern_of(pixel_format) names."""
    img = np.asarray(buffer).reshape(int(height), int(width))
    return demosaic_np(img, pattern_of(pixel_format))


def gray_np(raw, pattern):
    """cv2.cvtColor(demosaiced, COLOR_BGR2GRAY): what stage 2 reads.  The identity for MONO."""
    return ed.bgr_to_gray_np(demosaic_np(raw, pattern))


def raw_resize_np(raw, pattern, roi_xywh, size_hw):
    """uint8 [..,oh,ow,3]: the crop roi_xywh = (x0, y0, cw, ch) of the demosaiced frame (None: all of it), then
    cv2.resize(INTER_LINEAR) as tiling.resize_linear_u8_np states it.  The demosaic's phase comes from the frame's coordinates:
    an odd x0 or y0 does not shift the pattern."""
    raw = np.asarray(raw)
    bgr = demosaic_np(raw, pattern)
    h, w = raw.shape[-2:]
    x0, y0, cw, ch = _check_roi(roi_xywh, h, w)
    oh, ow = _check_size(size_hw)
    crop = bgr[..., y0:y0 + ch, x0:x0 + cw, :]
    if raw.ndim == 2:
        return tl.resize_linear_u8_np(crop, (ow, oh))
    return np.stack([tl.resize_linear_u8_np(f, (ow, oh)) for f in crop])


def correlation_form_np(raw, pattern):
    """The interior of demosaic_np a second way, for the tests: with P_c the raw plane with every site that does not measure c
    set to zero, red and blue are (correlate(P_c, [[1,2,1],[2,4,2],[1,2,1]]) + 2) >> 2 and green is
    (correlate(P_g, [[0,1,0],[1,4,1],[0,1,0]]) + 2) >> 2.  uint8 [H-2,W-2,3] BGR for uint8 [H,W]."""
    raw = np.asarray(raw)
    h, w = raw.shape
    ry, rx = RED_SITE[_check_pattern(pattern)]
    yy, xx = np.mgrid[0:h, 0:w]
    is_r = ((yy & 1) == ry) & ((xx & 1) == rx)
    is_b = ((yy & 1) != ry) & ((xx & 1) != rx)
    box = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]])
    plus = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]])

    def corr(mask, k):
        p = np.where(mask, raw, 0).astype(np.int64)
        acc = np.zeros((h - 2, w - 2), np.int64)
        for dy in range(3):
            for dx in range(3):
                acc += k[dy, dx] * p[dy:dy + h - 2, dx:dx + w - 2]
        return (acc + 2) >> 2
    return np.stack([corr(is_b, box), corr(~(is_r | is_b), plus), corr(is_r, box)], axis=-1).astype(np.uint8)


# ---- seeded inputs of the fixture and the tests --------------------------------------------------------------------------------------
FIXTURE_FORMATS = ("BayerRG8", "BayerBG8", "Mono8", "BayerGR8", "NoSuchFormat12")
FIXTURE_SHAPES = ((12, 10), (33, 17), (64, 48))                       # (height, width)


def make_raw(b, h, w, seed):
    """uint8 [b,h,w]: a smooth scene with an edge under a colour-filter mosaic of unequal gains, plus noise and a few 0 / 255."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((b, h, w), np.uint8)
    for i in range(b):
        scene = 120 + 70 * np.sin(x / (3.0 + i)) * np.cos(y / 4.0) + 50 * ((x + 2 * y) // 9 % 2)
        gain = np.array([[1.0, 0.7], [0.8, 0.45]])[y & 1, x & 1]
        v = np.clip(scene * gain + r.normal(0, 5, (h, w)), 0, 255).astype(np.uint8)
        flat = v.reshape(-1)
        flat[r.integers(0, flat.size, 4)] = 255
        flat[r.integers(0, flat.size, 4)] = 0
        out[i] = v
    return out


# ---- the device path (torch imported lazily, as in simple_loops.py) ---------------------------------------------------------------------
def _raw(model, raw):
    """(tensor, b, h, w, row stride, frame stride in bytes).  A raw tensor whose pixels are consecutive and whose rows and frames
    do not overlap is read in place, so a padded GenTL line is passed through; any other layout is copied."""
    import torch
    if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dtype == torch.uint8 and raw.dim() == 3):
        raise RuntimeError("raw must be a uint8 CUDA tensor [B,H,W]")
    b, h, w = (int(v) for v in raw.shape)
    sf, sr, sp = (int(v) for v in raw.stride())
    in_place = min(b, h, w) >= 1 and (sp == 1 or w == 1) and (sr >= w or h == 1) and (b == 1 or sf >= (h - 1) * sr + w)
    if in_place:
        model._input(raw[:1, :1, :1], "raw")                         # the device checks of every module, on a view of one byte
    else:
        raw = model._input(raw, "raw")
        sf, sr = h * w, w
    if h == 1:
        sr = w
    if b == 1:
        sf = (h - 1) * sr + w
    return raw, b, h, w, sr, sf


def _to_bgr(model, raw, pattern, want_bgr, want_gray):
    import torch
    raw, b, h, w, sr, sf = _raw(model, raw)
    _check_shape(h, w, pattern)
    bgr = torch.empty((b, h, w, 3), dtype=torch.uint8, device=raw.device) if want_bgr else None
    gray = torch.empty((b, h, w), dtype=torch.uint8, device=raw.device) if want_gray else None
    model._call("unetpp_raw_to_bgr_u8", raw, sr, sf, b, h, w, PATTERNS[pattern], bgr, gray, stream_of=raw)
    return bgr, gray


def to_bgr(model, raw, pixel_format=None, *, pattern=None, want_gray=False, bgr=True):
    """demosaic_np on the device for a uint8 CUDA tensor [B,H,W], one launch: uint8 [B,H,W,3] BGR; with want_gray (bgr, gray),
    gray uint8 [B,H,W] = gray_np; with bgr=False the grey frame alone, and the BGR frame is never written.  pixel_format is the
    camera's string, read as _to_bgr reads it (pattern_of); pattern= names one of BG, GB, RG, GR, MONO instead."""
    pattern = _pattern_arg(pixel_format, pattern)
    if not bgr and not want_gray:
        raise ValueError("nothing to compute: bgr=False needs want_gray=True")
    out_bgr, out_gray = _to_bgr(model, raw, pattern, bool(bgr), bool(want_gray))
    return (out_bgr, out_gray) if bgr and want_gray else (out_bgr if bgr else out_gray)


def to_gray(model, raw, pixel_format=None, *, pattern=None):
    """gray_np on the device for a uint8 CUDA tensor [B,H,W]: uint8 [B,H,W], one launch that writes 1 B/px."""
    return _to_bgr(model, raw, _pattern_arg(pixel_format, pattern), False, True)[1]


def resize(model, raw, pattern, size_hw, roi_xywh=None):
    """raw_resize_np on the device for a uint8 CUDA tensor [B,H,W]: uint8 [B,oh,ow,3] BGR, ready for segment(), one launch from
    the raw bytes; only the taps the resize reads are demosaiced."""
    import torch
    _check_pattern(pattern)
    raw, b, h, w, sr, sf = _raw(model, raw)
    _check_shape(h, w, pattern)
    x0, y0, cw, ch = _check_roi(roi_xywh, h, w)
    oh, ow = _check_size(size_hw)
    out = torch.empty((b, oh, ow, 3), dtype=torch.uint8, device=raw.device)
    model._call("unetpp_raw_resize_u8", raw, sr, sf, b, h, w, PATTERNS[pattern], x0, y0, cw, ch, out, oh, ow, stream_of=raw)
    return out
