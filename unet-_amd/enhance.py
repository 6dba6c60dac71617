"""CPU restatement (NumPy only) of the grey-frame enhancement in front of the network (include/unetpp.h,
unetpp_gray_decision, unetpp_clahe_u8, unetpp_bilateral_u8, unetpp_enhance_u8) and of the reference functions the
NestedUNet methods restate:
  is_grayscale_frame, enhance_grayscale_frame, preprocess_frame, crop_roi      src/refactor/preprocess.py:12-113
with PreprocessConfig's defaults (src/refactor/config.py:44-52), plus the scene generator the tests and fixtures share.

The primitives are restated from OpenCV's published algorithms for 8-bit images: CLAHE_Impl::apply (clahe_np), the
scalar loop of bilateralFilter (bilateral_np), BGR2GRAY (edges.bgr_to_gray_np).  cv2 is not installed where this project
is built and tested, so cv2's own results -- in particular the summation order of its SIMD paths in the bilateral
filter -- stay unpinned, as for blur / Canny / resize; bilateral_np takes `tables=` for cv2's own
weights and tap order.  The device kernels match THIS module bit for bit: every float operation below is a float32
operation rounded on its own (no fused multiply-add), in the order written.
"""
from __future__ import annotations

import numpy as np

from . import edges as ed
from .geometry import reflect101

MAX_GRID = 16           # tiles per side of the CLAHE grid
MAX_RADIUS = 4          # of the bilateral filter (d <= 9)
MAX_SIDE = 65535
MAX_PIXELS = 1 << 30
DEFAULTS = dict(clip_limit=2.0, tile_grid=8, gamma=0.8, denoise_method="bilateral", denoise_strength=5)   # PreprocessConfig


def grid_of(tile_grid):
    """(tilesX, tilesY) of cv2.createCLAHE's tileGridSize; an int n means (n, n), PreprocessConfig.clahe_tile_size."""
    if isinstance(tile_grid, (int, np.integer)):
        return int(tile_grid), int(tile_grid)
    tx, ty = tile_grid
    return int(tx), int(ty)


def check_limits(H, W, tile_grid=None, radius=None):
    """ValueError for what the device path refuses too: 1 <= tilesX, tilesY <= 16, H > tilesY, W > tilesX,
    radius <= 4, H, W > radius, H, W <= 65535, H * W <= 2^30."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE or H * W > MAX_PIXELS:
        raise ValueError(f"image is {H}x{W}: needs 1 <= H, W <= {MAX_SIDE} and H * W <= 2^30")
    if tile_grid is not None:
        tx, ty = grid_of(tile_grid)
        if not (1 <= tx <= MAX_GRID and 1 <= ty <= MAX_GRID):
            raise ValueError(f"tile grid {tx}x{ty}: 1 <= tilesX, tilesY <= {MAX_GRID}")
        if H <= ty or W <= tx:
            raise ValueError(f"image is {H}x{W}: needs H > tilesY = {ty} and W > tilesX = {tx}")
    if radius is not None:
        if not 1 <= int(radius) <= MAX_RADIUS:
            raise ValueError(f"bilateral radius {radius}: 1 <= radius <= {MAX_RADIUS} (d <= {2 * MAX_RADIUS + 1})")
        if H <= radius or W <= radius:
            raise ValueError(f"image is {H}x{W}: needs H, W > radius = {radius}")


def _u8_image(a, what="gray"):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f"{what} must be uint8 [H,W], got {a.dtype} {a.shape}")
    return a


# ---- the grey / colour decision ------------------------------------------------------------------------------------------
def channel_diff_sums(frame_bgr):
    """The three sums of |b - g|, |g - r|, |r - b| over a uint8 [H,W,3] frame as exact Python integers."""
    f = np.asarray(frame_bgr)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError(f"frame must be uint8 [H,W,3], got {f.dtype} {f.shape}")
    b, g, r = (f[..., c].astype(np.int64) for c in range(3))
    return int(np.abs(b - g).sum()), int(np.abs(g - r).sum()), int(np.abs(r - b).sum())


def is_grayscale_np(frame_bgr, threshold=10.0):
    """is_grayscale_frame (preprocess.py:12-32): max(sums) / N < threshold, one float64 division of exact integers --
    what np.abs(...).mean() yields while the sum is exact in a double (N < 2^53 / 255; here N <= 2^30).  A frame that is
    not [H,W,3] counts as grey."""
    f = np.asarray(frame_bgr)
    if f.ndim != 3 or f.shape[2] != 3:
        return True
    n = f.shape[0] * f.shape[1]
    return bool(float(max(channel_diff_sums(f))) / float(n) < float(threshold))


def make_boundary_frame(H, W, total):
    """A uint8 [H,W,3] frame whose largest channel-difference sum is exactly `total` (0 <= total <= 200 H W): g = r = 20,
    b = 20 + d with the d's summing to `total`, spread as evenly as integers allow."""
    n = H * W
    total = int(total)
    if not 0 <= total <= 200 * n:
        raise ValueError(f"total {total} not in [0, {200 * n}]")
    d = np.full(n, total // n, np.int64)
    d[:total - (total // n) * n] += 1
    f = np.full((H, W, 3), 20, np.uint8)
    f[..., 0] = (20 + d).reshape(H, W).astype(np.uint8)
    return f


# ---- CLAHE -------------------------------------------------------------------------------------------------------------------
def clahe_geometry(H, W, tile_grid=(8, 8)):
    """(tilesX, tilesY, tw, th, pad_x, pad_y) of CLAHE_Impl::apply.  When BOTH W % tilesX == 0 and H % tilesY == 0 the
    histograms come from the image itself; otherwise from the image extended with BORDER_REFLECT_101 by
    tilesY - H % tilesY rows at the bottom and tilesX - W % tilesX columns on the right -- so a dimension that IS
    divisible still gets a whole extra `tiles` rows or columns when the other one is not (64 x 90 on an 8 x 8 grid: 72
    rows, tile height 9).  OpenCV's quirk, kept."""
    tx, ty = grid_of(tile_grid)
    check_limits(H, W, (tx, ty))
    if W % tx == 0 and H % ty == 0:
        px = py = 0
    else:
        px, py = tx - W % tx, ty - H % ty
    return tx, ty, (W + px) // tx, (H + py) // ty, px, py


def clahe_clip(clip_limit, tile_area):
    """The integer clip of a bin: max(int(clip_limit * tileArea / 256), 1) for clip_limit > 0 (in double), else 0 = none."""
    return max(int(float(clip_limit) * tile_area / 256), 1) if clip_limit > 0 else 0


def clahe_luts_np(gray, clip_limit=2.0, tile_grid=(8, 8)):
    """The per-tile look-up tables, uint8 [tilesY * tilesX, 256], tile (ty, tx) at row ty * tilesX + tx.  Per tile:
    histogram of the (extended) tile; bins clipped to `clip`, the excess `clipped` redistributed: batch = clipped // 256
    to every bin, then residual = clipped - 256 batch single counts, one to every step-th bin from bin 0 with
    step = max(256 // residual, 1); lut[i] = saturate_u8(rint(float32(cumsum_i) * lutScale)), lutScale = float32(255) /
    float32(tileArea), rint half to even."""
    gray = _u8_image(gray)
    H, W = gray.shape
    tx, ty, tw, th, px, py = clahe_geometry(H, W, tile_grid)
    ext = gray[reflect101(np.arange(H + py), H)][:, reflect101(np.arange(W + px), W)]
    tiles = ext.reshape(ty, th, tx, tw).transpose(0, 2, 1, 3).reshape(ty * tx, th * tw)
    hist = np.stack([np.bincount(t, minlength=256) for t in tiles]).astype(np.int64)
    area = tw * th
    clip = clahe_clip(clip_limit, area)
    if clip > 0:
        clipped = np.maximum(hist - clip, 0).sum(axis=1)
        hist = np.minimum(hist, clip)
        batch = clipped // 256
        residual = clipped - 256 * batch
        hist = hist + batch[:, None]
        step = np.maximum(256 // np.maximum(residual, 1), 1)
        i = np.arange(256)[None, :]
        hist = hist + ((i % step[:, None] == 0) & (i // step[:, None] < residual[:, None]))
    scale = np.float32(255) / np.float32(area)
    lut = np.rint(np.cumsum(hist, axis=1).astype(np.float32) * scale)
    return np.clip(lut, 0, 255).astype(np.uint8)


def _clahe_axis(n, tile, tiles):
    """Per coordinate 0..n-1: (t1, t2, a, a1) of CLAHE_Interpolation_Body, float32."""
    inv = np.float32(1) / np.float32(tile)
    tf = np.arange(n, dtype=np.float32) * inv - np.float32(0.5)
    t1 = np.floor(tf)
    a = tf - t1
    a1 = np.float32(1) - a
    t1 = t1.astype(np.int64)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a.astype(np.float32), a1.astype(np.float32)


def clahe_interpolate_np(gray, luts, tile_grid=(8, 8)):
    """The bilinear blend of the four surrounding tiles' tables for every pixel of the ORIGINAL image, float32:
    res = (L11[v] xa1 + L12[v] xa) ya1 + (L21[v] xa1 + L22[v] xa) ya; out = saturate_u8(rint(res))."""
    gray = _u8_image(gray)
    H, W = gray.shape
    tx, ty, tw, th, _, _ = clahe_geometry(H, W, tile_grid)
    x1, x2, xa, xa1 = _clahe_axis(W, tw, tx)
    y1, y2, ya, ya1 = _clahe_axis(H, th, ty)
    L = np.asarray(luts, np.uint8).reshape(ty, tx, 256).astype(np.float32)
    v = gray.astype(np.int64)
    y1, y2, ya, ya1 = y1[:, None], y2[:, None], ya[:, None], ya1[:, None]
    x1, x2, xa, xa1 = x1[None, :], x2[None, :], xa[None, :], xa1[None, :]
    top = L[y1, x1, v] * xa1 + L[y1, x2, v] * xa
    bot = L[y2, x1, v] * xa1 + L[y2, x2, v] * xa
    res = top * ya1 + bot * ya
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe_np(gray, clip_limit=2.0, tile_grid=(8, 8), return_luts=False):
    """cv2.createCLAHE(clip_limit, tile_grid).apply(gray) for uint8 [H,W] as OpenCV's CLAHE_Impl::apply computes it
    (clahe_geometry, clahe_luts_np, clahe_interpolate_np); cv2's own result is unpinned (module docstring)."""
    luts = clahe_luts_np(gray, clip_limit, tile_grid)
    out = clahe_interpolate_np(gray, luts, tile_grid)
    return (out, luts) if return_luts else out


# ---- gamma -------------------------------------------------------------------------------------------------------------------
def gamma_table(gamma):
    """The look-up table of enhance_grayscale_frame (preprocess.py:60-62): (i / 255) ^ (1 / gamma) * 255 in Python
    floats, truncated to uint8; None for gamma == 1.0 (the reference skips the step)."""
    gamma = float(gamma)
    if gamma == 1.0:
        return None
    if not gamma > 0:
        raise ValueError(f"gamma must be positive, got {gamma!r}")
    inv = 1.0 / gamma
    return np.array([((i / 255.0) ** inv) * 255 for i in range(256)], np.float64).astype(np.uint8)


# ---- bilateral filter ------------------------------------------------------------------------------------------------------
def bilateral_tables(d=5, sigma_color=75.0, sigma_space=75.0):
    """(radius, color_w float32 [256], space_w float32 [n], dy int32 [n], dx int32 [n]) of cv2.bilateralFilter's 8-bit
    path: radius = d // 2 for d > 0 else round(1.5 sigma_space), at least 1; color_w[i] = float32(exp(i i (-0.5 /
    sigma_color^2))); the taps are the offsets (dy, dx), dy outer and dx inner from -radius to radius, with
    sqrt(dy^2 + dx^2) <= radius, space_w = float32(exp(r^2 (-0.5 / sigma_space^2))).  A sigma <= 0 counts as 1.
    d = 3, 5, 9 give 5, 13, 49 taps."""
    sc = float(sigma_color) if sigma_color > 0 else 1.0
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    radius = int(d) // 2 if int(d) > 0 else int(round(ss * 1.5))
    radius = max(radius, 1)
    if radius > MAX_RADIUS:
        raise ValueError(f"bilateral radius {radius}: 1 <= radius <= {MAX_RADIUS} (d <= {2 * MAX_RADIUS + 1})")
    gc, gs = -0.5 / (sc * sc), -0.5 / (ss * ss)
    i = np.arange(256, dtype=np.float64)
    color_w = np.exp(i * i * gc).astype(np.float32)
    dy, dx, sw = [], [], []
    for a in range(-radius, radius + 1):
        for b in range(-radius, radius + 1):
            r = np.sqrt(float(a) * a + float(b) * b)
            if r > radius:
                continue
            dy.append(a); dx.append(b); sw.append(np.exp(r * r * gs))
    return radius, color_w, np.asarray(sw, np.float64).astype(np.float32), np.asarray(dy, np.int32), np.asarray(dx, np.int32)


def check_tables(tables):
    """`tables` as bilateral_tables returns them, checked: float32 / int32 C-contiguous arrays, 1 <= n <= (2 radius + 1)^2
    taps, every offset within the radius, finite non-negative weights and a positive weight on some tap for every
    colour distance that can meet it (the centre tap with color_w[0] > 0 suffices: wsum > 0)."""
    radius, color_w, space_w, dy, dx = tables
    radius = int(radius)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"bilateral radius {radius}: 1 <= radius <= {MAX_RADIUS} (d <= {2 * MAX_RADIUS + 1})")
    color_w = np.ascontiguousarray(np.asarray(color_w, np.float32).reshape(-1))
    space_w = np.ascontiguousarray(np.asarray(space_w, np.float32).reshape(-1))
    dy = np.ascontiguousarray(np.asarray(dy, np.int32).reshape(-1))
    dx = np.ascontiguousarray(np.asarray(dx, np.int32).reshape(-1))
    n = len(space_w)
    if len(color_w) != 256 or not 1 <= n <= (2 * radius + 1) ** 2 or len(dy) != n or len(dx) != n:
        raise ValueError(f"bilateral tables: 256 colour weights and 1..{(2 * radius + 1) ** 2} taps, got {len(color_w)} and {n}")
    if np.abs(dy).max() > radius or np.abs(dx).max() > radius:
        raise ValueError(f"bilateral tables: a tap lies outside the radius {radius}")
    if not (np.isfinite(color_w).all() and np.isfinite(space_w).all() and (color_w >= 0).all() and (space_w >= 0).all()):
        raise ValueError("bilateral tables: weights must be finite and non-negative")
    centre = (dy == 0) & (dx == 0)
    if not (color_w[0] > 0 and centre.any() and (space_w[centre] > 0).any()):
        raise ValueError("bilateral tables: the centre tap must carry a positive weight (the weight sum divides)")
    return radius, color_w, space_w, dy, dx


def bilateral_np(gray, d=5, sigma_color=75.0, sigma_space=75.0, tables=None):
    """cv2.bilateralFilter(gray, d, sigma_color, sigma_space) for uint8 [H,W] with BORDER_REFLECT_101, as OpenCV's scalar
    8-bit loop computes it: per pixel, over the taps in table order, float32 without contraction,
      w = space_w[k] * color_w[|val - val0|];  sum += val * w;  wsum += w;   out = rint(sum / wsum).
    tables: bilateral_tables' tuple, e.g. with cv2's own weights or tap order (cv2's result is unpinned)."""
    gray = _u8_image(gray)
    radius, color_w, space_w, dy, dx = check_tables(bilateral_tables(d, sigma_color, sigma_space) if tables is None else tables)
    H, W = gray.shape
    check_limits(H, W, None, radius)
    pad = gray[reflect101(np.arange(-radius, H + radius), H)][:, reflect101(np.arange(-radius, W + radius), W)].astype(np.int32)
    val0 = pad[radius:radius + H, radius:radius + W]
    s = np.zeros((H, W), np.float32)
    ws = np.zeros((H, W), np.float32)
    for k in range(len(space_w)):
        val = pad[radius + dy[k]:radius + dy[k] + H, radius + dx[k]:radius + dx[k] + W]
        w = space_w[k] * color_w[np.abs(val - val0)]
        s = s + val.astype(np.float32) * w
        ws = ws + w
    assert s.dtype == np.float32 and ws.dtype == np.float32
    return np.clip(np.rint(s / ws), 0, 255).astype(np.uint8)


def denoise_tables(denoise_method, denoise_strength):
    """The bilateral tables of enhance_grayscale_frame's denoising step (preprocess.py:65-69), or None for no filter:
    'bilateral' is cv2.bilateralFilter(img, denoise_strength, 75, 75); any other string does nothing, as in the
    reference; 'fastNlMeans' is not restated here (ValueError)."""
    if denoise_method == "fastNlMeans":
        raise ValueError("denoise_method 'fastNlMeans' is not supported: only 'bilateral' (or any other string for none)")
    if denoise_method != "bilateral":
        return None
    return bilateral_tables(int(denoise_strength), 75.0, 75.0)


# ---- the reference's two compositions ------------------------------------------------------------------------------------
def enhance_grayscale_np(frame, clip_limit=2.0, tile_grid=8, gamma=0.8, denoise_method="bilateral", denoise_strength=5,
                         channels_out=3):
    """enhance_grayscale_frame (preprocess.py:35-74) for a uint8 frame [H,W,3] (BGR) or [H,W]: BGR2GRAY, CLAHE, the gamma
    table, the bilateral filter, GRAY2BGR -> uint8 [H,W,3] (channels_out = 1: [H,W])."""
    tables = denoise_tables(denoise_method, denoise_strength)
    f = np.asarray(frame)
    gray = ed.bgr_to_gray_np(f) if f.ndim == 3 else _u8_image(f).copy()
    H, W = gray.shape
    check_limits(H, W, tile_grid, None if tables is None else tables[0])
    out = clahe_np(gray, clip_limit, grid_of(tile_grid))
    table = gamma_table(gamma)
    if table is not None:
        out = table[out]
    if tables is not None:
        out = bilateral_np(out, tables=tables)
    if channels_out == 1:
        return out
    if channels_out != 3:
        raise ValueError(f"channels_out must be 1 or 3, got {channels_out!r}")
    return np.ascontiguousarray(np.repeat(out[..., None], 3, axis=2))


def preprocess_frame_np(frame, enable=True, threshold=10.0, **cfg):
    """preprocess_frame (preprocess.py:77-91): the enhanced frame when `enable` and the frame is grey, else a copy."""
    if enable and is_grayscale_np(frame, threshold):
        return enhance_grayscale_np(frame, **cfg)
    denoise_tables(cfg.get("denoise_method", "bilateral"), cfg.get("denoise_strength", 5))     # the same ValueError either way
    return np.array(frame, copy=True)


def crop_roi_np(frame, roi_xywh):
    """crop_roi (preprocess.py:94-113): the slice [max(0, y) : min(H, y + h), max(0, x) : min(W, x + w)], copied."""
    x1, y1, x2, y2 = roi_bounds(frame.shape[0], frame.shape[1], roi_xywh)
    return np.array(frame[y1:y2, x1:x2], copy=True)


def roi_bounds(H, W, roi_xywh):
    """(x1, y1, x2, y2) of crop_roi's clamped slice for roi = (x, y, w, h)."""
    x, y, w, h = (int(v) for v in roi_xywh)
    return max(0, x), max(0, y), min(int(W), x + w), min(int(H), y + h)


# The parameter sets of the fixtures (scripts/make_golden_enhance.py, tests): PreprocessConfig() and one field changed.
FIXTURE_VARIANTS = {
    "default": {}, "gamma1": {"gamma": 1.0}, "tile4": {"tile_grid": 4}, "clip4": {"clip_limit": 4.0},
    "none": {"denoise_method": "none"}, "strength9": {"denoise_strength": 9}, "disabled": {"enable": False},
}


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def make_enhance_scene(H, W, seed, kind="grey"):
    """A uint8 [H,W,3] BGR frame for the enhancement tests.
      grey    a smooth illumination gradient plus two low-frequency waves and sigma = 6 noise, a dark cable band (about
              0.18 W wide, swaying) with a brighter tape section; replicated to three channels, each with its own noise of
              0..3 levels, so that the frame is grey by the reference's rule but not channel-equal
      colour  the same luminance with channel gains and offsets far beyond the threshold
      flat    one value (97) everywhere"""
    if kind not in ("grey", "colour", "flat"):
        raise ValueError(f"kind must be 'grey', 'colour' or 'flat', got {kind!r}")
    if kind == "flat":
        return np.full((H, W, 3), 97, np.uint8)
    r = np.random.default_rng(7001 + seed)
    y = np.arange(H)[:, None] / max(H - 1, 1)
    x = np.arange(W)[None, :] / max(W - 1, 1)
    lum = 90 + 70 * x + 40 * y + 25 * np.sin(6.28 * (1.5 * x + r.uniform(0, 1))) * np.cos(6.28 * (y + r.uniform(0, 1)))
    cx = 0.5 + 0.06 * np.sin(6.28 * y * r.uniform(0.5, 1.5)) + r.uniform(-0.05, 0.05)
    d = np.abs(x - cx)
    lum = np.where(d < 0.09, 35 + 10 * np.cos(d / 0.09 * 1.57), lum)
    lum = np.where((d < 0.12) & (y > 0.35) & (y < 0.8), 200 - 30 * d / 0.12, lum)
    lum = lum + r.normal(0.0, 6.0, (H, W))
    if kind == "grey":
        f = lum[..., None] + r.integers(0, 4, (H, W, 3))
    else:
        f = lum[..., None] * np.array([0.55, 1.0, 1.3])[None, None, :] + np.array([40.0, -10.0, 5.0])[None, None, :]
        f = f + r.integers(0, 4, (H, W, 3))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)
