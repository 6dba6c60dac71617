"""Non-local-means denoising of one 8-bit channel: cv2.fastNlMeansDenoising(img, None, h, 7, 21), the 'fastNlMeans'
denoiser of enhance_grayscale_frame (src/refactor/preprocess.py:68-69, PreprocessConfig.denoise_method), in NumPy
(torch-free) and on the device (include/unetpp.h, unetpp_nlmeans_u8; csrc/nlmeans.h).

The NumPy form restates OpenCV's published FastNlMeansDenoisingInvoker<uchar, int, unsigned, DistSquared, int>.  cv2 is
not installed where this project is built and tested, so cv2's own output stays unpinned, as for every other primitive
(DESIGN.md §5.15); nl_means_np takes `weights=` for a table from elsewhere.  The device kernel matches THIS module bit
for bit: the arithmetic is integer throughout, so no summation order has to be pinned.

With template size t, search size s, th = t // 2, sh = s // 2 and border b = th + sh:
  ext        the image padded by b with BORDER_REFLECT_101
  constants  fixed_point_mult = min(INT32_MAX // (s s 255), INT32_MAX); shift = the smallest p with 2^p >= t t;
             mul = 2^shift / (t t) in float64; n = int(65025 / mul + 1)                       (19096, 6, 49785 for 7 / 21)
  weights    weights[a] = rint(fixed_point_mult exp(-(a mul) / hh)) for a < n, 0 where that is below 0.001
             fixed_point_mult; hh = float32(h) float32(h) widened to float64, exp in float64, rint half to even; h = 0
             gives fixed_point_mult everywhere
  per pixel  over the s s offsets o: D = the sum over the t x t window of (ext[p] - ext[p + o])^2, w = weights[D >> shift],
             est += w ext[centre + o], wsum += w;   out = (uint32(est) + wsum // 2) // wsum
The centre offset has D = 0, so wsum >= weights[0]; est reaches 2,147,440,680 on a constant 255 image and the rounding
term takes it past INT32_MAX: unsigned (here int64).

`enhance_grayscale_nlm*` / `preprocess_frame(s)_nlm*` are enhance_grayscale_frame / preprocess_frame with
denoise_method='fastNlMeans'.  The two NestedUNet methods of those names keep refusing 'fastNlMeans' (their tests pin
it); the functions here take the model as frame_loop.measure_frames does.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import enhance as en
from .geometry import reflect101

INT32_MAX = 2 ** 31 - 1
DEVICE_TEMPLATE, DEVICE_SEARCH = 7, 21          # the sizes the kernel is compiled for (the only ones the reference uses)
MAX_PREFIX = 8192                               # longest non-zero prefix of the weight table the kernel stages
MIN_SIDE = DEVICE_TEMPLATE // 2 + DEVICE_SEARCH // 2 + 1        # 14: the border never reflects twice
DEFAULTS = dict(clip_limit=2.0, tile_grid=8, gamma=0.8, denoise_strength=5)      # PreprocessConfig, denoise_method='fastNlMeans'


def _sizes(t, s):
    t, s = int(t), int(s)
    if t < 1 or s < 1 or t % 2 == 0 or s % 2 == 0:
        raise ValueError(f"template and search window sizes must be odd and positive, got {t} and {s}")
    return t, s


def nlm_constants(t=7, s=21):
    """(fixed_point_mult, shift, mul, n) of the invoker for template size t and search size s."""
    t, s = _sizes(t, s)
    fixed_point_mult = min(INT32_MAX // (s * s * 255), INT32_MAX)
    shift = 0
    while (1 << shift) < t * t:
        shift += 1
    mul = float(1 << shift) / float(t * t)
    return fixed_point_mult, shift, mul, int(65025 / mul + 1)


def nlm_weights(h, t=7, s=21):
    """The weight table int64 [n] for filter strength h (module docstring)."""
    fpm, _, mul, n = nlm_constants(t, s)
    hh = float(np.float32(h) * np.float32(h))
    if not hh >= 0 or not np.isfinite(hh):
        raise ValueError(f"h must be a finite number, got {h!r}")
    a = np.arange(n, dtype=np.float64)
    w = np.exp(-(a * mul) / hh) if hh > 0 else np.ones(n, np.float64)
    w = np.rint(fpm * w)
    w[w < 0.001 * fpm] = 0
    return w.astype(np.int64)


def check_weights(weights, t=7, s=21):
    """A caller's table as int64 [<= n]: integers in [0, fixed_point_mult], entry 0 positive (it divides).  Entries past
    its end count as 0."""
    fpm, _, _, n = nlm_constants(t, s)
    w = np.asarray(weights)
    if w.ndim != 1 or not np.issubdtype(w.dtype, np.integer) or not 1 <= len(w) <= n:
        raise ValueError(f"weights must be a 1-D integer table of 1..{n} entries, got {w.dtype} {w.shape}")
    w = w.astype(np.int64)
    if w.min() < 0 or w.max() > fpm or w[0] < 1:
        raise ValueError(f"weights must lie in [0, {fpm}] with weights[0] >= 1 (the sums are 32-bit and weights[0] divides)")
    return w


def prefix_length(weights):
    """Entries up to the last non-zero one."""
    nz = np.flatnonzero(np.asarray(weights))
    return int(nz[-1]) + 1 if len(nz) else 0


def check_limits(H, W, t=7, s=21, weights=None, device=False):
    """ValueError for what nl_means_np refuses: H, W > t // 2 + s // 2 (the border reflects once), H, W <= 65535,
    H W <= 2^30.  device=True adds what the kernel refuses: (t, s) other than (7, 21), and with `weights` a non-zero
    prefix longer than 8,192 entries."""
    t, s = _sizes(t, s)
    if device and (t, s) != (DEVICE_TEMPLATE, DEVICE_SEARCH):
        raise ValueError(f"template_window_size {t} and search_window_size {s}: the device path supports only "
                         f"{DEVICE_TEMPLATE} and {DEVICE_SEARCH}")
    if device and weights is not None and prefix_length(weights) > MAX_PREFIX:
        raise ValueError(f"the weight table's non-zero prefix has {prefix_length(weights)} entries: the device path takes at most "
                         f"{MAX_PREFIX} (h up to about 39)")
    if H is None:
        return
    H, W, b = int(H), int(W), t // 2 + s // 2
    if H <= b or W <= b or H > en.MAX_SIDE or W > en.MAX_SIDE or H * W > en.MAX_PIXELS:
        raise ValueError(f"image is {H}x{W}: needs {b + 1} <= H, W <= {en.MAX_SIDE} and H * W <= 2^30")


def _table(h, t, s, weights):
    return nlm_weights(h, t, s) if weights is None else check_weights(weights, t, s)


def _lookup(w, idx):
    return np.where(idx < len(w), w[np.minimum(idx, len(w) - 1)], 0)


def nl_means_np(gray, h=3.0, t=7, s=21, weights=None):
    """cv2.fastNlMeansDenoising(gray, None, h, t, s) for uint8 [H,W] as the invoker computes it (module docstring), one
    pass per offset with the box sums of the squared differences by cumulative sums.  weights: a table instead of
    nlm_weights(h, t, s)."""
    gray = en._u8_image(gray)
    t, s = _sizes(t, s)
    H, W = gray.shape
    check_limits(H, W, t, s)
    w = _table(h, t, s, weights)
    _, shift, _, _ = nlm_constants(t, s)
    th, sh = t // 2, s // 2
    b = th + sh
    ext = gray[reflect101(np.arange(-b, H + b), H)][:, reflect101(np.arange(-b, W + b), W)].astype(np.int64)
    base = ext[sh:sh + H + 2 * th, sh:sh + W + 2 * th]            # the pixels the centre patches cover
    est = np.zeros((H, W), np.int64)
    wsum = np.zeros((H, W), np.int64)
    ii = np.zeros((H + 2 * th + 1, W + 2 * th + 1), np.int64)
    for dy in range(-sh, sh + 1):
        for dx in range(-sh, sh + 1):
            d = base - ext[sh + dy:sh + dy + H + 2 * th, sh + dx:sh + dx + W + 2 * th]
            np.cumsum(np.cumsum(d * d, axis=0), axis=1, out=ii[1:, 1:])
            D = ii[t:, t:] - ii[:-t, t:] - ii[t:, :-t] + ii[:-t, :-t]
            wt = _lookup(w, D >> shift)
            est += wt * ext[b + dy:b + dy + H, b + dx:b + dx + W]
            wsum += wt
    assert est.max() < 2 ** 32 - wsum.max()
    return ((est + wsum // 2) // wsum).astype(np.uint8)


def nl_means_literal_np(gray, h=3.0, t=7, s=21, weights=None):
    """The same, pixel by pixel with every patch difference squared and summed on its own: a cross-check for tiny images."""
    gray = en._u8_image(gray)
    t, s = _sizes(t, s)
    H, W = gray.shape
    check_limits(H, W, t, s)
    w = _table(h, t, s, weights)
    _, shift, _, _ = nlm_constants(t, s)
    th, sh = t // 2, s // 2
    b = th + sh
    ext = np.pad(gray, b, mode="reflect").astype(np.int64)
    patches = np.lib.stride_tricks.sliding_window_view(ext, (t, t))       # patches[y, x] = ext[y : y + t, x : x + t]
    out = np.zeros((H, W), np.uint8)
    for i in range(H):
        for j in range(W):
            p0 = patches[i + sh, j + sh]                                  # centred on ext[i + b, j + b]
            D = ((patches[i:i + s, j:j + s] - p0) ** 2).sum(axis=(2, 3))     # [s, s], offset (dy, dx) at [dy + sh, dx + sh]
            wt = _lookup(w, D >> shift)
            est = int((wt * ext[i + th:i + th + s, j + th:j + th + s]).sum())
            wsum = int(wt.sum())
            out[i, j] = ((est & 0xFFFFFFFF) + wsum // 2) // wsum
    return out


# ---- the reference's two compositions with denoise_method='fastNlMeans' ---------------------------------------------------
def enhance_grayscale_nlm_np(frame, clip_limit=2.0, tile_grid=8, gamma=0.8, denoise_strength=5, channels_out=3):
    """enhance_grayscale_frame (preprocess.py:35-74) with denoise_method='fastNlMeans' for a uint8 frame [H,W,3] (BGR) or
    [H,W]: BGR2GRAY, CLAHE, the gamma table, cv2.fastNlMeansDenoising(img, None, denoise_strength, 7, 21), GRAY2BGR ->
    uint8 [H,W,3] (channels_out = 1: [H,W])."""
    if channels_out not in (1, 3):
        raise ValueError(f"channels_out must be 1 or 3, got {channels_out!r}")
    f = np.asarray(frame)
    check_limits(f.shape[0], f.shape[1])
    out = en.enhance_grayscale_np(f, clip_limit, tile_grid, gamma, "none", 0, channels_out=1)
    out = nl_means_np(out, float(denoise_strength), 7, 21)
    return out if channels_out == 1 else np.ascontiguousarray(np.repeat(out[..., None], 3, axis=2))


def preprocess_frame_nlm_np(frame, enable=True, threshold=10.0, **cfg):
    """preprocess_frame (preprocess.py:77-91) with denoise_method='fastNlMeans': the enhanced frame when `enable` and the
    frame is grey, else a copy."""
    if enable and en.is_grayscale_np(frame, threshold):
        return enhance_grayscale_nlm_np(frame, **cfg)
    return np.array(frame, copy=True)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def make_nlm_scene(H, W, seed, kind="ramp"):
    """A uint8 [H,W,3] BGR frame for the denoising tests and fixtures.
      ramp    a quiet scene: the plane 60 + 108 x + 33 y (x, y in 0..1 over max(W, 90) and max(H, 67) pixels: at most 1.2 and
              0.5 levels per pixel) plus a step of 40 levels along a slanted line, Gaussian noise of sigma 0.6..1.5 (by
              seed); replicated to three channels, each with its own 0..1 levels on top, so the frame is grey by the
              reference's rule but not channel-equal.  The noise stays below the weight cut-off after CLAHE and gamma, so
              the filter changes most pixels already at h = 5 (enhance.make_enhance_scene's sigma 6 is changed in none)
      colour  enhance.make_enhance_scene's colour frame (copied through by preprocess_frame)"""
    if kind == "colour":
        return en.make_enhance_scene(H, W, seed, "colour")
    if kind != "ramp":
        raise ValueError(f"kind must be 'ramp' or 'colour', got {kind!r}")
    r = np.random.default_rng(9100 + seed)
    y = np.arange(H)[:, None] / max(H - 1, 66)
    x = np.arange(W)[None, :] / max(W - 1, 89)
    lum = 60 + 108 * x + 33 * y + 40 * ((x - 0.25 * y) > r.uniform(0.35, 0.6))
    lum = lum + r.normal(0.0, r.uniform(0.6, 1.5), (H, W))
    f = lum[..., None] + r.integers(0, 2, (H, W, 3))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


# ---- the device path (torch imported lazily, as in frame_loop.py) ---------------------------------------------------------
_DEVICE_TABLES = {}                # (device index, table bytes) -> (int16 CUDA tensor holding the uint16 prefix, its length)
_MAX_CACHED_TABLES = 32


def device_table(device, h=3.0, weights=None):
    """(tensor, n): the non-zero prefix of the table as uint16 on `device` (kept in an int16 tensor), cached per device and
    table contents.  ValueError for a prefix longer than 8,192 entries."""
    import torch
    w = _table(h, DEVICE_TEMPLATE, DEVICE_SEARCH, weights)
    check_limits(None, None, weights=w, device=True)
    prefix = np.ascontiguousarray(w[:prefix_length(w)].astype(np.uint16))
    key = (torch.device(device).index, prefix.tobytes())
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        if len(_DEVICE_TABLES) >= _MAX_CACHED_TABLES:
            _DEVICE_TABLES.pop(next(iter(_DEVICE_TABLES)))
        hit = _DEVICE_TABLES[key] = (torch.from_numpy(prefix.view(np.int16).copy()).to(device), len(prefix))
    return hit


def _launch(model, src, cin, cout, decisions, table, n):
    """unetpp_nlmeans_u8 on the current stream: one launch, nothing read back."""
    import torch
    b, h, w = src.shape[:3]
    check_limits(h, w, device=True)
    if b > 65535:
        raise ValueError(f"batch {b}: at most 65535")
    out = torch.empty((b, h, w, 3) if cout == 3 else (b, h, w), dtype=torch.uint8, device=src.device)
    model._call("unetpp_nlmeans_u8", src, b, h, w, cin, cout, decisions, table, n, out, stream_of=src)
    return out


def nl_means(model, gray, h=3.0, template_window_size=7, search_window_size=21, weights=None):
    """cv2.fastNlMeansDenoising(gray, None, h, 7, 21) for a uint8 CUDA tensor [B,H,W] -> the same shape, as nl_means_np
    computes it, bit for bit (cv2's own result is unpinned).  The defaults are cv2's.  Only template 7 / search 21 run on
    the device; H, W >= 14; the table's non-zero prefix has at most 8,192 entries (h up to about 39).  weights: a
    caller's integer table instead of nlm_weights(h)."""
    check_limits(None, None, template_window_size, search_window_size, device=True)
    if weights is not None:
        check_limits(None, None, weights=check_weights(weights), device=True)
    gray = model._input(gray)
    table, n = device_table(gray.device, h, weights)
    return _launch(model, gray, 1, 1, None, table, n)


def enhance_grayscale_nlm(model, frames, *, clip_limit=2.0, tile_grid=8, gamma=0.8, denoise_strength=5, channels_out=3):
    """enhance_grayscale_frame with denoise_method='fastNlMeans' for uint8 CUDA frames [B,H,W,3] (BGR) or [B,H,W]:
    NestedUNet.enhance_grayscale's launches without a filter, then one non-local-means launch -> uint8 [B,H,W,3]
    (channels_out = 1: [B,H,W]); every frame is enhanced, nothing is read back (enhance_grayscale_nlm_np is the NumPy form)."""
    from . import _lib
    if channels_out not in (1, 3):
        raise ValueError(f"channels_out must be 1 or 3, got {channels_out!r}")
    frames, cin = model._enhance_input(frames)
    check_limits(frames.shape[1], frames.shape[2], device=True)
    table, n = device_table(frames.device, float(denoise_strength))
    mid = model._enhance(frames, cin, 1, _lib.ENHANCE_ALWAYS, 0.0, clip_limit, tile_grid, en.gamma_table(gamma), None)[0]
    return _launch(model, mid, 1, int(channels_out), None, table, n)


def preprocess_frames_nlm(model, frames, enable=True, threshold=10.0, *, clip_limit=2.0, tile_grid=8, gamma=0.8, denoise_strength=5,
                          return_decisions=False):
    """preprocess_frame with denoise_method='fastNlMeans' for a batch of uint8 CUDA frames [B,H,W,3]: the launches of
    NestedUNet.preprocess_frames(denoise_method="none") -- grey frames through CLAHE and gamma, colour frames copied, the
    decision byte of every frame left ON THE DEVICE -- then one non-local-means launch gated by those bytes: a colour
    frame is copied through again, all three channels.  No synchronisation and no read-back between the first and the
    last launch.  Frames [B,H,W] always count as grey and come back as [B,H,W,3].  return_decisions: also bool [B]."""
    import torch
    from . import _lib
    frames, cin = model._enhance_input(frames)
    check_limits(frames.shape[1], frames.shape[2], device=True)
    table, n = device_table(frames.device, float(denoise_strength))
    if not enable:
        out = frames.clone() if cin == 3 else frames[..., None].expand(-1, -1, -1, 3).contiguous()
        return (out, torch.zeros((frames.shape[0],), dtype=torch.bool, device=frames.device)) if return_decisions else out
    mid, _, dec = model._enhance(frames, cin, 3, _lib.ENHANCE_IF_GREY, threshold, clip_limit, tile_grid, en.gamma_table(gamma), None,
                                 want_decisions=True)
    out = _launch(model, mid, 3, 3, dec, table, n)
    return (out, dec != 0) if return_decisions else out


def layout():
    """(rows, columns) of output one workgroup of the kernel owns (unetpp_nlmeans_layout)."""
    from . import _lib
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    if _lib.load().unetpp_nlmeans_layout(ctypes.byref(rows), ctypes.byref(cols)) != 0:
        raise RuntimeError("unetpp_nlmeans_layout failed")
    return rows.value, cols.value
