"""Training batches: what the reference's dataset classes do per sample and per pixel on the host, in NumPy (torch-free, the
definition) and on the device (include/unetpp_train_batch.h; csrc/train_batch.h), one launch per batch.

  CableDefectDataset.__getitem__    src/data/dataset.py:45-133        resize, flip, flip, HSV brightness, / 255, CHW
  the class maps on top of it       tools/train_3class_high_precision.py:74-115, tools/train_3class.py:27-53,
                                    src/data/advanced_dataset.py:273-294
  PatchDefectDataset                src/data/patch_dataset.py:105-233  crop, fliplr, flipud, rot90, convertScaleAbs, resize,
                                    / 255, CHW, the binary defect target
  _tape_focused_crop                src/data/advanced_dataset.py:143-186 in front of the legacy path :234-263

Every sample goes through the same fixed stages; a plan row says which of them do something:
  1. crop             the rectangle (x1, y1, x2, y2) of the item, inline or a row of the table crop_rects wrote
  2. geometry A       fliplr, then flipud, then np.rot90(., k)                       (patch_dataset.py:176-189)
  3. byte look-up     a 256-entry table on every source byte                         (convertScaleAbs precedes the resize)
  4. resize           cv2.INTER_LINEAR for the image (tiling.resize_linear_u8_np), INTER_NEAREST for the mask
                      (robust.resize_nearest_np); equal sizes give the source bytes
  5. geometry B       flip(., 1), then flip(., 0)                                    (dataset.py:116-123, after its resize)
  6. brightness       RGB -> HSV, V through a 256-entry table, HSV -> RGB            (dataset.py:126-131)
  7. / 255            through divide_255_table(), CHW float32; or the bytes, HWC
The mask takes 1, 2, 4 and 5 and then one class look-up.  cv2's tap rounding is not mirror-symmetric, so a flip before the
resize and a flip after it differ in bits: the two datasets flip on different sides, hence the two geometry stages.

The brightness step.  `hsv[:, :, 2] *= factor` acts on float32 integers, so the new V depends on V alone:
value_scale_lut(factor).  RGB -> HSV is the integer form of OpenCV's published 8-bit conversion (hue range 180, the two
12-bit division tables, the rounding shift), HSV -> RGB its published float32 form (sector table, saturate_cast<uchar>(x *
255)), every float operation rounded on its own.  cv2 is not installed where this project is built and tested, so cv2's own
conversions stay unpinned; hsv_value_scale_np is the definition and the device equals it bit for bit.

The draw replays consume np.random / random in the order the reference's methods do, so seeding the reference and seeding a
replay give the same plan.  The functions take the model, as the newer modules do.
"""
from __future__ import annotations

import numpy as np

from . import robust as rb
from . import tiling as tl

_f = np.float32

PLAN_COLS = 16
(P_ITEM, P_RECT_ROW, P_X1, P_Y1, P_X2, P_Y2, P_FLIP_H, P_FLIP_V, P_ROT, P_BYTE_LUT, P_POST_FLIP_H, P_POST_FLIP_V,
 P_VALUE_LUT) = range(13)
RECT_COLS = 6                       # x1, y1, x2, y2, n_found, valid
REQUEST_COLS = 5                    # item, k, crop_h, crop_w, class
ITEM_COLS = 4                       # image offset, mask offset (bytes), h, w
IMAGE_FORMATS = {"chw_f32": 0, "hwc_u8": 1}
CHANNEL_ORDERS = ("rgb", "bgr")
MAX_SIDE = 65535
DEFECT_CLASSES = (3, 4, 5)          # patch_dataset.py:47


# ---- look-up builders -------------------------------------------------------------------------------------------------------------
def _table(t):
    t = np.asarray(t)
    if t.dtype != np.uint8 or t.shape != (256,):
        raise ValueError(f"a look-up table must be uint8 [256], got {t.dtype} {list(t.shape)}")
    return t


def divide_255_table():
    """float32 [256]: i / 255.0 by IEEE division (`astype(float32) / 255.0`, dataset.py:95)."""
    return (np.arange(256, dtype=_f) / _f(255.0)).astype(_f)


def convert_scale_abs_lut(alpha, beta):
    """uint8 [256]: cv2.convertScaleAbs(x, alpha=alpha, beta=beta) restated, float32 |x alpha + beta| rounded half to even and
    saturated.  A caller who has cv2 passes cv2's own 256 outputs instead."""
    x = np.arange(256, dtype=_f)
    v = np.abs((x * _f(alpha)).astype(_f) + _f(beta)).astype(_f)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def value_scale_lut(factor):
    """uint8 [256]: V -> uint8(clip(float32(V) * float32(factor), 0, 255)), truncated (dataset.py:129-131)."""
    v = (np.arange(256, dtype=_f) * _f(factor)).astype(_f)
    return np.clip(v, 0, 255).astype(np.uint8)


def class_lut(mapping, default="keep"):
    """uint8 [256] from {mask byte: class}.  default="keep": other bytes stay (the NumPy branch of remap_mask_to_3class starts
    from mask.copy()); "zero": they become 0 (the torch branch and the dataset classes start from zeros_like)."""
    if default not in ("keep", "zero"):
        raise ValueError(f"default must be 'keep' or 'zero', got {default!r}")
    t = np.arange(256, dtype=np.int64) if default == "keep" else np.zeros(256, np.int64)
    for k, v in dict(mapping).items():
        if not (0 <= int(k) <= 255 and 0 <= int(v) <= 255):
            raise ValueError(f"class map entry {k!r}: {v!r} outside 0..255")
        t[int(k)] = int(v)
    return t.astype(np.uint8)


def binary_defect_lut(classes=DEFECT_CLASSES):
    """uint8 [256]: 1 for the defect classes, else 0 (patch_dataset.py:227-231)."""
    return class_lut({c: 1 for c in classes}, default="zero")


# ---- the brightness step -----------------------------------------------------------------------------------------------------------
def hsv_division_tables():
    """(sdiv, hdiv) int32 [256]: saturate_cast<int>((255 << 12) / (1. * i)) and saturate_cast<int>((180 << 12) / (6. * i)),
    rounded half to even in float64, 0 at i = 0."""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, np.int32), np.zeros(256, np.int32)
    sdiv[1:] = np.rint(np.float64(255 << 12) / i).astype(np.int32)
    hdiv[1:] = np.rint(np.float64(180 << 12) / (np.float64(6.0) * i)).astype(np.int32)
    return sdiv, hdiv


_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]], np.int64)        # (b, g, r) per sector


def rgb_to_hsv_u8_np(rgb):
    """uint8 [...,3] RGB -> (h, s, v) uint8 arrays: the integer 8-bit RGB2HSV, hue range 180."""
    x = np.asarray(rgb)
    if x.dtype != np.uint8 or x.shape[-1] != 3:
        raise ValueError("rgb must be uint8 [...,3]")
    sdiv, hdiv = hsv_division_tables()
    r, g, b = (x[..., c].astype(np.int32) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.clip(h, 0, 255).astype(np.uint8), np.clip(s, 0, 255).astype(np.uint8), v.astype(np.uint8)


def hsv_to_rgb_u8_np(h, s, v):
    """(h, s, v) uint8 arrays -> uint8 [...,3] RGB: the float32 8-bit HSV2RGB, every operation rounded on its own."""
    hf = (np.asarray(h).astype(_f) * (_f(6.0) / _f(180.0))).astype(_f)
    sf = (np.asarray(s).astype(_f) * (_f(1.0) / _f(255.0))).astype(_f)
    vf = (np.asarray(v).astype(_f) * (_f(1.0) / _f(255.0))).astype(_f)
    hf = np.fmod(hf, _f(6.0)).astype(_f)
    sector = np.floor(hf).astype(np.int64)
    hf = (hf - sector.astype(_f)).astype(_f)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    hf = np.where(bad, _f(0.0), hf).astype(_f)
    one = _f(1.0)
    tab = np.stack([vf, (vf * (one - sf)).astype(_f), (vf * (one - (sf * hf).astype(_f))).astype(_f),
                    (vf * (one - (sf * (one - hf)).astype(_f))).astype(_f)], axis=-1)
    pick = _SECTOR[sector]                                                          # [...,3] in (b, g, r) order
    bgr = np.take_along_axis(tab, pick, axis=-1)
    bgr = np.where((sf == 0)[..., None], vf[..., None], bgr).astype(_f)
    out = np.clip(np.rint((bgr * _f(255.0)).astype(_f)), 0, 255).astype(np.uint8)
    return out[..., ::-1]


def hsv_value_scale_np(rgb, table):
    """dataset.py:128-131 for a uint8 RGB image [...,3]: RGB -> HSV, V through `table` (uint8 [256]), HSV -> RGB."""
    table = _table(table)
    h, s, v = rgb_to_hsv_u8_np(rgb)
    return hsv_to_rgb_u8_np(h, s, table[v])


# ---- the data-dependent crop --------------------------------------------------------------------------------------------------------
def tape_crop_rect_np(mask, k, crop_h, crop_w, cls=2):
    """advanced_dataset.py:148-186 for one mask [h,w]: (x1, y1, x2, y2, n_found, valid) with the k-th pixel of class `cls` in
    raster order as the centre, the integer lines :165-180 as they stand (the adjusted rectangle may stay smaller than crop_h x
    crop_w).  No pixel of the class: the whole image, valid 1 (the reference returns the original).  k outside 0 .. n_found - 1
    (a stale count): the whole image, valid 0."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask must be [h,w]")
    crop_h, crop_w, k = int(crop_h), int(crop_w), int(k)
    if crop_h < 1 or crop_w < 1:
        raise ValueError(f"crop size {crop_h}x{crop_w} must be at least 1x1")
    h, w = m.shape
    ys, xs = np.where(m == cls)
    n = len(ys)
    if n == 0:
        return (0, 0, w, h, 0, 1)
    if not 0 <= k < n:
        return (0, 0, w, h, n, 0)
    center_y, center_x = int(ys[k]), int(xs[k])
    y1 = max(0, center_y - crop_h // 2)
    y2 = min(h, center_y + crop_h // 2)
    x1 = max(0, center_x - crop_w // 2)
    x2 = min(w, center_x + crop_w // 2)
    if y2 - y1 < crop_h:
        if y1 == 0:
            y2 = min(h, y1 + crop_h)
        else:
            y1 = max(0, y2 - crop_h)
    if x2 - x1 < crop_w:
        if x1 == 0:
            x2 = min(w, x1 + crop_w)
        else:
            x1 = max(0, x2 - crop_w)
    return (x1, y1, x2, y2, n, 1)


def crop_rects_np(masks, requests):
    """int32 [B,6] for requests int32 [B,5] = (item, k, crop_h, crop_w, class) over the list `masks`."""
    req = _requests(requests, len(masks))
    return np.array([tape_crop_rect_np(masks[r[0]], r[1], r[2], r[3], r[4]) for r in req], np.int32).reshape(-1, RECT_COLS)


def _requests(requests, n_items):
    req = np.asarray(requests)
    if req.ndim != 2 or req.shape[1] != REQUEST_COLS or not np.issubdtype(req.dtype, np.integer) or len(req) < 1:
        raise ValueError(f"requests must be an integer table [B,{REQUEST_COLS}] = (item, k, crop_h, crop_w, class)")
    req = req.astype(np.int64)
    if ((req[:, 0] < 0) | (req[:, 0] >= n_items)).any():
        raise ValueError(f"a request names an item outside 0..{n_items - 1}")
    if (req[:, 2:4] < 1).any() or (req[:, 2:4] > MAX_SIDE).any():
        raise ValueError("crop_h and crop_w must lie in 1..65535")
    if ((req[:, 4] < 0) | (req[:, 4] > 255)).any():
        raise ValueError("class must lie in 0..255")
    if (np.abs(req[:, 1]) >= 2 ** 31).any():
        raise ValueError("k must fit an int32")
    return req.astype(np.int32)


# ---- plans -------------------------------------------------------------------------------------------------------------------------
def sample(item, rect=None, rect_row=None, flip_h=False, flip_v=False, rot90=0, byte_lut=None, post_flip_h=False, post_flip_v=False,
           value_lut=None):
    """One output sample as a dict: rect (x1, y1, x2, y2) inline, or rect_row, the row of the rect table; neither: the whole
    item.  byte_lut / value_lut: uint8 [256] or None."""
    if rect is not None and rect_row is not None:
        raise ValueError("give rect or rect_row, not both")
    return dict(item=int(item), rect=None if rect is None else tuple(int(v) for v in rect), rect_row=rect_row, flip_h=bool(flip_h),
                flip_v=bool(flip_v), rot90=int(rot90) % 4, byte_lut=None if byte_lut is None else _table(byte_lut),
                post_flip_h=bool(post_flip_h), post_flip_v=bool(post_flip_v), value_lut=None if value_lut is None else _table(value_lut))


def build_plan(samples, sizes):
    """(plan int32 [B,16], luts uint8 [n,256]) from sample() dicts; `sizes` = [(h, w)] per item.  Equal tables share a row."""
    samples = list(samples)
    if not samples:
        raise ValueError("a plan needs at least one sample")
    plan = np.zeros((len(samples), PLAN_COLS), np.int32)
    luts, index = [], {}

    def row(t):
        if t is None:
            return -1
        key = t.tobytes()
        if key not in index:
            index[key] = len(luts)
            luts.append(t)
        return index[key]

    for b, s in enumerate(samples):
        if not 0 <= s["item"] < len(sizes):
            raise ValueError(f"sample {b}: item {s['item']} outside 0..{len(sizes) - 1}")
        h, w = sizes[s["item"]]
        p = plan[b]
        p[P_ITEM], p[P_RECT_ROW] = s["item"], -1
        if s["rect_row"] is not None:
            if int(s["rect_row"]) < 0:
                raise ValueError(f"sample {b}: rect_row {s['rect_row']} is negative")
            p[P_RECT_ROW] = int(s["rect_row"])
        else:
            x1, y1, x2, y2 = s["rect"] if s["rect"] is not None else (0, 0, w, h)
            if not (0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h):
                raise ValueError(f"sample {b}: rect {(x1, y1, x2, y2)} is empty or outside the {h}x{w} item")
            p[P_X1:P_Y2 + 1] = (x1, y1, x2, y2)
        p[P_FLIP_H], p[P_FLIP_V], p[P_ROT] = s["flip_h"], s["flip_v"], s["rot90"]
        p[P_POST_FLIP_H], p[P_POST_FLIP_V] = s["post_flip_h"], s["post_flip_v"]
        p[P_BYTE_LUT], p[P_VALUE_LUT] = row(s["byte_lut"]), row(s["value_lut"])
    return plan, (np.stack(luts) if luts else np.zeros((0, 256), np.uint8))


def check_plan(plan, luts, n_items, rects=None):
    plan = np.asarray(plan)
    if plan.dtype != np.int32 or plan.ndim != 2 or plan.shape[1] != PLAN_COLS or len(plan) < 1:
        raise ValueError(f"plan must be int32 [B,{PLAN_COLS}], got {plan.dtype} {list(plan.shape)}")
    luts = np.asarray(luts)
    if luts.dtype != np.uint8 or luts.ndim != 2 or luts.shape[1] != 256:
        raise ValueError(f"luts must be uint8 [n,256], got {luts.dtype} {list(luts.shape)}")
    if ((plan[:, P_ITEM] < 0) | (plan[:, P_ITEM] >= n_items)).any():
        raise ValueError(f"plan: an item outside 0..{n_items - 1}")
    for col in (P_BYTE_LUT, P_VALUE_LUT):
        if ((plan[:, col] < -1) | (plan[:, col] >= len(luts))).any():
            raise ValueError(f"plan: a look-up row outside -1..{len(luts) - 1}")
    if ((plan[:, P_ROT] < 0) | (plan[:, P_ROT] > 3)).any():
        raise ValueError("plan: rot90 outside 0..3")
    rows = plan[:, P_RECT_ROW]
    n_rects = 0 if rects is None else int(rects.shape[0])
    if (rows < -1).any() or (rows >= n_rects).any():
        raise ValueError(f"plan: a rect row outside the rect table's {n_rects} rows")
    return plan, luts


def _size(size_hw):
    oh, ow = (int(v) for v in size_hw)
    if not (1 <= oh <= MAX_SIDE and 1 <= ow <= MAX_SIDE):
        raise ValueError(f"size_hw {size_hw} outside 1..65535")
    return oh, ow


def _format(image_format, channel_order):
    if image_format not in IMAGE_FORMATS:
        raise ValueError(f"image_format must be one of {sorted(IMAGE_FORMATS)}, got {image_format!r}")
    if channel_order not in CHANNEL_ORDERS:
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
    if image_format == "chw_f32" and channel_order != "rgb":
        raise ValueError("channel_order='bgr' needs image_format='hwc_u8': the float tensor is the reference's, RGB")
    return 0 if image_format == "chw_f32" else (1 if channel_order == "rgb" else 2)


def _check_items(images, masks):
    if len(images) != len(masks) or not len(images):
        raise ValueError("images and masks must be two lists of the same, non-zero length")
    for i, (im, m) in enumerate(zip(images, masks)):
        im, m = np.asarray(im), np.asarray(m)
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or m.dtype != np.uint8 or m.ndim != 2 or im.shape[:2] != m.shape:
            raise ValueError(f"item {i}: the image must be uint8 [h,w,3] and the mask uint8 [h,w] of the same size")
        if not (1 <= m.shape[0] <= MAX_SIDE and 1 <= m.shape[1] <= MAX_SIDE and m.shape[0] * m.shape[1] < 2 ** 31):
            raise ValueError(f"item {i}: size {m.shape} outside 1..65535 per side and 2^31 - 1 pixels")


def assemble_np(images, masks, plan, luts, size_hw, class_table=None, rects=None, image_format="chw_f32", channel_order="rgb"):
    """The batch of `plan` (build_plan) over the lists images (uint8 [h_i,w_i,3] RGB) and masks (uint8 [h_i,w_i]), one sample
    at a time: (image float32 [B,3,H,W], or uint8 [B,H,W,3] for image_format="hwc_u8"; target uint8 [B,H,W]).  rects: the int32
    [n,6] table of crop_rects_np for the samples that name a row of it.  class_table: uint8 [256] for the mask, or None."""
    _check_items(images, masks)
    plan, luts = check_plan(plan, luts, len(images), rects)
    oh, ow = _size(size_hw)
    fmt = _format(image_format, channel_order)
    ctab = np.arange(256, dtype=np.uint8) if class_table is None else _table(class_table)
    div = divide_255_table()
    out_i = np.zeros((len(plan), 3, oh, ow), _f) if fmt == 0 else np.zeros((len(plan), oh, ow, 3), np.uint8)
    out_t = np.zeros((len(plan), oh, ow), np.uint8)
    for b, p in enumerate(plan):
        img, msk = np.asarray(images[p[P_ITEM]]), np.asarray(masks[p[P_ITEM]])
        h, w = msk.shape
        x1, y1, x2, y2 = (rects[p[P_RECT_ROW]][:4] if p[P_RECT_ROW] >= 0 else p[P_X1:P_Y2 + 1])
        x1, x2 = min(max(int(x1), 0), w), min(max(int(x2), 0), w)
        y1, y2 = min(max(int(y1), 0), h), min(max(int(y2), 0), h)
        if x2 <= x1 or y2 <= y1:
            continue                                         # an empty rectangle: the sample stays zero, as the kernel leaves it
        ci, cm = img[y1:y2, x1:x2], msk[y1:y2, x1:x2]
        if p[P_FLIP_H]:
            ci, cm = np.fliplr(ci), np.fliplr(cm)
        if p[P_FLIP_V]:
            ci, cm = np.flipud(ci), np.flipud(cm)
        if p[P_ROT]:
            ci, cm = np.rot90(ci, int(p[P_ROT])), np.rot90(cm, int(p[P_ROT]))
        ci, cm = np.ascontiguousarray(ci), np.ascontiguousarray(cm)
        if p[P_BYTE_LUT] >= 0:
            ci = luts[p[P_BYTE_LUT]][ci]
        ci = tl.resize_linear_u8_np(ci, (ow, oh))
        cm = rb.resize_nearest_np(cm, (ow, oh))
        if p[P_POST_FLIP_H]:
            ci, cm = ci[:, ::-1], cm[:, ::-1]
        if p[P_POST_FLIP_V]:
            ci, cm = ci[::-1], cm[::-1]
        if p[P_VALUE_LUT] >= 0:
            ci = hsv_value_scale_np(np.ascontiguousarray(ci), luts[p[P_VALUE_LUT]])
        out_t[b] = ctab[cm]
        if fmt == 0:
            out_i[b] = div[ci].transpose(2, 0, 1)
        else:
            out_i[b] = ci if fmt == 1 else ci[..., ::-1]
    return out_i, out_t


# ---- draw replays: the reference's consumption of np.random / random, in its order ---------------------------------------------------
DRAW_CODES = {"np.random.random": 0, "np.random.randint": 1, "random.random": 2, "random.randint": 3, "random.uniform": 4}


class ReplayRng:
    """Stands for np.random (which="np") or the random module ("py") and hands back recorded draws, float64 [n,2] = (call of
    DRAW_CODES, value), in order; a call of another kind than the recorded one, or a draw outside the asked range, raises."""

    def __init__(self, draws, which="np"):
        self.draws = np.asarray(draws, np.float64).reshape(-1, 2)
        self.at, self.which = 0, which

    def _next(self, name):
        if self.at >= len(self.draws):
            raise AssertionError(f"{name} called after the {len(self.draws)} recorded draws")
        code, v = self.draws[self.at]
        want = DRAW_CODES[("np.random." if self.which == "np" else "random.") + name]
        if int(code) != want:
            raise AssertionError(f"draw {self.at}: {name} called, call {int(code)} recorded")
        self.at += 1
        return v

    def random(self):
        return float(self._next("random"))

    def randint(self, a, b):
        v = int(self._next("randint"))
        if not (a <= v < b if self.which == "np" else a <= v <= b):
            raise AssertionError(f"draw {self.at - 1}: randint({a}, {b}) recorded {v}")
        return v

    def uniform(self, a, b):
        return float(self._next("uniform"))

    def exhausted(self):
        return self.at == len(self.draws)


def draw_cable_defect(rng):
    """_apply_augmentation (dataset.py:115-131) on `rng` (np.random or a RandomState): a draw per flip, one for the brightness
    decision and, when taken, one for the factor.  Returns sample() keywords for the stages after the resize."""
    flip_h = rng.random() < 0.5
    flip_v = rng.random() < 0.5
    factor = None
    if rng.random() < 0.5:
        factor = 0.7 + rng.random() * 0.6
    return dict(post_flip_h=bool(flip_h), post_flip_v=bool(flip_v), value_lut=None if factor is None else value_scale_lut(factor)), factor


def draw_tape_crop(rng, h, w, n_tape, tape_crop_prob=None):
    """advanced_dataset.py:214-215 and :148-162 on `rng`: with tape_crop_prob given, the draw that decides whether the crop
    runs; then, when the mask has tape, randint for the pixel and a draw for the scale.  Returns None (no crop) or
    (k, crop_h, crop_w)."""
    if tape_crop_prob is not None and not rng.random() < tape_crop_prob:
        return None
    if n_tape == 0:
        return None
    k = int(rng.randint(0, n_tape))
    crop_scale = 0.6 + rng.random() * 0.4
    return k, int(h * crop_scale), int(w * crop_scale)


def patch_rect(rng, sample_type, patch_size, sizes, defect_items, bboxes, normal_items):
    """_crop_patch (patch_dataset.py:107-169) on `rng` (the random module or a random.Random): (item, (x1, y1, x2, y2)).
    defect_items / normal_items: item indices in the reference's list order; bboxes: (rmin, rmax, cmin, cmax) per defect item."""
    ps = int(patch_size)
    if sample_type == "defect":
        idx = rng.randint(0, len(defect_items) - 1)
        item = defect_items[idx]
        rmin, rmax, cmin, cmax = (int(v) for v in bboxes[idx])
        center_r, center_c = (rmin + rmax) // 2, (cmin + cmax) // 2
        h, w = sizes[item]
        jitter = ps // 2
        new_r = center_r + rng.randint(-jitter, jitter)
        new_c = center_c + rng.randint(-jitter, jitter)
        new_r = max(ps // 2, min(h - ps // 2, new_r))
        new_c = max(ps // 2, min(w - ps // 2, new_c))
        r1, c1 = new_r - ps // 2, new_c - ps // 2
    else:
        idx = rng.randint(0, len(normal_items) - 1)
        item = normal_items[idx]
        h, w = sizes[item]
        r1 = rng.randint(0, h - ps)
        c1 = rng.randint(0, w - ps)
    h, w = sizes[item]
    # the slices [r1:r1 + ps, c1:c1 + ps] of the reference clip at the image's end
    return item, (c1, r1, min(c1 + ps, w), min(r1 + ps, h))


def draw_patch_augment(rng):
    """_augment (patch_dataset.py:175-195) on `rng`: sample() keywords for the stages before the resize, and (alpha, beta)."""
    flip_h = rng.random() > 0.5
    flip_v = rng.random() > 0.5
    k = 0
    if rng.random() > 0.5:
        k = rng.randint(1, 3)
    ab = None
    if rng.random() > 0.5:
        alpha = rng.uniform(0.8, 1.2)
        beta = rng.randint(-20, 20)
        ab = (alpha, beta)
    return dict(flip_h=bool(flip_h), flip_v=bool(flip_v), rot90=int(k), byte_lut=None if ab is None else convert_scale_abs_lut(*ab)), ab


def draw_patch(rng, sample_type, patch_size, sizes, defect_items, bboxes, normal_items, augment=True):
    """PatchDefectDataset.__getitem__ up to its resize: _crop_patch, then _augment when `augment`.  Returns a sample()."""
    item, rect = patch_rect(rng, sample_type, patch_size, sizes, defect_items, bboxes, normal_items)
    kw = draw_patch_augment(rng)[0] if augment else {}
    return sample(item, rect=rect, **kw)


def defect_bboxes(class_tables, classes=DEFECT_CLASSES):
    """PatchDefectDataset.__init__:49-84 from per-item class tables int [n,>=6,5] (count, x0, y0, x1, y1): (defect_items,
    bboxes (rmin, rmax, cmin, cmax), normal_items)."""
    defect, boxes, normal = [], [], []
    for i, t in enumerate(np.asarray(class_tables)):
        rows = [t[c] for c in classes if t[c][0] > 0]
        if rows:
            r = np.array(rows)
            defect.append(i)
            boxes.append((int(r[:, 2].min()), int(r[:, 4].max()), int(r[:, 1].min()), int(r[:, 3].max())))
        else:
            normal.append(i)
    return defect, boxes, normal


# ---- the device ---------------------------------------------------------------------------------------------------------------------
def layout():
    """(tile_w, tile_h, segment_bytes, plan_columns) of the kernels."""
    import ctypes
    from . import _lib
    v = [ctypes.c_int(0) for _ in range(4)]
    rc = _lib.load().unetpp_train_batch_layout(*[ctypes.byref(x) for x in v])
    if rc != 0:
        raise RuntimeError(f"unetpp_train_batch_layout failed ({rc})")
    return tuple(x.value for x in v)


class TrainSet:
    """The decoded dataset resident on the device: uint8 RGB images [h_i,w_i,3] and masks [h_i,w_i] of any, differing sizes
    packed into two arenas with an item table int64 [n,4] = (image offset, mask offset, h, w).  Per item it keeps the count of
    every class (counts int64 [n,256], which tape_focused needs to draw its pixel) and the bounding box of classes {3,4,5}
    (PatchDefectDataset.__init__:49-84), both from multiclass.class_table on the device with one read-back.  align: the byte
    multiple each item starts at in its arena."""

    def __init__(self, model, images, masks, align=16, device=None):
        import torch
        _check_items(images, masks)
        align = int(align)
        if align < 1:
            raise ValueError("align must be at least 1")
        self.sizes = [tuple(int(v) for v in np.asarray(m).shape) for m in masks]
        items = np.zeros((len(masks), ITEM_COLS), np.int64)
        io = mo = 0
        for i, (h, w) in enumerate(self.sizes):
            io, mo = -(-io // align) * align, -(-mo // align) * align
            items[i] = (io, mo, h, w)
            io, mo = io + 3 * h * w, mo + h * w
        host_i, host_m = np.zeros(io, np.uint8), np.zeros(mo, np.uint8)
        for (o_i, o_m, h, w), im, m in zip(items, images, masks):
            host_i[o_i:o_i + 3 * h * w] = np.ascontiguousarray(im).reshape(-1)
            host_m[o_m:o_m + h * w] = np.ascontiguousarray(m).reshape(-1)
        dev = torch.device(device if device is not None else (f"cuda:{model._device_index}" if model._device_index is not None else "cuda:0"))
        self.model, self.device = model, dev
        self.images, self.masks = torch.from_numpy(host_i).to(dev), torch.from_numpy(host_m).to(dev)
        self.items, self.items_host = torch.from_numpy(items).to(dev), items
        self._stats()

    @classmethod
    def resident(cls, model, dev_images, dev_masks, items_host, dev_items=None, stats=True):
        """A TrainSet over arenas that are on the device already: uint8 CUDA tensors [N] and the item table int64 [n,4] on the
        host (and, if the caller has it there, on the device)."""
        import torch
        self = cls.__new__(cls)
        items = np.ascontiguousarray(items_host, np.int64).reshape(-1, ITEM_COLS)
        for i, (io, mo, h, w) in enumerate(items):
            if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and h * w < 2 ** 31 and 0 <= io <= dev_images.numel() - 3 * h * w and
                    0 <= mo <= dev_masks.numel() - h * w):
                raise ValueError(f"item {i}: {(int(io), int(mo), int(h), int(w))} does not fit the arenas")
        self.model, self.device = model, dev_images.device
        self.images, self.masks, self.items_host = dev_images, dev_masks, items
        self.items = torch.from_numpy(items).to(self.device) if dev_items is None else dev_items
        self.sizes = [(int(h), int(w)) for _, _, h, w in items]
        if stats:
            self._stats()
        return self

    def _stats(self):
        import torch
        from . import multiclass as mc
        tables = [mc.class_table(self.model, self.masks[o_m:o_m + h * w].view(1, h, w)) for _, o_m, h, w in self.items_host.tolist()]
        self.class_tables = torch.cat(tables).cpu().numpy().astype(np.int64)          # the one read-back
        self.counts = self.class_tables[:, :, 0].copy()
        self.defect_items, self.bboxes, self.normal_items = defect_bboxes(self.class_tables)

    def __len__(self):
        return len(self.sizes)


def _dev_table(torch, a, device):
    """A small host table on the device, allocated with torch.empty as every buffer the library is handed."""
    a = np.ascontiguousarray(a)
    t = torch.empty(a.shape, dtype=getattr(torch, a.dtype.name), device=device)
    t.copy_(torch.from_numpy(a))
    return t


def crop_rects(model, trainset, items, k, crop_hw, cls=2):
    """tape_crop_rect_np on the device for B samples: items, k [B] integers, crop_hw [B,2] (or one pair), cls one class or [B]
    -> the rect table int32 [B,6] = (x1, y1, x2, y2, n_found, valid) ON THE DEVICE, which make_batch reads.  One launch (one
    workgroup per sample); nothing is read back."""
    import torch
    items = np.asarray(items, np.int64).reshape(-1)
    b = len(items)
    req = np.zeros((b, REQUEST_COLS), np.int64)
    req[:, 0], req[:, 1] = items, np.broadcast_to(np.asarray(k, np.int64), (b,))
    req[:, 2:4] = np.broadcast_to(np.asarray(crop_hw, np.int64), (b, 2))
    req[:, 4] = np.broadcast_to(np.asarray(cls, np.int64), (b,))
    req = _requests(req, len(trainset))
    masks = model._input(trainset.masks, "trainset.masks", "[N]", "uint8")
    dev_req = _dev_table(torch, req, masks.device)
    out = torch.empty((b, RECT_COLS), dtype=torch.int32, device=masks.device)
    model._call("unetpp_train_crop_rects", masks, masks.numel(), trainset.items, len(trainset), dev_req, b, out, stream_of=masks)
    return out


def make_batch(model, trainset, plan, size_hw, luts=None, class_table=None, rects=None, image_format="chw_f32", channel_order="rgb",
               target_dtype=None):
    """assemble_np on the device: plan int32 [B,16] and luts uint8 [n,256] (build_plan), rects None or the int32 CUDA table of
    crop_rects -> (image, target) on the device, ONE launch on the current stream, nothing read back.  image is float32
    [B,3,H,W], the reference's tensor, or with image_format="hwc_u8" uint8 [B,H,W,3] in channel_order, what segment() and
    evaluate_batches take.  target is uint8 [B,H,W], what loss_grad takes; target_dtype=torch.int64 adds a torch cast."""
    import torch
    luts = np.zeros((0, 256), np.uint8) if luts is None else luts
    if rects is not None and not (isinstance(rects, torch.Tensor) and rects.is_cuda and rects.dtype == torch.int32 and rects.dim() == 2 and
                                  rects.shape[1] == RECT_COLS and rects.is_contiguous()):
        raise RuntimeError(f"rects must be a contiguous int32 CUDA tensor [n,{RECT_COLS}] (crop_rects)")
    plan, luts = check_plan(plan, luts, len(trainset), rects)
    oh, ow = _size(size_hw)
    fmt = _format(image_format, channel_order)
    ctab = None if class_table is None else _table(class_table)
    images = model._input(trainset.images, "trainset.images", "[N]", "uint8")
    masks = model._input(trainset.masks, "trainset.masks", "[N]", "uint8")
    dev = images.device
    b = len(plan)
    # two uploads: the plan; the look-ups with the class table behind them
    dev_plan = _dev_table(torch, plan, dev)
    dev_luts = dev_ctab = None
    if len(luts) or ctab is not None:
        packed = _dev_table(torch, np.concatenate([luts.reshape(-1), ctab if ctab is not None else np.zeros(0, np.uint8)]), dev)
        dev_luts = packed[:luts.size] if len(luts) else None
        dev_ctab = packed[luts.size:] if ctab is not None else None
    image = torch.empty((b, 3, oh, ow), dtype=torch.float32, device=dev) if fmt == 0 else torch.empty((b, oh, ow, 3), dtype=torch.uint8, device=dev)
    target = torch.empty((b, oh, ow), dtype=torch.uint8, device=dev)
    model._call("unetpp_train_batch_u8", images, images.numel(), masks, masks.numel(), trainset.items, len(trainset), dev_plan, b, rects,
                0 if rects is None else int(rects.shape[0]), dev_luts, len(luts), dev_ctab, oh, ow, fmt, image, target,
                stream_of=images)
    if target_dtype is not None and target_dtype != torch.uint8:
        target = target.to(target_dtype)
    return image, target


# ---- iterators that mirror the reference's classes ------------------------------------------------------------------------------------
def _chunks(indices, batch_size):
    indices = list(indices)
    for i in range(0, len(indices), int(batch_size)):
        yield indices[i:i + int(batch_size)]


def cable_defect_batches(model, trainset, size_hw, batch_size, indices=None, augment=False, rng=None, class_table=None, **fmt):
    """CableDefectDataset (and, with class_table, the class maps on top of it) over `indices` (default: every item in order):
    yields (image, target) per batch.  size_hw=None is target_size=None: every item of a batch must then have one size.  The
    draws come from `rng` (default np.random) sample by sample, as a DataLoader without workers makes them."""
    rng = np.random if rng is None else rng
    for chunk in _chunks(range(len(trainset)) if indices is None else indices, batch_size):
        samples = [sample(i, **(draw_cable_defect(rng)[0] if augment else {})) for i in chunk]
        hw = trainset.sizes[chunk[0]] if size_hw is None else size_hw
        if size_hw is None and any(trainset.sizes[i] != hw for i in chunk):
            raise ValueError("size_hw=None needs items of one size in a batch (torch's collate would fail as well)")
        plan, luts = build_plan(samples, trainset.sizes)
        yield make_batch(model, trainset, plan, hw, luts, class_table, **fmt)


def tape_focused_batches(model, trainset, size_hw, batch_size, indices=None, augment=True, tape_crop_prob=0.5, rng=None, class_table=None,
                         cls=2, **fmt):
    """CableDefectDatasetAdvanced's legacy path (advanced_dataset.py:213-263, no hard negatives): the tape-focused crop with
    probability tape_crop_prob, then CableDefectDataset's steps.  The rectangles are found on the device (crop_rects) and read
    by make_batch from the device table."""
    rng = np.random if rng is None else rng
    for chunk in _chunks(range(len(trainset)) if indices is None else indices, batch_size):
        samples, req = [], []
        for i in chunk:
            h, w = trainset.sizes[i]
            crop = draw_tape_crop(rng, h, w, int(trainset.counts[i, cls]), tape_crop_prob) if augment else None
            kw = draw_cable_defect(rng)[0] if augment else {}
            if crop is None or crop[1] < 1 or crop[2] < 1:
                samples.append(sample(i, **kw))
            else:
                samples.append(sample(i, rect_row=len(req), **kw))
                req.append((i, crop[0], crop[1], crop[2]))
        rects = None
        if req:
            r = np.array(req, np.int64)
            rects = crop_rects(model, trainset, r[:, 0], r[:, 1], r[:, 2:4], cls)
        plan, luts = build_plan(samples, trainset.sizes)
        yield make_batch(model, trainset, plan, size_hw, luts, class_table, rects, **fmt)


def patch_defect_batches(model, trainset, sample_types, batch_size, patch_size=640, target_size=None, augment=True, rng=None, **fmt):
    """PatchDefectDataset.__getitem__ over `sample_types` ('defect' / 'normal' per sample, the reference's shuffled
    sample_indices): yields (image, binary target).  The draws come from `rng` (default the random module)."""
    import random as _random
    rng = _random if rng is None else rng
    ts = patch_size if target_size is None else target_size
    hw = (ts, ts) if isinstance(ts, int) else (ts[1], ts[0])           # cv2.resize takes (width, height)
    for chunk in _chunks(sample_types, batch_size):
        samples = [draw_patch(rng, t, patch_size, trainset.sizes, trainset.defect_items, trainset.bboxes, trainset.normal_items, augment)
                   for t in chunk]
        plan, luts = build_plan(samples, trainset.sizes)
        yield make_batch(model, trainset, plan, hw, luts, binary_defect_lut(), **fmt)
