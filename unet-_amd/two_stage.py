"""The two-stage loop's own steps (infer_two_stage_burr.py), in NumPy (torch-free) and on the device (include/unetpp_two_stage.h;
csrc/two_stage.h):
  the two class masks at frame size :303-314, their sums :333-334   -> class_masks_np / class_masks
  visualize_two_stage's four blends :132-153, the burr count :321   -> overlay_np / overlay (overlay_table is the kernel's table)
  cv2.rotate(frame, ROTATE_90_COUNTERCLOCKWISE) :276                -> rotate_np / rotate
  the ratios and the [BURR!] flag :336-342                          -> ratios (host, on a table already read back)
Every device function takes the model and has its NumPy form here; the device results equal them bit for bit.  The whole loop is
frame_loop.process_frames_two_stage; stream.FrameStream overlaps its copies with its compute.

cv2.addWeighted is the restatement multiclass.overlay_np(mode="weighted") uses: float32 a * alpha + b * beta, rounded to nearest
even, saturated.  cv2's own addWeighted stays unpinned, as it is there.  The ROI box, the text and the contour outlines of
visualize_two_stage (cv2.rectangle, putText, findContours / drawContours, :155-168) stay on the host.
"""
from __future__ import annotations

import numpy as np

from . import _lib

CLASS_COLORS = {1: (0, 255, 0), 2: (255, 0, 0), 3: (255, 0, 255)}       # BGR: cable, tape, burr (infer_two_stage_burr.py:22-27)
WEIGHTS = ((0.7, 0.3), (0.6, 0.4), (0.6, 0.4), (0.5, 0.5))              # the ROI dimming, then cable, tape, burr (:141, :151-153)
ROTATE_CODES = _lib.ROTATE_CODES                                        # name -> cv2's / UNETPP_ROTATE_* number
N_STATES = 16                                                           # 8 inside + 4 cable + 2 tape + burr


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _check_roi(roi, h, w):
    """(x1, y1, x2, y2) as the slice [y1:y2, x1:x2] takes it for non-negative bounds; None is the whole frame."""
    if roi is None:
        return 0, 0, int(w), int(h)
    x1, y1, x2, y2 = (int(v) for v in roi)
    if min(x1, y1, x2, y2) < 0:
        raise ValueError(f"roi (x1, y1, x2, y2) = {(x1, y1, x2, y2)} has a negative bound")
    return x1, y1, x2, y2


def roi_area(roi):
    """(x2 - x1) * (y2 - y1) of :336, as the reference forms it (no clamp to the frame)."""
    x1, y1, x2, y2 = (int(v) for v in roi)
    return (x2 - x1) * (y2 - y1)


def _check_colors(colors):
    colors = CLASS_COLORS if colors is None else colors
    out = []
    for cid in (1, 2, 3):
        col = tuple(int(v) for v in colors[cid])
        if len(col) != 3 or any(not 0 <= v <= 255 for v in col):
            raise ValueError(f"colour {cid}: {colors[cid]!r} is not three values 0..255")
        out.append(col)
    return tuple(out)


def _check_weights(weights):
    weights = WEIGHTS if weights is None else weights
    out = tuple((float(a), float(b)) for a, b in weights)
    if len(out) != 4 or any(v != v for p in out for v in p):
        raise ValueError("weights must be four (alpha, beta) pairs of numbers: the ROI dimming, cable, tape, burr")
    return out


def _check_code(code):
    code = ROTATE_CODES.get(code, code) if isinstance(code, str) else code
    if code not in (0, 1, 2) or isinstance(code, bool):
        raise ValueError(f"code must be 0 (90 degrees clockwise), 1 (180) or 2 (90 counter-clockwise) or one of {sorted(ROTATE_CODES)}, got {code!r}")
    return int(code)


# ---- the NumPy forms ---------------------------------------------------------------------------------------------------------------
def nearest_index(n_dst, n_src):
    """resizeNN's source index per destination index: min(floor(d * (1 / (n_dst / n_src))), n_src - 1) in double."""
    ifx = np.float64(1.0) / (np.float64(n_dst) / np.float64(n_src))
    return np.minimum(np.floor(np.arange(n_dst, dtype=np.float64) * ifx).astype(np.int64), n_src - 1)


def class_masks_np(pred, frame_size_wh, roi=None):
    """:303-314 and :333-334 for pred uint8 [B,th,tw]: (mask_cable, mask_tape uint8 0/1 [B,fh,fw], counts int64 [B,2]).
    (pred == 1) and (pred == 2), cv2.resize(INTER_NEAREST) to frame_size_wh = (width, height), zeros outside
    roi = (x1, y1, x2, y2) (None: no clip; an empty ROI gives zero masks)."""
    pred = np.asarray(pred)
    if pred.dtype != np.uint8 or pred.ndim != 3:
        raise ValueError(f"pred must be uint8 [B,H,W], got {pred.dtype} {list(pred.shape)}")
    fw, fh = int(frame_size_wh[0]), int(frame_size_wh[1])
    if fw < 1 or fh < 1:
        raise ValueError(f"frame_size_wh must be positive, got {frame_size_wh!r}")
    x1, y1, x2, y2 = _check_roi(roi, fh, fw)
    full = pred[:, nearest_index(fh, pred.shape[1])][:, :, nearest_index(fw, pred.shape[2])]
    out = []
    for c in (1, 2):
        m = np.zeros(full.shape, np.uint8)
        m[:, y1:y2, x1:x2] = (full == c)[:, y1:y2, x1:x2]
        out.append(m)
    counts = np.stack([out[0].sum(axis=(1, 2), dtype=np.int64), out[1].sum(axis=(1, 2), dtype=np.int64)], axis=1)
    return out[0], out[1], counts


def add_weighted_np(a, alpha, b, beta):
    """cv2.addWeighted(a, alpha, b, beta, 0) for uint8 arrays as the project restates it (module docstring)."""
    v = np.asarray(a).astype(np.float32) * np.float32(alpha) + np.asarray(b).astype(np.float32) * np.float32(beta)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def overlay_np(frames, cable, tape, burr, roi=None, colors=None, weights=None):
    """visualize_two_stage :132-153 for uint8 BGR frames [B,H,W,3] and three uint8 masks [B,H,W] (non-zero = set): (result uint8
    [B,H,W,3], burr pixels int64 [B]).  Four addWeighted passes over every pixel: weights[0] against the frame blacked outside roi,
    then weights[1..3] against a zero image carrying colors[1], [2], [3] under the cable, the tape, the burr."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be uint8 [B,H,W,3], got {frames.dtype} {list(frames.shape)}")
    masks = [np.asarray(m) for m in (cable, tape, burr)]
    for m, what in zip(masks, ("cable", "tape", "burr")):
        if m.dtype != np.uint8 or m.shape != frames.shape[:3]:
            raise ValueError(f"{what} must be uint8 {list(frames.shape[:3])} like the frames, got {m.dtype} {list(m.shape)}")
    b, h, w = frames.shape[:3]
    x1, y1, x2, y2 = _check_roi(roi, h, w)
    cols, wts = _check_colors(colors), _check_weights(weights)
    dimmed = np.zeros_like(frames)
    dimmed[:, y1:y2, x1:x2] = frames[:, y1:y2, x1:x2]
    result = add_weighted_np(frames, wts[0][0], dimmed, wts[0][1])
    for m, col, (alpha, beta) in zip(masks, cols, wts[1:]):
        layer = np.zeros_like(frames)
        layer[m > 0] = col
        result = add_weighted_np(result, alpha, layer, beta)
    return result, np.count_nonzero(masks[2], axis=(1, 2)).astype(np.int64)


def overlay_table(colors=None, weights=None):
    """uint8 [16,3,256]: table[state, channel, v] = what overlay_np makes of byte v in `channel` of a pixel in `state` =
    8 * inside the ROI + 4 * cable + 2 * tape + burr.  Built by running overlay_np itself on a 16 x 256 frame whose row is the
    state and whose column is the byte, so the device holds no arithmetic of its own."""
    frames = np.empty((1, N_STATES, 256, 3), np.uint8)
    frames[0, :, :, :] = np.arange(256, dtype=np.uint8)[None, :, None]
    state = np.arange(N_STATES)[:, None].repeat(256, axis=1)
    masks = [((state >> bit) & 1).astype(np.uint8)[None] for bit in (2, 1, 0)]
    out, _ = overlay_np(frames, masks[0], masks[1], masks[2], (0, 8, 256, N_STATES), colors, weights)      # rows 8..15 lie inside
    return np.ascontiguousarray(out[0].transpose(0, 2, 1))


def overlay_states_np(shape_hw, cable, tape, burr, roi=None):
    """uint8 [B,H,W]: the state of every pixel, as overlay_table and the kernel number them."""
    h, w = int(shape_hw[0]), int(shape_hw[1])
    x1, y1, x2, y2 = _check_roi(roi, h, w)
    inside = np.zeros((h, w), np.uint8)
    inside[y1:y2, x1:x2] = 1
    return (8 * inside[None] + 4 * (np.asarray(cable) > 0) + 2 * (np.asarray(tape) > 0) + (np.asarray(burr) > 0)).astype(np.uint8)


def rotate_np(frames, code):
    """cv2.rotate(frame, code) for uint8 [B,H,W,C]: code 0 a quarter turn clockwise, 1 a half turn, 2 a quarter turn
    counter-clockwise (cv2's numbering; the names of ROTATE_CODES are taken too)."""
    frames = np.asarray(frames)
    if frames.ndim != 4:
        raise ValueError(f"frames must be [B,H,W,C], got {list(frames.shape)}")
    code = _check_code(code)
    if code == 0:
        out = frames[:, ::-1].transpose(0, 2, 1, 3)             # out[y, x] = in[H - 1 - x, y]
    elif code == 1:
        out = frames[:, ::-1, ::-1]
    else:
        out = frames[:, :, ::-1].transpose(0, 2, 1, 3)          # out[y, x] = in[x, W - 1 - y]
    return np.ascontiguousarray(out)


def ratios(counts, roi_area):
    """:338-342 on the host for counts [B,3] (cable, tape, burr pixels; an array already read back, or anything np.asarray
    takes) and roi_area: a list of B dicts with cable_ratio, tape_ratio, burr_ratio in percent (0 when roi_area <= 0) and
    burr = burr pixels > 0, status "[BURR!]" or "[OK]"."""
    rows = np.asarray(counts).reshape(-1, 3).tolist()
    area = int(roi_area)
    pct = (lambda n: n / area * 100) if area > 0 else (lambda n: 0)
    return [{"cable_ratio": pct(c), "tape_ratio": pct(t), "burr_ratio": pct(b), "burr": b > 0, "status": "[BURR!]" if b > 0 else "[OK]"}
            for c, t, b in rows]


# ---- seeded inputs of the fixture and the tests --------------------------------------------------------------------------------------
FIXTURE_SCENES = (("a", 37, 53, 0, 1), ("b", 16, 64, 1, 255), ("c", 48, 40, 2, 1))     # (tag, height, width, seed, mask value)


def make_scene(h, w, seed, value=1):
    """(frame uint8 [h,w,3], cable, tape, burr uint8 [h,w] with `value` where set, roi): a smooth coloured frame with noise and a
    few 0 / 255, a cable band, a tape band that crosses it, burr blobs on all of them, and a ROI strictly inside the frame that
    every mask crosses -- so all 16 states of the overlay occur."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 120 + 80 * np.sin(x / 5.0 + seed) * np.cos(y / 4.0)
    frame = np.clip(np.stack([base + 30 * c + r.normal(0, 12, (h, w)) for c in (-1, 0, 1)], axis=-1), 0, 255).astype(np.uint8)
    flat = frame.reshape(-1)
    flat[r.integers(0, flat.size, 6)] = 255
    flat[r.integers(0, flat.size, 6)] = 0
    roi = (w // 5, h // 6, w // 2 + 1, h - h // 5)                # the cable's right half and its crossing with the tape lie outside
    cable = (np.abs(x - w // 2 - (y - h // 2) // 4) <= max(w // 6, 2))
    tape = (np.abs(y - h // 2) <= max(h // 5, 2)) & (x >= w // 10)
    burr = ((x // 3 + y // 2) % 4 == 0) & ((x + 2 * y) % 3 != 0)
    return frame, (cable * value).astype(np.uint8), (tape * value).astype(np.uint8), (burr * value).astype(np.uint8), roi


# ---- the device path (torch imported lazily, as in raw_frames.py) --------------------------------------------------------------------------
def class_masks(model, pred, frame_size_wh, roi=None):
    """class_masks_np on the device for a uint8 CUDA tensor [B,th,tw] (segment()'s class map), ONE launch that reads pred once:
    (mask_cable, mask_tape uint8 0/1 [B,fh,fw], counts int64 [B,2]), all on the device.  Bit for bit two
    model.resize_masks(pred, frame_size_wh, match_class=c, roi=roi) calls and their sums."""
    import torch
    pred = model._input(pred, "pred")
    b, th, tw = (int(v) for v in pred.shape)
    fw, fh = int(frame_size_wh[0]), int(frame_size_wh[1])
    if fw < 1 or fh < 1:
        raise ValueError(f"frame_size_wh must be positive, got {frame_size_wh!r}")
    x1, y1, x2, y2 = _check_roi(roi, fh, fw)
    cable = torch.empty((b, fh, fw), dtype=torch.uint8, device=pred.device)
    tape = torch.empty((b, fh, fw), dtype=torch.uint8, device=pred.device)
    counts = torch.empty((b, 2), dtype=torch.int64, device=pred.device)
    model._call("unetpp_two_stage_masks_u8", pred, b, th, tw, cable, tape, fh, fw, x1, y1, x2, y2, counts, stream_of=pred)
    return cable, tape, counts


_TABLES = {}                                                            # (colours, weights) -> the host table
_DEFAULT_KEY = (tuple(CLASS_COLORS[c] for c in (1, 2, 3)), WEIGHTS)


def _device_table(model, colors, weights, device):
    """The look-up table on the device, uploaded once per (colours, weights) and kept with the model's scratch buffers."""
    import torch
    key = _DEFAULT_KEY if colors is None and weights is None else (_check_colors(colors), _check_weights(weights))
    cached = model._cc_workspaces.get(("two_stage_table",) + key)
    if cached is None or cached.device != device:
        if key not in _TABLES:
            _TABLES[key] = overlay_table(dict(zip((1, 2, 3), key[0])), key[1])
        cached = torch.empty((N_STATES, 3, 256), dtype=torch.uint8, device=device)
        cached.copy_(torch.from_numpy(_TABLES[key]))
        model._cc_workspaces[("two_stage_table",) + key] = cached
    return cached


def overlay(model, frames, cable, tape, burr, roi=None, *, colors=None, weights=None):
    """overlay_np on the device for uint8 CUDA frames [B,H,W,3] (BGR) and three uint8 masks [B,H,W] (non-zero = set): (result uint8
    [B,H,W,3], burr pixels int64 [B]), ONE launch of look-ups in overlay_table(colors, weights) that reads 6 bytes per pixel and
    writes 3.  colors {1: cable, 2: tape, 3: burr} as (b, g, r) and weights, four (alpha, beta) pairs, default to the reference's.
    cv2.rectangle, putText and findContours / drawContours (:155-168) stay on the host."""
    import torch
    frames = model._input(frames, "frames", "[B,H,W,3]")
    b, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    planes = []
    for t, what in ((cable, "cable"), (tape, "tape"), (burr, "burr")):
        t = model._input(t, what)
        if tuple(t.shape) != (b, h, w):
            raise RuntimeError(f"{what} {tuple(t.shape)} does not match the frames {(b, h, w)}")
        planes.append(t)
    x1, y1, x2, y2 = _check_roi(roi, h, w)
    table = _device_table(model, colors, weights, frames.device)
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=frames.device)
    count = torch.empty((b,), dtype=torch.int64, device=frames.device)
    model._call("unetpp_two_stage_overlay_u8", frames, planes[0], planes[1], planes[2], b, h, w, x1, y1, x2, y2, table, out, count, stream_of=frames)
    return out, count


def rotate(model, frames, code):
    """rotate_np on the device for a uint8 CUDA tensor [B,H,W,C], C 1 or 3: tile transposes through LDS, one launch."""
    import torch
    code = _check_code(code)
    frames = model._input(frames, "frames", "[B,H,W,C]")
    b, h, w, c = (int(v) for v in frames.shape)
    if c not in (1, 3):
        raise ValueError(f"frames have {c} channels, 1 or 3 are supported")
    oh, ow = (h, w) if code == 1 else (w, h)
    out = torch.empty((b, oh, ow, c), dtype=torch.uint8, device=frames.device)
    model._call("unetpp_rotate_u8", frames, b, h, w, c, code, out, stream_of=frames)
    return out
