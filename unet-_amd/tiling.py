"""Sliding-window inference: the host plan and the CPU restatement (NumPy only) of what the device does in
unetpp_tile_gather_u8, unetpp_tile_blend_f32 and unetpp_tile_gate_f32 (include/unetpp.h), i.e. of
  SlidingWindowInference.predict            tools/inference_binary_patch.py:19-115      (logits are blended)
  OptimizedSlidingWindowInference.predict   tools/inference_binary_optimized.py:21-113  (softmax maps, patch gate)
Both cut the image into patch_size squares at `stride`, resize each to target_size for the network, resize the
network's map back to patch_size, sum the maps into a full-size array in patch order, divide by the cover count and
(the first one) take the argmax.

Importable without a GPU.  The two resizes are cv2.resize(..., INTER_LINEAR) restated from OpenCV's published code:
the uint8 one with 11-bit fixed-point coefficients (as unetpp_resize_linear_u8), the float32 one with the float
coefficients 1 - fx and fx, horizontal pass S[s0] * a0 + S[s1] * a1 first, then the vertical pass, every product and
sum rounded to float32.  cv2 is not installed where this project is built and tested, so cv2's own float resize
(the order of its SIMD paths) stays unpinned; what the tests pin is the composition, on the
reference's own predict run over these restatements.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

MAX_AXIS = 64           # patch origins per axis the device kernels take
MAX_CLASSES = 8         # the engine's limit
BLENDS = ("logits", "probs")
CHANNEL_ORDERS = {"bgr": 0, "rgb": 1}


class TilePlan(NamedTuple):
    """Patch origins per axis; patch (i, j) has its top-left corner at (ys[i], xs[j]) and index i * len(xs) + j."""
    ys: tuple
    xs: tuple

    @property
    def n_patches(self):
        return len(self.ys) * len(self.xs)

    @property
    def origins(self):
        """[(y, x)] in the reference's loop order: i outer, j inner."""
        return [(y, x) for y in self.ys for x in self.xs]


def _axis_origins(n, patch_size, stride):
    """One axis of predict (inference_binary_patch.py:41-48, :59-68): the count with its + 1 for a non-zero remainder
    (Python's floor division and modulo, also below zero), each origin clamped to max(0, end - patch_size)."""
    count = (n - patch_size) // stride + 1
    if (n - patch_size) % stride != 0:
        count += 1
    out = []
    for i in range(count):
        end = min(i * stride + patch_size, n)
        out.append(max(0, end - patch_size))
    return tuple(out)


def tile_plan(h, w, patch_size=384, stride=192):
    """The patches predict visits for an h x w image.  An axis shorter than the patch gives one patch (reflect
    padding) when (n - patch_size) % stride != 0 and none when it is 0, as the reference's arithmetic does."""
    h, w, patch_size, stride = int(h), int(w), int(patch_size), int(stride)
    if h < 1 or w < 1 or patch_size < 1:
        raise ValueError(f"bad plan {h}x{w}, patch_size {patch_size}")
    if stride < 1:
        raise ValueError(f"stride must be at least 1, got {stride}")
    return TilePlan(_axis_origins(h, patch_size, stride), _axis_origins(w, patch_size, stride))


# ---- cv2.resize(..., INTER_LINEAR) ------------------------------------------------------------------------------------
def linear_index_tables(n_src, n_dst):
    """resizeGeneric_'s source index and fraction per destination index: fx = (float)((d + 0.5) * scale - 0.5) with
    scale = 1 / (n_dst / n_src) in double, s0 = floor(fx), fx -= s0, both clamped at the borders with fx = 0.
    Returns (s0 int32, s1 = min(s0 + 1, n_src - 1) int32, fx float32)."""
    inv_scale = np.float64(n_dst) / np.float64(n_src)
    scale = np.float64(1.0) / inv_scale
    d = np.arange(n_dst, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(fx).astype(np.int32)
    fx = (fx - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    fx[lo] = 0.0; s[lo] = 0
    hi = s >= n_src - 1
    fx[hi] = 0.0; s[hi] = n_src - 1
    return s, np.minimum(s + 1, n_src - 1).astype(np.int32), fx


def linear_tables_f32(n_src, n_dst):
    """(s0, s1, a0 = 1 - fx, a1 = fx) with float32 coefficients: the tables of the float32 resize."""
    s0, s1, fx = linear_index_tables(n_src, n_dst)
    return s0, s1, (np.float32(1.0) - fx).astype(np.float32), fx


def linear_tables_u8(n_src, n_dst):
    """(s0, s1, a0, a1) with the coefficients saturate_cast<short>(c * 2048), round-half-even: the uint8 resize."""
    s0, s1, fx = linear_index_tables(n_src, n_dst)
    c0 = (np.float32(1.0) - fx).astype(np.float32) * np.float32(2048)
    c1 = fx * np.float32(2048)
    a0 = np.clip(np.rint(c0), -32768, 32767).astype(np.int32)
    a1 = np.clip(np.rint(c1), -32768, 32767).astype(np.int32)
    return s0, s1, a0, a1


def resize_linear_f32_np(img, dsize):
    """cv2.resize(img, (dst_w, dst_h), interpolation=cv2.INTER_LINEAR) for float32 [H,W,C] (or [H,W]) as the module
    docstring states it.  At equal size every coefficient pair is (1, 0) and the result equals the input."""
    dw, dh = int(dsize[0]), int(dsize[1])
    x = np.asarray(img)
    if x.dtype != np.float32 or x.ndim not in (2, 3):
        raise ValueError("img must be float32 [H,W] or [H,W,C]")
    flat = x.ndim == 2
    if flat:
        x = x[:, :, None]
    xs0, xs1, xa0, xa1 = linear_tables_f32(x.shape[1], dw)
    ys0, ys1, yb0, yb1 = linear_tables_f32(x.shape[0], dh)
    hrow = x[:, xs0, :] * xa0[None, :, None] + x[:, xs1, :] * xa1[None, :, None]          # [H, dw, C]
    out = hrow[ys0] * yb0[:, None, None] + hrow[ys1] * yb1[:, None, None]
    out = np.ascontiguousarray(out, dtype=np.float32)
    return out[:, :, 0] if flat else out


def resize_linear_u8_np(img, dsize):
    """cv2.resize(img, (dst_w, dst_h), interpolation=cv2.INTER_LINEAR) for uint8 [H,W,C]: what unetpp_resize_linear_u8
    computes (horizontal pass in int32, vertical pass (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2)."""
    dw, dh = int(dsize[0]), int(dsize[1])
    x = np.asarray(img)
    if x.dtype != np.uint8 or x.ndim != 3:
        raise ValueError("img must be uint8 [H,W,C]")
    xs0, xs1, xa0, xa1 = linear_tables_u8(x.shape[1], dw)
    ys0, ys1, yb0, yb1 = linear_tables_u8(x.shape[0], dh)
    xi = x.astype(np.int32)
    hrow = xi[:, xs0, :] * xa0[None, :, None] + xi[:, xs1, :] * xa1[None, :, None]
    out = (((yb0[:, None, None] * (hrow[ys0] >> 4)) >> 16) + ((yb1[:, None, None] * (hrow[ys1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- the three device steps ---------------------------------------------------------------------------------------------
def check_padding(h, w, patch_size):
    """np.pad(mode="reflect") of predict mirrors once for a pad below the axis length; the device kernel takes that
    case only (a longer pad is what unetpp_tile_gather_u8 answers with UNETPP_E_UNSUPPORTED)."""
    for n in (h, w):
        if patch_size > n and patch_size - n >= n:
            raise ValueError(f"unsupported: reflect padding of {patch_size - n} on an axis of {n} (must be below the axis length)")


def gather_tiles_np(image_u8, plan, patch_size, target_size, channel_order="rgb"):
    """The patches predict feeds the network, for one uint8 image [H,W,3]: crop at each origin, reflect padding at the
    bottom and right, uint8 resize to target_size.  Returns uint8 [P,T,T,3] in BGR, the engine's uint8 input order:
    channel_order="rgb" (the reference's predict gets RGB) reverses the channels, "bgr" keeps them."""
    if channel_order not in CHANNEL_ORDERS:
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
    img = np.asarray(image_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("image must be uint8 [H,W,3]")
    h, w = img.shape[:2]
    check_padding(h, w, patch_size)
    out = np.zeros((plan.n_patches, target_size, target_size, 3), np.uint8)
    for n, (y, x) in enumerate(plan.origins):
        patch = img[y:min(y + patch_size, h), x:min(x + patch_size, w)]
        if patch.shape[0] != patch_size or patch.shape[1] != patch_size:
            patch = np.pad(patch, ((0, patch_size - patch.shape[0]), (0, patch_size - patch.shape[1]), (0, 0)), mode="reflect")
        r = resize_linear_u8_np(patch, (target_size, target_size))
        out[n] = r[..., ::-1] if channel_order == "rgb" else r
    return out


def tile_gate_np(maps, gate_thr, gate_class=1):
    """The window gate of inference_binary_optimized.py:91-98 for maps float32 [N,C,T,T]: (include bool [N], scores
    float32 [N]) with score = max over the patch of class gate_class and include = score >= float32(gate_thr)."""
    maps = np.asarray(maps, dtype=np.float32)
    if not 0 <= int(gate_class) < maps.shape[1]:
        raise ValueError(f"gate_class {gate_class} not in [0,{maps.shape[1]})")
    scores = maps[:, int(gate_class)].reshape(len(maps), -1).max(axis=1)
    return scores >= np.float32(gate_thr), scores


def blend_tiles_np(maps, plan, h, w, patch_size, include=None):
    """The fold of predict for one image: maps float32 [P,C,T,T] in plan order -> (mask uint8 [h,w], output float32
    [h,w,C]).  Each map goes HWC, is resized to patch_size, cropped to the image and added in patch order; patches
    whose `include` is false are skipped; output / (count + 1e-8) in float32; np.argmax (first maximum)."""
    maps = np.asarray(maps)
    if maps.dtype != np.float32 or maps.ndim != 4 or maps.shape[0] != plan.n_patches or maps.shape[2] != maps.shape[3]:
        raise ValueError(f"maps must be float32 [{plan.n_patches},C,T,T], got {maps.dtype} {maps.shape}")
    c = maps.shape[1]
    output = np.zeros((h, w, c), np.float32)
    count = np.zeros((h, w, 1), np.float32)
    for n, (y, x) in enumerate(plan.origins):
        if include is not None and not include[n]:
            continue
        y_end, x_end = min(y + patch_size, h), min(x + patch_size, w)
        pred = resize_linear_f32_np(np.ascontiguousarray(maps[n].transpose(1, 2, 0)), (patch_size, patch_size))
        output[y:y_end, x:x_end] += pred[:y_end - y, :x_end - x]
        count[y:y_end, x:x_end] += 1
    output = output / (count + np.float32(1e-8))
    return np.argmax(output, axis=-1).astype(np.uint8), output


def predict_tiled_np(image_u8, model_fn, patch_size=384, stride=192, target_size=256, num_classes=2, blend="logits",
                     gate_thr=None, gate_class=1, channel_order="rgb"):
    """The whole of predict for one uint8 image [H,W,3].  model_fn maps the patch batch (uint8 [P,T,T,3] BGR, see
    gather_tiles_np) to the maps that are blended, float32 [P,num_classes,T,T]: logits for blend="logits", softmax
    probabilities for blend="probs".  gate_thr (blend="probs" only; None is use_gating=False) drops the patches whose
    gate score is below it.  Returns (mask uint8 [H,W], output float32 [H,W,C]); a plan with no patch gives zeros."""
    if blend not in BLENDS:
        raise ValueError(f"blend must be 'logits' or 'probs', got {blend!r}")
    if gate_thr is not None and blend != "probs":
        raise ValueError("gate_thr needs blend='probs': the gate score is a probability")
    h, w = np.asarray(image_u8).shape[:2]
    plan = tile_plan(h, w, patch_size, stride)
    if plan.n_patches == 0:
        return np.zeros((h, w), np.uint8), np.zeros((h, w, num_classes), np.float32)
    maps = np.asarray(model_fn(gather_tiles_np(image_u8, plan, patch_size, target_size, channel_order)), dtype=np.float32)
    if maps.shape != (plan.n_patches, num_classes, target_size, target_size):
        raise ValueError(f"model_fn returned {maps.shape}, expected {(plan.n_patches, num_classes, target_size, target_size)}")
    include = None if gate_thr is None else tile_gate_np(maps, gate_thr, gate_class)[0]
    return blend_tiles_np(maps, plan, h, w, patch_size, include)
