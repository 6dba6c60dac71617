"""Validation losses: the five sums per frame and class that every loss of the reference's src/models/losses.py is a
function of, in NumPy (torch-free) and on the device (include/unetpp_loss.h, unetpp_loss_sums_f32; csrc/loss.h), and the
losses themselves as float64 algebra on that table.

The reference's CombinedLoss (cross-entropy + Dice) and AdvancedCombinedLoss (Focal + Tversky + Dice) decide checkpoint
selection and early stopping in every tools/train*.py; with deep supervision they are applied to each of
[out, out1, out2, out3].  In torch they take a softmax, a one-hot the size of the logits, a second log_softmax and a dozen
full-size temporaries.  With p = softmax over the classes and nll = -log p[target] per pixel, all of them follow from
  table[n, c] = (T, P, I, NLL, FOC)      uint64 [B,C,5]
    T    pixels with target c (an integer)
    P    sum over all pixels of p_c,                         in units of 2^-32
    I    sum over the pixels with target c of p_c,           in units of 2^-32
    NLL  sum over the pixels with target c of nll,           in units of 2^-24
    FOC  sum over the pixels with target c of (1 - p_c)^gamma nll,  in units of 2^-24
  outside[n] = (pixels with target >= C, the remaining pixels with a non-finite logit)      uint32 [B,2]
Both kinds of pixel stay out of every sum, and table[n, :, 0].sum() + outside[n].sum() == H W.

Per pixel, in float32 without contraction and in this order (x_c the logits):
  m = max_c x_c;  d_c = x_c - m;  e_c = exp32(d_c);  s = e_0 + e_1 + ... (class order);  p_c = e_c / s
  nll = max(0, log32(s) - d_t);  foc = (1 - p_t)^gamma nll      ((.)^gamma by repeated multiplication, gamma 0..4)
P and I add floor(p 2^32); NLL and FOC add rint(min(v, 131072) 2^24), round-to-nearest-even: truncation there is a bias of
2^-25 per pixel, 1.2e-7 of a cross-entropy of 0.24, more than the reference's own float32 noise (tests/golden/README_loss.txt).
Sums of integers: no result depends on the order
in which threads arrive, and a frame's row is the same in any batch.  exp32 and log32 are the Cephes single-precision forms
written as explicit float32 operations (exp32_np, log32_np), so that NumPy performs the same operations as the kernel and
loss_sums_np returns the same bits as loss_sums.

A table of several frames is ONE batch in the reference's sense.  Cross-entropy and Focal are means over pixels and do not
care where a batch ends; Dice and Tversky average a ratio over (n, c), Dice's skip_empty and its all-empty fallback look at
the whole batch, so the losses of two batches are not the loss of their union: pass the frames of one reference batch
together (evaluate_losses keeps the batches apart and averages their losses, as the reference's validation loops do).

The functions take the model, as evaluation.py and roi_loop.py do.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np

MIN_CLASSES, MAX_CLASSES = 2, 8                 # the engine's HEAD_FUSED_MAX_CLASSES
MAX_GAMMA = 4
MAX_PIXELS = 1 << 22                            # H W: with it no column can overflow 64 bits (csrc/loss.h)
COLUMNS = ("T", "P", "I", "NLL", "FOC")
P_SCALE, V_SCALE, V_CLAMP = 2.0 ** 32, 2.0 ** 24, 131072.0
LOSSES = ("ce", "dice", "focal", "tversky", "combined", "advanced")

_f = np.float32


# ---- argument checks shared by the NumPy and the device forms (they look only at .shape and .dtype) -------------------------
def _dtype_name(a):
    return str(a.dtype).rsplit(".", 1)[-1]


def check_args(logits, target, gamma=2):
    """(B, C, H, W, gamma).  ValueError unless logits are float32 [B,C,H,W] with C in 2..8, target is uint8 [B,H,W] of the
    same B, H, W, 1 <= B <= 65535, H W <= 2^22 and gamma is an integer in 0..4."""
    if _dtype_name(logits) != "float32" or len(logits.shape) != 4:
        raise ValueError(f"logits must be float32 [B,C,H,W], got {_dtype_name(logits)} {list(logits.shape)}")
    if _dtype_name(target) != "uint8" or len(target.shape) != 3:
        raise ValueError(f"target must be uint8 [B,H,W], got {_dtype_name(target)} {list(target.shape)}")
    b, c, h, w = (int(v) for v in logits.shape)
    if tuple(int(v) for v in target.shape) != (b, h, w):
        raise ValueError(f"logits are {list(logits.shape)}, target is {list(target.shape)}: B, H and W must be equal")
    if not MIN_CLASSES <= c <= MAX_CLASSES:
        raise ValueError(f"logits have {c} classes: the kernel takes {MIN_CLASSES}..{MAX_CLASSES}")
    if not 1 <= b <= 65535 or h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise ValueError(f"logits are {list(logits.shape)}: needs 1 <= B <= 65535, H, W >= 1 and H W <= 2^22")
    if isinstance(gamma, bool) or int(gamma) != gamma or not 0 <= int(gamma) <= MAX_GAMMA:
        raise ValueError(f"gamma must be an integer in 0..{MAX_GAMMA}, got {gamma!r}")
    return b, c, h, w, int(gamma)


# ---- exp and log as explicit float32 operations ------------------------------------------------------------------------------
EXP_MIN = _f(-87.0)
LOG2E, EXP_C1, EXP_C2 = _f(1.44269504088896341), _f(0.693359375), _f(-2.12194440e-4)
EXP_POLY = tuple(_f(v) for v in (1.9875691500e-4, 1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1))
SQRTH = _f(0.70710678118654752440)
LOG_POLY = tuple(_f(v) for v in (7.0376836292e-2, -1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1,
                                 -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1, 3.3333331174e-1))


def exp32_np(d):
    """exp(d) for float32 d <= 0, every operation a float32 operation in the kernel's order (Cephes expf): 0 for d < -87;
    otherwise n = rint(d log2 e), r = (d - n C1) - n C2 with ln 2 = C1 + C2, a degree-5 polynomial in Horner form,
    (poly r^2 + r) + 1, scaled by 2^n (exact: the result is a normal number)."""
    d = np.asarray(d, _f)
    x = np.maximum(d, EXP_MIN)
    n = np.rint(LOG2E * x)
    r = x - n * EXP_C1
    r = r - n * EXP_C2
    q = EXP_POLY[0]
    for k in EXP_POLY[1:]:
        q = q * r + k
    y = q * (r * r) + r
    y = y + _f(1.0)
    return np.where(d < EXP_MIN, _f(0.0), np.ldexp(y, n.astype(np.int32))).astype(_f)


def log32_np(s):
    """log(s) for float32 s >= 1, every operation a float32 operation in the kernel's order (Cephes logf): s = f 2^e with f
    in [0.5, 1) (frexp); f < sqrt(1/2): e -= 1, x = (f + f) - 1, else x = f - 1; a degree-8 polynomial in Horner form;
    y = poly x x^2 + e C2 - 0.5 x^2; (x + y) + e C1.  log32_np(1) == 0."""
    s = np.asarray(s, _f)
    f, e = np.frexp(s)
    low = f < SQRTH
    fe = (e - low).astype(_f)
    x = np.where(low, f + f, f) - _f(1.0)
    z = x * x
    q = LOG_POLY[0]
    for k in LOG_POLY[1:]:
        q = q * x + k
    y = q * x * z
    y = y + EXP_C2 * fe
    y = y + _f(-0.5) * z
    r = x + y
    return (r + EXP_C1 * fe).astype(_f)


def ulp_error(got, want64):
    """The largest |got - want| in units of the float32 spacing at |want| (want in float64)."""
    want64 = np.asarray(want64, np.float64)
    ulp = np.spacing(np.abs(want64).astype(_f)).astype(np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want64) / ulp).max())


# ---- the NumPy form of the kernel ---------------------------------------------------------------------------------------------
def pixel_terms_np(logits, target, gamma=2):
    """Per pixel, with the kernel's arithmetic: (p float32 [B,C,H W], nll, foc float32 [B,H W], t int64 [B,H W],
    kind uint8 [B,H W]: 0 a pixel of the sums, 1 target >= C, 2 a non-finite logit).  Pixels of kind 1 and 2 are
    computed on logits 0 and target 0 and mean nothing."""
    logits, target = np.asarray(logits), np.asarray(target)
    b, c, h, w, gamma = check_args(logits, target, gamma)
    x = logits.reshape(b, c, h * w)
    t = target.reshape(b, h * w).astype(np.int64)
    kind = np.where(t >= c, 1, np.where(~np.isfinite(x).all(1), 2, 0)).astype(np.uint8)
    x = np.where((kind != 0)[:, None, :], _f(0.0), x)
    t = np.where(kind != 0, 0, t)
    with np.errstate(over="ignore", invalid="ignore"):
        m = x[:, 0]
        for k in range(1, c):
            m = np.where(x[:, k] > m, x[:, k], m)
        d = x - m[:, None, :]                                    # -inf where the difference leaves float32: exp32 gives 0
        e = exp32_np(d)
        s = e[:, 0]
        for k in range(1, c):
            s = s + e[:, k]
        p = e / s[:, None, :]
        d_t = np.take_along_axis(d, t[:, None, :], 1)[:, 0]
        p_t = np.take_along_axis(p, t[:, None, :], 1)[:, 0]
        nll = np.maximum(_f(0.0), log32_np(s) - d_t)
        q = _f(1.0) - p_t
        wgt = np.ones_like(q)
        for _ in range(gamma):
            wgt = wgt * q
        foc = wgt * nll
    return p, nll, foc, t, kind


def _fixed(v, scale, to_int=np.floor):
    """floor(v scale), or rint(v scale), of float32 v >= 0 as uint64; scale is a power of two, so the product is exact in
    float32 and so is either rounding of it."""
    return to_int(v.astype(_f) * _f(scale)).astype(np.uint64)


def loss_sums_np(logits, target, gamma=2):
    """(table uint64 [B,C,5], outside uint32 [B,2]) of float32 logits [B,C,H,W] and a uint8 target [B,H,W] (module
    docstring): bit for bit what the kernel writes."""
    p, nll, foc, t, kind = pixel_terms_np(logits, target, gamma)
    b, c, _ = p.shape
    live = kind == 0
    table = np.zeros((b, c, 5), np.uint64)
    pq = _fixed(p, P_SCALE)
    nq = _fixed(np.minimum(nll, _f(V_CLAMP)), V_SCALE, np.rint)
    fq = _fixed(np.minimum(foc, _f(V_CLAMP)), V_SCALE, np.rint)
    for k in range(c):
        sel = live & (t == k)
        table[:, k, 0] = sel.sum(1)
        table[:, k, 1] = np.where(live, pq[:, k], 0).sum(1, dtype=np.uint64)
        table[:, k, 2] = np.where(sel, pq[:, k], 0).sum(1, dtype=np.uint64)
        table[:, k, 3] = np.where(sel, nq, 0).sum(1, dtype=np.uint64)
        table[:, k, 4] = np.where(sel, fq, 0).sum(1, dtype=np.uint64)
    outside = np.stack([(kind == 1).sum(1), (kind == 2).sum(1)], 1).astype(np.uint32)
    return table, outside


# ---- the losses as float64 algebra on a table, with the reference's expressions and argument names -----------------------------
def _columns(table):
    t = np.asarray(table)
    if t.ndim != 3 or t.shape[2] != 5 or t.dtype.kind not in "iu":
        raise ValueError(f"table must be an integer array [B,C,5], got {t.dtype} {list(t.shape)}")
    t = t.astype(np.uint64)                                      # the device hands out uint64 bits in int64
    return (t[..., 0].astype(np.float64), t[..., 1].astype(np.float64) / P_SCALE, t[..., 2].astype(np.float64) / P_SCALE,
            t[..., 3].astype(np.float64) / V_SCALE, t[..., 4].astype(np.float64) / V_SCALE)


def _weights(class_weights, c, what="class_weights"):
    if class_weights is None:
        return None
    w = np.asarray(class_weights, np.float64).reshape(-1)
    if w.shape != (c,):
        raise ValueError(f"{what} must hold one weight per class ({c}), got {list(np.shape(class_weights))}")
    return w


def cross_entropy_from_sums(table, class_weights=None):
    """nn.CrossEntropyLoss(weight=class_weights)(pred, target), reduction 'mean': sum w_c NLL / sum w_c T over the batch."""
    T, _, _, NLL, _ = _columns(table)
    w = _weights(class_weights, T.shape[1])
    w = np.ones(T.shape[1]) if w is None else w
    return float((NLL * w).sum() / (T * w).sum())


def dice_from_sums(table, smooth=1e-5, ignore_bg=True, skip_empty=True, class_weights=None):
    """DiceLoss(smooth, ignore_bg, skip_empty, class_weights)(pred, target) (losses.py:32-83): intersection = I,
    union = P + T, dice = (2 I + smooth) / (union + smooth) per (n, c); the classes of the mean are all but the background
    (ignore_bg) and those with T > 0 in their frame (skip_empty); when none is left, all but the background again; the mean
    is sum(dice w) / (sum(w) + 1e-6) over them with class weights, their plain mean without."""
    T, P, I, _, _ = _columns(table)
    n, c = T.shape
    dice = (2 * I + smooth) / (P + T + smooth)

    def everything():
        v = np.ones((n, c), bool)
        if ignore_bg:
            v[:, 0] = False
        return v
    valid = everything()
    if skip_empty:
        valid &= T > 0
    if valid.sum() == 0:
        valid = everything()
    w = _weights(class_weights, c)
    if w is not None:
        wv = np.where(valid, np.broadcast_to(w, (n, c)), 0.0)
        mean = (dice * wv).sum() / (wv.sum() + 1e-6)
    else:
        mean = dice[valid].mean()
    return float(1.0 - mean)


def focal_from_sums(table, hw, alpha=None):
    """FocalLoss(gamma, alpha)(pred, target) (losses.py:107-140) with the table's gamma: sum alpha_c FOC / (N H W); hw = H W.
    The mean runs over every pixel, as the reference's does (its ignore_index never matches a class)."""
    T, _, _, _, FOC = _columns(table)
    a = _weights(alpha, T.shape[1], "alpha")
    a = np.ones(T.shape[1]) if a is None else a
    return float((FOC * a).sum() / (T.shape[0] * int(hw)))


def tversky_from_sums(table, alpha=0.3, beta=0.7, smooth=1e-5, ignore_bg=True):
    """TverskyLoss(alpha, beta, smooth, ignore_bg)(pred, target) (losses.py:168-200): TP = I, FP = P - I, FN = T - I."""
    T, P, I, _, _ = _columns(table)
    TP, FP, FN = I, P - I, T - I
    tversky = (TP + smooth) / (TP + alpha * FN + beta * FP + smooth)
    if ignore_bg:
        tversky = tversky[:, 1:]
    return float(1.0 - tversky.mean())


def combined_from_sums(table, weight_ce=1.0, weight_dice=1.0, class_weights=None, dice_ignore_bg=True, dice_skip_empty=True):
    """CombinedLoss(...)(pred, target) (losses.py:203-241) -> (loss, ce, dice)."""
    ce = cross_entropy_from_sums(table, class_weights)
    dice = dice_from_sums(table, ignore_bg=dice_ignore_bg, skip_empty=dice_skip_empty, class_weights=class_weights)
    return weight_ce * ce + weight_dice * dice, ce, dice


def advanced_combined_from_sums(table, hw, weight_focal=0.4, weight_tversky=0.4, weight_dice=0.2, tversky_alpha=0.3, tversky_beta=0.7,
                                class_weights=None, dice_ignore_bg=True):
    """AdvancedCombinedLoss(...)(pred, target) (losses.py:244-302) -> (loss, focal, tversky, dice); focal_gamma is the gamma
    the table was made with.  Its Dice always skips empty classes."""
    focal = focal_from_sums(table, hw, class_weights)
    tversky = tversky_from_sums(table, tversky_alpha, tversky_beta, ignore_bg=dice_ignore_bg)
    dice = dice_from_sums(table, ignore_bg=dice_ignore_bg, skip_empty=True, class_weights=class_weights)
    return weight_focal * focal + weight_tversky * tversky + weight_dice * dice, focal, tversky, dice


CRITERIA = ("combined", "advanced")


def _criterion(table, hw, criterion, kw):
    if criterion == "combined":
        return combined_from_sums(table, **kw)
    if criterion == "advanced":
        return advanced_combined_from_sums(table, hw, **kw)
    raise ValueError(f"criterion must be one of {CRITERIA}, got {criterion!r}")


# ---- seeded scenes for tests and fixtures -------------------------------------------------------------------------------------
LOGIT_KINDS = ("plain", "confident", "uniform", "wide", "nonfinite")
TARGET_KINDS = ("plain", "absent_one", "background", "out_of_range")


def _regions(B, C, H, W, r):
    """int64 [B,H,W]: the cells of 2 C + 3 random sites per frame, the first C sites covering the classes in turn."""
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W), np.int64)
    for b in range(B):
        k = 2 * C + 3
        sy, sx = r.uniform(0, H, k), r.uniform(0, W, k)
        cls = r.integers(0, C, k)
        cls[:C] = np.arange(C)
        d = (y[None] - sy[:, None, None]) ** 2 + (x[None] - sx[:, None, None]) ** 2
        out[b] = cls[d.argmin(0)]
        if H * W >= 8 * C:                                       # a class whose cell came out empty gets one pixel
            out[b].reshape(-1)[r.permutation(H * W)[:C]] = np.arange(C)
    return out


def make_target(B, C, H, W, seed, kind="plain"):
    """A seeded uint8 target [B,H,W] of piecewise-constant regions in which every class occurs in every frame (frames of
    at least 8 C pixels), then by `kind`: absent_one relabels the last class of frame 0 as background (absent from one frame
    only when B > 1), background is all zeros (every other class absent from every frame: Dice's fallback),
    out_of_range sets about 1 % of the pixels (at least one) to values >= C."""
    if kind not in TARGET_KINDS:
        raise ValueError(f"kind must be one of {TARGET_KINDS}, got {kind!r}")
    r = np.random.default_rng(9100 + 977 * int(seed) + C)
    t = _regions(B, C, H, W, r).astype(np.uint8)
    if kind == "absent_one":
        t[0][t[0] == C - 1] = 0
    elif kind == "background":
        t[:] = 0
    elif kind == "out_of_range":
        hit = r.random((B, H, W)) < 0.01
        hit.reshape(-1)[r.integers(0, hit.size)] = True
        t[hit] = r.integers(C, 256, int(hit.sum())).astype(np.uint8)
    return t


def make_logits(B, C, H, W, seed, kind="plain"):
    """Seeded float32 logits [B,C,H,W] that lean towards make_target(B, C, H, W, seed) with 5 % of the pixels leaning
    elsewhere: plain N(0, 1.5) + 2.5 at the favoured class; confident N(0, 1) + 7; uniform N(0, 0.05) (near-uniform
    probabilities); wide uniform in +-60 (exp32 underflows to 0); nonfinite is plain with a few pixels holding +inf, -inf
    or NaN in one class."""
    if kind not in LOGIT_KINDS:
        raise ValueError(f"kind must be one of {LOGIT_KINDS}, got {kind!r}")
    guess = make_target(B, C, H, W, seed).astype(np.int64)
    r = np.random.default_rng(9300 + 977 * int(seed) + C)
    flip = r.random(guess.shape) < 0.05
    guess[flip] = r.integers(0, C, int(flip.sum()))
    onehot = (np.arange(C)[None, :, None, None] == guess[:, None]).astype(np.float64)
    if kind == "confident":
        x = r.normal(0, 1.0, (B, C, H, W)) + 7.0 * onehot
    elif kind == "uniform":
        x = r.normal(0, 0.05, (B, C, H, W))
    elif kind == "wide":
        x = r.uniform(-60, 60, (B, C, H, W))
    else:
        x = r.normal(0, 1.5, (B, C, H, W)) + 2.5 * onehot
    x = x.astype(np.float32)
    if kind == "nonfinite":
        flat = x.reshape(-1)
        idx = r.permutation(flat.size)[:max(3, flat.size // 200)]
        flat[idx] = np.resize(np.float32([np.inf, -np.inf, np.nan]), idx.size)
    return x


# (name, B, C, H, W, seed, logit kind, target kind); the first group is compared with the reference (no special pixels)
LOSS_SCENES = [
    ("plain3", 2, 3, 17, 23, 0, "plain", "plain"),
    ("plain7", 3, 7, 48, 80, 1, "plain", "plain"),
    ("confident3", 2, 3, 40, 64, 2, "confident", "plain"),
    ("uniform3", 2, 3, 24, 40, 3, "uniform", "plain"),
    ("wide4", 2, 4, 24, 40, 4, "wide", "plain"),
    ("absent3", 3, 3, 24, 40, 5, "plain", "absent_one"),
    ("absent7_single", 1, 7, 33, 57, 6, "plain", "absent_one"),
    ("background3", 2, 3, 24, 40, 7, "plain", "background"),
    ("confident8", 2, 8, 16, 20, 8, "confident", "plain"),
    ("plain3_256", 4, 3, 256, 256, 9, "plain", "plain"),
    ("nonfinite3", 2, 3, 24, 40, 10, "nonfinite", "plain"),
    ("range7", 2, 7, 24, 40, 11, "plain", "out_of_range"),
    ("both3", 3, 3, 17, 23, 12, "nonfinite", "out_of_range"),
]
SPECIAL = {"nonfinite", "out_of_range"}
# name -> (ignore_bg, skip_empty, weighted): the defaults, tools/train_3class.py's Dice, each with and without class weights
PARAM_SETS = {"default": (True, True, False), "default_w": (True, True, True), "3class": (False, False, False), "3class_w": (False, False, True)}


def scene_class_weights(C):
    """The class weights of the weighted parameter sets: 0.5, 0.75, 1.0, ... (exact in float32)."""
    return 0.5 + 0.25 * np.arange(C, dtype=np.float64)


def make_scene(name):
    _, B, C, H, W, seed, lk, tk = next(s for s in LOSS_SCENES if s[0] == name)
    return make_logits(B, C, H, W, seed, lk), make_target(B, C, H, W, seed, tk)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scene_losses(table, hw, params):
    """float64 [6]: LOSSES of one table under one of PARAM_SETS, as the generator stores the reference's."""
    ignore_bg, skip_empty, weighted = PARAM_SETS[params]
    cw = scene_class_weights(np.asarray(table).shape[1]) if weighted else None
    comb = combined_from_sums(table, class_weights=cw, dice_ignore_bg=ignore_bg, dice_skip_empty=skip_empty)
    adv = advanced_combined_from_sums(table, hw, class_weights=cw, dice_ignore_bg=ignore_bg)
    return np.array([comb[1], comb[2], adv[1], adv[2], comb[0], adv[0]], np.float64)


def fixture_facts(g):
    """What both the generator and tests/test_loss_host.py assert of the fixture `g` (the loaded .npz as a dict): the
    inputs are the regenerated scenes, the compared scenes have no special pixel, every branch of the algebra is met.
    Returns {"dist": {loss: the largest |form - ref64| / |ref64| over scenes and parameter sets}, "worst": {loss: (scene,
    params)}, "branches": the set met}."""
    branches, dist, worst = set(), {k: 0.0 for k in LOSSES}, {k: None for k in LOSSES}
    for name, B, C, H, W, seed, lk, tk in LOSS_SCENES:
        logits, target = make_logits(B, C, H, W, seed, lk), make_target(B, C, H, W, seed, tk)
        assert sha256(logits) == str(g[f"{name}_logits_sha"]) and sha256(target) == str(g[f"{name}_target_sha"]), name
        table, outside = loss_sums_np(logits, target, 2)
        assert (table[:, :, 0].sum(1) + outside.sum(1) == H * W).all(), name
        special = lk in SPECIAL or tk in SPECIAL
        assert special == bool(outside.any()), name
        if special:
            assert f"{name}_ref64" not in g
            branches.add(("outside", tuple(bool(v) for v in outside.any(0))))
            continue
        assert np.isfinite(logits).all() and int(target.max()) < C
        T = table[:, :, 0]
        if not T[:, 1:].any():
            branches.add("dice_fallback")
        if B == 1 and (T[0, 1:] == 0).any() and T[0, 1:].any():
            branches.add("skip_empty_single_frame")
        if B > 1 and (T[:, 1:] == 0).any(0).any() and ((T[:, 1:] == 0).sum(0) == 1).any():
            branches.add("absent_from_one_frame_only")
        if (pixel_terms_np(logits, target)[0] == 0).any():
            branches.add("exp32_underflow")
        ref64 = g[f"{name}_ref64"]
        for j, params in enumerate(PARAM_SETS):
            branches.add(("weighted", PARAM_SETS[params][2]))
            got = scene_losses(table, H * W, params)
            for k, loss in enumerate(LOSSES):
                rel = abs(got[k] - ref64[j, k]) / abs(ref64[j, k])
                if rel > dist[loss]:
                    dist[loss], worst[loss] = float(rel), (name, params)
    need = {"dice_fallback", "skip_empty_single_frame", "absent_from_one_frame_only", "exp32_underflow", ("weighted", False), ("weighted", True),
            ("outside", (False, True)), ("outside", (True, False)), ("outside", (True, True))}
    assert branches >= need, need - branches
    return {"dist": dist, "worst": worst, "branches": branches}


# ---- the device path (torch imported lazily, as in evaluation.py) --------------------------------------------------------------
def layout():
    """The pixels of a frame one workgroup of the kernel owns (unetpp_loss_layout)."""
    from . import _lib
    span = ctypes.c_int(-1)
    if _lib.load().unetpp_loss_layout(ctypes.byref(span)) != 0:
        raise RuntimeError("unetpp_loss_layout failed")
    return span.value


def _rows(torch, frames, c, device):
    """One allocation for `frames` frames: (table int64 [frames,C,5], outside int32 [frames,2]), the second directly
    behind the first so that the entry clears both with one memset."""
    raw = torch.empty((frames * (c * 5 + 1),), dtype=torch.int64, device=device)
    return raw[:frames * c * 5].view(frames, c, 5), raw[frames * c * 5:].view(torch.int32).view(frames, 2)


def loss_sums(model, logits, target, gamma=2, out=None):
    """loss_sums_np on the device for float32 CUDA logits [B,C,H,W] (the layout of forward and
    segment(return_logits=True)) and a uint8 CUDA target [B,H,W], any alignment of either -> (table int64 [B,C,5] holding the
    uint64 values, all below 2^63; outside int32 [B,2]) on the device; one launch on the current stream, nothing is read
    back.  out: a (table, outside) pair of contiguous views to write instead of new tensors (evaluate_losses)."""
    import torch
    b, c, h, w, gamma = check_args(logits, target, gamma)
    logits = model._input(logits, "logits", "[B,C,H,W]", "float32")
    target = model._input(target, "target")
    table, outside = _rows(torch, b, c, logits.device) if out is None else out
    model._call("unetpp_loss_sums_f32", logits, target, b, c, h, w, gamma, table, outside, stream_of=logits)
    return table, outside


def _raise_outside(outside, c, first=0):
    bad = np.flatnonzero(np.asarray(outside).any(1))
    if bad.size:
        o = np.asarray(outside)[bad[0]]
        raise ValueError(f"frame {first + int(bad[0])}: {int(o[0])} pixels have a target >= num_classes {c} and {int(o[1])} more a non-finite logit "
                         f"(the reference's scatter_ raises on the first kind and returns NaN on the second)")


def _read_back(torch, table, outside):
    """One copy to the host for both tensors -> (uint64 [B,C,5], uint32 [B,2])."""
    got = torch.cat([table.reshape(-1), outside.reshape(-1).long()]).cpu().numpy()
    n = table.numel()
    return got[:n].view(np.uint64).reshape(tuple(table.shape)), got[n:].astype(np.uint32).reshape(tuple(outside.shape))


def _device_loss(model, logits, target, criterion, gamma, check, kw):
    import torch
    table, outside = loss_sums(model, logits, target, gamma)
    t, o = _read_back(torch, table, outside)
    if check:
        _raise_outside(o, t.shape[1])
    return _criterion(t, logits.shape[2] * logits.shape[3], criterion, kw)


def combined_loss(model, logits, target, check=True, **kw):
    """CombinedLoss(**kw)(logits, target) -> (loss, ce, dice) as Python floats: one launch, one read-back (synchronises),
    then combined_from_sums.  check=True raises ValueError when a pixel's target is >= C or a logit is not finite; with
    check=False such pixels are left out of every sum."""
    return _device_loss(model, logits, target, "combined", 0, check, kw)


def advanced_combined_loss(model, logits, target, focal_gamma=2, check=True, **kw):
    """AdvancedCombinedLoss(focal_gamma=focal_gamma, **kw)(logits, target) -> (loss, focal, tversky, dice), as combined_loss."""
    return _device_loss(model, logits, target, "advanced", focal_gamma, check, kw)


def deep_supervision_losses(model, x, target, criterion="combined", focal_gamma=2, check=True, **kw):
    """The criterion on each of forward_deep_supervision(x) = [out, out1, out2, out3] against one target, as the training
    loops apply it to the list -> (the four loss tuples, the mean of their totals).  Four launches into one table, one
    read-back."""
    import torch
    outs = model.forward_deep_supervision(x)
    b, c, h, w, gamma = check_args(outs[0], target, focal_gamma if criterion == "advanced" else 0)
    table, outside = _rows(torch, len(outs) * b, c, outs[0].device)
    for k, o in enumerate(outs):
        loss_sums(model, o, target, gamma, out=(table[k * b:(k + 1) * b], outside[k * b:(k + 1) * b]))
    t, o = _read_back(torch, table, outside)
    if check:
        _raise_outside(o.reshape(len(outs), b, 2).sum(0), c)
    losses = [_criterion(t[k * b:(k + 1) * b], h * w, criterion, kw) for k in range(len(outs))]
    return losses, float(np.mean([v[0] for v in losses]))


def evaluate_losses(model, batches, criterion="combined", focal_gamma=2, output=0, check=True, capacity=None, **kw):
    """The loss half of a validation loop (tools/train_simple.py:188-207) over `batches`, an iterable of (x, target): x
    anything forward() accepts, target a uint8 CUDA tensor [B,H,W].  Per batch forward(x, output=output) and one launch
    into a slice of one preallocated device table; ONE synchronisation and read-back at the end.  capacity: the frames to
    preallocate (default: len(batches) times the first batch's B when batches has a length, else 64 batches of it; another
    block is added when it runs out).  Returns a dict: losses (one tuple per batch, as the criterion returns them), mean
    (float64 array: the mean of each tuple entry over the batches, mean[0] the validation loss) and frames."""
    import torch
    gamma = focal_gamma if criterion == "advanced" else 0
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}, got {criterion!r}")
    blocks, spans, used, hw, c = [], [], 0, None, None
    for x, target in batches:
        logits = model.forward(x, output=output)
        b, c, h, w, _ = check_args(logits, target, gamma)
        if hw not in (None, h * w):
            raise ValueError(f"every batch must have the frame size of the first one ({hw} pixels), got {h}x{w}")
        hw = h * w
        if not blocks or used + b > blocks[-1][0].shape[0]:
            n = max(b, int(capacity) if capacity is not None else b * (len(batches) if hasattr(batches, "__len__") else 64))
            blocks.append(_rows(torch, n, c, logits.device))
            used = 0
        table, outside = blocks[-1]
        loss_sums(model, logits, target, gamma, out=(table[used:used + b], outside[used:used + b]))
        spans.append((len(blocks) - 1, used, b))
        used += b
    if not blocks:
        raise ValueError("evaluate_losses needs at least one batch")
    n_t = [t.numel() for t, _ in blocks]
    got = torch.cat([t.reshape(-1) for t, _ in blocks] + [o.reshape(-1).long() for _, o in blocks]).cpu().numpy()      # the one read-back
    tables, outsides, at = [], [], 0
    for n, (t, _) in zip(n_t, blocks):
        tables.append(got[at:at + n].view(np.uint64).reshape(tuple(t.shape)))
        at += n
    for _, o in blocks:
        outsides.append(got[at:at + o.numel()].reshape(tuple(o.shape)))
        at += o.numel()
    losses, first = [], 0
    for k, u, b in spans:
        if check:
            _raise_outside(outsides[k][u:u + b], c, first)
        losses.append(_criterion(tables[k][u:u + b], hw, criterion, kw))
        first += b
    return {"losses": losses, "mean": np.mean(np.array(losses, np.float64), 0), "frames": first}
