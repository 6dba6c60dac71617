"""Loss gradients: d loss / d logits of the reference's CombinedLoss (cross-entropy + Dice) and AdvancedCombinedLoss (Focal +
Tversky + Dice) of src/models/losses.py, in NumPy (torch-free) and on the device (include/unetpp_loss_grad.h,
unetpp_loss_grad_f32; csrc/loss_grad.h), and the two criteria as torch modules that stand where the reference's stand in a
training loop: `loss, *parts = criterion(pred, target); loss.backward()`.

The forward is the one of loss.py: one launch for the five sums per frame and class, one read-back, float64 algebra.  From
the same table the host derives coef float32 [B,C,4] = (A, G, K_ce, K_foc):
  G = d loss / d P_bc and A = d loss / d I_bc of the region losses (Dice and Tversky are functions of T, P, I alone),
  K_ce and K_foc the factors of the two per-pixel losses (cross-entropy's weighted mean, Focal's mean over every pixel);
include/unetpp_loss_grad.h has the expressions.  With p = softmax(x), y_c = p_c - [c = t] and phi the factor with
d[(1 - p_t)^gamma nll] / d x_c = phi y_c, a pixel's gradient is
  g_c = (K_ce[t] + K_foc[t] phi) y_c + p_c (u_c - sum_k p_k u_k),      u_c = G_c + [c = t] A_c
so the backward is one pass that reads logits and target once and writes the gradient once: no atomics, nothing depends on
the order in which threads arrive.  Every operation is an explicit float32 operation in a stated order (the header), so
loss_grad_np performs the same operations as the kernel and returns the same bits.

Pixels the forward leaves out (target >= C, a non-finite logit) get a gradient of exactly +0.

The functions take the model, as loss.py's do; a weightless NestedUNet(C).to(device) is enough.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import loss as ls

_f = np.float32
SMOOTH = 1e-5                                   # DiceLoss's and TverskyLoss's default, which neither criterion changes
DS_WEIGHTS = (0.1, 0.2, 0.3, 0.4)               # tools/train_3class_advanced.py:297

# the reference's constructors: keyword -> default
DEFAULTS = {
    "combined": dict(weight_ce=1.0, weight_dice=1.0, class_weights=None, dice_ignore_bg=True, dice_skip_empty=True),
    "advanced": dict(weight_focal=0.4, weight_tversky=0.4, weight_dice=0.2, focal_gamma=2, tversky_alpha=0.3, tversky_beta=0.7,
                     class_weights=None, dice_ignore_bg=True),
}


def _keywords(criterion, kw):
    if criterion not in DEFAULTS:
        raise ValueError(f"criterion must be one of {ls.CRITERIA}, got {criterion!r}")
    unknown = set(kw) - set(DEFAULTS[criterion])
    if unknown:
        raise TypeError(f"{criterion}: unexpected keyword(s) {sorted(unknown)}; the reference's are {sorted(DEFAULTS[criterion])}")
    return {**DEFAULTS[criterion], **kw}


def _gamma(criterion, kw):
    """The integer gamma of the kernels: focal_gamma for the advanced criterion, 0 (no Focal term) for the combined one."""
    if criterion != "advanced":
        return 0
    g = kw.get("focal_gamma", 2)
    if isinstance(g, bool) or int(g) != g or not 0 <= int(g) <= ls.MAX_GAMMA:
        raise ValueError(f"focal_gamma must be an integer in 0..{ls.MAX_GAMMA}, got {g!r}")
    return int(g)


# ---- the coefficients: float64 algebra on the columns T, P, I ---------------------------------------------------------------------
def coefficients_from_columns(T, P, I, hw, criterion, **kw):
    """float64 [B,C,4] = (A, G, K_ce, K_foc) from the columns T, P, I [B,C] as real numbers (module docstring;
    include/unetpp_loss_grad.h has the expressions), hw = H W, `kw` the keywords of the reference's constructor."""
    k = _keywords(criterion, kw)
    T, P, I = (np.asarray(v, np.float64) for v in (T, P, I))
    n, c = T.shape
    w = ls._weights(k["class_weights"], c)
    ignore_bg = bool(k["dice_ignore_bg"])
    skip_empty = bool(k["dice_skip_empty"]) if criterion == "combined" else True
    s = SMOOTH

    # Dice: the valid set of loss.dice_from_sums, then d(1 - sum omega dice) / dI and / dP
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
    if w is not None:
        wv = np.where(valid, np.broadcast_to(w, (n, c)), 0.0)
        omega = wv / (wv.sum() + 1e-6)
    else:
        omega = valid / valid.sum()
    U = P + T + s
    A = k["weight_dice"] * (-2.0 * omega / U)
    G = k["weight_dice"] * (omega * (2.0 * I + s) / (U * U))
    out = np.zeros((n, c, 4), np.float64)
    if criterion == "advanced":
        alpha, beta = float(k["tversky_alpha"]), float(k["tversky_beta"])
        om_tv = np.full((n, c), 1.0 / (n * (c - 1 if ignore_bg else c)))
        if ignore_bg:
            om_tv[:, 0] = 0.0
        D = I + alpha * (T - I) + beta * (P - I) + s
        A = A + k["weight_tversky"] * (-om_tv * (1.0 / D - (I + s) * (1.0 - alpha - beta) / (D * D)))
        G = G + k["weight_tversky"] * (om_tv * beta * (I + s) / (D * D))
        a = np.ones(c) if w is None else w
        out[:, :, 3] = k["weight_focal"] * a / (n * int(hw))
    else:
        wc = np.ones(c) if w is None else w
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, :, 2] = k["weight_ce"] * wc / (T * wc).sum()
    out[:, :, 0], out[:, :, 1] = A, G
    return out


def coefficients_from_sums(table, hw, criterion, **kw):
    """float32 [B,C,4] = (A, G, K_ce, K_foc) of the uint64 table loss.loss_sums returns: coefficients_from_columns in float64,
    rounded once."""
    T, P, I, _, _ = ls._columns(table)
    with np.errstate(over="ignore"):
        return coefficients_from_columns(T, P, I, hw, criterion, **kw).astype(_f)


# ---- the NumPy form of the kernel --------------------------------------------------------------------------------------------------
def check_coef(coef, b, c):
    coef = np.asarray(coef)
    if coef.shape != (b, c, 4) or coef.dtype.kind != "f":
        raise ValueError(f"coef must be a float array [{b},{c},4], got {coef.dtype} {list(coef.shape)}")
    return coef


def _exact_terms(logits, target, c):
    """p float64 [B,C,HW], nll float64 [B,HW], t, kind of the float64 evaluation (np.exp / np.log)."""
    b = logits.shape[0]
    x = np.asarray(logits, np.float64).reshape(b, c, -1)
    t = np.asarray(target).reshape(b, -1).astype(np.int64)
    kind = np.where(t >= c, 1, np.where(~np.isfinite(x).all(1), 2, 0)).astype(np.uint8)
    x = np.where((kind != 0)[:, None, :], 0.0, x)
    t = np.where(kind != 0, 0, t)
    d = x - x.max(1, keepdims=True)
    e = np.exp(d)
    s = e.sum(1)
    p = e / s[:, None, :]
    nll = np.log(s) - np.take_along_axis(d, t[:, None, :], 1)[:, 0]
    return p, nll, t, kind


def loss_grad_np(logits, target, coef, gamma, scale=None, exact=False):
    """float32 [B,C,H,W]: the gradient of float32 logits [B,C,H,W] and a uint8 target [B,H,W] under coef [B,C,4], bit for
    bit what the kernel writes (include/unetpp_loss_grad.h states the operations).  scale: None, or the float32 factor of
    every element.  exact=True: the same formulas in float64 with np.exp / np.log and coef as it is given (float64 [B,C,H,W]),
    for comparisons with calculus."""
    logits, target = np.asarray(logits), np.asarray(target)
    if exact:
        b, c, h, w, gamma = ls.check_args(logits.astype(_f), target, gamma)
        f = np.float64
        coef = check_coef(coef, b, c).astype(f)
        p, nll, t, kind = _exact_terms(logits, target, c)
    else:
        b, c, h, w, gamma = ls.check_args(logits, target, gamma)
        f = _f
        coef = check_coef(coef, b, c)
        if coef.dtype != _f:
            raise ValueError(f"coef must be float32 (coefficients_from_sums), got {coef.dtype}")
        p, nll, _, t, kind = ls.pixel_terms_np(logits, target, gamma)
        nll = np.minimum(nll, _f(ls.V_CLAMP))
    with np.errstate(over="ignore", invalid="ignore"):
        onehot = np.arange(c)[None, :, None] == t[:, None, :]
        p_t = np.take_along_axis(p, t[:, None, :], 1)[:, 0]
        om = f(1.0) - p_t
        w1 = np.ones_like(om)
        for _ in range(gamma - 1):
            w1 = w1 * om
        wg = w1 * om if gamma >= 1 else np.ones_like(om)
        phi = wg + ((f(gamma) * p_t) * w1) * nll if gamma else np.ones_like(om)
        A, G = coef[:, :, 0][:, :, None], coef[:, :, 1][:, :, None]
        u = np.where(onehot, G + A, G)
        dot = p[:, 0] * u[:, 0]
        for k in range(1, c):
            dot = dot + p[:, k] * u[:, k]
        r = p * (u - dot[:, None, :])
        kk = np.take_along_axis(coef[:, :, 2], t, 1) + np.take_along_axis(coef[:, :, 3], t, 1) * phi
        y = np.where(onehot, p - f(1.0), p)
        g = kk[:, None, :] * y + r
        if scale is not None:
            g = g * f(scale)
    g = np.where((kind != 0)[:, None, :], f(0.0), g)
    assert g.dtype == f
    return g.reshape(b, c, h, w)


# ---- the device path (torch imported lazily, as in loss.py) -----------------------------------------------------------------------
def layout():
    """The pixels of a frame one workgroup of the gradient kernel owns (unetpp_loss_grad_layout)."""
    from . import _lib
    span = ctypes.c_int(-1)
    if _lib.load().unetpp_loss_grad_layout(ctypes.byref(span)) != 0:
        raise RuntimeError("unetpp_loss_grad_layout failed")
    return span.value


def narrow_target(model, target_i64):
    """An int64 CUDA target of any shape (the reference's, dataset.py:100-101) -> uint8 of the same shape: values 0..254
    copied, every other value (ignore_index -100 included) 255, which the loss kernels count as outside the classes.  One
    launch on the current stream."""
    import torch
    if not (isinstance(target_i64, torch.Tensor) and target_i64.is_cuda and target_i64.dtype == torch.int64 and target_i64.numel() > 0):
        raise RuntimeError("target must be a non-empty int64 CUDA tensor")
    src = model._input(target_i64.reshape(1, 1, -1), "target", "[B,H,W]", "int64")
    out = torch.empty((src.numel(),), dtype=torch.uint8, device=src.device)
    model._call("unetpp_loss_narrow_target_i64", src, src.numel(), out, stream_of=src)
    return out.view(target_i64.shape)


def loss_grad(model, logits, target, coef, gamma, scale=None, out=None):
    """loss_grad_np on the device: float32 CUDA logits [B,C,H,W], a uint8 CUDA target [B,H,W], coef a float32 CUDA tensor
    [B,C,4], scale None or a float32 CUDA tensor of one element -> the float32 gradient [B,C,H,W]; one launch on the current
    stream, nothing is read back.  out: a contiguous float32 CUDA tensor [B,C,H,W] to write; out=logits is the in-place form."""
    import torch
    b, c, h, w, gamma = ls.check_args(logits, target, gamma)
    logits = model._input(logits, "logits", "[B,C,H,W]", "float32")
    target = model._input(target, "target")
    coef = model._input(coef, "coef", f"[{b},{c},4]", "float32")
    if scale is not None:
        scale = model._input(scale.reshape(1) if isinstance(scale, torch.Tensor) else scale, "scale", "[1]", "float32")
    if out is None:
        out = torch.empty((b, c, h, w), dtype=torch.float32, device=logits.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (b, c, h, w) and
              out.is_contiguous() and out.device == logits.device):
        raise RuntimeError(f"out must be a contiguous float32 CUDA tensor {[b, c, h, w]} on the logits' device")
    model._call("unetpp_loss_grad_f32", logits, target, b, c, h, w, gamma, coef, scale, out, stream_of=logits)
    return out


def _apply(m, preds, target):
    """The criterion module `m` on each tensor of `preds` against one target -> one tuple per tensor, as m.forward returns
    it.  Half and bfloat16 logits go through torch's own .float(), so that the gradient flows back through that cast; an
    int64 target is narrowed on the device.  One sums launch per tensor into ONE table, one read-back; a tensor that requires
    a gradient gets its coefficients and the loss value in one upload (1 KB at most) and the Function below."""
    import torch
    if isinstance(target, torch.Tensor) and target.dtype == torch.int64:
        target = narrow_target(m.model, target)
    preds = [p.float() if isinstance(p, torch.Tensor) and p.dtype in (torch.float16, torch.bfloat16) else p for p in preds]
    b, c, h, w, gamma = ls.check_args(preds[0], target, m.gamma)
    preds = [m.model._input(p, "pred", f"[{b},{c},{h},{w}]", "float32") for p in preds]
    table, outside = ls._rows(torch, len(preds) * b, c, preds[0].device)
    for k, p in enumerate(preds):
        ls.loss_sums(m.model, p.detach(), target, gamma, out=(table[k * b:(k + 1) * b], outside[k * b:(k + 1) * b]))
    t, o = ls._read_back(torch, table, outside)
    if m.check:
        ls._raise_outside(o.reshape(len(preds), b, 2).sum(0), c)
    kw = {k: v for k, v in m.kw.items() if k != "focal_gamma"}
    results = []
    for k, p in enumerate(preds):
        tk = t[k * b:(k + 1) * b]
        losses = ls._criterion(tk, h * w, m.criterion, kw)
        if p.requires_grad and torch.is_grad_enabled():
            coef = coefficients_from_sums(tk, h * w, m.criterion, **kw)
            packed = torch.from_numpy(np.concatenate([coef.reshape(-1), np.array([losses[0]], _f)])).to(p.device)
            loss = _torch_classes()["LossGrad"].apply(p, target, packed, m.model, gamma)
        else:
            loss = torch.tensor(losses[0], dtype=torch.float32, device=p.device)
        results.append((loss,) + tuple(losses[1:]))
    return results


_classes = {}


def _torch_classes():
    """The autograd Function and the two modules, defined on first use: they derive from torch classes, and importing this
    module needs no torch (the NumPy forms run without it)."""
    if _classes:
        return _classes
    import torch

    class LossGrad(torch.autograd.Function):
        """forward: handed what the one read-back produced (packed = coef [B,C,4] and the loss value), returns the loss.
        backward: ONE unetpp_loss_grad_f32 launch with grad_output as dev_scale; no synchronisation, no torch op over
        [N,C,H,W]."""

        @staticmethod
        def forward(ctx, pred, target, packed, model, gamma):
            ctx.model, ctx.gamma = model, gamma
            ctx.save_for_backward(pred, target, packed)
            return packed[-1].clone()

        @staticmethod
        def backward(ctx, grad_output):
            pred, target, packed = ctx.saved_tensors
            b, c = pred.shape[:2]
            grad = loss_grad(ctx.model, pred, target, packed[:-1].view(b, c, 4), ctx.gamma, scale=grad_output.to(torch.float32).reshape(1))
            return grad, None, None, None, None

    class _Criterion(torch.nn.Module):
        criterion = None

        def _setup(self, model, check, kw):
            super().__init__()
            object.__setattr__(self, "model", model)              # not a submodule: the criterion owns no parameters
            self.check = bool(check)
            self.kw = _keywords(self.criterion, kw)
            cw = self.kw["class_weights"]
            if cw is not None:
                self.kw["class_weights"] = np.asarray(cw.detach().cpu().numpy() if isinstance(cw, torch.Tensor) else cw, np.float64)
            self.gamma = _gamma(self.criterion, self.kw)

        def forward(self, pred, target):
            return _apply(self, [pred], target)[0]

    class CombinedLoss(_Criterion):
        """CombinedLoss(...) of the reference (losses.py:203-241) with its keywords and defaults, on `model`'s device.
        forward(pred, target) -> (loss, ce, dice): loss a 0-d float32 CUDA tensor attached to the graph, ce and dice Python
        floats, the values loss.combined_loss returns.  pred float32 (or half / bfloat16) CUDA [B,C,H,W], target int64 or uint8
        CUDA [B,H,W].  check=True raises ValueError when a pixel's target is >= C or a logit is not finite."""
        criterion = "combined"

        def __init__(self, model, weight_ce=1.0, weight_dice=1.0, class_weights=None, dice_ignore_bg=True, dice_skip_empty=True, check=True):
            self._setup(model, check, dict(weight_ce=weight_ce, weight_dice=weight_dice, class_weights=class_weights,
                                           dice_ignore_bg=dice_ignore_bg, dice_skip_empty=dice_skip_empty))

    class AdvancedCombinedLoss(_Criterion):
        """AdvancedCombinedLoss(...) of the reference (losses.py:244-302) with its keywords and defaults; focal_gamma an
        integer in 0..4.  forward(pred, target) -> (loss, focal, tversky, dice), as CombinedLoss; the values
        loss.advanced_combined_loss returns."""
        criterion = "advanced"

        def __init__(self, model, weight_focal=0.4, weight_tversky=0.4, weight_dice=0.2, focal_gamma=2.0, tversky_alpha=0.3, tversky_beta=0.7,
                     class_weights=None, dice_ignore_bg=True, check=True):
            self._setup(model, check, dict(weight_focal=weight_focal, weight_tversky=weight_tversky, weight_dice=weight_dice, focal_gamma=focal_gamma,
                                           tversky_alpha=tversky_alpha, tversky_beta=tversky_beta, class_weights=class_weights,
                                           dice_ignore_bg=dice_ignore_bg))

    _classes.update(LossGrad=LossGrad, CombinedLoss=CombinedLoss, AdvancedCombinedLoss=AdvancedCombinedLoss)
    return _classes


def __getattr__(name):
    if name in ("CombinedLoss", "AdvancedCombinedLoss"):
        return _torch_classes()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def deep_supervision_criterion(criterion_module, outputs, target, ds_weights=DS_WEIGHTS):
    """tools/train_3class_advanced.py:294-304 for a list of outputs: loss = sum_k w_k criterion(outputs[k], target)[0] with
    the last len(outputs) of ds_weights -> (loss, the per-output tuples, each as the module returns it).  One sums launch per
    output into ONE table and one read-back; the backward issues one gradient launch per output."""
    outputs = list(outputs)
    weights = list(ds_weights)[-len(outputs):] if outputs else []
    if not outputs or len(weights) != len(outputs):
        raise ValueError(f"deep_supervision_criterion needs 1..{len(list(ds_weights))} outputs (one of ds_weights each), got {len(outputs)}")
    results = _apply(criterion_module, outputs, target)
    total = 0.0
    for w, r in zip(weights, results):
        total = total + w * r[0]
    return total, results


# ---- the fixture: scenes, combinations and what the generator and the host test both assert -------------------------------------
# (criterion, parameter set of loss.PARAM_SETS): both criteria, weighted and not, both Dice settings
GRAD_COMBOS = (("combined", "default_w"), ("combined", "3class"), ("advanced", "default"), ("advanced", "3class_w"))
GRAD_SCENES = tuple(s[0] for s in ls.LOSS_SCENES if s[6] not in ls.SPECIAL and s[7] not in ls.SPECIAL)
GRAD_POSITIONS = 256
# FINDING: the pairs whose gradient, over all positions, lies FURTHER from the reference's float64 gradient
# than the reference's own float32 gradient does (form > e32; tests/golden/README_loss_grad.txt has both numbers of each).
# The generator and tests/test_loss_grad_host.py assert that exactly these miss the bar and every other pair meets it.
KNOWN_MISSES = frozenset((
    ('plain3', 'combined', '3class'),
    ('plain3', 'advanced', 'default'),
    ('plain3', 'advanced', '3class_w'),
    ('plain7', 'combined', 'default_w'),
    ('plain7', 'advanced', 'default'),
    ('plain7', 'advanced', '3class_w'),
    ('uniform3', 'combined', 'default_w'),
    ('uniform3', 'advanced', '3class_w'),
    ('wide4', 'advanced', 'default'),
    ('wide4', 'advanced', '3class_w'),
    ('absent3', 'advanced', '3class_w'),
    ('absent7_single', 'combined', 'default_w'),
    ('absent7_single', 'advanced', 'default'),
    ('absent7_single', 'advanced', '3class_w'),
    ('confident8', 'advanced', '3class_w'),
    ('plain3_256', 'advanced', 'default'),
    ('plain3_256', 'advanced', '3class_w'),
))


def combo_keywords(criterion, params, c):
    """The constructor keywords of one combination at c classes (class weights as float64, exact in float32)."""
    ignore_bg, skip_empty, weighted = ls.PARAM_SETS[params]
    kw = dict(class_weights=ls.scene_class_weights(c) if weighted else None, dice_ignore_bg=ignore_bg)
    if criterion == "combined":
        kw["dice_skip_empty"] = skip_empty
    return kw


def sample_positions(name):
    """int64 [<= 256]: the seeded flat (frame, pixel) positions of scene `name` whose gradient the fixture stores."""
    _, B, C, H, W, seed, _, _ = next(s for s in ls.LOSS_SCENES if s[0] == name)
    r = np.random.default_rng(9500 + 977 * int(seed) + C)
    return np.sort(r.permutation(B * H * W)[:GRAD_POSITIONS])


def scene_gradient(name, criterion, params):
    """loss_grad_np of one scene under one combination, with the criterion's own gamma (2 for advanced) -> float32 [B,C,H,W]."""
    logits, target = ls.make_scene(name)
    B, C, H, W = logits.shape
    kw = combo_keywords(criterion, params, C)
    gamma = 2 if criterion == "advanced" else 0
    table, _ = ls.loss_sums_np(logits, target, gamma)
    return loss_grad_np(logits, target, coefficients_from_sums(table, H * W, criterion, **kw), gamma)


def at_positions(g, pos):
    """[n, C] of a gradient [B,C,H,W] at flat (frame, pixel) positions."""
    B, C, H, W = g.shape
    return g.reshape(B, C, H * W).transpose(0, 2, 1).reshape(B * H * W, C)[pos]


def fixture_facts(g):
    """What the host test asserts of the fixture `g` (the loaded .npz as a dict), per scene and combination ->
    {(scene, criterion, params): (at, sums, e32, form)}: e32 and form as stored (over all positions); at = the largest
    |loss_grad_np - g64| / gmax at the stored positions; sums = the largest |plane sum of loss_grad_np - plane sum of g64|
    over the (frame, class) planes as a fraction of its bound
        3 u sum_plane |g| + 4 sqrt(H W) e32 gmax,      u = 2^-24.
    The first term is what acts coherently on a whole plane: the float32 rounding of the coefficients (K, and G + A: at
    most u relative each, three of them in an element, cancellation between k y and r ignored).  The second is the rest
    taken as H W independent errors of at most e32 gmax each without a common sign: their sum has a standard deviation of
    at most sqrt(H W) e32 gmax, four of which are allowed.  A bias of the per-pixel arithmetic (truncation in place of
    rounding, say) adds up as H W times itself and breaks this bound long before any element leaves the per-element bar."""
    out = {}
    for name in GRAD_SCENES:
        logits, target = ls.make_scene(name)
        assert ls.sha256(logits) == str(g[f"{name}_logits_sha"]) and ls.sha256(target) == str(g[f"{name}_target_sha"]), name
        pos = sample_positions(name)
        assert np.array_equal(pos, g[f"{name}_pos"]), name
        hw = logits.shape[2] * logits.shape[3]
        for criterion, params in GRAD_COMBOS:
            key = f"{name}_{criterion}_{params}"
            gmax, e32, form = (float(v) for v in g[f"{key}_stats"])
            got = scene_gradient(name, criterion, params).astype(np.float64)
            at = float(np.abs(at_positions(got, pos) - g[f"{key}_g64"]).max() / gmax)
            bound = 3 * 2.0 ** -24 * np.abs(got).sum((2, 3)) + 4 * np.sqrt(hw) * e32 * gmax
            sums = float((np.abs(got.sum((2, 3)) - g[f"{key}_sums"]) / bound).max())
            out[(name, criterion, params)] = (at, sums, e32, form)
    return out
