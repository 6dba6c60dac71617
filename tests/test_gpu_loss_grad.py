"""The loss gradients on the device (unetpp_loss_grad_f32, unetpp_loss_narrow_target_i64 and the modules of
unet_amd/loss_grad.py built on them) against the NumPy form, bit for bit: the kernel and loss_grad_np perform the same
float32 operations in the same order, and a pixel's gradient depends on that pixel and the coefficient table alone.
Run on the GPU box:  python -m pytest tests/test_gpu_loss_grad.py -m gpu"""
import ctypes

import numpy as np
import pytest

from unet_amd import loss as ls
from unet_amd import loss_grad as lg

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2                              # include/unetpp.h


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: the criteria need none


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def scene(shape, seed, logit_kind="plain", target_kind="plain"):
    B, C, H, W = shape
    return ls.make_logits(B, C, H, W, seed, logit_kind), ls.make_target(B, C, H, W, seed, target_kind)


def both_coef(logits, target, gamma):
    """A table with all four columns in use: CombinedLoss's coefficients plus AdvancedCombinedLoss's (weighted)."""
    C, hw = logits.shape[1], logits.shape[2] * logits.shape[3]
    table, _ = ls.loss_sums_np(logits, target, gamma)
    cw = ls.scene_class_weights(C)
    with np.errstate(all="ignore"):
        coef = (lg.coefficients_from_sums(table, hw, "combined", class_weights=cw, dice_ignore_bg=False, dice_skip_empty=False) +
                lg.coefficients_from_sums(table, hw, "advanced", class_weights=cw, focal_gamma=gamma))
    assert coef.dtype == np.float32 and np.isfinite(coef).all() and (coef != 0).all(-1).any()
    return coef


def check_grad(torch, model, logits, target, coef, gamma, scale=None, inplace=False):
    want = lg.loss_grad_np(logits, target, coef, gamma, scale)
    lgt = dev(torch, logits)
    got = lg.loss_grad(model, lgt, dev(torch, target), dev(torch, coef), gamma, None if scale is None else dev(torch, np.float32([scale])),
                       out=lgt if inplace else None)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == logits.shape
    assert (got.data_ptr() == lgt.data_ptr()) == inplace
    if not inplace:
        assert bool((bits(lgt.cpu().numpy()) == bits(logits)).all())                # the logits were not written
    got = got.cpu().numpy()
    bad = bits(got) != bits(want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
    return got


# ---- 1. the shapes at which the kernel can go wrong -----------------------------------------------------------------------------------
SHAPES = [(1, 2, 1, 1),        # one pixel
          (2, 3, 1, 3),        # less than one group
          (2, 3, 3, 5),        # H W = 15: every plane of every frame at another alignment
          (2, 3, 17, 23),      # C H W odd: the frames' pads differ, planes misaligned
          (1, 3, 64, 64),      # exactly one span
          (1, 3, 65, 64),      # one span plus 64 pixels
          (3, 7, 33, 57),      # seven classes, odd H W
          (2, 8, 16, 20)]      # C at its maximum


def test_span_is_what_the_shapes_assume():
    span = lg.layout()
    assert span == ls.layout() == 64 * 64 and 65 * 64 == span + 64


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(torch_cuda, model, shape):
    logits, target = scene(shape, 20 + shape[1])
    g = check_grad(torch_cuda, model, logits, target, both_coef(logits, target, 2), 2)
    assert np.isfinite(g).all() and (g != 0).any()


@pytest.mark.parametrize("gamma", range(5))
def test_gamma(torch_cuda, model, gamma):
    logits, target = scene((2, 3, 17, 23), 40)
    check_grad(torch_cuda, model, logits, target, both_coef(logits, target, gamma), gamma)


@pytest.mark.parametrize("shape", [(2, 3, 17, 23), (1, 3, 65, 64)], ids=lambda s: "x".join(map(str, s)))
def test_scale_and_in_place(torch_cuda, model, shape):
    """dev_scale NULL and set (the same bits as the unscaled gradient times the scale), and out=logits."""
    logits, target = scene(shape, 41)
    coef = both_coef(logits, target, 2)
    g = check_grad(torch_cuda, model, logits, target, coef, 2)
    gs = check_grad(torch_cuda, model, logits, target, coef, 2, scale=0.2)
    assert bool((bits(gs) == bits(g * np.float32(0.2))).all())
    check_grad(torch_cuda, model, logits, target, coef, 2, scale=-3.0)
    for scale in (None, 0.2):
        gi = check_grad(torch_cuda, model, logits, target, coef, 2, scale=scale, inplace=True)
        assert bool((bits(gi) == bits(g if scale is None else gs)).all())


@pytest.mark.parametrize("name", ["nonfinite3", "range7", "both3"])
def test_special_pixels_get_zero_rows(torch_cuda, model, name):
    logits, target = ls.make_scene(name)
    B, C, H, W = logits.shape
    g = check_grad(torch_cuda, model, logits, target, both_coef(logits, target, 2), 2, scale=-1.5)
    kind = ls.pixel_terms_np(logits, target)[4].reshape(B, H, W)
    assert (kind != 0).any() and (bits(g).transpose(0, 2, 3, 1)[kind != 0] == 0).all() and np.isfinite(g).all()


def test_extreme_logits(torch_cuda, model):
    """Logits at +-6e4 (the fp16 range) and +-3e38: d = -inf, p = 0, nll at its clamp; every gradient finite."""
    logits, target = scene((2, 3, 17, 23), 42)
    flat = logits.reshape(-1)
    r = np.random.default_rng(3)
    idx = r.permutation(flat.size)[:200]
    flat[idx] = np.resize(np.float32([6e4, -6e4, 3e38, -3e38]), idx.size)
    for gamma in (0, 2, 4):
        g = check_grad(torch_cuda, model, logits, target, both_coef(logits, target, gamma), gamma)
        assert np.isfinite(g).all()
    assert (ls.pixel_terms_np(logits, target)[1] > 131072).any()                  # the clamp was reached


def test_repeating_a_call_returns_the_same_bits(torch_cuda, model):
    torch = torch_cuda
    logits, target = scene((3, 7, 33, 57), 43)
    args = (dev(torch, logits), dev(torch, target), dev(torch, both_coef(logits, target, 2)), 2)
    runs = [lg.loss_grad(model, *args).cpu().numpy().tobytes() for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


# ---- 2. the int64 target -------------------------------------------------------------------------------------------------------------
def test_narrow_target(torch_cuda, model):
    torch = torch_cuda
    r = np.random.default_rng(4)
    for n in (1, 15, 16, 17, 782, 3 * 33 * 57):
        t = r.integers(0, 8, n).astype(np.int64)
        t[r.permutation(n)[:max(1, n // 5)]] = np.resize(np.int64([-100, 254, 255, 256, -1, 2 ** 40, -2 ** 63, 2 ** 63 - 1, 300]), max(1, n // 5))
        want = np.where((t >= 0) & (t <= 254), t, 255).astype(np.uint8)
        got = lg.narrow_target(model, dev(torch, t))
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), n
    shaped = lg.narrow_target(model, dev(torch, np.arange(24, dtype=np.int64).reshape(2, 3, 4)))
    assert tuple(shaped.shape) == (2, 3, 4) and shaped.cpu().numpy().reshape(-1).tolist() == list(range(24))


# ---- 3. the modules -------------------------------------------------------------------------------------------------------------------
CASES = [("combined", dict(class_weights=[0.5, 1.0, 2.0])), ("combined", dict(weight_ce=0.7, weight_dice=1.3, dice_ignore_bg=False, dice_skip_empty=False)),
         ("advanced", dict()), ("advanced", dict(class_weights=[0.5, 1.0, 2.0], dice_ignore_bg=False, focal_gamma=3))]


def make_module(criterion, model, **kw):
    return (lg.CombinedLoss if criterion == "combined" else lg.AdvancedCombinedLoss)(model, **kw)


def chain_scale(torch):
    """d (0.4 * loss / 2) / d loss as torch computes it in float32."""
    s = torch.ones((), dtype=torch.float32, requires_grad=True)
    (0.4 * s / 2).backward()
    return np.float32(s.grad.item())


@pytest.mark.parametrize("criterion,kw", CASES, ids=lambda v: v if isinstance(v, str) else "-".join(v) or "defaults")
def test_modules(torch_cuda, model, criterion, kw):
    """Values == loss.combined_loss / advanced_combined_loss; pred.grad after (0.4 * loss / 2).backward() == the NumPy form
    with that float32 scale; int64 and uint8 targets give the same bits."""
    torch = torch_cuda
    logits, target = scene((2, 3, 17, 23), 50)
    gamma = int(kw.get("focal_gamma", 2)) if criterion == "advanced" else 0
    loss_kw = {k: v for k, v in kw.items() if k != "focal_gamma"}
    want = (ls.combined_loss(model, dev(torch, logits), dev(torch, target), **loss_kw) if criterion == "combined" else
            ls.advanced_combined_loss(model, dev(torch, logits), dev(torch, target), focal_gamma=gamma, **loss_kw))
    table, _ = ls.loss_sums_np(logits, target, gamma)
    coef = lg.coefficients_from_sums(table, 17 * 23, criterion, **kw)
    want_grad = lg.loss_grad_np(logits, target, coef, gamma, chain_scale(torch))
    module = make_module(criterion, model, **kw)
    grads = []
    for tgt in (dev(torch, target), dev(torch, target.astype(np.int64))):
        pred = dev(torch, logits).requires_grad_()
        out = module(pred, tgt)
        loss = out[0]
        assert isinstance(loss, torch.Tensor) and loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
        assert tuple(out[1:]) == tuple(want[1:]) and all(isinstance(v, float) for v in out[1:])
        assert loss.item() == float(np.float32(want[0]))
        (0.4 * loss / 2).backward()
        grads.append(pred.grad.cpu().numpy())
        assert bool((bits(grads[-1]) == bits(want_grad)).all())
    assert grads[0].tobytes() == grads[1].tobytes()


def test_module_without_grad_half_and_check(torch_cuda, model):
    torch = torch_cuda
    logits, target = scene((2, 3, 17, 23), 51)
    module = lg.CombinedLoss(model)
    # no gradient asked for: a plain tensor, no graph
    for pred in (dev(torch, logits), ):
        loss = module(pred, dev(torch, target))[0]
        assert loss.grad_fn is None and not loss.requires_grad
    with torch.no_grad():
        assert module(dev(torch, logits).requires_grad_(), dev(torch, target))[0].grad_fn is None
    # half logits: torch's own cast before the Function, the gradient flows back through it
    half = dev(torch, logits).half().requires_grad_()
    out = module(half, dev(torch, target))
    out[0].backward()
    l32 = half.detach().float().cpu().numpy()
    table, _ = ls.loss_sums_np(l32, target, 0)
    want = lg.loss_grad_np(l32, target, lg.coefficients_from_sums(table, 17 * 23, "combined"), 0, np.float32(1.0))
    assert half.grad.dtype == torch.float16 and torch.equal(half.grad.cpu(), torch.from_numpy(want).half())
    assert out[1:] == ls.combined_loss(model, half.detach().float(), dev(torch, target))[1:]
    # check=True raises as loss._raise_outside does; ignore_index -100 becomes 255
    bad = target.astype(np.int64)
    bad[1, 3, 3] = -100
    with pytest.raises(ValueError, match=r"^frame 1: 1 pixels have a target >= num_classes 3"):
        module(dev(torch, logits).requires_grad_(), dev(torch, bad))
    pred = dev(torch, logits).requires_grad_()
    lg.CombinedLoss(model, check=False)(pred, dev(torch, bad))[0].backward()
    assert bool((pred.grad[1, :, 3, 3] == 0).all()) and bool((pred.grad[1, :, 3, 4] != 0).all())


@pytest.mark.parametrize("criterion", ls.CRITERIA)
def test_deep_supervision_criterion(torch_cuda, model, criterion):
    """Four random logit tensors against four separate module calls combined as tools/train_3class_advanced.py:294-304 does:
    the same loss, tuples and gradients, bit for bit."""
    torch = torch_cuda
    B, C, H, W = 2, 3, 17, 23
    target = dev(torch, ls.make_target(B, C, H, W, 60).astype(np.int64))
    maps = [ls.make_logits(B, C, H, W, 60 + k) for k in range(4)]
    module = make_module(criterion, model, class_weights=[0.5, 1.0, 2.0])
    a = [dev(torch, m).requires_grad_() for m in maps]
    loss_a, parts_a = 0.0, []
    for o, w in zip(a, lg.DS_WEIGHTS):
        r = module(o, target)
        parts_a.append(r)
        loss_a += w * r[0]
    (loss_a / 2).backward()
    b = [dev(torch, m).requires_grad_() for m in maps]
    loss_b, parts_b = lg.deep_supervision_criterion(module, b, target)
    (loss_b / 2).backward()
    assert loss_a.item() == loss_b.item() and len(parts_b) == 4
    for pa, pb, x, y in zip(parts_a, parts_b, a, b):
        assert pa[0].item() == pb[0].item() and tuple(pa[1:]) == tuple(pb[1:])
        assert x.grad.cpu().numpy().tobytes() == y.grad.cpu().numpy().tobytes() and bool((x.grad != 0).any())
    # fewer outputs take the last weights
    two, _ = lg.deep_supervision_criterion(module, [dev(torch, m) for m in maps[:2]], target)
    assert two.grad_fn is None and two.item() == (0.3 * parts_a[0][0].detach() + 0.4 * parts_a[1][0].detach()).item()


# ---- 4. the C ABI's refusals ------------------------------------------------------------------------------------------------------------
def test_c_abi_errors_launch_nothing(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    lgt = torch.zeros((2 * 3 * 4 * 5 + 8,), dtype=torch.float32, device="cuda")
    tg = torch.zeros((1, 4, 5), dtype=torch.uint8, device="cuda")
    model._input(tg, "target")                                   # makes the engine
    coef = torch.zeros((1, 3, 4), dtype=torch.float32, device="cuda")
    grad = torch.full((1, 3, 4, 5), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    h = model._handle
    f = lib.unetpp_loss_grad_f32
    assert f(None, p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef), None, p(grad), None) == E_INVALID
    for args in ((None, p(tg), 1, 3, 4, 5, 2, p(coef), None, p(grad)), (p(lgt), None, 1, 3, 4, 5, 2, p(coef), None, p(grad)),
                 (p(lgt), p(tg), 1, 3, 4, 5, 2, None, None, p(grad)), (p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef), None, None),
                 (p(lgt), p(tg), 0, 3, 4, 5, 2, p(coef), None, p(grad)), (p(lgt), p(tg), 65536, 3, 4, 5, 2, p(coef), None, p(grad)),
                 (p(lgt), p(tg), 1, 1, 4, 5, 2, p(coef), None, p(grad)), (p(lgt), p(tg), 1, 9, 4, 5, 2, p(coef), None, p(grad)),
                 (p(lgt), p(tg), 1, 3, 0, 5, 2, p(coef), None, p(grad)), (p(lgt), p(tg), 1, 3, 2049, 2048, 2, p(coef), None, p(grad)),
                 (p(lgt), p(tg), 1, 3, 4, 5, -1, p(coef), None, p(grad)), (p(lgt), p(tg), 1, 3, 4, 5, 5, p(coef), None, p(grad)),
                 (p(lgt, 2), p(tg), 1, 3, 4, 5, 2, p(coef), None, p(grad)), (p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef, 2), None, p(grad)),
                 (p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef), p(coef, 2), p(grad)), (p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef), None, p(grad, 2)),
                 (p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef), None, p(lgt, 4)),          # a partial overlap of gradient and logits
                 (p(lgt, 16), p(tg), 1, 3, 4, 5, 2, p(coef), None, p(lgt)),
                 (p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef), None, p(coef)), (p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef), p(grad, 8), p(grad))):
        assert f(h, *args, None) == E_UNSUPPORTED, args
    n = lib.unetpp_loss_narrow_target_i64
    src = torch.zeros((8,), dtype=torch.int64, device="cuda")
    dst = torch.full((64,), 9, dtype=torch.uint8, device="cuda")
    assert n(None, p(src), 8, p(dst), None) == E_INVALID
    for args in ((None, 8, p(dst)), (p(src), 8, None), (p(src), 0, p(dst)), (p(src), -1, p(dst)), (p(src), 65535 * 2 ** 22 + 1, p(dst)),
                 (p(src, 4), 4, p(dst)), (p(src), 8, p(src, 8)), (p(src), 8, p(src, 63))):
        assert n(h, *args, None) == E_UNSUPPORTED, args
    torch.cuda.synchronize()
    assert bool((grad == 7).all()) and bool((lgt == 0).all()) and bool((dst == 9).all()) and bool((src == 0).all())
    # the exact alias is allowed
    assert f(h, p(lgt), p(tg), 1, 3, 4, 5, 2, p(coef), None, p(lgt), None) == 0
    torch.cuda.synchronize()
