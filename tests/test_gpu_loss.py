"""The validation-loss sums on the device (unetpp_loss_sums_f32 and the functions of unet_amd/loss.py built on it) against
the NumPy form, bit for bit (== on both tensors: the kernel and loss_sums_np perform the same float32 operations and add
integers), and the losses against the reference's float64 run within the reference's own float32 noise
(tests/golden/loss_scenes.npz, d32).
Run on the GPU box:  python -m pytest tests/test_gpu_loss.py -m gpu"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import loss as ls

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
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: the sums need none


@pytest.fixture(scope="module")
def net(torch_cuda, syn):
    """A small synthetic 3-class model with deep supervision, for the calls that run the network."""
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=True, max_batch=3, max_hw=(48, 80)).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    return m.eval()


@pytest.fixture(scope="module")
def golden():
    g = load_golden("loss_scenes")
    return {k: g[k] for k in g.files}


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def embedded(torch, a, offset):
    """A CUDA view of `a` at byte `offset` of a larger buffer whose other bytes are 255 (uint8 255, float32 NaN)."""
    buf = torch.full((a.nbytes + offset + 64,), 255, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + a.nbytes].view(getattr(torch, str(a.dtype))).view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == (buf.data_ptr() + offset) % 16
    return view


def check_sums(torch, model, logits, target, gamma=2, logits_dev=None, target_dev=None):
    want_t, want_o = ls.loss_sums_np(logits, target, gamma)
    got_t, got_o = ls.loss_sums(model, dev(torch, logits) if logits_dev is None else logits_dev,
                                dev(torch, target) if target_dev is None else target_dev, gamma)
    assert got_t.dtype == torch.int64 and got_o.dtype == torch.int32 and got_t.is_cuda and got_o.is_cuda
    got_t, got_o = got_t.cpu().numpy().view(np.uint64), got_o.cpu().numpy().view(np.uint32)
    assert got_t.shape == want_t.shape and got_o.shape == want_o.shape
    assert bool((got_t == want_t).all()) and bool((got_o == want_o).all()), (np.argwhere(got_t != want_t)[:4], got_o, want_o)
    hw = logits.shape[2] * logits.shape[3]
    assert bool((got_t[:, :, 0].sum(1) + got_o.sum(1) == hw).all())
    return got_t, got_o


def scene(shape, seed, logit_kind="plain", target_kind="plain"):
    B, C, H, W = shape
    return ls.make_logits(B, C, H, W, seed, logit_kind), ls.make_target(B, C, H, W, seed, target_kind)


# ---- 1. the shapes at which the kernel can go wrong -------------------------------------------------------------------------------
SHAPES = [(1, 2, 1, 1),        # one pixel
          (3, 3, 17, 23),      # odd H W: every plane of every frame at another alignment
          (2, 7, 5, 9),        # H W smaller than one group per thread
          (2, 8, 16, 20),      # C at its maximum
          (2, 3, 96, 100)]     # three workgroup spans per frame, the last one partial


def test_span_is_what_the_shapes_assume():
    span = ls.layout()
    assert span == 4096 and 2 * span < 96 * 100 < 3 * span and 5 * 9 < 256


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["plain", "confident", "uniform", "wide"])
def test_shapes(torch_cuda, model, shape, kind):
    logits, target = scene(shape, 20 + shape[1], kind)
    t, o = check_sums(torch_cuda, model, logits, target)
    assert not o.any()
    if kind == "wide" and shape[2] * shape[3] > 100:
        assert (ls.pixel_terms_np(logits, target)[0] == 0).any()             # exp32 underflowed somewhere


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_views(torch_cuda, model, shape):
    """Logits 4, 8 and 12 bytes off a 16-byte boundary, the target at odd bytes, in buffers of NaN and 255: a read outside
    the tensors would land in `outside`."""
    logits, target = scene(shape, 31)
    want = None
    for off_l, off_t in ((0, 0), (4, 1), (8, 2), (12, 3), (4, 15), (16, 7)):
        t, o = check_sums(torch_cuda, model, logits, target, logits_dev=embedded(torch_cuda, logits, off_l),
                          target_dev=embedded(torch_cuda, target, off_t))
        assert not o.any()
        want = t if want is None else want
        assert bool((t == want).all())


@pytest.mark.parametrize("gamma", [0, 2, 3])
def test_gamma(torch_cuda, model, gamma):
    logits, target = scene((2, 3, 24, 40), 40)
    t, _ = check_sums(torch_cuda, model, logits, target, gamma)
    if gamma == 0:
        assert bool((t[:, :, 4] == t[:, :, 3]).all())


@pytest.mark.parametrize("name", [s[0] for s in ls.LOSS_SCENES if s[6] in ls.SPECIAL or s[7] in ls.SPECIAL])
def test_special_pixels(torch_cuda, model, name):
    logits, target = ls.make_scene(name)
    _, o = check_sums(torch_cuda, model, logits, target)
    assert o.any()
    with pytest.raises(ValueError, match=r"^frame \d+: \d+ pixels have a target >= num_classes"):
        ls.combined_loss(model, dev(torch_cuda, logits), dev(torch_cuda, target))
    loss = ls.combined_loss(model, dev(torch_cuda, logits), dev(torch_cuda, target), check=False)
    assert all(np.isfinite(v) for v in loss)


def test_extreme_logits_reach_the_clamp(torch_cuda, model):
    x = np.zeros((1, 2, 1, 2), np.float32)
    x[0, 0, 0, 0], x[0, 1, 0, 0] = -3e38, 3e38
    t, o = check_sums(torch_cuda, model, x, np.uint8([[[0, 1]]]))
    assert not o.any() and t[0, 0].tolist() == [1, 2 ** 31, 0, 2 ** 41, 2 ** 41]


def test_one_class_frame_and_the_largest_frame(torch_cuda, model):
    """A frame of one class (every wave reduces its run once) and H W at its limit 2^22 (the last pixel index)."""
    logits, target = scene((1, 3, 96, 100), 41, "plain", "background")
    check_sums(torch_cuda, model, logits, target)
    r = np.random.default_rng(5)
    big = r.normal(0, 2, (1, 2, 2048, 2048)).astype(np.float32)
    tb = (r.random((1, 2048, 2048)) < 0.3).astype(np.uint8)
    tb[0, -1, -1] = 9
    _, o = check_sums(torch_cuda, model, big, tb)
    assert o.tolist() == [[1, 0]]


def test_two_runs_and_batches_agree(torch_cuda, model):
    """Two runs bitwise equal; a frame's row is the same in batches of 1 and 3."""
    torch = torch_cuda
    logits, target = scene((3, 7, 48, 80), 42)
    lg, tg = dev(torch, logits), dev(torch, target)
    runs = [b"".join(x.cpu().numpy().tobytes() for x in ls.loss_sums(model, lg, tg)) for _ in range(2)]
    assert runs[0] == runs[1]
    t3, o3 = ls.loss_sums(model, lg, tg)
    for b in range(3):
        t1, o1 = ls.loss_sums(model, lg[b:b + 1], tg[b:b + 1])
        assert torch.equal(t1[0], t3[b]) and torch.equal(o1[0], o3[b])


# ---- 2. the losses against the reference ---------------------------------------------------------------------------------------------
def test_losses_against_the_reference(torch_cuda, model, golden):
    """combined_loss and advanced_combined_loss on the fixture scenes: each number within d32 (relative) of the reference's
    float64 run, and equal to the algebra on the NumPy form's table."""
    torch = torch_cuda
    d32 = dict(zip(ls.LOSSES, golden["d32"]))
    n = 0
    for name, B, C, H, W, seed, lk, tk in ls.LOSS_SCENES:
        if lk in ls.SPECIAL or tk in ls.SPECIAL:
            continue
        logits, target = ls.make_scene(name)
        lg, tg = dev(torch, logits), dev(torch, target)
        table = ls.loss_sums_np(logits, target)[0]
        for j, (params, (ignore_bg, skip_empty, weighted)) in enumerate(ls.PARAM_SETS.items()):
            cw = ls.scene_class_weights(C) if weighted else None
            comb = ls.combined_loss(model, lg, tg, class_weights=cw, dice_ignore_bg=ignore_bg, dice_skip_empty=skip_empty)
            adv = ls.advanced_combined_loss(model, lg, tg, class_weights=cw, dice_ignore_bg=ignore_bg)
            got = np.array([comb[1], comb[2], adv[1], adv[2], comb[0], adv[0]])
            assert np.array_equal(got, ls.scene_losses(table, H * W, params)), (name, params)
            ref = golden[f"{name}_ref64"][j]
            for k, loss in enumerate(ls.LOSSES):
                assert abs(got[k] - ref[k]) <= d32[loss] * abs(ref[k]), (name, params, loss, got[k], ref[k])
            n += 1
    assert n >= 32


# ---- 3. the calls that run the network -----------------------------------------------------------------------------------------------
def frames(torch, syn, B, H, W, first=0):
    return torch.from_numpy(syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 7, first))).cuda()


@pytest.mark.parametrize("shape", [(1, 16, 16), (3, 16, 80), (2, 48, 80)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("criterion", ls.CRITERIA)
def test_deep_supervision_losses(torch_cuda, net, syn, shape, criterion):
    """The engine's own four maps: the losses equal the algebra on loss_sums_np of the maps read back."""
    torch = torch_cuda
    B, H, W = shape
    x = frames(torch, syn, B, H, W)
    target = ls.make_target(B, 3, H, W, 50)
    kw = dict(class_weights=[0.5, 1.0, 2.0])
    losses, mean = ls.deep_supervision_losses(net, x, dev(torch, target), criterion=criterion, **kw)
    maps = [o.cpu().numpy() for o in net.forward_deep_supervision(x)]
    assert len(losses) == 4
    for got, m in zip(losses, maps):
        table = ls.loss_sums_np(m, target, 2 if criterion == "advanced" else 0)[0]
        want = ls.combined_from_sums(table, **kw) if criterion == "combined" else ls.advanced_combined_from_sums(table, H * W, **kw)
        assert got == want and all(np.isfinite(v) and v > 0 for v in got)
    assert mean == float(np.mean([v[0] for v in losses]))
    assert len({v[0] for v in losses}) == 4                                        # four different maps


def test_evaluate_losses(torch_cuda, net, syn):
    """Three batches (the last one smaller) against per-batch calls: the same tuples, their mean, one table for all."""
    torch = torch_cuda
    H, W = 48, 80
    batches = [(frames(torch, syn, b, H, W, first), dev(torch, ls.make_target(b, 3, H, W, 60 + first))) for b, first in ((2, 0), (2, 2), (1, 4))]
    for criterion in ls.CRITERIA:
        got = ls.evaluate_losses(net, batches, criterion=criterion)
        one = ls.combined_loss if criterion == "combined" else ls.advanced_combined_loss
        want = [one(net, net.forward(x), t) for x, t in batches]
        assert got["losses"] == want and got["frames"] == 5
        assert np.array_equal(got["mean"], np.mean(np.array(want), 0))
        # an iterator has no length: the table grows by blocks
        again = ls.evaluate_losses(net, iter(batches), criterion=criterion, capacity=2)
        assert again["losses"] == want
    bad = batches[0][1].clone()
    bad[1, 3, 3] = 3
    with pytest.raises(ValueError, match="^frame 3: 1 pixels have a target >= num_classes 3"):
        ls.evaluate_losses(net, [batches[1], (batches[0][0], bad)])
    with pytest.raises(ValueError, match="at least one batch"):
        ls.evaluate_losses(net, [])


# ---- 4. the C ABI's refusals -----------------------------------------------------------------------------------------------------------
def test_c_abi_errors_launch_nothing(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    lg = torch.zeros((1, 3, 4, 5), dtype=torch.float32, device="cuda")
    tg = torch.zeros((1, 4, 5), dtype=torch.uint8, device="cuda")
    model._input(tg, "target")                                   # makes the engine
    table = torch.full((2 * 3 * 5,), 7, dtype=torch.int64, device="cuda")
    outside = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    h = model._handle
    f = lib.unetpp_loss_sums_f32
    assert f(None, p(lg), p(tg), 1, 3, 4, 5, 2, p(table), p(outside), None) == E_INVALID
    for args in ((None, p(tg), 1, 3, 4, 5, 2, p(table), p(outside)), (p(lg), None, 1, 3, 4, 5, 2, p(table), p(outside)),
                 (p(lg), p(tg), 1, 3, 4, 5, 2, None, p(outside)), (p(lg), p(tg), 1, 3, 4, 5, 2, p(table), None),
                 (p(lg), p(tg), 0, 3, 4, 5, 2, p(table), p(outside)), (p(lg), p(tg), 65536, 3, 4, 5, 2, p(table), p(outside)),
                 (p(lg), p(tg), 1, 1, 4, 5, 2, p(table), p(outside)), (p(lg), p(tg), 1, 9, 4, 5, 2, p(table), p(outside)),
                 (p(lg), p(tg), 1, 3, 0, 5, 2, p(table), p(outside)), (p(lg), p(tg), 1, 3, 4, 0, 2, p(table), p(outside)),
                 (p(lg), p(tg), 1, 3, 2049, 2048, 2, p(table), p(outside)), (p(lg), p(tg), 1, 3, 65536, 65536, 2, p(table), p(outside)),
                 (p(lg), p(tg), 1, 3, 4, 5, -1, p(table), p(outside)), (p(lg), p(tg), 1, 3, 4, 5, 5, p(table), p(outside)),
                 (p(lg, 2), p(tg), 1, 3, 4, 5, 2, p(table), p(outside)), (p(lg), p(tg), 1, 3, 4, 5, 2, p(table, 4), p(outside)),
                 (p(lg), p(tg), 1, 3, 4, 5, 2, p(table), p(outside, 2)), (p(lg), p(tg), 1, 3, 4, 5, 2, p(table), p(table, 8)),
                 (p(lg), p(tg), 1, 3, 4, 5, 2, p(lg), p(outside))):
        assert f(h, *args, None) == E_UNSUPPORTED, args
    torch.cuda.synchronize()
    assert bool((table == 7).all()) and bool((outside == 7).all())      # nothing was cleared, nothing was launched
    # outside directly behind the table, and apart from it: the same result
    raw = torch.full((3 * 5 + 1,), 7, dtype=torch.int64, device="cuda")
    assert f(h, p(lg), p(tg), 1, 3, 4, 5, 2, p(raw), p(raw, 3 * 5 * 8), None) == 0
    assert f(h, p(lg), p(tg), 1, 3, 4, 5, 2, p(table), p(outside), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw[:15], table[:15]) and torch.equal(raw[15:].view(torch.int32), outside[:2]) and int(table[0]) == 20
    assert bool((table[15:] == 7).all()) and bool((outside[2:] == 7).all())
