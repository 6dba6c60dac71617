"""Segmentation evaluation on the device (unetpp_confusion_u8, unetpp_mask_disagreement and the functions of
unet_amd/evaluation.py built on them) against the NumPy restatement and the fixtures made from the reference's own
functions (tests/golden/eval_scenes.npz).  Everything is an integer sum, a minimum or a maximum of float32 values: exact
equality everywhere, no tolerance, nothing left out.
Run on the GPU box:  python -m pytest tests/test_gpu_evaluation.py -m gpu"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import evaluation as ev

pytestmark = pytest.mark.gpu

IGNORE_INDICES = (-1, 0, 2)
E_INVALID = -1                                                 # UNETPP_E_INVALID of include/unetpp.h


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: only evaluate_batches needs any


@pytest.fixture(scope="module")
def span():
    """The pixels of a frame one workgroup owns, from the library."""
    n = ev.layout()
    assert n >= 256 and n % 16 == 0
    return n


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_pair(shape, C, seed, flip=0.3):
    """Masks with runs of every length: rows of make_eval_scene are too regular for shapes of a few pixels."""
    r = np.random.default_rng(seed)
    target = r.integers(0, C, shape).astype(np.uint8)
    target[r.random(shape) < 0.5] = 0
    pred = np.where(r.random(shape) < flip, r.integers(0, C, shape), target).astype(np.uint8)
    return pred, target


def embedded(torch, a, offset):
    """A [B,H,W] CUDA view at byte `offset` of a larger buffer whose other bytes are 255."""
    buf = torch.full((a.size + offset + 64,), 255, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == (buf.data_ptr() + offset) % 16
    return view


def check_confusion(torch, model, pred, target, C, ignore_value=None, pred_dev=None, target_dev=None, **kw):
    want_c, want_o = ev.confusion_np(pred, target, C, ignore_value)
    got_c, got_o = ev.confusion(model, dev(torch, pred) if pred_dev is None else pred_dev,
                                dev(torch, target) if target_dev is None else target_dev, C, ignore_value, **kw)
    assert got_c.dtype == got_o.dtype == torch.int64 and got_c.is_cuda
    got_c, got_o = got_c.cpu().numpy(), got_o.cpu().numpy()
    assert got_c.shape == want_c.shape and got_o.shape == want_o.shape
    assert np.array_equal(got_c, want_c) and np.array_equal(got_o, want_o), (got_c, want_c, got_o, want_o)
    assert np.array_equal(got_c.sum((1, 2)) + got_o.sum(1), np.full(pred.shape[0], pred.shape[1] * pred.shape[2]))
    return got_c, got_o


# ---- 1. the smallest and the misaligned shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 1, 1), (3, 5, 7), (2, 1, 16), (2, 1, 17), (5, 3, 21)])
def test_smallest_and_misaligned_shapes(torch_cuda, model, shape):
    pred, target = random_pair(shape, 3, 1)
    check_confusion(torch_cuda, model, pred, target, 3)
    if shape[0] > 1 and (shape[1] * shape[2]) % 16:
        # views into buffers of 255s: a byte read outside a frame's mask would land in `outside`
        for off_p, off_t in ((16, 16), (3, 3), (13, 29), (5, 9), (0, 7)):        # the last two: no common alignment
            c, o = check_confusion(torch_cuda, model, pred, target, 3, pred_dev=embedded(torch_cuda, pred, off_p),
                                   target_dev=embedded(torch_cuda, target, off_t))
            assert not o.any()


@pytest.mark.parametrize("extra", [0, 1])
def test_one_workgroup_span_and_a_pixel_more(torch_cuda, model, span, extra):
    pred, target = random_pair((2, 1, span + extra), 3, 2 + extra)
    check_confusion(torch_cuda, model, pred, target, 3)
    for off in (1, 15):                                        # the head moves the seam off the workgroup boundary
        c, o = check_confusion(torch_cuda, model, pred, target, 3, pred_dev=embedded(torch_cuda, pred, off),
                               target_dev=embedded(torch_cuda, target, off))
        assert not o.any()


# ---- 2. class counts ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene16():
    """One 40 x 64 scene with 16 classes in which every (target, pred) pair occurs."""
    pred, target = ev.make_eval_batch(2, 40, 64, 21, 16)
    combos = np.arange(256)
    target[1, :4] = (combos // 16).reshape(4, 64)
    pred[1, :4] = (combos % 16).reshape(4, 64)
    return pred, target


@pytest.mark.parametrize("C", [2, 3, 7, 16])
def test_class_counts(torch_cuda, model, scene16, C):
    pred, target = scene16[0] % C, scene16[1] % C
    c, o = check_confusion(torch_cuda, model, pred, target, C)
    assert not o.any()
    if C == 16:
        assert (c.sum(0) > 0).all()                            # every one of the 256 bins


# ---- 3. ignore and invalid ------------------------------------------------------------------------------------------------
def test_ignore_value_255(torch_cuda, model):
    pred, target = ev.make_eval_batch(2, 40, 64, 3, 3)
    target[np.random.default_rng(0).random(target.shape) < 0.1] = 255
    _, o = check_confusion(torch_cuda, model, pred, target, 3, ignore_value=255)
    assert o[:, 0].min() > 100 and not o[:, 1].any()


def test_ignore_value_0(torch_cuda, model):
    pred, target = ev.make_eval_batch(2, 40, 64, 3, 3)
    c, o = check_confusion(torch_cuda, model, pred, target, 3, ignore_value=0)
    assert np.array_equal(o[:, 0], (target == 0).sum((1, 2))) and not c[:, 0].any()


@pytest.mark.parametrize("where", ["pred", "target", "both"])
def test_values_outside_the_classes(torch_cuda, model, where):
    pred, target = ev.make_eval_batch(3, 24, 40, 4, 3)
    hit = np.zeros(pred.shape, bool)
    hit[1] = np.random.default_rng(1).random(pred.shape[1:]) < 0.02
    if where in ("pred", "both"):
        pred[hit] = 3
    if where in ("target", "both"):
        target[hit] = 200
    _, o = check_confusion(torch_cuda, model, pred, target, 3, check=False)
    assert o[:, 1].tolist() == [0, int(hit.sum()), 0] and hit.sum() > 0
    with pytest.raises(ValueError, match=rf"^frame 1: {int(hit.sum())} pixels"):
        ev.confusion(model, dev(torch_cuda, pred), dev(torch_cuda, target), 3)
    if where == "target":                                      # ignored, the same pixels are no error
        check_confusion(torch_cuda, model, pred, target, 3, ignore_value=200, check=True)
    else:                                                      # ignored target, invalid pred: ignored only
        target[hit] = 255
        _, o = check_confusion(torch_cuda, model, pred, target, 3, ignore_value=255, check=True)
        assert o.tolist() == [[0, 0], [int(hit.sum()), 0], [0, 0]]


# ---- 4. counter width and contention --------------------------------------------------------------------------------------
def test_one_bin_holds_more_than_16_bits(torch_cuda, model):
    pred = np.full((1, 300, 300), 1, np.uint8)
    target = np.full((1, 300, 300), 2, np.uint8)
    c, _ = check_confusion(torch_cuda, model, pred, target, 3)
    assert c[0, 2, 1] == 90000 > 65535
    pred[0, -1, -1] = 0                                        # a single odd pixel at the last index
    c, _ = check_confusion(torch_cuda, model, pred, target, 3)
    assert c[0, 2, 1] == 89999 and c[0, 2, 0] == 1


# ---- 5. the running total -------------------------------------------------------------------------------------------------
def test_running_total(torch_cuda, model):
    torch = torch_cuda
    C = 3
    p1, t1 = ev.make_eval_batch(2, 33, 57, 5, C)
    p2, t2 = ev.make_eval_batch(3, 24, 40, 6, C)
    t2[np.random.default_rng(2).random(t2.shape) < 0.05] = 255
    p2[0, 0, :3] = 9
    total = torch.zeros((C * C + 2,), dtype=torch.int64, device="cuda")
    c1, o1 = check_confusion(torch, model, p1, t1, C, ignore_value=255, total=total)
    c2, o2 = check_confusion(torch, model, p2, t2, C, ignore_value=255, total=total, check=False)
    want = np.concatenate([(c1.sum(0) + c2.sum(0)).ravel(), o1.sum(0) + o2.sum(0)])
    assert np.array_equal(total.cpu().numpy(), want) and want[-1] == 3 and want[-2] > 0
    # a call without `total` leaves an existing one untouched
    check_confusion(torch, model, p1, t1, C)
    assert np.array_equal(total.cpu().numpy(), want)
    host = np.zeros((C * C + 2,), np.int64)
    ev.confusion_np(p1, t1, C, 255, total=host)
    ev.confusion_np(p2, t2, C, 255, total=host)
    assert np.array_equal(host, want)


def test_running_total_carries_into_the_high_word(torch_cuda, model):
    torch = torch_cuda
    pred = np.zeros((1, 4, 5), np.uint8)
    total = torch.zeros((3 * 3 + 2,), dtype=torch.int64, device="cuda")
    total[0] = 2 ** 32 - 5
    ev.confusion(model, dev(torch, pred), dev(torch, pred), 3, total=total)
    got = total.cpu().numpy()
    assert int(got[0]) == 2 ** 32 - 5 + 20 == 2 ** 32 + 15 and not got[1:].any()


def test_total_argument_errors(torch_cuda, model):
    torch = torch_cuda
    m = dev(torch, np.zeros((1, 4, 5), np.uint8))
    for total in (torch.zeros((10,), dtype=torch.int64, device="cuda"), torch.zeros((11,), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError, match="total must be int64"):
            ev.confusion(model, m, m, 3, total=total)
    with pytest.raises(ValueError, match="contiguous"):
        ev.confusion(model, m, m, 3, total=torch.zeros((22,), dtype=torch.int64, device="cuda")[::2])
    with pytest.raises(ValueError, match="shapes must be equal"):
        ev.confusion(model, m, m[:, :3], 3)
    for C in (1, 17):
        with pytest.raises(ValueError, match="num_classes"):
            ev.confusion(model, m, m, C)
    assert ev.confusion(model, m, m)[0].shape == (1, 3, 3)       # num_classes=None: the model's


# ---- 6. reproducible ------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes(torch_cuda, model):
    torch = torch_cuda
    pred, target = ev.make_eval_batch(4, 96, 200, 8, 7)
    p, t = dev(torch, pred), dev(torch, target)
    lg = torch.from_numpy(np.random.default_rng(3).normal(0, 1, (4, 7, 96, 200)).astype(np.float32)).cuda()
    runs = []
    for _ in range(2):
        total = torch.zeros((51,), dtype=torch.int64, device="cuda")
        c, o = ev.confusion(model, p, t, 7, total=total)
        d = ev.mask_disagreement(model, p, t, lg)
        runs.append(b"".join(x.cpu().numpy().tobytes() for x in (c, o, total, d["n_diff"], d["first"], d["max_margin"], d["n_nan"])))
    assert runs[0] == runs[1]


# ---- 7. the reference's fixtures ------------------------------------------------------------------------------------------
def pack(result, C):
    miou, precision, recall, iou = result
    return np.array([miou] + [float(d.get(c, -1.0)) for d in (precision, recall, iou) for c in range(C)], np.float64)


def test_fixtures(torch_cuda, model):
    g = load_golden("eval_scenes")
    assert len(g["cases"]) >= 12
    for tag, C, B, H, W, seed, variant, _, _ in g["cases"]:
        C, B, H, W, seed = int(C), int(B), int(H), int(W), int(seed)
        pred, target = ev.make_eval_batch(B, H, W, seed, C, variant)
        counts, _ = check_confusion(torch_cuda, model, pred, target, C)
        assert np.array_equal(counts.sum(0), g[tag + "_cm"]), tag
        for k in IGNORE_INDICES:
            got, want = pack(ev.metrics_from_confusion(counts, k), C), g[f"{tag}_m{k}"]
            assert got.shape == want.shape and bool((got == want).all()), (tag, k, got, want)       # == on the floats
        ipc = np.stack([ev.iou_per_class_from_confusion(f) for f in counts])
        assert np.array_equal(ipc, g[tag + "_ipc"]), tag


# ---- 8. disagreement ------------------------------------------------------------------------------------------------------
def check_disagreement(torch, model, a, b, logits=None, a_dev=None, b_dev=None):
    want = ev.disagreement_np(a, b, logits)
    got = ev.mask_disagreement(model, dev(torch, a) if a_dev is None else a_dev, dev(torch, b) if b_dev is None else b_dev,
                               None if logits is None else dev(torch, logits))
    assert set(got) == set(want)
    assert got["first"].dtype == torch.int32 and got["n_diff"].dtype == torch.int64
    out = {k: v.cpu().numpy() for k, v in got.items()}
    for k in want:
        assert out[k].shape == want[k].shape, k
        if k == "max_margin":
            assert out[k].dtype == np.float32 and out[k].tobytes() == want[k].tobytes(), (out[k], want[k])     # bit for bit
        else:
            assert np.array_equal(out[k], want[k]), (k, out[k], want[k])
    return out


def test_disagreement_identical_first_and_last(torch_cuda, model, span):
    a = ev.make_eval_batch(3, 1, span + 1, 9, 3)[0]
    d = check_disagreement(torch_cuda, model, a, a.copy())
    assert d["n_diff"].tolist() == [0, 0, 0] and d["first"].tolist() == [-1, -1, -1]
    b = a.copy()
    b[0, 0, 0] ^= 1
    b[2, 0, -1] ^= 1
    d = check_disagreement(torch_cuda, model, a, b)
    assert d["n_diff"].tolist() == [1, 0, 1] and d["first"].tolist() == [0, -1, span]
    d = check_disagreement(torch_cuda, model, a, b, a_dev=embedded(torch_cuda, a, 7), b_dev=embedded(torch_cuda, b, 23))
    assert d["first"].tolist() == [0, -1, span]


def test_disagreement_random_small_pair(torch_cuda, model):
    a, b = random_pair((3, 5, 7), 3, 4)
    d = check_disagreement(torch_cuda, model, a, b)
    assert d["n_diff"].min() > 0
    for off_a, off_b in ((3, 3), (1, 6)):
        check_disagreement(torch_cuda, model, a, b, a_dev=embedded(torch_cuda, a, off_a), b_dev=embedded(torch_cuda, b, off_b))


@pytest.mark.parametrize("C", [3, 7])
def test_disagreement_with_logits(torch_cuda, model, C):
    a, b = ev.make_eval_batch(2, 33, 57, 10, C)
    lg = np.random.default_rng(C).normal(0, 3, (2, C, 33, 57)).astype(np.float32)
    d = check_disagreement(torch_cuda, model, a, b, lg)
    assert d["max_margin"].min() > 1.0 and d["n_diff"].min() > 10 and not d["n_nan"].any()
    d = check_disagreement(torch_cuda, model, a, a.copy(), lg)
    assert d["max_margin"].tolist() == [0.0, 0.0]


def test_disagreement_values_outside_the_logits_and_nan(torch_cuda, model):
    a, b = ev.make_eval_batch(2, 24, 40, 11, 3)
    lg = np.random.default_rng(5).normal(0, 3, (2, 3, 24, 40)).astype(np.float32)
    plain = ev.disagreement_np(a, b, lg)
    la = np.take_along_axis(lg[0], a[0][None].astype(np.int64), 0)[0]
    lb = np.take_along_axis(lg[0], b[0][None].astype(np.int64), 0)[0]
    margin = np.where(a[0] != b[0], np.abs(la - lb), -1.0)
    y, x = np.unravel_index(margin.argmax(), margin.shape)
    assert margin[y, x] == plain["max_margin"][0]
    b2 = b.copy()
    b2[0, y, x] = 3                                            # the pixel with the largest margin now holds a value >= C
    d = check_disagreement(torch_cuda, model, a, b2, lg)
    assert d["n_diff"][0] == plain["n_diff"][0] and d["max_margin"][0] < plain["max_margin"][0]
    lg2 = lg.copy()
    lg2[0, a[0, y, x], y, x] = np.nan                          # NaN at a differing pixel: counted, not in the maximum
    lg2[1, :, 0, 0] = np.nan                                   # and where the masks may agree
    d = check_disagreement(torch_cuda, model, a, b, lg2)
    assert d["n_nan"][0] == 1 and d["max_margin"][0] < plain["max_margin"][0] and not np.isnan(d["max_margin"]).any()
    lg3 = lg.copy()
    lg3[0, a[0, y, x], y, x] = np.inf                          # an infinite margin is a maximum, not a NaN
    d = check_disagreement(torch_cuda, model, a, b, lg3)
    assert np.isinf(d["max_margin"][0]) and d["n_nan"][0] == 0


# ---- 9. evaluate_batches on a small golden -----------------------------------------------------------------------------------
def test_evaluate_batches(torch_cuda, syn):
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    g = load_golden("s_c3_64x64")
    B, H, W, C = int(g["B"]), int(g["H"]), int(g["W"]), int(g["num_classes"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    net = NestedUNet(C, deep_supervision=bool(g["deep_supervision"]), max_batch=B, max_hw=(H, W)).to("cuda:0")
    net.load_state_dict(syn.make_state_dict(C, 3, bool(g["deep_supervision"]), int(g["wseed"])), strict=True)
    net.eval()
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    xs = [x, torch.flip(x, dims=[3]).contiguous()]
    masks = [net.segment(v).cpu().numpy() for v in xs]
    assert np.array_equal(masks[0], g["mask"])
    r = np.random.default_rng(12)
    targets = []
    for m in masks:                                            # a seeded target: the mask with a tenth of the pixels relabelled
        t = m.copy()
        hit = r.random(t.shape) < 0.1
        t[hit] = r.integers(0, C, int(hit.sum()))
        t[r.random(t.shape) < 0.02] = 255
        targets.append(t)
    got = ev.evaluate_batches(net, [(v, dev(torch, t)) for v, t in zip(xs, targets)], ignore_value=255, per_image=True)
    counts, outside = ev.confusion_np(np.concatenate(masks), np.concatenate(targets), C, 255)
    miou, precision, recall, iou = ev.metrics_from_confusion(counts)
    assert (got["miou"], got["precision"], got["recall"], got["iou"]) == (miou, precision, recall, iou) and 0.0 < miou < 1.0
    assert got["confusion_matrix"].dtype == np.int64 and np.array_equal(got["confusion_matrix"], counts.sum(0))
    assert got["ignored"] == int(outside[:, 0].sum()) > 0 and got["invalid"] == 0
    per = np.stack([ev.iou_per_class_from_confusion(f) for f in counts])
    assert got["iou_per_image"].shape == (2 * B, C) and np.array_equal(got["iou_per_image"], per)
    assert np.array_equal(got["mean_iou_per_image"], per.mean(0))
    plain = ev.evaluate_batches(net, [(v, dev(torch, t)) for v, t in zip(xs, targets)], ignore_value=255)
    assert "iou_per_image" not in plain and plain["miou"] == miou
    with pytest.raises(ValueError, match="pixels have a target or pred value"):
        ev.evaluate_batches(net, [(v, dev(torch, t)) for v, t in zip(xs, targets)])        # the 255s without an ignore value


# ---- 10. the C ABI's refusals ---------------------------------------------------------------------------------------------
def test_c_abi_errors_launch_nothing(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    m = dev(torch, np.zeros((1, 4, 5), np.uint8))
    model._input(m, "mask")                                    # makes the engine
    counts = torch.full((16 * 16,), 7, dtype=torch.int32, device="cuda")
    outside = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    h = model._handle
    conf = lib.unetpp_confusion_u8
    assert conf(h, None, p(m), 1, 4, 5, 3, -1, p(counts), p(outside), None, None) == E_INVALID
    assert conf(h, p(m), None, 1, 4, 5, 3, -1, p(counts), p(outside), None, None) == E_INVALID
    assert conf(h, p(m), p(m), 1, 4, 5, 3, -1, None, p(outside), None, None) == E_INVALID
    assert conf(h, p(m), p(m), 1, 4, 5, 3, -1, p(counts), None, None, None) == E_INVALID
    assert conf(None, p(m), p(m), 1, 4, 5, 3, -1, p(counts), p(outside), None, None) == E_INVALID
    for C in (1, 17):
        assert conf(h, p(m), p(m), 1, 4, 5, C, -1, p(counts), p(outside), None, None) == E_INVALID
    for ign in (-2, 256):
        assert conf(h, p(m), p(m), 1, 4, 5, 3, ign, p(counts), p(outside), None, None) == E_INVALID
    for b, hh, ww in ((0, 4, 5), (1, 0, 5), (1, 4, 0), (1, 65536, 65536)):      # 2^32 pixels
        assert conf(h, p(m), p(m), b, hh, ww, 3, -1, p(counts), p(outside), None, None) == E_INVALID
    assert conf(h, p(m), p(m), 1, 4, 5, 3, -1, p(counts), p(outside), ctypes.c_void_p(counts.data_ptr() + 4), None) == E_INVALID
    dis = lib.unetpp_mask_disagreement
    assert dis(h, None, p(m), 1, 4, 5, None, 0, p(counts), p(outside), None, None, None) == E_INVALID
    assert dis(h, p(m), p(m), 1, 4, 5, None, 0, None, p(outside), None, None, None) == E_INVALID
    lg = torch.zeros((1, 3, 4, 5), dtype=torch.float32, device="cuda")
    assert dis(h, p(m), p(m), 1, 4, 5, p(lg), 3, p(counts), p(outside), None, None, None) == E_INVALID       # logits without their outputs
    assert dis(h, p(m), p(m), 1, 4, 5, p(lg), 0, p(counts), p(outside), p(counts), p(counts), None) == E_INVALID
    assert dis(h, p(m), p(m), 1, 32768, 65536, None, 0, p(counts), p(outside), None, None, None) == E_INVALID   # 2^31 pixels
    assert lib.unetpp_evaluation_layout(None) == E_INVALID
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and bool((outside == 7).all())      # nothing was cleared, nothing was launched
