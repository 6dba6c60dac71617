"""The device forms of unet_amd/multiclass.py on a real MI355X: every kernel against its NumPy form, bit for bit, at the smallest
shapes where it can still go wrong, the compositions against the reference's stored results (tests/golden/multiclass_scenes.npz,
scripts/make_golden_multiclass.py), determinism, refusals, and the loop with its two read-backs."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import frame_loop
from unet_amd import multiclass as mc

pytestmark = pytest.mark.gpu

COLORS = {1: (0, 255, 0), 2: (255, 0, 0), 3: (0, 0, 255), 5: (255, 0, 255), 6: (0, 165, 255), 9: (7, 8, 9)}      # 4 has none


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(7, max_batch=1, max_hw=(16, 16)).to("cuda:0")       # no weights: only the loop test needs any


@pytest.fixture(scope="module")
def golden():
    return load_golden("multiclass_scenes")


def dev(torch, a, offset=0):
    """A CUDA copy of `a`; with offset, a view at that BYTE offset of a larger buffer filled with 255."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    assert a.dtype == np.uint8
    buf = torch.full((a.size + offset + 64,), 255, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + a.size].view(*a.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == offset % 16
    return view


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def same_gate(got, want):
    """Every output of the gate equals the NumPy form bit for bit."""
    is_bad, reason, lap_var, gray_std, mad, gray = host(*got)
    assert is_bad.dtype == np.bool_ and reason.dtype == np.uint8 and lap_var.dtype == np.float64
    assert np.array_equal(gray, want[5])
    assert np.array_equal(is_bad, want[0]) and np.array_equal(reason, want[1])
    for g, w in zip((lap_var, gray_std, mad), want[2:5]):
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (g, w)


# six planes and 42 rows of reach on a map 1500 wide do not fit bands of full-width rows: tiles with a halo on all four sides
PLANES_WIDE = (((1,), (("close", ("rect", 21)),), 1), ((2,), (("dilate", ("ellipse", (9, 3))),), 7), ((3,), (), 3), ((4,), (), -1),
               ((5,), (), 5), ((6,), (), 8))


def class_noise(shape, r):
    """Classes 0..6 in blocks with sparse single-pixel noise: material for the closes and the merge order."""
    b, h, w = shape
    blocks = r.integers(0, 7, (b, (h + 4) // 5, (w + 4) // 5), dtype=np.uint8)
    m = blocks.repeat(5, 1).repeat(5, 2)[:, :h, :w].copy()
    noise = r.random(shape) < 0.08
    m[noise] = r.integers(0, 7, int(noise.sum()), dtype=np.uint8)
    return m


def seam_scene(b, h, w, band, cols, as_bits):
    """Structures straddling the rows k * band and the columns k * cols: gaps one pixel wide in bands of class 1 and 2 (a close
    bridges them across the seam), defects on the seams, and noise."""
    r = np.random.default_rng(h * 1000 + w)
    m = np.zeros((b, h, w), np.uint8)
    m[:, :, : w // 2] = 1
    m[:, :, w // 2:] = 2
    for y in range(band, h, band):
        m[:, y - 1, ::2] = 0
        m[:, y, 1::3] = 0
        m[:, max(y - 2, 0):y + 2, w // 3:w // 3 + 5] = 3
    for x in range(cols, w, cols):
        m[:, ::2, x - 1] = 0
        m[:, 1::3, x] = 0
        m[:, h // 2:h // 2 + 4, max(x - 2, 0):x + 2] = 5
    noise = r.random(m.shape) < 0.03
    m[noise] = r.integers(0, 7, int(noise.sum()), dtype=np.uint8)
    if as_bits:
        m = (np.uint8(1) << m).astype(np.uint8) >> 1 & 31          # class k -> bit k - 1; 0 and 6 -> no bit
        m[noise] |= r.integers(0, 32, int(noise.sum()), dtype=np.uint8)
    return m


# ---- 1. the quality gate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 1, 33), (3, 17, 1), (2, 15, 17), (3, 33, 130), (1, 18, 264), (2, 1, 1)], ids=str)
def test_gate_equals_numpy_at_odd_shapes(torch_cuda, model, shape):
    torch = torch_cuda
    r = np.random.default_rng(sum(shape))
    frames = r.integers(0, 256, shape + (3,), dtype=np.uint8)
    prev = r.integers(0, 256, shape[1:], dtype=np.uint8)
    for p in (None, prev):
        for off in (0, 1):
            got = mc.quality_gate(model, dev(torch, frames, off), None if p is None else dev(torch, p, off))
            same_gate(got, mc.quality_gate_np(frames, p))
    got = mc.quality_gate(model, dev(torch, frames), dev(torch, prev), enable=False)
    same_gate(got, mc.quality_gate_np(frames, prev, enable=False))


def test_gate_reasons_and_extremes(torch_cuda, model):
    torch = torch_cuda
    frames = mc.make_gate_sequence(48, 80, 0)
    want = mc.quality_gate_np(frames, None)
    assert set(want[1].tolist()) == {1, 2, 3, 4}
    same_gate(mc.quality_gate(model, dev(torch, frames)), want)
    flat = np.stack([np.full((40, 72, 3), v, np.uint8) for v in (0, 255, 255)])
    checker = (np.indices((40, 72)).sum(0) % 2 * 255).astype(np.uint8)
    flat[2] = checker[..., None]                                   # the largest Laplacian and difference a frame can have
    same_gate(mc.quality_gate(model, dev(torch, flat), dev(torch, checker)), mc.quality_gate_np(flat, checker))
    with pytest.raises(ValueError, match="NaN"):
        mc.quality_gate(model, dev(torch, flat), blur_th=float("nan"))
    with pytest.raises(ValueError, match="prev_gray"):
        mc.quality_gate(model, dev(torch, flat), dev(torch, checker[:-1]))


# ---- 2. merge_classes and the class table ------------------------------------------------------------------------------------------
def check_merge(torch, model, mask, planes, lut=None, num_classes=256, off=0):
    want_m, want_t = mc.merge_classes_np(mask, planes, lut=lut, num_classes=num_classes)
    got_m, got_t = mc.merge_classes(model, dev(torch, mask, off), planes, lut=lut, num_classes=num_classes)
    assert got_m.dtype == torch.uint8 and got_t.dtype == torch.int32 and tuple(got_t.shape) == want_t.shape
    assert np.array_equal(got_m.cpu().numpy(), want_m), mask.shape
    assert np.array_equal(got_t.cpu().numpy(), want_t), (mask.shape, got_t.cpu().numpy()[0, :8], want_t[0, :8])
    return want_m, want_t


@pytest.mark.parametrize("shape", [(2, 1, 33), (2, 17, 1), (3, 15, 17), (1, 33, 64), (2, 40, 130)], ids=str)
def test_merge_equals_numpy_at_odd_shapes(torch_cuda, model, shape):
    r = np.random.default_rng(7 + sum(shape))
    mask = class_noise(shape, r)
    for off in (0, 1):
        check_merge(torch_cuda, model, mask, mc.PLANES_VIDEO, num_classes=7, off=off)
    bits = r.integers(0, 32, shape, dtype=np.uint8) & r.integers(0, 32, shape, dtype=np.uint8)
    check_merge(torch_cuda, model, bits, mc.PLANES_V3, lut=mc.LUT_BITS, num_classes=8)


@pytest.mark.parametrize("planes,lut", [(mc.PLANES_VIDEO, None), (mc.PLANES_V3, mc.LUT_BITS), (PLANES_WIDE, None)], ids=["video", "v3", "wide"])
def test_merge_across_workgroup_seams(torch_cuda, model, planes, lut):
    """Frames just over one band of rows, and for the wide programs (whose rows are split into tiles) several tiles across, with
    structures on the seams."""
    wide = planes is PLANES_WIDE
    h0, w0 = (200, 1500) if wide else (24, 200)
    band, cols = mc.merge_layout((2, h0, w0), planes, lut)
    h, w = band + 3, w0
    band2, cols2 = mc.merge_layout((2, h, w), planes, lut)
    assert band2 < h and (cols2 < w) == wide, (band, cols, band2, cols2)
    mask = seam_scene(2, h, w, band2, min(cols2, w), lut is not None)
    check_merge(torch_cuda, model, mask, planes, lut=lut, num_classes=9)


def test_merge_empty_full_borders_and_own_values(torch_cuda, model):
    torch = torch_cuda
    zero = np.zeros((2, 37, 70), np.uint8)
    _, t = check_merge(torch, model, zero, mc.PLANES_VIDEO, num_classes=7)
    assert t[0, 0].tolist() == [37 * 70, 0, 0, 69, 36] and (t[:, 1:, 0] == 0).all() and (t[:, 1:, 1:] == -1).all()
    one = np.full((1, 37, 70), 2, np.uint8)
    _, t = check_merge(torch, model, one, mc.PLANES_VIDEO, num_classes=7)
    assert t[0, 2].tolist() == [37 * 70, 0, 0, 69, 36] and t[0, 0].tolist() == [0, -1, -1, -1, -1]
    four = np.full((1, 20, 20), 4, np.uint8)
    m, _ = check_merge(torch, model, four, mc.PLANES_VIDEO, num_classes=7)
    assert not m.any()                                              # the untrained class disappears
    corners = np.zeros((1, 33, 47), np.uint8)
    corners[0, 0, 0] = corners[0, 32, 46] = 3
    corners[0, 0, 46] = corners[0, 32, 0] = 5
    corners[0, 16, :] = 200                                         # above num_classes: merged as itself, not tabulated
    planes = (((3, 5, 200), (), -1),)
    m, t = check_merge(torch, model, corners, planes, num_classes=7)
    assert t[0, 3].tolist() == [2, 0, 0, 46, 32] and t[0, 5].tolist() == [2, 0, 0, 46, 32] and (m[0, 16] == 200).all()
    want = mc.class_table_np(corners, 256)
    assert np.array_equal(mc.class_table(model, dev(torch, corners)).cpu().numpy(), want) and want[0, 200, 0] == 47
    assert np.array_equal(mc.class_table(model, dev(torch, corners, 1), 4).cpu().numpy(), mc.class_table_np(corners, 4))


def test_merge_refusals_leave_outputs_untouched(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    mask = torch.zeros((1, 32, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="planes"):
        mc.merge_classes(model, mask, [((1,), (), 1)] * 7)
    with pytest.raises(ValueError, match="reach"):
        mc.merge_classes(model, mask, [((1,), (("close", 33),), 1)] * 2)
    with pytest.raises(RuntimeError, match="mask must be a uint8 CUDA tensor"):
        mc.merge_classes(model, mask.cpu(), mc.PLANES_VIDEO)
    mc.merge_classes(model, mask, mc.PLANES_VIDEO)                  # the engine exists from here on
    buf = torch.full((2048,), 9, dtype=torch.uint8, device="cuda")
    table = torch.full((256 * 5,), 7, dtype=torch.int32, device="cuda")
    lut = (ctypes.c_uint8 * 256)(*([0, 1] + [0] * 254))
    ov = (ctypes.c_int32 * 1)(1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    h = model._handle
    assert lib.unetpp_merge_classes(h, p(buf), 1, 32, 32, lut, 1, ov, None, 0, None, 0, p(buf[16:]), p(table), 256, None) == -1      # aliasing
    assert lib.unetpp_merge_classes(h, p(buf), 1, 32, 32, lut, 7, ov, None, 0, None, 0, p(buf[1024:]), p(table), 256, None) == -2    # 7 planes
    assert lib.unetpp_merge_classes(h, p(buf), 1, 32, 32, lut, 1, ov, None, 0, None, 0, None, None, 256, None) == -1                 # no output
    ov[0] = 0
    assert lib.unetpp_merge_classes(h, p(buf), 1, 32, 32, lut, 1, ov, None, 0, None, 0, p(buf[1024:]), p(table), 256, None) == -1    # out value 0
    colors, has = (ctypes.c_uint8 * 768)(), (ctypes.c_uint8 * 256)()
    assert lib.unetpp_overlay_u8(h, p(buf), p(buf[1536:]), 1, 8, 8, colors, has, 0.5, 0.5, 0, p(buf[100:]), None) == -1             # aliasing
    assert lib.unetpp_overlay_u8(h, p(buf), p(buf[1536:]), 1, 8, 8, colors, has, 0.5, 1.5, 0, p(buf[1024:]), None) == -1            # weight
    torch.cuda.synchronize()
    assert (buf == 9).all() and (table == 7).all()


# ---- 3. threshold_classes and predict_v3 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 6])
def test_threshold_planes_in_place_and_resized(torch_cuda, model, stride):
    """Planes 32 x 48 with pixel_stride 1 (NCHW), 2 and 6 (NHWC), resized to 67 x 101 and at their own size."""
    torch = torch_cuda
    planes = mc.make_prob_planes(2, 32, 48, 90 + stride)                                   # [2,5,32,48], thresholds' neighbours planted
    if stride == 1:
        probs, kw = np.concatenate([planes[:, :1] * 0, planes], 1), dict(channels=(1, 2, 3, 4, 5))
    else:
        order = (1, 0, 5, 3, 2)[:5] if stride == 6 else None
        if stride == 2:
            probs, kw = np.ascontiguousarray(np.stack([planes[:, 0], planes[:, 1]], -1)), dict(channels=(0, 1, 1, 0, 1), layout="nhwc")
        else:
            probs = np.zeros((2, 32, 48, 6), np.float32)
            probs[..., list(order)] = planes.transpose(0, 2, 3, 1)
            kw = dict(channels=order, layout="nhwc")
    pd = dev(torch, probs)
    for hw in (None, (32, 48), (67, 101), (15, 17), (1, 33)):
        want = mc.threshold_classes_np(probs, hw, **kw)
        got = mc.threshold_classes(model, pd, hw, **kw)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (stride, hw)
        assert want.any() and (want < 32).all()
    want = mc.threshold_classes_np(probs, (67, 101), cable_thr=0.3, tape_thr=0.9, defect_thr=0.5, ratio=0.8, **kw)
    assert np.array_equal(mc.threshold_classes(model, pd, (67, 101), cable_thr=0.3, tape_thr=0.9, defect_thr=0.5, ratio=0.8, **kw).cpu().numpy(), want)


def test_threshold_nan_and_exact_thresholds(torch_cuda, model):
    torch = torch_cuda
    t6, t7 = np.float32(0.60), np.float32(0.70)
    below, above = (lambda v: np.nextafter(v, np.float32(0))), (lambda v: np.nextafter(v, np.float32(1)))
    vals = np.array([np.nan, t6, below(t6), above(t6), t7, below(t7), above(t7), 0.0, 1.0, np.inf, t6 * np.float32(1.2), 0.5], np.float32)
    probs = np.zeros((1, 5, 12, 12), np.float32)
    probs[0, 0] = vals[:, None]
    probs[0, 1] = vals[None, :]
    probs[0, 2:] = vals.reshape(3, 4).repeat(4, 0).repeat(3, 1)[None]
    want = mc.threshold_classes_np(probs, channels=(0, 1, 2, 3, 4))
    got = mc.threshold_classes(model, dev(torch, probs), channels=(0, 1, 2, 3, 4)).cpu().numpy()
    assert np.array_equal(got, want) and want[0, 0].max() == 0 and (want[0, 1] & 1).any() and not (want[0, 2] & 1).any()
    with pytest.raises(ValueError, match="channels"):
        mc.threshold_classes(model, dev(torch, probs), channels=(0, 1, 2, 3, 5))
    with pytest.raises(RuntimeError, match="probs must be a float32 CUDA tensor"):
        mc.threshold_classes(model, dev(torch, probs).double())


def test_predict_v3_resized(torch_cuda, model):
    torch = torch_cuda
    planes = mc.make_prob_planes(2, 32, 48, 5)
    for hw in ((67, 101), None):
        want_m, want_t = mc.predict_v3_np(planes, hw, channels=(0, 1, 2, 3, 4), num_classes=7)
        got_m, got_t = mc.predict_v3(model, dev(torch, planes), hw, channels=(0, 1, 2, 3, 4), num_classes=7)
        assert np.array_equal(got_m.cpu().numpy(), want_m) and np.array_equal(got_t.cpu().numpy(), want_t)
        assert set(np.unique(want_m)) >= {0, 1, 2}


# ---- 4. the overlay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 33), (2, 17, 1), (3, 15, 17), (2, 33, 48), (1, 1, 1)], ids=str)
def test_overlay_equals_numpy(torch_cuda, model, shape):
    torch = torch_cuda
    r = np.random.default_rng(3 + sum(shape))
    frames = r.integers(0, 256, shape + (3,), dtype=np.uint8)
    frames.reshape(-1)[:3] = (0, 255, 1)
    mask = r.choice(np.array([0, 0, 1, 2, 3, 4, 5, 6, 9, 77], np.uint8), shape)
    for mode in ("region", "weighted"):
        for alpha in (0.5, 0.6, 0.0, 1.0):
            for off in ((0, 0), (1, 0), (0, 1)) if alpha == 0.6 else ((0, 0),):
                for ncls in (None, 7):
                    want = mc.overlay_np(frames, mask, COLORS, alpha, mode, ncls)
                    got = mc.overlay(model, dev(torch, frames, off[0]), dev(torch, mask, off[1]), COLORS, alpha, mode, ncls)
                    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (mode, alpha, off, ncls)
    for mode in ("region", "weighted"):
        zero = np.zeros(shape, np.uint8)
        got = mc.overlay(model, dev(torch, frames), dev(torch, zero), COLORS, 0.6, mode).cpu().numpy()
        assert np.array_equal(got, mc.overlay_np(frames, zero, COLORS, 0.6, mode))
        if mode == "region":
            assert np.array_equal(got, frames)


def test_overlay_all_byte_pairs(torch_cuda, model):
    """Every (frame byte, colour byte) pair under both modes and both alphas: 65536 pairs per case."""
    torch = torch_cuda
    f, c = np.divmod(np.arange(65536), 256)
    frames = np.repeat(f.astype(np.uint8), 3).reshape(1, 256, 256, 3)
    mask = (c % 255 + 1).astype(np.uint8).reshape(1, 256, 256)
    colors = {v: (v, 255 - v, (v * 7) % 256) for v in range(1, 256)}
    for mode in ("region", "weighted"):
        for alpha in (0.5, 0.6):
            want = mc.overlay_np(frames, mask, colors, alpha, mode)
            assert np.array_equal(mc.overlay(model, dev(torch, frames), dev(torch, mask), colors, alpha, mode).cpu().numpy(), want)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes(torch_cuda, model):
    torch = torch_cuda
    r = np.random.default_rng(11)
    frames = dev(torch, r.integers(0, 256, (3, 70, 150, 3), dtype=np.uint8))
    mask = dev(torch, class_noise((3, 70, 150), r))
    probs = dev(torch, mc.make_prob_planes(3, 32, 48, 8))
    runs = []
    for _ in range(2):
        outs = list(mc.quality_gate(model, frames))
        outs += list(mc.clean_classes_video(model, mask)) + [mc.class_table(model, mask)]
        outs += list(mc.predict_v3(model, probs, (70, 150), channels=(0, 1, 2, 3, 4)))
        outs += [mc.overlay(model, frames, mask, COLORS, 0.6, m) for m in ("region", "weighted")]
        runs.append(b"".join(x.cpu().numpy().tobytes() for x in outs))
    assert runs[0] == runs[1]


# ---- 6. the reference's stored results --------------------------------------------------------------------------------------------
def pair(g, which):
    return g["colors_" + which][:, :3], g["colors_" + which][:, 3]


def test_fixture_gate_sequences(torch_cuda, model, golden):
    torch = torch_cuda
    for name, kind, h, w, seed, digest in golden["gate"]:
        frames = mc.make_gate_sequence(int(h), int(w), int(seed), str(kind))
        assert mc.sha(frames) == digest
        is_bad, reason, lap_var, gray_std, mad, gray = host(*mc.quality_gate(model, dev(torch, frames)))
        assert np.array_equal(is_bad, golden[name + "_is_bad"]) and np.array_equal(reason, golden[name + "_reason"])
        assert np.array_equal(mad, golden[name + "_mad"])           # an exact integer below 2^53 divided once, here and there
        # the device value is the correctly rounded closed form of exact integer sums; NumPy's two-pass float64 std / var with
        # pairwise summation differs from it by a few ulps: 2.2e-16 x a summation depth of at most about 21 x a small constant
        assert np.allclose(gray_std, golden[name + "_gray_std"], rtol=1e-12, atol=0)
        assert np.allclose(lap_var, golden[name + "_lap_var"], rtol=1e-12, atol=0)
        assert mc.sha(gray[-1]) == str(golden[name + "_gray_sha"])
        off = host(*mc.quality_gate(model, dev(torch, frames), enable=False))
        assert not off[0].any() and not off[1].any() and not off[2].any() and not off[4].any()
        assert np.allclose(off[3], golden[name + "_disabled_std"], rtol=1e-12, atol=0)
        if str(kind) == "moving":
            alone = host(*mc.quality_gate(model, dev(torch, frames[1:])))
            assert bool(alone[0][0]) == bool(golden[name + "_alone_bad"]) and is_bad[1] and not alone[0][0]


def test_fixture_class_scenes_and_overlays(torch_cuda, model, golden):
    torch = torch_cuda
    for name, h, w, seed, pred_sha, frame_sha in golden["video"]:
        pred, frame = mc.make_class_scene(int(h), int(w), int(seed))
        assert mc.sha(pred) == pred_sha and mc.sha(frame) == frame_sha
        want = golden[name + "_video"]
        got_m, got_t = mc.clean_classes_video(model, dev(torch, pred[None]), num_classes=7)
        assert np.array_equal(got_m[0].cpu().numpy(), want)
        assert np.array_equal(got_t.cpu().numpy(), mc.class_table_np(want[None], 7))
        fd = dev(torch, frame[None])
        for alpha, tag in ((0.5, "a50"), (0.6, "a60")):
            ov = mc.overlay(model, fd, got_m, pair(golden, "video"), alpha, "region", 7)
            assert mc.sha(ov[0].cpu().numpy()) == str(golden[f"{name}_region_{tag}"])
            ov = mc.overlay(model, fd, got_m, pair(golden, "opt"), alpha, "weighted")
            assert mc.sha(ov[0].cpu().numpy()) == str(golden[f"{name}_weighted_{tag}"])
        ov = mc.overlay(model, fd, got_m, pair(golden, "video"), 0.6, "region", 6)          # class 6 blends with black
        assert mc.sha(ov[0].cpu().numpy()) == str(golden[name + "_region6_a60"])
        kw = dict(zip(("min_cable_area", "cable_coverage_threshold", "min_defect_area", "edge_margin"), golden["validate"].tolist()))
        valid, defects = mc.validate_detection(got_t[0], (int(h), int(w)), **kw)
        assert valid == bool(golden[name + "_valid"])
        assert [[d["class_id"], *d["bbox"], d["area"]] for d in defects] == golden[name + "_defects"].tolist()
    for name, side, seed, _ in golden["v3"]:
        planes = golden[name + "_planes"]                          # the five planes the reference's predict handed to cv2.resize
        want = golden[name + "_v3"]
        got = mc.predict_v3(model, dev(torch, planes[None]), None, channels=(0, 1, 2, 3, 4), want_table=False)
        assert np.array_equal(got[0].cpu().numpy(), want)
        frame = np.random.default_rng(int(seed)).integers(0, 256, want.shape + (3,), dtype=np.uint8)
        with_three = want.copy()
        with_three[:4, :4] = 3                                     # a value the v3 colours do not know
        ov = mc.overlay(model, dev(torch, frame[None]), dev(torch, with_three[None]), pair(golden, "v3"), 0.5, "region", 6)
        assert mc.sha(ov[0].cpu().numpy()) == str(golden[name + "_region_a50"])


# ---- 7. the loop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["video", "v3"])
def test_loop_runs_end_to_end_with_two_read_backs(torch_cuda, variant, syn, monkeypatch):
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(7, deep_supervision=False, max_batch=4, max_hw=(48, 80)).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(7, 3, False, 5))
    frames = np.stack([syn.make_frame_u8(60, 100, 3, "smooth", s) for s in (1, 2, 3)])
    frames[1] = 127                                                 # a glitch frame: gated
    fd = dev(torch, frames)
    calls = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (calls.append(tuple(t.shape)), real_cpu(t, *a, **k))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("sync"))
    monkeypatch.setattr(torch.Tensor, "item", lambda t: calls.append("item"))
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: calls.append("tolist"))
    records, overlays, last_gray = frame_loop.process_frames_multiclass(m, fd, None, input_size=(48, 80), variant=variant, colors=COLORS,
                                                                         alpha=0.6, min_area_px=5)
    monkeypatch.undo()
    assert len(calls) == 2 and "sync" not in calls, calls            # the gate's flags, then the tables
    assert records[1] is None and records[0] is not None and records[2] is not None
    assert overlays.dtype == torch.uint8 and tuple(overlays.shape) == (3, 60, 100, 3) and tuple(last_gray.shape) == (60, 100)
    gate = mc.quality_gate_np(frames, None)
    assert gate[1].tolist() == [4, 1, 4] and np.array_equal(last_gray.cpu().numpy(), gate[5][2])
    assert np.array_equal(overlays[1].cpu().numpy(), frames[1])      # a gated frame comes back as it went in
    good = dev(torch, frames[[0, 2]])
    small = m.resize_frames(good, (48, 80))
    if variant == "video":
        mask = mc.clean_classes_video_np(m.resize_masks(m.segment(small), (100, 60)).cpu().numpy(), want_table=False)
    else:
        mask = mc.predict_v3_np(m.predict_proba(small).cpu().numpy(), (60, 100), want_table=False)
    table = mc.class_table_np(mask, 7)
    for k, i in enumerate((0, 2)):
        assert np.array_equal(records[i]["table"], table[k]) and records[i]["reason"] == "ok"
        assert records[i]["events"] == mc.defect_events(table[k], min_area_px=5)
        assert np.array_equal(overlays[i].cpu().numpy(), mc.overlay_np(frames[i:i + 1], mask[k:k + 1], COLORS, 0.6, "region", 7)[0])
        assert records[i]["gray_std"] == gate[3][i] and records[i]["lap_var"] == gate[2][i] and records[i]["mad"] == gate[4][i]
