"""The tail of the refactored loop on the device (include/unetpp_contours.h, unet_amd/contours.py) against the NumPy forms,
with == throughout: the border, the labels and areas of the external contours, the circle, the diameter, the paste, the
chained overlay, and process_frames_refactored_full against the same steps composed from the NumPy forms on the device's
own `pred`.
Run on the GPU box:  python -m pytest tests/test_gpu_contours.py -m gpu"""
import numpy as np
import pytest

from conftest import load_golden
from unet_amd import components as cc
from unet_amd import contours as ct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: the contour functions need none


@pytest.fixture(scope="module")
def golden():
    g = load_golden("contours_scenes")
    return {k: g[k] for k in g.files}


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def embedded(torch, a, offset):
    """A CUDA view of `a` at byte `offset` of a larger buffer whose other bytes are 255."""
    buf = torch.full((a.nbytes + offset + 64,), 255, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + a.nbytes].view(getattr(torch, str(a.dtype))).view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == (buf.data_ptr() + offset) % 16
    return view


def random_masks(b, h, w, seed, classes=False):
    """Blobs, rings with blobs in their holes and speckle: several contours of different areas per frame."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((b, h, w), np.uint8)
    for i in range(b):
        m = r.random((h, w)) < 0.04
        for _ in range(int(r.integers(2, 6))):
            cy, cx, rad = r.integers(0, h), r.integers(0, w), r.integers(2, max(3, min(h, w) // 3))
            d2 = (y - cy) ** 2 + (x - cx) ** 2
            m |= (d2 <= rad * rad) & ~((d2 <= (rad - 2) ** 2) & (d2 > (rad // 3) ** 2) & (r.random() < 0.6))
        m &= r.random((h, w)) > 0.03
        out[i] = m * (r.integers(1, 3, (h, w)) if classes else 255)
    return out


def check_all(torch, model, masks, match_class=-1, mask_dev=None, k=8192):
    """Every contour function on one batch against the NumPy forms."""
    d = dev(torch, masks) if mask_dev is None else mask_dev
    border = ct.outer_border(model, d, match_class, k)
    labels, num, area2 = ct.external_contour_areas(model, d, match_class, k)
    table = ct.enclosing_circle(model, d, match_class, k)
    diam = ct.measure_diameter(model, d, match_class, k)
    assert border.dtype == torch.uint8 and labels.dtype == torch.int32 and area2.dtype == torch.int64 and table.dtype == torch.int32
    assert tuple(area2.shape) == (len(masks), k) and tuple(table.shape) == (len(masks), 8) and diam.dtype == np.float64
    border, labels, num, area2, table = (t.cpu().numpy() for t in (border, labels, num, area2, table))
    circles = ct.circle_from_support(table)
    chosen_all = []
    for i, m in enumerate(masks):
        assert (border[i] == ct.outer_border_np(m, match_class)).all(), f"frame {i}: border"
        want_l, want_n, want_a = ct.external_contour_areas_np(m, match_class)
        assert (labels[i] == want_l).all() and num[i] == want_n, f"frame {i}: labels"
        assert (area2[i, :want_n] == want_a).all() and not area2[i, want_n:].any(), f"frame {i}: areas"
        chosen, circle = ct.support_table_np(m, match_class)
        assert table[i, 7] == chosen and circles[i] == circle, (i, table[i], circle)
        fg = cc.foreground(m, match_class)
        for p in range(table[i, 0]):                                   # the support points are pixels of the chosen contour
            x, y = table[i, 1 + 2 * p], table[i, 2 + 2 * p]
            assert fg[y, x] and want_l[y, x] == chosen
        assert (table[i, 0] == 0) == (want_n < 2) and not table[i, 1 + 2 * table[i, 0]:7].any()
        assert diam[i] == 2.0 * circle[1]
        if match_class < 0:
            assert diam[i] == ct.measure_diameter_np(m), (i, diam[i], ct.measure_diameter_np(m))
        chosen_all.append(chosen)
    return chosen_all


def test_golden_scenes(torch_cuda, model, golden):
    for n in (str(v) for v in golden["names"]):
        m = golden[n + "/mask"]
        check_all(torch_cuda, model, m[None])
        got = ct.measure_diameter(model, dev(torch_cuda, m[None]))[0]
        want = float(golden[n + "/diameter"])
        assert abs(got - want) <= 1e-12 * abs(want), (n, got, want)
        _, _, area2 = ct.external_contour_areas(model, dev(torch_cuda, m[None]))
        areas = golden[n + "/areas"]
        assert (area2[0, 1:1 + areas.size].cpu().numpy() == 2 * areas).all(), n


@pytest.mark.parametrize("shape", [(1, 32, 48), (3, 32, 48), (1, 64, 96), (3, 64, 96), (2, 37, 131)], ids=lambda s: "x".join(map(str, s)))
def test_random_masks(torch_cuda, model, shape):
    b, h, w = shape
    chosen = check_all(torch_cuda, model, random_masks(b, h, w, h + b))
    if b == 3:
        assert len(set(chosen)) > 1, "the frames of this batch should choose different labels"
    check_all(torch_cuda, model, random_masks(b, h, w, h + b + 1, classes=True), match_class=2)
    check_all(torch_cuda, model, random_masks(b, h, w, h + b + 1, classes=True), match_class=-1)


def test_empty_beside_full_and_several_tiles(torch_cuda, model):
    m = np.zeros((3, 70, 300), np.uint8)                              # wider and higher than one labelling tile
    m[1] = 255
    m[2, 3:66, 5:290] = 7
    m[2, 10:60, 20:280] = 0
    m[2, 30:34, 100:200] = 7
    assert check_all(torch_cuda, model, m) == [0, 1, 1]
    assert ct.measure_diameter(model, dev(torch_cuda, m)).tolist() == [0.0, float(np.sqrt(299.0 ** 2 + 69.0 ** 2)), float(np.sqrt(284.0 ** 2 + 62.0 ** 2))]


def test_byte_paths(torch_cuda, model):
    torch = torch_cuda
    m = random_masks(2, 33, 45, 3)                                    # a width that is no multiple of 16
    check_all(torch, model, m, mask_dev=embedded(torch, m, 1))       # and a view one byte off
    check_all(torch, model, m, mask_dev=embedded(torch, m, 0))
    r = np.random.default_rng(4)
    for (b, h, w), off in (((2, 33, 45), 1), ((2, 33, 45), 0), ((1, 32, 48), 0), ((3, 17, 21), 5)):
        frames = r.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
        masks = [(r.random((b, h, w)) < 0.5).astype(np.uint8) * 255 for _ in range(3)]
        want = np.stack([ct.create_overlay_masks_np(frames[i], masks[0][i], masks[1][i], masks[2][i]) for i in range(b)])
        got = ct.create_overlay_masks(model, embedded(torch, frames, off), *[embedded(torch, x, off) for x in masks])
        assert got.dtype == torch.uint8 and (got.cpu().numpy() == want).all(), ((b, h, w), off)
        got = ct.create_overlay_masks(model, embedded(torch, frames, off), dev(torch, masks[0]), dev(torch, masks[1]), dev(torch, np.zeros_like(masks[2])))
        want = np.stack([ct.create_overlay_masks_np(frames[i], masks[0][i], masks[1][i], np.zeros_like(masks[2][i])) for i in range(b)])
        assert (got.cpu().numpy() == want).all()
        roi_mask = masks[0][:, :h - 3, :w - 5]
        for roi, fhw in (((4, 2, w - 5, h - 3), (h + 9, w + 11)), ((w - 8, h - 6, w - 5, h - 3), (h + 1, w + 3)), ((-3, -2, w, h), (h, w - 1))):
            got = ct.paste_roi_masks(model, embedded(torch, roi_mask, off), roi, fhw)
            assert (got.cpu().numpy() == ct.paste_roi_masks_np(roi_mask, roi, fhw)).all(), (roi, fhw)


def test_paste_and_overlay_golden(torch_cuda, model, golden):
    torch = torch_cuda
    for tag in ("paste_inside", "paste_overhang"):
        got = ct.paste_roi_masks(model, dev(torch, golden[tag + "/roi_mask"][None]), golden[tag + "/roi"].tolist(), golden[tag + "/frame_hw"].tolist())
        assert (got[0].cpu().numpy() == golden[tag + "/full"]).all(), tag
    got = ct.create_overlay_masks(model, *[dev(torch, golden["overlay/" + k][None]) for k in ("frame", "cable", "tape", "burr")])
    assert (got[0].cpu().numpy() == golden["overlay/out"]).all()


def test_refusals(torch_cuda, model):
    torch = torch_cuda
    m = dev(torch, random_masks(2, 32, 48, 9))
    speckle = np.zeros((1, 32, 48), np.uint8)
    speckle[0, ::2, ::2] = 1                                           # 384 contours
    for fn in (ct.external_contour_areas, ct.enclosing_circle, ct.measure_diameter):
        with pytest.raises(ValueError, match="more than max_components = 100"):
            fn(model, dev(torch, speckle), -1, 100)
    labels, num, _ = ct.external_contour_areas(model, dev(torch, speckle), -1, 100, check=False)
    assert num.tolist() == [385] and (labels[0].cpu().numpy() == ct.external_contour_areas_np(speckle[0])[0]).all()
    with pytest.raises(ValueError):
        ct.external_contour_areas(model, m, -1, 1)
    with pytest.raises(ValueError):
        ct.measure_diameter(model, torch.zeros((1, 4096, 8), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ct.paste_roi_masks(model, m, (60, 60, 48, 32), (40, 50))      # the ROI misses the frame
    with pytest.raises(RuntimeError):
        ct.create_overlay_masks(model, torch.zeros((2, 32, 48, 3), dtype=torch.uint8, device="cuda"), m, m, m[:1])
    with pytest.raises(RuntimeError):
        ct.outer_border(model, m.cpu())


@pytest.fixture(scope="module")
def net(torch_cuda, syn):
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=False, max_batch=2, max_hw=(64, 64)).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    return m.eval()


def test_process_frames_refactored_full_equals_the_numpy_chain(torch_cuda, net, syn):
    torch = torch_cuda
    from unet_amd import edges as ed
    from unet_amd import frame_loop
    from unet_amd import morphology as mo
    from unet_amd import robust as rb
    frames = syn.make_frames_u8(2, 96, 128, "smooth", 77)
    roi = (40, 20, 64, 64)
    cfg = dict(min_area=4, min_aspect=0.1, max_center_offset=0.9, ring_dilate=5, ring_erode=1, band_out=3, laplacian_threshold=2, burr_min_area=1,
               burr_max_area=400)
    metrics, overlays, (cable, tape, burr) = frame_loop.process_frames_refactored_full(net, frames, roi, input_size=64, **cfg)
    pred, _, _ = frame_loop.process_frames_refactored(net, frames, roi, input_size=64)
    pred = pred.cpu().numpy()
    assert overlays.is_cuda and cable.is_cuda and tuple(overlays.shape) == (2, 96, 128, 3) and tuple(cable.shape) == (2, 96, 128)
    some = 0
    for i in range(2):
        pred_roi = rb.resize_nearest_np(pred[i], (64, 64))
        c_roi = cc.filter_components_np(pred_roi, 1, "cable_shape", out_value=255, roi_width=64, min_area=4, min_aspect=0.1, max_center_offset=0.9)
        t_roi = mo.constrain_tape_to_ring_np(pred_roi, c_roi, 2, -1, 5, 1, 255)
        c_full, t_full = ct.paste_roi_masks_np(c_roi, roi, (96, 128)), ct.paste_roi_masks_np(t_roi, roi, (96, 128))
        assert (cable[i].cpu().numpy() == c_full).all() and (tape[i].cpu().numpy() == t_full).all()
        b_full = ed.burr_mask_rulebased_np(ed.bgr_to_gray_np(frames[i]), c_full, band_out=3, laplacian_threshold=2, min_area=1, max_area=400)
        assert (burr[i].cpu().numpy() == b_full).all()
        dc, dt = ct.measure_diameter_np(c_full), ct.measure_diameter_np(t_full)
        want = {"dc_px": dc, "dt_px": dt, "delta_d_px": dt - dc, "ratio": dt / dc if dc > 0 else None, "has_burr": bool(b_full.max() > 0),
                "cable_coverage": np.sum(c_full > 0) / (128 * 96), "tape_coverage": np.sum(t_full > 0) / (128 * 96)}
        assert metrics[i] == want, (metrics[i], want)
        assert (overlays[i].cpu().numpy() == ct.create_overlay_masks_np(frames[i], c_full, t_full, b_full)).all()
        some += int(c_full.any()) + int(t_full.any())
    assert some, "the synthetic network should leave at least one mask non-empty"
    with pytest.raises(ValueError):
        frame_loop.process_frames_refactored_full(net, frames, (200, 200, 64, 64), input_size=64)
