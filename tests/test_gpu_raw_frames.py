"""Raw camera frames on the device (include/unetpp_raw.h, unet_amd/raw_frames.py) against the NumPy forms, with == throughout
(everything is integer): the demosaic with its three output forms, the demosaic fused into the resize against both the NumPy form
and the unfused composition on the device, the whole raw loop against process_frames, and the refusals.

Shapes.  rf_to_bgr_kernel's tile is 128 x 16 pixels: 3x3 is the smallest frame, 5x7 odd in both axes, 18x34 two row tiles, 33x65
a last tile that also takes the extra row (33 - 1 is a multiple of 16), 70x130 more than one tile in both directions with a
ragged last one, and 17x129 the frame whose last column AND row are the extra ones of a tile (tile + 1 in both axes).
rf_resize_kernel stages a tile's source rectangle in LDS while it fits 16 KiB and reads its taps in place beyond that: the four
shapes of the issue all stage it, 150x900 -> 3x2 does not.
Run on the GPU box:  python -m pytest tests/test_gpu_raw_frames.py -m gpu"""
import numpy as np
import pytest

from unet_amd import raw_frames as rf

pytestmark = pytest.mark.gpu
BAYER = ("BG", "GB", "RG", "GR")
SHAPES = [(3, 3), (5, 7), (18, 34), (33, 65), (70, 130), (17, 129)]
# (h, w) -> (oh, ow), an ROI (x0, y0, cw, ch) with an odd origin
RESIZES = [((37, 53), (16, 24), (5, 3, 40, 31)), ((9, 11), (32, 16), (1, 3, 9, 5)), ((64, 48), (64, 48), (7, 9, 33, 40)),
           ((35, 70), (16, 16), (3, 1, 60, 33)), ((150, 900), (3, 2), (11, 5, 880, 140))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: these functions need none


@pytest.fixture(scope="module")
def net(torch_cuda, syn):
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=False, max_batch=2, max_hw=(32, 32)).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    return m.eval()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what):
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pattern", BAYER + ("MONO",))
def test_to_bgr_equals_the_numpy_form(torch_cuda, model, pattern, shape):
    """Every pattern at every shape, B = 1 and 3, the three output forms, and rows 5 bytes longer than the frame is wide."""
    h, w = shape
    for b in (1, 3):
        raw = rf.make_raw(b, h, w, 100 * h + w + b)
        want_bgr, want_gray = rf.demosaic_np(raw, pattern), rf.gray_np(raw, pattern)
        t = dev(torch_cuda, raw)
        same(rf.to_bgr(model, t, pattern=pattern), want_bgr, "bgr only")
        same(rf.to_gray(model, t, pattern=pattern), want_gray, "grey only")
        both = rf.to_bgr(model, t, pattern=pattern, want_gray=True)
        same(both[0], want_bgr, "bgr of both")
        same(both[1], want_gray, "grey of both")
        same(rf.to_bgr(model, t, pattern=pattern, want_gray=True, bgr=False), want_gray, "bgr=False")
        padded = torch_cuda.full((b, h, w + 5), 255, dtype=torch_cuda.uint8, device="cuda")
        padded[:, :, :w] = t
        view = padded[:, :, :w]
        assert not view.is_contiguous() or h == 1
        got = rf.to_bgr(model, view, pattern=pattern, want_gray=True)
        same(got[0], want_bgr, "row stride w + 5: bgr")
        same(got[1], want_gray, "row stride w + 5: grey")


def test_to_bgr_reads_the_pixel_format_as_the_reference_does(torch_cuda, model):
    raw = rf.make_raw(2, 12, 10, 5)
    t = dev(torch_cuda, raw)
    for name in rf.FIXTURE_FORMATS:
        want = np.stack([rf.to_bgr_np(f.reshape(-1), name, 10, 12) for f in raw])
        same(rf.to_bgr(model, t, name), want, name)
        same(rf.to_gray(model, t, name), rf.gray_np(raw, rf.pattern_of(name)), name + " grey")


@pytest.mark.parametrize("case", RESIZES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
@pytest.mark.parametrize("pattern", BAYER + ("MONO",))
def test_resize_equals_the_numpy_form_and_the_unfused_composition(torch_cuda, model, pattern, case):
    (h, w), size, roi = case
    raw = rf.make_raw(2, h, w, 7 * h + w)
    t = dev(torch_cuda, raw)
    bgr = rf.to_bgr(model, t, pattern=pattern)
    for r in (None, roi):
        got = rf.resize(model, t, pattern, size, r)
        same(got, rf.raw_resize_np(raw, pattern, r, size), f"roi {r}: NumPy form")
        x0, y0, cw, ch = r or (0, 0, w, h)
        unfused = model.resize_frames(bgr[:, y0:y0 + ch, x0:x0 + cw].contiguous(), size)
        assert torch_cuda.equal(got, unfused), f"roi {r}: the fused launch differs from resize_frames(to_bgr(raw)[roi])"
    if pattern != "MONO":                                                 # an odd origin must not shift the pattern
        x0, y0, cw, ch = roi
        shifted = rf.raw_resize_np(np.ascontiguousarray(raw[:, y0:y0 + ch, x0:x0 + cw]), pattern, None, size)
        assert (rf.resize(model, t, pattern, size, roi).cpu().numpy() != shifted).any()


def test_resize_reads_padded_rows_in_place(torch_cuda, model):
    raw = rf.make_raw(2, 37, 53, 3)
    padded = torch_cuda.full((2, 37, 58), 255, dtype=torch_cuda.uint8, device="cuda")
    padded[:, :, :53] = dev(torch_cuda, raw)
    same(rf.resize(model, padded[:, :, :53], "RG", (16, 24), (5, 3, 40, 31)), rf.raw_resize_np(raw, "RG", (5, 3, 40, 31), (16, 24)), "row stride w + 5")


def test_process_raw_frames_equals_process_frames_on_the_demosaiced_frame(torch_cuda, net):
    from unet_amd import frame_loop
    raw = rf.make_raw(2, 45, 70, 11)
    t = dev(torch_cuda, raw)
    for name in ("BayerRG8", "BayerBG8", "Mono8"):
        bgr, gray = rf.to_bgr(net, t, name, want_gray=True)
        for roi in ("fixed", None, (10, 5, 50, 40)):
            want = frame_loop.process_frames(net, bgr, target_size=(32, 32), roi=roi)
            got = frame_loop.process_raw_frames(net, t, name, target_size=(32, 32), roi=roi, want_gray=True)
            assert len(got) == 4
            for g, w_, what in zip(got, want + (gray,), ("pred", "cable", "tape", "grey")):
                assert torch_cuda.equal(g, w_), (name, roi, what)
        assert len(frame_loop.process_raw_frames(net, raw, name, target_size=(32, 32))) == 3      # a host array is uploaded


def test_bad_arguments_are_refused(torch_cuda, model):
    torch = torch_cuda
    t = dev(torch, rf.make_raw(1, 8, 8, 0))
    with pytest.raises(RuntimeError, match=r"raw must be a uint8 CUDA tensor \[B,H,W\]"):
        rf.to_bgr(model, t.cpu(), "BayerRG8")
    with pytest.raises(RuntimeError, match=r"raw must be a uint8 CUDA tensor \[B,H,W\]"):
        rf.resize(model, t.float(), "RG", (4, 4))
    with pytest.raises(RuntimeError, match=r"raw must be a uint8 CUDA tensor \[B,H,W\]"):
        rf.to_gray(model, t[0], "Mono8")
    with pytest.raises(ValueError, match="pattern must be one of"):
        rf.to_bgr(model, t, pattern="RGGB")
    with pytest.raises(ValueError, match="not both"):
        rf.to_bgr(model, t, "BayerRG8", pattern="RG")
    with pytest.raises(ValueError, match="not both"):
        rf.to_bgr(model, t)
    with pytest.raises(ValueError, match="nothing to compute"):
        rf.to_bgr(model, t, "BayerRG8", bgr=False)
    with pytest.raises(ValueError, match="needs H, W >= 3"):
        rf.to_bgr(model, t[:, :2], pattern="BG")
    with pytest.raises(ValueError, match="needs H, W >= 3"):
        rf.resize(model, t[:, :, :2], "GR", (4, 4))
    with pytest.raises(ValueError, match="does not lie inside"):
        rf.resize(model, t, "RG", (4, 4), (4, 0, 5, 8))
    with pytest.raises(ValueError, match="size_hw must be positive"):
        rf.resize(model, t, "RG", (0, 4))
    assert rf.to_bgr(model, t[:, :2, :1], "Mono8").shape == (1, 2, 1, 3)      # mono has no border rule and no smallest frame


def test_the_library_refuses_what_the_wrappers_cannot_send(torch_cuda, model):
    """UNETPP_E_UNSUPPORTED (-2) for every bad argument but the NULL engine: strides, pattern, both outputs NULL, overlap."""
    import ctypes
    from unet_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    t = dev(torch, rf.make_raw(1, 8, 8, 0))
    model._input(t, "raw")
    buf = torch.empty(8 * 8 * 4, dtype=torch.uint8, device="cuda")
    p, o = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(buf.data_ptr())
    e = model._handle
    assert lib.unetpp_raw_to_bgr_u8(e, p, 8, 64, 1, 8, 8, 0, o, None, None) == 0
    for args in ((e, p, 7, 64, 1, 8, 8, 0, o, None, None), (e, p, 8, 63, 2, 8, 8, 0, o, None, None), (e, p, 8, 64, 1, 8, 8, 5, o, None, None),
                 (e, p, 8, 64, 1, 8, 8, -1, o, None, None), (e, p, 8, 64, 1, 8, 8, 0, None, None, None), (e, None, 8, 64, 1, 8, 8, 0, o, None, None),
                 (e, p, 8, 64, 1, 2, 8, 0, o, None, None), (e, p, 8, 64, 1, 8, 8, 0, p, None, None), (e, p, 8, 64, 1, 8, 8, 0, o, o, None)):
        assert lib.unetpp_raw_to_bgr_u8(*args) == -2, args[2:8]
    assert lib.unetpp_raw_resize_u8(e, p, 8, 64, 1, 8, 8, 2, 1, 1, 7, 7, o, 4, 4, None) == 0
    for args in ((e, p, 8, 64, 1, 8, 8, 2, 1, 1, 8, 7, o, 4, 4, None), (e, p, 8, 64, 1, 8, 8, 2, -1, 0, 4, 4, o, 4, 4, None),
                 (e, p, 8, 64, 1, 8, 8, 2, 0, 0, 0, 4, o, 4, 4, None), (e, p, 8, 64, 1, 8, 8, 2, 0, 0, 8, 8, o, 0, 4, None),
                 (e, p, 8, 64, 1, 8, 8, 2, 0, 0, 8, 8, p, 4, 4, None), (e, p, 8, 64, 1, 8, 8, 9, 0, 0, 8, 8, o, 4, 4, None),
                 (e, p, 8, 64, 1, 8, 8, 2, 0, 0, 8, 8, None, 4, 4, None)):
        assert lib.unetpp_raw_resize_u8(*args) == -2, args[2:12]
    torch.cuda.synchronize()
