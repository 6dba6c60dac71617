"""Non-local-means denoising on the device (unetpp_nlmeans_u8 and the functions of unet_amd/nlmeans.py built on it) against
the NumPy restatement and the fixtures made from the reference's own functions (tests/golden/nlmeans_scenes.npz).  The
arithmetic is integer on both sides: exact equality everywhere, no tolerance, nothing left out.
Run on the GPU box:  python -m pytest tests/test_gpu_nlmeans.py -m gpu"""
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import edges as ed
from unet_amd import enhance as en
from unet_amd import nlmeans as nm

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
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: none of this needs any


@pytest.fixture(scope="module")
def tile():
    """(rows, columns) of output one workgroup owns, from the library."""
    rows, cols = nm.layout()
    assert rows >= 8 and cols >= 8
    return rows, cols


def dev(torch, *frames):
    return torch.from_numpy(np.stack(frames)).cuda()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def quiet(H, W, seed, sigma=1.5):
    """A smooth image with a step and a little noise: one the filter changes at every strength."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(np.rint(70 + 130.0 * x / W + 40.0 * y / H + 40 * (x > W // 2) + r.normal(0, sigma, (H, W))), 0, 255).astype(np.uint8)


# ---- 1. the smallest shapes at which the kernel can go wrong ---------------------------------------------------------------
@pytest.mark.parametrize("shape", [(14, 14), (14, 40), (40, 14)])
def test_minimum_and_thin_shapes(torch_cuda, model, shape):
    img = quiet(*shape, 1)
    want = nm.nl_means_np(img, 10)
    assert not np.array_equal(want, img)
    got = nm.nl_means(model, dev(torch_cuda, img), 10)
    assert got.dtype == torch_cuda.uint8 and tuple(got.shape) == (1,) + shape
    assert np.array_equal(got.cpu().numpy()[0], want)


def test_two_seams_cross_off_grid(torch_cuda, model, tile):
    rows, cols = tile
    H, W = 2 * rows + 3, 2 * cols + 5
    img = quiet(H, W, 2)
    want = nm.nl_means_np(img, 10)
    got = nm.nl_means(model, dev(torch_cuda, img), 10).cpu().numpy()[0]
    for y in (rows - 1, rows, 2 * rows - 1, 2 * rows, H - 1):
        assert np.array_equal(got[y], want[y]), f"row {y}"
    for x in (cols - 1, cols, 2 * cols - 1, 2 * cols, W - 1):
        assert np.array_equal(got[:, x], want[:, x]), f"column {x}"
    assert np.array_equal(got, want)
    # the seam must matter: the filter reads across it
    assert not np.array_equal(want[rows - 4:rows + 4], np.concatenate([nm.nl_means_np(img[:rows], 10)[-4:], nm.nl_means_np(img[rows:], 10)[:4]]))


@pytest.mark.parametrize("h", [3, 5, 10, 30])
def test_strengths(torch_cuda, model, h):
    img = quiet(37, 45, 3, sigma=1.0)
    want = nm.nl_means_np(img, h)
    assert not np.array_equal(want, img)
    assert np.array_equal(nm.nl_means(model, dev(torch_cuda, img), h).cpu().numpy()[0], want)


def test_checkerboard_constant_255_and_word_stores(torch_cuda, model):
    torch = torch_cuda
    y, x = np.mgrid[0:24, 0:28]
    board = (((x + y) % 2) * 255).astype(np.uint8)                           # reaches the largest D: the zero tail of the table
    board[5:9, 7:13] = 255
    white = np.full((24, 28), 255, np.uint8)                                 # est + wsum / 2 passes INT32_MAX
    black = np.zeros((24, 28), np.uint8)
    got = nm.nl_means(model, dev(torch, board, white, black), 30).cpu().numpy()     # width % 4 == 0: the word stores
    assert np.array_equal(got[0], nm.nl_means_np(board, 30))
    assert np.array_equal(got[1], white) and np.array_equal(got[2], black)
    assert int(((board[12:19, 14:21].astype(np.int64) - board[12:19, 15:22]) ** 2).sum()) >> 6 == 49784     # the table's last index
    odd = quiet(21, 30, 4)                                                   # width % 4 != 0: the byte stores
    assert np.array_equal(nm.nl_means(model, dev(torch, odd), 10).cpu().numpy()[0], nm.nl_means_np(odd, 10))


def test_injected_tables(torch_cuda, model):
    torch = torch_cuda
    # An image that reaches the LAST entry of an 8,192-entry prefix: zeros on the left; on the right a pattern of period 7
    # in both directions, so that every 7 x 7 patch there holds the same 49 values, 47 x 103, 120 and 106, and its
    # distance from a patch of zeros is 47 * 103^2 + 120^2 + 106^2 = 524,259 = 64 * 8191 + 35.
    cell = np.full(49, 103, np.uint8)
    cell[[10, 30]] = (120, 106)
    yy, xx = np.mgrid[0:30, 0:44]
    img = np.where(xx >= 22, cell.reshape(7, 7)[yy % 7, xx % 7], 0).astype(np.uint8)
    assert int((img[10:17, 30:37].astype(np.int64) ** 2).sum()) >> 6 == 8191
    x = dev(torch, img)
    full = np.ones(8192, np.int64)
    full[8191] = 19096                                                       # a prefix of exactly 8,192 entries, the last one decisive
    assert nm.prefix_length(full) == 8192
    want = nm.nl_means_np(img, weights=full)
    assert not np.array_equal(want, nm.nl_means_np(img, weights=full[:8191]))      # the last entry is used
    assert np.array_equal(nm.nl_means(model, x, weights=full).cpu().numpy()[0], want)
    img = quiet(30, 33, 5, sigma=3.0)
    x = dev(torch, img)
    one = np.array([123])                                                    # a prefix of one entry
    assert np.array_equal(nm.nl_means(model, x, weights=one).cpu().numpy()[0], nm.nl_means_np(img, weights=one))
    assert np.array_equal(nm.nl_means(model, x, weights=nm.nlm_weights(10)).cpu().numpy()[0], nm.nl_means_np(img, 10))
    with pytest.raises(ValueError, match="8192"):
        nm.nl_means(model, x, 40)
    with pytest.raises(ValueError, match="supports only 7 and 21"):
        nm.nl_means(model, x, 5, 5, 21)
    with pytest.raises(ValueError):
        nm.nl_means(model, dev(torch, img[:13]), 5)


# ---- 2. the decisions on the device ----------------------------------------------------------------------------------------
def test_mixed_batch_with_decisions(torch_cuda, model):
    torch = torch_cuda
    H, W = 41, 52
    frames = [nm.make_nlm_scene(H, W, 20), nm.make_nlm_scene(H, W, 21, "colour"), nm.make_nlm_scene(H, W, 22)]
    x = dev(torch, *frames)
    got, dec = nm.preprocess_frames_nlm(model, x, return_decisions=True, denoise_strength=10)
    assert dec.dtype == torch.bool and dec.cpu().tolist() == [True, False, True]
    got = got.cpu().numpy()
    assert got.shape == (3, H, W, 3) and np.array_equal(got[1], frames[1])   # the colour frame comes back byte-identical
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], nm.preprocess_frame_nlm_np(f, denoise_strength=10)), i
    assert not np.array_equal(got[0], en.preprocess_frame_np(frames[0], denoise_method="none"))
    off, dec0 = nm.preprocess_frames_nlm(model, x, enable=False, return_decisions=True)
    assert off.data_ptr() != x.data_ptr() and torch.equal(off, x) and dec0.cpu().tolist() == [False] * 3
    gray = np.stack([ed.bgr_to_gray_np(f) for f in frames])                  # 2-D frames always count as grey
    got2, dec2 = nm.preprocess_frames_nlm(model, torch.from_numpy(gray).cuda(), return_decisions=True)
    assert dec2.cpu().tolist() == [True] * 3
    for i in range(3):
        assert np.array_equal(got2.cpu().numpy()[i], nm.preprocess_frame_nlm_np(gray[i])), i


# ---- 3. the fixtures from the reference's own functions, through every entry ----------------------------------------------
def test_fixture_cases_through_the_device_functions(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import frame_loop, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=False, precision="exact", max_batch=1, max_hw=(32, 32)).to("cuda:0")
    m.load_state_dict(syn.make_trained_like_state_dict(3, 3, False, 0), strict=True)
    m.eval()
    g = load_golden("nlmeans_scenes")
    rows = [tuple(r) for r in g["cases"].tolist()]
    assert len(rows) == 10
    for tag, fn, H, W, seed, kind, strength, ndim, in_sha, decision, out_sha, stored in rows:
        H, W, seed, strength = int(H), int(W), int(seed), int(strength)
        frame = nm.make_nlm_scene(H, W, seed, kind)
        if ndim == "2":
            frame = ed.bgr_to_gray_np(frame)
        assert sha(frame) == in_sha, tag
        x = dev(torch, frame)
        grey = decision == "1"
        assert grey or fn == "preprocess", tag                               # an enhance row of a colour frame would need its own expectation
        want = np.repeat(g[tag + "_out"][..., None], 3, axis=2) if stored == "grey" else None

        def check(got, what):
            got = got.cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == (1, H, W, 3), (tag, what)
            assert sha(got[0]) == out_sha, (tag, what)
            if want is not None:
                assert np.array_equal(got[0], want), (tag, what)
            else:
                assert np.array_equal(got[0][:32, :32], g[tag + "_corner"]), (tag, what)
            return got[0]

        # a grey frame gives the same output through either composition; a colour frame is copied by preprocess_frame only
        pre, dec = nm.preprocess_frames_nlm(model, x, denoise_strength=strength, return_decisions=True)
        assert bool(dec[0]) == grey, tag
        out = check(pre, "preprocess_frames_nlm")
        if grey:
            enh = nm.enhance_grayscale_nlm(model, x, denoise_strength=strength)
            check(enh, "enhance_grayscale_nlm")
            assert torch.equal(nm.enhance_grayscale_nlm(model, x, denoise_strength=strength, channels_out=1), enh[..., 0]), tag
        else:
            assert np.array_equal(out, frame), tag
        # the head of the refactored loop: the same frames reach the network as when the fixture's output is fed in
        roi = (5, -3, W - 11, H - 9)
        a = frame_loop.process_frames_refactored(m, frame[None], roi, 32, denoise_method="fastNlMeans", denoise_strength=strength)
        b = frame_loop.process_frames(m, np.ascontiguousarray(en.crop_roi_np(out, roi)[None]), (32, 32), roi=None)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), tag
    assert m.status() == 0


# ---- 4. repeatability, streams, status ---------------------------------------------------------------------------------------
def test_repeatable_stream_independent_and_clean_status(torch_cuda, model):
    torch = torch_cuda
    frames = [nm.make_nlm_scene(35, 70, 30 + i, k) for i, k in enumerate(("ramp", "colour", "ramp"))]
    x = dev(torch, *frames)
    a = nm.preprocess_frames_nlm(model, x)
    b = nm.preprocess_frames_nlm(model, x)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = nm.preprocess_frames_nlm(model, x)
        d = nm.nl_means(model, x[..., 0].contiguous(), 10)
    s.synchronize()
    assert torch.equal(a, c)
    for i, f in enumerate(frames):
        assert np.array_equal(a.cpu().numpy()[i], nm.preprocess_frame_nlm_np(f)), i
        assert np.array_equal(d.cpu().numpy()[i], nm.nl_means_np(f[..., 0], 10)), i
    assert model.status() == 0
