"""The grey-frame enhancement on the device (unetpp_gray_decision, unetpp_clahe_u8, unetpp_bilateral_u8,
unetpp_enhance_u8 and the NestedUNet methods built on them) against the NumPy restatement (unet_amd/enhance.py) and the
fixtures made from the reference's own functions (tests/golden/enhance_scenes.npz).  The float steps are float32 in a
fixed order without contraction on both sides: exact equality everywhere, no tolerance, nothing left out.
Run on the GPU box:  python -m pytest tests/test_gpu_enhance.py -m gpu"""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import edges as ed
from unet_amd import enhance as en

pytestmark = pytest.mark.gpu

SHAPES = ((67, 90), (64, 90), (64, 64))          # nothing divides / the padding quirk / clip = 1 and the residual walk


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
    """(core rows, core columns) of one workgroup of the apply kernel, from the library."""
    from unet_amd import _lib
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().unetpp_enhance_layout(ctypes.byref(rows), ctypes.byref(cols)) == 0
    assert rows.value >= 8 and cols.value >= 16
    return rows.value, cols.value


@pytest.fixture(scope="module")
def scenes():
    """The grey scenes of SHAPES, made once: {(H, W): uint8 [H,W,3]}."""
    return {(H, W): en.make_enhance_scene(H, W, 20 + i) for i, (H, W) in enumerate(SHAPES)}


def dev(torch, *frames):
    return torch.from_numpy(np.stack(frames)).cuda()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- 1. the fixtures from the reference's own functions ----------------------------------------------------------------
def test_fixture_cases_through_the_public_methods(torch_cuda, model):
    torch = torch_cuda
    g = load_golden("enhance_scenes")
    rows = [tuple(r) for r in g["cases"].tolist()]
    assert len(rows) == 23
    for tag, fn, H, W, seed, kind, variant, ndim, in_sha, decision, out_sha, stored in rows:
        H, W, seed = int(H), int(W), int(seed)
        frame = en.make_enhance_scene(H, W, seed, kind)
        if ndim == "2":
            frame = ed.bgr_to_gray_np(frame)
        assert sha(frame) == in_sha, tag
        v = dict(en.FIXTURE_VARIANTS[variant])
        other = ed.bgr_to_gray_np(en.make_enhance_scene(H, W, 99, "colour")) if ndim == "2" else en.make_enhance_scene(H, W, 99, "colour")
        # once the frame alone, once in a batch between a colour frame and a second copy
        for batch in (1, 3):
            x = dev(torch, *([frame] if batch == 1 else [other, frame, frame]))
            if fn == "preprocess":
                got, dec = model.preprocess_frames(x, return_decisions=True, **v)
                want_dec = decision == "1" and v.get("enable", True)
                assert dec.cpu().numpy()[batch // 2] == want_dec, tag
                assert model.is_grayscale(x).cpu().numpy()[batch // 2] == (decision == "1"), tag
            else:
                got = model.enhance_grayscale(x, **v)
            got = got.cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == (batch, H, W, 3), tag
            for i in ([0] if batch == 1 else [1, 2]):
                assert sha(got[i]) == out_sha, (tag, batch, i)
                if stored == "grey":
                    assert np.array_equal(got[i], np.repeat(g[tag + "_out"][..., None], 3, axis=2)), (tag, batch, i)
                else:
                    assert np.array_equal(got[i][:32, :32], g[tag + "_corner"]), (tag, batch, i)


# ---- 2. the smallest shapes at which the kernels can go wrong ---------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_enhance_small_shapes(torch_cuda, model, scenes, shape):
    torch = torch_cuda
    f = scenes[shape]
    x = dev(torch, f)
    assert np.array_equal(model.enhance_grayscale(x).cpu().numpy()[0], en.enhance_grayscale_np(f))
    got, dec = model.preprocess_frames(x, return_decisions=True)
    assert bool(dec[0]) is True and np.array_equal(got.cpu().numpy()[0], en.preprocess_frame_np(f))
    gray = ed.bgr_to_gray_np(f)
    assert np.array_equal(model.clahe(dev(torch, gray)).cpu().numpy()[0], en.clahe_np(gray))
    assert np.array_equal(model.bilateral_filter(dev(torch, gray)).cpu().numpy()[0], en.bilateral_np(gray))


def test_apply_seams_and_partial_last_tile(torch_cuda, model, tile):
    torch = torch_cuda
    rows, cols = tile
    H, W = 2 * rows + 3, 2 * cols + 5
    f = en.make_enhance_scene(H, W, 31)
    want = en.enhance_grayscale_np(f, denoise_strength=9)
    got = model.enhance_grayscale(dev(torch, f), denoise_strength=9).cpu().numpy()[0]
    for y in (rows - 1, rows, 2 * rows - 1, 2 * rows, H - 1):
        assert np.array_equal(got[y], want[y]), f"row {y}"
    for x in (cols - 1, cols, 2 * cols - 1, 2 * cols, W - 1):
        assert np.array_equal(got[:, x], want[:, x]), f"column {x}"
    assert np.array_equal(got, want)
    # the seam must matter: the filter reads across it
    gray = ed.bgr_to_gray_np(f)
    assert not np.array_equal(en.bilateral_np(gray, 9)[rows - 4:rows + 4], np.concatenate([en.bilateral_np(gray[:rows], 9)[-4:],
                                                                                         en.bilateral_np(gray[rows:], 9)[:4]]))


@pytest.mark.parametrize("grid", [(1, 1), (4, 4), (8, 8), (16, 16), (3, 5)])
def test_clahe_grids_and_luts(torch_cuda, model, scenes, grid):
    torch = torch_cuda
    for shape in ((67, 90), (64, 64)):
        gray = ed.bgr_to_gray_np(scenes[shape])
        for clip in (2.0, 0.0, 40.0):
            want, want_luts = en.clahe_np(gray, clip, grid, return_luts=True)
            got, luts = model.clahe(dev(torch, gray, gray[::-1].copy()), clip, grid, return_luts=True)
            assert luts.shape == (2, grid[0] * grid[1], 256)
            assert np.array_equal(luts.cpu().numpy()[0], want_luts), (shape, clip)
            assert np.array_equal(got.cpu().numpy()[0], want), (shape, clip)
            assert np.array_equal(got.cpu().numpy()[1], en.clahe_np(gray[::-1].copy(), clip, grid)), (shape, clip)
    f = scenes[(67, 90)]
    assert np.array_equal(model.enhance_grayscale(dev(torch, f), tile_grid=grid).cpu().numpy()[0], en.enhance_grayscale_np(f, tile_grid=grid))


@pytest.mark.parametrize("d", [3, 5, 9])
@pytest.mark.parametrize("gamma", [0.8, 1.0, 2.2])
def test_filter_sizes_and_gammas(torch_cuda, model, scenes, d, gamma):
    torch = torch_cuda
    f = scenes[(67, 90)]
    got = model.enhance_grayscale(dev(torch, f), gamma=gamma, denoise_strength=d).cpu().numpy()[0]
    assert np.array_equal(got, en.enhance_grayscale_np(f, gamma=gamma, denoise_strength=d))


def test_denoise_none_and_fastnlmeans(torch_cuda, model, scenes):
    torch = torch_cuda
    f = scenes[(64, 90)]
    x = dev(torch, f)
    want = en.enhance_grayscale_np(f, denoise_method="none")
    assert np.array_equal(model.enhance_grayscale(x, denoise_method="none").cpu().numpy()[0], want)
    assert not np.array_equal(want, en.enhance_grayscale_np(f))
    with pytest.raises(ValueError, match="fastNlMeans"):
        model.enhance_grayscale(x, denoise_method="fastNlMeans")
    with pytest.raises(ValueError, match="fastNlMeans"):
        model.preprocess_frames(x, denoise_method="fastNlMeans")
    with pytest.raises(ValueError):
        model.clahe(dev(torch, ed.bgr_to_gray_np(f)), 2.0, (17, 8))
    with pytest.raises(ValueError):
        model.bilateral_filter(dev(torch, ed.bgr_to_gray_np(f)), d=11)


# ---- 3. the decision on the device ----------------------------------------------------------------------------------------
def test_mixed_batch_through_preprocess_frames(torch_cuda, model):
    torch = torch_cuda
    H, W = 67, 90
    frames = [en.make_enhance_scene(H, W, 40, "grey"), en.make_enhance_scene(H, W, 41, "colour"), en.make_enhance_scene(H, W, 42, "flat")]
    x = dev(torch, *frames)
    got, dec = model.preprocess_frames(x, return_decisions=True)
    got = got.cpu().numpy()
    assert dec.dtype == torch.bool and dec.cpu().tolist() == [en.is_grayscale_np(f) for f in frames] == [True, False, True]
    assert np.array_equal(got[1], frames[1])                                # the colour frame comes back bit-identical
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], en.preprocess_frame_np(f)), i
    off = model.preprocess_frames(x, enable=False)
    assert off.data_ptr() != x.data_ptr() and torch.equal(off, x)
    d2, sums = model.is_grayscale(x, return_sums=True)
    assert d2.cpu().tolist() == [True, False, True]
    assert sums.cpu().tolist() == [list(en.channel_diff_sums(f)) for f in frames]


@pytest.mark.parametrize("threshold", [10.0, 2.5])
def test_decision_at_the_boundary(torch_cuda, model, threshold):
    torch = torch_cuda
    H, W = 30, 40
    edge = int(threshold * H * W)
    frames = [en.make_boundary_frame(H, W, edge + k) for k in (-1, 0, 1)]
    x = dev(torch, *frames)
    want = [en.is_grayscale_np(f, threshold) for f in frames]
    assert want == [True, False, False]
    dec, sums = model.is_grayscale(x, threshold, return_sums=True)
    assert dec.cpu().tolist() == want
    assert sums.cpu().numpy().max(axis=1).tolist() == [edge - 1, edge, edge + 1]
    got, dec2 = model.preprocess_frames(x, True, threshold, return_decisions=True)
    assert dec2.cpu().tolist() == want
    for i, f in enumerate(frames):
        assert np.array_equal(got.cpu().numpy()[i], en.preprocess_frame_np(f, True, threshold)), i


# ---- 4. inputs and outputs ---------------------------------------------------------------------------------------------------
def test_two_dimensional_frames_and_channels_out(torch_cuda, model, scenes):
    torch = torch_cuda
    f = scenes[(67, 90)]
    gray = ed.bgr_to_gray_np(f)
    want = en.enhance_grayscale_np(f)
    x3, x1 = dev(torch, f, f), dev(torch, gray, gray)
    for x in (x3, x1):
        out3 = model.enhance_grayscale(x).cpu().numpy()
        out1 = model.enhance_grayscale(x, channels_out=1).cpu().numpy()
        assert out3.shape == (2, 67, 90, 3) and out1.shape == (2, 67, 90)
        for i in range(2):
            assert np.array_equal(out3[i], want) and np.array_equal(out1[i], want[..., 0])
    got, dec = model.preprocess_frames(x1, return_decisions=True)          # a 2-D frame counts as grey
    assert dec.cpu().tolist() == [True, True] and np.array_equal(got.cpu().numpy()[1], want)
    assert model.is_grayscale(x1).cpu().tolist() == [True, True]
    # a width that is a multiple of 4 takes the word stores, 90 the byte stores
    f4 = en.make_enhance_scene(40, 132, 50)
    assert np.array_equal(model.enhance_grayscale(dev(torch, f4)).cpu().numpy()[0], en.enhance_grayscale_np(f4))
    assert np.array_equal(model.enhance_grayscale(dev(torch, f4), channels_out=1).cpu().numpy()[0], en.enhance_grayscale_np(f4, channels_out=1))


def test_bilateral_tables_with_a_permuted_tap_order(torch_cuda, model, scenes):
    torch = torch_cuda
    gray = ed.bgr_to_gray_np(scenes[(67, 90)])
    t = en.bilateral_tables(5, 20.0, 2.0)
    perm = np.random.default_rng(3).permutation(len(t[2]))
    tp = (t[0], t[1], t[2][perm], t[3][perm], t[4][perm])
    x = dev(torch, gray)
    for tables in (t, tp):
        assert np.array_equal(model.bilateral_filter(x, tables=tables).cpu().numpy()[0], en.bilateral_np(gray, tables=tables))
    assert np.array_equal(model.bilateral_filter(x, 5, 20.0, 2.0).cpu().numpy()[0], en.bilateral_np(gray, 5, 20.0, 2.0))


# ---- 5. repeatability and streams -----------------------------------------------------------------------------------------
def test_repeatable_and_stream_independent(torch_cuda, model):
    torch = torch_cuda
    frames = [en.make_enhance_scene(67, 261, 60 + i, k) for i, k in enumerate(("grey", "colour", "grey"))]
    x = dev(torch, *frames)
    a = model.preprocess_frames(x)
    b = model.preprocess_frames(x)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = model.preprocess_frames(x)
    s.synchronize()
    assert torch.equal(a, c)
    for i, f in enumerate(frames):
        assert np.array_equal(a.cpu().numpy()[i], en.preprocess_frame_np(f)), i


# ---- 6. the head of the refactored loop -------------------------------------------------------------------------------------
def test_process_frames_refactored(torch_cuda):
    torch = torch_cuda
    from unet_amd import frame_loop, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=False, precision="exact", max_batch=2, max_hw=(64, 64)).to("cuda:0")
    m.load_state_dict(syn.make_trained_like_state_dict(3, 3, False, 0), strict=True)
    m.eval()
    H, W = 96, 136
    frames = [en.make_enhance_scene(H, W, 70, "grey"), en.make_enhance_scene(H, W, 71, "colour")]
    roi = (30, -4, 70, 60)                                                   # x, y, w, h: clamped at the top
    pred, cable, tape = frame_loop.process_frames_refactored(m, np.stack(frames), roi, 64)
    crops = np.stack([en.crop_roi_np(en.preprocess_frame_np(f), roi) for f in frames])
    assert crops.shape == (2, 56, 70, 3)
    pred2, cable2, tape2 = frame_loop.process_frames(m, crops, (64, 64), roi=None)
    assert pred.shape == (2, 64, 64) and cable.shape == (2, 56, 70)
    assert torch.equal(pred, pred2) and torch.equal(cable, cable2) and torch.equal(tape, tape2)
    with pytest.raises(ValueError):
        frame_loop.process_frames_refactored(m, np.stack(frames), (200, 0, 10, 10), 64)
