"""The NumPy restatement of non-local-means denoising (unet_amd/nlmeans.py): the constants and the weight table of
OpenCV's published invoker, the vectorised form against the literal per-pixel one, properties that follow from the
algorithm, the fixtures made from the reference's own functions (tests/golden/nlmeans_scenes.npz), the limits, and the
surface of the device path as far as it shows without a device.  No GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from unet_amd import edges as ed
from unet_amd import enhance as en
from unet_amd import nlmeans as nm


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def quiet(H, W, seed, sigma=1.5):
    """A smooth image with a little noise: one the filter changes at every strength."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(np.rint(80 + 3.0 * x + 2.0 * y + 40 * (x > W // 2) + r.normal(0, sigma, (H, W))), 0, 255).astype(np.uint8)


# ---- 1. constants and the table ------------------------------------------------------------------------------------------
def test_constants_and_weight_table():
    assert nm.nlm_constants(7, 21) == (19096, 6, 64 / 49, 49785)
    assert nm.nlm_constants()[:2] == (19096, 6)
    for h, prefix in ((3, 48), (5, 132), (10, 528), (30, 4746), (40, 8437)):
        w = nm.nlm_weights(h)
        assert w.shape == (49785,) and w.dtype == np.int64
        assert w[0] == 19096 and (np.diff(w) <= 0).all()
        assert nm.prefix_length(w) == prefix and (w[:prefix] > 0).all() and not w[prefix:].any(), h
        assert w[prefix - 1] >= 0.001 * 19096
    assert (nm.nlm_weights(0) == 19096).all()                              # h = 0: weight 1.0 everywhere
    a = 100
    assert nm.nlm_weights(10)[a] == int(np.rint(19096 * np.exp(-(a * (64 / 49)) / 100.0)))


# ---- 2. the two NumPy forms, and properties --------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [5, 30])
def test_vectorised_form_equals_the_literal_loop(h):
    for img in (quiet(15, 17, 1), np.random.default_rng(2).integers(0, 256, (15, 17)).astype(np.uint8)):
        got = nm.nl_means_np(img, h)
        assert got.dtype == np.uint8 and np.array_equal(got, nm.nl_means_literal_np(img, h))
    assert not np.array_equal(nm.nl_means_np(quiet(15, 17, 1), h), quiet(15, 17, 1))          # the filter does something


def test_flip_and_transpose_equivariance():
    img = quiet(23, 31, 3)
    out = nm.nl_means_np(img, 10)
    assert not np.array_equal(out, img)
    assert np.array_equal(nm.nl_means_np(img[::-1].copy(), 10), out[::-1])
    assert np.array_equal(nm.nl_means_np(img[:, ::-1].copy(), 10), out[:, ::-1])
    assert np.array_equal(nm.nl_means_np(img.T.copy(), 10), out.T)


def test_constant_images_and_the_unsigned_accumulator():
    for v in (0, 255, 97):
        c = np.full((20, 20), v, np.uint8)
        for h in (3, 30):
            assert np.array_equal(nm.nl_means_np(c, h), c), (v, h)
    assert 441 * 19096 * 255 == 2147440680 and 441 * 19096 * 255 + 441 * 19096 // 2 > 2 ** 31 - 1      # why int32 would not do


def test_output_lies_within_each_search_window():
    img = quiet(30, 37, 4, sigma=4.0)
    ext = np.pad(img, 10, mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(ext, (21, 21))
    for h in (5, 30):
        out = nm.nl_means_np(img, h)
        assert (out >= win.min(axis=(2, 3))).all() and (out <= win.max(axis=(2, 3))).all()


def test_injected_tables():
    img = quiet(16, 18, 5)
    assert np.array_equal(nm.nl_means_np(img, 0.0, weights=nm.nlm_weights(10)), nm.nl_means_np(img, 10))
    assert np.array_equal(nm.nl_means_np(img, weights=nm.nlm_weights(10)[:528]), nm.nl_means_np(img, 10))    # the tail counts as 0
    one = nm.nl_means_np(img, weights=np.array([7]))                       # only patches at distance < 64 / 49 per pixel count
    assert np.array_equal(one, nm.nl_means_literal_np(img, weights=np.array([7])))
    for bad in (np.array([0, 5]), np.array([19097]), np.array([-1, 3]), np.array([1.0]), np.zeros((2, 2), np.int64), np.ones(49786, np.int64)):
        with pytest.raises(ValueError):
            nm.check_weights(bad)


# ---- 3. the fixtures from the reference's own functions ------------------------------------------------------------------
def fixture_cases():
    g = load_golden("nlmeans_scenes")
    out = []
    for tag, fn, H, W, seed, kind, strength, ndim, in_sha, decision, out_sha, stored in (tuple(r) for r in g["cases"].tolist()):
        frame = nm.make_nlm_scene(int(H), int(W), int(seed), kind)
        if ndim == "2":
            frame = ed.bgr_to_gray_np(frame)
        assert sha(frame) == in_sha, tag
        whole = np.repeat(g[tag + "_out"][..., None], 3, axis=2) if stored == "grey" else None
        corner = g[tag + "_corner"] if stored == "corner" else None
        out.append((dict(tag=tag, fn=fn, strength=int(strength), decision=decision == "1", out_sha=out_sha, kind=kind), frame, whole, corner))
    return out


def test_fixture_cases_through_the_np_compositions():
    cases = fixture_cases()
    assert len(cases) == 10 and {c[0]["fn"] for c in cases} == {"enhance", "preprocess"}
    assert {c[0]["strength"] for c in cases} == {5, 10} and {c[1].ndim for c in cases} == {2, 3}
    assert any(not c[0]["decision"] for c in cases)                          # a colour frame, copied
    rows, cols = 128, 64                                                     # one workgroup's tile (test_gpu_nlmeans.py asks the library)
    assert any(c[1].shape[0] > rows and c[1].shape[1] > cols and c[1].shape[0] % 8 and c[1].shape[1] % 8 for c in cases)
    for row, frame, whole, corner in cases:
        s = row["strength"]
        got = nm.preprocess_frame_nlm_np(frame, denoise_strength=s) if row["fn"] == "preprocess" else nm.enhance_grayscale_nlm_np(frame, denoise_strength=s)
        assert got.dtype == np.uint8 and got.shape == frame.shape[:2] + (3,)
        assert en.is_grayscale_np(frame) == row["decision"], row["tag"]
        assert sha(got) == row["out_sha"], row["tag"]
        if whole is not None:
            assert np.array_equal(got, whole), row["tag"]
        else:
            assert np.array_equal(got[:32, :32], corner), row["tag"]
        if row["decision"] or row["fn"] == "enhance":                        # the filter matters in every enhanced row
            plain = en.enhance_grayscale_np(frame, denoise_method="none")
            assert (got != plain).mean() >= 0.25, row["tag"]
        else:
            assert np.array_equal(got, frame)


def test_compositions_are_the_none_path_followed_by_the_filter():
    f = nm.make_nlm_scene(40, 52, 11)
    mid = en.enhance_grayscale_np(f, denoise_method="none", channels_out=1)
    assert np.array_equal(nm.enhance_grayscale_nlm_np(f, denoise_strength=7, channels_out=1), nm.nl_means_np(mid, 7.0))
    mid = en.enhance_grayscale_np(f, 4.0, 4, 1.0, "none", channels_out=1)
    assert np.array_equal(nm.enhance_grayscale_nlm_np(f, 4.0, 4, 1.0, 10)[..., 2], nm.nl_means_np(mid, 10.0))
    assert np.array_equal(nm.preprocess_frame_nlm_np(f, enable=False), f)
    assert np.array_equal(nm.preprocess_frame_nlm_np(f, True, 0.0), f)      # nothing is grey below a threshold of 0
    # the pinned refusals stay: the two enhance.py compositions do not take the method by name
    with pytest.raises(ValueError, match="fastNlMeans"):
        en.enhance_grayscale_np(f, denoise_method="fastNlMeans")
    with pytest.raises(ValueError, match="fastNlMeans"):
        en.preprocess_frame_np(f, denoise_method="fastNlMeans")


# ---- 4. limits and refusals --------------------------------------------------------------------------------------------------
def test_limits():
    nm.check_limits(14, 14)
    nm.check_limits(14, 14, device=True)
    for H, W in ((13, 40), (40, 13), (65536, 14), (40000, 40000)):
        with pytest.raises(ValueError):
            nm.check_limits(H, W)
    with pytest.raises(ValueError):
        nm.nl_means_np(np.zeros((13, 20), np.uint8), 5)
    with pytest.raises(ValueError):
        nm.enhance_grayscale_nlm_np(np.zeros((13, 20, 3), np.uint8))
    nm.check_limits(12, 12, 5, 15)                                           # other sizes are the host form's business ...
    assert np.array_equal(nm.nl_means_np(quiet(12, 12, 6), 10, 5, 15), nm.nl_means_literal_np(quiet(12, 12, 6), 10, 5, 15))
    for t, s in ((5, 21), (7, 15), (3, 7)):                                  # ... and refused on the device path, by name
        with pytest.raises(ValueError, match="supports only 7 and 21"):
            nm.check_limits(64, 64, t, s, device=True)
    with pytest.raises(ValueError):
        nm.check_limits(64, 64, 6, 21)
    nm.check_limits(None, None, weights=nm.nlm_weights(39), device=True)     # 8,020 entries
    with pytest.raises(ValueError, match="8192"):
        nm.check_limits(None, None, weights=nm.nlm_weights(40), device=True)  # 8,437
    w = np.zeros(8193, np.int64); w[0] = w[8192] = 1
    with pytest.raises(ValueError, match="8192"):
        nm.check_limits(None, None, weights=w, device=True)
    nm.check_limits(None, None, weights=w[:8192], device=True)


# ---- 5. the surface of the device path -----------------------------------------------------------------------------------------
def test_abi_symbols_and_header():
    from unet_amd import _lib
    new = {"unetpp_nlmeans_layout", "unetpp_nlmeans_u8"}
    assert new <= set(_lib.ABI_SYMBOLS) and "nlmeans.h" in _lib.HEADERS
    header = open(os.path.join(ROOT, "include", "unetpp.h")).read()
    assert new <= set(re.findall(r"\b(unetpp_[a-z0-9_]+)\s*\(", header))
    assert len(_lib.ABI["unetpp_nlmeans_u8"][1]) == 12


@pytest.mark.parametrize("cls", ["NestedUNet", "SimpleUNet"])
def test_host_tensors_and_unsupported_sizes_are_refused_before_the_device_is_touched(cls):
    import torch
    from unet_amd import frame_loop, nested_unet
    model = getattr(nested_unet, cls)(3)
    gray, frames = torch.zeros((1, 16, 16), dtype=torch.uint8), torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError) as err:
        nm.nl_means(model, gray)
    assert str(err.value) == "gray must be a uint8 CUDA tensor [B,H,W]"
    for fn in (nm.enhance_grayscale_nlm, nm.preprocess_frames_nlm):
        for t in (frames, gray.float(), frames[0]):
            with pytest.raises(RuntimeError) as err:
                fn(model, t)
            assert str(err.value) == "frames must be a uint8 CUDA tensor [B,H,W,3] or [B,H,W]"
    with pytest.raises(ValueError, match="supports only 7 and 21"):
        nm.nl_means(model, gray, 3.0, 5, 21)
    with pytest.raises(ValueError, match="supports only 7 and 21"):
        nm.nl_means(model, gray, 3.0, 7, 35)
    with pytest.raises(ValueError, match="8192"):
        nm.nl_means(model, gray, weights=nm.nlm_weights(40))
    with pytest.raises(ValueError):
        nm.enhance_grayscale_nlm(model, frames, channels_out=2)
    assert model._handle is None
    # the model's own two methods keep their refusal
    with pytest.raises(ValueError, match="fastNlMeans"):
        model.enhance_grayscale(frames, denoise_method="fastNlMeans")
    with pytest.raises(ValueError, match="fastNlMeans"):
        model.preprocess_frames(frames, denoise_method="fastNlMeans")
    assert model._handle is None
    assert "nlmeans" in frame_loop.process_frames_refactored.__doc__
