"""The NumPy restatement of the multi-scale and the DoG burr detector (unet_amd/edges.py: sobel_xy_np, sobel_edges_np,
sobel_s_threshold, edges_combined_np, detect_burrs_enhanced_np, dog_u8_np, burr_mask_dog_np, has_burr_np) against the
fixtures made from the reference's own functions (tests/golden/burr_enhanced_scenes.npz) and against itself.  Integer
and correctly rounded float64 arithmetic only: exact equality.  No GPU."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import edges as ed


def _rows():
    g = load_golden("burr_enhanced_scenes")
    return g, [tuple(r) for r in g["cases"].tolist()]


def _sha(*arrays):
    return hashlib.sha256(np.stack(arrays).tobytes()).hexdigest()


def test_fixture_holds_every_case():
    _, rows = _rows()
    kinds = [r[1] for r in rows]
    assert kinds.count("enhanced") == 3 and kinds.count("dog") == 6 and kinds.count("crafted") == 1
    assert sorted({(int(r[2]), int(r[3])) for r in rows if r[1] != "crafted"}) == [(96, 200), (448, 800), (512, 512)]


@pytest.mark.parametrize("index", range(3))
def test_enhanced_matches_the_reference(index):
    g, rows = _rows()
    tag, _, H, W, seed, sigma, sha = [r for r in rows if r[1] == "enhanced"][index]
    H, W = int(H), int(W)
    grey, cable = ed.make_burr_scene(H, W, int(seed), noise_sigma=float(sigma))
    assert sha == _sha(grey, cable)
    ref = np.unpackbits(g[tag + "_out"])[:H * W].reshape(H, W)           # the reference's burr mask is 0 / 1
    got = ed.detect_burrs_enhanced_np(grey, cable)
    assert got.dtype == np.uint8 and np.array_equal(got, ref) and ref.any()
    assert not ed.detect_burrs_enhanced_np(grey, np.zeros_like(cable)).any()       # the early returns


@pytest.mark.parametrize("index", range(3))
def test_dog_matches_the_reference(index):
    g, rows = _rows()
    mine = [r for r in rows if r[1] == "dog"][2 * index:2 * index + 2]
    H, W, seed = int(mine[0][2]), int(mine[0][3]), int(mine[0][4])
    grey, cable = ed.make_burr_scene(H, W, seed)
    for tag, _, _, _, _, scale, sha in mine:
        assert sha == _sha(grey, cable)
        ref = np.unpackbits(g[tag + "_out"])[:H * W].reshape(H, W) * np.uint8(255)
        got = ed.burr_mask_dog_np(grey, cable * int(scale))
        assert got.dtype == np.uint8 and np.array_equal(got, ref) and ref.any()
    assert not ed.burr_mask_dog_np(grey, np.zeros_like(cable)).any()


def test_crafted_tail_matches_the_reference_clause_by_clause():
    g, rows = _rows()
    (tag, _, H, W, _, _, sha), = [r for r in rows if r[1] == "crafted"]
    grey, edges, cable, boxes = ed.make_crafted_enhanced_case(return_boxes=True)
    assert (int(H), int(W)) == edges.shape and sha == _sha(grey, edges, cable)
    ref = np.unpackbits(g[tag + "_out"])[:edges.size].reshape(edges.shape)
    combined = ed.edges_combined_np(grey, edges)
    assert (combined != edges).any()                                       # Sobel and Laplacian fire, outside the band
    got = ed.burrs_from_edges_np(combined, cable, band_ksize=25, close_ksize=5, open_ksize=3, min_area=50, max_area=500, max_aspect=6.0,
                                 min_side=4)
    assert np.array_equal(got, ref)
    kept = {hw: bool(ref[y + h // 2, x + w // 2]) for (y, x, h, w), hw in zip(boxes, ed.CRAFTED_ENHANCED_RECTS)}
    assert not kept[(14, 4)] and kept[(14, 5)] and not kept[(4, 14)] and kept[(5, 14)]          # w >= 5, h >= 5
    assert kept[(6, 9)] and not kept[(6, 8)] and kept[(24, 21)] and not kept[(23, 22)]          # 50 <= area <= 500
    assert kept[(30, 5)] and not kept[(31, 5)]                                                  # aspect < 6


def test_sobel_xy_is_the_reflect_101_operator():
    ndi = pytest.importorskip("scipy.ndimage")
    r = np.random.default_rng(1)
    for H, W in ((8, 8), (9, 17), (33, 40)):
        grey = r.integers(0, 256, (H, W), dtype=np.uint8)
        kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
        dx, dy = ed.sobel_xy_np(grey)
        assert np.array_equal(dx, ndi.correlate(grey.astype(np.int32), kx, mode="mirror"))
        assert np.array_equal(dy, ndi.correlate(grey.astype(np.int32), kx.T, mode="mirror"))
        cx, cy = ed.sobel_np(grey)                                         # Canny's Sobel replicates: the border differs
        assert np.array_equal(dx[1:-1, 1:-1], cx[1:-1, 1:-1]) and np.array_equal(dy[1:-1, 1:-1], cy[1:-1, 1:-1])
        assert not dx[:, 0].any() and not dx[:, -1].any() and not dy[0].any() and not dy[-1].any()
        assert cx[:, 0].any() and cy[0].any()


def _per_pixel(s, smax, thr):
    """The reference's expression on an array of s with the frame maximum smax."""
    v = (np.sqrt(s.astype(np.float64)) / np.sqrt(np.float64(smax)) * 255).astype(np.uint8)
    return v > thr


def test_integer_threshold_equals_the_per_pixel_form_for_every_smax_of_a_sweep():
    sweep = [1, 2, 3, 4, 5, 7, 8, 9, 10, 15, 16, 17, 25, 26, 99, 100, 101, 255, 256, 1000, 2601, 65025, 65536, 260100, 10 ** 6, 1040400,
             2080799, ed.SOBEL_S_MAX]
    sweep += np.random.default_rng(2).integers(1, ed.SOBEL_S_MAX + 1, 40).tolist()
    for smax in sweep:
        for thr in (50, 0, 1, 127, 253, 254):
            c = ed.sobel_s_threshold(smax, thr)
            assert 0 <= c <= smax + 1
            # every s in a window around the threshold, the ends of the range, and a stride through all of it
            near = np.arange(max(c - 300, 0), min(c + 300, smax) + 1)
            s = np.unique(np.concatenate([near, np.arange(0, min(smax, 300) + 1), np.arange(max(smax - 300, 0), smax + 1),
                                          np.arange(0, smax + 1, max(smax // 5000, 1))]))
            assert np.array_equal(_per_pixel(s, smax, thr), s >= c), (smax, thr, c)
    for smax in (1, 2, 1000, ed.SOBEL_S_MAX):                              # all of the range for small maxima, and the limits
        assert ed.sobel_s_threshold(smax, 255) == smax + 1 and ed.sobel_s_threshold(smax, 300) == smax + 1
        assert ed.sobel_s_threshold(smax, -1) == 0 and ed.sobel_s_threshold(smax, 254) == smax
    assert ed.sobel_s_threshold(0, 50) == 1 and ed.sobel_s_threshold(0, -1) == 1
    assert ed.sobel_s_threshold(1, 50) == 1 and ed.sobel_s_threshold(2, 50) == 1 and ed.sobel_s_threshold(2, 180) == 2


def test_integer_threshold_equals_the_per_pixel_form_over_random_frames():
    r = np.random.default_rng(3)
    frames = [r.integers(0, 256, (40, 56), dtype=np.uint8), r.integers(100, 104, (40, 56), dtype=np.uint8),
              (np.arange(40)[:, None] * 3 + np.arange(56)[None, :] * 2).astype(np.uint8), ed.make_burr_scene(96, 200, 2)[0]]
    for grey in frames:
        dx, dy = ed.sobel_xy_np(grey)
        s = dx.astype(np.int64) ** 2 + dy.astype(np.int64) ** 2
        for thr in (50, 10, 200, 50.9, -3, 255):
            want = ed.sobel_edges_np(grey, thr)
            assert np.array_equal(want != 0, s >= ed.sobel_s_threshold(int(s.max()), thr)), thr
            assert set(np.unique(want)) <= {0, 255}
        assert ed.sobel_edges_np(grey).any() and not ed.sobel_edges_np(grey).all()
    # the stated departure: a constant frame is 0 / 0 in the reference and has no Sobel edges here
    flat = np.full((12, 20), 77, np.uint8)
    assert not ed.sobel_edges_np(flat).any() and not ed.sobel_edges_np(flat, -1).any()
    assert not ed.edges_combined_np(flat, np.zeros_like(flat)).any()


def test_laplacian_edges_keep_the_wrap_and_the_union_is_bytewise():
    grey = np.zeros((20, 24), np.uint8)
    grey[5, 5] = 255; grey[10, 5] = 75; grey[15, 5] = 64; grey[5, 15] = 4          # |lap| 1020 -> 252, 300 -> 44, 256 -> 0, 16
    lap = ed.laplacian_edges_np(grey)
    assert lap[5, 5] == 255 and lap[10, 5] == 255 and lap[15, 5] == 0 and lap[5, 15] == 255 and lap[5, 14] == 0
    assert ed.laplacian_edges_np(grey, 16)[5, 15] == 0 and ed.laplacian_edges_np(grey, 15.9)[5, 15] == 255
    canny = np.zeros_like(grey); canny[0, 0] = 255; canny[19, 23] = 1
    both = ed.edges_combined_np(grey, canny)
    assert np.array_equal(both, canny | ed.sobel_edges_np(grey) | lap) and both[0, 0] == 255 and both[19, 23] == 1
    with pytest.raises(ValueError):
        ed.edges_combined_np(grey, canny[:, :-1])


def test_dog_saturates_and_never_wraps():
    r = np.random.default_rng(4)
    grey = r.integers(0, 256, (33, 47), dtype=np.uint8)
    grey[10:20, 10:30] = 0; grey[14, 20] = 255                             # a bright pixel on dark, and the dark around bright
    t1, t2 = ed.gaussian_taps(3, 1.0), ed.gaussian_taps(7, 2.0)
    b1, b2 = ed.gaussian_blur_np(grey, t1).astype(int), ed.gaussian_blur_np(grey, t2).astype(int)
    d = ed.dog_u8_np(grey)
    assert d.dtype == np.uint8 and np.array_equal(d, np.maximum(b1 - b2, 0))
    assert (b1 < b2).sum() > 100 and not d[b1 < b2].any()                  # a wrap would give 256 - |difference| there
    assert np.array_equal(np.abs(d), d) and d[14, 20] > 30
    assert np.array_equal(ed.dog_u8_np(grey, t2, t1), np.maximum(b2 - b1, 0))              # taps1= / taps2= are the two kernels
    assert not ed.dog_u8_np(grey, t1, t1).any()


def test_tap_sums_are_256():
    t1, t2 = ed.resolve_dog_taps()
    assert len(t1) == 3 and len(t2) == 7 and int(t1.sum()) == 256 and int(t2.sum()) == 256
    assert np.array_equal(t1, t1[::-1]) and np.array_equal(t2, t2[::-1]) and t1.min() > 0 and t2.min() > 0
    assert int(ed.gaussian_taps(5, 1.0).sum()) == 256
    with pytest.raises(ValueError):
        ed.resolve_dog_taps(np.array([100, 100, 100], np.int32), None)
    with pytest.raises(ValueError):
        ed.resolve_dog_taps(None, np.full(9, 28, np.int32))


def test_has_burr_counts_non_zero_pixels():
    m = np.zeros((10, 10), np.uint8)
    m.ravel()[:49] = 255
    assert not ed.has_burr_np(m)
    m.ravel()[49] = 1
    assert ed.has_burr_np(m) and ed.has_burr_np(m, 50) and not ed.has_burr_np(m, 51)
    assert ed.has_burr_np(np.zeros((4, 4), np.uint8), 0)
