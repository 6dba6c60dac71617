"""The NumPy restatement of the grey-frame enhancement (unet_amd/enhance.py): the fixtures made from the reference's own
functions (tests/golden/enhance_scenes.npz), properties of CLAHE and the bilateral filter that follow from OpenCV's
published algorithms, the grey decision at its boundary, and the limits.  No GPU."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import edges as ed
from unet_amd import enhance as en


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fixture_cases():
    """(row fields, input frame, expected whole output or None, corner or None) per fixture case."""
    g = load_golden("enhance_scenes")
    out = []
    for tag, fn, H, W, seed, kind, variant, ndim, in_sha, decision, out_sha, stored in (tuple(r) for r in g["cases"].tolist()):
        H, W, seed = int(H), int(W), int(seed)
        frame = en.make_enhance_scene(H, W, seed, kind)
        if ndim == "2":
            frame = ed.bgr_to_gray_np(frame)
        assert sha(frame) == in_sha, tag
        whole = np.repeat(g[tag + "_out"][..., None], 3, axis=2) if stored == "grey" else None
        corner = g[tag + "_corner"] if stored == "corner" else None
        out.append((dict(tag=tag, fn=fn, variant=variant, decision=decision == "1", out_sha=out_sha), frame, whole, corner))
    return out


def test_fixture_cases_through_the_np_compositions():
    cases = fixture_cases()
    assert len(cases) == 23 and {c[0]["fn"] for c in cases} == {"enhance", "preprocess"}
    assert {c[0]["variant"] for c in cases} == set(en.FIXTURE_VARIANTS)
    for row, frame, whole, corner in cases:
        v = en.FIXTURE_VARIANTS[row["variant"]]
        got = en.preprocess_frame_np(frame, **v) if row["fn"] == "preprocess" else en.enhance_grayscale_np(frame, **v)
        assert got.dtype == np.uint8 and got.shape == frame.shape[:2] + (3,)
        assert en.is_grayscale_np(frame) == row["decision"], row["tag"]
        assert sha(got) == row["out_sha"], row["tag"]
        if whole is not None:
            assert np.array_equal(got, whole), row["tag"]
        else:
            assert np.array_equal(got[:32, :32], corner), row["tag"]


def test_clahe_one_tile_without_clip_is_global_equalisation():
    g = ed.bgr_to_gray_np(en.make_enhance_scene(45, 70, 11))
    cdf = np.cumsum(np.bincount(g.ravel(), minlength=256))
    lut = np.clip(np.rint(cdf.astype(np.float32) * (np.float32(255) / np.float32(g.size))), 0, 255).astype(np.uint8)
    out, luts = en.clahe_np(g, 0.0, (1, 1), return_luts=True)
    assert luts.shape == (1, 256) and np.array_equal(luts[0], lut)
    assert np.array_equal(out, lut[g])


def test_clahe_flat_image_against_a_hand_computed_lut():
    # 40 x 50 on 8 x 8: 50 % 8 = 2, so the image is extended to 48 x 56 and a tile is 6 x 7 = 42 pixels, all in bin 97.
    # clip = max(int(2 * 42 / 256), 1) = 1: 41 counts are clipped; batch = 0, residual = 41, step = 256 // 41 = 6: bins
    # 0, 6, ..., 240 get one each.  cumsum_i = (number of multiples of 6 in [0, i], capped at 41) + (1 if i >= 97).
    flat = np.full((40, 50), 97, np.uint8)
    assert en.clahe_geometry(40, 50, (8, 8)) == (8, 8, 7, 6, 6, 8)
    i = np.arange(256)
    cum = np.minimum(i // 6 + 1, 41) + (i >= 97)
    lut = np.rint(cum.astype(np.float32) * (np.float32(255) / np.float32(42))).astype(np.uint8)
    assert lut[97] == 109 and lut[255] == 255 and lut[0] == 6
    out, luts = en.clahe_np(flat, 2.0, (8, 8), return_luts=True)
    assert all(np.array_equal(l, lut) for l in luts)
    assert (out == 109).all()


def test_clahe_padding_quirk_rows_divisible_columns_not():
    assert en.clahe_geometry(64, 90, (8, 8)) == (8, 8, 12, 9, 6, 8)        # 72 rows: tile height 9, not 8
    assert en.clahe_geometry(64, 96, (8, 8)) == (8, 8, 12, 8, 0, 0)
    g = ed.bgr_to_gray_np(en.make_enhance_scene(64, 90, 1))
    luts = en.clahe_luts_np(g, 2.0, (8, 8))
    # the last tile row's histogram holds rows 63 .. 71 of the extended image: row 63 and rows 62 .. 55 (reflected)
    rows = g[[63, 62, 61, 60, 59, 58, 57, 56, 55]]
    cols = np.r_[np.arange(84, 90), 88 - np.arange(6)]                      # columns 84 .. 95: 84 .. 89, then 88 .. 83
    hist = np.bincount(rows[:, cols].ravel(), minlength=256)
    assert hist.sum() == 108
    clipped = np.maximum(hist - 1, 0).sum()                                 # clip = max(int(2 * 108 / 256), 1) = 1
    h2 = np.minimum(hist, 1) + clipped // 256
    res = clipped % 256
    if res:
        step = max(256 // res, 1)
        k = np.arange(256)
        h2 = h2 + ((k % step == 0) & (k // step < res))
    lut = np.clip(np.rint(np.cumsum(h2).astype(np.float32) * (np.float32(255) / np.float32(108))), 0, 255).astype(np.uint8)
    assert np.array_equal(luts[63], lut)


def test_bilateral_flat_identity_and_spatial_mean():
    flat = np.full((20, 30), 141, np.uint8)
    assert np.array_equal(en.bilateral_np(flat), flat)
    g = ed.bgr_to_gray_np(en.make_enhance_scene(33, 47, 12))
    radius, color_w, space_w, dy, dx = en.bilateral_tables(5, 1e6, 75.0)
    assert len(space_w) == 13 and color_w.min() >= np.float32(1) - np.float32(2.0 ** -23)     # every colour weight is 1 to 2 ulp
    pad = np.pad(g, 2, mode="reflect").astype(np.float64)
    s = sum(pad[2 + dy[k]:2 + dy[k] + 33, 2 + dx[k]:2 + dx[k] + 47] * float(space_w[k]) for k in range(13))
    mean = s / float(space_w.astype(np.float64).sum())
    assert np.abs(mean - np.rint(mean)).max() < 0.5 - 1e-4                  # no pixel sits on a rounding tie
    assert np.array_equal(en.bilateral_np(g, 5, 1e6, 75.0), np.rint(mean).astype(np.uint8))


def test_bilateral_tap_counts_and_order():
    assert [len(en.bilateral_tables(d)[2]) for d in (3, 5, 9)] == [5, 13, 49]
    radius, _, space_w, dy, dx = en.bilateral_tables(5)
    assert radius == 2 and list(zip(dy[:4], dx[:4])) == [(-2, 0), (-1, -1), (-1, 0), (-1, 1)] and (dy[6], dx[6]) == (0, 0)
    assert space_w[6] == 1 and space_w[0] == np.float32(np.exp(4 * (-0.5 / 75.0 ** 2)))
    assert en.bilateral_tables(0, 75, 1.0)[0] == 2 and en.bilateral_tables(-1, 75, 0.1)[0] == 1
    # a permuted tap order is another summation order: the tables are honoured as given
    g = ed.bgr_to_gray_np(en.make_enhance_scene(33, 47, 12))
    t = en.bilateral_tables(5, 20.0, 2.0)
    perm = np.random.default_rng(0).permutation(13)
    a, b = en.bilateral_np(g, tables=t), en.bilateral_np(g, tables=(t[0], t[1], t[2][perm], t[3][perm], t[4][perm]))
    assert np.abs(a.astype(int) - b.astype(int)).max() <= 1


def test_gamma_table():
    assert en.gamma_table(1.0) is None
    t = en.gamma_table(0.8)
    assert t.dtype == np.uint8 and t[0] == 0 and t[255] == 255 and t[128] == int(((128 / 255.0) ** 1.25) * 255) == 107
    assert (np.diff(t.astype(int)) >= 0).all() and (en.gamma_table(2.2) >= t).all()


@pytest.mark.parametrize("threshold", [10.0, 2.5, 0.1])
def test_grey_decision_at_the_boundary(threshold):
    H, W = 30, 40
    n = H * W
    edge = int(threshold * n)
    assert edge == threshold * n
    for total, want in ((edge - 1, True), (edge, False), (edge + 1, False)):
        f = en.make_boundary_frame(H, W, total)
        assert max(en.channel_diff_sums(f)) == total
        assert en.is_grayscale_np(f, threshold) is want
        b, g, r = (f[..., c].astype(float) for c in range(3))                # the reference's expression
        ref = max(np.abs(b - g).mean(), np.abs(g - r).mean(), np.abs(r - b).mean()) < threshold
        assert bool(ref) is want
    assert en.is_grayscale_np(np.zeros((H, W), np.uint8)) is True           # a 2-D frame counts as grey


def test_limits_and_fastnlmeans():
    g = np.zeros((20, 20), np.uint8)
    for bad in ((0, 8), (8, 17), (20, 8), (8, 20)):
        with pytest.raises(ValueError):
            en.clahe_np(g, 2.0, bad)
    en.clahe_np(g, 2.0, (16, 16))
    with pytest.raises(ValueError, match="radius"):
        en.bilateral_np(g, d=11)
    with pytest.raises(ValueError, match="radius"):
        en.bilateral_np(np.zeros((4, 20), np.uint8), d=9)
    en.bilateral_np(np.zeros((5, 5), np.uint8), d=9)
    with pytest.raises(ValueError):
        en.check_limits(2 ** 15 + 1, 2 ** 15)
    with pytest.raises(ValueError):
        en.check_limits(65536, 4)
    t = en.bilateral_tables(5)
    with pytest.raises(ValueError, match="outside the radius"):
        en.bilateral_np(g, tables=(1, t[1], t[2][:5], t[3][:5], t[4][:5]))      # tap 0 is (-2, 0)
    for fn in (en.enhance_grayscale_np, en.preprocess_frame_np):
        with pytest.raises(ValueError, match="fastNlMeans"):
            fn(en.make_enhance_scene(20, 20, 0), denoise_method="fastNlMeans")
    with pytest.raises(ValueError, match="fastNlMeans"):
        en.preprocess_frame_np(en.make_enhance_scene(20, 20, 0, "colour"), denoise_method="fastNlMeans")
    f = en.make_enhance_scene(20, 24, 0)
    assert np.array_equal(en.enhance_grayscale_np(f, denoise_method="median"), en.enhance_grayscale_np(f, denoise_method="none"))
    assert np.array_equal(en.crop_roi_np(f, (-3, 5, 10, 100)), f[5:20, 0:7])
    # the workspace totals where the 256-byte rounding of a part decides, and the shapes either side of a limit (no device)
    import ctypes
    from unet_amd import _lib
    lib = ctypes.CDLL(_lib.build())
    lib.unetpp_enhance_workspace_bytes.restype = ctypes.c_size_t
    for (b, h, w, tx, ty), n in {(1, 2, 2, 1, 1): 2048, (1, 17, 17, 1, 1): 2304, (1, 16, 16, 8, 8): 82688, (1, 17, 17, 8, 8): 82944,
                                 (1, 33, 129, 8, 8): 86784, (1, 33, 129, 16, 16): 332544, (16, 33, 129, 8, 8): 1379840,
                                 (1, 512, 512, 8, 8): 344576, (1, 32768, 32768, 8, 8): 1073824256, (1, 32768, 32769, 8, 8): 0,
                                 (1, 1, 1, 1, 1): 0, (1, 16, 16, 16, 16): 0, (1, 33, 129, 17, 1): 0, (1, 33, 129, 1, 17): 0,
                                 (1, 33, 129, 0, 1): 0, (1, 65536, 8, 1, 1): 0, (0, 33, 129, 8, 8): 0, (65536, 33, 129, 8, 8): 0}.items():
        assert lib.unetpp_enhance_workspace_bytes(b, h, w, tx, ty) == n, (b, h, w, tx, ty)
