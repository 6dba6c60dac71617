"""Sliding-window inference, host side: the plan and the NumPy restatement (unet_amd/tiling.py) against the fixtures made
from the reference's own predict methods (tests/golden/tiled_scenes.npz, scripts/make_golden_tiled.py).  The blend is
float32 arithmetic in a fixed order: exact equality of the bits, no tolerance.  No GPU is needed."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import tiling as tl


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def load_cases():
    g = load_golden("tiled_scenes")
    cases = []
    for r in g["cases"].tolist():
        tag, C, H, W, index, seed, patch, stride, target, blend, thr, gate_class, frame_sha, fed_sha = r
        cases.append(dict(tag=tag, C=int(C), H=int(H), W=int(W), index=int(index), seed=int(seed), patch=int(patch), stride=int(stride),
                          target=int(target), blend=blend, thr=float(thr) if thr else None, gate_class=int(gate_class),
                          frame_sha=frame_sha, fed_sha=fed_sha))
    return g, cases


G, CASES = load_cases()
TAGS = [c["tag"] for c in CASES]


def frame_rgb(syn, c):
    img = np.ascontiguousarray(syn.make_frame_u8(c["H"], c["W"], c["index"], "smooth", c["seed"])[..., ::-1])
    assert sha(img) == c["frame_sha"], c["tag"]
    return img


def test_fixture_has_every_branch():
    assert len(CASES) == 6 and {c["C"] for c in CASES} == {2, 3}
    assert all((c["patch"], c["stride"]) == (64, 32) for c in CASES)
    assert {(c["H"], c["W"]) for c in CASES} >= {(100, 150), (128, 96), (48, 150)}
    assert any(c["target"] == c["patch"] for c in CASES) and any(c["target"] == 32 for c in CASES)
    assert {c["C"] for c in CASES if c["thr"] is not None} == {2, 3}
    for c in CASES:
        out = G[c["tag"] + "_output"]
        assert out.dtype == np.float32 and out.shape == (c["H"], c["W"], c["C"])
        top = np.sort(out, axis=-1)
        assert ((top[..., -1] - top[..., -2]) < 2e-3).mean() <= 0.01, c["tag"]
        if c["thr"] is not None:
            s = G[c["tag"] + "_scores"]
            assert np.abs(s - np.float32(c["thr"])).min() > 1e-2 and 0 < (s >= c["thr"]).sum() < len(s), c["tag"]


@pytest.mark.parametrize("tag", TAGS)
def test_predict_tiled_np_equals_reference_bits(syn, tag):
    c = CASES[TAGS.index(tag)]
    img = frame_rgb(syn, c)
    maps = G[tag + "_maps"]
    seen = []

    def model_fn(patches):
        seen.append(patches)
        return maps

    mask, output = tl.predict_tiled_np(img, model_fn, c["patch"], c["stride"], c["target"], c["C"], c["blend"], c["thr"], c["gate_class"])
    # the patch batch is what the reference resized for its network (it feeds RGB; the batch is BGR for the engine)
    assert seen[0].dtype == np.uint8 and sha(seen[0][..., ::-1]) == c["fed_sha"], tag
    assert output.dtype == np.float32 and np.array_equal(bits(output), bits(G[tag + "_output"])), tag
    assert mask.dtype == np.uint8 and np.array_equal(mask, G[tag + "_mask"]), tag
    if c["thr"] is not None:
        include, scores = tl.tile_gate_np(maps, c["thr"], c["gate_class"])
        assert np.array_equal(scores, G[tag + "_scores"]) and 0 < include.sum() < len(include)
        # the gate matters: without it the output differs
        assert not np.array_equal(tl.blend_tiles_np(maps, tl.tile_plan(c["H"], c["W"], c["patch"], c["stride"]), c["H"], c["W"], c["patch"])[1],
                                  output)


def test_channel_order(syn):
    c = CASES[0]
    img = frame_rgb(syn, c)
    plan = tl.tile_plan(c["H"], c["W"], c["patch"], c["stride"])
    a = tl.gather_tiles_np(img, plan, c["patch"], c["target"], "rgb")
    b = tl.gather_tiles_np(np.ascontiguousarray(img[..., ::-1]), plan, c["patch"], c["target"], "bgr")
    assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        tl.gather_tiles_np(img, plan, c["patch"], c["target"], "gbr")


# ---- the plan -------------------------------------------------------------------------------------------------------------
def reference_axis(n, patch, stride):
    """The reference's arithmetic for one axis, written out as its loop runs (inference_binary_patch.py:41-68)."""
    k = (n - patch) // stride + 1
    if (n - patch) % stride != 0:
        k += 1
    return [max(0, min(i * stride + patch, n) - patch) for i in range(k)]


@pytest.mark.parametrize("h,w,patch,stride", [(100, 150, 64, 32), (128, 96, 64, 32), (48, 150, 64, 32), (1080, 1920, 384, 192),
                                              (64, 64, 64, 32), (65, 64, 64, 32), (200, 200, 64, 64), (300, 210, 64, 100), (70, 133, 64, 7)])
def test_plan_properties(h, w, patch, stride):
    plan = tl.tile_plan(h, w, patch, stride)
    assert list(plan.ys) == reference_axis(h, patch, stride) and list(plan.xs) == reference_axis(w, patch, stride)
    assert plan.n_patches == len(plan.ys) * len(plan.xs) == len(plan.origins)
    assert plan.origins == [(y, x) for y in plan.ys for x in plan.xs]                      # (i, j) order, j fastest
    for n, origins in ((h, plan.ys), (w, plan.xs)):
        assert list(origins) == sorted(origins) and origins[0] == 0
        assert all(0 <= o and (o + patch <= n or o == 0) for o in origins)                 # clamped: never past the end
        assert origins[-1] == max(0, n - patch)                                            # the last patch ends at the border
        if stride <= patch:                                                                # then the patches leave no gap
            cover = np.zeros(n, bool)
            for o in origins:
                cover[o:o + patch] = True
            assert cover.all()
        assert all(b - a <= stride for a, b in zip(origins, origins[1:]))


def test_plan_of_the_issue_workload():
    plan = tl.tile_plan(1080, 1920, 384, 192)
    assert plan.ys == (0, 192, 384, 576, 696) and len(plan.xs) == 9 and plan.n_patches == 45


def test_plan_smaller_than_the_patch():
    assert tl.tile_plan(48, 150, 64, 32).ys == (0,)             # (48 - 64) % 32 != 0: one patch, padded
    assert tl.tile_plan(32, 150, 64, 32).ys == ()               # (32 - 64) % 32 == 0: Python's floor division gives none
    assert tl.tile_plan(32, 150, 64, 32).n_patches == 0
    mask, out = tl.predict_tiled_np(np.zeros((32, 150, 3), np.uint8), None, 64, 32, 32, 3)
    assert mask.shape == (32, 150) and not mask.any() and out.shape == (32, 150, 3) and not out.any()
    with pytest.raises(ValueError):
        tl.tile_plan(100, 100, 64, 0)
    with pytest.raises(ValueError):                              # a pad of the axis length or more: np.pad would mirror twice
        assert tl.tile_plan(20, 150, 64, 64).ys == (0,)
        tl.gather_tiles_np(np.zeros((20, 150, 3), np.uint8), tl.tile_plan(20, 150, 64, 64), 64, 32)


def test_uncovered_pixel_is_zero_and_class_zero():
    plan = tl.tile_plan(64, 96, 64, 32)
    maps = np.full((2, 2, 32, 32), 3.0, np.float32)
    maps[:, 0] = 1.0
    mask, out = tl.blend_tiles_np(maps, plan, 64, 96, 64, include=np.array([True, False]))
    assert (mask[:, :64] == 1).all() and (out[:, :64] == np.float32([1, 3])).all()
    assert not mask[:, 64:].any() and not out[:, 64:].any()


# ---- the float resize ---------------------------------------------------------------------------------------------------------
def test_resize_f32_identity_and_dtype():
    r = np.random.default_rng(0)
    x = r.standard_normal((17, 23, 3)).astype(np.float32)
    y = tl.resize_linear_f32_np(x, (23, 17))
    assert y.dtype == np.float32 and np.array_equal(y, x)
    assert tl.resize_linear_f32_np(x[:, :, 0], (46, 34)).shape == (34, 46)
    with pytest.raises(ValueError):
        tl.resize_linear_f32_np(x.astype(np.float64), (23, 17))


@pytest.mark.parametrize("ratio", [2, 3])
def test_resize_f32_against_scipy_on_integer_upscale(ratio):
    """Half-pixel centres with edge replication: dst d samples src (d + 0.5) / ratio - 0.5, which scipy.ndimage's
    map_coordinates(order=1, mode="nearest") evaluates in float64.  The float32 restatement differs from it by the
    rounding of the coordinate (half a float32 ulp of a value below 32: 2^-20 of a pixel step, times a slope of at most
    the value range 8), and of two coefficients, four products and three sums (2^-24 relative each, values below 4):
    7.6e-6 + 1.7e-6, bounded here by 2^-19 times the value range = 1.5e-5."""
    from scipy import ndimage
    r = np.random.default_rng(1)
    x = r.uniform(-4, 4, (16, 24, 2)).astype(np.float32)
    h, w = 16 * ratio, 24 * ratio
    got = tl.resize_linear_f32_np(x, (w, h))
    yy = (np.arange(h) + 0.5) / ratio - 0.5
    xx = (np.arange(w) + 0.5) / ratio - 0.5
    grid = np.meshgrid(yy, xx, indexing="ij")
    want = np.stack([ndimage.map_coordinates(x[..., c].astype(np.float64), grid, order=1, mode="nearest") for c in range(2)], -1)
    assert np.abs(got - want).max() <= 8.0 * 2.0 ** -19


def test_resize_u8_matches_the_oracle(oracle):
    r = np.random.default_rng(2)
    img = r.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    for size in ((32, 32), (64, 64), (48, 80)):
        assert np.array_equal(tl.resize_linear_u8_np(img, size), oracle.cv2_resize_linear_u8_np(img, size))
    assert np.array_equal(tl.resize_linear_u8_np(img, (64, 64)), img)


def test_abi_lists_the_new_entry_points():
    from unet_amd import _lib
    assert {"unetpp_tile_gather_u8", "unetpp_tile_gate_f32", "unetpp_tile_blend_f32"} <= set(_lib.ABI_SYMBOLS)
    assert "tiling.h" in _lib.HEADERS
