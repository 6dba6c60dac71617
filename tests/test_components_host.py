"""CPU side of the connected-component feature: the NumPy restatement (unet_amd/components.py) against scipy, its
three filters against the fixtures made from the reference's own functions (scripts/make_golden_cc.py), and the
binding's bookkeeping.  The device side is tests/test_gpu_components.py."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import components as cc

# kept pixels, 8-connectivity, reference defaults (largest: min_area=50, cable_shape: roi_width=W):
# (H, W, seed, class) -> (components, largest, cable_shape, spatial)
SCENE_TABLE = {
    (512, 512, 0, 1): (1487, 21511, 21511, 32258), (512, 512, 0, 2): (1386, 38827, 0, 38827),
    (512, 512, 1, 1): (1479, 22276, 22276, 33003), (512, 512, 1, 2): (1462, 37601, 0, 37601),
    (448, 800, 0, 1): (2070, 29434, 0, 44143), (448, 800, 0, 2): (1927, 53028, 0, 53028),
    (448, 800, 1, 1): (2011, 30480, 0, 45197), (448, 800, 1, 2): (1945, 51421, 0, 51421),
}
SCENE_SHA = {(512, 512, 1): "ca478a86fc3fd61c", (448, 800, 0): "bfdced768338d28b", (448, 800, 1): "1aa6ab3a49be73ce"}
RULE_KW = {"largest": {"min_area": 50}, "cable_shape": {}, "spatial": {}}


def golden_cases(name):
    g = load_golden(name)
    return g, [tuple(r) for r in g["cases"].tolist()]


def scipy_reference(fg, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    labels, n = ndimage.label(fg, structure=np.ones((3, 3), int) if connectivity == 8 else None)
    idx = np.arange(n + 1)
    stats = np.zeros((n + 1, 5), np.int32)
    for i, box in enumerate(ndimage.find_objects(labels + 1)):
        if box is not None:
            stats[i, :4] = (box[1].start, box[0].start, box[1].stop - box[1].start, box[0].stop - box[0].start)
    stats[:, 4] = ndimage.sum(np.ones_like(labels), labels, idx)
    ys, xs = np.indices(labels.shape)
    sums = np.stack([ndimage.sum(xs, labels, idx), ndimage.sum(ys, labels, idx)], 1).astype(np.uint64)
    return labels.astype(np.int32), stats, sums


def check_against_scipy(mask, connectivity, match_class=-1):
    labels, stats, sums = cc.components_np(mask, connectivity, match_class)
    rl, rs, rsum = scipy_reference(cc.foreground(mask, match_class), connectivity)
    assert labels.dtype == np.int32 and stats.dtype == np.int32 and sums.dtype == np.uint64
    assert np.array_equal(labels, rl)
    assert np.array_equal(stats, rs)
    assert np.array_equal(sums, rsum)


def test_scene_generator_is_the_issues():
    for (H, W, seed), sha in SCENE_SHA.items():
        assert hashlib.sha256(cc.make_scene_mask(H, W, seed).tobytes()).hexdigest().startswith(sha)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_matches_scipy_on_scenes(connectivity):
    for H, W, seed in ((512, 512, 0), (448, 800, 1)):
        mask = cc.make_scene_mask(H, W, seed)
        for cls in (1, 2, -1):
            check_against_scipy(mask, connectivity, cls)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_matches_scipy_on_speckle_and_ragged(connectivity):
    net = load_golden("b_c3_512x512")["mask"]
    for cls in (0, 1, 2):
        check_against_scipy(net[0], connectivity, cls)
    r = np.random.default_rng(5)
    for H, W in ((37, 300), (1, 1), (5, 1027), (1, 40), (40, 1)):
        for density in (0.2, 0.5, 0.8):
            check_against_scipy((r.random((H, W)) < density).astype(np.uint8), connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_matches_scipy_on_adversarial_shapes(connectivity):
    for name, mask in cc.make_adversarial_masks(128, 256).items():
        check_against_scipy(mask, connectivity)
    for name in ("serpentine", "tile_corners"):
        check_against_scipy(cc.make_adversarial_masks()[name], connectivity)


def test_adversarial_component_counts():
    m = cc.make_adversarial_masks()
    n = lambda name, c: len(cc.components_np(m[name], c)[1]) - 1
    assert (n("ones", 8), n("zeros", 8), n("serpentine", 4), n("comb", 4)) == (1, 0, 1, 1)
    assert (n("diagonal", 8), n("diagonal", 4), n("antidiagonal", 8), n("antidiagonal", 4)) == (1, 512, 1, 512)
    assert (n("checkerboard", 8), n("checkerboard", 4)) == (1, 512 * 512 // 2)
    assert n("tile_corners", 8) == 5 * 17 and n("tile_corners", 4) == 5 * 17      # 2x2 blocks where four tiles meet


def test_labels_are_numbered_in_raster_order_of_first_pixels():
    mask = np.array([[0, 0, 0, 0, 1, 0, 1],
                     [1, 0, 1, 0, 1, 0, 1],
                     [1, 0, 1, 1, 1, 0, 0],
                     [0, 0, 0, 0, 0, 1, 0]], np.uint8)
    l8, s8, sums8 = cc.components_np(mask, 8)
    assert l8.tolist() == [[0, 0, 0, 0, 1, 0, 2], [3, 0, 1, 0, 1, 0, 2], [3, 0, 1, 1, 1, 0, 0], [0, 0, 0, 0, 0, 1, 0]]
    l4, s4, _ = cc.components_np(mask, 4)
    assert l4[3, 5] == 4 and len(s4) == 5
    assert s8[1].tolist() == [2, 0, 4, 4, 7] and s8[0].tolist() == [0, 0, 7, 4, 28 - 11]
    assert sums8[1].tolist() == [4 + 2 + 4 + 2 + 3 + 4 + 5, 0 + 1 + 1 + 2 + 2 + 2 + 3] and sums8[2].tolist() == [12, 1]
    for labels in (l8, l4):
        first = [int(np.flatnonzero(labels.ravel() == k)[0]) for k in range(1, labels.max() + 1)]
        assert first == sorted(first)
    cen = cc.centroids_np(s8, sums8)
    assert cen.dtype == np.float64 and cen[2].tolist() == [6.0, 0.5]


def test_match_class_and_argument_checks():
    mask = np.array([[1, 2, 0], [2, 2, 1]], np.uint8)
    assert cc.components_np(mask, 8, 2)[0].tolist() == [[0, 1, 0], [1, 1, 0]]
    assert cc.components_np(mask, 4, 1)[0].tolist() == [[1, 0, 0], [0, 0, 2]]
    assert cc.components_np(mask, 8, -1)[0].tolist() == [[1, 1, 0], [1, 1, 1]]
    with pytest.raises(ValueError):
        cc.components_np(mask, 6)
    with pytest.raises(ValueError):
        cc.filter_components_np(mask, 1, rule="biggest")


@pytest.mark.parametrize("name", ["cc_scenes", "cc_net_masks"])
def test_numpy_filters_match_the_references_functions(name):
    g, cases = golden_cases(name)
    net = load_golden("b_c3_512x512")["mask"] if name == "cc_net_masks" else None
    for tag, H, W, which, cls, sha in cases:
        H, W, which, cls = int(H), int(W), int(which), int(cls)
        mask = cc.make_scene_mask(H, W, which) if net is None else net[which]
        assert hashlib.sha256(mask.tobytes()).hexdigest() == sha
        labels, stats, sums = cc.components_np(mask, 8, cls)
        assert len(stats) == int(g[tag + "_num"])
        assert np.array_equal(stats[:64], g[tag + "_stats"])
        assert np.array_equal(cc.centroids_np(stats, sums)[1:64], g[tag + "_centroids"][1:64])     # bitwise: one division
        for rule, kw in RULE_KW.items():
            got = cc.filter_components_np(mask, cls, rule, out_value=255, **kw)
            ref = np.unpackbits(g[f"{tag}_{rule}"])[:H * W].reshape(H, W)
            assert set(np.unique(got)) <= {0, 255}
            assert np.array_equal(got != 0, ref != 0), (tag, rule)
            if net is None:
                want = SCENE_TABLE[(H, W, which, cls)]
                assert len(stats) - 1 == want[0]
                assert int((got != 0).sum()) == want[1 + list(RULE_KW).index(rule)], (tag, rule)


def test_filter_tie_breaks_and_thresholds():
    mask = np.zeros((40, 60), np.uint8)
    mask[2:12, 30:34] = 1          # area 40, label 1
    mask[20:30, 2:6] = 1           # area 40, label 2: the tie goes to the lower label
    mask[35, 50] = 1
    labels, stats, sums = cc.components_np(mask, 8)
    assert cc.keep_largest(stats, 40).tolist() == [False, True, False, False]
    assert not cc.keep_largest(stats, 41).any()
    assert cc.keep_largest(stats, 0)[1]
    assert not cc.keep_largest(cc.components_np(np.zeros((4, 4), np.uint8))[1], 0).any()
    assert cc.keep_spatial(stats, 40, min_area=39, min_width=4, max_width=4, min_height_ratio=0.25).tolist() == [False, True, True, False]
    assert not cc.keep_spatial(stats, 40, min_area=40, min_width=4, max_width=4, min_height_ratio=0.25).any()     # area > min_area
    assert cc.keep_cable_shape(stats, sums, 60, min_area=40).tolist() == [False, True, False, False]       # label 2 is off centre
    assert cc.keep_cable_shape(stats, sums, 60, min_area=40, max_center_offset=0.5).tolist() == [False, True, False, False]
    assert cc.keep_cable_shape(stats, sums, 8, min_area=40, max_center_offset=10).tolist() == [False, False, True, False]


def test_binding_lists_the_component_symbols():
    from unet_amd import _lib
    assert {"unetpp_components_workspace_bytes", "unetpp_components", "unetpp_components_filter"} <= set(_lib.ABI_SYMBOLS)
    assert "components.h" in _lib.HEADERS
    assert _lib.CC_RULES == cc.RULES
    assert [n for n, _ in _lib.CcRule._fields_] == ["min_area", "min_width", "max_width", "min_height_ratio", "min_aspect",
                                                    "max_center_offset", "roi_width"]
    # the workspace totals where the 256-byte rounding of a part decides, and the shapes either side of a limit (no device)
    import ctypes
    lib = ctypes.CDLL(_lib.build())
    lib.unetpp_components_workspace_bytes.restype = ctypes.c_size_t
    for (b, h, w, cap), n in {(1, 1, 1, 2): 768, (1, 8, 8, 2): 768, (1, 8, 8, 8192): 8704, (1, 33, 129, 2): 17664,
                              (1, 33, 129, 8192): 25600, (16, 33, 129, 2): 273152, (1, 65535, 1, 2): 262656, (65535, 1, 1, 2): 655360,
                              (1, 512, 512, 2): 1049088, (1, 32768, 32768, 2): 4296016128, (1, 32768, 32769, 2): 0,
                              (1, 8, 8, 1): 0, (0, 8, 8, 2): 0, (65536, 1, 1, 2): 0, (1, 65536, 8, 2): 0}.items():
        assert lib.unetpp_components_workspace_bytes(b, h, w, cap) == n, (b, h, w, cap)


def test_methods_check_their_arguments_without_a_device():
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    for model in (NestedUNet(3), SimpleUNet(3)):
        with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
            model.components(np.zeros((1, 4, 4), np.uint8))
        with pytest.raises(ValueError, match="rule must be one of"):
            model.filter_components(None, 1, rule="biggest")
        with pytest.raises(ValueError, match="out_value"):
            model.filter_components(None, 1, out_value=0)
