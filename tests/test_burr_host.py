"""CPU checks of the burr-detection restatement (unet_amd/edges.py): the primitives against scipy, the properties of
Canny, the compositions against the fixtures made from the reference's own functions (tests/golden/burr_scenes.npz),
and the argument checks of the new methods that need no device.  Integer arithmetic: exact equality everywhere."""
import ctypes
import hashlib
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from unet_amd import components as cc
from unet_amd import edges as ed
from unet_amd import morphology as mo

ndimage = pytest.importorskip("scipy.ndimage")


def images():
    """Random and crafted images, the smallest sizes included."""
    r = np.random.default_rng(0)
    out = [r.integers(0, 256, hw, dtype=np.uint8) for hw in ((8, 8), (9, 17), (64, 70), (33, 129))]
    out.append(np.zeros((8, 8), np.uint8))
    out.append(np.full((9, 17), 255, np.uint8))
    chess = ((np.indices((16, 20)).sum(0) % 2) * 255).astype(np.uint8)          # the largest gradients and Laplacians
    out.append(chess)
    step = np.zeros((12, 12), np.uint8); step[:, 6:] = 255; step[0, :] = 255
    out.append(step)
    return out


# ---- 1. the primitives against scipy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ksize,sigma", [(3, 1.0), (5, 1.0), (7, 2.0)])
def test_taps_are_symmetric_sum_to_256_and_round_the_gaussian(ksize, sigma):
    t = ed.gaussian_taps(ksize, sigma)
    assert t.dtype == np.int32 and len(t) == ksize and np.array_equal(t, t[::-1]) and int(t.sum()) == 256
    x = np.arange(ksize) - ksize // 2
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    assert np.abs(t - 256.0 * g / g.sum()).max() < 1.0
    assert (t > 0).all() and t[ksize // 2] == t.max()
    assert np.array_equal(ed.check_taps(t), t)


def test_taps_of_the_reference_blur_and_default_sigma():
    assert ed.gaussian_taps(5, 1.0).tolist() == [14, 62, 104, 62, 14]           # cv2.GaussianBlur(gray, (5, 5), 1.0)
    assert ed.gaussian_taps(1, 1.0).tolist() == [256]
    assert np.array_equal(ed.gaussian_taps(5, 0), ed.gaussian_taps(5, 0.3 * (2 - 1) + 0.8))   # cv2's sigma for sigma <= 0
    for bad in (0, 4, -3):
        with pytest.raises(ValueError, match="odd and positive"):
            ed.gaussian_taps(bad, 1.0)


def test_blur_matches_scipy_correlate1d_mirror():
    for g in images():
        for ksize, sigma in ((3, 1.0), (5, 1.0), (7, 2.0)):
            t = ed.gaussian_taps(ksize, sigma).astype(np.int64)
            hor = ndimage.correlate1d(g.astype(np.int64), t, axis=1, mode="mirror")
            assert hor.max() < 65536                                           # the 16-bit intermediate holds it
            ver = ndimage.correlate1d(hor, t, axis=0, mode="mirror")
            assert np.array_equal(ed.gaussian_blur_np(g, t), ((ver + 32768) >> 16).astype(np.uint8)), (g.shape, ksize)
        assert np.array_equal(ed.gaussian_blur_np(g, [256]), g)                 # the identity tap
        skew = np.array([0, 3, 200, 50, 3])
        hor = ndimage.correlate1d(g.astype(np.int64), skew, axis=1, mode="mirror")
        ver = ndimage.correlate1d(hor, skew, axis=0, mode="mirror")
        assert np.array_equal(ed.gaussian_blur_np(g, skew), ((ver + 32768) >> 16).astype(np.uint8))
    flat = np.full((8, 8), 201, np.uint8)
    assert np.array_equal(ed.gaussian_blur_np(flat, ed.gaussian_taps(7, 2.0)), flat)   # taps summing to 256 keep a constant


def test_sobel_and_laplacian_match_scipy():
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    kl = np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]])
    for g in images():
        dx, dy = ed.sobel_np(g)
        assert np.array_equal(dx, ndimage.correlate(g.astype(np.int64), kx, mode="nearest"))
        assert np.array_equal(dy, ndimage.correlate(g.astype(np.int64), kx.T, mode="nearest"))
        lap = ndimage.correlate(g.astype(np.int64), kl, mode="mirror")
        assert np.array_equal(ed.laplacian_np(g), lap)
        assert np.array_equal(ed.laplacian_abs_u8_np(g), (np.abs(lap) % 256).astype(np.uint8))


def test_laplacian_cast_wraps_like_the_reference():
    """np.abs(lap).astype(np.uint8) of burr_detector.py:44-45 on float64 above 255."""
    g = np.zeros((9, 9), np.uint8)
    g[2, 2] = 255; g[2, 6] = 75; g[6, 2] = 64
    u = ed.laplacian_abs_u8_np(g)
    assert (int(u[2, 2]), int(u[2, 6]), int(u[6, 2])) == (252, 44, 0)          # 1020, 300, 256
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.abs(ed.laplacian_np(g).astype(np.float64)).astype(np.uint8), u)


def test_hysteresis_matches_ndimage_label_with_strong_seeds():
    for g in images():
        for low, high in ((50, 150), (200, 600), (0, 0), (1500, 1900)):
            m = ed.canny_map_np(g, low, high)
            lab, n = ndimage.label(m != 0, structure=np.ones((3, 3)))
            keep = np.zeros(n + 1, bool)
            keep[np.unique(lab[m == 2])] = True
            keep[0] = False
            assert np.array_equal(ed.canny_np(g, low, high), keep[lab] * np.uint8(255)), (g.shape, low, high)


def test_grey_is_the_identity_on_grey_pixels_and_uses_opencv4_constants():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ed.bgr_to_gray_np(np.stack([v, v, v], -1)), v)
    assert 3735 + 19235 + 9798 == 1 << 15
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 90]], np.uint8)  # B, G, R
    assert ed.bgr_to_gray_np(px).tolist() == [29, 150, 76, (3735 * 10 + 19235 * 200 + 9798 * 90 + 16384) >> 15]
    with pytest.raises(ValueError):
        ed.bgr_to_gray_np(np.zeros((4, 4), np.uint8))


# ---- 2. properties of Canny ---------------------------------------------------------------------------------------------
def test_canny_output_lies_in_the_candidates_and_every_component_holds_a_seed():
    for g in images():
        dx, dy = ed.sobel_np(g)
        mag = np.abs(dx) + np.abs(dy)
        for low, high in ((50, 150), (200, 600)):
            out = ed.canny_np(g, low, high)
            assert set(np.unique(out)) <= {0, 255}
            assert not (out[mag <= low] != 0).any()
            lab, n = ndimage.label(out != 0, structure=np.ones((3, 3)))
            for l in range(1, n + 1):
                assert (mag[lab == l] > high).any()
            assert np.array_equal(out, ed.canny_np(g, high, low))                # low > high swaps
            assert np.array_equal(out, ed.canny_np(g, low + 0.9, high + 0.9))    # thresholds are floored


def test_thresholds_are_strict():
    g = np.full((12, 12), 100, np.uint8)
    g[:, 6:] = 120                                                               # |dx| = 80 along the step
    dx, dy = ed.sobel_np(g)
    assert (np.abs(dx) + np.abs(dy)).max() == 80
    assert (ed.canny_map_np(g, 79, 1000) == 1).sum() == 12                       # one column of candidates
    assert not ed.canny_map_np(g, 80, 1000).any()                                # m == low is not a candidate
    assert (ed.canny_map_np(g, 10, 80) == 2).sum() == 0                          # m == high is not a seed
    assert (ed.canny_map_np(g, 10, 79) == 2).sum() == 12
    assert not ed.canny_np(g, 10, 80).any() and (ed.canny_np(g, 10, 79) != 0).sum() == 12


def test_plateau_picks_one_side_only():
    """A step gives two equal magnitudes side by side: `>` towards the left / upper neighbour, `>=` towards the other."""
    g = np.full((12, 12), 100, np.uint8)
    g[:, 6:] = 120
    m = ed.canny_map_np(g, 50, 1000)
    assert np.array_equal(np.nonzero(m.any(0))[0], [5])                          # columns 5 and 6 tie: the left one wins
    m = ed.canny_map_np(np.ascontiguousarray(g.T), 50, 1000)
    assert np.array_equal(np.nonzero(m.any(1))[0], [5])                          # rows 5 and 6 tie: the upper one wins


def test_direction_cases_reach_every_branch():
    frames = ed.make_direction_cases()
    assert frames.shape == (16, 40, 40)
    seen = np.zeros(4, np.int64)
    for f in frames:
        c = ed.canny_map_np(f, 50, 150) != 0
        dx, dy = ed.sobel_np(f)
        x, y = np.abs(dx), np.abs(dy) << 15
        hz = y < x * ed.TG22
        vt = ~hz & (y > x * ed.TG22 + (x << 16))
        neg = (dx ^ dy) < 0
        seen += [(c & hz).sum(), (c & vt).sum(), (c & ~hz & ~vt & ~neg).sum(), (c & ~hz & ~vt & neg).sum()]
    assert seen.min() >= 100, seen
    assert ed.TG22 == int(math.tan(math.radians(22.5)) * (1 << 15) + 0.5)


def test_hysteresis_adversaries_are_what_they_claim():
    th, tw = 32, 128
    adv = ed.make_hysteresis_adversaries(th, tw)
    seeded, unseeded = ed.canny_map_np(adv["serpentine_seeded"], 50, 150), ed.canny_map_np(adv["serpentine_unseeded"], 50, 150)
    assert len(cc.components_np(seeded, 8, -1)[1]) == 2 and 1 <= (seeded == 2).sum() <= 16 and not (unseeded == 2).any()
    ys, xs = np.nonzero(ed.hysteresis_np(seeded))
    assert len(set(zip((ys // th).tolist(), (xs // tw).tolist()))) >= 6 and len(ys) == (seeded != 0).sum() > 3000
    assert (unseeded != 0).sum() > 3000 and not ed.hysteresis_np(unseeded).any()
    pair = ed.canny_map_np(adv["diagonal_pair"], 50, 150)
    labels, stats, _ = cc.components_np(pair, 8, -1)
    assert len(stats) == 3 and pair[th - 2, tw - 2] and pair[th, tw] and not pair[th - 1, tw - 1]
    assert np.array_equal(ed.hysteresis_np(pair) != 0, labels == labels[th - 2, tw - 2])
    assert len(cc.components_np(pair, 4, -1)[1]) > 3                             # the chains need connectivity 8


# ---- 3. the box rule and the program -------------------------------------------------------------------------------------
def test_keep_box_clauses():
    stats = np.array([[0, 0, 9, 9, 0], [0, 0, 5, 6, 30], [0, 0, 5, 6, 29], [0, 0, 28, 29, 800], [0, 0, 28, 29, 801], [0, 0, 7, 34, 200],
                      [0, 0, 7, 35, 200], [0, 0, 36, 7, 200], [0, 0, 3, 12, 36], [0, 0, 12, 3, 36], [0, 0, 4, 12, 40]], np.int32)
    assert ed.keep_box(stats, 30, 800, 5.0, 3).tolist() == [False, True, False, True, False, True, True, False, False, False, True]
    # 35 / (7 + 1e-6) < 5: the reference's 1e-6 lets the exact ratio 5 pass; 36 / 7 does not
    assert 35 / (7 + 1e-6) < 5.0 < 36 / (7 + 1e-6)
    assert ed.keep_box(stats, 1, 10 ** 9, math.inf, 0)[1:].all() and not ed.keep_box(stats, 0, 0)[0]


def test_program_burr_fits_the_morphology_limits():
    el, steps, res = ed.program_burr()
    assert len(steps) == 7 <= mo.MAX_STEPS and len(el) == 3 <= mo.MAX_ELEMENTS and res == 2
    assert [e.shape for e in el] == [(8, 8), (3, 3), (2, 2)]
    mo.check_program(el, steps, res)
    assert [s[0] for s in steps] == ["dilate", "andnot", "and", "dilate", "erode", "erode", "dilate"]
    # step by step against the primitives, on a scene
    grey, cable = ed.make_burr_scene(96, 200, 2)
    edges = ed.canny_np(ed.gaussian_blur_np(grey, ed.gaussian_taps(5, 1.0)), 50, 150)
    band = mo.dilate_np(cable, el[0]) & ~(cable != 0)
    x = (edges != 0) & band
    x = mo.erode_np(mo.dilate_np(x, el[1]), el[1])
    x = mo.dilate_np(mo.erode_np(x, el[2]), el[2])
    assert np.array_equal(mo.run_program_np(edges, cable, el, steps, -1, -1, res, 1), x.astype(np.uint8)) and x.any()


# ---- 4. the compositions against the fixtures from the reference's own functions --------------------------------------------
def test_compositions_equal_every_fixture_case():
    g = load_golden("burr_scenes")
    kinds = {}
    scenes = {}
    for tag, kind, H, W, seed, param, sha in (tuple(r) for r in g["cases"].tolist()):
        H, W, seed = int(H), int(W), int(seed)
        ref = np.unpackbits(g[tag + "_out"])[:H * W].reshape(H, W)
        kinds[kind] = kinds.get(kind, 0) + 1
        if kind == "crafted":
            edges, cable = ed.make_crafted_burr_case()
            assert edges.shape == (H, W) and sha == hashlib.sha256(np.stack([edges, cable]).tobytes()).hexdigest()
            p = ed.PRESETS[param]
            got = ed.burrs_from_edges_np(edges, cable, min_area=p["min_area"], max_area=p["max_area"])
            assert np.array_equal(got, ref), tag
            continue
        if (H, W, seed) not in scenes:
            scenes[(H, W, seed)] = ed.make_burr_scene(H, W, seed)
        grey, cable = scenes[(H, W, seed)]
        assert sha == hashlib.sha256(np.stack([grey, cable]).tobytes()).hexdigest(), tag
        if kind == "detect":
            p = ed.PRESETS[param]
            got = ed.detect_burrs_np(grey, cable, min_area=p["min_area"], max_area=p["max_area"])
            assert got.max() == 1 and np.array_equal(got, ref), tag
            assert cc.components_np(got, 8, -1)[1].shape[0] - 1 >= 5             # what the generator asserted
        else:
            got = ed.burr_mask_rulebased_np(grey, cable * np.uint8(int(param)))
            assert got.max() == 255 and np.array_equal(got != 0, ref != 0), tag
    assert kinds == {"detect": 9, "rulebased": 6, "crafted": 2}
    # the three presets give three different masks per scene
    for H, W, seed in scenes:
        outs = [g[f"detect_{name}_{H}x{W}_{seed}_out"] for name in ed.PRESETS]
        assert not any(np.array_equal(outs[i], outs[j]) for i in range(3) for j in range(i))


def test_empty_cable_gives_empty_results():
    grey, cable = ed.make_burr_scene(96, 200, 2)
    zero = np.zeros_like(cable)
    assert not ed.detect_burrs_np(grey, zero).any() and not ed.burr_mask_rulebased_np(grey, zero).any()
    assert ed.detect_burrs_np(grey, cable).any()
    assert np.array_equal(ed.detect_burrs_np(grey, cable * np.uint8(5), 5), ed.detect_burrs_np(grey, cable))
    assert ed.detect_burrs_np(grey, cable, out_value=200).max() == 200


def test_presets_are_the_reference_table():
    assert {k: (v["min_area"], v["max_area"]) for k, v in ed.PRESETS.items()} == {"low": (50, 800), "medium": (30, 800), "high": (20, 1000)}


# ---- 5. binding and argument checks ----------------------------------------------------------------------------------------
def test_binding_lists_the_burr_symbols():
    from unet_amd import _lib
    new = {"unetpp_gray_u8", "unetpp_gaussian_blur_u8", "unetpp_canny_workspace_bytes", "unetpp_canny_layout", "unetpp_canny_u8",
           "unetpp_laplacian_band_u8", "unetpp_components_filter_box"}
    assert new <= set(_lib.ABI_SYMBOLS) and "edges.h" in _lib.HEADERS
    assert [n for n, _ in _lib.CcBoxRule._fields_] == ["min_area", "max_area", "max_aspect", "min_side"]
    assert [n for n, _ in _lib.CcRule._fields_] == ["min_area", "min_width", "max_width", "min_height_ratio", "min_aspect",
                                                    "max_center_offset", "roi_width"]          # unetpp_cc_rule keeps its layout
    header = open(os.path.join(ROOT, "include", "unetpp.h")).read()
    box = re.search(r"typedef struct unetpp_cc_box_rule \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"double (\w+);", box) == ["min_area", "max_area", "max_aspect", "min_side"]


def test_layout_and_workspace_queries_without_a_device():
    from unet_amd import _lib
    lib = ctypes.CDLL(_lib.build())
    lib.unetpp_canny_workspace_bytes.restype = ctypes.c_size_t
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.unetpp_canny_layout(448, 800, ctypes.byref(rows), ctypes.byref(cols)) == 0
    assert rows.value >= 8 and cols.value % 16 == 0 and cols.value >= 16
    assert lib.unetpp_canny_layout(7, 800, ctypes.byref(rows), ctypes.byref(cols)) == -2
    assert lib.unetpp_canny_layout(448, 800, None, ctypes.byref(cols)) == -1
    for b, h, w in ((1, 8, 8), (16, 512, 512), (32, 448, 800), (1, 1080, 1920), (2, 9, 17)):
        n = lib.unetpp_canny_workspace_bytes(b, h, w)
        assert 6 * b * h * w <= n <= 6 * b * h * w + 4 * b * (h * w // 4096 + 1) + 4 * 256      # parent + map + flags (+ chunk counts)
    for b, h, w in ((0, 64, 64), (1, 7, 64), (1, 64, 7), (1, 65536, 8), (1, 40000, 40000)):
        assert lib.unetpp_canny_workspace_bytes(b, h, w) == 0
    # the totals where the 256-byte rounding of a part decides, and the shapes either side of a limit
    for (b, h, w), n in {(1, 8, 8): 1024, (1, 9, 9): 1280, (1, 33, 129): 26112, (16, 33, 129): 409600, (1, 512, 512): 1573120,
                         (1, 32768, 32768): 6443499520, (1, 32768, 32769): 0, (1, 8, 7): 0, (1, 7, 800): 0, (1, 65535, 1): 0,
                         (65536, 8, 8): 0}.items():
        assert lib.unetpp_canny_workspace_bytes(b, h, w) == n, (b, h, w)
    lib.unetpp_edges_union_workspace_bytes.restype = ctypes.c_size_t
    assert [lib.unetpp_edges_union_workspace_bytes(b) for b in (0, 1, 64, 65, 65535, 65536)] == [0, 256, 256, 512, 262144, 0]


def test_methods_check_their_arguments_without_a_device():
    import torch
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    small = torch.zeros((1, 7, 40), dtype=torch.uint8)
    for model in (NestedUNet(3), SimpleUNet(3)):
        with pytest.raises(ValueError, match="sum to 256"):
            model.gaussian_blur(None, taps=[14, 62, 104, 62, 15])
        with pytest.raises(ValueError, match="odd and positive"):
            model.gaussian_blur(None, ksize=4)
        with pytest.raises(ValueError, match="at most 7"):
            model.canny(None, 50, 150, blur=(9, 2.0))
        with pytest.raises(ValueError, match="at most 7"):
            model.detect_burrs(None, None, blur_ksize=9)
        with pytest.raises(ValueError, match="non-negative"):
            model.canny(None, -1, 150)
        with pytest.raises(ValueError, match="non-negative"):
            model.canny(None, 50, float("nan"))
        with pytest.raises(ValueError, match="8 <= H, W"):
            model.canny(small, 50, 150)
        with pytest.raises(ValueError, match="8 <= H, W"):
            model.gaussian_blur(small)
        with pytest.raises(ValueError, match="8 <= H, W"):
            model.detect_burrs(small, small)
        with pytest.raises(ValueError, match="out_value"):
            model.detect_burrs(None, None, out_value=0)
        with pytest.raises(ValueError, match="out_value"):
            model.burr_mask_rulebased(None, None, out_value=256)
        with pytest.raises(ValueError, match="NaN"):
            model.filter_components_box(None, min_area=float("nan"))
        with pytest.raises(ValueError, match="NaN"):
            model.detect_burrs(None, None, max_aspect=float("nan"))
        with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
            model.canny(np.zeros((1, 16, 16), np.uint8), 50, 150)                 # a host array
        with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
            model.bgr_to_gray(np.zeros((1, 16, 16, 3), np.uint8))
        with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
            model.burr_mask_rulebased(np.zeros((1, 16, 16), np.uint8), np.zeros((1, 16, 16), np.uint8))
        with pytest.raises(RuntimeError, match="differ in shape"):
            model.detect_burrs(np.zeros((1, 16, 16), np.uint8), np.zeros((1, 16, 17), np.uint8))
