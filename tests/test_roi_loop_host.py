"""The NumPy forms of the ROI and full-frame 3-class loops (unet_amd/roi_loop.py) against the reference's own results
(tests/golden/roi_scenes.npz, scripts/make_golden_roi.py), what is particular to include/unetpp_roi.h, and the argument checks
that need no device.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from unet_amd import _lib
from unet_amd import components as cc
from unet_amd import edges as ed
from unet_amd import roi_loop as rl



@pytest.fixture(scope="module")
def golden():
    g = load_golden("roi_scenes")
    return {k: g[k] for k in g.files}


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------
def test_fixture_facts(golden):
    """Everything the generator asserted, again: inputs by SHA-256, the input conditions, every _np form == the reference
    (the threshold table within the recorded distance), every branch met."""
    facts = rl.fixture_facts(golden)
    assert facts["threshold_ulps"] <= int(golden["threshold_ulps"])
    with open(os.path.join(ROOT, "tests", "golden", "README_roi.txt")) as f:
        assert f"Largest distance of the two threshold tables: {int(golden['threshold_ulps'])} float32 ulps" in f.read()


@pytest.mark.parametrize("W", [1, 5, 20, 29, 30, 31, 96, 640])
def test_box_sums_are_np_convolve_same(W):
    """The offset of the window-30 box sum, pinned on np.convolve(..., mode='same') itself, W < 30 included (its result then
    has 30 entries)."""
    c = np.random.default_rng(W).integers(0, 200, W)
    want = np.convolve(c, np.ones(rl.BOX), mode="same")
    got = rl.box_sums_np(c)
    assert got.shape == want.shape == (max(W, 30),) and np.array_equal(got, want.astype(np.int64))


@pytest.mark.parametrize("name,kind,H,W,seed", rl.PROJECTION_SCENES)
def test_projection_decision_is_the_float_comparison(golden, name, kind, H, W, seed):
    """10 S_i > 3 S_max selects the columns of the reference's smooth > 0.3 * max on these frames (no column is a tie)."""
    edges = ed.canny_np(ed.bgr_to_gray_np(rl.make_projection_frame(H, W, seed, kind)[None])[0], 50, 150)
    assert rl.roi_condition_np(edges)
    smooth = np.convolve(np.sum(edges, axis=0), np.ones(30) / 30, mode="same")
    s = rl.box_sums_np(np.count_nonzero(edges, axis=0))
    assert np.array_equal(smooth > np.max(smooth) * 0.3, 10 * s > 3 * s.max())
    roi = rl.roi_from_edges_np(edges)
    assert np.array_equal(roi, rl.detect_roi_np(rl.make_projection_frame(H, W, seed, kind)))
    assert roi[3] == (roi[1] > roi[0]) and 0 <= roi[0] and roi[1] <= W


def test_threshold_table_against_the_reference(golden):
    bar = int(golden["threshold_ulps"]) + 1
    for name, S, seed, cable, tape, b in rl.PROB_SCENES:
        thr, means, maxima = rl.adaptive_thresholds_np(rl.make_probs(S, S, seed, cable, tape, b))
        assert thr.tobytes() == golden[f"{name}_thr_np"].tobytes()
        assert rl.ulp_distance(thr, golden[f"{name}_thr_ref"]) <= bar, name
        assert (means > 0).all() and (maxima <= 1).all() and (maxima >= means).all()


def test_q32_and_the_mean():
    p = np.float32([0.0, -1.0, np.nan, 1.0, 2.0, 0.5, 2.0 ** -33, 1 - 2.0 ** -24])
    assert rl.q32_np(p).tolist() == [0, 0, 0, 2 ** 32, 2 ** 32, 2 ** 31, 0, 2 ** 32 - 256]
    probs = np.full((3, 4, 4), 0.25, np.float32)
    thr, means, maxima = rl.adaptive_thresholds_np(probs)
    assert means.tolist() == [0.25] * 3 and maxima.tolist() == [0.25] * 3
    assert thr.tolist() == [np.float32(0.5), np.float32(0.75), np.float32(0.75)]


def test_ultra_strict_rule_by_rule():
    #          bg    cable tape
    px = [(0.1, 0.8, 0.1),     # cable
          (0.1, 0.1, 0.8),     # tape
          (0.4, 0.4, 0.2),     # the first maximum is the background
          (0.1, 0.45, 0.45),   # cable before tape
          (0.3, 0.59, 0.11),   # cable > 2 bg fails (0.59 < 0.6)
          (0.25, 0.55, 0.2),   # cable >= bg + margin fails with margin 0.35
          (0.1, 0.49, 0.41)]   # below t_cable
    p = np.float32(px).T.reshape(3, 1, len(px)).copy()
    c, t = rl.ultra_strict_np(p, np.float32([0.45, 0.5, 0.35]))
    assert c[0].tolist() == [1, 0, 0, 1, 0, 0, 1] and t[0].tolist() == [0, 1, 0, 0, 0, 0, 0]
    c, t = rl.ultra_strict_np(p, np.float32([0.5, 0.5, 0.2]))
    assert c[0].tolist() == [1, 0, 0, 0, 0, 1, 0]


def test_component_rules_trace():
    m = rl.make_component_scene()
    labels, stats, sums = cc.components_np(m, 8, -1)
    keep, why = rl.geometry_keep(stats, sums, m.shape[1], return_trace=True)
    assert sorted(v for v in why.values() if v) == ["area", "area", "aspect", "edge"] and keep.sum() == 2
    best, scores = rl.primary_label(stats, sums, m.shape[1], return_trace=True)
    assert best == 2 and len(scores) == 3
    # every constant is a parameter
    assert rl.geometry_keep(stats, sums, m.shape[1], min_area=1).sum() == 4 and rl.geometry_keep(stats, sums, m.shape[1], large_area=1e9).sum() == 1
    assert rl.primary_label(stats, sums, m.shape[1], min_aspect=100.0) == -1
    assert not rl.refine_by_geometry_np(np.zeros((8, 8), np.uint8)).any() and not rl.select_primary_np(np.zeros((8, 8), np.uint8)).any()


def test_keep_largest_cc_is_the_largest_rule():
    """keep_largest_cc(mask, min_area) of infer_video_3class_full.py restated, against filter_components_np(rule='largest')."""
    def keep_largest_cc(mask, min_area):
        labels, stats, _ = cc.components_np(mask, 8, -1)
        areas = stats[1:, cc.CC_STAT_AREA]
        if len(stats) <= 1:
            return mask
        if len(areas) == 0 or np.max(areas) < min_area:
            return np.zeros_like(mask)
        return (labels == np.argmax(areas) + 1).astype(np.uint8)

    for kind in ("all", "ties"):
        m = rl.make_component_scene(kind=kind)
        for min_area in (0, 500, 4720, 4721, 11340, 11341, 10 ** 6):
            assert np.array_equal(keep_largest_cc(m, min_area), cc.filter_components_np(m, -1, "largest", 8, 1, min_area=min_area)), (kind, min_area)
    z = np.zeros((16, 16), np.uint8)
    assert np.array_equal(keep_largest_cc(z, 500), cc.filter_components_np(z, -1, "largest", 8, 1, min_area=500))


def test_crop_and_paste_forms():
    f = np.random.default_rng(0).integers(0, 256, (20, 40, 3), dtype=np.uint8)
    assert np.array_equal(rl.crop_resize_np(f, (0, 40, 0, 1), (20, 40)), f)                    # equal size: the identity
    assert not rl.crop_resize_np(f, (7, 7, 1, 0), 16).any() and rl.crop_resize_np(f, (7, 8, 1, 1), 16).shape == (16, 16, 3)
    m = (f[:, :, 0] > 128).astype(np.uint8)
    assert np.array_equal(rl.paste_mask_np(m, (0, 40, 0, 1), (20, 40)), m)
    out = rl.paste_mask_np(m, (10, 25, 1, 1), (30, 50))
    assert not out[:, :10].any() and not out[:, 25:].any() and out.shape == (30, 50)
    assert not rl.paste_mask_np(m, (10, 10, 1, 0), (30, 50)).any()


# ---- the header's entries (names, types, build inputs and guard coverage: tests/test_bindings_host.py) --------------------------------
def test_workspace_sizes():
    lib = _lib.load()
    assert lib.unetpp_roi_projection_workspace_bytes(2, 100) >= 800 and lib.unetpp_roi_projection_workspace_bytes(0, 100) == 0
    assert lib.unetpp_roi_stats_workspace_bytes(4) >= 4 * 3 * 12 and lib.unetpp_roi_stats_workspace_bytes(0) == 0


def test_header_is_c99(tmp_path):
    cc_ = shutil.which("cc") or shutil.which("gcc")
    assert cc_, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "unetpp_roi.h"\nint main(void) { unetpp_roi_cc_rule r = {0}; (void)r; return UNETPP_ROI_RULE_PRIMARY - 1; }\n')
    subprocess.run([cc_, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True, text=True)


def test_null_engine_is_refused():
    lib = _lib.load()
    assert lib.unetpp_roi_from_edges_u8(None, None, 1, 8, 8, None, None, None) == -1
    assert lib.unetpp_roi_paste_masks_u8(None, None, None, 1, 8, 8, None, None, None, 8, 8, None) == -1


# ---- argument checks that need no device --------------------------------------------------------------------------------------------
class _NoDevice:
    """Stands in for the model: the checks under test run before anything reaches the device."""

    def _input(self, t, what="gray", shape="[B,H,W]", dtype="uint8"):
        raise RuntimeError(f"{what} must be a {dtype} CUDA tensor {shape}")

    @staticmethod
    def _check_out_value(v):
        if not 1 <= int(v) <= 255:
            raise ValueError("out_value")
        return int(v)


def test_argument_checks():
    import torch
    m = _NoDevice()
    with pytest.raises(ValueError, match="at least 3 classes"):
        rl.adaptive_thresholds(m, torch.zeros((1, 2, 8, 8)))
    with pytest.raises(ValueError, match="at least 3 classes"):
        rl.ultra_strict(m, torch.zeros((1, 2, 8, 8)), torch.zeros((1, 3)))
    with pytest.raises(RuntimeError, match="float32 CUDA tensor"):
        rl.adaptive_thresholds(m, torch.zeros((1, 3, 8, 8), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
        rl.roi_from_edges(m, torch.zeros((1, 8, 8), dtype=torch.float32))
    with pytest.raises(RuntimeError, match=r"\[B,H,W,C\]"):
        rl.crop_resize(m, torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="NaN"):
        rl.refine_by_geometry(m, torch.zeros((1, 8, 8), dtype=torch.uint8), min_area=float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        rl.select_primary(m, torch.zeros((1, 8, 8), dtype=torch.uint8), min_aspect=float("nan"))
    with pytest.raises(ValueError, match="out_value"):
        rl.refine_by_geometry(m, torch.zeros((1, 8, 8), dtype=torch.uint8), out_value=0)
    for bad in (np.zeros((3, 8), np.float32), np.zeros((2, 8, 8), np.float32), np.zeros((3, 8, 8), np.float64)):
        with pytest.raises(ValueError):
            rl.adaptive_thresholds_np(bad)
        with pytest.raises(ValueError):
            rl.ultra_strict_np(bad, np.float32([0.5, 0.5, 0.2]))
    with pytest.raises(ValueError):
        rl.roi_from_edges_np(np.zeros((2, 8, 8), np.uint8))
    with pytest.raises(ValueError):
        rl.crop_resize_np(np.zeros((8, 8), np.uint8), (0, 8, 0, 1))
