"""Host tests of unet_amd/simple_loops.py: every NumPy form against the reference's own results (tests/golden/
simple_loops_scenes.npz, written by scripts/make_golden_simple_loops.py) with ==, the argument checks, and what is particular to
include/unetpp_simple_loops.h.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from unet_amd import _lib
from unet_amd import components as cc
from unet_amd import multiclass as mc
from unet_amd import simple_loops as sl


@pytest.fixture(scope="module")
def golden():
    g = load_golden("simple_loops_scenes")
    return {k: g[k] for k in g.files}


def probs_of(row):
    name, b, c, h, w, seed, specials = row
    return name, sl.make_probs(b, c, h, w, seed, specials)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
def test_fixture_facts(golden):
    facts = sl.fixture_facts(golden)
    assert facts["overlap_pixels"] == 3 and facts["backup_tape_overwritten"] > 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "simple_loops_scenes.npz")) < 64 * 1024


@pytest.mark.parametrize("row", sl.FIXTURE_PROBS, ids=[r[0] for r in sl.FIXTURE_PROBS])
def test_pixel_rules_against_the_reference(golden, row):
    name, p = probs_of(row)
    assert sl.sha(p) == str(golden[name + "_sha"])
    shape = (p.shape[0],) + p.shape[2:]
    nhwc = np.ascontiguousarray(p.transpose(0, 2, 3, 1))
    for tag, fn in (("rel", sl.relative_threshold_np), ("conf", lambda x, **kw: sl.confidence_threshold_np(x, 0.3, **kw))):
        for probs, kw in ((p, {}), (nhwc, {"layout": "nhwc"})):
            c, t = fn(probs, **kw)
            assert c.dtype == np.uint8 and t.dtype == np.uint8
            assert (c == sl.unbits(golden[f"{name}_{tag}_cable"], shape)).all() and (t == sl.unbits(golden[f"{name}_{tag}_tape"], shape)).all()


def test_nan_and_infinity_follow_numpy():
    """What the module docstring promises, stated on single pixels: the first NaN wins the argmax, a comparison with a NaN is false."""
    nan, inf = np.nan, np.inf
    px = lambda *v: np.array(v, np.float32).reshape(1, 3, 1, 1)
    conf = lambda *v: tuple(int(m[0, 0, 0]) for m in sl.confidence_threshold_np(px(*v), 0.3))
    rel = lambda *v: tuple(int(m[0, 0, 0]) for m in sl.relative_threshold_np(px(*v)))
    assert conf(nan, 0.9, 0.1) == (0, 0) and conf(0.1, nan, 0.9) == (0, 0) and conf(0.1, 0.5, nan) == (0, 0)
    assert conf(0.1, nan, nan) == (0, 0) and conf(0.1, inf, inf) == (1, 0) and conf(-inf, 0.4, 0.4) == (1, 0)
    assert conf(0.5, 0.5, 0.5) == (0, 0) and conf(0.2, 0.4, 0.4) == (1, 0) and conf(0.2, 0.3, 0.5) == (0, 1)
    assert rel(nan, 0.9, 0.9) == (0, 0) and rel(0.1, nan, 0.9) == (0, 1) and rel(0.1, 0.9, nan) == (1, 0)
    assert rel(-inf, 0.2, 0.3) == (0, 1) and rel(0.0, 0.0, 0.0) == (0, 0) and rel(0.1, inf, inf) == (1, 0)
    assert rel(0.1, 0.45, 0.45) == (1, 0) and rel(0.1, 0.4, 0.5) == (0, 1) and rel(0.1, 0.5, 0.4) == (1, 0)


def test_ratios_are_rounded_to_float32():
    """bg * ratio is a float32 product of the ratio rounded to float32: a pixel exactly on that product is not above it."""
    bg = np.float32(0.3)
    edge = bg * np.float32(2.1)
    p = np.array([bg, edge, 0], np.float32).reshape(1, 3, 1, 1)
    assert sl.relative_threshold_np(p, 2.1)[0][0, 0, 0] == 0
    p[0, 1] = np.nextafter(edge, np.float32(1))
    assert sl.relative_threshold_np(p, 2.1)[0][0, 0, 0] == 1


def test_band_against_the_reference(golden):
    for key in (k for k in golden if k.startswith("band_")):
        h, w = (int(v) for v in key[5:].split("x"))
        ones = np.full((2, h, w), 255, np.uint8)
        assert (sl.column_band_np(ones) == sl.unbits(golden[key], (h, w))[None]).all(), key
    assert sl.band_columns(512) == (128, 384) and sl.band_columns(23) == (5, 17) and sl.band_columns(3) == (0, 2)


def test_tape_filter_against_the_reference(golden):
    for kind in sl.TAPE_SCENES:
        tape, cable = sl.make_tape_scene(kind)
        out, table = sl.tape_position_filter_np(tape[None], cable[None])
        assert (out[0] == sl.unbits(golden[f"tape_{kind}_out"], tape.shape)).all(), kind
        assert table.dtype == np.int32 and table[0].tolist() == golden[f"tape_{kind}_table"].tolist(), kind


def test_tape_filter_areas_are_sums_of_values():
    """The reference's np.sum(mask) and `tape & valid` on masks that are not 0/1: values add up, the AND keeps bit 0."""
    tape, cable = sl.make_tape_scene("filtered")
    out, table = sl.tape_position_filter_np((tape * 3)[None], (cable * 200)[None])
    ref, ref_table = sl.tape_position_filter_np(tape[None], cable[None])
    assert table[0, 2] == 3 * ref_table[0, 2] and table[0, 3] == ref_table[0, 3] and table[0, 4] == 0      # 2 f < 3 o: back unchanged
    assert (out[0] == tape * 3).all()
    out, table = sl.tape_position_filter_np((tape * 255)[None], cable[None])
    assert table[0, 4] == 0 and table[0, 2] == 255 * ref_table[0, 2]


def test_valid_ranges():
    assert sl.valid_ranges(36, 59, 96) == (25, 43, 52, 70)
    assert sl.valid_ranges(0, 95, 96) == (0, 31, 64, 96)                 # clamped on both sides
    assert sl.valid_ranges(32, 32, 96) == (32, 32, 32, 32)               # cw = 0: both empty
    assert sl.valid_ranges(10, 11, 96) == (10, 10, 11, 11)               # cw = 1: 1 // 2 = 0, 2 // 3 = 0


def test_components_against_the_reference(golden):
    scene = sl.make_component_scene()
    for name, lo, hi, wd in sl.FIXTURE_COMPONENTS:
        out = sl.keep_components_np(scene[None], lo, hi, wd)
        assert (out[0] == sl.unbits(golden["components_" + name], scene.shape)).all(), name
    # the bounds are inclusive on every side, and floats bound integers as they compare
    assert sl.keep_components_np(scene[None], 99.5, 100.5)[0].sum() == 100
    assert sl.keep_components_np(scene[None], 100, 100)[0].sum() == 100 and sl.keep_components_np(scene[None], 101, 479)[0].sum() == 0
    assert sl.keep_components_np(scene[None], 1, None, 40)[0].sum() == 480 + 800 and sl.keep_components_np(scene[None], 1, None, 41)[0].sum() == 0
    two = (scene * 2)[None]
    assert (sl.keep_components_np(two, 100, match_class=2, out_value=7) == 7 * sl.keep_components_np(scene[None], 100)).all()
    assert sl.keep_components_np(two, 100, match_class=1).sum() == 0
    assert sl.component_bounds(0.5, None, 19.2) == (1, sl.INT_MAX, 20) and sl.component_bounds(3, 1e30, 0) == (3, sl.INT_MAX, 0)


def test_loops_against_the_reference(golden):
    name, p = probs_of(sl.FIXTURE_LOOP_PROBS)
    assert sl.sha(p) == str(golden[name + "_sha"])
    fh, fw = sl.FIXTURE_LOOP_FRAME
    full = (p.shape[0], fh, fw)
    cable, tape, metrics = sl.postprocess_spatial_np(p, (fh, fw))
    assert (cable == sl.unbits(golden["spatial_cable"], full)).all() and (tape == sl.unbits(golden["spatial_tape"], full)).all()
    assert [[m["cable_coverage"], m["tape_coverage"]] for m in metrics] == golden["spatial_coverage"].tolist()
    c, t = sl.confidence_threshold_np(p, 0.3)
    cable, tape, metrics, pred = sl.measured_tail_np(c, t, (fh, fw))
    assert (cable == sl.unbits(golden["confidence_cable"], full)).all() and (tape == sl.unbits(golden["confidence_tape"], full)).all()
    assert [[m[f] for f in ("dc_px", "dt_px", "delta_d_px", "cable_coverage", "tape_coverage")] for m in metrics] == golden["confidence_metrics"].tolist()
    assert (pred == golden["confidence_pred"]).all()
    scene = sl.make_component_scene()
    cable, tape, metrics, pred = sl.postprocess_fixed_np(scene[None], np.ascontiguousarray(scene[:, ::-1])[None], (fh, fw), 480, 100, 100000, 600)
    assert (cable[0] == sl.unbits(golden["fixed_cable"], (fh, fw))).all() and (tape[0] == sl.unbits(golden["fixed_tape"], (fh, fw))).all()
    assert [metrics[0][f] for f in ("dc_px", "dt_px", "delta_d_px", "cable_coverage", "tape_coverage")] == golden["fixed_metrics"].tolist()
    assert (pred[0] == golden["fixed_pred"]).all() and {1, 2} <= set(np.unique(pred).tolist())


def test_predict_against_the_reference(golden):
    planes = sl.make_simple_batch()
    assert sl.sha(planes) == str(golden["planes_sha"])
    for variant in ("simple", "optimized"):
        out, table, tape_table = sl.predict_simple_np(planes, sl.FIXTURE_FRAME, variant, return_tape_table=True)
        assert out.dtype == np.uint8 and (out == golden[f"predict_{variant}_map"]).all(), variant
        assert (table == mc.class_table_np(golden[f"predict_{variant}_map"])).all()
        if variant == "optimized":
            assert tape_table.tolist() == golden["predict_optimized_tape_table"].tolist()
        else:
            assert tape_table is None
    bm = sl.make_backup_map()
    out, table = sl.predict_simple_backup_np(bm[None])
    assert (out[0] == golden["backup_map"]).all() and (table == mc.class_table_np(golden["backup_map"][None])).all()
    # merge_classes cuts every plane from the input map and so keeps the swallowed tape: the reason for the two launches
    merged = mc.merge_classes_np(bm[None], (((range(1, 256)), (), -1), ((1,), (("close", 3),), 1), ((2,), (("close", 3),), 2)), want_table=False)
    assert (merged[0] != out[0]).any()


def test_scaled_tape_constants_reach_the_other_branches():
    """At the scaled-down constants of the device tests the tape survives in both verdicts and a burr is dropped by area."""
    planes = sl.make_simple_batch()
    out, _, tape_table = sl.predict_simple_np(planes, sl.FIXTURE_FRAME, "optimized", return_tape_table=True, **sl.SCALED_TAPE)
    assert tape_table[:, 4].tolist() == [1, 0, 0, 0] and (out[0] == 2).any() and (out[1] == 2).any()
    big = sl.predict_simple_np(planes, sl.FIXTURE_FRAME, "optimized", want_table=False, min_tape_area=5000)
    assert not (big == 2).any()


def test_threshold_classes_bits_2_to_4_are_plain_thresholds():
    """threshold_planes reuses unetpp_threshold_classes_f32: in its NumPy form, bits 2..4 of planes (k, k, k, k, k) are `resized
    plane k >= threshold`, and bits 0 and 1 stay clear for the arguments threshold_planes passes (one plane twice, threshold and
    ratio +inf), NaN and infinities included."""
    p = sl.make_random_probs(2, 7, 17, 23, 5, specials=True)
    for frame_hw in ((17, 23), (40, 31)):
        for thr in (0.3, 0.55, 0.7):
            want = sl.threshold_planes_np(p, frame_hw, (thr, thr, thr))
            for k, bit in zip(sl.PLANE_CHANNELS, (sl.BIT_CABLE, sl.BIT_TAPE, sl.BIT_BURR)):
                got = mc.threshold_classes_np(p, frame_hw, cable_thr=np.inf, tape_thr=np.inf, defect_thr=thr, ratio=np.inf, channels=(k, k, k, k, k))
                assert (got == ((want & bit) != 0) * np.uint8(28)).all()          # bits 0 and 1 never set, bits 2..4 the plain threshold
    assert (sl.BIT_CABLE, sl.BIT_TAPE, sl.BIT_BURR) == (4, 8, 16)


def test_merge_tables():
    assert sl.LUT_BURR[sl.BIT_BURR] == 1 and sl.LUT_BURR[sl.BIT_CABLE | sl.BIT_TAPE | 3] == 0
    assert sl.LUT_SIMPLE[sl.BIT_CABLE | sl.BIT_KEPT_BURR | 1] == 0b101 and sl.LUT_SIMPLE[sl.BIT_BURR] == 0
    assert sl.LUT_TAPE_CABLE[sl.BIT_TAPE] == 1 and sl.LUT_TAPE_CABLE[sl.BIT_CABLE] == 2 and sl.LUT_JOINED[7] == 7
    for planes, lut in ((sl.PLANES_BURR, sl.LUT_BURR), (sl.PLANES_JOINED, sl.LUT_JOINED), (sl.PLANES_BACKUP[0], None), (sl.PLANES_BACKUP[1], None)):
        mc.check_planes(planes, lut)
    for v in sl.VARIANTS.values():
        mc.check_planes(((None, v["cable"], 1), (None, v["tape"], 2), (None, (), 5)), sl.LUT_SIMPLE)


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    p = sl.make_probs(1, 3, 8, 8, 0)
    m = np.zeros((1, 8, 8), np.uint8)
    bad = [
        lambda: sl.relative_threshold_np(p.astype(np.float64)), lambda: sl.relative_threshold_np(p[0]), lambda: sl.relative_threshold_np(p[:, :2]),
        lambda: sl.relative_threshold_np(p, layout="chw"), lambda: sl.relative_threshold_np(p, float("nan")), lambda: sl.confidence_threshold_np(p, float("nan")),
        lambda: sl.confidence_threshold_np(p.transpose(0, 2, 3, 1)[..., :2], layout="nhwc"),
        lambda: sl.keep_components_np(m[0], 1), lambda: sl.keep_components_np(m.astype(np.int32), 1), lambda: sl.keep_components_np(m, float("nan")),
        lambda: sl.keep_components_np(m, 1, float("nan")), lambda: sl.tape_position_filter_np(m, m[:, :4]), lambda: sl.tape_position_filter_np(m, m.astype(bool)),
        lambda: sl.column_band_np(m, 0.25, 1.5), lambda: sl.column_band_np(m[0]),
        lambda: sl.predict_simple_np(sl.make_simple_batch(("filtered",)), (16, 16), "backup"), lambda: sl.predict_simple_np(sl.make_simple_batch(("filtered",))[:, :5], (16, 16)),
        lambda: sl.predict_simple_np(sl.make_simple_batch(("filtered",)), (0, 16)), lambda: sl.threshold_planes_np(p, (8, 8), (0.1, 0.2)),
        lambda: sl.threshold_planes_np(p, (8, 8), (0.1, 0.2, float("nan"))), lambda: sl.predict_simple_backup_np(m[0]),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"call {i} was accepted")


# ---- the header's entries (names, types, build inputs and guard coverage: tests/test_bindings_host.py) -----------------------------------
def test_header_is_c99(tmp_path):
    cc_ = shutil.which("cc") or shutil.which("gcc")
    assert cc_, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "unetpp_simple_loops.h"\nint main(void) { int32_t t[UNETPP_TAPE_TABLE_COLUMNS] = {0}; (void)t; '
                   'return UNETPP_PIXEL_CONFIDENCE - 1 + (UNETPP_TAPE_MAX_PIXELS != 8388608); }\n')
    subprocess.run([cc_, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True, text=True)


def test_entries_refuse_a_null_engine():
    lib = _lib.load()
    assert lib.unetpp_pixel_rules_f32(None, None, 1, 1, 1, 1, 8, 8, 0, 2.0, 2.5, None, None, None) == -1
    assert lib.unetpp_components_keep(None, None, None, None, 1, 8, 8, 16, 1, 2, 0, 1, None, None, None) == -1
    assert lib.unetpp_tape_position_filter_u8(None, None, -1, None, -1, 1, 8, 8, None, None, None) == -1
    assert lib.unetpp_column_band_u8(None, None, 1, 8, 8, 2, 6, None, None) == -1
    assert lib.unetpp_mask_join_u8(None, None, 255, None, 0, None, 0, 1, 8, 8, None, None) == -1


def test_components_np_is_the_labelling_the_rule_reads():
    """keep_components decides from unetpp_components' stats: WIDTH is the bounding box's, AREA the pixel count (an L has both)."""
    m = np.zeros((1, 12, 30), np.uint8)
    m[0, 2:10, 3] = 1
    m[0, 9, 3:25] = 1                                # an L: area 8 + 21 = 29, box width 22
    _, stats, _ = cc.components_np(m[0], 8, -1)
    assert stats[1, cc.CC_STAT_AREA] == 29 and stats[1, cc.CC_STAT_WIDTH] == 22
    assert sl.keep_components_np(m, 29, 29, 22).sum() == 29 and sl.keep_components_np(m, 29, 29, 23).sum() == 0
