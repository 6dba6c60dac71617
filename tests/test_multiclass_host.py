"""unet_amd/multiclass.py without a device: the NumPy forms against the reference's stored results
(tests/golden/multiclass_scenes.npz, scripts/make_golden_multiclass.py), the conditions the fixture must meet, argument checks,
the limits of unetpp_merge_classes through its layout query, and the host rules on the class table."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import morphology as mo
from unet_amd import multiclass as mc

UNSUPPORTED, INVALID = -2, -1


@pytest.fixture(scope="module")
def golden():
    return load_golden("multiclass_scenes")


def pair(g, which):
    return g["colors_" + which][:, :3], g["colors_" + which][:, 3]


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_fixture_meets_its_conditions(golden):
    facts = mc.fixture_facts(golden)
    assert facts["edge_rule"][0] > 0 and facts["edge_rule"][1] > 0 and facts["moving"] == "moving"
    assert str(golden["numpy_version"]) and {"colors_video", "colors_v3", "colors_opt"} <= set(golden.files)
    assert not golden["colors_v3"][3, 3] and golden["colors_v3"][4, 3] and golden["colors_video"][1:7, 3].all()


def test_gate_against_the_reference(golden):
    for name, kind, h, w, seed, digest in golden["gate"]:
        frames = mc.make_gate_sequence(int(h), int(w), int(seed), str(kind))
        assert mc.sha(frames) == digest
        is_bad, reason, lap_var, gray_std, mad, gray = mc.quality_gate_np(frames)
        assert np.array_equal(is_bad, golden[name + "_is_bad"]) and np.array_equal(reason, golden[name + "_reason"])
        assert np.array_equal(mad, golden[name + "_mad"])           # an exact integer below 2^53 divided once, here and there
        # the closed form of exact integer sums, correctly rounded, against NumPy's two-pass float64 std / var with pairwise
        # summation: a few ulps, 2.2e-16 x a summation depth of at most about 21 x a small constant
        assert np.allclose(gray_std, golden[name + "_gray_std"], rtol=1e-12, atol=0)
        assert np.allclose(lap_var, golden[name + "_lap_var"], rtol=1e-12, atol=0)
        assert mc.sha(gray[-1]) == str(golden[name + "_gray_sha"])
        off = mc.quality_gate_np(frames, enable=False)
        assert not off[0].any() and not off[1].any() and not off[2].any() and not off[4].any()
        assert np.allclose(off[3], golden[name + "_disabled_std"], rtol=1e-12, atol=0)
        # a batch cut in two with the grey frame handed on is the same sequence
        cut = len(frames) // 2
        first, second = mc.quality_gate_np(frames[:cut]) if cut else None, None
        if cut:
            second = mc.quality_gate_np(frames[cut:], first[5][-1])
            for k in range(5):
                assert np.array_equal(np.concatenate([first[k], second[k]]), (is_bad, reason, lap_var, gray_std, mad)[k])


def test_class_scenes_against_the_reference(golden):
    kw = dict(zip(("min_cable_area", "cable_coverage_threshold", "min_defect_area", "edge_margin"), golden["validate"].tolist()))
    for name, h, w, seed, pred_sha, frame_sha in golden["video"]:
        h, w = int(h), int(w)
        pred, frame = mc.make_class_scene(h, w, int(seed))
        assert mc.sha(pred) == pred_sha and mc.sha(frame) == frame_sha
        want = golden[name + "_video"]
        got, table = mc.clean_classes_video_np(pred[None], num_classes=7)
        assert np.array_equal(got[0], want) and np.array_equal(table, mc.class_table_np(want[None], 7))
        assert int(table[0, :, 0].sum()) == h * w
        for alpha, tag in ((0.5, "a50"), (0.6, "a60")):
            assert mc.sha(mc.overlay_np(frame[None], got, pair(golden, "video"), alpha, "region", 7)[0]) == str(golden[f"{name}_region_{tag}"])
            assert mc.sha(mc.overlay_np(frame[None], got, pair(golden, "opt"), alpha, "weighted")[0]) == str(golden[f"{name}_weighted_{tag}"])
        assert mc.sha(mc.overlay_np(frame[None], got, pair(golden, "video"), 0.6, "region", 6)[0]) == str(golden[name + "_region6_a60"])
        valid, defects = mc.validate_detection(table[0], (h, w), **kw)
        assert valid == bool(golden[name + "_valid"])
        assert [[d["class_id"], *d["bbox"], d["area"]] for d in defects] == golden[name + "_defects"].tolist()
        # the event rule's area and box part, against the reference's own expressions on the mask
        events = mc.defect_events(table[0], min_area_px=50)
        for cid in (3, 5, 6):
            ys, xs = np.where(want == cid)
            if len(ys) >= min(50, 10):
                assert {"class_id": cid, "bbox": (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())), "area": len(ys)} in events
        assert [e["class_id"] for e in events] == [c for c in (3, 5, 6) if (want == c).sum() >= 10]
    for name, side, seed, digest in golden["v3"]:
        assert mc.sha(mc.make_v3_logits(int(side), int(seed))) == digest
        planes, want = golden[name + "_planes"], golden[name + "_v3"]
        got, table = mc.predict_v3_np(planes[None], None, channels=(0, 1, 2, 3, 4), num_classes=7)
        assert np.array_equal(got[0], want) and table[0, 3, 0] == 0 and set(np.unique(want)) == {0, 1, 2, 4, 5, 6}
        nhwc = np.ascontiguousarray(planes.transpose(1, 2, 0))[None]
        assert np.array_equal(mc.predict_v3_np(nhwc, None, channels=(0, 1, 2, 3, 4), layout="nhwc", want_table=False)[0], want)
        frame = np.random.default_rng(int(seed)).integers(0, 256, want.shape + (3,), dtype=np.uint8)
        with_three = want.copy()
        with_three[:4, :4] = 3
        assert mc.sha(mc.overlay_np(frame[None], with_three[None], pair(golden, "v3"), 0.5, "region", 6)[0]) == str(golden[name + "_region_a50"])


# ---- the NumPy forms on their own ---------------------------------------------------------------------------------------------------
def test_statistics_are_the_rounded_closed_form():
    from fractions import Fraction
    r = np.random.default_rng(5)
    frames = r.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    gray, sums = mc.quality_sums_np(frames)
    n = 37 * 53
    _, _, lap_var, gray_std, mad, _ = mc.quality_gate_np(frames)
    for b, (s1, s2, l1, l2, d) in enumerate(sums):
        g = gray[b].astype(np.int64)
        assert s1 == g.sum() and s2 == (g * g).sum() and l1 == mc.laplacian_np(gray[b]).sum()
        assert lap_var[b] == float(Fraction(n * l2 - l1 * l1, n * n)) and mad[b] == float(Fraction(d, n))
        assert abs(gray_std[b] - gray[b].std()) <= 1e-12 * gray_std[b] and abs(lap_var[b] - mc.laplacian_np(gray[b]).astype(np.float64).var()) <= 1e-12 * lap_var[b]
    assert sums[0][4] == 0 and sums[1][4] == np.abs(gray[1].astype(int) - gray[0].astype(int)).sum()
    one = mc.laplacian_np(np.array([[7]], np.uint8))
    assert one.tolist() == [[0]] and mc.laplacian_np(np.array([[1, 5, 2]], np.uint8)).tolist() == [[8, -7, 6]]


def test_merge_is_the_reference_order_of_operations():
    r = np.random.default_rng(2)
    pred = r.integers(0, 7, (1, 40, 60), dtype=np.uint8)
    e3 = mo.structuring_element("ellipse", 3)
    raw = np.where(pred[0] == 4, 0, pred[0]).astype(np.uint8)
    want = np.zeros_like(raw)
    want[mo.erode_np(mo.dilate_np(raw == 1, e3), e3)] = 1
    want[mo.erode_np(mo.dilate_np(raw == 2, e3), e3)] = 2
    d = np.isin(raw, (3, 5, 6))
    want[d] = raw[d]
    got, table = mc.clean_classes_video_np(pred, num_classes=7)
    assert np.array_equal(got[0], want) and table[0, 4].tolist() == [0, -1, -1, -1, -1]
    only_table = mc.merge_classes_np(pred, mc.PLANES_TABLE, want_table=True)
    assert np.array_equal(only_table[0], pred) and np.array_equal(only_table[1], mc.class_table_np(pred))
    empty = np.zeros((1, 9, 9), np.uint8)
    assert not mc.merge_classes_np(empty, mc.PLANES_V3, lut=mc.LUT_BITS, want_table=False).any()      # the v3 guards are no-ops


def test_threshold_scalars_are_rounded_to_float32_first():
    t = np.float32(0.6)
    p = np.zeros((1, 5, 1, 4), np.float32)
    p[0, 0, 0] = (t, np.nextafter(t, np.float32(0)), 0.9, 0.9)
    p[0, 1, 0] = (0.0, 0.0, np.float32(0.9) / np.float32(1.2), 0.74)
    bits = mc.threshold_classes_np(p, channels=(0, 1, 2, 3, 4))[0, 0]
    assert (bits & 1).tolist() == [1, 0, int(np.float32(0.9) > p[0, 1, 0, 2] * np.float32(1.2)), 1]
    assert (p[0, 0] >= 0.6).tolist()[0][:2] == [True, False]       # what NumPy itself does with the Python scalar
    p[0, 2, 0, 0] = np.nan
    assert mc.threshold_classes_np(p, channels=(0, 1, 2, 3, 4))[0, 0, 0] == 1
    same = mc.make_prob_planes(1, 12, 20, 1)
    assert np.array_equal(mc.threshold_classes_np(same, (12, 20), channels=(0, 1, 2, 3, 4)), mc.threshold_classes_np(same, channels=(0, 1, 2, 3, 4)))
    assert mc.threshold_classes_np(same, (25, 33), channels=(0, 1, 2, 3, 4)).shape == (1, 25, 33)


def test_overlay_modes():
    frames = np.array([[[[10, 20, 30], [200, 100, 50], [255, 255, 255], [1, 2, 3]]]], np.uint8)
    mask = np.array([[[0, 1, 9, 2]]], np.uint8)
    colors = {0: (9, 9, 9), 1: (255, 0, 0), 2: (0, 255, 0)}
    out = mc.overlay_np(frames, mask, colors, 0.5, "region")
    assert out[0, 0, 0].tolist() == [10, 20, 30] and out[0, 0, 1].tolist() == [227, 50, 25] and out[0, 0, 2].tolist() == [127, 127, 127]
    out = mc.overlay_np(frames, mask, colors, 0.5, "weighted")
    assert out[0, 0, 0].tolist() == [10, 20, 30] and out[0, 0, 1].tolist() == [228, 50, 25] and out[0, 0, 2].tolist() == [255, 255, 255]
    assert mc.overlay_np(frames, mask, colors, 0.5, "region", 2)[0, 0, 3].tolist() == [0, 1, 1]        # class 2 dropped: black
    table, has = mc.color_table(colors)
    assert has[:3].tolist() == [0, 1, 1] and table[1].tolist() == [255, 0, 0]


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="frames must be uint8"):
        mc.quality_gate_np(frames[..., :2])
    with pytest.raises(ValueError, match="prev_gray"):
        mc.quality_gate_np(frames, np.zeros((8, 7), np.uint8))
    with pytest.raises(ValueError, match="NaN"):
        mc.quality_gate_np(frames, flat_th=float("nan"))
    mask = np.zeros((1, 8, 8), np.uint8)
    for planes, text in (([], "planes"), ([((1,), (), 1)] * 7, "planes"), ([((1,), (), 0)], "out_value"), ([((300,), (), 1)], "not in 0..255"),
                         ([((1,), (("blur", 3),), 1)], "op must be"), ([((1,), (("close", 3, 0),), 1)], "iterations"), ([(None, (), 1)], "no lut"),
                         ([((1,), (("close", 65),), 1)], "at most 63"), ([((1,), (("close", 3),) * 9, 1)], "steps"),
                         ([((1,), tuple(("dilate", k) for k in (3, 5, 7, 9, 11)), 1)], "elements"), ([((1,), (("close", 33),), 1)] * 2, "reach")):
        with pytest.raises(ValueError, match=text):
            mc.merge_classes_np(mask, planes)
    with pytest.raises(ValueError, match="lut"):
        mc.merge_classes_np(mask, [(None, (), 1)], lut=np.full(256, 2, np.uint8))
    with pytest.raises(ValueError, match="num_classes"):
        mc.class_table_np(mask, 257)
    probs = np.zeros((1, 6, 4, 4), np.float32)
    with pytest.raises(ValueError, match="channels"):
        mc.threshold_classes_np(probs, channels=(1, 2, 3, 4, 6))
    with pytest.raises(ValueError, match="layout"):
        mc.threshold_classes_np(probs, layout="chw")
    with pytest.raises(ValueError, match="probs must be float32"):
        mc.threshold_classes_np(probs.astype(np.float64))
    with pytest.raises(ValueError, match="NaN"):
        mc.threshold_classes_np(probs, ratio=float("nan"))
    with pytest.raises(ValueError, match="alpha"):
        mc.overlay_np(frames, np.zeros((2, 8, 8), np.uint8), {1: (1, 2, 3)}, 1.5)
    with pytest.raises(ValueError, match="mode"):
        mc.overlay_np(frames, np.zeros((2, 8, 8), np.uint8), {1: (1, 2, 3)}, 0.5, "blend")
    with pytest.raises(ValueError, match="mask must be uint8"):
        mc.overlay_np(frames, np.zeros((2, 8, 7), np.uint8), {1: (1, 2, 3)})
    with pytest.raises(ValueError, match="colour"):
        mc.color_table({1: (1, 2, 300)})


def test_limits_are_unsupported_never_wrong():
    """The limits of unetpp_morphology applied to all planes together, asked of the layout query (no engine, no device)."""
    from unet_amd import _lib
    lib = _lib.load()
    e3, e33 = mo.structuring_element("ellipse", 3), mo.structuring_element("ellipse", 33)
    big = np.ones((65, 65), np.uint8)
    els = (_lib.MorphElement * 5)(*[_lib.MorphElement(a.shape[1], a.shape[0], -1, -1, a.ctypes.data) for a in (e3, e33, big, e3, e3)])
    band, cols = ctypes.c_int(), ctypes.c_int()

    def ask(n_planes, n_el, steps, h=64, w=64, first=0):
        st = (_lib.MergeStep * max(len(steps), 1))(*[_lib.MergeStep(*s) for s in steps])
        first_el = ctypes.cast(ctypes.byref(els, first * ctypes.sizeof(_lib.MorphElement)), ctypes.POINTER(_lib.MorphElement))
        return lib.unetpp_merge_classes_layout(1, h, w, n_planes, first_el, n_el, st, len(steps), ctypes.byref(band), ctypes.byref(cols))

    close = _lib.MERGE_OPS["close"]
    assert ask(2, 1, [(0, close, 0, 1), (1, close, 0, 1)]) == 0 and band.value >= 1 and cols.value % 64 == 0
    assert ask(7, 1, []) == UNSUPPORTED                                           # planes
    assert ask(1, 5, []) == UNSUPPORTED                                           # elements
    assert ask(2, 1, [(k % 2, close, 0, 1) for k in range(9)]) == UNSUPPORTED     # steps over all planes
    assert ask(2, 2, [(0, close, 1, 1), (1, close, 1, 1)]) == UNSUPPORTED         # reach 2 x 64 over all planes
    assert ask(1, 2, [(0, close, 1, 1)]) == 0                                     # one of them alone fits
    assert ask(1, 1, [(0, close, 0, 1)], first=2) == UNSUPPORTED                  # a 65 x 65 element
    assert ask(1, 1, [(0, close, 0, 127)]) == UNSUPPORTED                         # iterations
    assert ask(1, 1, [(1, close, 0, 1)]) == INVALID and ask(1, 1, [(0, 2, 0, 1)]) == INVALID and ask(0, 0, []) == INVALID
    assert ask(1, 1, [(0, close, 0, 1)], h=0) == INVALID
    rows, width = mc.merge_layout((1, 64, 64), mc.PLANES_VIDEO)
    assert 1 <= rows <= 64 and width == 64
    with pytest.raises(ValueError):
        mc.merge_layout((1, 0, 64), mc.PLANES_VIDEO)


# ---- the host rules -----------------------------------------------------------------------------------------------------------------
def table_of(mask):
    return mc.class_table_np(mask[None], 7)[0]


def test_validate_detection_rules():
    kw = dict(min_cable_area=50, cable_coverage_threshold=0.1, min_defect_area=4, edge_margin=5)
    m = np.zeros((40, 60), np.uint8)
    assert mc.validate_detection(table_of(m), m.shape, **kw) == (False, [])       # no cable
    m[:, 20:23] = 1
    assert mc.validate_detection(table_of(m), m.shape, **kw) == (False, [])       # coverage 0.05
    m[:, 20:30] = 1
    m[10:14, 30:34] = 3                                                           # away from every edge
    m[0:3, 40:50] = 5                                                             # mostly inside the top margin: dropped
    m[20:30, 50:58] = 6                                                           # touches the right margin: kept
    valid, defects = mc.validate_detection(table_of(m), m.shape, **kw)
    assert valid and [(d["class_id"], d["bbox"], d["area"]) for d in defects] == [(3, (30, 10, 33, 13), 16), (6, (50, 20, 57, 29), 80)]
    m[5:12, 0] = 4                                                                # one pixel wide at the edge
    with pytest.raises(ZeroDivisionError):
        mc.validate_detection(table_of(m), m.shape, **kw)
    assert mc.validate_detection(table_of(m), m.shape, defect_classes=(3,), **kw)[1][0]["class_id"] == 3
    with pytest.raises(ValueError, match="table"):
        mc.validate_detection(np.zeros((7, 4), np.int32), m.shape, **kw)


def test_defect_events_rule():
    m = np.zeros((30, 30), np.uint8)
    m[2:5, 3:6] = 3                                                               # 9 pixels
    m[10:20, 10:12] = 5                                                           # 20 pixels
    m[25, 25] = 4
    t = table_of(m)
    assert mc.defect_events(t, min_area_px=50) == [{"class_id": 5, "bbox": (10, 10, 11, 19), "area": 20}]       # min(50, 10)
    assert [e["class_id"] for e in mc.defect_events(t, min_area_px=5)] == [3, 5]
    assert mc.defect_events(t, classes=(4, 6), min_area_px=1) == [{"class_id": 4, "bbox": (25, 25, 25, 25), "area": 1}]
    assert mc.defect_events(t[:4], min_area_px=1) == [{"class_id": 3, "bbox": (3, 2, 5, 4), "area": 9}]
