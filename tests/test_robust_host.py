"""The NumPy forms of the robust loop's mask rules (unet_amd/robust.py) against each other and against the fixtures made from
the reference's own functions (tests/golden/robust_scenes.npz, scripts/make_golden_robust.py).  No GPU.  Everything is
compared exactly: integers, float32 bits, `==` on float64."""
import hashlib
import json

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import robust as rb

METRICS = ("l2", "l1", "c")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("robust_scenes")
    return g, [tuple(r) for r in g["cases"].tolist()]


def regenerate(row):
    """(tag, cable, tape, parameters) of a fixture row, SHA-checked."""
    tag, H, W, seed, opts, params, sha_c, sha_t = row
    c, t = rb.make_robust_scene(int(H), int(W), int(seed), **json.loads(opts))
    assert hashlib.sha256(np.ascontiguousarray(c).tobytes()).hexdigest() == sha_c, tag
    assert hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest() == sha_t, tag
    return tag, c, t, json.loads(params)


def unpack(g, key, shape):
    return np.unpackbits(g[key])[:shape[0] * shape[1]].reshape(shape)


# ---- the distance transform: the two scans against the closed form -------------------------------------------------------
SHAPES = [(1, 70), (70, 1), (33, 57), (96, 200)]


def planes(shape):
    """The issue's planes for one shape: random zero densities, all zero, all non-zero, one zero in a corner."""
    r = np.random.default_rng(1000 + shape[0] * 7 + shape[1])
    out = {f"density_{d}": (r.random(shape) >= d).astype(np.uint8) for d in (0.5, 0.1, 0.01, 0.001)}
    out["all_zero"], out["all_nonzero"] = np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    out["corner"] = np.ones(shape, np.uint8)
    out["corner"][-1, 0] = 0
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_pass_equals_the_closed_form(shape):
    for name, m in planes(shape).items():
        closed = rb.distance_fixed_closed_all_np(m, METRICS)
        for metric in METRICS:
            a, b = rb.distance_fixed_np(m, metric), closed[metric]
            assert a.dtype == np.int64 and np.array_equal(a, b), (shape, name, metric)
            fa, fb = rb.distance_transform_np(m, metric), rb.fixed_to_float(b)
            assert fa.dtype == np.float32 and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), (shape, name, metric)
        assert np.array_equal(rb.distance_transform_closed_np(m, "c"), rb.fixed_to_float(closed["c"]))
        if name == "all_nonzero":
            assert (rb.distance_transform_np(m) == np.float32(8192.0)).all() and (rb.distance_fixed_np(m) == (2 ** 31 - 1) >> 2).all()
        if name == "all_zero":
            assert not rb.distance_fixed_np(m).any()


@pytest.mark.parametrize("shape", [(1, 70), (70, 1), (33, 57)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_scans_equal_the_pixel_loops(shape):
    """distance_fixed_np forms each row's scan as a running minimum; OpenCV's loops pixel by pixel give the same integers."""
    for name, m in planes(shape).items():
        for metric in METRICS:
            assert np.array_equal(rb.distance_fixed_np(m, metric), rb.distance_fixed_literal_np(m, metric)), (shape, name, metric)


def test_weights_and_float_conversion():
    assert rb.METRICS == {"l2": (62587, 89738), "l1": (65536, 131072), "c": (65536, 65536)}
    assert int(np.rint(np.float32(0.955) * np.float32(65536))) == 62587 and int(np.rint(np.float32(1.3693) * np.float32(65536))) == 89738
    assert rb.DIST_CAP == 536870911 and rb.fixed_to_float(rb.DIST_CAP) == np.float32(8192.0)
    # t is rounded to float32, then scaled: `d >= 2` begins at t = 131072 (131071 is below) and `d <= 20` ends at 1310720
    t = np.arange(131060, 131080)
    assert int(t[rb.fixed_to_float(t) >= 2][0]) == 131073 - 1
    t = np.arange(1310700, 1310740)
    assert int(t[rb.fixed_to_float(t) <= 20][-1]) == 1310720
    big = np.array([2 ** 24 + 1, 2 ** 29 - 3])                    # not float32 numbers: rounded first
    assert np.array_equal(rb.fixed_to_float(big), np.array([256.0, 8192.0], np.float32))
    # one step along a row, a column and a diagonal
    m = np.ones((3, 3), np.uint8)
    m[1, 1] = 0
    d = rb.distance_fixed_np(m)
    assert d[1, 0] == d[0, 1] == 62587 and d[0, 0] == d[2, 2] == 89738
    with pytest.raises(ValueError):
        rb.distance_transform_np(m, "l3")


def test_ring_bounds_are_compared_in_float32():
    m = np.ones((1, 40), np.uint8)
    m[0, 0] = 0
    d = rb.distance_transform_np(m)
    lo = float(d[0, 3]) + 1e-9                                      # rounds to d[0, 3] in float32: the pixel stays in
    ring = rb.ring_np(m, None, lo, 20)
    assert ring[0, 3] == 1 and ring[0, 2] == 0 and ring[0, 0] == 0
    assert ring.sum() == int(((d >= np.float32(lo)) & (d <= np.float32(20))).sum())


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
def test_fixture_has_the_promised_scenes(golden):
    g, rows = golden
    assert sorted((int(r[1]), int(r[2])) for r in rows) == [(33, 57)] * 2 + [(96, 200)] * 2 + [(512, 512)] * 2
    call_site = [json.loads(r[5]) for r in rows if int(r[1]) == 512]
    assert all(p == {"close_ksize": 5, "min_area": 2000, "min_h_ratio": 0.35, "min_aspect": 3.0, "max_w_ratio": 0.2, "band_out": 20,
                     "band_in": 2, "tape_min_area": 500, "pad": 80} for p in call_site)
    kept = [int(np.unpackbits(g[r[0] + "_tape"]).sum()) for r in rows]
    assert sum(1 for k in kept if k) >= 4 and sum(1 for k in kept if not k) >= 2


@pytest.mark.parametrize("index", range(6))
def test_compositions_equal_the_fixture(golden, index):
    g, rows = golden
    tag, c, t, P = regenerate(rows[index])
    shape = c.shape
    best_raw = rb.keep_best_cable_np(c, P["min_area"], P["min_h_ratio"], P["min_aspect"], P["max_w_ratio"])
    assert np.array_equal(best_raw, unpack(g, tag + "_best_raw", shape)), tag
    ring_raw = rb.restrict_tape_to_ring_np(t, best_raw, P["band_out"], P["band_in"], P["tape_min_area"])
    assert np.array_equal(ring_raw, unpack(g, tag + "_ring_raw", shape)), tag
    assert np.array_equal(rb.roi_limit_np(t, best_raw, P["pad"]), unpack(g, tag + "_roi_raw", shape)), tag
    cable, tape = rb.postprocess_robust_np(c, t, P["close_ksize"], P["min_area"], P["min_h_ratio"], P["min_aspect"], P["max_w_ratio"],
                                           P["band_out"], P["band_in"], P["tape_min_area"], P["pad"])
    assert np.array_equal(cable, unpack(g, tag + "_cable", shape)) and np.array_equal(tape, unpack(g, tag + "_tape", shape)), tag
    m = rb.measure_diameters_np(cable, tape)
    want = g[tag + "_measure"]
    for k, name in enumerate(rb.MEASURE_FIELDS):
        assert isinstance(m[name], float) and m[name] == want[k], (tag, name, m[name], want[k])


def test_best_cable_meets_every_rejection_and_unique_scores(golden):
    from unet_amd import components as cc
    g, rows = golden
    seen, counts = set(), []
    for row in rows:
        tag, c, _, P = regenerate(row)
        _, stats, _ = cc.components_np(c, 8, -1)
        best, why, scores = rb.best_cable_label(stats, c.shape[0], c.shape[1], P["min_area"], P["min_h_ratio"], P["min_aspect"], P["max_w_ratio"],
                                                return_trace=True)
        seen.update(v for v in why.values() if v)
        counts.append(len(scores))
        if scores:
            assert sorted(scores.values())[-1] > ([-1.0] + sorted(scores.values()))[-2] and scores[best] == max(scores.values()), tag
    assert seen == {"area", "height", "width", "aspect"} and max(counts) >= 2 and min(counts) == 0


def test_median_and_empty_cases():
    m = np.zeros((6, 9), np.uint8)
    assert rb.row_width_median_np(m) == 0.0
    m[0, 2] = 1                                                   # one pixel: xs.size > 1 fails
    assert rb.row_width_median_np(m) == 0.0
    m[1, 1:4] = 1
    m[2, [0, 8]] = 1                                              # widths 3 and 9: an even count, the mean of the two
    assert rb.row_width_median_np(m) == 6.0
    m[3, 0:2] = 1
    assert rb.row_width_median_np(m) == 3.0
    d = rb.measure_diameters_np(np.zeros((6, 9), np.uint8), m)
    assert d["dc_px"] == 0.0 and d["dt_px"] == 3.0 and d["delta_d_px"] == 0.0 and d["tape_coverage"] == 8 / 54
    assert not rb.roi_limit_np(m, np.zeros_like(m)).any() and not rb.restrict_tape_to_ring_np(m, np.zeros_like(m), 10 ** 6, 0, 1).any()


# ---- letterbox ------------------------------------------------------------------------------------------------------------
def test_letterbox_plan_equals_the_reference_meta(golden):
    g, _ = golden
    shapes = [tuple(s) for s in g["letterbox_shapes"].tolist()]
    assert shapes == [(1080, 1920), (1920, 1080), (512, 512), (37, 53), (480, 640)]
    for (h, w), want in zip(shapes, g["letterbox_meta"]):
        plan = rb.letterbox_plan(h, w, 512)
        assert isinstance(plan[0], float) and all(isinstance(v, int) for v in plan[1:])
        assert [float(v) for v in plan] == want.tolist(), (h, w)
    with pytest.raises(ValueError):
        rb.letterbox_plan(1, 2000, 512)


def test_letterbox_and_unletterbox_equal_the_fixture(golden):
    g, _ = golden
    r = np.random.default_rng(7)
    frame = r.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    mask = (r.random((64, 64)) < 0.4).astype(np.uint8)
    assert hashlib.sha256(frame.tobytes()).hexdigest() == str(g["lb_frame_sha"]) and hashlib.sha256(mask.tobytes()).hexdigest() == str(g["lb_mask_sha"])
    canvas, plan = rb.letterbox_np(frame, 64)
    assert [float(v) for v in plan] == g["lb_meta"].tolist() and np.array_equal(canvas, g["lb_canvas"])
    assert np.array_equal(rb.unletterbox_mask_np(mask, plan), g["lb_unletterbox"])


def test_bindings_and_source_hash_cover_the_new_entries():
    from unet_amd import _lib
    for name in ("unetpp_distance_transform_u8", "unetpp_distance_workspace_bytes", "unetpp_components_best_cable", "unetpp_roi_limit_u8",
                 "unetpp_roi_limit_workspace_bytes", "unetpp_row_width_median"):
        assert name in _lib.ABI
    assert "distance.h" in _lib.HEADERS
    assert _lib.CC_RULES == {"largest": 0, "spatial": 1, "cable_shape": 2}
