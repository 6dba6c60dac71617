"""The NumPy restatement of the measurement step (unet_amd/geometry.py) against the fixtures made from the reference's own
functions (tests/golden/geometry_scenes.npz, scripts/make_golden_geometry.py) and against independent definitions of its
primitives.  No GPU.  Fixture comparisons are exact (== on float64 and float32)."""
import hashlib
import json

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import components as cc
from unet_amd import geometry as ge
from unet_amd import morphology as mo


@pytest.fixture(scope="module")
def golden():
    g = load_golden("geometry_scenes")
    return g, [tuple(r) for r in g["cases"].tolist()]


def regenerate(row):
    """(pred uint8 [H,W], min_valid_rows) of a fixture row, SHA-checked."""
    tag, kind, gen, H, W, seed, opts, sha = row
    H, W, seed, opts = int(H), int(W), int(seed), json.loads(opts)
    mvr = opts.pop("min_valid_rows", 20)
    if gen == "wrap":
        m = ge.make_wrap_scene(H, W, seed, **opts)
    elif gen == "scene":
        m = cc.make_scene_mask(H, W, seed)
    else:
        m = mo.make_hole_scene(H, W, seed, noise=opts["noise"])
    assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() == sha, tag
    return m, mvr


METRIC_F64 = ("dc_px", "dt_px", "delta_d_px", "dc_mm", "dt_mm", "delta_d_mm", "cable_coverage", "tape_coverage")
DEFECT_F64 = ("tape_hole_ratio", "tape_coverage", "tape_largest_area_ratio")
DEFECT_I64 = ("tape_num_holes", "cable_num_components", "tape_num_components", "total_defect_area")


def test_fixture_has_the_promised_cases(golden):
    g, rows = golden
    metrics = [r for r in rows if r[1] == "metrics"]
    assert len(metrics) == 14 and len([r for r in rows if r[1] == "defects"]) == 4
    rows_of = {r[0]: int(g[r[0] + "_valid_rows"]) for r in metrics}
    assert {v % 2 for t, v in rows_of.items() if t.startswith("wrap_5") or t.startswith("wrap_4")} == {0, 1}
    assert any(0 < v < 20 for v in rows_of.values()) and any(v == 0 for v in rows_of.values())
    assert [rows_of[f"scene_{t}"] for t in ("512x512_0", "512x512_1", "448x800_0", "96x200_2", "40x64_3", "24x48_4")] == [31, 30, 31, 30, 31, 24]
    assert g["scene_512x512_0_f64"][0] == 53.165401458740234 and g["scene_512x512_0_f64"][1] == 70.55188751220703
    assert g["scene_512x512_0_f64"][6] == 0.08205795288085938
    assert any(int(r[3]) <= 15 for r in metrics)                                  # H <= r: the reflect loop


@pytest.mark.parametrize("index", range(14))
def test_metrics_equal_the_fixture(golden, index):
    g, rows = golden
    row = [r for r in rows if r[1] == "metrics"][index]
    tag = row[0]
    m, mvr = regenerate(row)
    mm = float(g["mm_per_px"])
    d = ge.diameter_metrics_np(m, mm_per_px=mm, min_valid_rows=mvr)
    want = g[tag + "_f64"]
    for k, name in enumerate(METRIC_F64):
        assert d[name] == want[k], (tag, name, d[name], want[k])
    assert d["valid_rows"] == int(g[tag + "_valid_rows"])
    H = m.shape[0]
    delta, valid = ge.thickness_profile_np(m, mm_per_px=mm)
    assert delta.dtype == np.float32 and np.array_equal(delta, g[tag + "_delta_d_mm"])
    assert np.array_equal(valid, np.unpackbits(g[tag + "_valid_mask"])[:H].astype(bool))
    wc, ww, v = ge.diameter_profile_np(m, 1, 2)
    assert wc.dtype == np.float32 and np.array_equal(wc, g[tag + "_w_cable_px"]) and np.array_equal(ww, g[tag + "_w_wrap_px"])
    assert v.dtype == np.uint8 and np.array_equal(v, np.unpackbits(g[tag + "_valid"])[:H])


@pytest.mark.parametrize("index", range(4))
def test_defects_equal_the_fixture(golden, index):
    g, rows = golden
    row = [r for r in rows if r[1] == "defects"][index]
    tag = row[0]
    m, _ = regenerate(row)
    a = ge.analyze_defects_np(m)
    for k, name in enumerate(DEFECT_F64):
        assert a[name] == g[tag + "_f64"][k], (tag, name)
    want = g[tag + "_i64"]
    assert [a[n] for n in DEFECT_I64] + a["defect_areas"] == want.tolist(), tag


def test_the_largest_component_filter_matters(golden):
    g, rows = golden
    changed = 0
    for row in [r for r in rows if r[0].startswith("wrap_") and json.loads(r[6]) == {}]:
        m, _ = regenerate(row)
        widths, _ = ge.row_widths_np(m, 1, m, 2)
        _, _, dc, dt, n = ge.width_profile_np(widths, ge.gaussian_taps_f32(31))
        changed += (n, float(dc), float(dt)) != (int(g[row[0] + "_valid_rows"]), g[row[0] + "_f64"][0], g[row[0] + "_f64"][1])
    assert changed >= 1


# ---- the primitives against independent definitions ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7, 9, 21, 31, 63, 127])
def test_taps_symmetric_positive_sum_to_one(k):
    t = ge.gaussian_taps_f32(k)
    assert t.dtype == np.float32 and len(t) == k
    assert np.array_equal(t, t[::-1]) and (t > 0).all()
    assert abs(float(t.astype(np.float64).sum()) - 1.0) <= k * 2.0 ** -24
    assert np.argmax(t) == k // 2


def test_taps_even_and_small_sizes():
    assert np.array_equal(ge.gaussian_taps_f32(30), ge.gaussian_taps_f32(31))
    assert np.array_equal(ge.gaussian_taps_f32(1), [1.0]) and np.array_equal(ge.gaussian_taps_f32(0), [1.0])
    assert ge.odd_kernel_size(20) == 21 and ge.odd_kernel_size(21) == 21 and ge.odd_kernel_size(-3) == 1
    w = np.arange(7, dtype=np.float32)
    assert np.array_equal(ge.smooth_widths_np(w, ge.gaussian_taps_f32(1)), w)         # the identity


def test_taps_follow_the_stated_formula():
    k = 31
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    c = np.exp(-0.5 / sigma ** 2 * (np.arange(k) - (k - 1) / 2) ** 2).astype(np.float32)
    s = 0.0
    for v in c:
        s += float(v)
    assert np.array_equal(ge.gaussian_taps_f32(k), (c.astype(np.float64) * (1.0 / s)).astype(np.float32))


@pytest.mark.parametrize("n,r", [(2, 1), (5, 3), (16, 15), (40, 15), (200, 63)])
def test_reflect101_is_numpy_reflect_padding(n, r):
    assert n > r
    a = np.arange(n)
    assert np.array_equal(a[ge.reflect101(np.arange(-r, n + r), n)], np.pad(a, r, mode="reflect"))


@pytest.mark.parametrize("n,r", [(1, 15), (2, 15), (3, 7), (12, 15), (15, 15), (7, 63)])
def test_reflect101_loop_for_short_vectors(n, r):
    def loop(p):
        if n == 1:
            return 0
        while p < 0 or p >= n:
            p = -p if p < 0 else 2 * (n - 1) - p
        return p
    ps = np.arange(-r, n + r)
    got = ge.reflect101(ps, n)
    assert got.tolist() == [loop(int(p)) for p in ps]
    assert ge.reflect101(-r, n) == loop(-r) and isinstance(ge.reflect101(-r, n), int)


@pytest.mark.parametrize("H,k", [(1, 31), (2, 3), (12, 31), (31, 31), (97, 21), (512, 31), (300, 127)])
def test_smoothing_against_scipy_correlate(H, k):
    from scipy.ndimage import correlate1d
    r = np.random.default_rng(H * 1000 + k)
    w = np.floor(r.uniform(0, 700, H)).astype(np.float32)
    w[r.random(H) < 0.2] = 0
    t = ge.gaussian_taps_f32(k)
    got = ge.smooth_widths_np(w, t)
    assert got.dtype == np.float32 and got.shape == (H,)
    want = correlate1d(w.astype(np.float64), t.astype(np.float64), mode="mirror")
    # k products and k sums of non-negative terms whose taps sum to 1, doubled for the taps' own rounding
    bound = 2 * (k + 2) * 2.0 ** -24 * float(w.max())
    assert np.abs(got.astype(np.float64) - want).max() <= bound
    both = ge.smooth_widths_np(np.stack([w, w[::-1]]), t)                              # the last axis of a batch
    assert np.array_equal(both[0], got) and np.array_equal(both[1], ge.smooth_widths_np(w[::-1].copy(), t))


def test_smoothing_order_is_the_stated_one():
    r = np.random.default_rng(3)
    w = np.floor(r.uniform(0, 500, 40)).astype(np.float32)
    t = ge.gaussian_taps_f32(9)
    got = ge.smooth_widths_np(w, t)
    for y in (0, 3, 20, 39):
        at = lambda p: w[ge.reflect101(p, 40)]
        s = np.float32(t[4] * at(y))
        for j in range(1, 5):
            s = np.float32(s + np.float32(t[4 + j] * np.float32(at(y + j) + at(y - j))))
        assert got[y] == s


@pytest.mark.parametrize("n", [1, 2, 3, 4, 255, 256])
def test_median_equals_numpy(n):
    r = np.random.default_rng(n)
    v = r.choice(np.float32([1.5, 2.25, 3.0, 7.125, 100.3, 0.1]), n).astype(np.float32) + np.float32(r.integers(0, 3, n))
    assert ge.median_f32(v) == np.median(v) and isinstance(ge.median_f32(v), np.float32)
    u = r.uniform(0.01, 900, n).astype(np.float32)
    assert ge.median_f32(u) == np.median(u)
    assert ge.median_f32(np.full(n, 3.3, np.float32)) == np.float32(3.3)


def test_row_widths_restate_the_reference_loop():
    r = np.random.default_rng(5)
    m = r.integers(0, 3, (9, 37), dtype=np.uint8) * (r.random((9, 37)) < 0.3)
    m[2] = 0; m[4] = 1; m[5, ::2] = 2; m[6] = 0; m[6, 0] = 1; m[7] = 0; m[7, -1] = 1
    widths, area = ge.row_widths_np(m, 1, m, 2)
    for p, cls in enumerate((1, 2)):
        for y in range(9):
            xs = np.where(m[y] == cls)[0]
            assert widths[p, y] == (float(xs.max() - xs.min() + 1) if xs.size else 0.0)
        assert area[p] == (m == cls).sum()
    w1, a1 = ge.row_widths_np(m, -1)
    assert not w1[1].any() and a1[1] == 0 and a1[0] == (m != 0).sum()
    wb, ab = ge.row_widths_np(np.stack([m, m[::-1]]), 1, np.stack([m, m[::-1]]), 2)
    assert np.array_equal(wb[0], widths) and np.array_equal(wb[1][:, ::-1], widths) and np.array_equal(ab[1], area)


def test_components_summary_np():
    m = mo.make_hole_scene(96, 200, 2, noise=0.02)
    _, stats, _ = cc.components_np(m, 8, 2)
    num = len(stats)
    area = stats[1:, 4].astype(np.int64)
    assert ge.components_summary_np(num, stats, 10).tolist() == [num - 1, int((area >= 10).sum()), int(area[area >= 10].sum()), int(area.max())]
    cut = stats[:5]                                                                     # a table with fewer rows than labels
    assert ge.components_summary_np(num, cut, 0).tolist() == [num - 1, 4, int(area[:4].sum()), int(area[:4].max())]
    assert ge.components_summary_np(1, np.zeros((4, 5), np.int32), 0).tolist() == [0, 0, 0, 0]
    assert ge.components_summary_np(0, np.zeros((4, 5), np.int32), 0).tolist() == [0, 0, 0, 0]


def test_wrap_scene_is_what_it_says():
    m = ge.make_wrap_scene(512, 512, 0, classes7=True)
    assert set(np.unique(m)) == set(range(7))
    for cls in (1, 2):
        _, stats, _ = cc.components_np(m, 8, cls)
        a = np.sort(stats[1:, 4])[::-1]
        assert a[1] >= 50, "the distractor"                                            # second largest component
    assert np.array_equal(m, ge.make_wrap_scene(512, 512, 0, classes7=True))
    assert not (ge.make_wrap_scene(96, 200, 5, cable=False, noise=0.0) == 1).any()


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors():
    with pytest.raises(ValueError):
        ge.check_taps(np.ones(4, np.float32) / 4)                                       # even
    with pytest.raises(ValueError):
        ge.check_taps(np.ones(129, np.float32) / 129)                                   # more than 127
    with pytest.raises(ValueError):
        ge.check_taps([])
    with pytest.raises(ValueError):
        ge.check_taps([0.2, 0.5, 0.3])                                                  # not symmetric
    with pytest.raises(ValueError):
        ge.check_taps([0.25, np.nan, 0.25])
    with pytest.raises(ValueError):
        ge.reflect101(0, 0)
    with pytest.raises(ValueError):
        ge.median_f32(np.zeros(0, np.float32))
    w = np.ones((2, 8), np.float32)
    with pytest.raises(ValueError):
        ge.width_profile_np(w, [1.0], min_valid_rows=0)
    with pytest.raises(ValueError):
        ge.diameter_metrics_np(np.zeros((8, 8), np.uint8), taps=[0.5, 0.5])
    d = ge.diameter_metrics_np(np.zeros((8, 8), np.uint8))
    assert d["valid_rows"] == 0 and d["dc_px"] == 0.0 and d["cable_coverage"] == 0.0
    a = ge.analyze_defects_np(np.zeros((8, 8), np.uint8))
    assert a["tape_hole_ratio"] == 0.0 and a["tape_largest_area_ratio"] == 0.0 and a["tape_num_components"] == 0
