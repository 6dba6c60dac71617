"""The measurement step on the device (unetpp_row_widths, unetpp_width_profile, unetpp_components_summary and the
NestedUNet methods built on them) against the NumPy restatement (unet_amd/geometry.py) and the fixtures made from the
reference's own functions (tests/golden/geometry_scenes.npz).  Integer arithmetic, float32 operations in a fixed order
and correctly rounded float64 expressions: exact equality, no tolerance.
Run on the GPU box:  python -m pytest tests/test_gpu_geometry.py -m gpu"""
import ctypes
import hashlib
import json

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import components as cc
from unet_amd import geometry as ge
from unet_amd import morphology as mo

pytestmark = pytest.mark.gpu

METRIC_F64 = ("dc_px", "dt_px", "delta_d_px", "dc_mm", "dt_mm", "delta_d_mm", "cable_coverage", "tape_coverage")
DEFECT_F64 = ("tape_hole_ratio", "tape_coverage", "tape_largest_area_ratio")
DEFECT_I64 = ("tape_num_holes", "cable_num_components", "tape_num_components", "total_defect_area")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: none of this needs any


@pytest.fixture(scope="module")
def model7(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(7, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # counts classes 3..6


@pytest.fixture(scope="module")
def golden():
    g = load_golden("geometry_scenes")
    return g, [tuple(r) for r in g["cases"].tolist()]


def regenerate(row):
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


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---- 1. the fixtures from the reference's own functions ----------------------------------------------------------------
@pytest.mark.parametrize("index", range(14))
def test_fixture_metrics_and_profiles(torch_cuda, model, golden, index):
    torch = torch_cuda
    g, rows = golden
    row = [r for r in rows if r[1] == "metrics"][index]
    tag = row[0]
    m, mvr = regenerate(row)
    H, W = m.shape
    mm = float(g["mm_per_px"])
    # the frame between an empty frame and a second copy: a batch must not mix its frames
    pred = torch.from_numpy(np.stack([m, np.zeros_like(m), m])).cuda()
    d = host(model.diameter_metrics(pred, mm_per_px=mm, min_valid_rows=mvr))
    want = g[tag + "_f64"]
    for k, name in enumerate(METRIC_F64):
        assert d[name].dtype == np.float64 and d[name].shape == (3,)
        assert d[name][0] == want[k] and d[name][2] == want[k] and d[name][1] == 0.0, (tag, name, d[name], want[k])
    assert d["valid_rows"].dtype == np.int64 and d["valid_rows"].tolist() == [int(g[tag + "_valid_rows"]), 0, int(g[tag + "_valid_rows"])]
    t = host(model.thickness_profile(pred, mm_per_px=mm))
    assert t["delta_d_mm"].dtype == np.float32 and t["delta_d_mm"].shape == (3, H) and t["valid_mask"].dtype == np.bool_
    for i in (0, 2):
        assert np.array_equal(t["delta_d_mm"][i], g[tag + "_delta_d_mm"]), tag
        assert np.array_equal(t["valid_mask"][i], np.unpackbits(g[tag + "_valid_mask"])[:H].astype(bool)), tag
    assert not t["delta_d_mm"][1].any() and not t["valid_mask"][1].any()
    p = host(model.diameter_profile(pred, 1, 2))
    assert p["w_cable_px"].dtype == np.float32 and p["valid"].dtype == np.uint8
    for i in (0, 2):
        assert np.array_equal(p["w_cable_px"][i], g[tag + "_w_cable_px"]) and np.array_equal(p["w_wrap_px"][i], g[tag + "_w_wrap_px"]), tag
        assert np.array_equal(p["valid"][i], np.unpackbits(g[tag + "_valid"])[:H]), tag


@pytest.mark.parametrize("index", range(4))
def test_fixture_defects(torch_cuda, model, model7, golden, index):
    torch = torch_cuda
    g, rows = golden
    row = [r for r in rows if r[1] == "defects"][index]
    tag = row[0]
    m, _ = regenerate(row)
    pred = torch.from_numpy(np.stack([m, np.zeros_like(m), m])).cuda()
    want_f, want_i = g[tag + "_f64"], g[tag + "_i64"]
    for mdl in (model7, model):
        a = host(mdl.analyze_defects(pred))
        for k, name in enumerate(DEFECT_F64):
            assert a[name].dtype == np.float64 and a[name].tolist() == [want_f[k], 0.0, want_f[k]], (tag, name)
        for k, name in enumerate(DEFECT_I64[:3]):
            assert a[name].dtype == np.int64 and a[name].tolist() == [want_i[k], 0, want_i[k]], (tag, name)
        assert a["defect_areas"].dtype == np.int64 and a["defect_areas"].shape == (3, 4)
        if mdl is model7:
            assert a["defect_areas"][0].tolist() == want_i[4:].tolist() and a["total_defect_area"].tolist() == [want_i[3], 0, want_i[3]]
        else:                                       # classes 3..6 are beyond a 3-class engine: area 0
            assert not a["defect_areas"].any() and not a["total_defect_area"].any()
    a = host(model7.analyze_defects(pred, defect_classes=(2, 9, 1)))
    assert a["defect_areas"][0].tolist() == [int((m == 2).sum()), 0, int((m == 1).sum())]
    b = host(model.analyze_defects(pred, hole_min_size=3))
    ref = ge.analyze_defects_np(m, hole_min_size=3)
    assert b["tape_num_holes"][0] == ref["tape_num_holes"] and b["tape_hole_ratio"][2] == ref["tape_hole_ratio"]


# ---- 2. row_widths against the restatement -----------------------------------------------------------------------------
def width_masks(H, W, B, seed):
    r = np.random.default_rng(seed)
    m = (r.integers(0, 4, (B, H, W), dtype=np.uint8) * (r.random((B, H, W)) < 0.15)).astype(np.uint8)
    for b in range(B):
        rows = list(range(H))
        r.shuffle(rows)
        pats = ["empty", "full1", "alt", "col0", "colW", "both", "full2"]
        for y, pat in zip(rows, pats[b % 3:] + pats[:b % 3]):
            m[b, y] = 0
            if pat == "full1":
                m[b, y] = 1
            elif pat == "full2":
                m[b, y] = 2
            elif pat == "alt":
                m[b, y, ::2] = 1; m[b, y, 1::2] = 2
            elif pat == "col0":
                m[b, y, 0] = 1
            elif pat == "colW":
                m[b, y, W - 1] = 2
            elif pat == "both":
                m[b, y, 0] = 1; m[b, y, W - 1] = 1
    return m


@pytest.mark.parametrize("H,W", [(1, 1), (3, 15), (5, 16), (4, 17), (7, 37), (9, 1024), (6, 1040), (5, 2100)])
@pytest.mark.parametrize("B", [1, 5])
def test_row_widths(torch_cuda, model, H, W, B):
    torch = torch_cuda
    m = width_masks(H, W, B, 100 * H + W + B)
    d = torch.from_numpy(m).cuda()

    def check(got, want):
        gw, ga = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert gw.dtype == np.float32 and gw.shape == (B, 2, H) and ga.dtype == np.int64 and ga.shape == (B, 2)
        assert np.array_equal(gw, want[0]) and np.array_equal(ga, want[1].astype(np.int64))

    check(model.row_widths(d, 1, d, 2), ge.row_widths_np(m, 1, m, 2))                    # one tensor, two classes
    check(model.row_widths(d, -1, d, 3), ge.row_widths_np(m, -1, m, 3))                  # match < 0: != 0
    check(model.row_widths(d, 2), ge.row_widths_np(m, 2))                                # one plane, NULL second mask
    other = m[:, ::-1, ::-1].copy()
    check(model.row_widths(d, 0, torch.from_numpy(other).cuda(), -1), ge.row_widths_np(m, 0, other, -1))    # class 0 counts too
    # a mask whose only pixels are column 0, column W - 1, or both
    for cols in ([0], [W - 1], [0, W - 1]):
        e = np.zeros((B, H, W), np.uint8)
        e[:, :, cols] = 7
        check(model.row_widths(torch.from_numpy(e).cuda(), 7), ge.row_widths_np(e, 7))
    # a slice that is not contiguous (and, made contiguous, not 16-byte aligned)
    wide = np.zeros((B, H + 2, W + 3), np.uint8)
    wide[:, 1:H + 1, 1:W + 1] = m
    sl = torch.from_numpy(wide).cuda()[:, 1:H + 1, 1:W + 1]
    assert sl.is_contiguous() == (B * H * W == 1)
    check(model.row_widths(sl, 1, sl, 2), ge.row_widths_np(m, 1, m, 2))
    flat = torch.zeros(B * H * W + 1, dtype=torch.uint8, device="cuda")                 # an odd start address: the bytewise path
    flat[1:] = d.flatten()
    off = flat[1:].view(B, H, W)
    check(model.row_widths(off, 1, d, 2), ge.row_widths_np(m, 1, m, 2))


# ---- 3. width_profile against the restatement ---------------------------------------------------------------------------
def synthetic_widths(H, seed):
    """[F,2,H] float32: random with gaps, all equal, increasing, decreasing, nothing, one row, two rows, no overlap."""
    r = np.random.default_rng(seed)
    f = []
    a = np.floor(r.uniform(1, 900, (2, H))).astype(np.float32)
    a[:, r.random(H) < 0.3] = 0
    a[0, r.random(H) < 0.1] = 0
    f.append(a)
    f.append(np.full((2, H), 37, np.float32))                                           # ties
    f.append(np.stack([np.arange(1, H + 1), 2 * np.arange(1, H + 1) + 1]).astype(np.float32))
    f.append(np.stack([np.arange(H, 0, -1), 3 * np.arange(H, 0, -1)]).astype(np.float32))
    f.append(np.zeros((2, H), np.float32))
    one = np.zeros((2, H), np.float32); one[:, H // 2] = (5, 9)
    f.append(one)
    two = np.zeros((2, H), np.float32); two[:, 0] = (4, 8); two[:, H - 1] = (6, 2)
    f.append(two)
    apart = np.zeros((2, H), np.float32); apart[0, :H // 2] = 11; apart[1, H // 2:] = 13
    f.append(apart)
    return np.stack(f)


@pytest.mark.parametrize("H", [1, 2, 8, 20, 31, 32, 255, 256, 257, 1024, 4096])
@pytest.mark.parametrize("n_taps", [1, 3, 31, 127])
def test_width_profile(torch_cuda, model, H, n_taps):
    torch = torch_cuda
    w = synthetic_widths(H, 7 * H + n_taps)
    taps = ge.gaussian_taps_f32(n_taps)
    assert len(taps) == n_taps
    d = torch.from_numpy(w).cuda()
    ref20 = [ge.width_profile_np(x, taps, 20) for x in w]
    counts = sorted({r[4] for r in ref20})
    if n_taps == 1:
        assert {0, 1, min(2, H), H} <= set(counts)                                       # valid_rows 0, 1, 2 and H all occur
    n0 = ref20[0][4]
    for mvr in sorted({1, 20, max(n0, 1), n0 + 1, H, H + 1}):                           # valid_rows = mvr - 1, mvr, ... among them
        sm, valid, delta, dc, dt, rows = [t.cpu().numpy() for t in model.width_profile(d, 1, mvr, taps)]
        assert sm.dtype == np.float32 and valid.dtype == np.uint8 and delta.dtype == np.float32 and dc.dtype == np.float32
        for i, x in enumerate(w):
            ws, v, mc, mt, n = ge.width_profile_np(x, taps, mvr)
            assert np.array_equal(sm[i], ws) and np.array_equal(valid[i], v.astype(np.uint8)), (H, n_taps, mvr, i)
            assert np.array_equal(delta[i], ws[1] - ws[0])
            assert rows[i] == n and dc[i] == mc and dt[i] == mt, (H, n_taps, mvr, i, n, dc[i], mc, dt[i], mt)
            if n >= mvr:
                assert dc[i] == np.median(ws[0][v]) and dt[i] == np.median(ws[1][v])
            else:
                assert dc[i] == 0 and dt[i] == 0
    no_delta = model.width_profile(d, 1, 1, taps, want_delta=False)
    assert no_delta[2] is None and np.array_equal(no_delta[0].cpu().numpy(), sm)


def test_width_profile_rejections(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    w = torch.zeros((1, 2, 4097), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        model.width_profile(w)                                                           # 4097 rows
    with pytest.raises(ValueError):
        model.width_profile(w[:, :, :64], taps=np.float32([0.5, 0.5]))                   # an even kernel
    with pytest.raises(ValueError):
        model.width_profile(w[:, :, :64], min_valid_rows=0)
    with pytest.raises(ValueError):
        model.diameter_metrics(torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda"), min_valid_rows=0)
    # the C ABI itself: UNETPP_E_INVALID (-1), nothing launched
    model.width_profile(w[:, :, :64].contiguous())                                      # the engine exists from here on
    sm, va = torch.zeros_like(w), torch.zeros((1, 4097), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    t3, t2 = (ctypes.c_float * 3)(0.25, 0.5, 0.25), (ctypes.c_float * 2)(0.5, 0.5)
    skew = (ctypes.c_float * 3)(0.25, 0.5, 0.125)
    call = lambda h, taps, n, mvr: lib.unetpp_width_profile(model._handle, p(w), 1, h, taps, n, mvr, p(sm), p(va), None, p(out), None)
    assert call(4097, t3, 3, 20) == -1
    assert call(64, t2, 2, 20) == -1
    assert call(64, t3, 3, 0) == -1
    assert call(64, skew, 3, 20) == -1
    assert call(0, t3, 3, 20) == -1
    assert call(4096, t3, 3, 20) == 0
    torch.cuda.synchronize()
    assert lib.unetpp_row_widths(model._handle, None, 1, None, 1, 1, 4, 4, p(sm), p(out), None) == -1
    assert lib.unetpp_components_summary(model._handle, p(out), None, 1, 1, 0, p(sm), None) == -1      # capacity < 2


# ---- 4. components_summary against NumPy ----------------------------------------------------------------------------------
def test_components_summary(torch_cuda, model):
    torch = torch_cuda
    hole = mo.make_hole_scene(96, 200, 2, noise=0.02)
    dots = np.zeros((96, 200), np.uint8); dots[::2, ::2] = 2                             # 4,800 one-pixel components
    board = (np.indices((96, 200)).sum(0) % 2 * 2).astype(np.uint8)                      # a checkerboard: one 8-connected component
    frames = np.stack([hole, np.zeros_like(hole), dots, board])
    d = torch.from_numpy(frames).cuda()
    for conn, k in ((8, 8192), (4, 8192), (8, 64), (4, 300)):
        _, num, stats, _ = model.components(d, 2, connectivity=conn, max_components=k)
        n, st = num.cpu().numpy(), stats.cpu().numpy()
        for min_area in (0, 1, 10, 10 ** 6):
            got = model.components_summary(num, stats, min_area).cpu().numpy()
            assert got.dtype == np.int64 and got.shape == (4, 4)
            for i in range(4):
                assert got[i].tolist() == ge.components_summary_np(n[i], st[i], min_area).tolist(), (conn, k, min_area, i)
        exact = [len(cc.components_np(f, conn, 2)[1]) - 1 for f in frames]
        assert model.components_summary(num, None).cpu().numpy()[:, 0].tolist() == exact   # exact beyond the capacity too
        assert model.components_summary(num, None).cpu().numpy()[:, 1:].any() == False
    assert exact[3] == 96 * 200 // 2 and exact[3] > 300                                 # 4-connected: every square its own
    # the methods raise under check=True where a labelling overflowed, and do not under check=False
    with pytest.raises(RuntimeError):
        model.analyze_defects(d, max_components=64)
    a = host(model.analyze_defects(d, max_components=64, check=False))
    assert a["tape_num_components"].tolist() == [len(cc.components_np(f, 8, 2)[1]) - 1 for f in frames]
    with pytest.raises(RuntimeError):
        model.diameter_metrics(d, max_components=64)
    with pytest.raises(RuntimeError):
        model.diameter_profile(d, 1, 2, max_components=64)


# ---- 5. the frame-loop tail -------------------------------------------------------------------------------------------------
def test_measure_frames_and_repeatability(torch_cuda, model7):
    torch = torch_cuda
    from unet_amd import frame_loop
    full = ge.make_wrap_scene(96, 200, 2, classes7=True)
    short = ge.make_wrap_scene(96, 200, 4, tape_start=60, cable_end=45)                 # 0 < valid_rows < 20
    frames = np.stack([full, short, np.zeros_like(full), full])
    pred = torch.from_numpy(frames).cuda()
    recs = frame_loop.measure_frames(model7, pred, mm_per_px=0.04)
    assert [r is None for r in recs] == [False, True, True, False]
    d, a = ge.diameter_metrics_np(full, mm_per_px=0.04), ge.analyze_defects_np(full)
    assert 0 < ge.diameter_metrics_np(short)["valid_rows"] < 20
    for r in (recs[0], recs[3]):
        assert r["diameter"] == d and r["delta_d_mm"] == d["delta_d_mm"] and r["wrap_diameter_mm"] == d["dt_mm"]
        assert type(r["diameter"]["valid_rows"]) is int and type(r["diameter"]["dc_px"]) is float
        want = dict(a, defect_areas=dict(zip((3, 4, 5, 6), a["defect_areas"])))
        assert r["defect_analysis"] == want
    assert all(v > 0 for v in recs[0]["defect_analysis"]["defect_areas"].values())
    # two calls, identical bits
    again = frame_loop.measure_frames(model7, pred, mm_per_px=0.04)
    assert again == recs
    big = torch.from_numpy(np.stack([ge.make_wrap_scene(448, 800, 0), ge.make_wrap_scene(448, 800, 1)])).cuda()
    for fn in (model7.diameter_metrics, model7.analyze_defects, model7.thickness_profile, lambda p: model7.diameter_profile(p, 1, 2)):
        x, y = host(fn(big)), host(fn(big))
        assert all(x[k].tobytes() == y[k].tobytes() for k in x)
