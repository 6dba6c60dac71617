"""The ROI and full-frame 3-class loops on the device (unet_amd/roi_loop.py, include/unetpp_roi.h) against their NumPy forms,
bit for bit, and against the fixtures made from the reference's own functions (tests/golden/roi_scenes.npz).
Run on the GPU box:  python -m pytest tests/test_gpu_roi_loop.py -m gpu"""
import numpy as np
import pytest

from conftest import load_golden
from unet_amd import edges as ed
from unet_amd import robust as rb
from unet_amd import roi_loop as rl

pytestmark = pytest.mark.gpu

# 2 x 32 x 128 aligned, one byte off, four bytes off; 3 x 33 x 129; 2 x 18 x 20
PLACEMENTS = [((2, 32, 128), 0), ((2, 32, 128), 1), ((2, 32, 128), 4), ((3, 33, 129), 0), ((2, 18, 20), 0)]
GEOMETRY = dict(min_area=20, min_aspect=1.0, wide_width=10, edge_lo=0.1, edge_hi=0.9, large_area=150)
PRIMARY = dict(min_area=20, min_aspect=0.5)
K = 1024


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: the rules need none


@pytest.fixture(scope="module")
def golden():
    g = load_golden("roi_scenes")
    return {k: g[k] for k in g.files}


def place(torch, a, off):
    """`a` on the device as a contiguous view `off` bytes behind a 16-byte aligned address (off a multiple of the item size)."""
    a = np.ascontiguousarray(a)
    off = off if off % a.dtype.itemsize == 0 else a.dtype.itemsize * (off // a.dtype.itemsize + 1)
    buf = torch.empty(a.nbytes + 32, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 16 + off
    v = buf[start:start + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == off % 16 and v.is_contiguous()
    return v


def blocks(shape, r, classes=3):
    B, H, W = shape
    coarse = r.integers(0, classes, (B, (H + 7) // 8, (W + 7) // 8), dtype=np.uint8)
    m = np.repeat(np.repeat(coarse, 8, 1), 8, 2)[:, :H, :W].copy()
    s = r.random(shape) < 0.02
    m[s] = r.integers(0, classes, int(s.sum()), dtype=np.uint8)
    return m


def frames_of(shape, r):
    B, H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    g = np.stack([96 + 60 * np.sin(x / (5.0 + b)) * np.cos(y / 4.0) + 40 * ((x // 16 + y // 8 + b) % 2) for b in range(B)])
    g = np.clip(g + r.normal(0, 6, shape), 0, 255)
    return np.clip(g[..., None] + r.integers(-40, 40, shape + (3,)), 0, 255).astype(np.uint8)


def probs_of(shape, r, C=3):
    B, H, W = shape
    p = r.dirichlet(np.ones(C) * 0.7, (B, H, W)).astype(np.float32)
    p = np.ascontiguousarray(p.transpose(0, 3, 1, 2))
    p.reshape(-1)[r.integers(0, p.size, 8)] = 0.0
    p.reshape(-1)[r.integers(0, p.size, 8)] = 1.0
    return p


def roi_table(B, W):
    rows = [(W // 5, W - W // 4, 1, 1), (3, 3, 1, 0), (0, W, 0, 1)]
    return np.int32([rows[b % 3] for b in range(B)])


def same_bits(got, want):
    got, want = np.ascontiguousarray(got.cpu().numpy()), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    assert got.tobytes() == want.tobytes(), f"{int((got != want).sum())} of {got.size} values differ"


# ---- 1. every call equals its NumPy form, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,off", PLACEMENTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"off{v}")
def test_device_equals_numpy(torch_cuda, model, shape, off):
    torch = torch_cuda
    r = np.random.default_rng(shape[1] * 1000 + shape[2])
    B, H, W = shape
    frames = frames_of(shape, r)
    gray = ed.bgr_to_gray_np(frames)
    edges = np.stack([ed.canny_np(g, 50, 150) for g in gray])
    edges[-1] = 0
    same_bits(rl.roi_from_edges(model, place(torch, edges, off)), np.stack([rl.roi_from_edges_np(e) for e in edges]))
    same_bits(rl.detect_roi(model, place(torch, frames, off)), np.stack([rl.detect_roi_np(f) for f in frames]))
    roi = roi_table(B, W)
    for size in ((24, 40), 16):
        same_bits(rl.crop_resize(model, place(torch, frames, off), place(torch, roi, off), size),
                  np.stack([rl.crop_resize_np(f, q, size) for f, q in zip(frames, roi)]))
    for C in (3, 5):
        probs = probs_of(shape, r, C)
        want = [rl.adaptive_thresholds_np(p) for p in probs]
        got = rl.adaptive_thresholds(model, place(torch, probs, off))
        for k in range(3):
            same_bits(got[k], np.stack([w[k] for w in want]))
        thr = np.float32([[0.5, 0.55, 0.2], [0.8, 0.3, 0.35], [0.1, 0.1, 0.05]])[np.arange(B) % 3]
        for table in (thr, np.stack([w[0] for w in want])):
            c, t = rl.ultra_strict(model, place(torch, probs, off), place(torch, table, off))
            wm = [rl.ultra_strict_np(p, q) for p, q in zip(probs, table)]
            same_bits(c, np.stack([w[0] for w in wm]))
            same_bits(t, np.stack([w[1] for w in wm]))
    mask = blocks(shape, r)
    same_bits(rl.refine_by_geometry(model, place(torch, mask, off), match_class=1, out_value=7, max_components=K, **GEOMETRY),
              np.stack([rl.refine_by_geometry_np(f == 1, out_value=7, **GEOMETRY) for f in mask]))
    same_bits(rl.select_primary(model, place(torch, mask, off), match_class=2, max_components=K, **PRIMARY),
              np.stack([rl.select_primary_np(f == 2, **PRIMARY) for f in mask]))
    m0, m1 = (mask == 1).astype(np.uint8), (mask == 2).astype(np.uint8)
    for frame_hw in ((47, 150), (H, W)):
        q = roi_table(B, frame_hw[1])
        g0, g1 = rl.paste_masks(model, (place(torch, m0, off), place(torch, m1, off)), place(torch, q, off), frame_hw)
        same_bits(g0, np.stack([rl.paste_mask_np(m, x, frame_hw) for m, x in zip(m0, q)]))
        same_bits(g1, np.stack([rl.paste_mask_np(m, x, frame_hw) for m, x in zip(m1, q)]))


@pytest.mark.parametrize("shape", [(2, 40, 20), (2, 18, 640)], ids=lambda s: "x".join(map(str, s)))
def test_projection_shapes(torch_cuda, model, shape):
    """W = 20: the box sum has 30 entries, more than the frame has columns; 2 x 18 x 640: three blocks of columns."""
    torch = torch_cuda
    B, H, W = shape
    frames = np.stack([rl.make_projection_frame(H, W, 5 + b, kind) for b, kind in zip(range(B), ("cable", "line"))])
    got = rl.detect_roi(model, torch.from_numpy(frames).cuda())
    same_bits(got, np.stack([rl.detect_roi_np(f) for f in frames]))
    r = np.random.default_rng(W)
    edges = ((r.random(shape) < 0.2) * 255).astype(np.uint8)
    edges[:, :, W // 2:] = 0
    same_bits(rl.roi_from_edges(model, torch.from_numpy(edges).cuda()), np.stack([rl.roi_from_edges_np(e) for e in edges]))


@pytest.mark.parametrize("name,kind,H,W,seed", rl.PROJECTION_SCENES)
def test_projection_fixtures(torch_cuda, model, golden, name, kind, H, W, seed):
    torch = torch_cuda
    frame = rl.make_projection_frame(H, W, seed, kind)
    roi = rl.detect_roi(model, torch.from_numpy(frame[None]).cuda()).cpu().numpy()[0]
    assert np.array_equal(roi[:2], golden[f"{name}_roi"]) and roi[3] == (roi[1] > roi[0]), (name, roi)


def test_a_frame_that_is_not_valid_gives_zero_masks(torch_cuda, model):
    torch = torch_cuda
    frame = rl.make_projection_frame(40, 20, 6, "line")                   # a single edge column at W = 20: x_min == x_max
    frames = torch.from_numpy(np.stack([frame, rl.make_projection_frame(40, 20, 5, "cable")])).cuda()
    roi = rl.detect_roi(model, frames)
    assert roi.cpu().numpy()[:, 3].tolist() == [0, 1]
    crop = rl.crop_resize(model, frames, roi, 32)
    assert not crop[0].any() and crop[1].any()
    ones = torch.ones((2, 32, 32), dtype=torch.uint8, device="cuda")
    c, t = rl.paste_masks(model, (ones, ones), roi, (40, 20))
    assert not c[0].any() and not t[0].any() and c[1].any()
    probs = torch.from_numpy(np.stack([rl.make_probs(192, 192, 0)] * 2)).cuda()
    c, t, counts, _ = rl.postprocess_roi(model, probs, roi, (40, 20))
    counts = counts.cpu().numpy()
    assert not c[0].any() and not t[0].any() and counts[0, :2].tolist() == [0, 0] and counts[1, 0] > 0 and counts[1, 1] > 0


# ---- 2. the fixtures from the reference's own functions -----------------------------------------------------------------------------
def unpack(g, key, shape):
    return np.unpackbits(g[key])[:shape[0] * shape[1]].reshape(shape)


def test_thresholds_and_masks_equal_the_reference(torch_cuda, model, golden):
    torch = torch_cuda
    probs = np.stack([rl.make_probs(S, S, seed, c, t, b) for _, S, seed, c, t, b in rl.PROB_SCENES])
    S = probs.shape[2]
    dev = torch.from_numpy(probs).cuda()
    thr = rl.adaptive_thresholds(model, dev)[0]
    ref = np.stack([golden[f"{n[0]}_thr_ref"] for n in rl.PROB_SCENES])
    same_bits(thr, np.stack([golden[f"{n[0]}_thr_np"] for n in rl.PROB_SCENES]))
    assert rl.ulp_distance(thr.cpu().numpy(), ref) <= int(golden["threshold_ulps"]) + 1
    for table in (thr, torch.from_numpy(ref).cuda()):                     # the reference's own table, and the device's
        c, t = rl.ultra_strict(model, dev, table)
        for i, row in enumerate(rl.PROB_SCENES):
            assert np.array_equal(c[i].cpu().numpy(), unpack(golden, f"{row[0]}_cable", (S, S))), row[0]
            assert np.array_equal(t[i].cpu().numpy(), unpack(golden, f"{row[0]}_tape", (S, S))), row[0]


def test_roi_loop_after_the_network_equals_the_reference(torch_cuda, model, golden):
    torch = torch_cuda
    names = [row[0] for row in rl.PROB_SCENES]
    probs = np.stack([rl.make_probs(S, S, seed, c, t, b) for _, S, seed, c, t, b in rl.PROB_SCENES])
    roi = torch.from_numpy(np.int32([rl.LOOP_ROIS[n] for n in names])).cuda()
    cable, tape, counts, _ = rl.postprocess_roi(model, torch.from_numpy(probs).cuda(), roi, rl.LOOP_FRAME)
    counts = counts.cpu().numpy()
    n = probs.shape[2] * probs.shape[3]
    for i, name in enumerate(names):
        assert np.array_equal(cable[i].cpu().numpy(), unpack(golden, f"{name}_full_cable", rl.LOOP_FRAME)), name
        assert np.array_equal(tape[i].cpu().numpy(), unpack(golden, f"{name}_full_tape", rl.LOOP_FRAME)), name
        assert [counts[i, 0] / n, counts[i, 1] / n] == golden[f"{name}_coverage"].tolist(), name
    assert cable.any() and tape.any()


def test_full_loop_after_the_network_equals_the_reference(torch_cuda, model, golden):
    torch = torch_cuda
    names = [row[0] for row in rl.PROB_SCENES]
    S = rl.PROB_SCENES[0][1]
    c0 = torch.from_numpy(np.stack([unpack(golden, f"{n}_ta_cable", (S, S)) for n in names])).cuda()
    t0 = torch.from_numpy(np.stack([unpack(golden, f"{n}_ta_tape", (S, S)) for n in names])).cuda()
    cable, tape, cs, ts, table = rl.postprocess_3class_full(model, c0, t0, rl.LOOP_FRAME)
    table = table.cpu().tolist()
    for i, name in enumerate(names):
        assert np.array_equal(cable[i].cpu().numpy(), unpack(golden, f"{name}_f3_cable", rl.LOOP_FRAME)), name
        assert np.array_equal(tape[i].cpu().numpy(), unpack(golden, f"{name}_f3_tape", rl.LOOP_FRAME)), name
        r = table[i]
        assert r[:3] + [int(r[3]) / (S * S), int(r[4]) / (S * S)] == golden[f"{name}_f3_metrics"].tolist(), name
    # a frame without a cable keeps its tape undilated (the reference's `if mask_cable_small.sum() > 0`)
    none = torch.zeros_like(c0)
    _, _, cs, ts, _ = rl.postprocess_3class_full(model, none, t0, rl.LOOP_FRAME)
    want = [rl.postprocess_3class_full_np(np.zeros((S, S), np.uint8), t, rl.LOOP_FRAME)[3] for t in t0.cpu().numpy()]
    assert not cs.any() and np.array_equal(ts.cpu().numpy(), np.stack(want)) and ts.any()


@pytest.mark.parametrize("name,kind", rl.COMPONENT_SCENES)
def test_component_rules_with_the_defaults(torch_cuda, model, golden, name, kind):
    torch = torch_cuda
    m = rl.component_scene(kind)
    dev = torch.from_numpy(np.stack([m, m[:, ::-1].copy()])).cuda()
    g = rl.refine_by_geometry(model, dev)
    p = rl.select_primary(model, dev)
    assert np.array_equal(g[0].cpu().numpy(), np.unpackbits(golden[f"{name}_geometry"]).reshape(m.shape))
    assert np.array_equal(p[0].cpu().numpy(), np.unpackbits(golden[f"{name}_primary"]).reshape(m.shape))
    same_bits(g[1], rl.refine_by_geometry_np(m[:, ::-1]))
    same_bits(p[1], rl.select_primary_np(m[:, ::-1]))


# ---- 3. argument checks that need the device ----------------------------------------------------------------------------------------
def test_argument_checks(torch_cuda, model):
    torch = torch_cuda
    u8 = torch.zeros((1, 16, 16), dtype=torch.uint8, device="cuda")
    roi = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="at least 3 classes"):
        rl.adaptive_thresholds(model, torch.zeros((1, 2, 16, 16), device="cuda"))
    with pytest.raises(RuntimeError, match="int32 CUDA tensor"):
        rl.crop_resize(model, torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda"), roi.to(torch.int64))
    with pytest.raises(RuntimeError, match=r"\[2,4\]"):
        rl.paste_masks(model, (torch.cat([u8, u8]), torch.cat([u8, u8])), roi, (16, 16))
    with pytest.raises(RuntimeError, match=r"\[1,3\]"):
        rl.ultra_strict(model, torch.zeros((1, 3, 16, 16), device="cuda"), torch.zeros((1, 4), device="cuda"))
    with pytest.raises(ValueError, match="NaN"):
        rl.refine_by_geometry(model, u8, edge_lo=float("nan"))
    with pytest.raises(ValueError, match="size"):
        rl.crop_resize(model, torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda"), roi, 0)
    # the C entries answer bad arguments with UNETPP_E_UNSUPPORTED (-2): ValueError through _call
    f32 = torch.zeros((1, 3, 16, 16), device="cuda")
    t3 = torch.zeros((1, 3), device="cuda")
    ws = torch.empty(1 << 12, dtype=torch.uint8, device="cuda")
    for name, args in (("unetpp_roi_from_edges_u8", (u8, 1, 0, 16, roi, ws)),
                       ("unetpp_roi_crop_resize_u8", (u8, 1, 16, 16, 5, roi, u8, 4, 4)),
                       ("unetpp_roi_adaptive_thresholds_f32", (f32, 1, 2, 16, 16, t3, t3, t3, ws)),
                       ("unetpp_roi_ultra_strict_f32", (f32, 1, 3, 16, 16, t3, u8, u8)),                  # the two masks overlap
                       ("unetpp_roi_paste_masks_u8", (u8, u8, 1, 16, 16, roi, u8, u8, 16, 16))):         # outputs alias inputs
        with pytest.raises(ValueError):
            model._call(name, *args, stream_of=u8)


# ---- 4. the whole loops ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(torch_cuda, syn):
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=False, max_batch=2, max_hw=(64, 64)).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    return m.eval()


@pytest.fixture(scope="module")
def sharp_net(torch_cuda, syn):
    """The same network with its head scaled: probabilities confident enough for ultra_strict_threshold to keep pixels."""
    from unet_amd.nested_unet import NestedUNet
    sd = dict(syn.make_state_dict(3, 3, False, 2))
    sd["final.weight"] = sd["final.weight"] * 8
    sd["final.bias"] = sd["final.bias"] * 8
    m = NestedUNet(3, deep_supervision=False, max_batch=2, max_hw=(64, 64)).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    return m.eval()


def test_process_frames_roi_equals_the_numpy_chain(torch_cuda, sharp_net, syn):
    torch = torch_cuda
    net = sharp_net
    from unet_amd import frame_loop
    frames = syn.make_frames_u8(2, 120, 200, "smooth", 77)
    geometry = dict(min_area=4, min_aspect=0.5, wide_width=20, large_area=200)
    for use_roi in (True, False):
        cable, tape, metrics, roi = frame_loop.process_frames_roi(net, frames, use_roi=use_roi, input_size=64, **geometry)
        assert cable.shape == (2, 120, 200) and cable.dtype == torch.uint8 and len(metrics) == 2
        want_roi = np.stack([rl.detect_roi_np(f) for f in frames]) if use_roi else rl.full_roi_np(2, 200)
        same_bits(roi, want_roi)
        x = torch.from_numpy(frames).cuda()
        crop = rl.crop_resize(net, x, roi, 64)
        same_bits(crop, np.stack([rl.crop_resize_np(f, q, 64) for f, q in zip(frames, want_roi)]))
        probs = net.predict_proba(crop).cpu().numpy()                    # the device's own probabilities: the chain around them
        strict = [rl.ultra_strict_np(p, rl.adaptive_thresholds_np(p)[0]) for p in probs]
        assert sum(int(c.sum()) + int(t.sum()) for c, t in strict) > 50, "the chain needs pixels to say anything"
        for f in range(2):
            wc, wt, cov_c, cov_t, _ = rl.postprocess_roi_np(probs[f], want_roi[f], (120, 200), **geometry)
            assert np.array_equal(cable[f].cpu().numpy(), wc) and np.array_equal(tape[f].cpu().numpy(), wt), (use_roi, f)
            assert metrics[f] == {"cable_coverage": cov_c, "tape_coverage": cov_t, "roi": (int(want_roi[f, 0]), int(want_roi[f, 1]))}
        print(f"process_frames_roi(use_roi={use_roi}): roi {want_roi[:, :2].tolist()} mask pixels cable {int(cable.sum())} tape {int(tape.sum())}")
        again = frame_loop.process_frames_roi(net, frames, use_roi=use_roi, input_size=64, **geometry)
        assert torch.equal(again[0], cable) and torch.equal(again[1], tape) and again[2] == metrics and torch.equal(again[3], roi)


def test_process_frames_3class_full_equals_the_numpy_chain(torch_cuda, net, syn):
    torch = torch_cuda
    from unet_amd import frame_loop
    frames = syn.make_frames_u8(2, 120, 200, "smooth", 77)
    cfg = dict(t_cable=0.34, t_tape=0.34, bg_margin=0.0, cc_min_area_cable=4, cc_min_area_tape=2, cable_min_aspect=0.1, tape_dilate_px=3)
    cable, tape, metrics, pred = frame_loop.process_frames_3class_full(net, frames, input_size=64, **cfg)
    resized = net.resize_frames(torch.from_numpy(frames).cuda(), (64, 64))
    cs, ts = net.segment_thresholded(resized, "thresholded_argmax", cfg["t_cable"], cfg["t_tape"], cfg["bg_margin"])
    cs, ts = cs.cpu().numpy(), ts.cpu().numpy()
    assert cs.sum() > 50 and ts.sum() > 50, "the chain needs both classes to say anything"
    for f in range(2):
        wc, wt, c1, t1, m = rl.postprocess_3class_full_np(cs[f], ts[f], (120, 200), cfg["cc_min_area_cable"], cfg["cc_min_area_tape"],
                                                          cfg["cable_min_aspect"], cfg["tape_dilate_px"])
        assert np.array_equal(cable[f].cpu().numpy(), wc) and np.array_equal(tape[f].cpu().numpy(), wt), f
        assert metrics[f] == m, (f, metrics[f], m)
        assert np.array_equal(pred[f].cpu().numpy(), np.where(t1 > 0, 2, c1))
    print(f"process_frames_3class_full: mask pixels at 64x64 cable {int(cs.sum())} tape {int(ts.sum())}; kept at frame size {int(cable.sum())} {int(tape.sum())}")
    again = frame_loop.process_frames_3class_full(net, frames, input_size=64, **cfg)
    assert torch.equal(again[0], cable) and torch.equal(again[1], tape) and again[2] == metrics and torch.equal(again[3], pred)
    plain = frame_loop.process_frames_3class_full(net, frames, input_size=64, use_cc_filter=False, **cfg)
    assert np.array_equal(plain[0].cpu().numpy(), np.stack([rb.resize_nearest_np(c, (200, 120)) for c in cs]))
