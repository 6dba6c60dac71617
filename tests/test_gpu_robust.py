"""The robust loop's mask rules on the device (unetpp_distance_transform_u8, unetpp_components_best_cable,
unetpp_roi_limit_u8, unetpp_row_width_median and unet_amd/robust.py's functions built on them) against the NumPy forms and
the fixtures made from the reference's own functions (tests/golden/robust_scenes.npz).  Integer arithmetic, float32 values
compared as bits, correctly rounded float64 expressions: exact equality, no tolerance.
Run on the GPU box:  python -m pytest tests/test_gpu_robust.py -m gpu"""
import hashlib
import json

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import robust as rb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: the mask rules need none


@pytest.fixture(scope="module")
def golden():
    g = load_golden("robust_scenes")
    return g, [tuple(r) for r in g["cases"].tolist()]


def regenerate(row):
    tag, H, W, seed, opts, params, sha_c, sha_t = row
    c, t = rb.make_robust_scene(int(H), int(W), int(seed), **json.loads(opts))
    assert hashlib.sha256(np.ascontiguousarray(c).tobytes()).hexdigest() == sha_c, tag
    assert hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest() == sha_t, tag
    return tag, c, t, json.loads(params)


def unpack(g, key, shape):
    return np.unpackbits(g[key])[:shape[0] * shape[1]].reshape(shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def odd_view(torch, a):
    """`a` on the device as a contiguous view that starts one byte behind an allocation."""
    buf = torch.empty(a.size + 1, dtype=torch.uint8, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 2 == 1 and v.is_contiguous()
    return v


def random_batch(shape, seed, golden):
    """uint8 [B,H,W] with values 0, 1, 2: frames of several zero densities, an all-non-zero and an all-zero one where the
    batch has room; at 2 x 96 x 200 the fixture's two cable masks."""
    B, H, W = shape
    if (H, W) == (96, 200):
        return np.stack([regenerate(r)[1] for r in golden[1] if (int(r[1]), int(r[2])) == (96, 200)])
    r = np.random.default_rng(seed)
    dens = [0.1, 0.002, 0.5]
    m = np.stack([(r.random((H, W)) >= dens[i % 3]).astype(np.uint8) * r.integers(1, 3, (H, W), dtype=np.uint8) for i in range(B)])
    if B >= 3:
        m[1], m[2] = 2, 0
    return m


# ---- 1. the distance map and the fused ring ------------------------------------------------------------------------------
SHAPES = [(2, 37, 53), (1, 1, 70), (1, 70, 1), (3, 64, 64), (2, 96, 200)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distance_and_ring_equal_numpy(torch_cuda, model, golden, shape):
    torch = torch_cuda
    m = random_batch(shape, 11 + shape[1], golden)
    dev = torch.from_numpy(m).cuda()
    other = (np.random.default_rng(5).random(m.shape) < 0.7).astype(np.uint8) * 3
    for metric in ("l2", "l1", "c"):
        for match, invert in ((-1, False), (-1, True), (2, False)):
            nz = ((m != 0) if match < 0 else (m == match)) != invert
            want = np.stack([rb.distance_transform_np(f, metric) for f in nz])
            got = rb.distance_transform(model, dev, match, invert, metric)
            assert got.dtype == torch.float32 and np.array_equal(bits(got.cpu().numpy()), bits(want)), (shape, metric, match, invert)
    # the ring: alone (the search is cut off beyond hi), beside the map, with and without the second mask, fractional bounds
    nz = m == 0
    d = np.stack([rb.distance_transform_np(f) for f in nz])
    for lo, hi, second in ((2, 20, True), (0, 3, False), (1.5, 2.75, True), (0, 1e9, True), (3, 1, False), (8192, 8192, False)):
        want = np.stack([rb.ring_np(f, o if second else None, lo, hi, out_value=7) for f, o in zip(nz, other)])
        o_dev = torch.from_numpy(other).cuda() if second else None
        alone = rb.distance_ring(model, dev, o_dev, lo, hi, out_value=7)
        ring, dist = rb.distance_ring(model, dev, o_dev, lo, hi, out_value=7, return_distance=True)
        assert np.array_equal(alone.cpu().numpy(), want) and np.array_equal(ring.cpu().numpy(), want), (shape, lo, hi, second)
        assert np.array_equal(bits(dist.cpu().numpy()), bits(d))
    want = np.stack([rb.ring_np(f, o == 3, 1, 4) for f, o in zip(m != 0, other)])
    assert np.array_equal(rb.distance_ring(model, dev, torch.from_numpy(other).cuda(), 1, 4, invert=False, match1=3).cpu().numpy(), want)


def test_views_at_an_odd_byte_offset(torch_cuda, model):
    """37 x 53: the width alone selects the byte path.  32 x 128: every size is a multiple of 16, so the pointer decides."""
    torch = torch_cuda
    for shape in ((2, 37, 53), (2, 32, 128)):
        r = np.random.default_rng(3)
        m = (r.random(shape) >= 0.05).astype(np.uint8)
        o = (r.random(shape) < 0.6).astype(np.uint8)
        a, b = odd_view(torch, m), odd_view(torch, o)
        want = np.stack([rb.distance_transform_np(f) for f in m])
        assert np.array_equal(bits(rb.distance_transform(model, a).cpu().numpy()), bits(want)), shape
        ring = rb.distance_ring(model, a, b, 1, 3, invert=False)
        assert np.array_equal(ring.cpu().numpy(), np.stack([rb.ring_np(f, g, 1, 3) for f, g in zip(m, o)])), shape
        assert np.array_equal(rb.roi_limit(model, b, a, 2).cpu().numpy(), np.stack([rb.roi_limit_np(g, f, 2) for f, g in zip(m, o)])), shape


def test_wide_rows_and_far_zeros(torch_cuda, model):
    """A row above 16,384 pixels (the row pass then asks for more LDS than the default limit) and distances beyond the cap's
    reach of 8192 columns."""
    torch = torch_cuda
    m = np.ones((2, 1, 20000), np.uint8)
    m[0, 0, 3] = 0
    m[1, 0, [9000, 9001, 19999]] = 0
    want = np.stack([rb.distance_transform_np(f) for f in m])
    assert want[0].max() == np.float32(8192.0) and want[0, 0, 8000] < 8192 and want[1, 0, 14000] < 8192
    got = rb.distance_transform(model, torch.from_numpy(m).cuda())
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    tall = np.ones((1, 9000, 3), np.uint8)
    tall[0, 8999, 1] = 0
    want = rb.distance_transform_np(tall[0], "c")
    assert want[0, 1] == np.float32(8192.0) and want[1000, 1] == np.float32(7999.0)
    assert np.array_equal(bits(rb.distance_transform(model, torch.from_numpy(tall).cuda(), metric="c").cpu().numpy()[0]), bits(want))


# ---- 2. the fixtures from the reference's own functions ------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(512, 512), (96, 200), (33, 57)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rules_equal_the_fixture(torch_cuda, model, golden, hw):
    torch = torch_cuda
    g, rows = golden
    scenes = [regenerate(r) for r in rows if (int(r[1]), int(r[2])) == hw]
    assert len(scenes) == 2
    P = scenes[0][3]
    assert scenes[1][3] == P
    tags = [s[0] for s in scenes]
    c = torch.from_numpy(np.stack([s[1] for s in scenes])).cuda()
    t = torch.from_numpy(np.stack([s[2] for s in scenes])).cuda()
    want = lambda key: np.stack([unpack(g, tag + key, hw) for tag in tags])
    best = rb.keep_best_cable(model, c, P["min_area"], P["min_h_ratio"], P["min_aspect"], P["max_w_ratio"])
    assert best.dtype == torch.uint8 and np.array_equal(best.cpu().numpy(), want("_best_raw"))
    ring = rb.restrict_tape_to_ring(model, t, best, P["band_out"], P["band_in"], P["tape_min_area"])
    assert np.array_equal(ring.cpu().numpy(), want("_ring_raw"))
    assert np.array_equal(rb.roi_limit(model, t, best, P["pad"]).cpu().numpy(), want("_roi_raw"))
    cable, tape = rb.postprocess_robust(model, c, t, close_ksize=P["close_ksize"], min_area=P["min_area"], min_h_ratio=P["min_h_ratio"],
                                        min_aspect=P["min_aspect"], max_w_ratio=P["max_w_ratio"], band_out=P["band_out"], band_in=P["band_in"],
                                        tape_min_area=P["tape_min_area"], pad=P["pad"])
    assert np.array_equal(cable.cpu().numpy(), want("_cable")) and np.array_equal(tape.cpu().numpy(), want("_tape"))
    got = rb.measure_robust(model, cable, tape)
    for tag, rec in zip(tags, got):
        assert [rec[f] for f in rb.MEASURE_FIELDS] == g[tag + "_measure"].tolist(), tag
        assert all(isinstance(v, float) for v in rec.values())
    # two runs give identical bytes
    again = rb.postprocess_robust(model, c, t, close_ksize=P["close_ksize"], min_area=P["min_area"], min_h_ratio=P["min_h_ratio"],
                                  min_aspect=P["min_aspect"], max_w_ratio=P["max_w_ratio"], band_out=P["band_out"], band_in=P["band_in"],
                                  tape_min_area=P["tape_min_area"], pad=P["pad"])
    assert torch.equal(again[0], cable) and torch.equal(again[1], tape)
    assert torch.equal(rb.distance_transform(model, c, invert=True), rb.distance_transform(model, c, invert=True))


def test_an_empty_cable_gives_all_zeros(torch_cuda, model):
    torch = torch_cuda
    r = np.random.default_rng(9)
    tape = (r.random((2, 40, 64)) < 0.5).astype(np.uint8)
    cable = np.zeros_like(tape)
    cable[1, 5:30, 30:34] = 1                                     # frame 0 has no cable, frame 1 has one
    td, cd = torch.from_numpy(tape).cuda(), torch.from_numpy(cable).cuda()
    # band_out beyond 8192: the distance of a frame without a zero pixel lies inside the band, the ROI step empties it
    ring = rb.restrict_tape_to_ring(model, td, cd, 10 ** 6, 0, 1).cpu().numpy()
    assert not ring[0].any() and ring[1].any()
    assert np.array_equal(ring, np.stack([rb.restrict_tape_to_ring_np(a, b, 10 ** 6, 0, 1) for a, b in zip(tape, cable)]))
    roi = rb.roi_limit(model, td, cd, 3).cpu().numpy()
    assert not roi[0].any() and np.array_equal(roi[1], rb.roi_limit_np(tape[1], cable[1], 3))
    rec = rb.measure_robust(model, cd, td)
    assert rec[0]["dc_px"] == 0.0 and rec[0]["delta_d_px"] == 0.0 and rec[0]["dt_px"] == rb.row_width_median_np(tape[0])
    assert rec[1] == rb.measure_diameters_np(cable[1], tape[1])
    best, kept = rb.postprocess_robust(model, torch.zeros_like(cd), td)
    assert not best.any() and not kept.any()


def test_medians_of_tall_frames_and_even_counts(torch_cuda, model):
    torch = torch_cuda
    r = np.random.default_rng(4)
    a = np.zeros((2, 5000, 40), np.uint8)                         # above the 4096 rows of unetpp_width_profile
    for f in range(2):
        for y in range(0, 5000 - f, 2):
            x0, n = int(r.integers(0, 20)), int(r.integers(1, 20))
            a[f, y, x0] = a[f, y, x0 + n - 1] = 1
    dev = torch.from_numpy(a).cuda()
    got = rb.measure_robust(model, dev, dev.flip(0))
    for f in range(2):
        assert got[f] == rb.measure_diameters_np(a[f], a[1 - f])


def test_more_components_than_max_components_raises(torch_cuda, model):
    torch = torch_cuda
    m = np.zeros((1, 32, 32), np.uint8)
    m[0, ::2, ::2] = 1                                            # 256 components
    dev = torch.from_numpy(m).cuda()
    with pytest.raises(RuntimeError, match="raise max_components"):
        rb.keep_best_cable(model, dev, 0, 0.0, 0.0, 1.0, max_components=64)
    assert not rb.keep_best_cable(model, dev, 0, 0.0, 0.0, 1.0, max_components=64, check=False).any()
    with pytest.raises(RuntimeError, match="raise max_components"):
        rb.restrict_tape_to_ring(model, dev, torch.from_numpy(np.roll(m, 1, 2)).cuda(), 3, 0, 0, max_components=64)
    with pytest.raises(RuntimeError, match="raise max_components"):
        rb.postprocess_robust(model, dev, dev, close_ksize=1, max_components=64)


# ---- 3. arguments ----------------------------------------------------------------------------------------------------------
def test_host_tensors_wrong_dtypes_and_bad_arguments_are_refused(torch_cuda, model):
    torch = torch_cuda
    host = torch.zeros((1, 16, 16), dtype=torch.uint8)
    dev = host.cuda()
    text = "mask must be a uint8 CUDA tensor [B,H,W]"
    calls = [lambda t: rb.distance_transform(model, t), lambda t: rb.distance_ring(model, t, None), lambda t: rb.keep_best_cable(model, t),
             lambda t: rb.restrict_tape_to_ring(model, t, dev), lambda t: rb.roi_limit(model, t, dev), lambda t: rb.postprocess_robust(model, t, dev),
             lambda t: rb.measure_robust(model, t, dev), lambda t: rb.unletterbox_masks(model, t, rb.letterbox_plan(16, 16, 16))]
    for call in calls:
        for bad in (host, dev.to(torch.int32), dev[0]):
            with pytest.raises(RuntimeError) as err:
                call(bad)
            assert str(err.value) == text
    with pytest.raises(RuntimeError) as err:
        rb.letterbox(model, host)
    assert str(err.value) == "frames must be a uint8 CUDA tensor [B,H,W,C]"
    with pytest.raises(RuntimeError, match="does not match"):
        rb.roi_limit(model, dev, torch.zeros((1, 16, 8), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="metric"):
        rb.distance_transform(model, dev, metric="l3")
    with pytest.raises(ValueError, match="out_value"):
        rb.distance_ring(model, dev, None, out_value=0)
    with pytest.raises(ValueError, match="pad"):
        rb.roi_limit(model, dev, dev, -1)
    # the C entries answer bad arguments with UNETPP_E_UNSUPPORTED (-2): ValueError through _call
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    out = torch.empty((1, 16, 16), dtype=torch.float32, device="cuda")
    for args in ((dev, -1, 0, 1, 16, 16, 9, out, None, -1, 0.0, 0.0, 1, None, ws),           # unknown metric
                 (dev, -1, 0, 1, 0, 16, 2, out, None, -1, 0.0, 0.0, 1, None, ws),            # h = 0
                 (dev, 256, 0, 1, 16, 16, 2, out, None, -1, 0.0, 0.0, 1, None, ws),          # match class
                 (dev, -1, 0, 1, 16, 16, 2, None, None, -1, 0.0, 0.0, 1, None, ws),          # neither output
                 (dev, -1, 0, 1, 16, 16, 2, None, None, -1, 0.0, 0.0, 0, dev, ws)):          # out_value 0
        with pytest.raises(ValueError):
            model._call("unetpp_distance_transform_u8", *args, stream_of=dev)
    with pytest.raises(ValueError):
        model._call("unetpp_roi_limit_u8", dev, dev, 1, 16, 16, -1, dev, ws, stream_of=dev)
    with pytest.raises(ValueError):
        model._call("unetpp_row_width_median", out, 1, 0, ws, stream_of=dev)
    from unet_amd import _lib
    assert _lib.load().unetpp_distance_workspace_bytes(1, 0, 16) == 0 and _lib.load().unetpp_distance_workspace_bytes(2, 37, 53) > 0


# ---- 4. the whole loop -------------------------------------------------------------------------------------------------------
def test_process_frames_robust_equals_the_numpy_chain(torch_cuda, syn):
    torch = torch_cuda
    from unet_amd import frame_loop
    from unet_amd.nested_unet import NestedUNet
    net = NestedUNet(3, deep_supervision=False, max_batch=2, max_hw=(64, 64)).to("cuda:0")
    net.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)     # a seed whose masks hold both classes
    net.eval()
    frames = syn.make_frames_u8(2, 120, 200, "smooth", 77)
    post = dict(close_ksize=3, min_area=4, min_h_ratio=0.05, min_aspect=0.0, max_w_ratio=1.0, band_out=6, band_in=1, tape_min_area=2, pad=5)
    thr = dict(t_cable=0.34, t_tape=0.34, bg_margin=0.0, ct_margin=0.0)
    cable, tape, metrics = frame_loop.process_frames_robust(net, frames, 64, **thr, **post)
    assert cable.shape == (2, 120, 200) and cable.dtype == torch.uint8 and len(metrics) == 2
    # the same chain from the NumPy forms around the device's own masks at the letterbox size
    x = torch.from_numpy(frames).cuda()
    canvas, plan = rb.letterbox(net, x, 64)
    assert plan == rb.letterbox_plan(120, 200, 64)
    want_canvas = np.stack([rb.letterbox_np(f, 64)[0] for f in frames])
    assert np.array_equal(canvas.cpu().numpy(), want_canvas)
    cs, ts = net.segment_thresholded(canvas, "exclusive", **thr)
    cs, ts = cs.cpu().numpy(), ts.cpu().numpy()
    assert cs.sum() > 100 and ts.sum() > 100, "the chain needs both classes to say anything"
    kept = 0
    for f in range(2):
        c0, t0 = rb.unletterbox_mask_np(cs[f], plan), rb.unletterbox_mask_np(ts[f], plan)
        wc, wt = rb.postprocess_robust_np(c0, t0, post["close_ksize"], post["min_area"], post["min_h_ratio"], post["min_aspect"],
                                          post["max_w_ratio"], post["band_out"], post["band_in"], post["tape_min_area"], post["pad"])
        assert np.array_equal(cable[f].cpu().numpy(), wc) and np.array_equal(tape[f].cpu().numpy(), wt), f
        assert metrics[f] == rb.measure_diameters_np(wc, wt), f
        kept += int(wc.sum())
    print(f"process_frames_robust: mask pixels at 64x64 cable {int(cs.sum())} tape {int(ts.sum())}; cable kept at frame size {kept}")
    again = frame_loop.process_frames_robust(net, frames, 64, **thr, **post)
    assert torch.equal(again[0], cable) and torch.equal(again[1], tape) and again[2] == metrics
