"""The two-stage loop's own steps on the device (include/unetpp_two_stage.h, unet_amd/two_stage.py) against the NumPy forms, with ==
throughout (everything is integer or a table look-up), the whole loop against the composition of its parts, and FrameStream against
direct sequential calls.

Shapes.  ts_masks_kernel's tile is 256 x 8 pixels: 37 x 53 and 19 x 23 frames are ragged in both axes with more than one row of
tiles, 300 x 20 takes a second column of tiles; 32 x 48 -> 37 x 53 is a non-integer upscale, -> 19 x 23 a downscale.
ts_overlay_kernel cuts a frame into 48-byte spans that start on the output's 16-byte boundaries: 37 x 53 (5883 bytes per frame, odd)
gives every frame of the batch another phase and ragged first and last spans, 16 x 64 (3072 = 64 spans) none at all.
ts_rotate_kernel's tile is 32 x 32: 37 x 53 is two tiles a side and ragged, 1 x 1 the smallest frame, 16 x 64 half a tile by two.
Run on the GPU box:  python -m pytest tests/test_gpu_two_stage.py -m gpu"""
import numpy as np
import pytest

from conftest import load_golden
from unet_amd import edges as ed
from unet_amd import frame_loop
from unet_amd import raw_frames as rf
from unet_amd import two_stage as ts

pytestmark = pytest.mark.gpu
NET_WH = (48, 32)                                                       # target_size = (width, height) of the loop tests


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: these functions need none


def make_net(syn):
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=False, max_batch=3, max_hw=(NET_WH[1], NET_WH[0])).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    return m.eval()


@pytest.fixture(scope="module")
def nets(torch_cuda, syn):
    """Two loaded models with the same weights: the two slots of a FrameStream."""
    return make_net(syn), make_net(syn)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what):
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"


# ---- class_masks ---------------------------------------------------------------------------------------------------------------------
ROIS = {"odd corners": lambda fw, fh: (5, 3, fw - 4, fh - 2), "full frame": lambda fw, fh: (0, 0, fw, fh), "none": lambda fw, fh: None,
        "empty": lambda fw, fh: (7, 9, 7, 12), "past the frame": lambda fw, fh: (2, 1, fw + 9, fh + 9)}


@pytest.mark.parametrize("roi", list(ROIS))
@pytest.mark.parametrize("size_wh", [(53, 37), (23, 19), (300, 20)], ids=lambda s: "%dx%d" % s)
def test_class_masks_equal_the_numpy_form_and_two_resize_masks_calls(torch_cuda, model, size_wh, roi):
    pred = np.random.default_rng(size_wh[0]).integers(0, 4, (3, 32, 48), dtype=np.uint8)       # class 3 belongs to neither mask
    pred[1, :, :24] = 1                                                 # a frame with large counts
    r = ROIS[roi](*size_wh)
    t = dev(torch_cuda, pred)
    cable, tape, counts = ts.class_masks(model, t, size_wh, r)
    want = ts.class_masks_np(pred, size_wh, r)
    same(cable, want[0], "cable")
    same(tape, want[1], "tape")
    same(counts, want[2], "counts")
    for got, c in ((cable, 1), (tape, 2)):
        old = model.resize_masks(t, size_wh, match_class=c, roi=r)
        assert torch_cuda.equal(got, old), f"class {c}: differs from resize_masks"
        assert torch_cuda.equal(counts[:, c - 1], old.sum(dim=(1, 2), dtype=torch_cuda.int64))
    if roi == "empty":
        assert not cable.any() and not tape.any() and not counts.any()
    again = ts.class_masks(model, t, size_wh, r)                         # the counts are zeroed by every call
    assert torch_cuda.equal(again[2], counts)


# ---- overlay -------------------------------------------------------------------------------------------------------------------------
def overlay_inputs(h, w, value):
    """B = 3 scenes of make_scene: the masks overlap pairwise and all three at once, the ROI lies strictly inside the frame."""
    parts = [ts.make_scene(h, w, seed, value) for seed in (3, 4, 5)]
    return [np.stack([p[i] for p in parts]) for i in range(4)], parts[0][4]


@pytest.mark.parametrize("value", [1, 255])
@pytest.mark.parametrize("shape", [(37, 53), (16, 64)], ids=lambda s: "%dx%d" % s)
def test_overlay_equals_the_numpy_form(torch_cuda, model, shape, value):
    (frames, cable, tape, burr), roi = overlay_inputs(shape[0], shape[1], value)
    states = set(np.unique(ts.overlay_states_np(shape, cable, tape, burr, roi)).tolist())
    assert states == set(range(16)), sorted(states)
    t = [dev(torch_cuda, a) for a in (frames, cable, tape, burr)]
    for kw in (dict(), dict(colors={1: (10, 250, 30), 2: (200, 100, 0), 3: (1, 2, 255)}, weights=((0.9, 0.1), (0.5, 0.5), (0.25, 0.75), (0.8, 0.3)))):
        got, n_burr = ts.overlay(model, *t, roi, **kw)
        want, want_n = ts.overlay_np(frames, cable, tape, burr, roi, kw.get("colors"), kw.get("weights"))
        same(got, want, f"overlay {sorted(kw)}")
        same(n_burr, want_n, "burr count")
    for r in (None, (0, 0, shape[1], shape[0]), (4, 4, 4, 9)):           # no ROI, the full frame, an empty one
        got, _ = ts.overlay(model, *t, r)
        same(got, ts.overlay_np(frames, cable, tape, burr, r)[0], f"roi {r}")


def test_overlay_equals_the_reference_on_the_fixture(torch_cuda, model):
    g = load_golden("two_stage_scenes")
    for tag, h, w, seed, value, _ in g["cases"]:
        frame, cable, tape, burr, roi = ts.make_scene(int(h), int(w), int(seed), int(value))
        got, n_burr = ts.overlay(model, *(dev(torch_cuda, a[None]) for a in (frame, cable, tape, burr)), roi)
        same(got[0], g[tag + "_out"], tag)
        assert n_burr.tolist() == [int(np.count_nonzero(burr))]


# ---- rotate --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 37, 53, 3), (2, 37, 53, 1), (2, 1, 1, 3), (2, 16, 64, 3), (1, 70, 33, 1)], ids=str)
def test_rotate_equals_rot90(torch_cuda, model, shape):
    x = np.random.default_rng(shape[2]).integers(0, 256, shape, dtype=np.uint8)
    t = dev(torch_cuda, x)
    for code, k in ((0, 3), (1, 2), (2, 1)):
        got = ts.rotate(model, t, code)
        same(got, np.ascontiguousarray(np.rot90(x, k, axes=(1, 2))), f"code {code}")
        same(got, ts.rotate_np(x, code), f"code {code}: NumPy form")
    assert torch_cuda.equal(ts.rotate(model, ts.rotate(model, t, "90_cw"), "90_ccw"), t)


def test_bad_arguments_are_refused(torch_cuda, model):
    torch = torch_cuda
    pred = dev(torch, np.zeros((1, 8, 8), np.uint8))
    frames = dev(torch, np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(RuntimeError, match=r"pred must be a uint8 CUDA tensor \[B,H,W\]"):
        ts.class_masks(model, pred.cpu(), (8, 8))
    with pytest.raises(ValueError, match="negative"):
        ts.class_masks(model, pred, (8, 8), (-1, 0, 4, 4))
    with pytest.raises(ValueError, match="frame_size_wh must be positive"):
        ts.class_masks(model, pred, (0, 8))
    with pytest.raises(RuntimeError, match="does not match the frames"):
        ts.overlay(model, frames, pred, pred[:, :4].contiguous(), pred, None)
    with pytest.raises(ValueError, match="code must be"):
        ts.rotate(model, frames, 3)
    with pytest.raises(ValueError, match="1 or 3 are supported"):
        ts.rotate(model, dev(torch, np.zeros((1, 4, 4, 2), np.uint8)), 0)


def test_the_library_refuses_what_the_wrappers_cannot_send(torch_cuda, model):
    """UNETPP_E_UNSUPPORTED (-2) for every bad argument but the NULL engine: shapes, NULL pointers, overlap, a misaligned count table."""
    import ctypes
    from unet_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    t = dev(torch, np.zeros((1, 8, 8), np.uint8))
    model._input(t, "pred")
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    table = dev(torch, ts.overlay_table())
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    P = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    e, p, c = model._handle, P(t), P(cnt)
    o1, o2, o3 = P(buf), P(buf, 1024), P(buf, 2048)
    assert lib.unetpp_two_stage_masks_u8(e, p, 1, 8, 8, o1, o2, 8, 8, 0, 0, 8, 8, c, None) == 0
    for args in ((e, p, 0, 8, 8, o1, o2, 8, 8, 0, 0, 8, 8, c, None), (e, p, 1, 8, 8, o1, o2, 0, 8, 0, 0, 8, 8, c, None),
                 (e, p, 1, 8, 8, o1, o2, 8, 8, -1, 0, 8, 8, c, None), (e, p, 1, 8, 8, o1, o1, 8, 8, 0, 0, 8, 8, c, None),
                 (e, p, 1, 8, 8, p, o2, 8, 8, 0, 0, 8, 8, c, None), (e, p, 1, 8, 8, o1, o2, 8, 8, 0, 0, 8, 8, P(cnt, 4), None),
                 (e, None, 1, 8, 8, o1, o2, 8, 8, 0, 0, 8, 8, c, None), (e, p, 1, 8, 8, o1, o2, 8, 8, 0, 0, 8, 8, None, None),
                 (e, p, 1, 8, 8, o1, o2, 8, 8, 0, 0, 8, 8, o1, None)):
        assert lib.unetpp_two_stage_masks_u8(*args) == -2, args[2:13]
    f = P(buf, 3072)                                                     # 1 x 8 x 8 x 3 = 192 bytes of "frame"
    tb = P(table)
    assert lib.unetpp_two_stage_overlay_u8(e, f, p, p, p, 1, 8, 8, 0, 0, 8, 8, tb, o1, c, None) == 0
    for args in ((e, f, p, p, p, 1, 8, 0, 0, 0, 8, 8, tb, o1, c, None), (e, f, p, p, p, 1, 8, 8, 0, -2, 8, 8, tb, o1, c, None),
                 (e, f, p, p, p, 1, 8, 8, 0, 0, 8, 8, None, o1, c, None), (e, f, p, p, p, 1, 8, 8, 0, 0, 8, 8, tb, f, c, None),
                 (e, f, p, p, p, 1, 8, 8, 0, 0, 8, 8, tb, p, c, None), (e, f, p, p, p, 1, 8, 8, 0, 0, 8, 8, tb, tb, c, None),
                 (e, f, p, p, p, 1, 8, 8, 0, 0, 8, 8, tb, o1, P(cnt, 1), None), (e, f, p, p, p, 1, 8, 8, 0, 0, 8, 8, tb, o1, None, None)):
        assert lib.unetpp_two_stage_overlay_u8(*args) == -2, args[5:12]
    assert lib.unetpp_rotate_u8(e, f, 1, 8, 8, 3, 2, o1, None) == 0
    for args in ((e, f, 1, 8, 8, 2, 2, o1, None), (e, f, 1, 8, 8, 3, 3, o1, None), (e, f, 1, 8, 8, 3, -1, o1, None), (e, f, 1, 0, 8, 3, 0, o1, None),
                 (e, f, 1, 8, 8, 3, 0, f, None), (e, None, 1, 8, 8, 3, 0, o1, None), (e, f, 1, 8, 8, 3, 0, None, None)):
        assert lib.unetpp_rotate_u8(*args) == -2, args[2:7]
    torch.cuda.synchronize()


# ---- the whole loop ------------------------------------------------------------------------------------------------------------------
def loop_frames(b=3, h=40, w=56, seed=21):
    """BGR frames on which the synthetic-weight network finds cable and tape and stage 2 finds burrs (synthetic's "uniform" kind)."""
    from unet_amd import synthetic
    return synthetic.make_frames_u8(b, h, w, "uniform", seed)


def check_against_the_parts(torch, res, frames, roi):
    """The record against the composition of the parts' NumPy forms on the device's own pred."""
    fh, fw = frames.shape[1:3]
    pred = res.pred.cpu().numpy()
    assert pred.shape == (frames.shape[0], NET_WH[1], NET_WH[0])
    cable, tape, counts = ts.class_masks_np(pred, (fw, fh), roi)
    same(res.mask_cable, cable, "mask_cable")
    same(res.mask_tape, tape, "mask_tape")
    gray = ed.bgr_to_gray_np(frames)
    burr = np.stack([ed.detect_burrs_np(g, c) for g, c in zip(gray, cable)])
    same(res.mask_burr, burr, "mask_burr")
    over, n_burr = ts.overlay_np(frames, cable, tape, burr, roi)
    same(res.result, over, "result")
    same(res.counts, np.concatenate([counts, n_burr[:, None]], axis=1), "counts")
    assert res.roi == tuple(roi) and res.roi_area == (roi[2] - roi[0]) * (roi[3] - roi[1])
    rows = ts.ratios(res.counts.cpu().numpy(), res.roi_area)
    assert [r["burr"] for r in rows] == [bool(n) for n in n_burr]


@pytest.mark.parametrize("rotate", [False, True], ids=["plain", "rotate"])
def test_process_frames_two_stage_equals_the_composition_of_its_parts(torch_cuda, nets, rotate):
    torch = torch_cuda
    net = nets[0]
    frames = loop_frames()
    seen = ts.rotate_np(frames, 2) if rotate else frames
    fh, fw = seen.shape[1:3]
    assert (fh, fw) == ((56, 40) if rotate else (40, 56))
    roi = (3, 2, fw - 5, fh - 3)                                         # a ROI of the caller's, strictly inside the frame
    res = frame_loop.process_frames_two_stage(net, frames, target_size=NET_WH, rotate=rotate, roi=roi)
    print("two-stage counts (cable, tape, burr):", res.counts.tolist())
    check_against_the_parts(torch, res, seen, roi)
    assert (res.counts.sum(dim=0) > 0).all(), "the frames leave a mask empty: the loop would be compared on nothing"
    # roi="fixed": map_roi_to_original of the frame size (at this target size it lies right of the frame: the empty-ROI route)
    fixed = frame_loop.process_frames_two_stage(net, frames, target_size=NET_WH, rotate=rotate)
    check_against_the_parts(torch, fixed, seen, frame_loop.map_roi_to_original((fw, fh), NET_WH))
    # frames already on the device, no overlay
    res2 = frame_loop.process_frames_two_stage(net, dev(torch, frames), target_size=NET_WH, rotate=rotate, roi=roi, want_overlay=False)
    assert res2.result is None
    for name in ("pred", "mask_cable", "mask_tape", "mask_burr", "counts"):
        assert torch.equal(getattr(res2, name), getattr(res, name)), f"no overlay: {name}"
    # the normalised resolution, no ROI
    res3 = frame_loop.process_frames_two_stage(net, frames, target_size=NET_WH, rotate=rotate, normalize_resolution=(64, 48), roi=None)
    from unet_amd import tiling as tl
    norm = np.stack([tl.resize_linear_u8_np(f, (64, 48)) for f in seen])
    check_against_the_parts(torch, res3, norm, (0, 0, 64, 48))
    # the same bits on a second call and on a second stream
    again = frame_loop.process_frames_two_stage(net, frames, target_size=NET_WH, rotate=rotate, roi=roi)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = frame_loop.process_frames_two_stage(net, frames, target_size=NET_WH, rotate=rotate, roi=roi)
    side.synchronize()
    for name in ("pred", "mask_cable", "mask_tape", "mask_burr", "result", "counts"):
        assert torch.equal(getattr(again, name), getattr(res, name)), f"second call: {name}"
        assert torch.equal(getattr(other, name), getattr(res, name)), f"second stream: {name}"


def test_the_raw_twin_equals_the_bgr_loop_on_the_demosaiced_frames(torch_cuda, nets):
    torch = torch_cuda
    net = nets[0]
    raw = rf.make_raw(3, 40, 56, 11)
    t = dev(torch, raw)
    for name in ("BayerRG8", "Mono8"):
        for want_overlay in (True, False):
            want = frame_loop.process_frames_two_stage(net, rf.to_bgr(net, t, name), target_size=NET_WH, roi=(4, 2, 50, 37), want_overlay=want_overlay)
            got = frame_loop.process_raw_frames_two_stage(net, t, name, target_size=NET_WH, roi=(4, 2, 50, 37), want_overlay=want_overlay)
            for field in ("pred", "mask_cable", "mask_tape", "mask_burr", "counts"):
                assert torch.equal(getattr(got, field), getattr(want, field)), (name, field)
            assert (got.result is None and want.result is None) if not want_overlay else torch.equal(got.result, want.result)
            assert (got.roi, got.roi_area) == (want.roi, want.roi_area)


# ---- FrameStream ---------------------------------------------------------------------------------------------------------------------
def stream_fn(m, x):
    return frame_loop.process_frames_two_stage(m, x, target_size=NET_WH, roi=(3, 2, 51, 37), check=False)


FIELDS = ("pred", "mask_cable", "mask_tape", "mask_burr", "result", "counts")


@pytest.mark.parametrize("n_slots", [1, 2])
def test_frame_stream_returns_what_sequential_calls_return(torch_cuda, nets, n_slots):
    from unet_amd.stream import FrameStream
    torch = torch_cuda
    batches = [loop_frames(3, seed=100 + 7 * i) for i in range(4)] + [loop_frames(2, seed=200)]      # five batches, the last of 2
    direct = []
    for b in batches:
        r = stream_fn(nets[0], b)
        direct.append({k: getattr(r, k).cpu().numpy() for k in FIELDS} | {"roi": r.roi, "roi_area": r.roi_area})
    fs = FrameStream(list(nets[:n_slots]), stream_fn)
    assert fs.n_slots == n_slots
    seen = 0
    for got, want in zip(fs.map(batches), direct):
        assert set(got) == set(want)
        for k in FIELDS:
            assert isinstance(got[k], np.ndarray) and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (seen, k)
        assert got["roi"] == want["roi"] and got["roi_area"] == want["roi_area"]
        seen += 1
    assert seen == 5
    # named outputs only; tickets answer in any order while their slot still holds them
    fs2 = FrameStream(list(nets[:n_slots]), stream_fn, outputs=("counts", "result"))
    tickets = [fs2.submit(b) for b in batches[:n_slots]]
    for i in reversed(range(n_slots)):
        got = fs2.result(tickets[i])
        assert sorted(got) == ["counts", "result"] and np.array_equal(got["counts"], direct[i]["counts"]) and np.array_equal(got["result"], direct[i]["result"])
    stale = tickets[0]
    fs2.submit(batches[0])
    if n_slots == 1:
        with pytest.raises(RuntimeError, match="taken another batch"):
            fs2.result(stale)
    fs2.synchronize()


def test_frame_stream_surfaces_an_exception_and_stays_usable(torch_cuda, nets):
    from unet_amd.stream import FrameStream
    batches = [loop_frames(3, seed=300), loop_frames(3, seed=301), loop_frames(3, seed=302)]
    calls = []

    def fn(m, x):
        calls.append(len(calls))
        if calls[-1] == 1:
            raise ValueError("the second batch is refused")
        return stream_fn(m, x)

    fs = FrameStream(list(nets), fn, outputs=("counts",))
    it = fs.map(batches)
    first = {k: v.copy() for k, v in next(it).items()}
    with pytest.raises(ValueError, match="the second batch is refused"):
        next(it)
    want = stream_fn(nets[0], batches[2]).counts.cpu().numpy()
    got = list(fs.map([batches[2]]))                                      # the stream still works
    assert len(got) == 1 and np.array_equal(got[0]["counts"], want)
    assert np.array_equal(first["counts"], stream_fn(nets[0], batches[0]).counts.cpu().numpy())
    t = fs.submit(batches[0])
    assert np.array_equal(fs.result(t)["counts"], first["counts"])
    unknown = FrameStream([nets[0]], stream_fn, outputs=("nothing",))     # a name fn's result does not have surfaces the same way
    with pytest.raises(KeyError, match="no member"):
        unknown.result(unknown.submit(batches[0]))
