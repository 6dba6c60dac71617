"""The spatial, fixed and simple loops on the device (include/unetpp_simple_loops.h, unet_amd/simple_loops.py) against the NumPy
forms, with == throughout: the two pixel rules, the component rule, the tape filter with its table, the focus band, the class
clean-ups of the three SimpleUNet scripts, and the six whole loops against the same steps composed from predict_proba / segment
and the NumPy forms on the host.  Shapes are the smallest that reach every path: ragged rows, pointers off by one element, more
than one workgroup, several row bands of the merge kernel (its tiles span whole rows, so there is one tile per row band).
Run on the GPU box:  python -m pytest tests/test_gpu_simple_loops.py -m gpu"""
import numpy as np
import pytest

from conftest import load_golden
from unet_amd import multiclass as mc
from unet_amd import simple_loops as sl
from unet_amd import synthetic

pytestmark = pytest.mark.gpu
COLORS = {1: (255, 0, 0), 2: (0, 255, 0), 5: (255, 0, 255)}
FIELDS = ("dc_px", "dt_px", "delta_d_px", "cable_coverage", "tape_coverage")


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


@pytest.fixture(scope="module")
def golden():
    g = load_golden("simple_loops_scenes")
    return {k: g[k] for k in g.files}


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def embedded(torch, a, offset):
    """A CUDA view of `a` at byte `offset` of a larger buffer whose other bytes are 255."""
    buf = torch.full((a.nbytes + offset + 64,), 255, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + a.nbytes].view(getattr(torch, str(a.dtype))).view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.is_contiguous() and view.data_ptr() % 16 == (buf.data_ptr() + offset) % 16
    return view


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"


# ---- 1. the pixel rules ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("channels", [3, 7])
@pytest.mark.parametrize("hw", [(17, 23), (64, 96)])
def test_pixel_rules_on_random_probabilities(torch_cuda, model, hw, channels, layout):
    """B = 2 with NaN and +-inf planted in every channel; once in a fresh tensor, once one float off 16-byte alignment."""
    p = sl.make_random_probs(2, channels, hw[0], hw[1], 3 * hw[0] + channels, True, layout)
    assert np.isnan(p).any() and np.isinf(p).any()
    for name, t in (("aligned", dev(torch_cuda, p)), ("off by 4 bytes", embedded(torch_cuda, p, 4))):
        for rule, fn, fn_np, args in (("relative", sl.relative_threshold, sl.relative_threshold_np, (2.0, 2.5)),
                                      ("relative 1.3 / 0.7", sl.relative_threshold, sl.relative_threshold_np, (1.3, 0.7)),
                                      ("confidence", sl.confidence_threshold, sl.confidence_threshold_np, (0.3,))):
            got, want = fn(model, t, *args, layout), fn_np(p, *args, layout)
            for g, w, which in zip(host(*got), want, ("cable", "tape")):
                same(g, w, f"{rule} {which} {layout} C={channels} {hw} {name}")
            assert want[0].any() and want[1].any()


def test_pixel_rules_on_the_fixtures(torch_cuda, model, golden):
    for name, b, c, h, w, seed, specials in sl.FIXTURE_PROBS:
        p = sl.make_probs(b, c, h, w, seed, specials)
        for tag, got in (("rel", sl.relative_threshold(model, dev(torch_cuda, p))), ("conf", sl.confidence_threshold(model, dev(torch_cuda, p), 0.3))):
            same(host(got[0])[0], sl.unbits(golden[f"{name}_{tag}_cable"], (b, h, w)), f"{name} {tag} cable")
            same(host(got[1])[0], sl.unbits(golden[f"{name}_{tag}_tape"], (b, h, w)), f"{name} {tag} tape")


def test_pixel_rules_refuse_bad_arguments(torch_cuda, model):
    p = dev(torch_cuda, sl.make_random_probs(1, 3, 8, 8, 0))
    with pytest.raises(ValueError):
        sl.relative_threshold(model, p, float("nan"))
    with pytest.raises(ValueError):
        sl.confidence_threshold(model, p[:, :2].contiguous())
    with pytest.raises(ValueError):
        sl.relative_threshold(model, p, layout="hwc")
    with pytest.raises(RuntimeError):
        sl.confidence_threshold(model, p.double())


# ---- 2. and 3. the component rule, the tape filter, the band ---------------------------------------------------------------------------
def random_masks(b, h, w, seed):
    """Blobs of many sizes and shapes plus speckle: components on both sides of any small bound."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((b, h, w), np.uint8)
    for i in range(b):
        m = r.random((h, w)) < 0.03
        for _ in range(int(r.integers(4, 9))):
            cy, cx, ry, rx = r.integers(0, h), r.integers(0, w), r.integers(1, h // 4), r.integers(1, w // 4)
            m |= ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1
        out[i] = m & (r.random((h, w)) > 0.02)
    return out


def test_keep_components(torch_cuda, model, golden):
    masks = random_masks(3, 64, 96, 1)
    for args, kw in (((100,), {}), ((20, 400), {}), ((30, None, 12), {}), ((1, 10 ** 12, 0), {"out_value": 255}), ((2.5, 399.5, 11.2), {})):
        for name, t in (("aligned", dev(torch_cuda, masks)), ("off by 1 byte", embedded(torch_cuda, masks, 1))):
            same(host(sl.keep_components(model, t, *args, **kw))[0], sl.keep_components_np(masks, *args, **kw), f"keep_components{args} {name}")
    want = sl.keep_components_np(masks, 20, 400)
    assert want.any() and (want != (masks > 0)).any()
    classes = masks * np.random.default_rng(2).integers(1, 3, masks.shape, dtype=np.uint8)
    same(host(sl.keep_components(model, dev(torch_cuda, classes), 5, 300, 3, match_class=2, out_value=7))[0],
         sl.keep_components_np(classes, 5, 300, 3, match_class=2, out_value=7), "keep_components class 2")
    scene = sl.make_component_scene()
    for name, lo, hi, wd in sl.FIXTURE_COMPONENTS:
        same(host(sl.keep_components(model, dev(torch_cuda, scene[None]), lo, hi, wd))[0][0], sl.unbits(golden["components_" + name], scene.shape), name)


def test_keep_components_overflow_and_empty_frames(torch_cuda, model):
    """A frame with more components than max_components raises with check=True and comes out all zero with check=False; the
    other frames of the batch are filtered as usual.  An all-zero frame stays all zero."""
    masks = np.zeros((3, 64, 96), np.uint8)
    masks[0, ::2, ::2] = 1                                   # 32 * 48 = 1536 single pixels
    masks[1, 10:30, 10:50] = 1
    t = dev(torch_cuda, masks)
    with pytest.raises(RuntimeError, match="max_components"):
        sl.keep_components(model, t, 1, max_components=64)
    got = host(sl.keep_components(model, t, 1, max_components=64, check=False))[0]
    assert not got[0].any() and not got[2].any()
    same(got[1], masks[1], "the frame beside the overflowing one")
    same(host(sl.keep_components(model, t, 1, max_components=2048))[0], masks, "with room for every component")
    with pytest.raises(ValueError):
        sl.keep_components(model, t, float("nan"))
    with pytest.raises(ValueError):
        sl.keep_components(model, t, 1, out_value=0)


def tape_batch(h, w, seed):
    """B = 3: a scene whose filter removes little, one whose filter removes most (fallback), random blobs; values beyond 0/1."""
    r = np.random.default_rng(seed)
    tape = np.stack([sl.make_tape_scene("filtered", h, w)[0], sl.make_tape_scene("fallback", h, w)[0], random_masks(1, h, w, seed)[0]])
    cable = np.stack([sl.make_tape_scene("filtered", h, w)[1], sl.make_tape_scene("fallback", h, w)[1], random_masks(1, h, w, seed + 1)[0] * 255])
    cable[2, :, : w // 3] = 0
    tape[2] *= r.integers(1, 4, (h, w), dtype=np.uint8)
    return tape, cable


def test_tape_position_filter(torch_cuda, model, golden):
    for h, w in ((64, 96), (33, 129)):
        tape, cable = tape_batch(h, w, 3)
        want, want_table = sl.tape_position_filter_np(tape, cable)
        assert want_table[:2, 4].tolist() == [1, 0]
        for name, t, c in (("aligned", dev(torch_cuda, tape), dev(torch_cuda, cable)), ("off by 1 and 3 bytes", embedded(torch_cuda, tape, 1), embedded(torch_cuda, cable, 3))):
            got, table = sl.tape_position_filter(model, t, c)
            assert table.dtype == torch_cuda.int32 and tuple(table.shape) == (3, 6)
            same(host(got)[0], want, f"tape filter {h}x{w} {name}")
            same(host(table)[0], want_table, f"tape table {h}x{w} {name}")
    for kind in sl.TAPE_SCENES:
        tape, cable = sl.make_tape_scene(kind)
        got, table = sl.tape_position_filter(model, dev(torch_cuda, tape[None]), dev(torch_cuda, cable[None]))
        same(host(got)[0][0], sl.unbits(golden[f"tape_{kind}_out"], tape.shape), kind)
        assert host(table)[0][0].tolist() == golden[f"tape_{kind}_table"].tolist(), kind
    zero = dev(torch_cuda, np.zeros((2, 17, 23), np.uint8))
    got, table = sl.tape_position_filter(model, zero, zero.clone())
    assert not host(got)[0].any() and host(table)[0].tolist() == [[-1, -1, 0, 0, 0, 0]] * 2
    with pytest.raises(ValueError):
        sl.tape_position_filter(model, zero, zero[:, :8].contiguous())


def test_column_band(torch_cuda, model, golden):
    for h, w in ((17, 23), (64, 96), (5, 3)):
        masks = np.random.default_rng(h).integers(0, 4, (2, h, w), dtype=np.uint8) * 85
        for args in ((), (0.1, 0.95), (0.0, 1.0), (0.5, 0.5)):
            same(host(sl.column_band(model, embedded(torch_cuda, masks, 1), *args))[0], sl.column_band_np(masks, *args), f"band {h}x{w} {args}")
    for key in (k for k in golden if k.startswith("band_")):
        h, w = (int(v) for v in key[5:].split("x"))
        same(host(sl.column_band(model, dev(torch_cuda, np.full((1, h, w), 255, np.uint8))))[0][0], sl.unbits(golden[key], (h, w)), key)


# ---- 4. the clean-ups ------------------------------------------------------------------------------------------------------------------
BIG_FRAME = (200, 300)


def test_the_large_frame_spans_several_row_bands():
    """The merge kernel's tiles span whole rows up to this width, so `several tiles` means several row bands."""
    for v in sl.VARIANTS.values():
        band, cols = mc.merge_layout((1,) + BIG_FRAME, ((None, v["cable"], 1), (None, v["tape"], 2), (None, (), 5)), sl.LUT_SIMPLE)
        assert 2 * band <= BIG_FRAME[0] and cols >= BIG_FRAME[1] and BIG_FRAME[0] <= 256 and BIG_FRAME[1] <= 384
    band, _ = mc.merge_layout((1,) + BIG_FRAME, sl.PLANES_BURR, sl.LUT_BURR)
    assert 2 * band <= BIG_FRAME[0]


def test_threshold_planes(torch_cuda, model):
    p = sl.make_random_probs(2, 7, 17, 23, 9, specials=True)
    for frame_hw in ((17, 23), (40, 31), (64, 96)):
        for thr in ((0.35, 0.35, 0.70), (0.30, 0.55, 0.70)):
            got = host(sl.threshold_planes(model, embedded(torch_cuda, p, 4), frame_hw, thr))[0]
            same(got, sl.threshold_planes_np(p, frame_hw, thr), f"threshold_planes {frame_hw} {thr}")


@pytest.mark.parametrize("frame_hw", [sl.FIXTURE_FRAME, BIG_FRAME])
@pytest.mark.parametrize("constants", ["reference", "scaled"])
@pytest.mark.parametrize("variant", ["simple", "optimized"])
def test_predict_simple(torch_cuda, model, golden, variant, constants, frame_hw):
    planes = sl.make_simple_batch()
    kw = {} if constants == "reference" else dict(sl.SCALED_TAPE)
    want = sl.predict_simple_np(planes, frame_hw, variant, return_tape_table=True, **kw)
    got = sl.predict_simple(model, dev(torch_cuda, planes), frame_hw, variant, return_tape_table=True, **kw)
    same(host(got[0])[0], want[0], f"{variant} map")
    same(host(got[1])[0], want[1], f"{variant} class table")
    if variant == "optimized":
        same(host(got[2])[0], want[2], "tape table")
        assert want[2][:, 4].tolist() == [1, 0, 0, 0]
    else:
        assert got[2] is None
    if frame_hw == sl.FIXTURE_FRAME and constants == "reference":
        same(want[0], golden[f"predict_{variant}_map"], "the NumPy form against the reference")
    only_map = sl.predict_simple(model, dev(torch_cuda, planes), frame_hw, variant, want_table=False, check=False, **kw)
    same(host(only_map)[0], want[0], f"{variant} map alone")


def test_predict_simple_on_an_empty_and_an_overfull_frame(torch_cuda, model):
    """An all-zero batch gives an all-zero map.  A burr plane of 64 isolated blocks has more components than max_components:
    check=True raises, check=False drops the burr of that frame and nothing else."""
    zero = np.zeros((2, 7, 32, 32), np.float32)
    for variant in ("simple", "optimized"):
        out, table = sl.predict_simple(model, dev(torch_cuda, zero), sl.FIXTURE_FRAME, variant)
        assert not host(out)[0].any() and (host(table)[0][:, 1:, 0] == 0).all()
    planes = sl.make_simple_batch(("filtered", "filtered"))
    planes[0, 5] = 0.0
    y, x = np.mgrid[0:32, 0:32]
    planes[0, 5][(y % 4 < 2) & (x % 4 < 2)] = 1.0             # 8 x 8 blocks of 2 x 2, about 4 x 6 at frame size: they survive the opening
    want = sl.predict_simple_np(planes, sl.FIXTURE_FRAME, "optimized", want_table=False, min_burr_area=1)
    assert (want[0] == 5).sum() > 0
    with pytest.raises(RuntimeError, match="max_components"):
        sl.predict_simple(model, dev(torch_cuda, planes), sl.FIXTURE_FRAME, "optimized", min_burr_area=1, max_components=32)
    got = host(sl.predict_simple(model, dev(torch_cuda, planes), sl.FIXTURE_FRAME, "optimized", want_table=False, min_burr_area=1, max_components=32,
                                 check=False))[0]
    no_burr = sl.predict_simple_np(planes, sl.FIXTURE_FRAME, "optimized", want_table=False, min_burr_area=10 ** 6)
    same(got[0], no_burr[0], "the overfull frame without its burr")
    same(got[1], want[1], "the frame beside it")


def test_predict_simple_backup(torch_cuda, model, golden):
    bm = sl.make_backup_map()
    out, table = sl.predict_simple_backup(model, dev(torch_cuda, bm[None]))
    same(host(out)[0][0], golden["backup_map"], "backup map against the reference")
    same(host(table)[0], mc.class_table_np(golden["backup_map"][None]), "backup table")
    r = np.random.default_rng(4)
    maps = np.stack([sl.make_backup_map(BIG_FRAME[0], BIG_FRAME[1], s) for s in (1, 2)])
    maps[1][r.random(BIG_FRAME) < 0.3] = 0
    want, want_table = sl.predict_simple_backup_np(maps)
    got, table = sl.predict_simple_backup(model, embedded(torch_cuda, maps, 1))
    same(host(got)[0], want, "backup map, several row bands")
    same(host(table)[0], want_table, "backup table, several row bands")
    assert ((maps == 2) & (want == 1)).any()


# ---- 5. the whole loops ------------------------------------------------------------------------------------------------------------------
SIZE, FRAME = 64, (96, 160)


@pytest.fixture(scope="module")
def frames(torch_cuda):
    return dev(torch_cuda, synthetic.make_frames_u8(2, FRAME[0], FRAME[1], "smooth", 11))


@pytest.fixture(scope="module")
def nested(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=True, pretrained_encoder=False, max_batch=2, max_hw=(SIZE, SIZE)).to("cuda:0")
    m.load_state_dict(synthetic.make_state_dict(3, 3, True, 2), strict=True)
    return m.eval()


@pytest.fixture(scope="module")
def simple(torch_cuda):
    from unet_amd.nested_unet import SimpleUNet
    m = SimpleUNet(num_classes=7, num_channels=3, max_batch=2, max_hw=(SIZE, SIZE)).to("cuda:0")
    m.load_state_dict(synthetic.make_simple_state_dict(7, 3, 3), strict=True)
    return m.eval()


def rows(metrics, fields):
    return [[m[f] for f in fields] for m in metrics]


def test_process_frames_spatial(torch_cuda, nested, frames):
    from unet_amd import frame_loop as fl
    cable, tape, metrics, probs = fl.process_frames_spatial(nested, frames, input_size=SIZE, cable_bg_ratio=0.8, tape_bg_ratio=0.8)
    p = host(nested.predict_proba(nested.resize_frames(frames, (SIZE, SIZE))))[0]
    same(host(probs)[0], p, "probs")
    wc, wt, wm = sl.postprocess_spatial_np(p, FRAME, 0.8, 0.8)
    same(host(cable)[0], wc, "cable")
    same(host(tape)[0], wt, "tape")
    assert rows(metrics, ("cable_coverage", "tape_coverage")) == rows(wm, ("cable_coverage", "tape_coverage"))
    print("spatial coverages", rows(metrics, ("cable_coverage", "tape_coverage")))


def test_process_frames_fixed(torch_cuda, nested, frames):
    from unet_amd import frame_loop as fl
    kw = dict(conf_cable=0.34, conf_tape=0.34, bg_margin=0.6, min_area_cable=12, min_area_tape=6, max_area_cable=3000, max_area_tape=2000)
    cable, tape, metrics, pred = fl.process_frames_fixed(nested, frames, input_size=SIZE, **kw)
    cs, ts = host(*nested.segment_thresholded(nested.resize_frames(frames, (SIZE, SIZE)), "strict_bg_check", 0.34, 0.34, 0.6))
    wc, wt, wm, wp = sl.postprocess_fixed_np(cs, ts, FRAME, 12, 6, 3000, 2000)
    same(host(cable)[0], wc, "cable")
    same(host(tape)[0], wt, "tape")
    same(host(pred)[0], wp, "pred")
    assert rows(metrics, FIELDS) == rows(wm, FIELDS)
    print("fixed: thresholded pixels", int(cs.sum()), int(ts.sum()), "kept", int(wp.astype(bool).sum()), rows(metrics, FIELDS))


def test_process_frames_confidence(torch_cuda, nested, frames):
    from unet_amd import frame_loop as fl
    cable, tape, metrics, pred, probs = fl.process_frames_confidence(nested, frames, input_size=SIZE, conf_threshold=0.3)
    p = host(nested.predict_proba(nested.resize_frames(frames, (SIZE, SIZE))))[0]
    same(host(probs)[0], p, "probs")
    wc, wt, wm, wp = sl.measured_tail_np(*sl.confidence_threshold_np(p, 0.3), FRAME)
    same(host(cable)[0], wc, "cable")
    same(host(tape)[0], wt, "tape")
    same(host(pred)[0], wp, "pred")
    assert rows(metrics, FIELDS) == rows(wm, FIELDS)
    print("confidence", rows(metrics, FIELDS))


@pytest.mark.parametrize("variant", ["simple", "optimized", "backup"])
def test_process_frames_simple(torch_cuda, simple, frames, variant):
    from unet_amd import frame_loop as fl
    kw = {} if variant == "backup" else dict(sl.SCALED_TAPE)
    out, table, over = fl.process_frames_simple(simple, frames, variant, SIZE, COLORS, 0.5, **kw)
    resized = simple.resize_frames(frames, (SIZE, SIZE))
    if variant == "backup":
        pred = host(simple.resize_masks(simple.segment(resized), (FRAME[1], FRAME[0])))[0]
        want, want_table = sl.predict_simple_backup_np(pred)
    else:
        want, want_table = sl.predict_simple_np(host(simple.predict_proba(resized))[0], FRAME, variant, **kw)
    same(host(out)[0], want, f"{variant} map")
    same(host(table)[0], want_table, f"{variant} table")
    same(host(over)[0], mc.overlay_np(host(frames)[0], want, COLORS, 0.5, "region", 7), f"{variant} overlay")
    print(variant, "classes", np.unique(want, return_counts=True))
    out2, table2, over2 = fl.process_frames_simple(simple, frames, variant, SIZE, want_table=False, **kw)
    assert table2 is None and over2 is None
    same(host(out2)[0], want, f"{variant} map alone")
