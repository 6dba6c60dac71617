"""Training batches on the device (unetpp_train_batch_u8, unetpp_train_crop_rects and the functions of
unet_amd/train_batch.py built on them) against the NumPy forms, bit for bit: on the fixture's scenes (what the reference's own
dataset classes returned) and on the smallest shapes at which the kernels can still go wrong.  None of the tests runs the network.
Run on the GPU box:  python -m pytest tests/test_gpu_train_batch.py -m gpu"""
import random

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import train_batch as tb

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
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: the batches need none


@pytest.fixture(scope="module")
def g():
    return load_golden("train_batch_scenes")


@pytest.fixture(scope="module")
def items(g):
    n = int(g["n_items"])
    return [g[f"img_{i}"] for i in range(n)], [g[f"msk_{i}"] for i in range(n)]


@pytest.fixture(scope="module")
def fixture_set(model, items):
    return tb.TrainSet(model, *items)


def make_items(sizes, seed, classes=7):
    r = np.random.default_rng(seed)
    return ([r.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes], [r.integers(0, classes, (h, w), dtype=np.uint8) for h, w in sizes])


def same(torch, got, want):
    """A device result (image, target) equals the NumPy form's: dtype, shape and every bit."""
    for a, b, what in zip(got, want, ("image", "target")):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, a.shape, b.dtype, b.shape)
        bad = a.view(np.uint8) != np.ascontiguousarray(b).view(np.uint8)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4])


def both(torch, model, ts, images, masks, samples, size_hw, class_table=None, rects_np=None, rects=None, **fmt):
    plan, luts = tb.build_plan(samples, ts.sizes)
    want = tb.assemble_np(images, masks, plan, luts, size_hw, class_table, rects_np, **fmt)
    got = tb.make_batch(model, ts, plan, size_hw, luts, class_table, rects, **fmt)
    same(torch, got, want)
    return got


def random_samples(r, sizes, n, stages="all"):
    """n samples with every stage drawn independently: a rectangle of any size down to one pixel, geometry on both sides, both
    look-ups."""
    out = []
    for _ in range(n):
        i = int(r.integers(0, len(sizes)))
        h, w = sizes[i]
        x1, y1 = int(r.integers(0, w)), int(r.integers(0, h))
        x2, y2 = int(r.integers(x1 + 1, w + 1)), int(r.integers(y1 + 1, h + 1))
        kw = dict(rect=(x1, y1, x2, y2) if r.random() < 0.7 else None, flip_h=r.random() < 0.5, flip_v=r.random() < 0.5, rot90=int(r.integers(0, 4)),
                  post_flip_h=r.random() < 0.5, post_flip_v=r.random() < 0.5)
        if stages == "all":
            kw["byte_lut"] = tb.convert_scale_abs_lut(r.uniform(0.8, 1.2), int(r.integers(-20, 21))) if r.random() < 0.5 else None
            kw["value_lut"] = tb.value_scale_lut(0.7 + r.random() * 0.6) if r.random() < 0.6 else None
        out.append(tb.sample(i, **kw))
    return out


# ---- the fixture's scenes -------------------------------------------------------------------------------------------------------------
CABLE = {"eval_32x32": (False, (32, 32)), "aug_17x23": (True, (17, 23)), "aug_48x40": (True, (48, 40))}
PATCH = {"p32_native": (32, None, True), "p32_to17": (32, 17, True), "p33_to40x48": (33, (40, 48), True), "p32_plain": (32, (40, 48), False)}


def sha_rows(image):
    import hashlib
    return [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in image]


@pytest.mark.parametrize("cfg", sorted(CABLE))
def test_fixture_cable_runs(torch_cuda, model, fixture_set, g, items, cfg):
    """One batch of differing items per run; the device equals the NumPy form and, through it, the reference's tensors."""
    augment, target = CABLE[cfg]
    n = int(g[f"cable_{cfg}_count"])
    samples = []
    for s in range(n):
        rng = tb.ReplayRng(g[f"cable_{cfg}_{s}_draws"], "np")
        samples.append(tb.sample(int(g[f"cable_{cfg}_{s}_item"]), **(tb.draw_cable_defect(rng)[0] if augment else {})))
    image, target_t = both(torch_cuda, model, fixture_set, *items, samples, target)
    assert sha_rows(image.cpu().numpy()) == [str(g[f"cable_{cfg}_{s}_sha"]) for s in range(n)]
    assert all((target_t[s].cpu().numpy() == g[f"cable_{cfg}_{s}_mask"]).all() for s in range(n))


def test_fixture_native_size_runs(torch_cuda, model, fixture_set, g, items):
    """target_size=None: one launch per item size, identity resize, flips and the brightness step on source bytes."""
    for cfg, augment in (("eval_native", False), ("aug_native", True)):
        for s in range(int(g[f"cable_{cfg}_count"])):
            i = int(g[f"cable_{cfg}_{s}_item"])
            kw = tb.draw_cable_defect(tb.ReplayRng(g[f"cable_{cfg}_{s}_draws"], "np"))[0] if augment else {}
            image, _ = both(torch_cuda, model, fixture_set, *items, [tb.sample(i, **kw)], fixture_set.sizes[i])
            assert sha_rows(image.cpu().numpy()) == [str(g[f"cable_{cfg}_{s}_sha"])]


@pytest.mark.parametrize("cfg", sorted(PATCH))
def test_fixture_patch_runs(torch_cuda, model, fixture_set, g, items, cfg):
    ps, target, augment = PATCH[cfg]
    types = g[f"patch_{cfg}_types"]
    n = int(g[f"patch_{cfg}_count"])
    assert fixture_set.defect_items == list(g[f"patch_{cfg}_defect_items"]) and fixture_set.normal_items == list(g[f"patch_{cfg}_normal_items"])
    assert np.array_equal(np.array(fixture_set.bboxes), g[f"patch_{cfg}_bboxes"])
    samples = [tb.draw_patch(tb.ReplayRng(g[f"patch_{cfg}_{s}_draws"], "py"), "defect" if types[s % len(types)] else "normal", ps, fixture_set.sizes,
                             fixture_set.defect_items, fixture_set.bboxes, fixture_set.normal_items, augment) for s in range(n)]
    hw = (ps, ps) if target is None else ((target, target) if isinstance(target, int) else (target[1], target[0]))
    image, target_t = both(torch_cuda, model, fixture_set, *items, samples, hw, tb.binary_defect_lut())
    assert sha_rows(image.cpu().numpy()) == [str(g[f"patch_{cfg}_{s}_sha"]) for s in range(n)]
    assert all((target_t[s].cpu().numpy() == g[f"patch_{cfg}_{s}_mask"]).all() for s in range(n))


@pytest.mark.parametrize("name", ["adv", "adv3"])
def test_fixture_tape_focused_runs(torch_cuda, model, fixture_set, g, items, name):
    """The rectangles come from crop_rects on the device and make_batch reads that table: nothing is read back or synchronised
    between the two launches."""
    ctab = tb.class_lut({1: 1, 2: 2}, "zero") if name == "adv3" else None
    n = int(g[f"{name}_count"])
    samples, req = [], []
    for s in range(n):
        i = int(g[f"{name}_{s}_item"])
        h, w = fixture_set.sizes[i]
        assert fixture_set.counts[i, 2] == (items[1][i] == 2).sum()
        rng = tb.ReplayRng(g[f"{name}_{s}_draws"], "np")
        crop = tb.draw_tape_crop(rng, h, w, int(fixture_set.counts[i, 2]), tape_crop_prob=0.7)
        kw = tb.draw_cable_defect(rng)[0]
        samples.append(tb.sample(i, rect_row=None if crop is None else len(req), **kw))
        if crop is not None:
            req.append((i,) + crop)
    req = np.array(req)
    rects = tb.crop_rects(model, fixture_set, req[:, 0], req[:, 1], req[:, 2:4])
    rects_np = tb.crop_rects_np(items[1], np.concatenate([req, np.full((len(req), 1), 2)], 1))
    image, target_t = both(torch_cuda, model, fixture_set, *items, samples, (32, 32), ctab, rects_np, rects)
    assert (rects.cpu().numpy() == rects_np).all()
    assert sha_rows(image.cpu().numpy()) == [str(g[f"{name}_{s}_sha"]) for s in range(n)]
    assert all((target_t[s].cpu().numpy() == g[f"{name}_{s}_mask"]).all() for s in range(n))


def test_seeded_cable_defect_batches_end_to_end(torch_cuda, model, fixture_set, g):
    """np.random seeded as the generator seeded the reference: the iterator's batches are the reference's tensors."""
    cfg = "aug_17x23"
    n, n_items = int(g[f"cable_{cfg}_count"]), len(fixture_set)
    state = np.random.get_state()
    try:
        np.random.seed(int(g[f"cable_{cfg}_seed"]))
        got = list(tb.cable_defect_batches(model, fixture_set, (17, 23), 8, indices=[s % n_items for s in range(n)], augment=True,
                                           target_dtype=torch_cuda.int64))
    finally:
        np.random.set_state(state)
    assert [len(b[0]) for b in got] == [8] * (n // 8) + ([n % 8] if n % 8 else [])
    image = torch_cuda.cat([b[0] for b in got]).cpu().numpy()
    target = torch_cuda.cat([b[1] for b in got])
    assert target.dtype == torch_cuda.int64 and image.dtype == np.float32
    assert sha_rows(image) == [str(g[f"cable_{cfg}_{s}_sha"]) for s in range(n)]
    assert all((target[s].cpu().numpy() == g[f"cable_{cfg}_{s}_mask"]).all() for s in range(n))


def test_seeded_patch_defect_batches_end_to_end(torch_cuda, model, fixture_set, g):
    cfg = "p32_to17"
    types = g[f"patch_{cfg}_types"]
    n = int(g[f"patch_{cfg}_count"])
    rng = random.Random(int(g[f"patch_{cfg}_seed"]))
    got = list(tb.patch_defect_batches(model, fixture_set, ["defect" if types[s % len(types)] else "normal" for s in range(n)], 5,
                                       patch_size=32, target_size=17, rng=rng))
    image = torch_cuda.cat([b[0] for b in got]).cpu().numpy()
    target = torch_cuda.cat([b[1] for b in got]).cpu().numpy()
    assert sha_rows(image) == [str(g[f"patch_{cfg}_{s}_sha"]) for s in range(n)]
    assert all((target[s] == g[f"patch_{cfg}_{s}_mask"]).all() for s in range(n))


def test_tape_focused_batches_equal_the_numpy_replay(torch_cuda, model, fixture_set, items):
    """The iterator under a seed against the same draws assembled in NumPy."""
    r = np.random.RandomState(9)
    got = list(tb.tape_focused_batches(model, fixture_set, (24, 40), 3, indices=[0, 1, 2, 3, 2, 0], tape_crop_prob=0.8, rng=r,
                                       image_format="hwc_u8", channel_order="bgr"))
    r = np.random.RandomState(9)
    at = 0
    for image, target in got:
        samples = []
        for i in [0, 1, 2, 3, 2, 0][at:at + 3]:
            h, w = fixture_set.sizes[i]
            crop = tb.draw_tape_crop(r, h, w, int((items[1][i] == 2).sum()), 0.8)
            kw = tb.draw_cable_defect(r)[0]
            samples.append(tb.sample(i, rect=None if crop is None else tb.tape_crop_rect_np(items[1][i], *crop)[:4], **kw))
        plan, luts = tb.build_plan(samples, fixture_set.sizes)
        same(torch_cuda, (image, target), tb.assemble_np(*items, plan, luts, (24, 40), image_format="hwc_u8", channel_order="bgr"))
        at += 3


# ---- the smallest shapes at which the assembly can go wrong -------------------------------------------------------------------------------
EDGE_SIZES = [(1, 1), (1, 29), (23, 1), (19, 45), (40, 33), (70, 67)]


@pytest.fixture(scope="module")
def edge(model):
    images, masks = make_items(EDGE_SIZES, 5)
    return images, masks, tb.TrainSet(model, images, masks, align=1)       # items at odd offsets of the arenas


@pytest.mark.parametrize("size_hw", [(1, 1), (17, 23), (33, 53), (40, 65), (7, 131)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt", [dict(), dict(image_format="hwc_u8"), dict(image_format="hwc_u8", channel_order="bgr")],
                         ids=["chw_f32", "hwc_rgb", "hwc_bgr"])
def test_random_plans(torch_cuda, model, edge, size_hw, fmt):
    """Every stage drawn independently over items from 1 x 1 to more than a tile: output widths (and 3 W) that are no multiple
    of 16, more than one tile per axis, up- and downscaling in one batch, rot90 of non-square crops, crops of one pixel."""
    images, masks, ts = edge
    r = np.random.default_rng(size_hw[0] * 1000 + size_hw[1])
    samples = random_samples(r, ts.sizes, 9)
    samples += [tb.sample(0, rot90=1, value_lut=tb.value_scale_lut(1.3)), tb.sample(1, flip_h=True, rot90=3), tb.sample(2, rot90=1),
                tb.sample(5, rect=(66, 69, 67, 70), post_flip_v=True), tb.sample(3, rect=(2, 3, 40, 10), rot90=1)]
    both(torch_cuda, model, ts, images, masks, samples, size_hw, tb.class_lut({3: 0, 4: 0, 5: 0, 6: 0}), **fmt)


def test_identity_size_gives_the_source_bytes(torch_cuda, model, edge):
    images, masks, ts = edge
    for i, (h, w) in enumerate(ts.sizes):
        image, target = both(torch_cuda, model, ts, images, masks, [tb.sample(i)], (h, w), image_format="hwc_u8")
        assert (image[0].cpu().numpy() == images[i]).all() and (target[0].cpu().numpy() == masks[i]).all()
        image, _ = both(torch_cuda, model, ts, images, masks, [tb.sample(i)], (h, w))
        assert image[0].cpu().numpy().tobytes() == (images[i].astype(np.float32) / 255.0).transpose(2, 0, 1).tobytes()


def test_batch_of_one_and_a_batch_of_one_item(torch_cuda, model, edge):
    images, masks, ts = edge
    both(torch_cuda, model, ts, images, masks, [tb.sample(4, flip_v=True, value_lut=tb.value_scale_lut(0.7))], (21, 19))
    r = np.random.default_rng(2)
    samples = [s for s in random_samples(r, [ts.sizes[3]] * 1, 6)]
    samples = [dict(s, item=3) for s in samples]
    both(torch_cuda, model, ts, images, masks, samples, (16, 48))


def test_brightness_step_on_every_grey_and_saturated_colour(torch_cuda, model):
    """A source made of the colours where the HSV conversions branch: greys (s = 0), each channel the maximum, ties between two
    channels, the extremes."""
    v = np.arange(256, dtype=np.uint8)
    r = np.random.default_rng(8)
    rows = [np.stack([v, v, v], -1), np.stack([v, v[::-1], v // 2], -1), np.stack([v // 3, v, v], -1), np.stack([v, v // 2, v], -1),
            np.stack([v, v, 255 - v], -1), r.integers(0, 256, (256, 3), dtype=np.uint8), np.stack([255 - v // 2, v, v[::-1]], -1)]
    img = np.ascontiguousarray(np.stack(rows))                     # [7,256,3]
    msk = np.zeros(img.shape[:2], np.uint8)
    ts = tb.TrainSet(model, [img], [msk])
    for factor in (0.7, 1.0, 1.3):
        both(torch_cuda, model, ts, [img], [msk], [tb.sample(0, value_lut=tb.value_scale_lut(factor))], img.shape[:2], image_format="hwc_u8")


def test_staged_and_in_place_source_rectangles(torch_cuda, model):
    """A 300 x 301 source: at 8 x 8, 40 x 33 and 150 x 151 a tile's source rectangle holds more bytes than its taps read (read
    in place), at 200 x 201 and at its own size it is staged, over several tiles and with rows at every address modulo 16."""
    images, masks = make_items([(300, 301)], 12)
    ts = tb.TrainSet(model, images, masks, align=1)
    samples = [tb.sample(0), tb.sample(0, rot90=1, flip_h=True, byte_lut=tb.convert_scale_abs_lut(1.15, -9)),
               tb.sample(0, rect=(5, 7, 290, 250), rot90=3, post_flip_h=True, value_lut=tb.value_scale_lut(1.2)),
               tb.sample(0, rect=(1, 0, 300, 299), flip_v=True, rot90=2, post_flip_v=True)]
    for size_hw in ((8, 8), (40, 33), (150, 151), (200, 201)):
        both(torch_cuda, model, ts, images, masks, samples, size_hw, image_format="hwc_u8")
    both(torch_cuda, model, ts, images, masks, samples[:1], (300, 301))
    both(torch_cuda, model, ts, images, masks, samples[1:2], (301, 300), image_format="hwc_u8", channel_order="bgr")


def test_target_dtype_and_checks(torch_cuda, model, edge):
    torch = torch_cuda
    images, masks, ts = edge
    plan, luts = tb.build_plan([tb.sample(3)], ts.sizes)
    image, target = tb.make_batch(model, ts, plan, (8, 8), luts, target_dtype=torch.int64)
    assert target.dtype == torch.int64 and image.dtype == torch.float32 and tuple(image.shape) == (1, 3, 8, 8)
    with pytest.raises(ValueError, match="rect row"):
        bad = plan.copy(); bad[0, tb.P_RECT_ROW] = 0
        tb.make_batch(model, ts, bad, (8, 8), luts)
    with pytest.raises(RuntimeError, match="rects must be"):
        tb.make_batch(model, ts, plan, (8, 8), luts, rects=torch.zeros((1, 6), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="size_hw"):
        tb.make_batch(model, ts, plan, (0, 8), luts)


# ---- the data-dependent rectangle ---------------------------------------------------------------------------------------------------------
def crafted_masks():
    """Masks for the k-th match: the class in the first and the last pixel, in the last byte of rows, only beyond one pass of
    the workgroup (4096 bytes), nowhere; sizes below one 16-byte segment and above three passes."""
    r = np.random.default_rng(4)
    out = []
    m = np.zeros((5, 3), np.uint8); m[0, 0] = m[4, 2] = 2; out.append(m)                        # first and last pixel, 15 bytes
    m = np.zeros((37, 53), np.uint8); m[:, 52] = 2; out.append(m)                               # the last byte of every row
    m = np.zeros((70, 67), np.uint8); m[62:, :] = 2; out.append(m)                              # 4690 bytes: all matches in the second pass
    m = r.integers(0, 4, (96, 130)).astype(np.uint8); out.append(m)                             # 12480 bytes, dense
    out.append(np.zeros((9, 9), np.uint8))                                                      # no match
    m = np.full((1, 1), 2, np.uint8); out.append(m)
    m = np.zeros((66, 64), np.uint8); m[65, 63] = 2; out.append(m)                              # the only match is the last byte, past a pass
    return out


@pytest.mark.parametrize("align", [1, 16, 7])
def test_crop_rects(torch_cuda, model, align):
    masks = crafted_masks()
    images = [np.zeros(m.shape + (3,), np.uint8) for m in masks]
    ts = tb.TrainSet(model, images, masks, align=align)
    req = []
    for i, m in enumerate(masks):
        n = int((m == 2).sum())
        h, w = m.shape
        for k in sorted({0, 1, n // 2, n - 2, n - 1, n, n + 5, -1}):
            for ch, cw in ((max(1, h // 2), max(1, (2 * w) // 3)), (1, 1), (h, w), (h + 3, 2 * w)):
                req.append((i, k, ch, cw, 2))
    req.append((3, 100, 40, 50, 3))                                                             # another class
    req.append((3, 0, 40, 50, 200))                                                             # a class no pixel has
    req = np.array(req)
    want = tb.crop_rects_np(masks, req)
    got = tb.crop_rects(model, ts, req[:, 0], req[:, 1], req[:, 2:4], req[:, 4]).cpu().numpy()
    assert got.dtype == np.int32 and (got == want).all(), np.argwhere((got != want).any(1))[:5]
    assert (want[:, 5] == 0).any() and ((want[:, 4] == 0) & (want[:, 5] == 1)).any()            # a stale k, and a mask without the class
    assert (ts.counts[:, 2] == [int((m == 2).sum()) for m in masks]).all()


def test_make_batch_reads_the_rect_table_without_a_synchronisation(torch_cuda, model, edge):
    """crop_rects and make_batch queued back to back on one stream; a stale k gives the whole item (valid = 0)."""
    images, masks, ts = edge
    req = np.array([(3, 5, 9, 20, 2), (4, 0, 30, 11, 1), (5, 10 ** 6, 8, 8, 2), (1, 2, 1, 7, 0)])
    rects = tb.crop_rects(model, ts, req[:, 0], req[:, 1], req[:, 2:4], req[:, 4])
    samples = [tb.sample(int(req[j, 0]), rect_row=j, flip_h=j % 2 == 1, rot90=j, post_flip_v=j == 2) for j in range(4)] + [tb.sample(2)]
    plan, luts = tb.build_plan(samples, ts.sizes)
    got = tb.make_batch(model, ts, plan, (20, 27), luts, rects=rects)
    rects_np = tb.crop_rects_np(masks, req)
    assert rects_np[2, 5] == 0 and tuple(rects_np[2, :4]) == (0, 0, 67, 70)
    same(torch_cuda, got, tb.assemble_np(images, masks, plan, luts, (20, 27), rects=rects_np))
    assert (rects.cpu().numpy() == rects_np).all()
