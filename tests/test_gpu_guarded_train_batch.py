"""Guard-band tests of the ninth binding table (include/unetpp_train_batch.h): both launching entries with every tensor between
random guard bytes (tests/guarded.py), with the assertions of tests/test_gpu_guarded.py: guards intact, equal to the NumPy form
bit for bit, the same bits with the filling complemented (so nothing outside the tensors reaches the result and every output
byte is written), inputs unchanged.
  train_batch: the image arena and the mask arena each at byte offsets 0..15, the uint8 outputs (the target, and the image in its
               hwc_u8 form) at 0..15, the float32 image at each 4-byte phase of a 16-byte line; items at odd offsets inside the
               arenas; ragged output sizes (W and 3 W no multiples of 16, more than one tile); a rect table read from the device.
  crop_rects:  the mask arena at 0..15, masks below one 16-byte segment and above one pass of the workgroup.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_train_batch.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_guarded as tg
from test_gpu_guarded import model, torch_cuda  # noqa: F401  (fixtures)
from unet_amd import train_batch as tb

COVERED = {"unetpp_train_batch_u8": "test_train_batch_f32, test_train_batch_u8", "unetpp_train_crop_rects": "test_crop_rects"}
# Symbols of the ninth table that write no caller-provided device buffer.
EXCLUDED_TRAIN_BATCH = {"unetpp_train_batch_layout": "layout query"}

# (image arena offset, mask arena offset, uint8 output offset): each runs through 0..15
ARENA_OFFSETS = [(a, (5 * a + 3) % 16, (11 * a + 7) % 16) for a in range(16)]
FLOAT_PHASES = (0, 4, 8, 12)
SIZES = [(1, 1), (19, 45), (40, 33), (70, 67)]
OUT_SIZES = [(17, 23), (33, 53)]


def scene(seed):
    r = np.random.default_rng(seed)
    images = [r.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    masks = [r.integers(0, 7, (h, w), dtype=np.uint8) for h, w in SIZES]
    items = np.zeros((len(SIZES), tb.ITEM_COLS), np.int64)
    io = mo = 0
    for i, (h, w) in enumerate(SIZES):
        io, mo = io + (i % 3), mo + ((2 * i + 1) % 5)                # gaps, so that items start at odd offsets
        items[i] = (io, mo, h, w)
        io, mo = io + 3 * h * w, mo + h * w
    arena_i, arena_m = r.integers(0, 256, io, dtype=np.uint8), r.integers(0, 256, mo, dtype=np.uint8)
    for (a, b, h, w), im, m in zip(items, images, masks):
        arena_i[a:a + 3 * h * w], arena_m[b:b + h * w] = im.reshape(-1), m.reshape(-1)
    samples = [tb.sample(3, rect_row=0, flip_h=True, rot90=1, byte_lut=tb.convert_scale_abs_lut(1.1, -7)),
               tb.sample(1, rect=(3, 2, 40, 17), flip_v=True, post_flip_h=True, value_lut=tb.value_scale_lut(1.25)),
               tb.sample(0, rot90=3, value_lut=tb.value_scale_lut(0.8)),
               tb.sample(2, rot90=2, post_flip_v=True, byte_lut=tb.convert_scale_abs_lut(0.9, 12), value_lut=tb.value_scale_lut(0.75)),
               tb.sample(3, rect=(66, 69, 67, 70))]
    plan, luts = tb.build_plan(samples, SIZES)
    req = np.array([(3, 40, 30, 41, 2)])
    return images, masks, items, arena_i, arena_m, plan, luts, req


def placed_set(g, model, items, arena_i, arena_m, ai, am):
    dev_i, dev_m = g.place(arena_i, ai, "image arena"), g.place(arena_m, am, "mask arena")
    return tb.TrainSet.resident(model, dev_i, dev_m, items, g.place(items, 8, "items"), stats=False), dev_i, dev_m


def run_batch(torch, model, ai, am, uo, size_hw, fmt, phase=0):
    from unet_amd import _lib
    images, masks, items, arena_i, arena_m, plan, luts, req = scene(ai)
    rects_np = tb.crop_rects_np(masks, req)
    ctab = tb.class_lut({3: 1, 4: 1, 5: 1}, "zero")
    want = tb.assemble_np(images, masks, plan, luts, size_hw, ctab, rects_np, **fmt)
    seen = {}

    def run(g):
        ts, dev_i, dev_m = placed_set(g, model, items, arena_i, arena_m, ai, am)
        rects = g.place(rects_np, 4, "rects")
        with g.allocations(models=[model], lib_module=_lib):
            out = tb.make_batch(model, ts, plan, size_hw, luts, ctab, rects, **fmt)
            torch.cuda.synchronize()
        seen["symbols"] = set(g.symbols) - set(tg.EXCLUDED)
        assert dev_i.data_ptr() % 16 == ai and dev_m.data_ptr() % 16 == am and out[1].data_ptr() % 16 == uo
        assert out[0].data_ptr() % 16 == (phase if not fmt else uo)
        for t, a in ((dev_i, arena_i), (dev_m, arena_m), (ts.items, items), (rects, rects_np)):
            assert t.cpu().numpy().tobytes() == a.tobytes(), "an input was written"
        return out

    got = guarded.two_fillings(torch, run, seed=ai + 16 * am, u8_out_offset=uo,
                               align=lambda s, dtype, ctx: phase if len(s) == 4 and dtype == torch.float32 else None)
    assert seen["symbols"] == {"unetpp_train_batch_u8"}
    for (_, dtype, shp, raw), w in zip(got, want):
        assert dtype == str(w.dtype) and tuple(shp) == w.shape
        assert np.array_equal(raw, np.ascontiguousarray(w).view(np.uint8).reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("ai,am,uo", ARENA_OFFSETS)
def test_train_batch_f32(torch_cuda, model, ai, am, uo):  # noqa: F811
    run_batch(torch_cuda, model, ai, am, uo, OUT_SIZES[ai % 2], {}, phase=FLOAT_PHASES[ai % 4])


@pytest.mark.gpu
@pytest.mark.parametrize("phase", FLOAT_PHASES)
@pytest.mark.parametrize("size_hw", OUT_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_train_batch_f32_phases(torch_cuda, model, size_hw, phase):  # noqa: F811
    run_batch(torch_cuda, model, 1, 2, 3, size_hw, {}, phase=phase)


@pytest.mark.gpu
@pytest.mark.parametrize("ai,am,uo", ARENA_OFFSETS)
def test_train_batch_u8(torch_cuda, model, ai, am, uo):  # noqa: F811
    run_batch(torch_cuda, model, ai, am, uo, OUT_SIZES[(ai + 1) % 2], dict(image_format="hwc_u8", channel_order="bgr" if ai % 2 else "rgb"))


@pytest.mark.gpu
@pytest.mark.parametrize("am", range(16))
def test_crop_rects(torch_cuda, model, am):  # noqa: F811
    from unet_amd import _lib
    torch = torch_cuda
    images, masks, items, arena_i, arena_m, _, _, _ = scene(100 + am)
    req = []
    for i, m in enumerate(masks):
        n = int((m == 2).sum())
        req += [(i, k, max(1, m.shape[0] // 2), max(1, m.shape[1] // 2), 2) for k in (0, n // 2, n - 1, n)]
    req.append((3, 0, 5, 5, 9))                                      # a class no pixel has
    req = np.array(req)
    want = tb.crop_rects_np(masks, req)
    seen = {}

    def run(g):
        ts, dev_i, dev_m = placed_set(g, model, items, arena_i, arena_m, 0, am)
        with g.allocations(models=[model], lib_module=_lib):
            out = tb.crop_rects(model, ts, req[:, 0], req[:, 1], req[:, 2:4], req[:, 4])
            torch.cuda.synchronize()
        seen["symbols"] = set(g.symbols) - set(tg.EXCLUDED)
        assert dev_m.data_ptr() % 16 == am
        assert dev_m.cpu().numpy().tobytes() == arena_m.tobytes() and ts.items.cpu().numpy().tobytes() == items.tobytes()
        return out

    (_, dtype, shp, raw), = guarded.two_fillings(torch, run, seed=am)
    assert seen["symbols"] == {"unetpp_train_crop_rects"} and dtype == "int32" and tuple(shp) == want.shape
    assert np.array_equal(raw.view(np.int32).reshape(want.shape), want)
