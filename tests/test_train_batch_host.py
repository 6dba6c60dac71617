"""Training batches without a device (unet_amd/train_batch.py): the NumPy forms against what the reference's own dataset classes
returned (tests/golden/train_batch_scenes.npz, scripts/make_golden_train_batch.py) with ==, float32 compared as bits (SHA-256
of the tensor's bytes); the draw replays against the recorded draws; the two cv2-free checks of the HSV restatement over all
2^24 colours; tape_crop_rect_np against a brute-force form; bad arguments; what is particular to include/unetpp_train_batch.h."""
import ctypes
import hashlib
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from unet_amd import _lib
from unet_amd import multiclass as mc
from unet_amd import train_batch as tb

CABLE = {"eval_native": (False, None), "eval_32x32": (False, (32, 32)), "aug_17x23": (True, (17, 23)), "aug_48x40": (True, (48, 40)),
         "aug_native": (True, None)}
PATCH = {"p32_native": (32, None, True), "p32_to17": (32, 17, True), "p33_to40x48": (33, (40, 48), True), "p32_plain": (32, (40, 48), False)}
MAP_BURR3 = {0: 0, 1: 1, 2: 2, 3: 3, 4: 0, 5: 0, 6: 0}          # tools/train_3class.py:35-43
MAP_3CLASS = {0: 0, 1: 1, 2: 2, 3: 0, 4: 0, 5: 0, 6: 0}         # tools/train_3class_high_precision.py:94-102


@pytest.fixture(scope="module")
def g():
    return load_golden("train_batch_scenes")


@pytest.fixture(scope="module")
def items(g):
    n = int(g["n_items"])
    return [g[f"img_{i}"] for i in range(n)], [g[f"msk_{i}"] for i in range(n)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check(g, key, image, target):
    """One assembled sample (image float32 [3,H,W], target uint8 [H,W]) against the reference's."""
    assert image.dtype == np.float32 and target.dtype == np.uint8
    assert target.shape == g[f"{key}_mask"].shape and (target == g[f"{key}_mask"]).all(), key
    if f"{key}_u8" in g.files:
        assert image.tobytes() == tb.divide_255_table()[g[f"{key}_u8"]].transpose(2, 0, 1).tobytes(), key
    assert sha(image) == str(g[f"{key}_sha"]), key


def one(items, smp, size_hw, class_table=None, **kw):
    sizes = [m.shape for m in items[1]]
    plan, luts = tb.build_plan([smp], sizes)
    image, target = tb.assemble_np(items[0], items[1], plan, luts, size_hw, class_table, **kw)
    return image[0], target[0]


# ---- the reference's classes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", sorted(CABLE))
def test_cable_defect_dataset(g, items, cfg):
    augment, target = CABLE[cfg]
    for s in range(int(g[f"cable_{cfg}_count"])):
        i = int(g[f"cable_{cfg}_{s}_item"])
        rng = tb.ReplayRng(g[f"cable_{cfg}_{s}_draws"], "np")
        kw = tb.draw_cable_defect(rng)[0] if augment else {}
        assert rng.exhausted(), "the replay consumed fewer draws than the reference"
        check(g, f"cable_{cfg}_{s}", *one(items, tb.sample(i, **kw), target or items[1][i].shape))


def test_a_seeded_replay_gives_the_seeded_references_batch(g, items):
    """np.random seeded as the generator seeded it: the replay on np.random itself reproduces the whole run."""
    cfg = "aug_17x23"
    state = np.random.get_state()
    try:
        np.random.seed(int(g[f"cable_{cfg}_seed"]))
        for s in range(int(g[f"cable_{cfg}_count"])):
            kw, _ = tb.draw_cable_defect(np.random)
            check(g, f"cable_{cfg}_{s}", *one(items, tb.sample(int(g[f"cable_{cfg}_{s}_item"]), **kw), CABLE[cfg][1]))
    finally:
        np.random.set_state(state)


def test_class_maps(g, items):
    burr3, three = tb.class_lut(MAP_BURR3, "zero"), tb.class_lut(MAP_3CLASS, "zero")
    keep = tb.class_lut(MAP_3CLASS, "keep")
    differ = False
    for i in range(len(items[0])):
        check(g, f"burr3_{i}", *one(items, tb.sample(i), (32, 32), burr3))
        check(g, f"hp3_{i}", *one(items, tb.sample(i), (32, 32), three))              # the dataset remaps a tensor: the torch branch
        assert (keep[items[1][i]] == g[f"remap_np_{i}"]).all() and (three[items[1][i]] == g[f"remap_torch_{i}"]).all()
        differ |= bool((g[f"remap_np_{i}"] != g[f"remap_torch_{i}"]).any())
    assert differ and keep[9] == 9 and three[9] == 0                                  # the two branches differ above 6


@pytest.mark.parametrize("name", ["adv", "adv3"])
def test_tape_focused_legacy_path(g, items, name):
    ctab = tb.class_lut({1: 1, 2: 2}, "zero") if name == "adv3" else None             # advanced_dataset.py:288-292
    cropped = 0
    for s in range(int(g[f"{name}_count"])):
        i = int(g[f"{name}_{s}_item"])
        h, w = items[1][i].shape
        rng = tb.ReplayRng(g[f"{name}_{s}_draws"], "np")
        crop = tb.draw_tape_crop(rng, h, w, int((items[1][i] == 2).sum()), tape_crop_prob=0.7)
        kw = tb.draw_cable_defect(rng)[0]
        assert rng.exhausted()
        rect = None
        if crop is not None:
            x1, y1, x2, y2, n_found, valid = tb.tape_crop_rect_np(items[1][i], *crop)
            assert valid == 1 and n_found == (items[1][i] == 2).sum()
            rect, cropped = (x1, y1, x2, y2), cropped + 1
        check(g, f"{name}_{s}", *one(items, tb.sample(i, rect=rect, **kw), (32, 32), ctab))
    assert 0 < cropped < int(g[f"{name}_count"])


def test_tape_focused_crop_alone(g, items):
    for t in range(int(g["tape_count"])):
        i = int(g[f"tape_{t}_item"])
        h, w = items[1][i].shape
        rng = tb.ReplayRng(g[f"tape_{t}_draws"], "np")
        crop = tb.draw_tape_crop(rng, h, w, int((items[1][i] == 2).sum()))
        assert rng.exhausted()
        want = tuple(int(v) for v in g[f"tape_{t}_rect"])
        if crop is None:
            assert want == (0, 0, w, h) and tb.tape_crop_rect_np(items[1][i], 0, h, w)[:4] == want
        else:
            assert tb.tape_crop_rect_np(items[1][i], *crop)[:4] == want, t


@pytest.mark.parametrize("cfg", sorted(PATCH))
def test_patch_defect_dataset(g, items, cfg):
    ps, target, augment = PATCH[cfg]
    sizes = [m.shape for m in items[1]]
    tables = np.concatenate([mc.class_table_np(m[None]) for m in items[1]])
    defect, boxes, normal = tb.defect_bboxes(tables)
    assert defect == list(g[f"patch_{cfg}_defect_items"]) and normal == list(g[f"patch_{cfg}_normal_items"])
    assert np.array_equal(np.array(boxes), g[f"patch_{cfg}_bboxes"])
    types = g[f"patch_{cfg}_types"]
    hw = (ps, ps) if target is None else ((target, target) if isinstance(target, int) else (target[1], target[0]))
    for s in range(int(g[f"patch_{cfg}_count"])):
        rng = tb.ReplayRng(g[f"patch_{cfg}_{s}_draws"], "py")
        smp = tb.draw_patch(rng, "defect" if types[s % len(types)] else "normal", ps, sizes, defect, boxes, normal, augment)
        assert rng.exhausted()
        check(g, f"patch_{cfg}_{s}", *one(items, smp, hw, tb.binary_defect_lut()))


def test_a_seeded_patch_replay_gives_the_seeded_references_batch(g, items):
    cfg = "p32_to17"
    ps, target, augment = PATCH[cfg]
    sizes = [m.shape for m in items[1]]
    defect, boxes, normal = tb.defect_bboxes(np.concatenate([mc.class_table_np(m[None]) for m in items[1]]))
    types = g[f"patch_{cfg}_types"]
    rng = random.Random(int(g[f"patch_{cfg}_seed"]))
    for s in range(int(g[f"patch_{cfg}_count"])):
        smp = tb.draw_patch(rng, "defect" if types[s % len(types)] else "normal", ps, sizes, defect, boxes, normal, augment)
        check(g, f"patch_{cfg}_{s}", *one(items, smp, (target, target), tb.binary_defect_lut()))


def test_replay_notices_a_wrong_order(g):
    d = g["cable_aug_17x23_0_draws"]
    with pytest.raises(AssertionError, match="recorded"):
        tb.ReplayRng(d, "np").randint(0, 5)
    r = tb.ReplayRng(d[:2], "np")
    with pytest.raises(AssertionError, match="after the 2 recorded"):
        tb.draw_cable_defect(r)


# ---- forms and formats ----------------------------------------------------------------------------------------------------------------
def test_equal_size_gives_the_source_bytes_and_formats_agree(items):
    for i, (img, msk) in enumerate(zip(*items)):
        rgb, t = one(items, tb.sample(i), msk.shape, image_format="hwc_u8")
        bgr, _ = one(items, tb.sample(i), msk.shape, image_format="hwc_u8", channel_order="bgr")
        f32, _ = one(items, tb.sample(i), msk.shape)
        assert (rgb == img).all() and (t == msk).all() and (bgr == img[..., ::-1]).all()
        assert f32.tobytes() == (img.astype(np.float32) / 255.0).transpose(2, 0, 1).tobytes()


def test_geometry_on_both_sides_of_the_resize_differs(items):
    """cv2's float32 tap positions are not mirror-symmetric at every size pair (53 -> 131 is one where two columns get other
    coefficients): there a flip before the resize and a flip after it are different images."""
    a, _ = one(items, tb.sample(0, flip_h=True), (17, 131), image_format="hwc_u8")
    b, _ = one(items, tb.sample(0, post_flip_h=True), (17, 131), image_format="hwc_u8")
    assert a.shape == b.shape and (a != b).any()
    # at equal size both are the mirrored source
    a, _ = one(items, tb.sample(2, flip_h=True, flip_v=True), items[1][2].shape, image_format="hwc_u8")
    b, _ = one(items, tb.sample(2, post_flip_h=True, post_flip_v=True), items[1][2].shape, image_format="hwc_u8")
    assert (a == b).all() and (a == items[0][2][::-1, ::-1]).all()


def test_rot90_matches_numpy(items):
    img, msk = items[0][0], items[1][0]
    for k in range(4):
        for fh in (False, True):
            want_i, want_m = np.rot90(np.fliplr(img) if fh else img, k), np.rot90(np.fliplr(msk) if fh else msk, k)
            got_i, got_m = one(items, tb.sample(0, flip_h=fh, rot90=k), want_m.shape, image_format="hwc_u8")
            assert (got_i == want_i).all() and (got_m == want_m).all()


def test_look_up_builders():
    d = tb.divide_255_table()
    assert d.dtype == np.float32 and d.shape == (256,) and d.tobytes() == (np.arange(256).astype(np.float32) / 255.0).astype(np.float32).tobytes()
    for factor in (0.7, 1.0, 1.3, 0.7 + 0.123456789 * 0.6):
        hsv_v = np.arange(256, dtype=np.uint8).astype(np.float32)
        hsv_v *= factor                                                            # dataset.py:129, on a float32 array
        assert (tb.value_scale_lut(factor) == np.clip(hsv_v, 0, 255).astype(np.uint8)).all()
    lut = tb.convert_scale_abs_lut(1.2, -20)
    assert lut[0] == 20 and lut[16] == 1 and lut[17] == 0 and lut[255] == 255 and tb.convert_scale_abs_lut(0.5, 0.5)[1] == 1
    assert tb.convert_scale_abs_lut(0.5, 0)[5] == 2 and tb.convert_scale_abs_lut(0.5, 0)[7] == 4          # 2.5 -> 2, 3.5 -> 4
    assert (tb.binary_defect_lut()[:8] == [0, 0, 0, 1, 1, 1, 0, 0]).all()


# ---- the HSV restatement, over all 2^24 colours -----------------------------------------------------------------------------------
def test_hsv_value_is_the_maximum_and_grey_stays_grey():
    v = np.arange(256, dtype=np.uint8)
    for r in range(0, 256):
        rgb = np.stack(np.meshgrid(np.uint8(r), v, v, indexing="ij"), -1).reshape(-1, 3)
        h, s, val = tb.rgb_to_hsv_u8_np(rgb)
        assert (val == rgb.max(1)).all() and h.max() < 180
        assert (s[rgb.min(1) == rgb.max(1)] == 0).all()
    grey = np.stack([v, v, v], -1)
    rng = np.random.default_rng(3)
    for table in [v, tb.value_scale_lut(0.7), tb.value_scale_lut(1.3), v[::-1].copy()] + [rng.integers(0, 256, 256, dtype=np.uint8) for _ in range(8)]:
        assert (tb.hsv_value_scale_np(grey, table) == np.stack([table] * 3, -1)).all()      # (T[v], T[v], T[v]); unchanged for the identity


def test_hsv_round_trip_bound_is_the_measured_one(g):
    v = np.arange(256, dtype=np.uint8)
    worst = 0
    for r in range(256):
        rgb = np.stack(np.meshgrid(np.uint8(r), v, v, indexing="ij"), -1).reshape(-1, 3)
        worst = max(worst, int(np.abs(tb.hsv_value_scale_np(rgb, v).astype(np.int64) - rgb).max()))
    assert worst == int(g["hsv_round_trip_levels"]) == 5
    with open(os.path.join(ROOT, "tests", "golden", "README_train_batch.txt")) as f:
        assert f"at most {worst} levels per channel" in f.read()


# ---- the data-dependent rectangle -------------------------------------------------------------------------------------------------------
def brute_rect(mask, k, crop_h, crop_w, cls):
    h, w = mask.shape
    seen, centre = 0, None
    for y in range(h):
        for x in range(w):
            if mask[y, x] == cls:
                if seen == k:
                    centre = (y, x)
                seen += 1
    if seen == 0:
        return (0, 0, w, h, 0, 1)
    if centre is None:
        return (0, 0, w, h, seen, 0)
    cy, cx = centre
    out = []
    for c, half, size, n in ((cx, crop_w // 2, crop_w, w), (cy, crop_h // 2, crop_h, h)):
        lo, hi = max(0, c - half), min(n, c + half)
        if hi - lo < size:
            if lo == 0:
                hi = min(n, size)
            else:
                lo = max(0, hi - size)
        out.append((lo, hi))
    return (out[0][0], out[1][0], out[0][1], out[1][1], seen, 1)


def test_tape_crop_rect_against_brute_force():
    rng = np.random.default_rng(11)
    smaller = stale = empty = 0
    for n in range(3000):
        h, w = (int(v) for v in rng.integers(1, 13, 2))
        mask = rng.integers(0, 4, (h, w)).astype(np.uint8) if n % 7 else np.zeros((h, w), np.uint8)
        count = int((mask == 2).sum())
        k = int(rng.integers(0, count + 2)) if n % 5 else -1
        ch, cw = (int(v) for v in rng.integers(1, 16, 2))                          # also larger than the image
        got = tb.tape_crop_rect_np(mask, k, ch, cw)
        assert got == brute_rect(mask, k, ch, cw, 2), (n, mask, k, ch, cw)
        x1, y1, x2, y2, n_found, valid = got
        assert 0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h and n_found == count
        smaller += valid and count and (x2 - x1 < cw or y2 - y1 < ch)
        stale += not valid
        empty += count == 0
    assert smaller > 100 and stale > 100 and empty > 100
    assert tb.tape_crop_rect_np(np.array([[2, 0, 2]], np.uint8), 1, 1, 1) == (1, 0, 2, 1, 2, 1)      # crop // 2 == 0: the lines' own 1 x 1, beside the centre
    assert (tb.crop_rects_np([np.full((3, 4), 2, np.uint8)], [[0, 11, 2, 2, 2], [0, 12, 2, 2, 2]]) == [[2, 1, 4, 3, 12, 1], [0, 0, 4, 3, 12, 0]]).all()


# ---- bad arguments ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise(items):
    images, masks = items
    sizes = [m.shape for m in masks]
    plan, luts = tb.build_plan([tb.sample(0)], sizes)
    with pytest.raises(ValueError, match="rect"):
        tb.build_plan([tb.sample(0, rect=(0, 0, 54, 10))], sizes)
    with pytest.raises(ValueError, match="rect"):
        tb.build_plan([tb.sample(0, rect=(5, 0, 5, 10))], sizes)
    with pytest.raises(ValueError, match="not both"):
        tb.sample(0, rect=(0, 0, 1, 1), rect_row=0)
    with pytest.raises(ValueError, match="item"):
        tb.build_plan([tb.sample(4)], sizes)
    with pytest.raises(ValueError, match="at least one"):
        tb.build_plan([], sizes)
    with pytest.raises(ValueError, match=r"uint8 \[256\]"):
        tb.sample(0, byte_lut=np.zeros(255, np.uint8))
    with pytest.raises(ValueError, match="size_hw"):
        tb.assemble_np(images, masks, plan, luts, (0, 5))
    with pytest.raises(ValueError, match="image_format"):
        tb.assemble_np(images, masks, plan, luts, (8, 8), image_format="nhwc")
    with pytest.raises(ValueError, match="channel_order"):
        tb.assemble_np(images, masks, plan, luts, (8, 8), channel_order="bgr")
    with pytest.raises(ValueError, match="plan must be int32"):
        tb.assemble_np(images, masks, plan.astype(np.int64), luts, (8, 8))
    bad = plan.copy(); bad[0, tb.P_BYTE_LUT] = 0
    with pytest.raises(ValueError, match="look-up row"):
        tb.assemble_np(images, masks, bad, luts, (8, 8))
    bad = plan.copy(); bad[0, tb.P_RECT_ROW] = 0
    with pytest.raises(ValueError, match="rect row"):
        tb.assemble_np(images, masks, bad, luts, (8, 8))
    with pytest.raises(ValueError, match="same size"):
        tb.assemble_np(images, [m[:-1] for m in masks], plan, luts, (8, 8))
    with pytest.raises(ValueError, match="crop size"):
        tb.tape_crop_rect_np(masks[0], 0, 0, 4)
    with pytest.raises(ValueError, match="crop_h and crop_w"):
        tb.crop_rects_np(masks, [[0, 0, 0, 4, 2]])
    with pytest.raises(ValueError, match="item outside"):
        tb.crop_rects_np(masks, [[9, 0, 4, 4, 2]])
    with pytest.raises(ValueError, match="default"):
        tb.class_lut({}, "one")
    with pytest.raises(ValueError, match="outside 0..255"):
        tb.class_lut({3: 256})


# ---- the header's entries (names, types, build inputs and guard coverage: tests/test_bindings_host.py) ------------------------------------
def test_the_kernel_reuses_the_resize_helpers_and_has_no_atomics():
    with open(os.path.join(_lib.CSRC, "train_batch.h")) as f:
        kernel = f.read()
    assert "roi_linear_coef(int" not in kernel and "rf_store_row(const" not in kernel                            # reused, not copied
    assert not re.search(r"\batomic[A-Z]\w*\s*\(", kernel)                                                      # no atomics on outputs


def test_header_is_c99(tmp_path):
    cc_ = shutil.which("cc") or shutil.which("gcc")
    assert cc_, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "unetpp_train_batch.h"\nint main(void) { int p[UNETPP_TRAIN_PLAN_COLUMNS] = {0}; (void)p; '
                   'return UNETPP_TRAIN_PLAN_COLUMNS - 16 + UNETPP_TRAIN_HWC_BGR - 2; }\n')
    subprocess.run([cc_, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True, text=True)


def test_layout_and_null_engine():
    lib = _lib.load()
    assert tb.layout() == (32, 32, 4096, tb.PLAN_COLS)
    assert (tb.PLAN_COLS, tb.RECT_COLS, tb.REQUEST_COLS, tb.ITEM_COLS) == (16, 6, 5, 4)
    v = ctypes.c_int(0)
    assert lib.unetpp_train_batch_layout(ctypes.byref(v), None, ctypes.byref(v), ctypes.byref(v)) == -2
    assert lib.unetpp_train_crop_rects(None, None, 1, None, 1, None, 1, None, None) == -1
    assert lib.unetpp_train_batch_u8(None, None, 3, None, 1, None, 1, None, 1, None, 0, None, 0, None, 8, 8, 0, None, None, None) == -1


def test_guard_cases_visit_every_offset():
    import test_gpu_guarded_train_batch as tgt
    assert {a for a, _, _ in tgt.ARENA_OFFSETS} == set(range(16)) and {m for _, m, _ in tgt.ARENA_OFFSETS} == set(range(16))
    assert {o for _, _, o in tgt.ARENA_OFFSETS} == set(range(16)) and set(tgt.FLOAT_PHASES) == {0, 4, 8, 12}
