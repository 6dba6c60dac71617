#!/usr/bin/env python3
"""Generate tests/golden/train_batch_scenes.npz and tests/golden/README_train_batch.txt from the REFERENCE's own dataset classes.

    python scripts/make_golden_train_batch.py

Runs where the reference source is checked out, on CPU torch; only the small .npz and the text file travel.  The reference's code
runs unchanged over the golden scripts' cv2 stub (make_golden_burr.cv2_stub), extended here with flip, convertScaleAbs, the two
colour conversions and the two resizes on the project's restatements, and with imdecode answering from an in-memory table.  The
files the classes list and open are written to a temporary directory: lossless PNG data (under the .jpg names PatchDefectDataset
globs for), which PIL decodes for patch_dataset.py and the stub's imdecode recognises by its bytes for dataset.py.

What runs, under fixed seeds, with every draw of np.random / random recorded:
  cable_<cfg>     CableDefectDataset.__getitem__ (src/data/dataset.py): augment off / on, target_size None / given
  burr3           CableTapeBurrDataset.__getitem__ (tools/train_3class.py)
  remap_np/_torch both branches of remap_mask_to_3class (tools/train_3class_high_precision.py), and its CableDefectDataset3Class
  adv / adv3      CableDefectDatasetAdvanced / CableDefectDataset3Class (src/data/advanced_dataset.py): the legacy path with the
                  tape-focused crop in front
  tape_<n>        _tape_focused_crop alone, on an image of coordinates, so that the rectangle can be read from the result
  patch_<cfg>     PatchDefectDataset.__init__ and __getitem__ (src/data/patch_dataset.py): _crop_patch for both sample kinds,
                  _augment, the resize and the binary target

Keys.  items: img_<i> uint8 [h,w,3] RGB, msk_<i> uint8 [h,w].  Per sample <s> of a run: <run>_<s>_sha the SHA-256 of the
returned float32 CHW bytes; for the first two samples of a run also <run>_<s>_u8 uint8 [H,W,3] = the image times 255 (the
generator asserts for every sample that divide_255_table()[u8] has the image's bits); <run>_<s>_mask uint8 [H,W] (returned as
int64; the generator asserts the range),
<run>_<s>_draws float64 [n,2] = (generator call, value) with the calls numbered as unet_amd.train_batch.DRAW_CODES, <run>_<s>_item.
"""
from __future__ import annotations

import importlib
import io
import os
import random
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_golden  # noqa: E402  (REF, sha, and the repository root on sys.path)
import make_golden_burr  # noqa: E402  (cv2_stub)

OUT = os.path.join(ROOT, "tests", "golden", "train_batch_scenes.npz")
README = os.path.join(ROOT, "tests", "golden", "README_train_batch.txt")

CABLE_CONFIGS = [("eval_native", False, None, 1), ("eval_32x32", False, (32, 32), 1), ("aug_17x23", True, (17, 23), 5),
                 ("aug_48x40", True, (48, 40), 4), ("aug_native", True, None, 1)]
# (name, patch_size, target_size, augment, repetitions)
PATCH_CONFIGS = [("p32_native", 32, None, True, 3), ("p32_to17", 32, 17, True, 3), ("p33_to40x48", 33, (40, 48), True, 4),
                 ("p32_plain", 32, (40, 48), False, 1)]


# ---- the items ---------------------------------------------------------------------------------------------------------------------
def make_items():
    """Four small items: 37 x 53 and 96 x 130 with tape and defects, two of 64 x 48 without defects, one of them without tape
    and with a byte no class has."""
    r = np.random.default_rng(20261021)
    images, masks = [], []
    for i, (h, w) in enumerate([(37, 53), (64, 48), (96, 130), (64, 48)]):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([40 + 150 * xx / w + 30 * np.sin(yy / 5.0), 200 - 120 * yy / h + 20 * np.cos(xx / 7.0), 90 + 60 * np.sin((xx + yy) / 9.0)], -1)
        img = np.clip(base + r.integers(-10, 11, (h, w, 3)), 0, 255).astype(np.uint8)
        img[h // 3:h // 3 + 3, :, :] = (img[h // 3:h // 3 + 3, :, :] // 16) * 16 + 7                 # a band of near-grey steps
        img[:, w // 2:w // 2 + 2, :] = img[:, w // 2:w // 2 + 2, :1]                                # two grey columns (s = 0)
        m = np.zeros((h, w), np.uint8)
        m[h // 4:3 * h // 4, :] = 1
        if i != 1:
            m[h // 4:3 * h // 4, w // 5:w // 5 + max(3, w // 6)] = 2
            m[h // 3:h // 2, w - 4:w] = 2                                                            # tape in the last byte of rows
            m[0, 0] = 2                                                                              # and in the first pixel
        if i == 0:
            m[5:9, 30:36], m[20:23, 2:5] = 3, 4
        if i == 2:
            m[90:96, 120:130], m[40:44, 60:70] = 5, 3                                                # a box that touches two borders
        if i == 1:
            m[10:14, 10:20], m[30:33, 5:9] = 6, 9
        images.append(img)
        masks.append(m)
    return images, masks


def png_bytes(a):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="PNG")
    return buf.getvalue()


# ---- the stub and the imports ------------------------------------------------------------------------------------------------------------
def cv2_stub(mo, ed, tb, tl, rb, table):
    cv2 = make_golden_burr.cv2_stub(mo, ed)
    cv2.IMREAD_COLOR, cv2.IMREAD_UNCHANGED = 1, -1
    cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2HSV, cv2.COLOR_HSV2RGB = 4, 41, 55
    cv2.INTER_NEAREST, cv2.INTER_LINEAR = 0, 1

    def imdecode(buf, flag):
        a = table[bytes(np.asarray(buf, np.uint8).tobytes())]
        if flag == cv2.IMREAD_COLOR:
            assert a.ndim == 3
            return a[..., ::-1].copy()                        # BGR, as cv2 decodes
        assert flag == cv2.IMREAD_UNCHANGED and a.ndim == 2
        return a.copy()

    def cvtColor(img, code):
        if code == cv2.COLOR_BGR2RGB:
            return img[..., ::-1].copy()
        if code == cv2.COLOR_RGB2HSV:
            return np.stack(tb.rgb_to_hsv_u8_np(img), -1)
        assert code == cv2.COLOR_HSV2RGB and img.dtype == np.uint8
        return tb.hsv_to_rgb_u8_np(img[..., 0], img[..., 1], img[..., 2])

    def resize(img, dsize, interpolation):
        img = np.ascontiguousarray(img)
        assert img.dtype == np.uint8
        if interpolation == cv2.INTER_LINEAR:
            return tl.resize_linear_u8_np(img, tuple(dsize))
        assert interpolation == cv2.INTER_NEAREST
        return np.ascontiguousarray(rb.resize_nearest_np(img, tuple(dsize)))

    def flip(img, code):
        assert code in (0, 1)
        return np.ascontiguousarray(img[:, ::-1] if code == 1 else img[::-1])

    def convertScaleAbs(img, alpha=1.0, beta=0.0):
        assert img.dtype == np.uint8
        return tb.convert_scale_abs_lut(alpha, beta)[img]

    cv2.imdecode, cv2.cvtColor, cv2.resize, cv2.flip, cv2.convertScaleAbs = imdecode, cvtColor, resize, flip, convertScaleAbs
    return cv2


def import_reference(stub):
    sys.modules["cv2"] = stub
    for name in ("torchvision", "torchvision.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    for p in (os.path.join(make_golden.REF, "tools"), os.path.join(make_golden.REF, "src")):
        if p not in sys.path:
            sys.path.insert(0, p)
    mods = {n: importlib.import_module(n) for n in ("data.dataset", "data.patch_dataset", "data.advanced_dataset", "train_3class",
                                                    "train_3class_high_precision")}
    assert not mods["data.advanced_dataset"].ALBUMENTATIONS_AVAILABLE, "the legacy path is the pinned one"
    return mods


class Recorder:
    """Wraps the generator calls the reference makes and logs (code, value) of each."""

    def __init__(self):
        self.log = []
        self.saved = {}

    def __enter__(self):
        def wrap(owner, name, code):
            orig = getattr(owner, name)
            self.saved[(owner, name)] = orig

            def call(*a, **k):
                v = orig(*a, **k)
                self.log.append((code, float(v)))
                return v
            setattr(owner, name, call)
        from unet_amd.train_batch import DRAW_CODES
        for owner, prefix, names in ((np.random, "np.random.", ("random", "randint")), (random, "random.", ("random", "randint", "uniform"))):
            for name in names:
                wrap(owner, name, DRAW_CODES[prefix + name])
        return self

    def __exit__(self, *exc):
        for (owner, name), orig in self.saved.items():
            setattr(owner, name, orig)

    def take(self):
        out = np.array(self.log, np.float64).reshape(-1, 2)
        self.log.clear()
        return out


def store(payload, tb, key, image, mask, draws, item):
    """One returned (image, mask) pair of the reference, checked and reduced as the module docstring says."""
    import torch
    assert image.dtype == torch.float32 and mask.dtype == torch.int64 and image.dim() == 3 and image.shape[0] == 3
    img = image.numpy()
    u8 = np.rint(img * 255.0).astype(np.uint8).transpose(1, 2, 0)
    assert tb.divide_255_table()[u8].transpose(2, 0, 1).tobytes() == np.ascontiguousarray(img).tobytes(), key
    m = mask.numpy()
    assert m.min() >= 0 and m.max() <= 255
    payload[f"{key}_sha"] = np.array(make_golden.sha(img))
    if key.rsplit("_", 1)[1] in ("0", "1"):                   # the bytes themselves for the first two samples of a run
        payload[f"{key}_u8"] = np.ascontiguousarray(u8)
    payload[f"{key}_mask"], payload[f"{key}_draws"], payload[f"{key}_item"] = m.astype(np.uint8), draws, np.array(item)


def main():
    import torch
    make_golden._load_synthetic()
    from unet_amd import edges as ed
    from unet_amd import morphology as mo
    from unet_amd import robust as rb
    from unet_amd import tiling as tl
    from unet_amd import train_batch as tb
    images, masks = make_items()
    table = {}
    ref = import_reference(cv2_stub(mo, ed, tb, tl, rb, table))
    payload = {"n_items": np.array(len(images))}
    seen = {"cable": set(), "patch": set(), "clip": set(), "tape_none": False, "adv_crop": set()}
    with tempfile.TemporaryDirectory() as tmp:
        idir, mdir = os.path.join(tmp, "images"), os.path.join(tmp, "masks")
        os.makedirs(idir); os.makedirs(mdir)
        for i, (im, m) in enumerate(zip(images, masks)):
            payload[f"img_{i}"], payload[f"msk_{i}"] = im, m
            for path, a in ((os.path.join(idir, f"a{i}.jpg"), im), (os.path.join(mdir, f"a{i}.png"), m)):
                data = png_bytes(a)
                table[data] = a
                with open(path, "wb") as f:
                    f.write(data)
        n = len(images)
        with Recorder() as rec:
            # ---- CableDefectDataset
            for cfg, augment, target, reps in CABLE_CONFIGS:
                ds = ref["data.dataset"].CableDefectDataset(idir, mdir, augment=augment, target_size=target)
                assert len(ds) == n
                np.random.seed(3000 + len(cfg))
                payload[f"cable_{cfg}_seed"] = np.array(3000 + len(cfg))
                for s in range(reps * n):
                    rec.take()
                    image, mask = ds[s % n]
                    d = rec.take()
                    store(payload, tb, f"cable_{cfg}_{s}", image, mask, d, s % n)
                    if augment:
                        seen["cable"].add((bool(d[0, 1] < 0.5), bool(d[1, 1] < 0.5), bool(d[2, 1] < 0.5)))
                payload[f"cable_{cfg}_count"] = np.array(reps * n)
            # ---- the class maps
            ds = ref["train_3class"].CableTapeBurrDataset(idir, mdir, augment=False, target_size=(32, 32))
            ds3 = ref["train_3class_high_precision"].CableDefectDataset3Class(idir, mdir, augment=False, target_size=(32, 32))
            remap = ref["train_3class_high_precision"].remap_mask_to_3class
            for i in range(n):
                rec.take()
                image, mask = ds[i]
                store(payload, tb, f"burr3_{i}", image, mask, rec.take(), i)
                image, mask = ds3[i]
                store(payload, tb, f"hp3_{i}", image, mask, rec.take(), i)
                payload[f"remap_np_{i}"] = remap(masks[i])
                payload[f"remap_torch_{i}"] = remap(torch.from_numpy(masks[i].astype(np.int64))).numpy().astype(np.uint8)
                assert payload[f"remap_np_{i}"].dtype == np.uint8
            assert any((payload[f"remap_np_{i}"] != payload[f"remap_torch_{i}"]).any() for i in range(n)), "no byte above 6 in any mask"
            # ---- the advanced dataset's legacy path
            adv_mod = ref["data.advanced_dataset"]
            for name, cls in (("adv", adv_mod.CableDefectDatasetAdvanced), ("adv3", adv_mod.CableDefectDataset3Class)):
                ds = cls(idir, mdir, augment=True, target_size=(32, 32), tape_crop_prob=0.7)
                assert ds.transform is None and not ds.hard_negative_files
                np.random.seed(77 + len(name))
                payload[f"{name}_seed"] = np.array(77 + len(name))
                for s in range(3 * n):
                    rec.take()
                    image, mask = ds[s % n]
                    d = rec.take()
                    store(payload, tb, f"{name}_{s}", image, mask, d, s % n)
                    seen["adv_crop"].add(bool(d[0, 1] < 0.7) and bool((masks[s % n] == 2).any()))
                payload[f"{name}_count"] = np.array(3 * n)
            # ---- _tape_focused_crop alone, on an image of coordinates
            crop = adv_mod.CableDefectDatasetAdvanced._tape_focused_crop
            np.random.seed(5)
            t = 0
            for rep in range(12):
                for i in range(n):
                    h, w = masks[i].shape
                    coords = np.stack(np.mgrid[0:h, 0:w], -1).astype(np.int32)
                    rec.take()
                    ci, cm = crop(None, coords, masks[i])
                    d = rec.take()
                    y1, x1 = (int(v) for v in ci[0, 0])
                    rect = (x1, y1, x1 + ci.shape[1], y1 + ci.shape[0])
                    assert cm.shape == ci.shape[:2] and (cm == masks[i][rect[1]:rect[3], rect[0]:rect[2]]).all()
                    payload[f"tape_{t}_rect"], payload[f"tape_{t}_draws"], payload[f"tape_{t}_item"] = np.array(rect), d, np.array(i)
                    if len(d) == 0:
                        seen["tape_none"] = True
                        assert rect == (0, 0, w, h)
                    else:
                        seen["clip"] |= {k for k, hit in (("left", x1 == 0), ("top", y1 == 0), ("right", rect[2] == w), ("bottom", rect[3] == h)) if hit}
                        # crop_scale <= 1, so the adjusted rectangle always reaches crop_h x crop_w here; the smaller ones
                        # (a crop larger than the image) are covered by tests/test_train_batch_host.py's brute force
                        assert (rect[2] - rect[0], rect[3] - rect[1]) == (int(w * (0.6 + d[1, 1] * 0.4)), int(h * (0.6 + d[1, 1] * 0.4)))
                    t += 1
            payload["tape_count"] = np.array(t)
            # ---- PatchDefectDataset
            for cfg, ps, target, augment, reps in PATCH_CONFIGS:
                random.seed(300 + ps)
                ds = ref["data.patch_dataset"].PatchDefectDataset(idir, mdir, patch_size=ps, defect_ratio=0.5, augment=augment, target_size=target)
                stems = [p.stem for p in ds.images]
                payload[f"patch_{cfg}_types"] = np.array([kind == "defect" for kind, _ in ds.sample_indices])
                payload[f"patch_{cfg}_defect_items"] = np.array([stems.index(s["image"].stem) for s in ds.defect_samples])
                payload[f"patch_{cfg}_bboxes"] = np.array([s["bbox"] for s in ds.defect_samples], np.int64)
                payload[f"patch_{cfg}_normal_items"] = np.array([stems.index(p.stem) for p in ds.normal_samples])
                random.seed(400 + ps)
                payload[f"patch_{cfg}_seed"] = np.array(400 + ps)
                for s in range(reps * len(ds)):
                    rec.take()
                    image, mask = ds[s % len(ds)]
                    d = rec.take()
                    store(payload, tb, f"patch_{cfg}_{s}", image, mask, d, -1)
                    assert set(np.unique(mask.numpy())) <= {0, 1}
                    if augment:
                        a = d[3:]                                  # both kinds of _crop_patch make three draws
                        fh, fv, rot = a[0, 1] > 0.5, a[1, 1] > 0.5, a[2, 1] > 0.5
                        k = int(a[3, 1]) if rot else 0
                        csa = a[3 + rot, 1] > 0.5
                        seen["patch"].add(("flip", fh, fv)); seen["patch"].add(("rot", k)); seen["patch"].add(("csa", bool(csa)))
                    sizes = [m.shape for m in masks]
                    _, (x1, y1, x2, y2) = tb.patch_rect(tb.ReplayRng(d, "py"), ds.sample_indices[s % len(ds)][0], ps, sizes,
                                                        list(payload[f"patch_{cfg}_defect_items"]), payload[f"patch_{cfg}_bboxes"],
                                                        list(payload[f"patch_{cfg}_normal_items"]))
                    if (x2 - x1, y2 - y1) != (ps, ps):
                        seen["patch"].add("clipped")
                payload[f"patch_{cfg}_count"] = np.array(reps * len(ds))
    # every branch occurred
    assert len(seen["cable"]) == 8, sorted(seen["cable"])
    assert {("flip", a, b) for a in (False, True) for b in (False, True)} | {("rot", k) for k in range(4)} | {("csa", False), ("csa", True), "clipped"} <= seen["patch"]
    assert seen["clip"] >= {"left", "top", "right", "bottom"}, seen["clip"]
    assert seen["tape_none"] and seen["adv_crop"] == {False, True}
    # the round trip of the brightness step's two conversions with the identity table, over all 2^24 colours
    v = np.arange(256, dtype=np.uint8)
    worst = 0
    for r in range(256):
        rgb = np.stack(np.meshgrid(np.uint8(r), v, v, indexing="ij"), -1).reshape(-1, 3)
        worst = max(worst, int(np.abs(tb.hsv_value_scale_np(rgb, v).astype(np.int64) - rgb).max()))
    payload["hsv_round_trip_levels"] = np.array(worst)
    payload["torch_version"], payload["numpy_version"] = np.array(torch.__version__), np.array(np.__version__)
    np.savez_compressed(OUT, **payload)
    lines = [
        "train_batch_scenes.npz: what the reference's dataset classes return for four small items (37 x 53, 64 x 48 twice, 96 x 130),",
        "written by scripts/make_golden_train_batch.py: CableDefectDataset (src/data/dataset.py), CableTapeBurrDataset",
        "(tools/train_3class.py), remap_mask_to_3class and CableDefectDataset3Class (tools/train_3class_high_precision.py),",
        "CableDefectDatasetAdvanced and CableDefectDataset3Class (src/data/advanced_dataset.py, the legacy path with",
        "_tape_focused_crop in front), _tape_focused_crop alone and PatchDefectDataset (src/data/patch_dataset.py), all run unchanged",
        "under fixed seeds with every draw of np.random / random recorded.  The file holds the items, the draws and the results (the",
        "mask, the SHA-256 of the float32 image and, for two samples per run, its bytes times 255); none of the reference's program text.  Read by",
        "tests/test_train_batch_host.py and tests/test_gpu_train_batch.py.",
        "",
        "What rests on restatements.  cv2 is not installed where this project is built and tested, so the reference ran over the",
        "golden scripts' cv2 stub, in which these primitives are the project's NumPy restatements of OpenCV's published code:",
        "  cv2.resize INTER_LINEAR (uint8)   tiling.resize_linear_u8_np      11-bit fixed point",
        "  cv2.resize INTER_NEAREST          robust.resize_nearest_np",
        "  cv2.cvtColor RGB2HSV (uint8)      train_batch.rgb_to_hsv_u8_np    integer form, hue range 180, 12-bit division tables",
        "  cv2.cvtColor HSV2RGB (uint8)      train_batch.hsv_to_rgb_u8_np    float32 form, sector table, saturate_cast<uchar>(x * 255)",
        "  cv2.convertScaleAbs               train_batch.convert_scale_abs_lut   float32 |x alpha + beta|, round half to even, saturated",
        "  cv2.flip, cv2.cvtColor BGR2RGB, cv2.imdecode   index reversal; imdecode answers from an in-memory table",
        "cv2's own results for them stay unpinned, like every primitive of DESIGN.md 5.10-5.24.  What the fixture pins is the",
        "composition: the order of the stages, the draws, the integer lines of the crops, NumPy's and torch's own arithmetic (the",
        "float32 brightness product, / 255, the class maps).  convertScaleAbs reaches the device as a 256-byte table, so a caller who",
        "has cv2 passes cv2's own outputs.",
        "",
        "Two checks of the HSV restatement that need no cv2 run in tests/test_train_batch_host.py over all 2^24 colours: V == max(r, g,",
        "b) and a grey pixel comes back as (T[v], T[v], T[v]) for any table T; and with the identity table the round trip differs from",
        f"the input by at most {worst} levels per channel.  That bound is measured here, not chosen, and asserted as measured.",
        "",
        "Branches the generator asserts to occur: each flip of dataset.py alone, together and not at all, with the brightness step on",
        "and off; each flip of patch_dataset.py likewise, every k of rot90 and none, convertScaleAbs on and off, a patch clipped at",
        "the image's end (patch_size 33); a tape-focused crop clipped at each of the four borders, and a mask without tape.",
        f"torch {torch.__version__}, numpy {np.__version__}", ""]
    with open(README, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 512 * 1024


if __name__ == "__main__":
    main()
