#!/usr/bin/env python
"""Generate tests/golden/contours_scenes.npz from the REFERENCE's own functions: measure_diameter and the blend lines of
create_overlay (infer_video_refactored.py:148-172, :191-201) and paste_roi_mask (src/refactor/preprocess.py:116-144), run
unchanged over the project's cv2 stub.

Runs where the reference source is checked out (like scripts/make_golden_burr.py), never on the GPU box; only the small .npz
(data: masks, frames, areas, diameters, pasted masks, one overlay) is committed.  cv2 is make_golden_burr's stub, extended
HERE with
  findContours / contourArea   on unet_amd.contours' restatement of the border following (so the fixtures pin the
                               composition: which contour measure_diameter picks, what it returns for empty masks)
  minEnclosingCircle           an independent brute force in float64: the smallest circle through 2 or 3 of the points that
                               holds them all (a tolerance of 1e-9 relative on the radius decides "holds")
  putText                      draws nothing: the fixtures pin lines :191-201 only, text pixels cannot be pinned without cv2
No scene may have two external contours of equal largest area (cv2's contour order is not pinned); asserted below.

    python scripts/make_golden_contours.py
"""
from __future__ import annotations

import importlib
import itertools
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_golden  # noqa: E402  (reference import helpers)
import make_golden_burr  # noqa: E402  (the cv2 stub with the grey-level calls)

OUT = os.path.join(ROOT, "tests", "golden", "contours_scenes.npz")


def brute_force_circle(points):
    """((cx, cy), radius): the smallest of the circles through every pair (as a diameter) and every triple (circumcircle) of
    the points that holds all of them, everything in float64."""
    p = np.unique(np.asarray(points, np.float64).reshape(-1, 2), axis=0)
    if len(p) == 1:
        return (float(p[0, 0]), float(p[0, 1])), 0.0
    cands = []
    i, j = np.triu_indices(len(p), 1)
    c2 = (p[i] + p[j]) / 2
    cands.append((c2, np.hypot(*(p[i] - p[j]).T) / 2))
    if len(p) >= 3:
        t = np.array(list(itertools.combinations(range(len(p)), 3)))
        a, b, c = p[t[:, 0]], p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
        d = 2 * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
        ok = d != 0
        a, b, c, d = a[ok], b[ok], c[ok], d[ok]
        b2, cc = (b ** 2).sum(1), (c ** 2).sum(1)
        u = np.stack(((c[:, 1] * b2 - b[:, 1] * cc) / d, (b[:, 0] * cc - c[:, 0] * b2) / d), 1)
        cands.append((a + u, np.hypot(u[:, 0], u[:, 1])))
    centre = np.concatenate([c for c, _ in cands])
    radius = np.concatenate([r for _, r in cands])
    best = None
    for lo in range(0, len(radius), 4096):                       # chunks: candidates x points
        cen, rad = centre[lo:lo + 4096], radius[lo:lo + 4096]
        dist = np.hypot(cen[:, None, 0] - p[None, :, 0], cen[:, None, 1] - p[None, :, 1])
        holds = (dist <= rad[:, None] * (1 + 1e-9)).all(1)
        if holds.any():
            k = np.flatnonzero(holds)[np.argmin(rad[holds])]
            if best is None or rad[k] < best[1]:
                best = ((float(cen[k, 0]), float(cen[k, 1])), float(rad[k]))
    return best


def cv2_stub(mo, ed, ct):
    cv2 = make_golden_burr.cv2_stub(mo, ed)
    cv2.FONT_HERSHEY_SIMPLEX = 0
    cv2.contour_calls = []

    def findContours(image, mode, method):
        assert mode == cv2.RETR_EXTERNAL and method == cv2.CHAIN_APPROX_SIMPLE and image.dtype == np.uint8
        contours = ct.find_external_contours_np(image)
        cv2.contour_calls.append(contours)
        return contours, None

    cv2.findContours, cv2.contourArea = findContours, ct.contour_area_np
    cv2.minEnclosingCircle = brute_force_circle
    cv2.putText = lambda img, *a, **k: img
    cv2.cvtColor = lambda img, code: ed.bgr_to_gray_np(img)
    return cv2


def import_reference(mo, ed, ct):
    sys.modules["cv2"] = cv2_stub(mo, ed, ct)
    for name in ("torchvision", "torchvision.models", "tqdm", "src.models", "src.models.unetpp"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["tqdm"].tqdm = getattr(sys.modules["tqdm"], "tqdm", None)
    sys.modules["src.models.unetpp"].NestedUNet = None         # the reference's model is never run here
    if make_golden.REF not in sys.path:
        sys.path.insert(0, make_golden.REF)
    loop = importlib.import_module("infer_video_refactored")
    refactor = importlib.import_module("src.refactor")
    return loop, refactor


def scenes(cc):
    y, x = np.mgrid[0:64, 0:96]
    z = lambda h, w: np.zeros((h, w), np.uint8)
    out = {}
    m = z(24, 40); m[11, 17] = 255
    out["single_pixel"] = m
    m = z(24, 40); m[5, 6] = m[6, 7] = 255
    out["diagonal_pair"] = m
    m = z(24, 40); m[3:20, 9] = 255; m[19, 9:31] = 255
    out["line"] = m
    out["disc"] = (((x - 47) ** 2 + (y - 30) ** 2) <= 23 ** 2).astype(np.uint8) * 255
    d2 = (x - 40) ** 2 + (y - 32) ** 2
    ring = ((d2 <= 26 ** 2) & (d2 >= 17 ** 2)) | (d2 <= 5 ** 2)                  # the blob in the hole must yield no contour
    ring[2:6, 80:90] = True                                                      # and a smaller second contour outside
    out["ring_with_blob"] = ring.astype(np.uint8) * 255
    m = z(32, 48); m[4:12, 5:15] = 255; m[12:27, 15:40] = 255                    # two blobs that touch only diagonally: one contour
    out["diagonal_touch"] = m
    m = z(32, 48); m[:, 20:23] = 255; m[14:17, :] = 255; m[5:9, 30:40] = 255
    out["all_edges"] = m
    out["zeros"] = z(24, 40)
    out["ones"] = np.full((24, 40), 255, np.uint8)
    scene = cc.make_scene_mask(64, 96, 3)
    out["network_cable"] = (scene == 1).astype(np.uint8) * 255
    out["network_tape"] = (scene == 2).astype(np.uint8) * 255
    return out


def main():
    make_golden._load_synthetic()                         # puts the repository root on sys.path
    from unet_amd import components as cc
    from unet_amd import contours as ct
    from unet_amd import edges as ed
    from unet_amd import morphology as mo
    loop, refactor = import_reference(mo, ed, ct)
    cv2 = sys.modules["cv2"]
    payload, names = {}, []
    for name, mask in scenes(cc).items():
        del cv2.contour_calls[:]
        diameter = loop.measure_diameter(mask)
        contours = cv2.contour_calls[0] if cv2.contour_calls else []
        areas = np.array([cv2.contourArea(c) for c in contours], np.float64)
        assert areas.size < 2 or np.sort(areas)[-1] > np.sort(areas)[-2], f"{name}: two external contours of equal largest area"
        assert mask.shape[0] in range(24, 65) and mask.shape[1] in range(40, 97)
        payload[name + "/mask"], payload[name + "/areas"], payload[name + "/diameter"] = mask, areas, np.float64(diameter)
        names.append(name)
        print(f"{name:16s} {mask.shape} contours {len(contours):3d} largest area {areas.max() if areas.size else 0:8.1f} diameter {diameter!r}")
    assert len(cv2.contour_calls) == 1 and payload["ring_with_blob/areas"].size == 2
    payload["names"] = np.array(names)

    r = np.random.default_rng(11)
    for tag, (fh, fw), roi in (("paste_inside", (48, 80), (9, 5, 40, 30)), ("paste_overhang", (48, 80), (60, 30, 40, 30))):
        cfg = refactor.ROIConfig(x=roi[0], y=roi[1], w=roi[2], h=roi[3])
        frame = r.integers(0, 256, (fh, fw), dtype=np.uint8)
        crop = refactor.crop_roi(frame, cfg)                                     # the ROI mask has the crop's size, as in the loop
        roi_mask = ((r.random(crop.shape) < 0.4) * 255).astype(np.uint8)
        full = refactor.paste_roi_mask(np.zeros((fh, fw), np.uint8), roi_mask, cfg)
        payload[tag + "/roi_mask"], payload[tag + "/roi"], payload[tag + "/frame_hw"], payload[tag + "/full"] = roi_mask, np.array(roi), np.array((fh, fw)), full
        print(f"{tag}: roi {roi} crop {crop.shape} pasted {int((full > 0).sum())} of {int((roi_mask > 0).sum())} pixels")

    fh, fw = 40, 72
    frame = r.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    masks = [np.zeros((fh, fw), np.uint8) for _ in range(3)]
    masks[0][5:30, 10:40] = 255; masks[1][20:38, 30:60] = 255; masks[2][25:33, 35:45] = 255        # all three overlap in one block
    metrics = refactor.FrameMetrics(frame_id=0, dc_px=0.0, dt_px=0.0, delta_d_px=0.0, ratio=None, has_burr=True, cable_coverage=0.0, tape_coverage=0.0)
    out = loop.create_overlay(frame, masks[0], masks[1], masks[2], metrics, ["event"])
    assert out.dtype == np.uint8 and (out != frame).any()
    payload.update({"overlay/frame": frame, "overlay/cable": masks[0], "overlay/tape": masks[1], "overlay/burr": masks[2], "overlay/out": out})

    np.savez_compressed(OUT, **payload)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    with open(os.path.join(ROOT, "tests", "golden", "README_contours.txt"), "w") as f:
        f.write("contours_scenes.npz: results of the reference's measure_diameter, paste_roi_mask and the blend lines of create_overlay\n"
                "(infer_video_refactored.py, src/refactor/preprocess.py) on small synthetic masks and frames, written by\n"
                "scripts/make_golden_contours.py.  Per scene: mask, the contourArea of every external contour in scan order, the\n"
                "diameter.  cv2 is a stub: findContours / contourArea on unet_amd.contours' restatement, minEnclosingCircle an\n"
                f"independent float64 brute force over all pairs and triples, putText drawing nothing.  numpy {np.__version__}.\n")


if __name__ == "__main__":
    main()
