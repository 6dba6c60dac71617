#!/usr/bin/env python3
"""The ROI and full-frame 3-class loops on the device: time per batch of each new call and of both loops, against the route the
parent commit offers and against the network.

Workloads: B = 16 frames of 512 x 512 and B = 4 frames of 1080 x 1920; the network and every probability / mask step run at
512 x 512.  Frames are roi_loop.make_projection_frame scenes tiled to the frame, probabilities roi_loop.make_probs.  Device
events around `--iters` calls after `--warmup` calls, median of three loops; the loops and the two routes with a read-back are
wall clock.  Per workload:
  roi_from_edges_us        memset + the column count + the decision, on Canny's output
  detect_roi_us            grey conversion + Canny + roi_from_edges
  crop_resize_us           one launch for the batch, the width read on the device (wall clock as well: crop_resize_wall_us)
  adaptive_thresholds_us   memset + the sums kernel + the table; thresholds_gbs against its 12 bytes per pixel (three planes read)
  ultra_strict_us          one launch; ultra_strict_gbs against its 14 bytes per pixel (three planes read, two masks written)
  refine_by_geometry_us / select_primary_us   labelling + the rule + the mask
  paste_masks_us           one launch for a mask pair
  loop_roi_us / loop_full_us   frame_loop.process_frames_roi / process_frames_3class_full, host time included
  segment_us               segment() of the same batch at 512 x 512 in `exact`
  route_probs_us           what the parent offers for steps 3-4: torch reductions (mean and max of three planes), torch.where
                           for the table, torch comparisons for the two masks.  No read-back, about twenty launches.
  route_crop_wall_us       what the parent offers for steps 1-2 once the ROI is known: a read-back of the table and one
                           resize_frames call per frame on a contiguous copy of its columns (host tables are keyed by extent)
Ratios: route_probs_over_kernels = route_probs_us / (adaptive_thresholds_us + ultra_strict_us), route_crop_over_crop =
route_crop_wall_us / crop_resize_wall_us, and each step over segment_us.  Before timing, every device result is compared with
the NumPy form on a 64 x 96 batch and the route's masks with ultra_strict's.  Not measured: hardware counters, the time of each
kernel inside a call, and the misaligned (byte) paths.

    python scripts/roi_bench.py [--iters 10] [--warmup 5] [--out FILE] [--inputs square,full_hd]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_timing import timed, wall  # noqa: E402
S = 512


def check_small(torch, model, rl):
    """Every new call against its NumPy form on a 2 x 64 x 96 batch."""
    frames = np.stack([rl.make_projection_frame(64, 96, s) for s in (0, 1)])
    dev = torch.from_numpy(frames).cuda()
    roi = rl.detect_roi(model, dev)
    want = np.stack([rl.detect_roi_np(f) for f in frames])
    assert np.array_equal(roi.cpu().numpy(), want), "detect_roi: device and host differ"
    assert np.array_equal(rl.crop_resize(model, dev, roi, 48).cpu().numpy(), np.stack([rl.crop_resize_np(f, q, 48) for f, q in zip(frames, want)]))
    probs = np.stack([rl.make_probs(64, 96, s, c) for s, c in ((0, 0.02), (1, 0.4))])
    p = torch.from_numpy(probs).cuda()
    thr = rl.adaptive_thresholds(model, p)[0]
    assert thr.cpu().numpy().tobytes() == np.stack([rl.adaptive_thresholds_np(x)[0] for x in probs]).tobytes()
    c, t = rl.ultra_strict(model, p, thr)
    for i in range(2):
        wc, wt = rl.ultra_strict_np(probs[i], thr[i].cpu().numpy())
        assert np.array_equal(c[i].cpu().numpy(), wc) and np.array_equal(t[i].cpu().numpy(), wt), "ultra_strict: device and host differ"
    g = rl.refine_by_geometry(model, c, min_area=20, wide_width=10, large_area=150)
    assert np.array_equal(g[0].cpu().numpy(), rl.refine_by_geometry_np(c[0].cpu().numpy(), min_area=20, wide_width=10, large_area=150))
    pc, pt = rl.paste_masks(model, (c, t), roi, (64, 96))
    assert np.array_equal(pc[1].cpu().numpy(), rl.paste_mask_np(c[1].cpu().numpy(), want[1], (64, 96)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="default: profiles/roi_<source hash>_bench.txt")
    ap.add_argument("--inputs", default="", help="comma list out of square,full_hd (default: both)")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, frame_loop, roi_loop as rl, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    out_path = args.out or os.path.join(ROOT, "profiles", f"roi_{_lib.source_hash()}_bench.txt")
    lines = [json.dumps({"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup})]
    print(lines[0])

    shapes = {"square": (16, 512, 512), "full_hd": (4, 1080, 1920)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W) in shapes.items():
        model = NestedUNet(3, deep_supervision=False, max_batch=B, max_hw=(S, S)).to("cuda:0")
        model.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
        model.eval()
        check_small(torch, model, rl)
        scenes = [np.tile(rl.make_projection_frame(64, 128, s), ((H + 63) // 64, 1, 1))[:H] for s in range(4)]
        # the reference scales a column as int(col * (W / 512)) although it projects at frame width: on a frame wider than 512 only a
        # cable within the left 512 columns has a range that is not empty, so the bar stands at column 200 there
        left = (W - 128) // 2 if W <= 512 else 200
        scenes = [np.concatenate([np.full((H, left, 3), 90, np.uint8), sc, np.full((H, W - 128 - left, 3), 90, np.uint8)], axis=1) for sc in scenes]
        frames = torch.from_numpy(np.stack([scenes[i % 4] for i in range(B)])).cuda()
        probs_np = np.stack([rl.make_probs(S, S, i, (0.02, 0.4)[i % 2], (0.01, 0.2)[(i // 2) % 2]) for i in range(B)])
        probs = torch.from_numpy(probs_np).cuda()
        t = lambda fn: timed(torch, fn, args.iters, args.warmup)
        row = {"input": name, "batch": B, "h": H, "w": W, "model_size": S}

        edges = model.canny(model.bgr_to_gray(frames), 50, 150)
        roi = rl.detect_roi(model, frames)
        row["roi"] = roi.cpu().numpy()[:, :2].tolist()[:4]
        assert bool(roi[:, 3].all()), f"a frame's range is empty: {roi.cpu().tolist()}"
        thr = rl.adaptive_thresholds(model, probs)[0]
        cable_s, tape_s = rl.ultra_strict(model, probs, thr)

        def route_probs():
            p = probs[:, :3]
            means = p.mean(dim=(2, 3))
            maxima = p.amax(dim=(2, 3))
            t_cable = torch.where(means[:, 1] > 0.3, torch.clamp(means[:, 1] + 0.4, max=0.85), torch.full_like(means[:, 1], 0.5))
            t_tape = torch.where(means[:, 2] > 0.15, torch.clamp(means[:, 2] + 0.5, max=0.85), torch.full_like(means[:, 2], 0.55))
            margin = torch.clamp(1.0 - means[:, 0], min=0.2)
            bg, c, tp = p[:, 0], p[:, 1], p[:, 2]
            winner = p.argmax(dim=1)
            floor_ = bg + margin[:, None, None]
            mc = (winner == 1) & (c >= t_cable[:, None, None]) & (c > bg * 2) & (c >= floor_)
            mt = (winner == 2) & (tp >= t_tape[:, None, None]) & (tp > bg * 2) & (tp >= floor_)
            return mc.to(torch.uint8), mt.to(torch.uint8), maxima

        rc, rt, _ = route_probs()
        row["route_masks_differ_px"] = int((rc != cable_s).sum() + (rt != tape_s).sum())      # torch's float32 mean is not the 64-bit sum

        def route_crop():
            table = roi.cpu().tolist()                                   # the read-back
            return [model.resize_frames(frames[i:i + 1, :, q[0]:q[1]].contiguous(), (S, S)) for i, q in enumerate(table) if q[3]]

        got = rl.crop_resize(model, frames, roi, S)
        for i, crop in enumerate(route_crop()):
            assert torch.equal(crop[0], got[i]), "the parent's route and crop_resize differ"

        px = B * S * S
        row["roi_from_edges_us"] = t(lambda: rl.roi_from_edges(model, edges))
        row["detect_roi_us"] = t(lambda: rl.detect_roi(model, frames))
        row["crop_resize_us"] = t(lambda: rl.crop_resize(model, frames, roi, S))
        row["adaptive_thresholds_us"] = t(lambda: rl.adaptive_thresholds(model, probs))
        row["thresholds_gbs"] = round(12 * px / row["adaptive_thresholds_us"] / 1e3, 1)
        row["ultra_strict_us"] = t(lambda: rl.ultra_strict(model, probs, thr))
        row["ultra_strict_gbs"] = round(14 * px / row["ultra_strict_us"] / 1e3, 1)
        row["refine_by_geometry_us"] = t(lambda: rl.refine_by_geometry(model, cable_s, check=False))
        row["select_primary_us"] = t(lambda: rl.select_primary(model, cable_s, check=False))
        row["paste_masks_us"] = t(lambda: rl.paste_masks(model, (cable_s, tape_s), roi, (H, W)))
        row["route_probs_us"] = t(route_probs)
        row["route_probs_over_kernels"] = round(row["route_probs_us"] / (row["adaptive_thresholds_us"] + row["ultra_strict_us"]), 2)
        loop_iters, loop_warm = max(args.iters // 2, 2), 2
        row["crop_resize_wall_us"] = wall(torch, lambda: rl.crop_resize(model, frames, roi, S), loop_iters, loop_warm)
        row["route_crop_wall_us"] = wall(torch, route_crop, loop_iters, loop_warm)
        row["route_crop_over_crop"] = round(row["route_crop_wall_us"] / row["crop_resize_wall_us"], 2)
        x = torch.from_numpy(syn.make_frames_u8(B, S, S, "smooth", 7)).cuda()
        row["segment_us"] = t(lambda: model.segment(x))
        row["loop_roi_us"] = wall(torch, lambda: frame_loop.process_frames_roi(model, frames, input_size=S), loop_iters, loop_warm)
        row["loop_full_us"] = wall(torch, lambda: frame_loop.process_frames_3class_full(model, frames, input_size=S), loop_iters, loop_warm)
        for k in ("roi_from_edges_us", "detect_roi_us", "crop_resize_us", "adaptive_thresholds_us", "ultra_strict_us", "refine_by_geometry_us",
                  "select_primary_us", "paste_masks_us", "route_probs_us", "loop_roi_us", "loop_full_us"):
            row[k.replace("_us", "_over_segment")] = round(row[k] / row["segment_us"], 4)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del model

    lines.append("not measured: hardware counters, per-kernel times inside a call, the misaligned (byte) paths")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
