#!/usr/bin/env python3
"""The 6- and 7-class video loops on the device: time per batch of each kernel, of the compositions and of the whole loop, against
the route the parent commit offers for the class clean-up and against the network.

Workloads: B = 32 of 448 x 800 and B = 4 of 1080 x 1920 (the network runs at 448 x 800 and at 1088 x 1920: rows rounded up to a
multiple of 16).  Class maps are unet_amd.multiclass.make_class_scene scenes (a 96 x 128 scene tiled to the frame), frames are
seeded noise, probability planes are make_prob_planes at a quarter of the frame size.  Device events around `--iters` calls
after `--warmup` calls (default 20), median of three loops.  Per workload:
  gate_us                  multiclass.quality_gate (memset, the sums kernel, the finishing kernel); gate_gbs = the bytes it must
                           move, 3 in + 1 out per pixel (+ 1 for frame 0's previous grey frame), per second.  The kernel reads
                           the previous frame's BGR pixel again for frames 1..B-1, which the figure does not count.
  overlay_region_us / overlay_weighted_us   multiclass.overlay; overlay_gbs = 4 in + 3 out per pixel, per second
  threshold_us             multiclass.threshold_classes, planes at a quarter size resized to the frame in the kernel
  merge_video_us           multiclass.clean_classes_video: ONE launch (plus the table's initialisation), mask and class table
  merge_v3_us              multiclass.merge_classes with the v3 programs on the bit map
  class_table_us           multiclass.class_table
  predict_v3_us            multiclass.predict_v3: threshold_classes + merge_classes
  route_video_us           what a user of the parent commit has for clean_classes_video's mask and counts: model.morphology per
                           closed plane, torch indexing for the merge, model.mask_stats for the counts.  These are the parent's
                           code paths, unchanged by this feature; boxes would cost the route another reduction, not timed.
  loop_video_us / loop_v3_us   frame_loop.process_frames_multiclass with its two read-backs (host time included: wall clock)
  segment_us               segment() of the same batch in `exact`
Ratios: route_over_merge = route_video_us / merge_video_us, and each step over segment_us.  Before timing, every device result is
compared with the NumPy form on the first frame.  Not measured: hardware counters, and the misaligned (byte) paths.

    python scripts/multiclass_bench.py [--iters 20] [--warmup 20] [--json OUT.json] [--inputs video,full_hd] [--no-segment]
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

COLORS = {1: (255, 0, 0), 2: (0, 255, 0), 3: (0, 0, 255), 4: (255, 255, 0), 5: (255, 0, 255), 6: (0, 165, 255)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of video,full_hd (default: both)")
    ap.add_argument("--no-segment", action="store_true", help="no segment() and no loop: the post-processing rows alone")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, frame_loop, multiclass as mc, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup, "rows": []}
    print(result["version"])

    shapes = {"video": (32, 448, 800), "full_hd": (4, 1080, 1920)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W) in shapes.items():
        Hs = (H + 15) // 16 * 16
        model = NestedUNet(7, deep_supervision=False, max_batch=B, max_hw=(Hs, W)).to("cuda:0")
        model.load_state_dict(syn.make_state_dict(7, 3, False, 2), strict=True)
        model.eval()
        scenes = [np.tile(mc.make_class_scene(96, 128, s)[0], ((H + 95) // 96, (W + 127) // 128))[:H, :W] for s in range(4)]
        pred_np = np.stack([scenes[i % 4] for i in range(B)])
        frames_np = np.random.default_rng(1).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        planes_np = mc.make_prob_planes(B, H // 4, W // 4, 3)
        pred, frames, planes = (torch.from_numpy(a).cuda() for a in (pred_np, frames_np, planes_np))
        ch = dict(channels=(0, 1, 2, 3, 4))
        row = {"input": name, "batch": B, "h": H, "w": W, "merge_layout_video": mc.merge_layout((B, H, W), mc.PLANES_VIDEO),
               "merge_layout_v3": mc.merge_layout((B, H, W), mc.PLANES_V3, mc.LUT_BITS)}
        t = lambda fn: timed(torch, fn, args.iters, args.warmup)

        # the same results as the NumPy forms, on the first frame
        got = [x.cpu().numpy() for x in mc.quality_gate(model, frames[:2])]
        want = mc.quality_gate_np(frames_np[:2])
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), "gate: device and host differ"
        m, tab = mc.clean_classes_video(model, pred[:1], num_classes=7)
        wm, wt = mc.clean_classes_video_np(pred_np[:1], num_classes=7)
        assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(tab.cpu().numpy(), wt), "merge: device and host differ"
        m3, t3 = mc.predict_v3(model, planes[:1], (H, W), num_classes=7, **ch)
        w3, wt3 = mc.predict_v3_np(planes_np[:1], (H, W), num_classes=7, **ch)
        assert np.array_equal(m3.cpu().numpy(), w3) and np.array_equal(t3.cpu().numpy(), wt3), "predict_v3: device and host differ"
        for mode in ("region", "weighted"):
            assert np.array_equal(mc.overlay(model, frames[:1], m, COLORS, 0.6, mode).cpu().numpy(), mc.overlay_np(frames_np[:1], wm, COLORS, 0.6, mode))

        def route():
            cable = model.morphology(pred, 1, "close", 3)
            tape = model.morphology(pred, 2, "close", 3)
            out = torch.zeros_like(pred)
            out[cable > 0] = 1
            out[tape > 0] = 2
            d = (pred == 3) | (pred == 5) | (pred == 6)
            out[d] = pred[d]
            return out, model.mask_stats(out)[0]

        r_out, r_counts = route()
        full, full_t = mc.clean_classes_video(model, pred, num_classes=7)
        assert torch.equal(r_out, full) and torch.equal(r_counts, full_t[:, :, 0].long()), "the parent's route and the merge kernel differ"

        px = B * H * W
        row["gate_us"] = t(lambda: mc.quality_gate(model, frames))
        row["gate_gbs"] = round((4 * px + H * W) / row["gate_us"] / 1e3, 1)
        for mode in ("region", "weighted"):
            row[f"overlay_{mode}_us"] = t(lambda: mc.overlay(model, frames, full, COLORS, 0.6, mode))
            row[f"overlay_{mode}_gbs"] = round(7 * px / row[f"overlay_{mode}_us"] / 1e3, 1)
        row["threshold_us"] = t(lambda: mc.threshold_classes(model, planes, (H, W), **ch))
        bits = mc.threshold_classes(model, planes, (H, W), **ch)
        row["merge_video_us"] = t(lambda: mc.clean_classes_video(model, pred, num_classes=7))
        row["merge_v3_us"] = t(lambda: mc.merge_classes(model, bits, mc.PLANES_V3, lut=mc.LUT_BITS, num_classes=7))
        row["class_table_us"] = t(lambda: mc.class_table(model, pred, 7))
        row["predict_v3_us"] = t(lambda: mc.predict_v3(model, planes, (H, W), num_classes=7, **ch))
        row["route_video_us"] = t(route)
        row["route_over_merge"] = round(row["route_video_us"] / row["merge_video_us"], 2)
        if not args.no_segment:
            x = torch.from_numpy(syn.make_frames_u8(B, Hs, W, "smooth", 7)).cuda()
            row["segment_h"] = Hs
            row["segment_us"] = t(lambda: model.segment(x))
            loop_iters, loop_warm = max(args.iters // 4, 2), 2
            for variant in ("video", "v3"):
                row[f"loop_{variant}_us"] = wall(torch, lambda: frame_loop.process_frames_multiclass(
                    model, frames, None, input_size=(Hs, W), variant=variant, colors=COLORS, gate=dict(enable=False)), loop_iters, loop_warm)
            for k in ("gate_us", "overlay_region_us", "overlay_weighted_us", "threshold_us", "merge_video_us", "merge_v3_us", "class_table_us",
                      "predict_v3_us", "route_video_us", "loop_video_us", "loop_v3_us"):
                row[k.replace("_us", "_over_segment")] = round(row[k] / row["segment_us"], 4)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        del model

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "route_over_merge", "rows": [(r["input"], r["merge_video_us"], r["route_video_us"], r["route_over_merge"])
                                                            for r in result["rows"]]}))


if __name__ == "__main__":
    main()
