#!/usr/bin/env python3
"""The tail of the refactored frame loop (infer_video_refactored.py:366-405) on the device: time per batch of every new call,
of the whole tail, of the same tail done on the host, and of segment().

Two workloads: B = 16 frames of 512 x 512 with a 320 x 448 ROI, and B = 4 frames of 1080 x 1920 with an 800 x 1000 ROI.  The
ROI masks are a cable and a tape of unet_amd.components.make_scene_mask with 0.05 % speckle (a few hundred small contours
beside the large one), 0 / 255; the frames are synthetic.smooth.  Device events around `--iters` calls after `--warmup`
calls, median of three loops.  Per workload:
  border_us, areas_us, circle_us, diameter_us      contours.outer_border, external_contour_areas(check=False),
                        enclosing_circle(check=False), measure_diameter (one read-back) on the full-frame cable mask
  paste_us, overlay_us  contours.paste_roi_masks of one mask, contours.create_overlay_masks
  tail_us               frame_loop._refactored_tail: two pastes, two circles, grey + burr mask, three counts, overlay, ONE
                        read-back and the float64 algebra on the host: lines :366-405 as process_frames_refactored_full runs them
  host_tail_us          the same lines the way the parent had to do them: .cpu() of the two ROI masks, then paste_roi_masks_np,
                        measure_diameter_np twice per frame, the coverages and create_overlay_masks_np on the host; the burr
                        mask stays on the device (burr_mask_rulebased on the uploaded cable mask, read back).  Host clock
                        around a synchronised call, `--host-iters` calls; checked against the device tail
  segment_us            segment() of B frames of 512 x 512 in `exact`: what the loop's model step costs at input_size = 512
  tail_over_segment, host_over_tail                 the ratios
Not measured here: hardware counters, per-kernel times (a run under rocprofv3 --kernel-trace --stats would give the latter).

    python scripts/contours_bench.py [--iters 20] [--warmup 3] [--host-iters 2] [--json OUT.json] [--inputs square]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_timing import timed, host_timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of square,hd (default: both)")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, components as cc, contours as ct, frame_loop, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup, "rows": []}
    print(result["version"])

    shapes = {"square": (16, 512, 512, (96, 32, 320, 448)), "hd": (4, 1080, 1920, (560, 40, 800, 1000))}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    model = NestedUNet(3, deep_supervision=False, max_batch=16, max_hw=(512, 512)).to("cuda:0")
    model.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    model.eval()
    k = 8192
    for name, (B, H, W, roi) in shapes.items():
        rw, rh = roi[2], roi[3]
        scene = np.stack([cc.make_scene_mask(rh, rw, s, noise=0.0005) for s in range(min(B, 4))] * (B // min(B, 4)))
        cable_np, tape_np = (scene == 1).astype(np.uint8) * 255, (scene == 2).astype(np.uint8) * 255
        frames_np = syn.make_frames_u8(B, H, W, "smooth", 7)
        cable_roi, tape_roi, x = torch.from_numpy(cable_np).cuda(), torch.from_numpy(tape_np).cuda(), torch.from_numpy(frames_np).cuda()
        row = {"input": name, "batch": B, "h": H, "w": W, "roi": list(roi)}
        t = lambda fn: timed(torch, fn, args.iters, args.warmup)
        full = ct.paste_roi_masks(model, cable_roi, roi, (H, W))
        tail = lambda: frame_loop._refactored_tail(model, x, cable_roi, tape_roi, roi, k, {})
        metrics, overlays, (cable, tape, burr) = tail()
        row["contours_per_frame"] = [int(v) - 1 for v in ct.external_contour_areas(model, full)[1].tolist()[:4]]
        row["dc_px"], row["dt_px"] = [m["dc_px"] for m in metrics[:4]], [m["dt_px"] for m in metrics[:4]]

        def host_tail():
            c, tp = cable_roi.cpu().numpy(), tape_roi.cpu().numpy()
            c_full, t_full = ct.paste_roi_masks_np(c, roi, (H, W)), ct.paste_roi_masks_np(tp, roi, (H, W))
            b_full = model.burr_mask_rulebased(model.bgr_to_gray(x), torch.from_numpy(c_full).cuda(), -1, max_components=k, check=False).cpu().numpy()
            out, over = [], np.empty_like(frames_np)
            for i in range(B):
                dc, dt = ct.measure_diameter_np(c_full[i]), ct.measure_diameter_np(t_full[i])
                out.append({"dc_px": dc, "dt_px": dt, "delta_d_px": dt - dc, "ratio": dt / dc if dc > 0 else None, "has_burr": bool(b_full[i].max() > 0),
                            "cable_coverage": np.sum(c_full[i] > 0) / (W * H), "tape_coverage": np.sum(t_full[i] > 0) / (W * H)})
                over[i] = ct.create_overlay_masks_np(frames_np[i], c_full[i], t_full[i], b_full[i])
            return out, over

        want, want_over = host_tail()
        assert want == metrics and (overlays.cpu().numpy() == want_over).all(), "device and host tails differ"
        row["border_us"] = t(lambda: ct.outer_border(model, full))
        row["areas_us"] = t(lambda: ct.external_contour_areas(model, full, check=False))
        row["circle_us"] = t(lambda: ct.enclosing_circle(model, full, check=False))
        row["diameter_us"] = t(lambda: ct.measure_diameter(model, full))
        row["paste_us"] = t(lambda: ct.paste_roi_masks(model, cable_roi, roi, (H, W)))
        row["overlay_us"] = t(lambda: ct.create_overlay_masks(model, x, cable, tape, burr))
        row["burr_us"] = t(lambda: model.burr_mask_rulebased(model.bgr_to_gray(x), cable, -1, max_components=k, check=False))
        row["tail_us"] = t(tail)
        row["host_tail_us"] = host_timed(torch, host_tail, args.host_iters)
        xs = torch.from_numpy(syn.make_frames_u8(B, 512, 512, "smooth", 7)).cuda()
        row["segment_us"] = t(lambda: model.segment(xs))
        row["tail_over_segment"] = round(row["tail_us"] / row["segment_us"], 3)
        row["host_over_tail"] = round(row["host_tail_us"] / row["tail_us"], 1)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "tail_us", "rows": [(r["input"], r["tail_us"], r["host_tail_us"], r["segment_us"]) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
