#!/usr/bin/env python3
"""Stage-2 burr detection on the device: time per call against the network and the host path it replaces.

B = 16 scenes at 512 x 512 and B = 32 at 448 x 800 from unet_amd.edges.make_burr_scene (four distinct scenes per
workload, repeated to the batch), through `canny` (blur fused), `detect_burrs` and `burr_mask_rulebased`: device events
around `--iters` calls after `--warmup` calls, median of three loops.  In the same run: `segment()` of a batch of the
same size in `exact` (the bar of DESIGN.md §5.8: detect_burrs must stay below it, so that the frame rate stays the
network's) and the host path detect_burrs replaces (pinned D2H of the grey frames and the cable masks, then
unet_amd.edges.detect_burrs_np on one thread, timed on `--host-frames` frames and reported per frame).

    python scripts/burr_bench.py [--iters 20] [--warmup 5] [--json OUT.json] [--only-burr] [--inputs square]

Per-launch times come from a run of its own under `rocprofv3 --kernel-trace --stats` with --only-burr (no counters in
that run); edge_map_kernel moves 2 bytes per pixel (grey in, map out), cc_apply_kernel 5 (labels in, mask out).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_timing import timed  # noqa: E402


def host_path(torch, ed, dg, dc, frames):
    """What a frame loop does today: grey frames and cable masks cross PCIe, one host thread runs the detection."""
    pg, pc = torch.empty(dg.shape, dtype=torch.uint8).pin_memory(), torch.empty(dc.shape, dtype=torch.uint8).pin_memory()
    t0 = time.perf_counter()
    pg.copy_(dg, non_blocking=True)
    pc.copy_(dc, non_blocking=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i in range(frames):
        ed.detect_burrs_np(pg[i].numpy(), pc[i].numpy())
    t2 = time.perf_counter()
    return {"d2h_us": round((t1 - t0) * 1e6), "detect_np_us_per_frame": round((t2 - t1) * 1e6 / frames), "frames_timed": frames}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of square,wide (default: both)")
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--only-burr", action="store_true", help="no segment(), no host path: the run to put under rocprofv3")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, edges as ed, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters,
              "warmup": args.warmup, "rows": []}
    print(result["version"])
    model = NestedUNet(3, deep_supervision=True, max_batch=16, max_hw=(512, 512)).to("cuda:0")
    model.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    model.eval()

    shapes = {"square": (16, 512, 512), "wide": (32, 448, 800)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W) in shapes.items():
        scenes = [ed.make_burr_scene(H, W, seed) for seed in range(4)]
        grey = np.stack([scenes[i % 4][0] for i in range(B)])
        cable = np.stack([scenes[i % 4][1] for i in range(B)])
        dg, dc = torch.from_numpy(grey).cuda(), torch.from_numpy(cable).cuda()
        row = {"input": name, "batch": B, "h": H, "w": W}
        if not args.only_burr:
            frames = np.stack([syn.make_frame_u8(H, W, i, ("smooth", "uniform")[i % 2], 1234) for i in range(B)])
            x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
            row["segment_us"] = timed(torch, lambda: model.segment(x), args.iters, args.warmup)
            del x
        row["gaussian_blur_us"] = timed(torch, lambda: model.gaussian_blur(dg), args.iters, args.warmup)
        row["canny_us"] = timed(torch, lambda: model.canny(dg, 50, 150, blur=(5, 1.0)), args.iters, args.warmup)
        row["detect_burrs_us"] = timed(torch, lambda: model.detect_burrs(dg, dc, check=False), args.iters, args.warmup)
        row["burr_mask_rulebased_us"] = timed(torch, lambda: model.burr_mask_rulebased(dg, dc, check=False), args.iters, args.warmup)
        row["burr_pixels"] = int(model.detect_burrs(dg, dc).count_nonzero())
        row["edge_pixels"] = int(model.canny(dg, 50, 150, blur=(5, 1.0)).count_nonzero())
        if not args.only_burr:
            row["host"] = host_path(torch, ed, dg, dc, min(args.host_frames, B))
            row["detect_over_segment"] = round(row["detect_burrs_us"] / row["segment_us"], 3)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "detect_burrs_us", "rows": [(r["input"], r["detect_burrs_us"], r.get("segment_us")) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
