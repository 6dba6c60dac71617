#!/usr/bin/env python3
"""Sliding-window inference on the device: time per call of predict_tiled and of its parts against the network.

1080 x 1920 frames, B = 1 and B = 4, the reference's defaults patch_size 384 / stride 192 / target_size 256 (45 patches
per frame), a 2-class NestedUNet in `exact` with max_batch 16.  Device events around `--iters` calls after `--warmup`
calls, median of three loops, all in one run:
  predict_tiled   the whole call, blend="probs" with a gate (every step runs)
  forward         predict_proba of the same patch batch in the same chunks: the bar (the steps below together must stay
                  under it, so that the frame rate stays the network's)
  gather, gate, blend   the three new launches alone
The blend's achieved bytes per second are its minimum traffic over its time: every map read once, mask and output
written once (the taps shared between neighbouring pixels and overlapping patches are served by the caches).

    python scripts/tiled_bench.py [--iters 20] [--warmup 5] [--json OUT.json] [--txt OUT.txt] [--batches 1,4]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_timing import timed  # noqa: E402

H, W, PATCH, STRIDE, TARGET, CLASSES, GATE_THR = 1080, 1920, 384, 192, 256, 2, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--txt", default="")
    ap.add_argument("--batches", default="1,4")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, synthetic as syn, tiling as tl
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
              "workload": {"h": H, "w": W, "patch_size": PATCH, "stride": STRIDE, "target_size": TARGET, "classes": CLASSES}, "rows": []}
    lines = [result["version"]]
    print(lines[0])
    model = NestedUNet(CLASSES, deep_supervision=False, max_batch=16, max_hw=(TARGET, TARGET)).to("cuda:0")
    model.load_state_dict(syn.make_trained_like_state_dict(CLASSES, 3, False, 0), strict=True)
    model.eval()
    plan = tl.tile_plan(H, W, PATCH, STRIDE)

    for B in [int(b) for b in args.batches.split(",")]:
        frames = torch.from_numpy(np.stack([syn.make_frame_u8(H, W, i, "smooth", 1234) for i in range(B)])).cuda()
        n = B * plan.n_patches
        row = {"batch": B, "patches": n}
        patches = model.gather_tiles(frames, PATCH, STRIDE, TARGET, "bgr")

        def forward():
            return [model.predict_proba(patches[k:k + 16]) for k in range(0, n, 16)]

        maps = torch.cat(forward())
        include, scores = model.tile_gate(maps, GATE_THR, 1)
        row["kept"] = int(include.sum())
        row["predict_tiled_us"] = timed(torch, lambda: model.predict_tiled(frames, PATCH, STRIDE, TARGET, blend="probs", gate_thr=GATE_THR,
                                                                           channel_order="bgr"), args.iters, args.warmup)
        row["forward_us"] = timed(torch, forward, args.iters, args.warmup)
        row["gather_us"] = timed(torch, lambda: model.gather_tiles(frames, PATCH, STRIDE, TARGET, "bgr"), args.iters, args.warmup)
        row["gate_us"] = timed(torch, lambda: model.tile_gate(maps, GATE_THR, 1), args.iters, args.warmup)
        row["blend_us"] = timed(torch, lambda: model.blend_tiles(maps, (H, W), PATCH, STRIDE, include), args.iters, args.warmup)
        row["blend_mask_only_us"] = timed(torch, lambda: model.blend_tiles(maps, (H, W), PATCH, STRIDE, include, False), args.iters, args.warmup)
        row["blend_min_bytes"] = int(maps.numel() * 4 + B * H * W * (1 + 4 * CLASSES) + n)
        row["blend_gbytes_per_s"] = round(row["blend_min_bytes"] / row["blend_us"] / 1e3, 1)
        row["glue_us"] = round(row["gather_us"] + row["gate_us"] + row["blend_us"], 1)
        row["glue_over_forward"] = round(row["glue_us"] / row["forward_us"], 4)
        result["rows"].append(row)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"metric": "gather_us+gate_us+blend_us over forward_us",
                      "rows": [(r["batch"], r["glue_us"], r["forward_us"], r["glue_over_forward"]) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
