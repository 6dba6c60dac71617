#!/usr/bin/env python3
"""The multi-scale and the DoG burr detector on the device: time per call against the network, in one run.

B = 16 scenes at 512 x 512 and B = 32 at 448 x 800 from unet_amd.edges.make_burr_scene (four distinct scenes per
workload, repeated to the batch; noise sigma 1 for the multi-scale detector, as in its fixtures), through
`edges_combined` (Canny with the blur fused, the Sobel maximum, the union), `detect_burrs_enhanced`, `burr_mask_dog`,
`dog_band` alone and `detect_burrs`, with the timing loop of scripts/burr_bench.py: device events around `--iters` calls
after `--warmup` calls, median of three loops.  In the same run: `segment()` of a batch of the same size in `exact`, the
bar of DESIGN.md §5.8 each detector must stay below.

    python scripts/burr_enhanced_bench.py [--iters 20] [--warmup 5] [--json OUT.json] [--only-burr] [--inputs square]

Per-launch times come from a run of its own under `rocprofv3 --kernel-trace --stats` with --only-burr (no counters in
that run).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of square,wide (default: both)")
    ap.add_argument("--only-burr", action="store_true", help="no segment(): the run to put under rocprofv3")
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
        noisy = [ed.make_burr_scene(H, W, seed) for seed in range(4)]
        quiet = [ed.make_burr_scene(H, W, seed, noise_sigma=1.0) for seed in range(4)]
        dg = torch.from_numpy(np.stack([noisy[i % 4][0] for i in range(B)])).cuda()
        dq = torch.from_numpy(np.stack([quiet[i % 4][0] for i in range(B)])).cuda()
        dc = torch.from_numpy(np.stack([noisy[i % 4][1] for i in range(B)])).cuda()
        band = model.boundary_band(dc)
        row = {"input": name, "batch": B, "h": H, "w": W}
        t = lambda fn: timed(torch, fn, args.iters, args.warmup)
        if not args.only_burr:
            frames = np.stack([syn.make_frame_u8(H, W, i, ("smooth", "uniform")[i % 2], 1234) for i in range(B)])
            x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
            row["segment_us"] = t(lambda: model.segment(x))
            del x
        row["canny_us"] = t(lambda: model.canny(dq, 30, 100, blur=(5, 1.0)))
        row["edges_combined_us"] = t(lambda: model.edges_combined(dq))
        row["detect_burrs_enhanced_us"] = t(lambda: model.detect_burrs_enhanced(dq, dc, check=False))
        row["dog_band_us"] = t(lambda: model.dog_band(dg, band))
        row["burr_mask_dog_us"] = t(lambda: model.burr_mask_dog(dg, dc, check=False))
        row["detect_burrs_us"] = t(lambda: model.detect_burrs(dg, dc, check=False))
        row["has_burr_us"] = t(lambda: model.has_burr(dc))
        row["enhanced_pixels"] = int(model.detect_burrs_enhanced(dq, dc).count_nonzero())
        row["dog_pixels"] = int(model.burr_mask_dog(dg, dc).count_nonzero())
        row["edge_pixels"] = int(model.edges_combined(dq).count_nonzero())
        if not args.only_burr:
            for k in ("edges_combined", "detect_burrs_enhanced", "burr_mask_dog", "detect_burrs"):
                row[k + "_over_segment"] = round(row[k + "_us"] / row["segment_us"], 3)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "detect_burrs_enhanced_us",
                      "rows": [(r["input"], r["detect_burrs_enhanced_us"], r["burr_mask_dog_us"], r.get("segment_us")) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
