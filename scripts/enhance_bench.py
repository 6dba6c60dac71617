#!/usr/bin/env python3
"""The grey-frame enhancement on the device: time per batch against the network and against the traffic floor.

`preprocess_frames` (is_grayscale_frame + CLAHE + gamma + bilateral filter, PreprocessConfig's defaults) on B = 4 frames
of 1080 x 1920 and B = 16 of 512 x 512, all grey (unet_amd.enhance.make_enhance_scene, four distinct scenes per workload
repeated to the batch): device events around `--iters` calls after `--warmup` calls, median of three loops.  In the same
run: `segment()` of the same batch in `exact` (the large frames resized to 512 x 512 first, as the frame loop does), and
the copy bandwidth scripts/hbm_probe.py measures, run as a child process before the engine exists.

The sequence's compulsory traffic is 8 bytes per pixel (stats: 3 read + 1 written; apply: 1 read + 3 written; the halo
and the tables come on top and mostly hit in cache), so `floor_us` = 8 H W B / copy bandwidth and `traffic_fraction` =
floor_us / preprocess_us.  The parts (`is_grayscale`, `clahe`, `bilateral_filter`,
`bgr_to_gray`) are timed alone as well.

    python scripts/enhance_bench.py [--iters 20] [--warmup 5] [--json OUT.json] [--only-enhance] [--inputs full]

Per-launch times come from a run of its own under `rocprofv3 --kernel-trace --stats` with --only-enhance (no counters in
that run).
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_timing import timed  # noqa: E402
BYTES_PER_PIXEL = 3 + 1 + 1 + 3            # stats reads BGR and writes grey; apply reads grey and writes BGR


def copy_bandwidth():
    """TB/s of the 1 GiB copy of scripts/hbm_probe.py, run as a child process of its own."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "hbm_probe.py")], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    m = re.search(r"^copy .*?([0-9.]+) TB/s", out, re.M)
    if not m:
        raise RuntimeError("hbm_probe.py printed no copy line:\n" + out)
    return float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of full,square (default: both)")
    ap.add_argument("--only-enhance", action="store_true", help="no segment(), no bandwidth probe: the run to put under rocprofv3")
    args = ap.parse_args()

    copy_tbs = None if args.only_enhance else copy_bandwidth()
    import torch
    from unet_amd import _lib, enhance as en, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters,
              "warmup": args.warmup, "copy_tb_per_s": copy_tbs, "rows": []}
    print(result["version"], "copy", copy_tbs, "TB/s")
    model = NestedUNet(3, deep_supervision=True, max_batch=16, max_hw=(512, 512)).to("cuda:0")
    model.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    model.eval()

    shapes = {"full": (4, 1080, 1920), "square": (16, 512, 512)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W) in shapes.items():
        scenes = [en.make_enhance_scene(H, W, seed) for seed in range(4)]
        x = torch.from_numpy(np.stack([scenes[i % 4] for i in range(B)])).cuda()
        row = {"input": name, "batch": B, "h": H, "w": W}
        out, dec = model.preprocess_frames(x, return_decisions=True)
        assert bool(dec.all()), "the bench frames must all be grey"
        row["out_sha_frame0"] = __import__("hashlib").sha256(out[0].cpu().numpy().tobytes()).hexdigest()[:16]
        row["preprocess_us"] = timed(torch, lambda: model.preprocess_frames(x), args.iters, args.warmup)
        row["preprocess_us_per_launch"] = round(row["preprocess_us"] / 4, 1)          # one memset and three kernels
        gray = model.bgr_to_gray(x)
        row["is_grayscale_us"] = timed(torch, lambda: model.is_grayscale(x), args.iters, args.warmup)
        row["bgr_to_gray_us"] = timed(torch, lambda: model.bgr_to_gray(x), args.iters, args.warmup)
        row["clahe_us"] = timed(torch, lambda: model.clahe(gray), args.iters, args.warmup)
        row["bilateral_us"] = timed(torch, lambda: model.bilateral_filter(gray), args.iters, args.warmup)
        if not args.only_enhance:
            small = out if (H, W) == (512, 512) else model.resize_frames(out, (512, 512))
            row["segment_us"] = timed(torch, lambda: model.segment(small), args.iters, args.warmup)
            row["preprocess_over_segment"] = round(row["preprocess_us"] / row["segment_us"], 3)
            row["floor_us"] = round(BYTES_PER_PIXEL * B * H * W / (copy_tbs * 1e12) * 1e6, 1)
            row["traffic_fraction"] = round(row["floor_us"] / row["preprocess_us"], 3)
            row["achieved_tb_per_s"] = round(BYTES_PER_PIXEL * B * H * W / (row["preprocess_us"] * 1e-6) / 1e12, 3)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "preprocess_us", "rows": [(r["input"], r["preprocess_us"], r.get("segment_us")) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
