#!/usr/bin/env python3
"""Non-local-means denoising on the device: time per batch against the parent's denoiser, the network and the host.

`nlmeans.nl_means` alone (on the grey plane CLAHE and gamma leave) and `nlmeans.preprocess_frames_nlm` (decision + CLAHE +
gamma, then the non-local-means launch gated by the decisions) for denoise_strength 5 and 10, on B = 4 frames of
1080 x 1920 and B = 16 of 512 x 512, all grey (unet_amd.nlmeans.make_nlm_scene, four distinct scenes per workload
repeated to the batch): device events around `--iters` calls after `--warmup` calls, median of three loops.  Timed in the
same run, as yardsticks:
  `model.preprocess_frames` with 'bilateral' on the same batch (the other denoiser),
  `segment()` of the same batch in `exact` (the large frames resized to 512 x 512 first, as the frame loop does),
  `nl_means_np` on ONE frame on the host (one run, wall clock).

The kernel's integer work is counted from its scheme (csrc/nlmeans.h), per thread (8 x 4 pixels) and offset: 140
subtractions (the byte extraction rides on them) + 14 x 13 multiply-adds for the row sums + 84 column-sum additions and
subtractions + 32 x (shift, min, multiply-add, addition) = 534 vector operations = 16.7 per pixel and offset, 7,359 per
pixel; LDS reads and address arithmetic are not counted, a multiply-add counts once.  `valu_fraction` is that count over
the time, against 78.6e12 lane-operations/s: the 157.3 TFLOP/s fp32 vector peak of the MI355X at two flops per
lane-operation.

    python scripts/nlmeans_bench.py [--iters 10] [--warmup 3] [--json OUT.json] [--only-nlm] [--inputs full]

Per-launch times come from a run of its own under `rocprofv3 --kernel-trace --stats` with --only-nlm (no counters in
that run).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_timing import timed  # noqa: E402
OPS_PER_PIXEL = 441 * (140 + 14 * 13 + 84 + 32 * 4) // 32            # see the docstring
VALU_LANE_OPS_PER_S = 157.3e12 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of full,square (default: both)")
    ap.add_argument("--only-nlm", action="store_true", help="no segment(), no host run: the run to put under rocprofv3")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, nlmeans as nm, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
              "ops_per_pixel": OPS_PER_PIXEL, "rows": []}
    print(result["version"])
    model = NestedUNet(3, deep_supervision=True, max_batch=16, max_hw=(512, 512)).to("cuda:0")
    model.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    model.eval()

    shapes = {"full": (4, 1080, 1920), "square": (16, 512, 512)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W) in shapes.items():
        scenes = [nm.make_nlm_scene(H, W, seed) for seed in range(4)]
        x = torch.from_numpy(np.stack([scenes[i % 4] for i in range(B)])).cuda()
        row = {"input": name, "batch": B, "h": H, "w": W}
        plain, dec = model.preprocess_frames(x, denoise_method="none", return_decisions=True)
        assert bool(dec.all()), "the bench frames must all be grey"
        gray = plain[..., 0].contiguous()                                # what the filter sees: CLAHE + gamma
        for h in (5, 10):
            out = nm.preprocess_frames_nlm(model, x, denoise_strength=h)
            row[f"changed_h{h}"] = round(float((out != plain).float().mean()), 3)
            row[f"out_sha_frame0_h{h}"] = hashlib.sha256(out[0].cpu().numpy().tobytes()).hexdigest()[:16]
            row[f"nl_means_us_h{h}"] = timed(torch, lambda: nm.nl_means(model, gray, h), args.iters, args.warmup)
            row[f"preprocess_nlm_us_h{h}"] = timed(torch, lambda: nm.preprocess_frames_nlm(model, x, denoise_strength=h), args.iters, args.warmup)
            rate = OPS_PER_PIXEL * B * H * W / (row[f"nl_means_us_h{h}"] * 1e-6)
            row[f"lane_ops_per_s_h{h}"] = float(f"{rate:.4g}")
            row[f"valu_fraction_h{h}"] = round(rate / VALU_LANE_OPS_PER_S, 3)
        row["preprocess_bilateral_us"] = timed(torch, lambda: model.preprocess_frames(x), args.iters, args.warmup)
        row["nlm_over_bilateral_h5"] = round(row["preprocess_nlm_us_h5"] / row["preprocess_bilateral_us"], 1)
        if not args.only_nlm:
            small = plain if (H, W) == (512, 512) else model.resize_frames(plain, (512, 512))
            row["segment_us"] = timed(torch, lambda: model.segment(small), args.iters, args.warmup)
            row["nlm_over_segment_h5"] = round(row["preprocess_nlm_us_h5"] / row["segment_us"], 2)
            g0 = gray[0].cpu().numpy()
            t0 = time.perf_counter()
            want = nm.nl_means_np(g0, 5)
            row["host_np_one_frame_s"] = round(time.perf_counter() - t0, 2)
            assert np.array_equal(nm.nl_means(model, gray[:1], 5)[0].cpu().numpy(), want), "device and host differ"
            row["host_np_batch_over_device_h5"] = round(row["host_np_one_frame_s"] * B / (row["nl_means_us_h5"] * 1e-6))
        result["rows"].append(row)
        print(json.dumps(row), flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "preprocess_nlm_us_h5", "rows": [(r["input"], r["preprocess_nlm_us_h5"], r.get("segment_us")) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
