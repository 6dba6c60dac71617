#!/usr/bin/env python3
"""The spatial, fixed and simple video loops on the device (unet_amd/simple_loops.py, frame_loop.process_frames_spatial, _fixed,
_confidence, _simple): time per batch of the new calls and of the six whole loops, against the same work on the host and
against predict_proba of the same batch.

Two workloads: B = 32 frames of 448 x 800 and B = 4 frames of 1080 x 1920, synthetic.smooth.  The SimpleUNet (7 classes) runs at
256 x 256, the NestedUNet (3 classes) at 512 x 512, both with synthetic weights in `exact`.  The planes of the clean-up
timings are simple_loops.make_simple_planes at 256 x 256 (the four scenes in turn), so that every class and both verdicts of the
tape filter occur; the loops run on whatever the synthetic weights give.  Device events around at least `--iters` calls (as many
as fill 50 ms) after `--warmup` calls, median of three loops.  Every call repeats on the same buffers, so inputs of up to
a few hundred MB are read from the last-level cache, not from HBM.  Per workload:
  relative_us, confidence_us      the pixel-rule launch on [B,3,512,512] probabilities
  tape_filter_us, keep_us         tape_position_filter and keep_components(500, min_width=20, check=False) on the frame-size masks
                                  of the clean-up
  predict_simple_us, predict_optimized_us, predict_backup_us      the three clean-ups from the planes / the class map on, with
                                  the table, check=True (one read-back)
  host_simple_us, host_optimized_us    the same from .cpu() of the planes on, the NumPy forms on the host; timed on the first
                                  `--host-frames` frames and scaled to B (the forms work frame by frame), host clock
  proba_simple_us, proba_nested_us     predict_proba of the B resized frames: the model step of the loops
  loop_<name>_us                  the six whole loops, frames on the device -> their results, one read-back each
  *_over_proba                    loop time over its model's predict_proba
Not measured here: hardware counters, per-kernel times, the misaligned byte paths (tested in tests/test_gpu_guarded_simple_loops.py).

    python scripts/simple_loops_bench.py [--iters 20] [--warmup 3] [--host-frames 2] [--json OUT.json] [--out OUT.txt] [--inputs video]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, iters, warmup, window_ms=50.0):
    """Median of three loops, in microseconds per call.  A loop holds at least `iters` calls and, for calls of a few
    microseconds, as many as fill `window_ms` (one trial loop sets the count)."""
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    iters = int(min(5000, max(iters, iters * window_ms / max(e0.elapsed_time(e1), 1e-3))))
    loops = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        loops.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return round(statistics.median(loops), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--json", default="")
    ap.add_argument("--out", default="", help="also write the result lines to this file")
    ap.add_argument("--inputs", default="", help="comma list out of video,hd (default: both)")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, frame_loop as fl, simple_loops as sl, synthetic as syn
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup, "rows": []}
    lines = [result["version"]]
    print(lines[0])

    shapes = {"video": (32, 448, 800), "hd": (4, 1080, 1920)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    nested = NestedUNet(3, deep_supervision=True, pretrained_encoder=False, max_batch=32, max_hw=(512, 512)).to("cuda:0")
    nested.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    simple = SimpleUNet(num_classes=7, num_channels=3, max_batch=32, max_hw=(256, 256)).to("cuda:0")
    simple.load_state_dict(syn.make_simple_state_dict(7, 3, 3), strict=True)
    nested.eval(), simple.eval()
    colors = {1: (255, 0, 0), 2: (0, 255, 0), 5: (255, 0, 255)}
    for name, (B, H, W) in shapes.items():
        t = lambda fn: timed(torch, fn, args.iters, args.warmup)
        row = {"input": name, "batch": B, "h": H, "w": W}
        planes_np = sl.make_simple_batch((sl.PLANE_SCENES * B)[:B], 256, 256, 5)
        planes = torch.from_numpy(planes_np).cuda()
        frames = torch.from_numpy(syn.make_frames_u8(B, H, W, "smooth", 7)).cuda()
        probs3 = torch.from_numpy(sl.make_random_probs(B, 3, 512, 512, 3)).cuda()
        row["relative_us"] = t(lambda: sl.relative_threshold(nested, probs3))
        row["confidence_us"] = t(lambda: sl.confidence_threshold(nested, probs3))
        both = sl.predict_simple(simple, planes, (H, W), "optimized", want_table=False, check=False)
        tape, cable = (both == 2).to(torch.uint8), (both == 1).to(torch.uint8)
        row["tape_filter_us"] = t(lambda: sl.tape_position_filter(simple, tape, cable))
        row["keep_us"] = t(lambda: sl.keep_components(simple, tape, 500, None, 20, check=False))
        nf = min(B, args.host_frames)
        for variant in ("simple", "optimized"):
            got, table = sl.predict_simple(simple, planes, (H, W), variant)
            row[f"predict_{variant}_us"] = t(lambda: sl.predict_simple(simple, planes, (H, W), variant))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want, want_table = sl.predict_simple_np(planes[:nf].cpu().numpy(), (H, W), variant)
            row[f"host_{variant}_us"] = round((time.perf_counter() - t0) * 1e6 * B / nf, 1)
            assert (got[:nf].cpu().numpy() == want).all() and (table[:nf].cpu().numpy() == want_table).all(), f"device and host differ: {variant}"
            row[f"host_over_{variant}"] = round(row[f"host_{variant}_us"] / row[f"predict_{variant}_us"], 1)
            row[f"classes_{variant}"] = np.unique(want).tolist()
        pred = simple.resize_masks(simple.segment(simple.resize_frames(frames, (256, 256))), (W, H))
        row["predict_backup_us"] = t(lambda: sl.predict_simple_backup(simple, pred))
        small_s, small_n = simple.resize_frames(frames, (256, 256)), nested.resize_frames(frames, (512, 512))
        row["proba_simple_us"] = t(lambda: simple.predict_proba(small_s))
        row["proba_nested_us"] = t(lambda: nested.predict_proba(small_n))
        loops = {"spatial": (nested, lambda: fl.process_frames_spatial(nested, frames)), "fixed": (nested, lambda: fl.process_frames_fixed(nested, frames)),
                 "confidence": (nested, lambda: fl.process_frames_confidence(nested, frames)),
                 "simple": (simple, lambda: fl.process_frames_simple(simple, frames, "simple", 256, colors)),
                 "optimized": (simple, lambda: fl.process_frames_simple(simple, frames, "optimized", 256, colors)),
                 "backup": (simple, lambda: fl.process_frames_simple(simple, frames, "backup", 256, colors))}
        for lname, (m, fn) in loops.items():
            row[f"loop_{lname}_us"] = t(fn)
            row[f"{lname}_over_proba"] = round(row[f"loop_{lname}_us"] / row["proba_nested_us" if m is nested else "proba_simple_us"], 2)
        result["rows"].append(row)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"metric": "predict_optimized_us", "rows": [(r["input"], r["predict_optimized_us"], r["host_optimized_us"], r["proba_simple_us"]) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
