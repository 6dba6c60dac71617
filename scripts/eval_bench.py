#!/usr/bin/env python3
"""Segmentation evaluation on the device: time per batch against the parent's one-mask reductions, the network and the host.

`evaluation.confusion` and `evaluation.mask_disagreement` on B = 16 masks of 512 x 512 with C = 3 and B = 32 of 448 x 800
with C = 7 (unet_amd.evaluation.make_eval_scene, four distinct scenes per workload repeated to the batch): device events
around `--iters` calls after `--warmup` calls, median of three loops.  Per workload:
  confusion_us / confusion_total_us            the function (check=False: nothing read back) on the realistic pair, without
                                               and with a running total
  confusion_bg_us / confusion_bg_total_us      the same on an all-background pair: every pixel in one bin, the worst contention
  confusion_entry_us / confusion_bg_entry_us   unetpp_confusion_u8 alone into preallocated outputs (memsets + one launch)
  disagreement_us / disagreement_logits_us     mask_disagreement without and with float32 logits [B,C,H,W]
Timed in the same run, as yardsticks:
  count_nonzero_us, count_nonzero_entry_us, mask_stats_us   the parent's kernels that read ONE mask, on the same batch
  segment_us                                   segment() of a batch of frames of the same shape, in `exact`
  host_confusion_np_one_frame_us               confusion_np on one frame on the host (wall clock, best of three)
  host_reference_passes_one_frame_us           the 6 C boolean reductions compute_metrics makes, on one frame on the host
Ratios: confusion_entry_us / count_nonzero_entry_us (two mask reads per pixel against one bound it at about two), and
all-background over realistic (above two would mean the run folding is not doing its job).  Neither is a test.

    python scripts/eval_bench.py [--iters 50] [--warmup 5] [--json OUT.json] [--inputs square] [--only-eval]

The loops above are bound by the host's launch rate (two memsets and a launch in about 14 us), not by the kernels.  The
kernels' own times come from runs under `rocprofv3 --kernel-trace --stats` with --trace-case, one variant of each kernel
per run (no counters in those runs).
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


def host_best(fn, runs=3):
    best = None
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return round(best * 1e6, 1)


def reference_shaped_passes(pred, target, C):
    """The boolean reductions compute_metrics makes per class over the flattened set (two target counts, two pred
    counts, the intersection and the union), for the time of it alone."""
    p, t = pred.reshape(-1), target.reshape(-1)
    acc = 0
    for c in range(C):
        tc, pc = t == c, p == c
        acc += int(tc.sum()) + int(pc.sum()) + int((pc & tc).sum()) + int((pc | tc).sum()) + int(pc.sum()) + int(tc.sum())
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of square,wide (default: both)")
    ap.add_argument("--only-eval", action="store_true", help="no segment(), no host runs")
    ap.add_argument("--trace-case", default="", help="realistic | background | realistic_total | background_total: only that confusion "
                    "entry, count_nonzero and mask_disagreement (with logits for the background cases), for a run under rocprofv3")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, evaluation as ev, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
              "workgroup_span": ev.layout(), "rows": []}
    print(result["version"])

    shapes = {"square": (16, 512, 512, 3), "wide": (32, 448, 800, 7)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W, C) in shapes.items():
        model = NestedUNet(C, deep_supervision=True, max_batch=B, max_hw=(H, W)).to("cuda:0")
        model.load_state_dict(syn.make_state_dict(C, 3, True, 2), strict=True)
        model.eval()
        scenes = [ev.make_eval_scene(H, W, seed, C) for seed in range(4)]
        pred_np = np.stack([scenes[i % 4][0] for i in range(B)])
        target_np = np.stack([scenes[i % 4][1] for i in range(B)])
        pred, target = torch.from_numpy(pred_np).cuda(), torch.from_numpy(target_np).cuda()
        zeros = torch.zeros_like(pred)
        logits = torch.randn((B, C, H, W), dtype=torch.float32, device="cuda")
        total = torch.zeros((C * C + 2,), dtype=torch.int64, device="cuda")
        row = {"input": name, "batch": B, "h": H, "w": W, "num_classes": C}

        want = ev.confusion_np(pred_np, target_np, C)
        if not args.trace_case:                                 # (a traced run holds one variant of each kernel and nothing else)
            counts, outside = ev.confusion(model, pred, target, C)
            assert np.array_equal(counts.cpu().numpy(), want[0]) and np.array_equal(outside.cpu().numpy(), want[1]), "device and host differ"
            d = ev.mask_disagreement(model, pred, target, logits)
            assert np.array_equal(d["n_diff"].cpu().numpy(), (pred_np != target_np).sum((1, 2)))
        row["differing_share"] = round(float((pred_np != target_np).mean()), 4)
        row["largest_bin_share"] = round(float(want[0].sum(0).max() / (B * H * W)), 3)
        row["miou"] = ev.metrics_from_confusion(want[0])[0]

        t = lambda fn: timed(torch, fn, args.iters, args.warmup)
        if args.trace_case:                                     # one variant of each kernel per run: the stats go by kernel name
            bg, tot = args.trace_case.startswith("background"), args.trace_case.endswith("_total")
            p, q = (zeros, zeros) if bg else (pred, target)
            raw_c = torch.empty((B, C, C), dtype=torch.int32, device="cuda")
            raw_o = torch.empty((B, 2), dtype=torch.int32, device="cuda")
            raw_n = torch.empty((B,), dtype=torch.int32, device="cuda")
            row["trace_case"] = args.trace_case
            model._input(pred, "pred")                          # makes the engine: the entries below are called directly
            row["confusion_entry_us"] = t(lambda: model._call("unetpp_confusion_u8", p, q, B, H, W, C, -1, raw_c, raw_o, total if tot else None, stream_of=pred))
            if not tot:
                row["count_nonzero_entry_us"] = t(lambda: model._call("unetpp_count_nonzero_u8", pred, B, H, W, raw_n, stream_of=pred))
                row["disagreement_us"] = t(lambda: ev.mask_disagreement(model, pred, target, logits if bg else None))
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            continue
        row["confusion_us"] = t(lambda: ev.confusion(model, pred, target, C, check=False))
        row["confusion_total_us"] = t(lambda: ev.confusion(model, pred, target, C, total=total, check=False))
        row["confusion_bg_us"] = t(lambda: ev.confusion(model, zeros, zeros, C, check=False))
        row["confusion_bg_total_us"] = t(lambda: ev.confusion(model, zeros, zeros, C, total=total, check=False))
        raw_c = torch.empty((B, C, C), dtype=torch.int32, device="cuda")
        raw_o = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        row["confusion_entry_us"] = t(lambda: model._call("unetpp_confusion_u8", pred, target, B, H, W, C, -1, raw_c, raw_o, None, stream_of=pred))
        row["confusion_entry_total_us"] = t(lambda: model._call("unetpp_confusion_u8", pred, target, B, H, W, C, -1, raw_c, raw_o, total, stream_of=pred))
        row["confusion_bg_entry_us"] = t(lambda: model._call("unetpp_confusion_u8", zeros, zeros, B, H, W, C, -1, raw_c, raw_o, None, stream_of=pred))
        row["confusion_bg_entry_total_us"] = t(lambda: model._call("unetpp_confusion_u8", zeros, zeros, B, H, W, C, -1, raw_c, raw_o, total, stream_of=pred))
        row["disagreement_us"] = t(lambda: ev.mask_disagreement(model, pred, target))
        row["disagreement_logits_us"] = t(lambda: ev.mask_disagreement(model, pred, target, logits))
        # the parent's one-mask reductions on the same batch
        row["count_nonzero_us"] = t(lambda: model.count_nonzero(pred))
        raw_n = torch.empty((B,), dtype=torch.int32, device="cuda")
        row["count_nonzero_entry_us"] = t(lambda: model._call("unetpp_count_nonzero_u8", pred, B, H, W, raw_n, stream_of=pred))
        if C == model.num_classes:
            row["mask_stats_us"] = t(lambda: model.mask_stats(pred))
        row["confusion_entry_over_count_nonzero_entry"] = round(row["confusion_entry_us"] / row["count_nonzero_entry_us"], 2)
        row["confusion_over_count_nonzero"] = round(row["confusion_us"] / row["count_nonzero_us"], 2)
        row["background_over_realistic_entry"] = round(row["confusion_bg_entry_us"] / row["confusion_entry_us"], 2)
        row["background_over_realistic"] = round(row["confusion_bg_us"] / row["confusion_us"], 2)
        if not args.only_eval:
            x = torch.from_numpy(syn.make_frames_u8(B, H, W, "smooth", 7)).cuda()
            row["segment_us"] = t(lambda: model.segment(x))
            row["confusion_over_segment"] = round(row["confusion_us"] / row["segment_us"], 4)
            row["host_confusion_np_one_frame_us"] = host_best(lambda: ev.confusion_np(pred_np[:1], target_np[:1], C))
            row["host_reference_passes_one_frame_us"] = host_best(lambda: reference_shaped_passes(pred_np[0], target_np[0], C))
            row["host_np_batch_over_device"] = round(row["host_confusion_np_one_frame_us"] * B / row["confusion_us"], 1)
            row["host_passes_batch_over_device"] = round(row["host_reference_passes_one_frame_us"] * B / row["confusion_us"], 1)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        del model

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if not args.trace_case:
        print(json.dumps({"metric": "confusion_us", "rows": [(r["input"], r["confusion_us"], r["confusion_bg_us"], r["count_nonzero_us"]) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
