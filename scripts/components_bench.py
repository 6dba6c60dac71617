#!/usr/bin/env python3
"""Connected components and the component filters on the device: time per call against the network and the host path.

B = 16 masks at 512 x 512 of three kinds -- (a) the structured scenes of unet_amd.components.make_scene_mask (class 1),
(b) the speckled class-2 masks of the synthetic net (tests/golden/b_c3_512x512_b16.npz), (c) the one-pixel serpentine
(one component, the longest union chain) -- through `unetpp_components` and each rule of `unetpp_components_filter`:
device events around `--iters` calls after `--warmup` calls, median of three loops.  In the same run: `segment()` of a
batch of the same size in `exact` (the bar: components + largest must not take longer, or the post-step and not the
network sets the frame rate) and, where scipy imports, the host path the device code replaces (pinned D2H of the
masks, then scipy.ndimage.label + find_objects + sum per frame on one thread).

    python scripts/components_bench.py [--iters 20] [--warmup 5] [--json OUT.json] [--only-components] [--inputs scenes]

Per-launch times come from runs of their own under `rocprofv3 --kernel-trace --stats` with --only-components, one per
input (--inputs); the `bytes` table printed at the end gives each launch's minimum HBM traffic to set them against.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 8192


def timed(torch, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    loops = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        loops.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return statistics.median(loops), loops


def host_path(torch, d, cls):
    """What the frame loops do today: the masks cross PCIe, then one host thread labels each frame."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    pinned = torch.empty(d.shape, dtype=torch.uint8).pin_memory()
    t0 = time.perf_counter()
    pinned.copy_(d, non_blocking=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ones = np.ones((3, 3), int)
    for m in pinned.numpy():
        labels, n = ndimage.label(m == cls, structure=ones)
        idx = np.arange(1, n + 1)
        ndimage.find_objects(labels)
        ndimage.sum(np.ones_like(labels), labels, idx)
    t2 = time.perf_counter()
    return {"d2h_us": (t1 - t0) * 1e6, "label_stats_us": (t2 - t1) * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of scenes,speckle,serpentine (default: all)")
    ap.add_argument("--only-components", action="store_true", help="no segment(), no host path: the run to put under rocprofv3")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, components as cc, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    S, B = args.size, args.batch
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "size": S, "batch": B,
              "iters": args.iters, "warmup": args.warmup, "rows": []}
    print(result["version"])

    model = NestedUNet(3, deep_supervision=True, max_batch=B, max_hw=(S, S)).to("cuda:0")
    model.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    model.eval()
    inputs = {"scenes": (np.stack([cc.make_scene_mask(S, S, seed) for seed in range(B)]), 1)}
    if S == 512:
        net = np.load(os.path.join(ROOT, "tests", "golden", "b_c3_512x512_b16.npz"))["mask"]
        inputs["speckle"] = (np.ascontiguousarray(np.concatenate([net] * ((B + 15) // 16))[:B]), 2)
    inputs["serpentine"] = (np.stack([cc.make_adversarial_masks(S, S)["serpentine"]] * B), 1)
    if args.inputs:
        inputs = {k: inputs[k] for k in args.inputs.split(",")}

    seg_us = None
    if not args.only_components:
        frames = np.stack([syn.make_frame_u8(S, S, i, ("smooth", "uniform")[i % 2], 1234) for i in range(B)])
        x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
        seg_us, loops = timed(torch, lambda: model.segment(x), args.iters, args.warmup)
        result["segment_us"] = round(seg_us, 1)
        print(f"segment() exact, B={B} {S}x{S}: {seg_us:9.1f} us/call  (loops {[round(v, 1) for v in loops]})", flush=True)

    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for name, (masks, cls) in inputs.items():
        d = torch.from_numpy(masks).cuda()
        labels, num, stats, sums, ws, stream = model._components(d, cls, 8, K, True)
        torch.cuda.synchronize()
        ncomp = (num.cpu().numpy() - 1).tolist()
        row = {"input": name, "class": cls, "components_per_frame": [min(ncomp), max(ncomp)]}
        row["components_us"], row["components_loops_us"] = timed(torch, lambda: model._components(d, cls, 8, K, True), args.iters, args.warmup)
        row["labels_only_us"], _ = timed(torch, lambda: model._components(d, cls, 8, K, False), args.iters, args.warmup)
        out = torch.empty_like(d)
        for rule, kw in (("largest", dict(min_area=50.0)), ("spatial", dict(min_area=1000.0)), ("cable_shape", dict(min_area=1000.0))):
            params = _lib.CcRule(kw["min_area"], 50.0, 300.0, 0.3, 1.6, 0.3, float(S))
            call = lambda: lib.unetpp_components_filter(model._handle, p(labels), p(num), p(stats), p(sums), B, S, S, K,
                                                        _lib.CC_RULES[rule], ctypes.byref(params), 1, p(out), p(ws), stream)
            assert call() == 0
            row[f"filter_{rule}_us"], _ = timed(torch, call, args.iters, args.warmup)
            row[f"kept_{rule}"] = int(out.count_nonzero())
        row["components_plus_largest_us"], _ = timed(
            torch, lambda: model.filter_components(d, cls, rule="largest", min_area=50, check=False), args.iters, args.warmup)
        if not args.only_components:
            row["host"] = host_path(torch, d, cls)
        for k, v in list(row.items()):
            if isinstance(v, float):
                row[k] = round(v, 1)
        result["rows"].append(row)
        line = (f"{name:10s} {row['components_per_frame'][0]:5d}-{row['components_per_frame'][1]:<5d} comps/frame  components {row['components_us']:8.1f} us"
                f"  (labels only {row['labels_only_us']:7.1f})  filters largest / spatial / cable_shape {row['filter_largest_us']:6.1f} /"
                f" {row['filter_spatial_us']:6.1f} / {row['filter_cable_shape_us']:6.1f} us   components + largest {row['components_plus_largest_us']:8.1f} us")
        if seg_us:
            line += f" = {row['components_plus_largest_us'] / seg_us:.3f} x segment()"
        if row.get("host"):
            line += f"   host: D2H {row['host']['d2h_us']:.0f} us + label/stats {row['host']['label_stats_us']:.0f} us"
        print(line, flush=True)

    px = B * S * S
    result["min_bytes"] = {"cc_tile_kernel": 5 * px, "cc_compress_kernel": 4 * px, "cc_number_kernel": 4 * px,
                           "cc_relabel_kernel": 8 * px, "cc_apply_kernel": 5 * px}
    print("minimum HBM bytes per launch (mask 1 B, parent / labels 4 B per pixel): "
          + ", ".join(f"{k} {v / 1e6:.1f} MB" for k, v in result["min_bytes"].items()))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "components_plus_largest_us", "segment_us": result.get("segment_us"),
                      "rows": [(r["input"], r["components_plus_largest_us"]) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
