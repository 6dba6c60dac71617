#!/usr/bin/env python3
"""Morphology programs on the device: time per call against the component filter, the network and the host path.

B = 16 masks at 512 x 512 of two kinds -- (a) the structured scenes of unet_amd.components.make_scene_mask, (b) the
speckled masks of the synthetic net (tests/golden/b_c3_512x512_b16.npz) -- and B = 32 scenes at 448 x 800, through
`unetpp_morphology` (close(E5) of the tape, dilate(E25) of the cable, the ring program tape & (dilate(cable, E15) -
erode(cable, E5))) called through ctypes as scripts/components_bench.py calls the filters, and through the methods
built on it (constrain_tape_to_ring, postprocess_masks, tape_holes): device events around `--iters` calls after
`--warmup` calls, median of three loops.  In the same run: the mask-in / mask-out launch the ring program is measured
against (`unetpp_components_filter`, rule largest), `components`, `filter_components(rule="largest")`, `segment()` of a
batch of the same size in `exact` (the bar: postprocess_masks must stay below it) and, where scipy imports, the host
path the ring replaces (pinned D2H of both masks, scipy.ndimage.binary_dilation / binary_erosion with the same
elements on one thread, H2D of the ring).

    python scripts/morphology_bench.py [--iters 20] [--warmup 5] [--json OUT.json] [--only-morphology] [--inputs scenes]

Per-launch times and the launch count come from a run of its own under `rocprofv3 --kernel-trace --stats` with
--only-morphology (no counters in that run).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_timing import timed  # noqa: E402

K = 8192


def host_ring(torch, d, mo):
    """What a frame loop does today for the ring: both class masks cross PCIe, one host thread runs the morphology,
    the ring crosses back."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    pinned = torch.empty(d.shape, dtype=torch.uint8).pin_memory()
    t0 = time.perf_counter()
    pinned.copy_(d, non_blocking=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    e15, e5 = mo.structuring_element("ellipse", 15), mo.structuring_element("ellipse", 5)
    host = pinned.numpy()
    ring = np.empty_like(host)
    for i, m in enumerate(host):
        cable = m == 1
        ring[i] = (m == 2) & ndimage.binary_dilation(cable, e15) & ~ndimage.binary_erosion(cable, e5, border_value=1)
    t2 = time.perf_counter()
    back = torch.from_numpy(ring).pin_memory().to(d.device, non_blocking=True)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    del back
    return {"d2h_us": round((t1 - t0) * 1e6), "morphology_us": round((t2 - t1) * 1e6), "h2d_us": round((t3 - t2) * 1e6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of scenes,speckle,wide (default: all)")
    ap.add_argument("--only-morphology", action="store_true", help="no segment(), no host path: the run to put under rocprofv3")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, components as cc, morphology as mo, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters,
              "warmup": args.warmup, "rows": []}
    print(result["version"])
    model = NestedUNet(3, deep_supervision=True, max_batch=16, max_hw=(512, 512)).to("cuda:0")
    model.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    model.eval()
    model._ensure_engine(1, 16, 16)

    net = np.load(os.path.join(ROOT, "tests", "golden", "b_c3_512x512_b16.npz"))["mask"]
    inputs = {"scenes": np.stack([cc.make_scene_mask(512, 512, seed) for seed in range(16)]),
              "speckle": np.ascontiguousarray(net[:16]),
              "wide": np.stack([cc.make_scene_mask(448, 800, seed) for seed in range(32)])}
    if args.inputs:
        inputs = {k: inputs[k] for k in args.inputs.split(",")}

    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for name, masks in inputs.items():
        B, H, W = masks.shape
        d = torch.from_numpy(masks).cuda()
        stream = ctypes.c_void_p(torch.cuda.current_stream(d.device).cuda_stream)
        out = torch.empty_like(d)
        row = {"input": name, "batch": B, "h": H, "w": W}
        if not args.only_morphology:
            frames = np.stack([syn.make_frame_u8(H, W, i, ("smooth", "uniform")[i % 2], 1234) for i in range(B)])
            x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
            row["segment_us"] = timed(torch, lambda: model.segment(x), args.iters, args.warmup)
            del x

        def program(key, builder, *params):
            _, c_el, n_el, c_st, n_st, res = model._morph_named(key, params, builder)
            return lambda m0, c0, m1, c1: lib.unetpp_morphology(model._handle, p(m0), c0, p(m1), c1, B, H, W, c_el, n_el, c_st, n_st,
                                                                res, 1, p(out), stream)

        close5 = program("bench_close", lambda: mo.program_single("close", mo.structuring_element("ellipse", 5)))
        dilate25 = program("bench_dilate", lambda: mo.program_single("dilate", mo.structuring_element("ellipse", 25)))
        ring = program("ring", mo.program_ring, 15, 5)
        for key, call in (("close5_us", lambda: close5(d, 2, None, -1)), ("dilate25_us", lambda: dilate25(d, 1, None, -1)),
                          ("ring_us", lambda: ring(d, 2, d, 1))):
            assert call() == 0
            row[key] = timed(torch, call, args.iters, args.warmup)
        row["ring_pixels"] = int(out.count_nonzero())

        # the mask-in / mask-out launch of the parent the ring program is measured against
        labels, num, stats, sums, ws, _ = model._components(d, 1, 8, K, True)
        params = _lib.CcRule(50.0, 50.0, 300.0, 0.3, 1.6, 0.3, float(W))
        filt = lambda: lib.unetpp_components_filter(model._handle, p(labels), p(num), p(stats), p(sums), B, H, W, K, 0,
                                                    ctypes.byref(params), 1, p(out), p(ws), stream)
        assert filt() == 0
        row["filter_largest_launch_us"] = timed(torch, filt, args.iters, args.warmup)
        row["ring_over_filter"] = round(row["ring_us"] / row["filter_largest_launch_us"], 2)
        row["components_us"] = timed(torch, lambda: model._components(d, 1, 8, K, True), args.iters, args.warmup)
        row["components_plus_largest_us"] = timed(torch, lambda: model.filter_components(d, 1, rule="largest", min_area=50, check=False),
                                                  args.iters, args.warmup)
        row["constrain_tape_to_ring_us"] = timed(torch, lambda: model.constrain_tape_to_ring(d, d, 2, 1, check=False), args.iters, args.warmup)
        row["postprocess_masks_us"] = timed(torch, lambda: model.postprocess_masks(d, 1, 2, W, check=False), args.iters, args.warmup)
        row["tape_holes_us"] = timed(torch, lambda: model.tape_holes(d), args.iters, args.warmup)
        if not args.only_morphology:
            row["host_ring"] = host_ring(torch, d, mo)
            row["postprocess_over_segment"] = round(row["postprocess_masks_us"] / row["segment_us"], 3)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "ring_us", "rows": [(r["input"], r["ring_us"], r["filter_largest_launch_us"]) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
