#!/usr/bin/env python3
"""The measurement step on the device: time per call against the network and the path the parent commit offered.

B = 16 wrap scenes at 512 x 512 and B = 32 at 448 x 800 from unet_amd.geometry.make_wrap_scene (four distinct scenes
per workload, repeated to the batch), through `diameter_metrics`, `analyze_defects`, `thickness_profile` and the three
new launches alone (`row_widths`, `width_profile`, `components_summary`): device events around `--iters` calls after
`--warmup` calls, median of three loops.  In the same run: `segment()` of a batch of the same size in `exact` (the bar
of DESIGN.md §5.8: diameter_metrics + analyze_defects must stay below it, so that the frame rate stays the network's)
and the path the parent commit offered for the diameters (filter_components twice, mask_stats, a read-back of the
widths and counts, then smooth_widths_np and the median on one host thread), timed with a wall clock around a
synchronised call.

    python scripts/geometry_bench.py [--iters 20] [--warmup 5] [--json OUT.json] [--only-geometry] [--inputs square]

Per-launch times come from a run of its own under `rocprofv3 --kernel-trace --stats` with --only-geometry (no counters
in that run).
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
from bench_timing import timed  # noqa: E402


def parent_path(torch, ge, model, pred, taps):
    """The diameters as the parent commit could form them: the two filters and mask_stats on the device, widths and
    counts across PCIe, smoothing and medians on one host thread.  Returns (dc_px, dt_px, valid_rows) per frame."""
    cable = model.filter_components(pred, 1, rule="largest", min_area=50, check=False)
    tape = model.filter_components(pred, 2, rule="largest", min_area=50, check=False)
    both = cable + 2 * tape                                      # classes are exclusive: one mask_stats call serves both
    counts, widths = model.mask_stats(both)
    w = widths[:, 1:3].cpu().numpy()
    counts.cpu()
    out = []
    for x in w:
        _, _, dc, dt, n = ge.width_profile_np(x, taps, 20)
        out.append((float(dc), float(dt), n))
    return out


def wall(torch, fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(ts), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of square,wide (default: both)")
    ap.add_argument("--only-geometry", action="store_true", help="no segment(), no parent path: the run to put under rocprofv3")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, geometry as ge, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters,
              "warmup": args.warmup, "rows": []}
    print(result["version"])
    model = NestedUNet(3, deep_supervision=True, max_batch=16, max_hw=(512, 512)).to("cuda:0")
    model.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    model.eval()
    taps = ge.gaussian_taps_f32(31)

    shapes = {"square": (16, 512, 512), "wide": (32, 448, 800)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W) in shapes.items():
        scenes = [ge.make_wrap_scene(H, W, seed) for seed in range(4)]
        pred = torch.from_numpy(np.stack([scenes[i % 4] for i in range(B)])).cuda()
        row = {"input": name, "batch": B, "h": H, "w": W}
        if not args.only_geometry:
            frames = np.stack([syn.make_frame_u8(H, W, i, ("smooth", "uniform")[i % 2], 1234) for i in range(B)])
            x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
            row["segment_us"] = timed(torch, lambda: model.segment(x), args.iters, args.warmup)
            del x
        row["diameter_metrics_us"] = timed(torch, lambda: model.diameter_metrics(pred, check=False), args.iters, args.warmup)
        row["analyze_defects_us"] = timed(torch, lambda: model.analyze_defects(pred, check=False), args.iters, args.warmup)
        row["thickness_profile_us"] = timed(torch, lambda: model.thickness_profile(pred), args.iters, args.warmup)
        row["row_widths_us"] = timed(torch, lambda: model.row_widths(pred, 1, pred, 2), args.iters, args.warmup)
        widths, _ = model.row_widths(pred, 1, pred, 2)
        row["width_profile_us"] = timed(torch, lambda: model.width_profile(widths, 1, 20, taps, False), args.iters, args.warmup)
        _, num, stats, _ = model.components(pred, 2)
        row["components_summary_us"] = timed(torch, lambda: model.components_summary(num, stats, 10), args.iters, args.warmup)
        d = model.diameter_metrics(pred)
        row["valid_rows"] = d["valid_rows"][:4].cpu().tolist()
        row["dc_px"] = d["dc_px"][:4].cpu().tolist()
        if not args.only_geometry:
            got = parent_path(torch, ge, model, pred, taps)
            assert [g[2] for g in got[:4]] == row["valid_rows"] and [g[0] for g in got[:4]] == row["dc_px"], "the two paths disagree"
            row["parent_path_wall_us"] = wall(torch, lambda: parent_path(torch, ge, model, pred, taps))
            row["diameter_metrics_wall_us"] = wall(torch, lambda: {k: v.cpu() for k, v in model.diameter_metrics(pred, check=False).items()})
            both = row["diameter_metrics_us"] + row["analyze_defects_us"]
            row["measure_over_segment"] = round(both / row["segment_us"], 3)
            row["parent_over_segment"] = round(row["parent_path_wall_us"] / row["segment_us"], 3)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "diameter_metrics_us+analyze_defects_us", "rows": [
        (r["input"], r["diameter_metrics_us"] + r["analyze_defects_us"], r.get("segment_us")) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
