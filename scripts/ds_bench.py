#!/usr/bin/env python3
"""Deep-supervision outputs and pruned UNet++ inference: speed and accuracy per output.

Times `segment(x, output=k)` (uint8 mask only) for k = 0..3 -- the full network for k = 0, a pass that stops after x1_3,
x2_2 or x3_1 for k = 1, 2, 3 -- at config 2 (3-class 512x512, B = 16) and at B = 1, in `exact` and `exact8`: device events
around `--iters` calls, after `--warmup` calls, median of three loops.  Then one profiled call per output prints the
per-launch times of profile_read().  The accuracy column is max |dlogit| of forward_deep_supervision against the
reference fixture tests/golden/ds_c3_64x64.npz (scripts/make_golden_ds.py).

    python scripts/ds_bench.py [--iters 20] [--warmup 5] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fixture_errors(precision, syn, NestedUNet, torch):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ds_c3_64x64.npz"))
    C, B, H, W = int(g["num_classes"]), int(g["B"]), int(g["H"]), int(g["W"])
    m = NestedUNet(C, deep_supervision=True, precision=precision, max_batch=B, max_hw=(H, W)).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(C, 3, True, int(g["wseed"])), strict=True)
    x = torch.from_numpy(syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"])))).cuda()
    outs = m.eval().forward_deep_supervision(x)
    torch.cuda.synchronize()
    return [float(np.abs(outs[k].cpu().numpy() - g[f"out{k}"]).max()) for k in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batches", default="16,1")
    ap.add_argument("--precisions", default="exact,exact8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    S = args.size
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "size": S, "iters": args.iters,
              "warmup": args.warmup, "rows": [], "launches": {}}
    print(result["version"])
    for precision in args.precisions.split(","):
        errs = fixture_errors(precision, syn, NestedUNet, torch)
        for B in (int(b) for b in args.batches.split(",")):
            model = NestedUNet(3, deep_supervision=True, precision=precision, max_batch=B, max_hw=(S, S)).to("cuda:0")
            model.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
            model.eval()
            frames = np.stack([syn.make_frame_u8(S, S, i, ("smooth", "uniform")[i % 2], 1234) for i in range(B)])
            x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
            base_ms = None
            for k in range(4):
                for _ in range(args.warmup):
                    model.segment(x, output=k)
                loops = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        model.segment(x, output=k)
                    e1.record()
                    torch.cuda.synchronize()
                    loops.append(e0.elapsed_time(e1) / args.iters)
                ms = statistics.median(loops)
                base_ms = ms if k == 0 else base_ms
                row = {"precision": precision, "batch": B, "output": k, "ms_per_call": round(ms, 4),
                       "frames_per_s": round(B * 1000.0 / ms, 1), "speedup_vs_out0": round(base_ms / ms, 3),
                       "loops_ms": [round(v, 4) for v in loops], "fixture_max_abs_dlogit": errs[k]}
                result["rows"].append(row)
                print(f"{precision:6s} B={B:2d} out{k}: {ms:8.3f} ms/call  {row['frames_per_s']:9.1f} frames/s  "
                      f"x{row['speedup_vs_out0']:.2f} vs out0   fixture max|dlogit| {errs[k]:.2e}", flush=True)
                model.profile(True)
                model.segment(x, output=k)
                rows = model.profile_read()
                model.profile(False)
                key = f"{precision}_b{B}_out{k}"
                result["launches"][key] = [[n, round(t, 4), f, b] for n, t, f, b in rows]
                ds_rows = [r for r in rows if r[0].startswith("ds")]
                tot = sum(r[1] for r in rows)
                print(f"    profiled: {len(rows)} launches, {tot:.3f} ms in launches"
                      + "".join(f"\n    {n:40s} {t * 1000:8.1f} us  {b / max(t, 1e-9) / 1e6:7.1f} GB/s" for n, t, _, b in ds_rows))
            del model
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "ds_segment_frames_per_s", "rows": [(r["precision"], r["batch"], r["output"], r["frames_per_s"])
                                                                     for r in result["rows"]]}))


if __name__ == "__main__":
    main()
