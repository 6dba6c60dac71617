#!/usr/bin/env python3
"""The probability-map rules on the device: time per batch against the route the parent offers and against the network.

The plane is class 1 of a float32 [B,H,W,2] map (the layout of predict_tiled(blend="probs")), read in place: B = 16 of
512 x 512 and B = 4 of 1080 x 1920, four distinct unet_amd.probmap.make_prob_scene scenes (a 256 x 256 scene tiled to the
frame) repeated to the batch.  Device events around `--iters` calls after `--warmup` calls, median of three loops.  Per
workload:
  levels_us                    probmap.threshold_levels (one launch)
  hysteresis_program_us        the morphology program of hysteresis on codes made beforehand (one launch)
  hysteresis_us                probmap.hysteresis: the two together
  sums_us                      probmap.component_prob_sums on labels made beforehand (one memset, one launch)
  filter_us                    unetpp_components_filter_mean alone on stats and sums made beforehand (two launches)
  filter_by_mean_prob_us       probmap.filter_by_mean_prob, check=False: cleanup program, components, sums, filter
  postprocess_us               probmap.postprocess_probmap, check=False: hysteresis, then the above
  scan25_us / scan49_us        probmap.threshold_histogram with the 25 / 49 thresholds of scan_thresholds: ONE pass over the map
  route25_us / route49_us      what a user of the parent commit has: per threshold torch.ge on the plane (its bool result
                               viewed as uint8, no further copy) and evaluation.confusion(check=False): T passes
  segment_us                   segment() of B frames of the same shape in `exact` (rows rounded up to a multiple of 16:
                               1088 x 1920 for the large workload)
Ratios: route49_over_scan49 = route49_us / scan49_us (the one-pass scan must not lose: above 1), and each step over
segment_us.  Before timing, every device result is compared with the NumPy form on the first frame.

    python scripts/probmap_bench.py [--iters 20] [--warmup 3] [--json OUT.json] [--inputs square] [--no-segment]
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


def tiled_scene(pm, H, W, seed):
    prob, target = pm.make_prob_scene(256, 256, seed)
    reps = ((H + 255) // 256, (W + 255) // 256)
    return np.tile(prob, reps)[:H, :W], np.tile(target, reps)[:H, :W]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of square,full_hd (default: both)")
    ap.add_argument("--no-segment", action="store_true", help="no segment(): the post-processing rows alone")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, evaluation as ev, morphology as mo, probmap as pm, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
              "workgroup_span": pm.layout(), "rows": []}
    print(result["version"])

    shapes = {"square": (16, 512, 512), "full_hd": (4, 1080, 1920)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    K = 8192
    for name, (B, H, W) in shapes.items():
        Hs = (H + 15) // 16 * 16
        model = NestedUNet(2, deep_supervision=False, max_batch=B, max_hw=(Hs, W)).to("cuda:0")
        model.load_state_dict(syn.make_state_dict(2, 3, False, 2), strict=True)
        model.eval()
        scenes = [tiled_scene(pm, H, W, seed) for seed in range(4)]
        prob_np = np.stack([scenes[i % 4][0] for i in range(B)])
        target_np = np.stack([scenes[i % 4][1] for i in range(B)])
        out4 = torch.from_numpy(np.stack([1 - prob_np, prob_np], -1)).cuda()           # [B,H,W,2]; the plane is channel 1
        target = torch.from_numpy(target_np).cuda()
        plane = out4[..., 1]
        row = {"input": name, "batch": B, "h": H, "w": W, "pixel_stride": 2, "defect_share": round(float(target_np.mean()), 4)}
        t = lambda fn: timed(torch, fn, args.iters, args.warmup)

        # the same results as the NumPy forms, on the first frame
        hyst, final = pm.postprocess_probmap(model, out4, channel=1)
        want_h, want_f = pm.postprocess_probmap_np(prob_np[:1])
        assert np.array_equal(hyst[0].cpu().numpy(), want_h[0]) and np.array_equal(final[0].cpu().numpy(), want_f[0]), "device and host differ"
        thr = {T: pm.check_thresholds(pm.scan_values((0.50, 0.99, 0.02 if T == 25 else 0.01))) for T in (25, 49)}
        assert len(thr[25]) == 25 and len(thr[49]) == 49
        hist = pm.threshold_histogram(model, out4, target, thr[49], channel=1)
        assert np.array_equal(hist[0].cpu().numpy(), pm.threshold_hist_np(prob_np[:1], target_np[:1], thr[49])[0]), "device and host differ"
        cm = pm.confusion_from_hist(hist)
        for j in (0, 24, 48):                                   # and the route it replaces gives the same tables
            counts, _ = ev.confusion(model, torch.ge(plane, float(thr[49][j])).view(torch.uint8), target, 2, check=False)
            assert np.array_equal(counts.cpu().numpy(), cm[:, j]), "one-pass scan and per-threshold route differ"
        row["kept_share"], row["hysteresis_share"] = round(float((final != 0).float().mean()), 4), round(float((hyst != 0).float().mean()), 4)

        row["levels_us"] = t(lambda: pm.threshold_levels(model, out4, 0.70, 0.90, channel=1))
        codes = pm.threshold_levels(model, out4, 0.70, 0.90, channel=1)
        program = model._morph_named("hysteresis", (5, 3), pm.program_hysteresis)
        row["hysteresis_program_us"] = t(lambda: model._morph_launch(program, codes, 2, codes, -1, 1))
        row["hysteresis_us"] = t(lambda: pm.hysteresis(model, out4, channel=1))
        cleaned = model._morph_launch(model._morph_named("cleanup", (3,), mo.program_cleanup), hyst, -1, None, -1, 1)
        labels, num, stats, _, ws, _ = model._components(cleaned, -1, 8, K, True)
        row["components_max"] = int(num.max()) - 1
        row["sums_us"] = t(lambda: pm.component_prob_sums(model, labels, num, out4, 1, K))
        sums = pm.component_prob_sums(model, labels, num, out4, 1, K)
        mask = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
        tq = pm.thr_q_of(0.85)
        row["filter_us"] = t(lambda: model._call("unetpp_components_filter_mean", labels, num, stats, sums, B, H, W, K, 50, tq, 1, mask, ws,
                                                 stream_of=labels))
        assert torch.equal(mask, final), "the filter entry and filter_by_mean_prob differ"
        row["filter_by_mean_prob_us"] = t(lambda: pm.filter_by_mean_prob(model, hyst, out4, channel=1, check=False))
        row["postprocess_us"] = t(lambda: pm.postprocess_probmap(model, out4, channel=1, check=False))
        for T in (25, 49):
            values = [float(v) for v in thr[T]]
            row[f"scan{T}_us"] = t(lambda: pm.threshold_histogram(model, out4, target, thr[T], channel=1))

            def route():
                for v in values:
                    ev.confusion(model, torch.ge(plane, v).view(torch.uint8), target, 2, check=False)
            row[f"route{T}_us"] = t(route)
            row[f"route{T}_over_scan{T}"] = round(row[f"route{T}_us"] / row[f"scan{T}_us"], 1)
        if not args.no_segment:
            x = torch.from_numpy(syn.make_frames_u8(B, Hs, W, "smooth", 7)).cuda()
            row["segment_h"] = Hs
            row["segment_us"] = t(lambda: model.segment(x))
            for k in ("levels_us", "hysteresis_us", "sums_us", "filter_us", "filter_by_mean_prob_us", "postprocess_us", "scan25_us", "scan49_us"):
                row[k.replace("_us", "_over_segment")] = round(row[k] / row["segment_us"], 4)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        del model

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"metric": "route49_over_scan49", "rows": [(r["input"], r["scan49_us"], r["route49_us"], r["route49_over_scan49"])
                                                               for r in result["rows"]]}))
    assert all(r["scan49_us"] < r["route49_us"] for r in result["rows"]), "the one-pass scan lost to the per-threshold route"


if __name__ == "__main__":
    main()
