#!/usr/bin/env python3
"""Validation losses on the device: time per batch of the kernel, of combined_loss, and of the same losses in plain torch.

B = 16 logit maps of 512 x 512 with C = 3 and B = 32 of 448 x 800 with C = 7 (unet_amd.loss.make_logits "plain" and
make_target, four distinct scenes per workload repeated to the batch): device events around `--iters` calls after
`--warmup` calls, median of three loops.  Per workload:
  entry_us              unetpp_loss_sums_f32 alone into a preallocated table (one memset + one launch per call)
  kernel_bytes          B H W (4 C + 1): what the kernel must read
  entry_share_of_hbm    kernel_bytes / entry_us as a fraction of 6.3 TB/s (the achievable HBM rate)
  loss_sums_us          loss.loss_sums (allocation + entry, nothing read back)
  combined_loss_us / advanced_loss_us      one launch, one read-back, the float64 algebra on the host
  torch_combined_us / torch_advanced_us    the route without this module: the same losses in plain torch ops on the device
                        (log_softmax, one-hot, products and sums; one .tolist() read-back), checked against the device call
  torch_over_combined, torch_over_advanced     the ratios
  segment_us            segment() of a batch of frames of the same shape, in `exact`, and each call as a fraction of it
The entry loop is bound by the kernel where the kernel is long (the 7-class workload) and by the host's launch rate where
it is short; the kernel's own time comes from a run under `rocprofv3 --kernel-trace --stats` with --trace (only the entry
is called, no counters in that run).

    python scripts/loss_bench.py [--iters 50] [--warmup 5] [--json OUT.json] [--inputs square] [--trace]
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
HBM_BYTES_PER_US = 6.3e6                                        # 6.3 TB/s


def torch_losses(torch, logits, target, advanced):
    """CombinedLoss / AdvancedCombinedLoss with their defaults, written with plain torch ops; one read-back."""
    C = logits.shape[1]
    logp = torch.log_softmax(logits, dim=1)
    p = torch.exp(logp)
    onehot = torch.nn.functional.one_hot(target.long(), C).permute(0, 3, 1, 2).to(logits.dtype)
    nll = -(logp * onehot).sum(1)
    inter, psum, tsum = (p * onehot).sum((2, 3)), p.sum((2, 3)), onehot.sum((2, 3))
    dice = (2 * inter + 1e-5) / (psum + tsum + 1e-5)
    valid = tsum > 0
    valid[:, 0] = False
    if not bool(valid.any()):
        valid[:, 1:] = True
    dice_loss = 1 - dice[valid].mean()
    if not advanced:
        ce = nll.mean()
        return torch.stack([ce + dice_loss, ce, dice_loss]).tolist()
    focal = ((1 - (p * onehot).sum(1)) ** 2 * nll).mean()
    tversky = 1 - ((inter + 1e-5) / (inter + 0.3 * (tsum - inter) + 0.7 * (psum - inter) + 1e-5))[:, 1:].mean()
    return torch.stack([0.4 * focal + 0.4 * tversky + 0.2 * dice_loss, focal, tversky, dice_loss]).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--inputs", default="", help="comma list out of square,wide (default: both)")
    ap.add_argument("--trace", action="store_true", help="only the entry, for a run under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, loss as ls, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
              "workgroup_span": ls.layout(), "rows": []}
    print(result["version"])

    shapes = {"square": (16, 512, 512, 3), "wide": (32, 448, 800, 7)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W, C) in shapes.items():
        model = NestedUNet(C, deep_supervision=True, max_batch=B, max_hw=(H, W)).to("cuda:0")
        model.load_state_dict(syn.make_state_dict(C, 3, True, 2), strict=True)
        model.eval()
        four_l, four_t = ls.make_logits(4, C, H, W, 1), ls.make_target(4, C, H, W, 1)
        logits_np = np.concatenate([four_l] * (B // 4))
        target_np = np.concatenate([four_t] * (B // 4))
        logits, target = torch.from_numpy(logits_np).cuda(), torch.from_numpy(target_np).cuda()
        row = {"input": name, "batch": B, "h": H, "w": W, "num_classes": C, "kernel_bytes": B * H * W * (4 * C + 1)}
        t = lambda fn: timed(torch, fn, args.iters, args.warmup)
        table, outside = ls._rows(torch, B, C, logits.device)
        model._input(target, "target")                              # makes the engine: the entry is called directly
        entry = lambda g=2: model._call("unetpp_loss_sums_f32", logits, target, B, C, H, W, g, table, outside, stream_of=logits)
        if args.trace:
            row["entry_us"] = t(entry)
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            continue
        want = ls.loss_sums_np(four_l, four_t)
        got = ls.loss_sums(model, logits, target)
        assert np.array_equal(got[0][:4].cpu().numpy().view(np.uint64), want[0]) and not got[1].any().item(), "device and host differ"
        comb, adv = ls.combined_loss(model, logits, target), ls.advanced_combined_loss(model, logits, target)
        tc, ta = torch_losses(torch, logits, target, False), torch_losses(torch, logits, target, True)
        row["combined"], row["torch_combined"], row["advanced"], row["torch_advanced"] = comb, tc, adv, ta
        assert np.allclose(comb, tc, rtol=1e-4) and np.allclose(adv, ta, rtol=1e-4), (comb, tc, adv, ta)
        row["entry_us"] = t(entry)
        row["entry_gamma0_us"] = t(lambda: entry(0))
        row["entry_share_of_hbm"] = round(row["kernel_bytes"] / row["entry_us"] / HBM_BYTES_PER_US, 3)
        row["loss_sums_us"] = t(lambda: ls.loss_sums(model, logits, target))
        row["combined_loss_us"] = t(lambda: ls.combined_loss(model, logits, target))
        row["advanced_loss_us"] = t(lambda: ls.advanced_combined_loss(model, logits, target))
        row["torch_combined_us"] = t(lambda: torch_losses(torch, logits, target, False))
        row["torch_advanced_us"] = t(lambda: torch_losses(torch, logits, target, True))
        row["torch_over_combined"] = round(row["torch_combined_us"] / row["combined_loss_us"], 1)
        row["torch_over_advanced"] = round(row["torch_advanced_us"] / row["advanced_loss_us"], 1)
        x = torch.from_numpy(syn.make_frames_u8(B, H, W, "smooth", 7)).cuda()
        row["segment_us"] = t(lambda: model.segment(x))
        for k in ("entry_us", "combined_loss_us", "advanced_loss_us", "torch_combined_us"):
            row[k.replace("_us", "_over_segment")] = round(row[k] / row["segment_us"], 4)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        del model

    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if not args.trace:
        print(json.dumps({"metric": "combined_loss_us", "rows": [(r["input"], r["entry_us"], r["combined_loss_us"], r["torch_combined_us"]) for r in result["rows"]]}))


if __name__ == "__main__":
    main()
