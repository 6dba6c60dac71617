#!/usr/bin/env python3
"""Loss gradients on the device: forward + backward of the criteria of unet_amd/loss_grad.py against the same criteria in
plain torch ops with autograd, the gradient kernel alone, and the memory both routes take.

B = 16 logit maps of 512 x 512 with C = 3 and B = 32 of 448 x 800 with C = 7 (the scenes of scripts/loss_bench.py): device
events around `--iters` calls after `--warmup` calls, three loops; every time is the median with the fastest and the slowest
loop beside it.  Per workload:
  module_combined_us / module_advanced_us   (a) criterion(pred, target) + loss.backward() with our modules, uint8 target
  module_advanced_i64_us                        the same with the reference's int64 target (one more launch: the narrowing)
  torch_combined_us / torch_advanced_us     (b) the same criteria (defaults) in plain torch ops + .backward(): the route
                                                without this module (the ops scripts/loss_bench.py times, with autograd)
  torch_over_module_*                           the ratios (b) / (a)
  grad_entry_us                             (c) unetpp_loss_grad_f32 alone into a preallocated gradient, gamma 2, with a scale
  sums_entry_us, grad_over_sums                 unetpp_loss_sums_f32 on the same input, and the ratio
  grad_bytes, grad_gb_s, grad_share_of_hbm  (d) B H W (8 C + 1) bytes (logits read, gradient written, target read) over
                                                grad_entry_us, and as a fraction of 6.3 TB/s
  module_*_peak_mb / torch_*_peak_mb        (e) torch.cuda.max_memory_allocated over one forward + backward, above what was
                                                allocated before it (logits, target and pred.grad's predecessor excluded)
The gradients of (a) and (b) are compared before anything is timed (5e-6 of the largest gradient).

    python scripts/loss_grad_bench.py [--iters 200] [--warmup 3] [--json OUT.json] [--out OUT.txt] [--inputs square]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_timing import timed_spread  # noqa: E402
HBM_BYTES_PER_US = 6.3e6                                        # 6.3 TB/s


def torch_criterion(torch, logits, target, advanced):
    """CombinedLoss / AdvancedCombinedLoss with their defaults in plain torch ops (scripts/loss_bench.py's), differentiable:
    the stacked (loss, parts...) tensor."""
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
        return torch.stack([ce + dice_loss, ce, dice_loss])
    focal = ((1 - (p * onehot).sum(1)) ** 2 * nll).mean()
    tversky = 1 - ((inter + 1e-5) / (inter + 0.3 * (tsum - inter) + 0.7 * (psum - inter) + 1e-5))[:, 1:].mean()
    return torch.stack([0.4 * focal + 0.4 * tversky + 0.2 * dice_loss, focal, tversky, dice_loss])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--out", default="", help="also write the printed lines to this text file")
    ap.add_argument("--inputs", default="", help="comma list out of square,wide (default: both)")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, loss as ls, loss_grad as lg
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
              "workgroup_span": lg.layout(), "rows": []}
    lines = [result["version"]]
    print(lines[0], flush=True)

    shapes = {"square": (16, 512, 512, 3), "wide": (32, 448, 800, 7)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    for name, (B, H, W, C) in shapes.items():
        model = NestedUNet(C, max_batch=1, max_hw=(16, 16)).to("cuda:0")          # no weights: the criteria need none
        four_l, four_t = ls.make_logits(4, C, H, W, 1), ls.make_target(4, C, H, W, 1)
        logits = torch.from_numpy(np.concatenate([four_l] * (B // 4))).cuda()
        target = torch.from_numpy(np.concatenate([four_t] * (B // 4))).cuda()
        target64 = target.long()
        row = {"input": name, "batch": B, "h": H, "w": W, "num_classes": C, "grad_bytes": B * H * W * (8 * C + 1)}
        t = lambda fn: timed_spread(torch, fn, args.iters, args.warmup)
        pred = logits.clone().requires_grad_()
        modules = {"combined": lg.CombinedLoss(model), "advanced": lg.AdvancedCombinedLoss(model)}

        def ours(kind, tgt=target):
            pred.grad = None
            out = modules[kind](pred, tgt)
            out[0].backward()
            return out

        def plain(kind):
            pred.grad = None
            out = torch_criterion(torch, pred, target, kind == "advanced")
            out[0].backward()
            return out.tolist()

        for kind in modules:                                          # the two routes agree before anything is timed
            a = ours(kind)
            ga = pred.grad.clone()
            b = plain(kind)
            gmax = float(ga.abs().max())
            diff = float((pred.grad - ga).abs().max())
            assert diff <= 5e-6 * gmax and np.allclose([a[0].item()] + list(a[1:]), b, rtol=1e-4), (kind, diff, gmax, a, b)
            row[f"{kind}_max_grad"], row[f"{kind}_torch_diff_over_max"] = gmax, round(diff / gmax, 9)
        del ga
        for kind in modules:
            row[f"module_{kind}_us"] = t(lambda: ours(kind))
        row["module_advanced_i64_us"] = t(lambda: ours("advanced", target64))
        for kind in modules:
            row[f"torch_{kind}_us"] = t(lambda: plain(kind))
            row[f"torch_over_module_{kind}"] = round(row[f"torch_{kind}_us"][0] / row[f"module_{kind}_us"][0], 2)
        # (c), (d): the entries alone
        table, outside = ls._rows(torch, B, C, logits.device)
        ls.loss_sums(model, logits, target, 2, out=(table, outside))
        tb, _ = ls._read_back(torch, table, outside)
        coef = torch.from_numpy(lg.coefficients_from_sums(tb, H * W, "advanced")).cuda()
        scale = torch.full((1,), 0.5, dtype=torch.float32, device="cuda")
        grad = torch.empty_like(logits)
        row["grad_entry_us"] = t(lambda: model._call("unetpp_loss_grad_f32", logits, target, B, C, H, W, 2, coef, scale, grad, stream_of=logits))
        row["sums_entry_us"] = t(lambda: model._call("unetpp_loss_sums_f32", logits, target, B, C, H, W, 2, table, outside, stream_of=logits))
        row["grad_over_sums"] = round(row["grad_entry_us"][0] / row["sums_entry_us"][0], 2)
        row["grad_gb_s"] = round(row["grad_bytes"] / row["grad_entry_us"][0] / 1e3, 1)
        row["grad_share_of_hbm"] = round(row["grad_bytes"] / row["grad_entry_us"][0] / HBM_BYTES_PER_US, 3)
        del grad
        # (e): peak memory of one forward + backward above what was there before
        for label, fn in (("module", ours), ("torch", plain)):
            for kind in modules:
                pred.grad = None
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn(kind)
                torch.cuda.synchronize()
                row[f"{label}_{kind}_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        row["logits_mb"] = round(logits.numel() * 4 / 2 ** 20, 1)
        result["rows"].append(row)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del model, pred, logits, target, target64
        torch.cuda.empty_cache()

    lines.append(json.dumps({"metric": "module_advanced_us", "rows": [(r["input"], r["module_advanced_us"][0], r["torch_advanced_us"][0],
                                                                      r["grad_entry_us"][0], r["grad_share_of_hbm"]) for r in result["rows"]]}))
    print(lines[-1])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
