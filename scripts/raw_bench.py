#!/usr/bin/env python3
"""Raw camera frames on the device: the demosaic fused into the resize against the routes that start from a BGR frame, and the
demosaic alone against its memory traffic.

Workloads: B = 4 raw frames of 1080 x 1920 and B = 16 of 512 x 512, BayerRG8 (the reference's default), resized to the network's
512 x 512.  Frames are raw_frames.make_raw scenes.  Device events around `--iters` calls after `--warmup` calls, median of three
loops; the end-to-end rows are wall clock.  Per workload:
  (a) fused_us            raw_frames.resize: one launch from 1 B/px of raw bytes to the network's input
      parent_resize_us    the parent commit's route on the device: resize_frames on a BGR frame ALREADY there (reads 3 B/px; the
                          demosaic ran on the host and is not in this figure).  fused_over_parent = fused_us / parent_resize_us
  (b) unfused_us          raw_frames.to_bgr + resize_frames: the same result in two launches through a full-size BGR frame
  (c) e2e_raw_wall_us     pinned host raw frames -> upload (1 B/px) -> frame_loop.process_raw_frames
      e2e_bgr_wall_us     pinned host BGR frames -> upload (3 B/px) -> frame_loop.process_frames (the parent's loop; the host's
                          cv2.cvtColor is NOT included).  At 512 x 512 process_frames skips its resize, the raw loop cannot.
  (d) to_bgr_us / to_bgr_gbs        the demosaic alone against its 4 B/px (1 read, 3 written)
      to_gray_us / to_gray_gbs      the grey-only form against its 2 B/px
      to_both_us                    BGR and grey in one launch (5 B/px)
  segment_us              segment() of the same batch at 512 x 512 in `exact`, for scale
No bar is fixed: nothing of this was measured before.  A fused launch slower than (a) is a finding to write down.  Before timing,
every device result is compared with the NumPy form on a small batch and the fused launch with the unfused route on the workload
itself.  Not measured: hardware counters, the misaligned (byte) paths, padded rows, the other patterns.

    python scripts/raw_bench.py [--iters 20] [--warmup 5] [--out FILE] [--inputs full_hd,square]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_timing import timed, wall  # noqa: E402

S = 512
FORMAT = "BayerRG8"


def check_small(torch, model, rf):
    raw = rf.make_raw(2, 37, 53, 0)
    dev = torch.from_numpy(raw).cuda()
    for pattern in rf.PATTERNS:
        bgr, gray = rf.to_bgr(model, dev, pattern=pattern, want_gray=True)
        assert np.array_equal(bgr.cpu().numpy(), rf.demosaic_np(raw, pattern)) and np.array_equal(gray.cpu().numpy(), rf.gray_np(raw, pattern)), pattern
        got = rf.resize(model, dev, pattern, (16, 24), (5, 3, 40, 31))
        assert np.array_equal(got.cpu().numpy(), rf.raw_resize_np(raw, pattern, (5, 3, 40, 31), (16, 24))), pattern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="default: profiles/raw_<source hash>_bench.txt")
    ap.add_argument("--inputs", default="", help="comma list out of full_hd,square (default: both)")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, frame_loop, raw_frames as rf, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    out_path = args.out or os.path.join(ROOT, "profiles", f"raw_{_lib.source_hash()}_bench.txt")
    lines = [json.dumps({"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
                         "pixel_format": FORMAT})]
    print(lines[0])

    shapes = {"full_hd": (4, 1080, 1920), "square": (16, 512, 512)}
    if args.inputs:
        shapes = {k: shapes[k] for k in args.inputs.split(",")}
    pattern = rf.pattern_of(FORMAT)
    for name, (B, H, W) in shapes.items():
        model = NestedUNet(3, deep_supervision=False, max_batch=B, max_hw=(S, S)).to("cuda:0")
        model.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
        model.eval()
        check_small(torch, model, rf)
        raw_np = rf.make_raw(B, H, W, 3)
        raw = torch.from_numpy(raw_np).cuda()
        bgr = rf.to_bgr(model, raw, FORMAT)
        fused = rf.resize(model, raw, pattern, (S, S))
        assert torch.equal(fused, model.resize_frames(bgr, (S, S))), "the fused launch and resize_frames(to_bgr(raw)) differ"
        t = lambda fn: timed(torch, fn, args.iters, args.warmup)
        px = B * H * W
        row = {"input": name, "batch": B, "h": H, "w": W, "model_size": S}
        row["fused_us"] = t(lambda: rf.resize(model, raw, pattern, (S, S)))
        row["parent_resize_us"] = t(lambda: model.resize_frames(bgr, (S, S)))
        row["fused_over_parent"] = round(row["fused_us"] / row["parent_resize_us"], 3)
        row["unfused_us"] = t(lambda: model.resize_frames(rf.to_bgr(model, raw, FORMAT), (S, S)))
        row["fused_over_unfused"] = round(row["fused_us"] / row["unfused_us"], 3)
        row["to_bgr_us"] = t(lambda: rf.to_bgr(model, raw, FORMAT))
        row["to_bgr_gbs"] = round(4 * px / row["to_bgr_us"] / 1e3, 1)
        row["to_gray_us"] = t(lambda: rf.to_gray(model, raw, FORMAT))
        row["to_gray_gbs"] = round(2 * px / row["to_gray_us"] / 1e3, 1)
        row["to_both_us"] = t(lambda: rf.to_bgr(model, raw, FORMAT, want_gray=True))
        x = torch.from_numpy(syn.make_frames_u8(B, S, S, "smooth", 7)).cuda()
        row["segment_us"] = t(lambda: model.segment(x))

        host_raw = torch.from_numpy(raw_np).pin_memory()
        host_bgr = bgr.cpu().pin_memory()
        want = frame_loop.process_frames(model, host_bgr, target_size=(S, S))
        got = frame_loop.process_raw_frames(model, host_raw, FORMAT, target_size=(S, S))
        assert all(torch.equal(a, b) for a, b in zip(got, want)), "process_raw_frames and process_frames differ"
        loop_iters, loop_warm = max(args.iters // 2, 2), 2
        row["e2e_raw_wall_us"] = wall(torch, lambda: frame_loop.process_raw_frames(model, host_raw, FORMAT, target_size=(S, S)), loop_iters, loop_warm)
        row["e2e_bgr_wall_us"] = wall(torch, lambda: frame_loop.process_frames(model, host_bgr, target_size=(S, S)), loop_iters, loop_warm)
        row["e2e_raw_over_bgr"] = round(row["e2e_raw_wall_us"] / row["e2e_bgr_wall_us"], 3)
        row["e2e_raw_frames_per_s"] = round(B * 1e6 / row["e2e_raw_wall_us"], 1)
        row["e2e_bgr_frames_per_s"] = round(B * 1e6 / row["e2e_bgr_wall_us"], 1)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del model

    lines.append("not measured: hardware counters, the misaligned (byte) paths, padded rows, the patterns other than RG, the host's cv2.cvtColor")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
