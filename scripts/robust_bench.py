#!/usr/bin/env python3
"""The robust loop's mask rules on the device: time per call against the network.

B = 16 at 512 x 512 and B = 4 at 1080 x 1920, each with four kinds of masks: `scene` (unet_amd.robust.make_robust_scene,
four distinct scenes repeated to the batch; at 1080 x 1920 the 1080 x 1080 scene in the middle of the frame), `nonzero` (an
empty cable: the transform of `cable == 0` has no zero pixel and takes its way out), `zero` (a cable that covers the
frame: every pixel is a zero pixel) and `corner` (one cable pixel in a corner: every other pixel searches all the way to
that column, the float map's worst case).  Timed with the method of scripts/geometry_bench.py: device events around
`--iters` calls after `--warmup` calls, median of three loops.  Per row:
  distance_us          distance_transform(cable, invert=True): the float32 map
  ring_us              distance_ring(cable, tape, 2, 20): the fused ring alone (no map written; the search ends beyond 20)
  morph_ring_us        the parent's ring built from morphology: the one launch of constrain_tape_to_ring (dilate E15, erode E5)
  constrain_tape_us    constrain_tape_to_ring itself (that launch and its largest-component filter)
  postprocess_us       postprocess_robust with the call-site constants (check=False: nothing read back)
  measure_us           measure_robust (two launches and its one read-back)
and per shape, on `scene` only: segment_us (segment() of a batch of that many frames at 512 x 512, `exact`) and
process_frames_robust_us (letterbox, segment_thresholded, unletterbox, post, measure on raw frames of the shape).

    python scripts/robust_bench.py [--iters 20] [--warmup 5] [--out profiles/robust_<source hash>_bench.txt]
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


def scene(H, W, seed, rb, **opts):
    """make_robust_scene; on a landscape frame the H x H scene in the middle of the frame, so that the cable keeps the
    upright shape the call-site constants of keep_best_cable_cc ask for (aspect >= 3)."""
    side = min(H, W)
    c, t = rb.make_robust_scene(H, side, seed, sway=0.005, **opts)
    left = (W - side) // 2
    return tuple(np.pad(m, ((0, 0), (left, W - side - left))) for m in (c, t))


def masks_of(kind, B, H, W, rb):
    if kind == "scene":
        pairs = [scene(H, W, seed, rb, second=(0.45, 0.1)) for seed in range(4)]
        return np.stack([pairs[i % 4][0] for i in range(B)]), np.stack([pairs[i % 4][1] for i in range(B)])
    tape = np.stack([scene(H, W, seed, rb)[1] for seed in range(2)] * (B // 2))
    cable = np.zeros((B, H, W), np.uint8)
    if kind == "zero":
        cable[:] = 1
    elif kind == "corner":
        cable[:, H - 1, 0] = 1
    return cable, tape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, frame_loop, morphology as mo, robust as rb, synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    out = args.out or os.path.join(ROOT, "profiles", f"robust_{_lib.source_hash()}_bench.txt")
    lines = [lib.unetpp_version().decode(), f"iters {args.iters} warmup {args.warmup}: microseconds per call, median of three loops"]
    print(lines[0])
    model = NestedUNet(3, deep_supervision=False, max_batch=16, max_hw=(512, 512)).to("cuda:0")
    model.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    model.eval()
    ring_program = model._morph_named("ring", (15, 5), mo.program_ring)

    for B, H, W in ((16, 512, 512), (4, 1080, 1920)):
        seg_us = None
        for kind in ("scene", "nonzero", "zero", "corner"):
            c, t = masks_of(kind, B, H, W, rb)
            cable, tape = torch.from_numpy(c).cuda(), torch.from_numpy(t).cuda()
            row = {"batch": B, "h": H, "w": W, "masks": kind}
            row["distance_us"] = timed(torch, lambda: rb.distance_transform(model, cable, invert=True), args.iters, args.warmup)
            row["ring_us"] = timed(torch, lambda: rb.distance_ring(model, cable, tape, 2, 20), args.iters, args.warmup)
            row["morph_ring_us"] = timed(torch, lambda: model._morph_launch(ring_program, tape, -1, cable, -1, 1), args.iters, args.warmup)
            row["constrain_tape_us"] = timed(torch, lambda: model.constrain_tape_to_ring(tape, cable, check=False), args.iters, args.warmup)
            row["postprocess_us"] = timed(torch, lambda: rb.postprocess_robust(model, cable, tape, check=False), args.iters, args.warmup)
            pc, pt = rb.postprocess_robust(model, cable, tape, check=False)
            row["measure_us"] = timed(torch, lambda: rb.measure_robust(model, pc, pt), args.iters, args.warmup)
            row["kept"] = [int(pc.count_nonzero()), int(pt.count_nonzero())]
            if kind == "scene":
                frames = np.stack([syn.make_frame_u8(H, W, i, ("smooth", "uniform")[i % 2], 1234) for i in range(B)])
                raw = torch.from_numpy(frames).cuda()
                small = raw if (H, W) == (512, 512) else rb.letterbox(model, raw, 512)[0]
                seg_us = row["segment_us"] = timed(torch, lambda: model.segment(small), args.iters, args.warmup)
                row["process_frames_robust_us"] = timed(torch, lambda: frame_loop.process_frames_robust(model, raw, 512, check=False),
                                                        args.iters, args.warmup)
                row["loop_over_segment"] = round(row["process_frames_robust_us"] / seg_us, 3)
            row["post_and_measure_over_segment"] = round((row["postprocess_us"] + row["measure_us"]) / seg_us, 3)
            row["distance_over_segment"] = round(row["distance_us"] / seg_us, 3)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)

    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
