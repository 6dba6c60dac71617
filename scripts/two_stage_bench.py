#!/usr/bin/env python3
"""The two-stage loop on the device: its new launches against the routes they replace, and FrameStream against sequential calls.

    python scripts/two_stage_bench.py [--step overlay|class_masks|loop|stream] [--inputs square,hd] [--iters 20] [--warmup 5]

Workloads: B = 16 frames of 512 x 512 ("square") and B = 4 of 1080 x 1920 ("hd"), scenes of unet_amd.two_stage.make_scene.
Every figure is the median of three timed loops, printed with the smallest and the largest of the three (the spread); device
times are events around --iters calls, frame rates are wall-clock over --batches batches with a synchronise at the end.
  overlay      two_stage.overlay against contours.create_overlay_masks (the parent's kernel: the same 9 bytes per pixel through the
               same kind of table) on the same buffers, and against the same chain in torch ops; GB/s of 9 B/px
  class_masks  two_stage.class_masks against two resize_masks launches plus mask_stats of each mask (the parent's route)
  loop         process_frames_two_stage (check=False) as a multiple of segment() of the same batch, and the host route its
               overlay replaces: .cpu() of the frames and three masks, then overlay_np on one thread (timed on two frames)
  stream       frames/s from pinned host frames: sequential process_frames / process_raw_frames (upload, call, synchronise; with and
               without the download of the two masks), FrameStream with one slot and with two, and the resident rate (frames
               already on the device) as the ceiling
Run one --step per process, each under its own time limit.  Not measured here: counters, per-kernel times, the misaligned byte
paths (tests/test_gpu_guarded_two_stage.py runs those)."""
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
SHAPES = {"square": (16, 512, 512), "hd": (4, 1080, 1920)}


def spread(loops):
    return {"median": round(statistics.median(loops), 2), "min": round(min(loops), 2), "max": round(max(loops), 2)}


def timed_us(torch, fn, iters, warmup):
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
    return spread(loops)


def rate_fps(torch, run, n_frames, warmup_runs=1):
    """run() processes n_frames frames and returns when they are done: frames/s, median of three with the spread."""
    for _ in range(warmup_runs):
        run()
    loops = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        loops.append(n_frames / (time.perf_counter() - t0))
    return spread(loops)


def scene_batch(ts, b, h, w):
    parts = [ts.make_scene(h, w, seed) for seed in range(min(b, 4))]
    stack = lambda i: np.stack([parts[k % len(parts)][i] for k in range(b)])
    return stack(0), stack(1), stack(2), stack(3), parts[0][4]


def make_model(torch, b):
    from unet_amd import synthetic as syn
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=False, max_batch=b, max_hw=(512, 512)).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    return m.eval()


def step_overlay(torch, args, name, shape, emit):
    from unet_amd import contours as ct, two_stage as ts
    b, h, w = shape
    model = make_model(torch, 1)
    frames, cable, tape, burr, roi = (torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) else a for a in scene_batch(ts, b, h, w))
    gb = 9.0 * b * h * w / 1e9
    new = timed_us(torch, lambda: ts.overlay(model, frames, cable, tape, burr, roi), args.iters, args.warmup)
    old = timed_us(torch, lambda: ct.create_overlay_masks(model, frames, cable, tape, burr), args.iters, args.warmup)
    x1, y1, x2, y2 = roi
    cols = [torch.tensor(ts.CLASS_COLORS[c], dtype=torch.float32, device="cuda") for c in (1, 2, 3)]

    def torch_chain():
        f = frames.float()
        dim = torch.zeros_like(f)
        dim[:, y1:y2, x1:x2] = f[:, y1:y2, x1:x2]
        r = torch.round(f * 0.7 + dim * 0.3).clamp_(0, 255)
        for m, col, (a_, b_) in zip((cable, tape, burr), cols, ts.WEIGHTS[1:]):
            r = torch.round(r * a_ + (m > 0)[..., None] * col * b_).clamp_(0, 255)
        return r.to(torch.uint8)
    same = bool(torch.equal(torch_chain(), ts.overlay(model, frames, cable, tape, burr, roi)[0]))
    plain = timed_us(torch, torch_chain, max(args.iters // 4, 3), 2)
    emit({"step": "overlay", "input": name, "shape": shape, "two_stage_overlay_us": new, "parent_overlay_chain_us": old, "torch_ops_us": plain,
          "torch_ops_equal": same, "two_stage_overlay_GBps": round(gb / (new["median"] * 1e-6), 1), "parent_overlay_chain_GBps": round(gb / (old["median"] * 1e-6), 1)})


def step_class_masks(torch, args, name, shape, emit):
    from unet_amd import two_stage as ts
    b, h, w = shape
    model = make_model(torch, 1)
    pred = torch.from_numpy(np.random.default_rng(0).integers(0, 3, (b, 512, 512), dtype=np.uint8)).cuda()
    from unet_amd import frame_loop
    roi = frame_loop.map_roi_to_original((w, h), (512, 512))

    def parent():
        c = model.resize_masks(pred, (w, h), match_class=1, roi=roi)
        t = model.resize_masks(pred, (w, h), match_class=2, roi=roi)
        return c, t, model.mask_stats(c)[0], model.mask_stats(t)[0]

    def parent_masks_only():
        return model.resize_masks(pred, (w, h), match_class=1, roi=roi), model.resize_masks(pred, (w, h), match_class=2, roi=roi)
    new = timed_us(torch, lambda: ts.class_masks(model, pred, (w, h), roi), args.iters, args.warmup)
    old = timed_us(torch, parent, args.iters, args.warmup)
    old2 = timed_us(torch, parent_masks_only, args.iters, args.warmup)
    emit({"step": "class_masks", "input": name, "shape": shape, "class_masks_us": new, "parent_two_resize_plus_mask_stats_us": old,
          "parent_two_resize_only_us": old2})


def step_loop(torch, args, name, shape, emit):
    from unet_amd import frame_loop, two_stage as ts
    b, h, w = shape
    model = make_model(torch, b)
    frames_np = scene_batch(ts, b, h, w)[0]
    frames = torch.from_numpy(frames_np).cuda()
    small = frames if (h, w) == (512, 512) else model.resize_frames(frames, (512, 512))
    seg = timed_us(torch, lambda: model.segment(small), args.iters, args.warmup)
    loop = timed_us(torch, lambda: frame_loop.process_frames_two_stage(model, frames, check=False), args.iters, args.warmup)
    bare = timed_us(torch, lambda: frame_loop.process_frames_two_stage(model, frames, check=False, want_overlay=False), args.iters, args.warmup)
    res = frame_loop.process_frames_two_stage(model, frames, check=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = [v.cpu().numpy() for v in (frames, res.mask_cable, res.mask_tape, res.mask_burr)]
    t1 = time.perf_counter()
    k = min(2, b)
    ts.overlay_np(host[0][:k], host[1][:k], host[2][:k], host[3][:k], res.roi)
    t2 = time.perf_counter()
    emit({"step": "loop", "input": name, "shape": shape, "segment_us": seg, "process_frames_two_stage_us": loop, "without_overlay_us": bare,
          "loop_over_segment": round(loop["median"] / seg["median"], 3), "counts_frame0": res.counts[0].tolist(),
          "host_route": {"d2h_us": round((t1 - t0) * 1e6), "overlay_np_us_per_frame": round((t2 - t1) * 1e6 / k), "frames_timed": k}})


def step_stream(torch, args, name, shape, emit):
    from unet_amd import frame_loop, raw_frames as rf, two_stage as ts
    from unet_amd.stream import FrameStream
    b, h, w = shape
    models = [make_model(torch, b), make_model(torch, b)]
    n = args.batches
    bgr = [np.ascontiguousarray(np.roll(scene_batch(ts, b, h, w)[0], i, axis=2)) for i in range(2)]
    raw = [rf.make_raw(b, h, w, i) for i in range(2)]
    pinned = {"bgr": [torch.from_numpy(a).pin_memory() for a in bgr], "raw": [torch.from_numpy(a).pin_memory() for a in raw]}
    fns = {"bgr": lambda m, x: frame_loop.process_frames(m, x), "raw": lambda m, x: frame_loop.process_raw_frames(m, x, "BayerRG8")}
    row = {"step": "stream", "input": name, "shape": shape, "batches": n}
    for kind in ("bgr", "raw"):
        fn, host, src = fns[kind], pinned[kind], (bgr if kind == "bgr" else raw)
        outs = [torch.empty((b, h, w), dtype=torch.uint8).pin_memory() for _ in range(2)]

        def sequential(download):
            for i in range(n):
                x = host[i % 2].to("cuda:0", non_blocking=True)
                r = fn(models[0], x)
                if download:
                    outs[0].copy_(r[1], non_blocking=True)
                    outs[1].copy_(r[2], non_blocking=True)
                torch.cuda.synchronize()
        resident = [h_.cuda() for h_ in host]

        def on_device():
            for i in range(n):
                fn(models[0], resident[i % 2])
            torch.cuda.synchronize()
        row[kind] = {"sequential_fps": rate_fps(torch, lambda: sequential(False), n * b),
                     "sequential_with_download_fps": rate_fps(torch, lambda: sequential(True), n * b),
                     "resident_fps": rate_fps(torch, on_device, n * b)}
        for slots in (1, 2):
            fs = FrameStream(models[:slots], fn, outputs=(1, 2))

            def streamed():
                for _ in fs.map(src[i % 2] for i in range(n)):
                    pass
            row[kind][f"frame_stream_{slots}_slot_fps"] = rate_fps(torch, streamed, n * b)
    for slots in (1, 2):
        fs = FrameStream(models[:slots], lambda m, x: frame_loop.process_frames_two_stage(m, x, check=False), outputs=("result", "counts"))

        def streamed():
            for _ in fs.map(bgr[i % 2] for i in range(n)):
                pass
        row[f"two_stage_frame_stream_{slots}_slot_fps"] = rate_fps(torch, streamed, n * b)
    emit(row)


STEPS = {"overlay": step_overlay, "class_masks": step_class_masks, "loop": step_loop, "stream": step_stream}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="one of %s (default: all, in one process)" % ", ".join(STEPS))
    ap.add_argument("--inputs", default="", help="comma list out of square,hd (default: both)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=24, help="batches per timed loop of the stream step")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib
    lib = _lib.load()
    print(json.dumps({"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    shapes = {k: SHAPES[k] for k in (args.inputs.split(",") if args.inputs else SHAPES)}
    for step in ([args.step] if args.step else list(STEPS)):
        for name, shape in shapes.items():
            STEPS[step](torch, args, name, shape, lambda row: print(json.dumps(row), flush=True))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
