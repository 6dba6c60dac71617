#!/usr/bin/env python3
"""Training batches on the device: one unetpp_train_batch_u8 launch per batch (unet_amd/train_batch.py) against the route the
engine offered before it and against the NumPy forms on one host thread.

Two workloads, B = 16, resident uint8 sources (four seeded images repeated):
  cable   1080 x 1920 -> 512 x 512, CableDefectDataset with augmentation (flips after the resize, the brightness step for the
          samples that draw it), the 7 -> 3 class map: the shape of the 3-class trainers
  patch   448 x 800 sources, 384 x 384 crops -> 256 x 256 (tools/train_binary_patch.py's patch_size / target_size), fliplr /
          flipud / rot90 before the resize, convertScaleAbs as a table, the binary defect target
Device events around `--iters` calls after `--warmup` calls, three loops; every time is the median with the fastest and the
slowest loop beside it.  Per workload:
  batch_us                 make_batch (two small uploads and ONE launch), float32 [B,3,H,W] + uint8 target
  batch_hwc_us             the same with image_format="hwc_u8" (what segment() / evaluate_batches take)
  batch_plain_us           make_batch without the brightness step: the work the device route below does
  entry_us                 unetpp_train_batch_u8 alone, tables already on the device
  entry_bytes, entry_gb_s, entry_share_of_hbm   per output pixel 12 tap bytes + 1 mask byte read and 12 + 1 written, over
                           entry_us, and as a fraction of 6.3 TB/s
  crop_rects_us            (cable only) unetpp_train_crop_rects for the batch: 16 workgroups, each reads its whole mask
  device_route_us          the route the engine had before: resize_frames + resize_masks (cable: the whole frames; patch: torch
                           slices, flips, rot90 and table indexing per sample first), then torch flips, the class table by
                           indexing, permute and / 255.  It has NO brightness step (the engine had no colour conversion): compare
                           it with batch_plain_us.  routes_equal: its tensors equal make_batch's bit for bit (checked first).
  device_over_batch        device_route_us / batch_plain_us
  host_ms, host_over_batch assemble_np on one host thread plus the upload of the float tensor and the target (what a loader
                           worker does), median of three runs, and its ratio to batch_us
  batch_peak_mb / device_route_peak_mb   torch.cuda.max_memory_allocated over one call above the resident set

    python scripts/train_batch_bench.py [--iters 50] [--warmup 3] [--json OUT.json] [--out OUT.txt] [--inputs cable,patch]
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
from bench_timing import timed_spread  # noqa: E402
HBM_BYTES_PER_US = 6.3e6                                        # 6.3 TB/s
MAP_3CLASS = {0: 0, 1: 1, 2: 2, 3: 0, 4: 0, 5: 0, 6: 0}


def sources(h, w, n, distinct=4):
    r = np.random.default_rng(h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    images, masks = [], []
    for i in range(distinct):
        base = np.stack([60 + 120 * xx / w, 200 - 100 * yy / h, 90 + 60 * np.sin((xx + yy) / (40.0 + i))], -1)
        images.append(np.clip(base + r.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8))
        m = np.zeros((h, w), np.uint8)
        m[h // 4:3 * h // 4, :] = 1
        m[h // 4:3 * h // 4, w // 3 + 20 * i:w // 3 + 20 * i + w // 8] = 2
        if i % 2 == 0:                                          # every second source has a defect, the others are 'normal' samples
            m[h // 2:h // 2 + 12, w // 2 + 30 * i:w // 2 + 30 * i + 25] = 3 + i % 3
        masks.append(m)
    return [images[i % distinct] for i in range(n)], [masks[i % distinct] for i in range(n)]


def peak(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--out", default="", help="also write the printed lines to this text file")
    ap.add_argument("--inputs", default="", help="comma list out of cable,patch (default: both)")
    args = ap.parse_args()

    import torch
    from unet_amd import _lib, train_batch as tb
    from unet_amd.nested_unet import NestedUNet
    lib = _lib.load()
    result = {"version": lib.unetpp_version().decode(), "source_hash": _lib.source_hash(), "iters": args.iters, "warmup": args.warmup,
              "layout": tb.layout(), "rows": []}
    lines = [result["version"]]
    print(lines[0], flush=True)
    model = NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")              # no weights: the batches need none
    B = 16
    t = lambda fn: timed_spread(torch, fn, args.iters, args.warmup)
    for name in (args.inputs.split(",") if args.inputs else ["cable", "patch"]):
        r = np.random.RandomState(7)
        if name == "cable":
            (h, w), (oh, ow) = (1080, 1920), (512, 512)
            images, masks = sources(h, w, B)
            ts = tb.TrainSet(model, images, masks)
            kws = [tb.draw_cable_defect(r)[0] for _ in range(B)]
            samples = [tb.sample(i, **kw) for i, kw in enumerate(kws)]
            plain = [tb.sample(i, **dict(kw, value_lut=None)) for i, kw in enumerate(kws)]
            ctab = tb.class_lut(MAP_3CLASS, "zero")
        else:
            import random
            (h, w), (oh, ow), ps = (448, 800), (256, 256), 384
            images, masks = sources(h, w, B)
            ts = tb.TrainSet(model, images, masks)
            rng = random.Random(7)
            samples = [tb.draw_patch(rng, "defect" if i % 2 == 0 else "normal", ps, ts.sizes, ts.defect_items, ts.bboxes, ts.normal_items) for i in range(B)]
            plain = samples
            ctab = tb.binary_defect_lut()
        plan, luts = tb.build_plan(samples, ts.sizes)
        plan_p, luts_p = tb.build_plan(plain, ts.sizes)
        row = {"input": name, "batch": B, "source_hw": [h, w], "out_hw": [oh, ow], "entry_bytes": B * oh * ow * (13 + 13),
               "resident_mb": round((ts.images.numel() + ts.masks.numel()) / 2 ** 20, 1),
               "brightness_samples": int((plan[:, tb.P_VALUE_LUT] >= 0).sum()), "byte_lut_samples": int((plan[:, tb.P_BYTE_LUT] >= 0).sum())}

        # ---- the route the engine had before: resize kernels + torch ops, no brightness step
        assert ts.images.numel() == B * h * w * 3                # one size, a multiple of the arena's alignment: the arena is the batch
        frames = ts.images.view(B, h, w, 3)
        mframes = ts.masks.view(B, h, w)
        dev_ctab = torch.from_numpy(ctab).cuda()
        dev_luts = torch.from_numpy(luts_p).cuda() if len(luts_p) else None
        div = torch.from_numpy(tb.divide_255_table()).cuda()

        def device_route():
            if name == "cable":
                img, msk = model.resize_frames(frames, (oh, ow)), model.resize_masks(mframes, (ow, oh))
                outs_i, outs_m = [], []
                for b, p in enumerate(plan_p):
                    dims = [d for d, on in ((1, p[tb.P_POST_FLIP_H]), (0, p[tb.P_POST_FLIP_V])) if on]
                    outs_i.append(torch.flip(img[b], dims) if dims else img[b])
                    outs_m.append(torch.flip(msk[b], dims) if dims else msk[b])
                img, msk = torch.stack(outs_i), torch.stack(outs_m)
            else:
                crops_i, crops_m = [], []
                for b, p in enumerate(plan_p):
                    x1, y1, x2, y2 = (int(v) for v in p[tb.P_X1:tb.P_Y2 + 1])
                    ci, cm = frames[p[tb.P_ITEM], y1:y2, x1:x2], mframes[p[tb.P_ITEM], y1:y2, x1:x2]
                    dims = [d for d, on in ((1, p[tb.P_FLIP_H]), (0, p[tb.P_FLIP_V])) if on]
                    if dims:
                        ci, cm = torch.flip(ci, dims), torch.flip(cm, dims)
                    if p[tb.P_ROT]:
                        ci, cm = torch.rot90(ci, int(p[tb.P_ROT]), (0, 1)), torch.rot90(cm, int(p[tb.P_ROT]), (0, 1))
                    if p[tb.P_BYTE_LUT] >= 0:
                        ci = dev_luts[p[tb.P_BYTE_LUT]][ci.long()]
                    crops_i.append(ci)
                    crops_m.append(cm)
                img = model.resize_frames(torch.stack(crops_i), (oh, ow))
                msk = model.resize_masks(torch.stack(crops_m), (ow, oh))
            return div[img.long()].permute(0, 3, 1, 2).contiguous(), dev_ctab[msk.long()]

        # the two routes agree before anything is timed
        a = tb.make_batch(model, ts, plan_p, (oh, ow), luts_p, ctab)
        d = device_route()
        row["routes_equal"] = bool(torch.equal(a[0], d[0]) and torch.equal(a[1], d[1]))
        del a, d
        row["batch_us"] = t(lambda: tb.make_batch(model, ts, plan, (oh, ow), luts, ctab))
        row["batch_hwc_us"] = t(lambda: tb.make_batch(model, ts, plan, (oh, ow), luts, ctab, image_format="hwc_u8", channel_order="bgr"))
        row["batch_plain_us"] = t(lambda: tb.make_batch(model, ts, plan_p, (oh, ow), luts_p, ctab))
        dplan, dl, dc = torch.from_numpy(plan).cuda(), torch.from_numpy(luts).cuda() if len(luts) else None, torch.from_numpy(ctab).cuda()
        out_i = torch.empty((B, 3, oh, ow), dtype=torch.float32, device="cuda")
        out_t = torch.empty((B, oh, ow), dtype=torch.uint8, device="cuda")
        row["entry_us"] = t(lambda: model._call("unetpp_train_batch_u8", ts.images, ts.images.numel(), ts.masks, ts.masks.numel(), ts.items, len(ts),
                                                dplan, B, None, 0, dl, len(luts), dc, oh, ow, 0, out_i, out_t, stream_of=ts.images))
        row["entry_gb_s"] = round(row["entry_bytes"] / row["entry_us"][0] / 1e3, 1)
        row["entry_share_of_hbm"] = round(row["entry_bytes"] / row["entry_us"][0] / HBM_BYTES_PER_US, 3)
        if name == "cable":
            ks = [int(ts.counts[i, 2]) // 2 for i in range(B)]
            row["crop_rects_us"] = t(lambda: tb.crop_rects(model, ts, np.arange(B), ks, (int(h * 0.8), int(w * 0.8))))
        row["device_route_us"] = t(device_route)
        row["device_over_batch"] = round(row["device_route_us"][0] / row["batch_plain_us"][0], 2)
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            hi, ht = tb.assemble_np(images, masks, plan, luts, (oh, ow), ctab)
            torch.from_numpy(hi).cuda(), torch.from_numpy(ht).cuda()
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) * 1e3)
        row["host_ms"] = [round(statistics.median(runs), 1), round(min(runs), 1), round(max(runs), 1)]
        row["host_over_batch"] = round(row["host_ms"][0] * 1e3 / row["batch_us"][0], 1)
        row["batch_peak_mb"] = peak(torch, lambda: tb.make_batch(model, ts, plan, (oh, ow), luts, ctab))
        row["device_route_peak_mb"] = peak(torch, device_route)
        row["batch_output_mb"] = round(B * oh * ow * 13 / 2 ** 20, 1)
        result["rows"].append(row)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del ts, frames, mframes, out_i, out_t
        torch.cuda.empty_cache()

    lines.append(json.dumps({"metric": "batch_us", "rows": [(r["input"], r["batch_us"][0], r["batch_plain_us"][0], r["device_route_us"][0],
                                                            r["host_ms"][0], r["entry_us"][0], r["entry_share_of_hbm"]) for r in result["rows"]]}))
    print(lines[-1])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
