#!/usr/bin/env python3
"""Generate the deep-supervision fixtures tests/golden/ds_*.npz from the REFERENCE model's own forward.

    python scripts/make_golden_ds.py

Runs where the reference source is checked out (see oracle/make_golden.py, whose import helpers are reused), never on
the GPU box; only the small .npz files travel.  The reference returns [out, out1, out2, out3] only in training mode
(src/models/unetpp.py:121-133), so the model is put in train() and every BatchNorm2d back in eval(): that is exactly
the deep-supervision forward with the running statistics the engine folds into its weights.

Each file holds, for B frames of synthetic.make_frames_u8 and synthetic.make_state_dict(C, 3, True, wseed):
  out0..out3      float32 [B,C,H,W]  the reference's list entries
  mask0..mask3    uint8   [B,H,W]    first-max argmax of each entry's logits
  margin0..margin3 float32 [B,H,W]   top-2 logit margin (a mask pixel may flip only where this is tiny)
and the SHA-256s of the frames and of the weights.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden  # noqa: E402  (reference import helpers)

OUT = os.path.join(ROOT, "tests", "golden")

# tag, C, wseed, B, H, W, frame kind, frame seed: the frames of s_c3_64x64 and s_c7_48x80
CASES = [
    ("ds_c3_64x64", 3, 8, 2, 64, 64, "uniform", 12),
    ("ds_c7_48x80", 7, 2, 1, 48, 80, "smooth", 13),      # 6x10 -> 48x80 for out3: non-square, non-dyadic extents
]


def reference_ds_outputs(NestedUNet, sd_np, C, x):
    model = NestedUNet(num_classes=C, input_channels=3, deep_supervision=True, pretrained_encoder=False)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    with torch.no_grad():
        outs = model(torch.from_numpy(x))
    assert isinstance(outs, list) and len(outs) == 4
    return [o.numpy().astype(np.float32) for o in outs]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)           # the thread count the other fixtures were made with
    syn = make_golden._load_synthetic()
    NestedUNet = make_golden._import_reference()
    for tag, C, wseed, B, H, W, kind, fseed in CASES:
        sd = syn.make_state_dict(C, 3, True, wseed)
        frames = syn.make_frames_u8(B, H, W, kind, fseed)
        outs = reference_ds_outputs(NestedUNet, sd, C, syn.frames_to_chw_f32(frames))
        payload = dict(num_classes=C, wseed=wseed, B=B, H=H, W=W, kind=kind, fseed=fseed, frames_sha=make_golden.sha(frames),
                       weights_sha=make_golden.sha(np.concatenate([v.ravel().astype(np.float64) for v in sd.values()])))
        line = [tag]
        for k, o in enumerate(outs):
            payload[f"out{k}"] = o
            payload[f"mask{k}"] = np.argmax(o, axis=1).astype(np.uint8)
            payload[f"margin{k}"] = make_golden.margin_of(o).astype(np.float32)
            line.append(f"out{k}[{o.min():.3f},{o.max():.3f}] min_margin={payload[f'margin{k}'].min():.2e}")
        path = os.path.join(OUT, tag + ".npz")
        np.savez_compressed(path, **payload)
        print(" ".join(line), f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
