#!/usr/bin/env python3
"""Where the distance of loss_grad_np from the exact gradient comes from, and what a float64 chain would give.

    python scripts/experiments/loss_grad_error_parts.py

CPU and NumPy only; reads tests/golden/loss_grad_scenes.npz.  Per scene and combination of unet_amd.loss_grad, relative to the
largest gradient and over all positions, against the float64 formulas with exact columns (loss_grad_np(exact=True)):
  table   the same formulas with the coefficients of the fixed-point table (float64 coefficients, float64 pixels)
  coef32  ... with those coefficients rounded to float32, float64 pixels
  full    loss_grad_np as it is: float32 coefficients and the float32 per-pixel chain
and, against the reference's float64 gradient at the fixture's stored positions:
  at32    loss_grad_np,   at64  the same steps in float64 (float64 coefficients, np.exp / np.log) rounded to float32 once,
  e32     the reference's own float32 noise (over all positions, as stored).
The last lines count the pairs whose at32 and at64 lie within e32."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from unet_amd import loss as ls, loss_grad as lg
    g = np.load(os.path.join(ROOT, "tests", "golden", "loss_grad_scenes.npz"))
    print(f"{'scene':<16} {'criterion':<9} {'params':<10} {'table':>9} {'coef32':>9} {'full':>9} | {'at32':>9} {'at64':>9} {'e32':>9}")
    worst, n32, n64 = np.zeros(3), 0, 0
    for name in lg.GRAD_SCENES:
        logits, target = ls.make_scene(name)
        B, C, H, W = logits.shape
        pos = g[f"{name}_pos"]
        for criterion, params in lg.GRAD_COMBOS:
            kw = lg.combo_keywords(criterion, params, C)
            gamma = 2 if criterion == "advanced" else 0
            table, _ = ls.loss_sums_np(logits, target, gamma)
            p, _, t, _ = lg._exact_terms(logits, target, C)
            onehot = np.arange(C)[None, :, None] == t[:, None, :]
            exact = lg.loss_grad_np(logits, target, lg.coefficients_from_columns(onehot.sum(2), p.sum(2), (p * onehot).sum(2), H * W, criterion, **kw),
                                    gamma, exact=True)
            gmax = np.abs(exact).max()
            T, P, I, _, _ = ls._columns(table)
            c64 = lg.coefficients_from_columns(T, P, I, H * W, criterion, **kw)
            c32 = lg.coefficients_from_sums(table, H * W, criterion, **kw)
            g64 = lg.loss_grad_np(logits, target, c64, gamma, exact=True)
            parts = np.array([np.abs(g64 - exact).max(), np.abs(lg.loss_grad_np(logits, target, c32.astype(np.float64), gamma, exact=True) - exact).max(),
                              np.abs(lg.loss_grad_np(logits, target, c32, gamma).astype(np.float64) - exact).max()]) / gmax
            worst = np.maximum(worst, parts)
            key = f"{name}_{criterion}_{params}"
            ref_max, e32, _ = g[f"{key}_stats"]
            at32 = np.abs(lg.at_positions(lg.loss_grad_np(logits, target, c32, gamma).astype(np.float64), pos) - g[f"{key}_g64"]).max() / ref_max
            at64 = np.abs(lg.at_positions(g64.astype(np.float32).astype(np.float64), pos) - g[f"{key}_g64"]).max() / ref_max
            n32, n64 = n32 + (at32 <= e32), n64 + (at64 <= e32)
            print(f"{name:<16} {criterion:<9} {params:<10} {parts[0]:9.2e} {parts[1]:9.2e} {parts[2]:9.2e} | {at32:9.2e} {at64:9.2e} {e32:9.2e}")
    print(f"largest: table {worst[0]:.2e}, coef32 {worst[1]:.2e}, full {worst[2]:.2e}")
    print(f"within e32 at the stored positions: the float32 chain {n32} of 40, a float64 chain {n64} of 40")


if __name__ == "__main__":
    main()
