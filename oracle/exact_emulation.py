"""TEST INFRASTRUCTURE — CPU emulation (torch, float64) of the ARITHMETIC of the engine's precision 'exact'
(include/unetpp.h UNETPP_PREC_EXACT; unet-_amd/csrc/conv3x3_mfma.h:24 "lo*hi, hi*lo, hi*hi"), following the
engine's own execution plan for NestedUNet (reference graph: src/models/unetpp.py:93-135).  The companion of
exact8_emulation.py, whose weight folding, weight scaling, epilogue, first conv and interpolation it shares.

This is NOT the parity oracle (unetpp_oracle.py) and not the code under test: it is the PREDICTED behaviour of the documented
arithmetic.  tests/test_value_range_host.py and tests/test_gpu_value_range.py use it to say where in the fp16 window a stored
tensor may sit before that arithmetic leaves its error bar (the `lo` plane becomes an fp16 subnormal, quantum 2^-24, as soon
as |v| < 0.25), and as a bound for what the device may lose there.  Only tests/ may import this file.

  stored activation   (h, l):  v clamped to +-65504;  h = fp16(v);  l = fp16(v - h);  read back as h + l
  weights             ws = w 2^k (max |ws| of an output channel in [2^13, 2^14));  wh = fp16(ws);  wl = fp16(ws - wh)
  product             acc += h wh + l wh + h wl   (l wl dropped);   v = relu(2^-k acc + bias)   in fp32

`knobs` are the negative controls of the tests (each makes the emulation wrong in one documented way):
  drop_lo={"x2_2", ...}   those tensors are stored without their lo plane
  clamp=32768.0           the storing epilogues clamp at another value than fp16's largest
  pool_unclamped=True     the pooled copy of a node is split from the unclamped fp32 value
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from exact8_emulation import _f16, _finish, _first_conv, _fold, _scaled, _t, _up

F16_MAX = 65504.0


class Act:
    """an activation tensor as the engine stores it in 'exact': two fp16 planes"""

    def __init__(self, v, clamp=F16_MAX, drop_lo=False):
        v = v.to(torch.float32).to(torch.float64).clamp(-clamp, clamp)      # the epilogue's fp32 value, clamped on its way out
        self.h = _f16(v)
        self.l = torch.zeros_like(v) if drop_lo else _f16(v - self.h)

    @property
    def value(self):
        return self.h + self.l


def act_from_planes(h, l) -> Act:
    """a tensor the engine stored, from its planes as unetpp_debug_read returns them ("name#hi", "name#lo")"""
    a = Act.__new__(Act)
    a.h, a.l = _t(h), _t(l)
    return a


def _cat(acts):
    a = Act.__new__(Act)
    a.h = torch.cat([t.h for t in acts], 1); a.l = torch.cat([t.l for t in acts], 1)
    return a


def _product(act: Act, ws, pad):
    """sum over taps and channels of the split product, in the accumulator domain (weights carry 2^k)"""
    wh = _f16(ws); wl = _f16(ws - wh)
    c = lambda a, b: F.conv2d(a, b, padding=pad)
    return c(act.h, wh) + c(act.l, wh) + c(act.h, wl)


def _conv(act: Act, w, b):
    ws, k = _scaled(w)
    return _finish(_product(act, ws, 1), k, b)


def conv_layer(inp: Act, sd, name):
    """fp32 output values of one conv3x3 + BN + ReLU in 'exact' arithmetic (before they are split into planes)"""
    w, b = _fold(sd, name)
    return _conv(inp, w, b)


def _decoder_conv1(skip: Act, low: Act, w, b, lowres_gemm: bool):
    """conv3x3(cat([skip, up(low)])) in both of the engine's forms (see exact8_emulation._decoder_conv1): the fused upsample
    interpolates the stored low-res values in the loader and splits the result; the low-resolution GEMM multiplies the up
    channels tap by tap at low resolution, interpolates the fp32 products and adds the taps that stay inside the image"""
    ws, k = _scaled(w)
    cs = skip.h.shape[1]
    if not lowres_gemm:
        return _finish(_product(_cat([skip, Act(_up(low.value))]), ws, 1), k, b)
    acc = _product(skip, ws[:, :cs], 1)
    H, W = skip.h.shape[2:]
    for dy in range(3):
        for dx in range(3):
            y = _product(low, ws[:, cs:, dy:dy + 1, dx:dx + 1], 0).to(torch.float32).to(torch.float64)   # Y is an fp32 tensor
            u = F.pad(_up(y), (1, 1, 1, 1))
            acc = acc + u[:, :, dy:dy + H, dx:dx + W]
    return _finish(acc, k, b)


def exact_forward(sd: dict, x: np.ndarray, tapmm_levels=(2, 3), return_nodes: bool = False,
                  drop_lo=(), clamp: float = F16_MAX, pool_unclamped: bool = False):
    """logits [B, C, H, W] float32 for float32 input x [B,3,H,W]; with return_nodes also every tensor as the engine would read
    it back: nodes 'x0_0' ..., inner tensors 'x1_0a' ... ('x0_0a' never leaves the first block's kernel: its entry is the value
    handed to conv0_0.conv2), pooled 'x0_0p' ... 'x3_0p'"""
    x = _t(x).to(torch.float32).to(torch.float64)
    rd = {}
    A = lambda name, v: Act(v, clamp, name in drop_lo)
    with torch.no_grad():
        def block(inp, name, tn, first=False, dec=None):
            w1, b1 = _fold(sd, f"{name}.conv1"); w2, b2 = _fold(sd, f"{name}.conv2")
            if first:
                v1 = _first_conv(inp, w1, b1)
            elif dec is not None:
                v1 = _decoder_conv1(inp, dec[0], w1, b1, dec[1])
            else:
                v1 = _conv(inp, w1, b1)
            a1 = A(tn + "a", v1)
            rd[tn + "a"] = a1.value
            return _conv(a1, w2, b2)                          # fp32 value of the block's output (before it is split)
        v, a = {}, {}
        v["x0_0"] = block(x, "conv0_0", "x0_0", first=True)
        for l in range(5):
            tn = f"x{l}_0"
            if l:
                pv = F.max_pool2d(v[f"x{l - 1}_0"], 2)       # on the epilogue's fp32 values (conv3x3_ws.h ws_epilogue, POOL)
                p = Act(pv, 3.0e38 if pool_unclamped else clamp, f"x{l - 1}_0p" in drop_lo)
                rd[f"x{l - 1}_0p"] = p.value
                v[tn] = block(p, f"conv{l}_0", tn)
            a[tn] = A(tn, v[tn])
        low = a["x4_0"]
        for l in (3, 2, 1, 0):
            tn = f"x{l}_{4 - l}"
            v[tn] = block(a[f"x{l}_0"], f"conv{l}_{4 - l}", tn, dec=(low, l in tapmm_levels))
            low = a[tn] = A(tn, v[tn])
        # the 1x1 head runs in fp32 on conv0_4.conv2's fp32 registers (nothing is split in between)
        wf = _t(sd["final.weight"]).to(torch.float32).to(torch.float64); bf = _t(sd["final.bias"]).to(torch.float32).to(torch.float64)
        logits = F.conv2d(v["x0_4"], wf) + bf[None, :, None, None]
    out = logits.numpy().astype(np.float32)
    if not return_nodes:
        return out
    for kk, t in a.items():
        rd[kk] = t.value
    return out, {kk: t.numpy().astype(np.float32) for kk, t in rd.items()}
