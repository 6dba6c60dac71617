"""TEST INFRASTRUCTURE — CPU emulation (torch, float64) of the ARITHMETIC of the engine's precision 'fast'
(include/unetpp.h UNETPP_PREC_FAST), layer by layer, following the engine's own execution plan for NestedUNet
(reference graph: src/models/unetpp.py:93-135) and SimpleUNet (src/models/simple_unet.py:94-128).  The companion of
exact8_emulation.py and exact_emulation.py, whose weight folding, weight scaling and float helpers it shares.

This is NOT the parity oracle (unetpp_oracle.py; 'fast' is quoted at 5e-3 against it) and not the code under test: it is the
PREDICTED behaviour of the arithmetic the kernels document, read off
  csrc/conv3x3_mfma.h   conv3x3_bias_relu_kernel<1, ...>: one fp16 plane, fp32 accumulator, epilogue, fused pool, fused head, UPF loader
  csrc/aux_kernels.h    convert_input_kernel<1>, weight_scale_kernel, weight_pack_kernel, upsample2x_kernel<1>, head_generic_kernel<1>
  csrc/convt2x2_mfma.h  convt2x2_kernel<1>, convt_scale_kernel
Only tests/ may import this file.  The product path never does.

  input               fp16(x) of the fp32 input clamped to +-65504, or fp16(u8 / 255) with the division correctly rounded in fp32
                      (BGR reversed to RGB); one block of 8 channels, 3..7 zero
  weights             wh = fp16(w 2^k), k per output channel: max |w 2^k| in [2^13, 2^14) (weight_scale_kernel)
  conv                acc = sum a wh in an fp32-class accumulator;  v = relu(2^-k acc + bias) in fp32;  stored fp16(min(v, 65504))
  pooled copy         the 2x2 maximum of the fp32 values v (before the clamp and the rounding, both monotone), stored the same way
  decoder level 0     the `up` channels are interpolated in the conv's loader: upsample2x_kernel's index and weight rule, rounded
                      to fp16, then the conv over cat([skip, up])
  levels 1-3          the stored tensor x{l}_{4-l}u = fp16(interpolation), same rule: fp32 source coordinate s = dst (in-1)/(out-1),
                      i0 = int(s), i1 = i0 + (i0 < in-1), l1 = fmaf((in-1)/(out-1), dst, -i0) (one fma, not s - i0),
                      l0 = 1 - l1 (all fp32); x inside a row first, then the y weights; ONE rounding to fp16 at the end: the
                      last fma of the chain writes fp16 directly (see upsample)
  fused head          fp32, on conv0_4.conv2's unrounded fp32 values v
  stand-alone heads   fp32, on the stored fp16 node (head_generic_kernel<1>: the unfused final layer, deep-supervision heads)
  transposed conv     out[2y+dy][2x+dx] = 2^-k sum a wh[.., dy, dx] + bias, no activation, clamped to +-65504, stored fp16

Every layer function takes STORED planes (float64 tensors holding fp16 values) and returns (v, S): v the fp32 value before it
is stored and S = sum |a| |w| 2^-k + |b|, the magnitude the summation error of a correct implementation scales with
(tests/test_gpu_fast.py states its tolerance in units of S).  With `fp32=True` a layer is computed by the VARIANT that rounds
its accumulator to fp32 after every tap of every 16-channel chunk, in the kernel's order (chunk by chunk, tap by tap): the
distance between the two, gamma = max |v32 - v64| / S, is what tests/test_fast_emulation_host.py measures and GAMMA records.
(The interpolation is the exception: the kernels spell its fp32 chain out operation by operation, so the chain IS the emulation
and float64 its companion; see upsample.)

`knobs` are the negative controls of the tests; each makes the emulation wrong in one way the 5e-2 end-to-end bar cannot see:
  seam_tap={"conv1_0.conv2", ...}   in those layers the tap that reaches across the 32-pixel seam (dy = 1, dx = 2 of output
                                    column 31, i.e. input column 32) is dropped for output channels 0..31 and the first
                                    eight input channels (one 16-byte unit of the halo image)
  up_round_x=True                   the interpolation rounds to fp16 between the x and the y step
  up0_unrounded=True                decoder level 0 feeds the conv its `up` channels without the rounding to fp16
  pool_wrong_row={"x1_0p", ...}     in odd tile rows (pooled rows 8..15 of every 16) the pooled copy of channels 0..7 (one 16-byte
                                    store) takes its 2x2 window one row down
(the tap and the pool knob dropped for whole 32-channel blocks move the logits by 0.1-0.4 with the synthetic weights: the 5e-2 bar
does see that, so they are no evidence of a gap; at eight channels they move them by 0.01-0.03 and it does not)
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from exact8_emulation import _f16, _fold, _scaled, _t, _up  # noqa: F401  (_up: the float64 interpolation, for comparisons)

F16_MAX = 65504.0
NB = (32, 64, 128, 256, 512)          # unetpp.py:49
SB = (64, 128, 256, 512)              # simple_unet.py
# gamma per kind of layer: max |v32 - v64| / S of the fp32-accumulating variant against the float64 layer, measured on the
# reference alone by tests/test_fast_emulation_host.py (which asserts that a fresh measurement does not exceed these figures and
# that they sit below the textbook bound); tests/test_gpu_fast.py allows the device 4 gamma S.
GAMMA = {
    "conv": 1.2e-7,         # every 3x3 conv (Cin 3 .. 768), its pooled copy included
    "up": 2.0e-7,           # the stored `u` tensors (four products, three roundings)
    "head": 1.4e-7,         # fused head (32 channels in two halves) and head_generic_kernel (sequential fma from the bias)
    "convt": 1.2e-7,        # 2x2 transposed conv
}


def _f32(t):
    return t.to(torch.float32).to(torch.float64)


def _plain(sd, name):
    """SimpleUNet's convs have no BatchNorm: the canonical blob holds the fp32 weights and biases as they are"""
    return _f32(_t(sd[f"{name}.weight"])), _f32(_t(sd[f"{name}.bias"]))


def _f16_once(t):
    """float64 -> fp16 in ONE correctly rounded step (numpy converts directly; torch goes through float32, a second rounding
    that matters for the interpolation's unrounded values)"""
    return torch.from_numpy(t.numpy().astype(np.float16).astype(np.float64))


def store(v):
    """the fp16 plane an epilogue writes for the values v (float64: fp32 values, or the interpolation's exact last fma)"""
    return _f16_once(v.clamp(-F16_MAX, F16_MAX))


def ulp16(v):
    """spacing of fp16 at |v| (float64 tensor): 2^(e-10) for normals, 2^-24 below 2^-14"""
    a = v.abs().clamp(2.0 ** -14, F16_MAX)
    return 2.0 ** (torch.floor(torch.log2(a)) - 10)


# ---- input ------------------------------------------------------------------------------------------------------------------
def input_plane(x):
    """`in8` [B, 8, H, W] from the float32 NCHW input, or from uint8 NHWC BGR frames (convert_input_kernel<1>)"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        v = (x[..., ::-1].astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)      # IEEE division, correctly rounded
    else:
        v = x.astype(np.float32)
    v = store(_t(v))
    return torch.cat([v, torch.zeros(v.shape[0], 5, *v.shape[2:], dtype=torch.float64)], 1)


# ---- 3x3 conv ---------------------------------------------------------------------------------------------------------------
def _acc32(a, wh, pad=1):
    """the accumulator of the variant: rounded to fp32 after every tap of every 16-channel chunk (the MFMA's K), chunks in
    channel order, taps dy-major inside a chunk -- the order of conv3x3_bias_relu_kernel's K loop (KC = 32 walks its two
    halves one after the other, which is the same order)"""
    B, C, H, W = a.shape
    kh, kw = wh.shape[2:]
    ap = F.pad(a, (pad, pad, pad, pad))
    acc = torch.zeros(B, wh.shape[0], H, W, dtype=torch.float64)
    for c0 in range(0, C, 16):
        for dy in range(kh):
            for dx in range(kw):
                part = F.conv2d(ap[:, c0:c0 + 16, dy:dy + H, dx:dx + W], wh[:, c0:c0 + 16, dy:dy + 1, dx:dx + 1])
                acc = _f32(acc + part)
    return acc


def conv(a, w, b, name="", knobs=None, fp32=False):
    """one conv3x3 + bias + ReLU on the stored plane a (float64 tensor of fp16 values, [B, Cin, H, W]; a tensor with more
    channels than the weight, like in8, is cut) -> (v, S)"""
    knobs = knobs or {}
    a = a[:, :w.shape[1]]
    ws, k = _scaled(w)
    wh = _f16(ws)
    sc = (2.0 ** -k)[None, :, None, None]
    acc = _acc32(a, wh) if fp32 else F.conv2d(a, wh, padding=1)
    if name in knobs.get("seam_tap", ()) and a.shape[3] > 32:
        one = torch.zeros_like(wh)
        one[:32, :8, 1, 2] = wh[:32, :8, 1, 2]
        acc[:, :, :, 31] -= F.conv2d(a, one, padding=1)[:, :, :, 31]
    v = _f32(torch.relu(acc * sc + b[None, :, None, None]))
    S = F.conv2d(a.abs(), wh.abs(), padding=1) * sc + b.abs()[None, :, None, None]
    return v, S


def pooled(v, name="", knobs=None, S=None):
    """the fused 2x2 max-pool of a conv's fp32 values (conv3x3_mfma.h POOL); with S also the S of the element each maximum took"""
    if S is not None:
        p, idx = F.max_pool2d(v, 2, return_indices=True)
        return p, S.flatten(2).gather(2, idx.flatten(2)).view_as(p)
    p = F.max_pool2d(v, 2)
    if name in (knobs or {}).get("pool_wrong_row", ()):
        H = v.shape[2]
        down = F.max_pool2d(torch.cat([v[:, :, 1:], v[:, :, H - 1:]], 2), 2)      # windows of rows 2py+1, 2py+2
        odd = ((torch.arange(H // 2) // 8) % 2 == 1)[None, None, :, None] & (torch.arange(v.shape[1]) < 8)[None, :, None, None]
        p = torch.where(odd, down, p)
    return p


# ---- bilinear x2 ------------------------------------------------------------------------------------------------------------
def _axis(n_out):
    """upsample2x_kernel's index and weight rule along one axis, every step in fp32: s = (in-1)/(out-1), src = s dst,
    i0 = int(src), i1 = i0 + (i0 < in-1).  The weight is ONE fused multiply-add, l1 = fmaf(s, dst, -i0), clamped to [0, 1]: the
    rounded exact difference, as both kernels write it -- not src - i0, which carries the rounding of src, up to 2^-24 of the
    COORDINATE (4e-6 at row 127, five times the fp32 allowance of a `u` tensor).  l0 = 1 - l1."""
    n_in = n_out // 2
    s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_in > 1 else np.float32(0.0)
    dst = np.arange(n_out, dtype=np.float32)
    f = (s * dst).astype(np.float32)
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    fused = (np.float64(s) * dst.astype(np.float64) - i0.astype(np.float64)).astype(np.float32)     # exact in float64, one rounding
    l1 = np.clip(fused, np.float32(0), np.float32(1))
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), _t(l0), _t(l1)


def upsample(a, knobs=None, fp32=True, loader=False):
    """bilinear x2, align_corners=True, of the stored plane a -> (v, S): x inside a row first, then y.  The kernels spell this
    chain out operation by operation, so the emulation IS the fp32 chain (a product of an fp32 weight and an fp16 or fp32 value
    is exact in float64; every step below rounds once); fp32=False computes the same formula in float64 -- the companion gamma
    is measured against.  v is the value BEFORE the one rounding to fp16: the last fused multiply-add of the chain writes its
    fp16 result directly (v_fma_mixlo_f16 / mixhi: the exact a b + c rounded once to fp16, no fp32 in between).
      per staged row k       t_k = fmaf(lx1, a[x1], lx0 * a[x0])                                   fp32
      upsample2x_kernel      rows k = 0, 1, 2 from ybase = int(s * 2r) of the output row pair r, weights wy_k = (k == y0 - ybase ?
                             ly0 : 0) + (k == y1 - ybase ? ly1 : 0);  v = wy_2 t_2 + fmaf(wy_1, t_1, wy_0 * t_0)
      loader (level 0)       v = ly1 t[y1] + ly0 * t[y0]        (conv3x3_mfma.h up_item)"""
    knobs = knobs or {}
    h = a.shape[2]
    H, W = 2 * h, 2 * a.shape[3]
    y0, y1, ly0, ly1 = _axis(H)
    x0, x1, lx0, lx1 = _axis(W)
    r = _f32 if fp32 else (lambda t: t)
    col = lambda w: w[None, None, :, None]
    if not loader:
        ybase = y0[0::2].repeat_interleave(2)                 # int(s * 2r): the even row's own y0
        k = torch.arange(3)[None, :]
        wy = r(torch.where(k == (y0 - ybase)[:, None], ly0[:, None], torch.zeros(1, dtype=torch.float64))
               + torch.where(k == (y1 - ybase)[:, None], ly1[:, None], torch.zeros(1, dtype=torch.float64)))
        rows = (ybase[:, None] + k).clamp(max=h - 1)

    def interp(src):
        t = r(lx1 * src[:, :, :, x1] + r(lx0 * src[:, :, :, x0]))
        if knobs.get("up_round_x"):
            t = _f16(t)
        if loader:
            return col(ly1) * t[:, :, y1] + r(col(ly0) * t[:, :, y0])
        return col(wy[:, 2]) * t[:, :, rows[:, 2]] + r(col(wy[:, 1]) * t[:, :, rows[:, 1]] + r(col(wy[:, 0]) * t[:, :, rows[:, 0]]))
    return interp(a), interp(a.abs())


def decoder_conv1_upf(skip, low, w, b, name="", knobs=None, fp32=False):
    """decoder level 0 (UPF loader): conv over cat([skip, fp16(up(low))]); fp32 selects the conv's variant only"""
    knobs = knobs or {}
    u, _ = upsample(low, knobs, loader=True)
    if not knobs.get("up0_unrounded"):
        u = store(u)
    return conv(torch.cat([skip, u], 1), w, b, name, knobs, fp32)


# ---- heads ------------------------------------------------------------------------------------------------------------------
def head_fused(v, w, b, fp32=False):
    """the 1x1 head in conv0_4.conv2's epilogue: fp32 on the unrounded fp32 values v [B, 32, H, W]; per lane fma over its 16
    channels (4h + 8q + i), the two halves added, then the bias"""
    w2 = w.reshape(w.shape[0], -1)
    S = torch.einsum("bchw,kc->bkhw", v.abs(), w2.abs()) + b.abs()[None, :, None, None]
    if not fp32:
        return _f32(torch.einsum("bchw,kc->bkhw", v, w2) + b[None, :, None, None]), S
    parts = []
    for h in (0, 1):
        p = torch.zeros(v.shape[0], w2.shape[0], *v.shape[2:], dtype=torch.float64)
        for r_ in range(16):
            c = (r_ & 3) + 8 * (r_ >> 2) + 4 * h
            p = _f32(p + v[:, c:c + 1] * w2[None, :, c, None, None])
        parts.append(p)
    return _f32(b[None, :, None, None] + _f32(parts[0] + parts[1])), S


def head_generic(a, w, b, fp32=False):
    """head_generic_kernel<1> on a stored node: s = bias, s = fmaf(x[c], w[c], s) for c in order"""
    w2 = w.reshape(w.shape[0], -1)
    S = torch.einsum("bchw,kc->bkhw", a.abs(), w2.abs()) + b.abs()[None, :, None, None]
    if not fp32:
        return _f32(torch.einsum("bchw,kc->bkhw", a, w2) + b[None, :, None, None]), S
    s = b[None, :, None, None].expand(a.shape[0], -1, *a.shape[2:]).clone()
    for c in range(a.shape[1]):
        s = _f32(s + a[:, c:c + 1] * w2[None, :, c, None, None])
    return s, S


def _head_wb(sd, name="final"):
    return _f32(_t(sd[f"{name}.weight"])), _f32(_t(sd[f"{name}.bias"]))


# ---- 2x2 transposed conv (SimpleUNet) ------------------------------------------------------------------------------------------
def convt(a, w, b, fp32=False):
    """ConvTranspose2d(k = 2, stride = 2) on the stored plane a; w [Cin, Cout, 2, 2], scaled per OUTPUT channel -> (v, S)"""
    m = w.abs().amax(dim=(0, 2, 3))
    k = torch.where(m > 0, 14 - (torch.floor(torch.log2(m.clamp_min(1e-300))) + 1), torch.zeros_like(m))
    wh = _f16(w * (2.0 ** k)[None, :, None, None])
    sc = (2.0 ** -k)[None, :, None, None]
    if fp32:
        B, C, H, W = a.shape
        acc = torch.zeros(B, w.shape[1], 2 * H, 2 * W, dtype=torch.float64)
        for c0 in range(0, C, 16):
            acc = _f32(acc + F.conv_transpose2d(a[:, c0:c0 + 16], wh[c0:c0 + 16], stride=2))
    else:
        acc = F.conv_transpose2d(a, wh, stride=2)
    v = _f32(acc * sc + b[None, :, None, None])
    S = F.conv_transpose2d(a.abs(), wh.abs(), stride=2) * sc + b.abs()[None, :, None, None]
    return v, S


# ---- whole networks -----------------------------------------------------------------------------------------------------------
def fast_forward(sd: dict, x, return_nodes: bool = False, fused_head: bool = True, **knobs):
    """logits [B, C, H, W] float32 for the float32 NCHW (or uint8 NHWC BGR) input x; with return_nodes also every stored tensor
    under the engine's names ('in8', 'x0_0a', 'x0_0', 'x0_0p', ..., 'x3_1u', 'x3_1a', 'x3_1', ..., 'x0_4'), as float32.
    fused_head=False: the head reads the stored x0_4 (the engine with debug_keep_intermediates)."""
    rd = {}
    with torch.no_grad():
        rd["in8"] = cur = input_plane(x)
        fv = {}                                                  # fp32 values of the nodes (before they are stored)
        for l in range(5):
            tn = f"x{l}_0"
            v1, _ = conv(cur, *_fold(sd, f"conv{l}_0.conv1"), f"conv{l}_0.conv1", knobs)
            rd[tn + "a"] = store(v1)
            fv[tn], _ = conv(rd[tn + "a"], *_fold(sd, f"conv{l}_0.conv2"), f"conv{l}_0.conv2", knobs)
            rd[tn] = store(fv[tn])
            if l < 4:
                rd[tn + "p"] = cur = store(pooled(fv[tn], tn + "p", knobs))
        low = rd["x4_0"]
        for l in (3, 2, 1, 0):
            tn, cn = f"x{l}_{4 - l}", f"conv{l}_{4 - l}"
            w1, b1 = _fold(sd, cn + ".conv1")
            if l == 0:
                v1, _ = decoder_conv1_upf(rd["x0_0"], low, w1, b1, cn + ".conv1", knobs)
            else:
                rd[tn + "u"] = store(upsample(low, knobs)[0])
                v1, _ = conv(torch.cat([rd[f"x{l}_0"], rd[tn + "u"]], 1), w1, b1, cn + ".conv1", knobs)
            rd[tn + "a"] = store(v1)
            fv[tn], _ = conv(rd[tn + "a"], *_fold(sd, cn + ".conv2"), cn + ".conv2", knobs)
            low = rd[tn] = store(fv[tn])
        wf, bf = _head_wb(sd)
        logits = head_fused(fv["x0_4"], wf, bf)[0] if fused_head else head_generic(rd["x0_4"], wf, bf)[0]
    out = logits.numpy().astype(np.float32)
    return (out, {k: t.numpy().astype(np.float32) for k, t in rd.items()}) if return_nodes else out


def fast_simple_forward(sd: dict, x, return_nodes: bool = False, **knobs):
    """SimpleUNet in 'fast': logits float32, and with return_nodes the stored tensors 'in8', 'enc1a', 'enc1', 'enc1p', ...,
    'up3t', 'dec3a', 'dec3', ..."""
    rd = {}
    with torch.no_grad():
        rd["in8"] = cur = input_plane(x)
        for l in range(4):
            tn = f"enc{l + 1}"
            rd[tn + "a"] = store(conv(cur, *_plain(sd, tn + ".0"), tn + ".0", knobs)[0])
            v, _ = conv(rd[tn + "a"], *_plain(sd, tn + ".2"), tn + ".2", knobs)
            rd[tn] = store(v)
            if l < 3:
                rd[tn + "p"] = cur = store(pooled(v, tn + "p", knobs))
        prev = rd["enc4"]
        for l in (3, 2, 1):
            rd[f"up{l}t"] = store(convt(prev, *_plain(sd, f"up{l}"))[0])
            tn = f"dec{l}"
            rd[tn + "a"] = store(conv(torch.cat([rd[f"up{l}t"], rd[f"enc{l}"]], 1), *_plain(sd, tn + ".0"), tn + ".0", knobs)[0])
            prev = rd[tn] = store(conv(rd[tn + "a"], *_plain(sd, tn + ".2"), tn + ".2", knobs)[0])
        logits = head_generic(prev, *_head_wb(sd))[0]
    out = logits.numpy().astype(np.float32)
    return (out, {k: t.numpy().astype(np.float32) for k, t in rd.items()}) if return_nodes else out


# ---- the per-layer criterion of tests/test_gpu_fast.py (and of the host's negative controls) ----------------------------------
def layer_check(got, v, S, gamma, rounded=True):
    """The stored value `got` is fp16(v') of the device's own fp32 value v', and v' may sit 4 gamma S from the emulation's v:
    |got - v| <= ulp16(fp16(v)) / 2 + 4 gamma S per element (rounded=False: fp32 outputs, |got - v| <= 4 gamma S).  Measured
    against the unrounded v, so that a value whose rounding flips because v' and v straddle a rounding boundary (one whole ulp
    from fp16(v), by a difference of 1e-7) passes, and one that is off by an ulp for any other reason does not.
    Returns (the largest share of the allowance 4 gamma S an element uses, (|got - v| - ulp / 2) / (4 gamma S), at least 0: the
    criterion holds when it is <= 1; share of elements that differ from the emulation's stored value fp16(v))."""
    got = _t(got)
    vc = v.clamp(-F16_MAX, F16_MAX) if rounded else v
    emu = _f16_once(vc) if rounded else v
    excess = (got - vc).abs() - (0.5 * ulp16(emu) if rounded else 0.0)
    used = float((excess / (4.0 * gamma * S).clamp_min(1e-300)).max().clamp_min(0.0))
    return used, (float((got != emu).double().mean()) if rounded else 0.0)
