"""Deterministic synthetic weights and frames (NumPy only, PCG64).

The reference ships no checkpoint and no sample video (its .gitignore:30-40 excludes them), so
every parity test and every bench line runs on synthetic data generated here.  The generator is
NumPy-only so that the GPU box (where /root/reference does not exist) regenerates bit-identical
weights and frames from the seed.

State-dict layout mirrors ``NestedUNet.state_dict()`` of the reference
(src/models/unetpp.py:13-26 ConvBlock, :66-91 NestedUNet members): per ConvBlock
``{conv1,conv2}.{weight[Co,Ci,3,3],bias[Co]}``, ``{bn1,bn2}.{weight,bias,running_mean,
running_var}[Co]`` + ``num_batches_tracked`` (int64 scalar); ``final.{weight[C,32,1,1],bias[C]}``;
with deep supervision also ``ds3_1/ds2_2/ds1_3.{weight,bias}``.

Default PyTorch init gives a degenerate net (every pixel argmaxes to one class), so weights are
He-normal with perturbed BN statistics: all classes appear and logits span roughly [-3, 2].
"""
from __future__ import annotations

import numpy as np

from .manifest import NB_FILTER, SIMPLE_WIDTHS, conv_blocks, simple_unet_manifest, state_dict_manifest  # noqa: F401 (re-exported)


def make_state_dict(num_classes: int = 3, in_channels: int = 3, deep_supervision: bool = True,
                    seed: int = 0) -> dict:
    """He-normal conv weights, N(0,0.05^2) biases, BN gamma/var ~ U[0.75,1.25], beta/mean ~ N(0,0.2^2)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, shape, dtype in state_dict_manifest(num_classes, in_channels, deep_supervision):
        leaf = key.split(".")[-1]
        parent = key.split(".")[-2]
        if dtype == "int64":
            sd[key] = np.array(100, dtype=np.int64)
        elif leaf == "weight" and len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            sd[key] = (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        elif leaf == "bias" and not parent.startswith("bn"):
            sd[key] = (rng.standard_normal(shape) * 0.05).astype(np.float32)
        elif leaf in ("weight", "running_var"):          # BN gamma, running variance
            sd[key] = rng.uniform(0.75, 1.25, shape).astype(np.float32)
        else:                                            # BN beta, running mean
            sd[key] = (rng.standard_normal(shape) * 0.2).astype(np.float32)
    return sd


def make_simple_state_dict(num_classes: int = 7, num_channels: int = 3, seed: int = 0) -> dict:
    """He-normal weights (fan_in of the forward contraction), N(0, 0.05^2) biases."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    sd = {}
    for key, shape, _ in simple_unet_manifest(num_classes, num_channels):
        if key.endswith("weight"):
            if key.startswith("up"):
                fan_in = shape[0]                      # each output pixel sees one tap of every input channel
            else:
                fan_in = shape[1] * shape[2] * shape[3]
            sd[key] = (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        else:
            sd[key] = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    return sd


def _bilinear_up(a: np.ndarray, h: int, w: int) -> np.ndarray:
    """Plain half-pixel bilinear resize of a [h0,w0,c] float array (frame synthesis only)."""
    h0, w0 = a.shape[:2]
    ys = np.clip((np.arange(h) + 0.5) * h0 / h - 0.5, 0, h0 - 1)
    xs = np.clip((np.arange(w) + 0.5) * w0 / w - 0.5, 0, w0 - 1)
    y0 = np.floor(ys).astype(int); y1 = np.minimum(y0 + 1, h0 - 1); fy = (ys - y0)[:, None, None]
    x0 = np.floor(xs).astype(int); x1 = np.minimum(x0 + 1, w0 - 1); fx = (xs - x0)[None, :, None]
    top = a[y0][:, x0] * (1 - fx) + a[y0][:, x1] * fx
    bot = a[y1][:, x0] * (1 - fx) + a[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def make_frame_u8(h: int, w: int, index: int = 0, kind: str = "smooth", seed: int = 1234) -> np.ndarray:
    """uint8 HWC 'BGR' frame, already at model resolution (the cv2 resize of
    infer_two_stage_burr.py:124 is outside the engine contract).

    kind='uniform': i.i.d. uniform bytes; kind='smooth': low-frequency field + 20 % noise
    (video-like: large flat regions, so near-tie pixels are rarer but class regions are coherent).
    """
    rng = np.random.Generator(np.random.PCG64(seed + index))
    if kind == "uniform":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    lo = rng.uniform(0.0, 255.0, (max(h // 32, 2), max(w // 32, 2), 3))
    noise = rng.uniform(0.0, 255.0, (h, w, 3))
    f = 0.8 * _bilinear_up(lo, h, w) + 0.2 * noise
    return np.ascontiguousarray(np.clip(np.rint(f), 0, 255).astype(np.uint8))     # C order: raw memcpy-able


def make_frames_u8(b: int, h: int, w: int, kind: str = "smooth", seed: int = 1234, first: int = 0) -> np.ndarray:
    return np.ascontiguousarray(np.stack([make_frame_u8(h, w, first + i, kind, seed) for i in range(b)]))


def frames_to_chw_f32(frames_u8: np.ndarray) -> np.ndarray:
    """uint8 [B,H,W,3] BGR -> float32 [B,3,H,W] RGB in [0,1]: the resize-free part of
    preprocess_image (infer_two_stage_burr.py:122-127): BGR->RGB, astype(float32)/255.0, HWC->CHW."""
    rgb = frames_u8[..., ::-1]
    x = rgb.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))


# ----------------------------------------------------------------------------- the float32 input domain
# forward() takes any float32 [B,3,H,W]: the reference normalises with ImageNet statistics in src/infer/preprocess.py:10-15 and
# with A.Normalize() in src/data/transforms.py:14,22, so its inputs are signed (about -2.1 ... 2.6), and nothing restricts them to
# k/255.  The families below cover what the ingest code (the fused first block's patch loader, convert_input_kernel) has to
# split into fp16 planes: signed, wide, full-mantissa, tiny and subnormal values, zeros of both signs
# (tests/test_input_domain_host.py, tests/test_gpu_input_domain.py).
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
INPUT_KINDS = ("unit", "imagenet", "bytes", "wide", "normal", "mantissa", "negated", "small", "denormal", "logspan", "impulses",
               "zeros", "signed_zeros")
PARITY_INPUT_KINDS = INPUT_KINDS[:-2]


def impulse_positions(h: int, w: int):
    """(row, col) of the four corners and of the tile seams of the first block (columns 31 / 32, rows 15 / 16; the image border
    where the image has no such row or column), crossed: 16 positions or fewer"""
    rows = sorted({0, min(15, h - 1), min(16, h - 1), h - 1})
    cols = sorted({0, min(31, w - 1), min(32, w - 1), w - 1})
    return [(r, c) for r in rows for c in cols]


def make_inputs_f32(kind: str, b: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """float32 [b,3,h,w] of one input family (INPUT_KINDS), bit for bit the same on every machine: NumPy + PCG64 only, the draws are
    integers or the float64 normals the weight generators use, everything after them float32 or integer arithmetic
    (tests/test_input_domain_host.py records a sha256 per kind and shape).  Families built on frames take
    `make_frames_u8(b, h, w, "smooth", seed)`."""
    if kind not in INPUT_KINDS:
        raise ValueError(f"unknown input kind {kind!r}: one of {INPUT_KINDS}")
    rng = np.random.Generator(np.random.PCG64([int(seed), INPUT_KINDS.index(kind)]))
    shape = (b, 3, h, w)
    f32 = np.float32

    def uniform24():
        """uniform float32 in [0, 1) from 24 random bits: every mantissa bit is used"""
        return (rng.integers(0, 1 << 24, shape, dtype=np.int64).astype(f32) * f32(2.0 ** -24)).astype(f32)

    if kind in ("unit", "imagenet", "bytes", "negated"):
        frames = make_frames_u8(b, h, w, "smooth", seed)
        if kind == "bytes":
            x = np.transpose(frames[..., ::-1].astype(f32), (0, 3, 1, 2))
        else:
            x = frames_to_chw_f32(frames)
        if kind == "imagenet":
            mean = np.array(IMAGENET_MEAN, dtype=f32)[None, :, None, None]
            std = np.array(IMAGENET_STD, dtype=f32)[None, :, None, None]
            x = ((x - mean) / std).astype(f32)
        elif kind == "negated":
            x = -x
    elif kind == "wide":
        x = (f32(255.0) * (f32(2.0) * uniform24() - f32(1.0))).astype(f32)
    elif kind == "mantissa":
        x = uniform24()
    elif kind == "normal":
        x = rng.standard_normal(shape).astype(f32)
    elif kind == "small":
        x = (f32(1e-3) * rng.standard_normal(shape).astype(f32)).astype(f32)
    elif kind == "denormal":
        n = rng.integers(-(1 << 22), (1 << 22) + 1, shape, dtype=np.int64)
        bits = (np.abs(n).astype(np.uint32) | np.where(n < 0, np.uint32(0x80000000), np.uint32(0))).astype(np.uint32)
        x = bits.view(f32)                                        # |n| 2^-149: the subnormal's bit pattern is the integer
    elif kind == "logspan":
        # +-2^e, e in [-30, 7): the integer part of e uniform over the 37 octaves, the position inside the octave from 23 random
        # mantissa bits (no exp2 call: its last bit is libm's) -- every magnitude the planes hold, each with a full mantissa
        e = rng.integers(-30, 7, shape, dtype=np.int64)
        frac = rng.integers(0, 1 << 23, shape, dtype=np.int64).astype(np.uint32)
        sign = rng.integers(0, 2, shape, dtype=np.int64).astype(np.uint32) << np.uint32(31)
        x = (((e + 127).astype(np.uint32) << np.uint32(23)) | frac | sign).view(f32)
    elif kind == "impulses":
        x = np.zeros(shape, dtype=f32)
        for r, c in impulse_positions(h, w):
            x[:, :, r, c] = np.where(rng.integers(0, 2, (b, 3)) == 1, f32(1.0), f32(-1.0))
    else:
        x = np.zeros(shape, dtype=f32)
        if kind == "signed_zeros":
            x = np.where(rng.integers(0, 2, shape) == 1, f32(-0.0), f32(0.0)).astype(f32)
    return np.ascontiguousarray(x, dtype=f32)


def make_trained_like_state_dict(num_classes: int = 3, in_channels: int = 3, deep_supervision: bool = True,
                                 seed: int = 2, big_gain: float = 3.0) -> dict:
    """`make_state_dict` with the BatchNorm statistics a trained checkpoint shows and He-init never does
    (probes BN folding and the fp16 dynamic range, reference unetpp.py:17-26): in every BN a few
      * dead channels   conv weight/bias and running_mean x 1e-4, running_var = 1e-8 (eps dominates the fold),
      * negative gamma, zero gamma, and large gamma (x big_gain) channels."""
    sd = make_state_dict(num_classes, in_channels, deep_supervision, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    for k in list(sd):
        if not k.endswith("running_var"):
            continue
        bn = k[:-len("running_var")]                  # 'conv0_0.bn1.'
        conv = bn.replace(".bn", ".conv")
        n = sd[k].shape[0]
        idx = rng.permutation(n)
        a, b = max(1, n // 16), max(1, n // 32)
        dead, neg, zero, big = idx[:a], idx[a:2 * a], idx[2 * a:2 * a + b], idx[2 * a + b:2 * a + 2 * b]
        sd[k][dead] = 1e-8
        sd[conv + "weight"][dead] *= 1e-4
        sd[conv + "bias"][dead] *= 1e-4
        sd[bn + "running_mean"][dead] *= 1e-4
        sd[bn + "weight"][neg] *= -1
        sd[bn + "weight"][zero] = 0
        sd[bn + "weight"][big] *= big_gain
    return sd


# ----------------------------------------------------------------------------- moving a tensor through the value range
# ConvBlock is conv -> BatchNorm -> ReLU (reference unetpp.py:23-26): a block's output scale (gamma, beta) and its consumers'
# weight scale trade any power of two without changing the function -- and, in fp32, without changing a bit of it.  The
# engine stores activations as fp16 planes, so where a tensor sits in that window is NOT arbitrary for it
# (tests/test_value_range_host.py, tests/test_gpu_value_range.py).
NESTED_NODES = ("x0_0", "x1_0", "x2_0", "x3_0", "x4_0", "x3_1", "x2_2", "x1_3", "x0_4")
NESTED_SITES = NESTED_NODES + tuple(n + "a" for n in NESTED_NODES)
SIMPLE_SITES = ("enc1a", "enc1", "enc2a", "enc2", "enc3a", "enc3", "enc4a", "enc4",
                "up3t", "dec3a", "dec3", "up2t", "dec2a", "dec2", "up1t", "dec1a", "dec1")


def _pow2(k: int) -> np.float32:
    k = int(k)
    if not -60 <= k <= 60:
        raise ValueError(f"k={k}: powers of two between 2^-60 and 2^60 only")
    return np.float32(2.0) ** np.float32(k)


def _mul(sd, key, f, cols=slice(None)):
    """sd[key][:, cols] *= f (f a power of two: exact in float32 short of under/overflow), on a fresh copy of that entry"""
    a = np.array(sd[key], dtype=np.float32, copy=True)
    if a.ndim == 1:
        a *= f
    else:
        a[:, cols] *= f
    sd[key] = a


def rescale_state_dict(sd: dict, site: str, k: int) -> dict:
    """A copy of a NestedUNet state dict in which tensor `site` is produced 2^k larger and consumed 2^-k smaller.

    site: a node 'x0_0' ... 'x4_0', 'x3_1', 'x2_2', 'x1_3', 'x0_4' (the block's bn2 weight and bias are multiplied; the
    consumers divided: the next encoder block's conv1 over all input channels -- the pool commutes with a positive scale --,
    the skip or up slice of the decoder conv1 that reads it (skip channels first, unetpp.py:112-116), its ds head if the
    checkpoint has one, `final` for x0_4), or a block's inner tensor 'x0_0a' ... (bn1 against conv2.weight).
    Every reference output is unchanged, bit for bit in float32.  site='logits' multiplies final.weight and final.bias
    instead: that one changes the function (logits x 2^k)."""
    out = dict(sd)
    up, down = _pow2(k), _pow2(-k)
    if site == "logits":
        _mul(out, "final.weight", up); _mul(out, "final.bias", up)
        return out
    if site not in NESTED_SITES:
        raise ValueError(f"unknown site {site!r}: one of {NESTED_SITES} or 'logits'")
    l, j = int(site[1]), int(site[3])
    blk = f"conv{l}_{j}"
    if site.endswith("a"):
        _mul(out, f"{blk}.bn1.weight", up); _mul(out, f"{blk}.bn1.bias", up)
        _mul(out, f"{blk}.conv2.weight", down)
        return out
    _mul(out, f"{blk}.bn2.weight", up); _mul(out, f"{blk}.bn2.bias", up)
    f = NB_FILTER
    if j == 0:
        if l < 4:
            _mul(out, f"conv{l + 1}_0.conv1.weight", down)                            # through the pool
            _mul(out, f"conv{l}_{4 - l}.conv1.weight", down, slice(0, f[l]))          # as the skip of its own level
        else:
            _mul(out, "conv3_1.conv1.weight", down, slice(f[3], None))                # as the up source of level 3
    elif l > 0:
        _mul(out, f"conv{l - 1}_{j + 1}.conv1.weight", down, slice(f[l - 1], None))   # up source of the level above
        if f"ds{l}_{j}.weight" in out:
            _mul(out, f"ds{l}_{j}.weight", down)
    else:
        _mul(out, "final.weight", down)
    return out


def rescale_simple_state_dict(sd: dict, site: str, k: int) -> dict:
    """The same for SimpleUNet (simple_unet.py:94-128), which has no BatchNorm: the producing conv's or transposed conv's
    weight and bias are multiplied, its consumers' weights divided (cat([up, skip]): up channels first).  Sites are the
    engine's tensor names: 'enc1a' (after enc1.0), 'enc1' (after enc1.2), 'up3t', 'dec3a', 'dec3', ...; 'logits'."""
    out = dict(sd)
    up, down = _pow2(k), _pow2(-k)
    if site == "logits":
        _mul(out, "final.weight", up); _mul(out, "final.bias", up)
        return out
    if site not in SIMPLE_SITES:
        raise ValueError(f"unknown site {site!r}: one of {SIMPLE_SITES} or 'logits'")
    w = SIMPLE_WIDTHS
    kind = site.rstrip("at0123456789")                         # 'enc', 'dec' or 'up'
    l = int(site[len(kind)])
    if site.startswith("up"):
        prod, cons = f"up{l}", [(f"dec{l}.0.weight", slice(0, w[l - 1]))]
    elif site.endswith("a"):
        prod, cons = f"{kind}{l}.0", [(f"{kind}{l}.2.weight", slice(None))]
    elif kind == "enc":
        prod = f"enc{l}.2"
        cons = [(f"enc{l + 1}.0.weight", slice(None)), (f"dec{l}.0.weight", slice(w[l - 1], None))] if l < 4 \
            else [("up3.weight", None)]
    else:
        prod = f"dec{l}.2"
        cons = [(f"up{l - 1}.weight", None)] if l > 1 else [("final.weight", slice(None))]
    if prod.startswith("up"):
        _mul(out, prod + ".weight", up, slice(None))           # ConvTranspose2d weight is [Cin, Cout, 2, 2]: all of it
    else:
        _mul(out, prod + ".weight", up)
    _mul(out, prod + ".bias", up)
    for key, cols in cons:
        if cols is None:                                       # a transposed conv consumes over dim 0: all of it
            out[key] = np.array(out[key], dtype=np.float32, copy=True) * down
        else:
            _mul(out, key, down, cols)
    return out


# ----------------------------------------------------------------------------- moving the 1x1 heads through the class indices
# `final` (unetpp.py:85,119; simple_unet.py:92,124) and the deep-supervision heads ds1_3 / ds2_2 / ds3_1 (unetpp.py:87-91) are
# one weight row and one bias per class.  He-normal rows let two or three classes win everywhere, so most class indices are
# never the answer of a test; the constructors below put a chosen row at a chosen index, tie two classes bit for bit, or pin
# every logit to a constant (tests/test_head_classes_host.py, tests/test_gpu_head_classes.py).
HEAD_NAMES = ("final", "ds1_3", "ds2_2", "ds3_1")


def _heads(sd):
    return [h for h in HEAD_NAMES if h + ".weight" in sd]


def _head_copy(sd, head):
    """(weight, bias) of one head as fresh float32 arrays (the input dict's arrays are never written)"""
    return (np.array(sd[head + ".weight"], dtype=np.float32, copy=True), np.array(sd[head + ".bias"], dtype=np.float32, copy=True))


def rotate_head(sd: dict, j: int) -> dict:
    """A copy of a state dict in which class c of every head has row and bias (c - j) mod C of the original: the logits are
    the original's, rolled by j along the class axis."""
    out = dict(sd)
    for head in _heads(sd):
        w, b = _head_copy(sd, head)
        out[head + ".weight"] = np.ascontiguousarray(np.roll(w, int(j), axis=0))
        out[head + ".bias"] = np.ascontiguousarray(np.roll(b, int(j), axis=0))
    return out


def tie_head(sd: dict, a: int, b: int) -> dict:
    """A copy in which row and bias b of every head are bit copies of row and bias a: classes a and b tie at every pixel."""
    out = dict(sd)
    for head in _heads(sd):
        w, bias = _head_copy(sd, head)
        C = w.shape[0]
        if not (0 <= a < C and 0 <= b < C and a != b):
            raise ValueError(f"tie_head: classes {a}, {b} of {C}")
        w[b] = w[a]
        bias[b] = bias[a]
        out[head + ".weight"], out[head + ".bias"] = w, bias
    return out


def constant_head(sd: dict, biases) -> dict:
    """A copy whose head weights are all +0.0 and whose biases are `biases` [C]: every logit of every pixel is its class's
    bias exactly (bias + sum of fma(v, +0.0, .) over finite v >= 0)."""
    out = dict(sd)
    for head in _heads(sd):
        w, _ = _head_copy(sd, head)
        bias = np.array(biases, dtype=np.float32, copy=True).reshape(-1)
        if bias.shape[0] != w.shape[0] or not np.isfinite(bias).all():
            raise ValueError(f"constant_head: {bias.shape[0]} finite biases wanted for {w.shape[0]} classes")
        out[head + ".weight"] = np.zeros_like(w)                 # +0.0, never -0.0
        out[head + ".bias"] = bias
    return out
