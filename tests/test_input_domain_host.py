"""CPU side of the input-domain tests (tests/test_gpu_input_domain.py is the device side).

Every other forward-pass test feeds the network k/255 in [0, 1] (or the uint8 frames that give exactly those values): 256 values
per channel, none negative.  Neither the code nor the reference restricts the input to that: the reference normalises with
ImageNet statistics (src/infer/preprocess.py:10-15, src/data/transforms.py:14,22: signed, about -2.1 ... 2.6), and the ingest
code claims the whole fp16 range -- conv3x3_ws.h's C0F patch loader splits every raw sample into fp16 hi + fp16 lo,
convert_input_kernel<1>, <2> and <2, true> write `in8`.  `synthetic.make_inputs_f32` generates the input families; checked
here, without a GPU, for every parity kind at the device tests' shapes and weights (CASES):

  * the generator's bits (a sha256 per kind and shape: the GPU machine regenerates the inputs from the seed),
  * the conditions the device tests rest on: every oracle tensor stays below 2^15 (so no range flag is due on the device) and
    at least two classes win,
  * the committed emulations of the three precisions stay within HALF the cap the device tests use (the device keeps its
    factor 2),
  * negative controls: a first conv that drops the input's lo plane, one that stores it with the wrong sign, and one that
    reads the channels as BGR each exceed the `exact` bar on x0_0 and on the logits -- except where they must not (integer
    inputs have no lo plane; grey inputs have no channel order).
"""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))

SEED = 7
# name -> (architecture, classes, (B, H, W), weights, plan switches of the device engine)
CASES = {
    "nested-2x32x48": ("nested", 3, (2, 32, 48), "he", {}),
    "nested-1x48x80": ("nested", 3, (1, 48, 80), "trained", {"UNETPP_PLAN_CUS": 2}),      # every workgroup walks several tiles
    "simple-2x24x40": ("simple", 7, (2, 24, 40), "simple", {}),
}
PRECISIONS = ("exact", "exact8", "fast")
EXACT_BAR = {"nested": 2e-5, "simple": 5e-5}        # tests/test_gpu_parity.py: the random-shape sweeps, times max(1, max|logit|)
NORTH_STAR = 1e-3                                   # exact8: test_logit_scale's ceiling / the SimpleUNet sweep's gate
FAST_TOL = 5e-2                                     # tests/test_gpu_parity.py FAST_TOL
LIMIT = 2.0 ** 15                                   # every oracle tensor below this: half the fp16 range, no flag is due
LO_KINDS = ("unit", "imagenet", "wide", "normal", "negated", "logspan")      # inputs with a lo plane the exact bar can see
SHA = {       # sha256(x.tobytes())[:16] of make_inputs_f32(kind, B, H, W, SEED)
    "unit 2x32x48": "3ee6787380b47b75",
    "imagenet 2x32x48": "4caab3b37667f241",
    "bytes 2x32x48": "fa45a1d1dcaa7fa3",
    "wide 2x32x48": "f73b6a0d47a65dda",
    "normal 2x32x48": "ffda9f3fc6a1c008",
    "mantissa 2x32x48": "9fe145bcabbd4cd0",
    "negated 2x32x48": "88ceeddab26080de",
    "small 2x32x48": "4b854d42c49b4580",
    "denormal 2x32x48": "e74ebd697d7e724a",
    "logspan 2x32x48": "162b901c913547c3",
    "impulses 2x32x48": "a3ac41af60f1500b",
    "zeros 2x32x48": "1c02730953829883",
    "signed_zeros 2x32x48": "28ecf66b6292a23c",
    "unit 1x48x80": "e32646edcf3a13b5",
    "imagenet 1x48x80": "963cbf7c2303e935",
    "bytes 1x48x80": "d9427db6abe59705",
    "wide 1x48x80": "3e7cebc495bd0489",
    "normal 1x48x80": "7c765f605a06578e",
    "mantissa 1x48x80": "8c5d64ee02d06149",
    "negated 1x48x80": "05d022592a9ee265",
    "small 1x48x80": "cc83a410970cf11d",
    "denormal 1x48x80": "89b32076a8a4a659",
    "logspan 1x48x80": "7a89cb7bfa64f020",
    "impulses 1x48x80": "64331ab5c1086120",
    "zeros 1x48x80": "7e36bec0af80ff78",
    "signed_zeros 1x48x80": "c3de65911ec0c34f",
    "unit 2x24x40": "8fc09820d8dd352f",
    "imagenet 2x24x40": "4f522826dd0eacf1",
    "bytes 2x24x40": "72de45d3bd529403",
    "wide 2x24x40": "728a2680cf32fde9",
    "normal 2x24x40": "9e5a50827d60970e",
    "mantissa 2x24x40": "e92b1d0925624c69",
    "negated 2x24x40": "c72e26c8e142aa0c",
    "small 2x24x40": "7561d1f875074cc8",
    "denormal 2x24x40": "39f2c612192e55c3",
    "logspan 2x24x40": "242117bdb43f125b",
    "impulses 2x24x40": "3916e1a6e4dcaec8",
    "zeros 2x24x40": "46e2096b90794736",
    "signed_zeros 2x24x40": "27ceaf8faf03f4ac",
}


def state_dict(case):
    from unet_amd import synthetic as syn
    arch, C, _, weights, _ = CASES[case]
    if weights == "he":
        return syn.make_state_dict(C, 3, True, 2)
    if weights == "trained":
        return syn.make_trained_like_state_dict(C, 3, True, 2)
    return syn.make_simple_state_dict(C, 3, 0)


def inputs(case, kind):
    from unet_amd import synthetic as syn
    return syn.make_inputs_f32(kind, *CASES[case][2], SEED)


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """(logits, {name: tensor}) of the oracle; computed once per (case, kind) and shared -- treat as read-only"""
    import unetpp_oracle as oracle
    fwd = oracle.torch_forward if CASES[case][0] == "nested" else oracle.simple_unet_torch_forward
    return fwd(state_dict(case), inputs(case, kind), return_intermediates=True)


@functools.lru_cache(maxsize=None)
def emulated(case, kind, precision):
    """logits of the committed emulation of `precision` (None where there is none: SimpleUNet has one for `fast` only)"""
    import exact8_emulation as em8
    import exact_emulation as em
    import fast_emulation as fe
    sd, x = state_dict(case), inputs(case, kind)
    if CASES[case][0] == "nested":
        return {"exact": em.exact_forward, "exact8": em8.exact8_forward, "fast": fe.fast_forward}[precision](sd, x)
    return fe.fast_simple_forward(sd, x) if precision == "fast" else None


def scale_of(ref):
    return max(1.0, float(np.abs(ref).max()))


def emulated_error(case, kind, precision):
    emu = emulated(case, kind, precision)
    return None if emu is None else float(np.abs(emu - reference(case, kind)[0]).max())


def device_cap(case, kind, precision):
    """the largest max|device logit - oracle logit| the device test accepts for this case"""
    arch = CASES[case][0]
    s = scale_of(reference(case, kind)[0])
    exact = EXACT_BAR[arch] * s
    if precision == "exact":
        return exact
    if precision == "exact8" and arch == "simple":
        return NORTH_STAR * s                       # no emulation: test_exact8_simple_unet_random_shapes_and_batch_rows' gate
    ceiling = (NORTH_STAR if precision == "exact8" else FAST_TOL) * s
    return min(2 * emulated_error(case, kind, precision) + exact, ceiling)


def first_block64(sd, x):
    """conv0_0 of NestedUNet (conv -> BatchNorm -> ReLU twice, src/models/unetpp.py:17-26) in float64 on x"""
    import torch
    import torch.nn.functional as F
    import exact8_emulation as em8
    v = torch.from_numpy(np.asarray(x, np.float64))
    with torch.no_grad():
        for conv in ("conv0_0.conv1", "conv0_0.conv2"):
            T = lambda n: torch.from_numpy(np.asarray(sd[n], np.float64))
            bn = conv.replace(".conv", ".bn")
            v = F.conv2d(v, T(conv + ".weight"), T(conv + ".bias"), padding=1)
            s = T(bn + ".weight") / torch.sqrt(T(bn + ".running_var") + em8.BN_EPS)
            v = torch.relu((v - T(bn + ".running_mean")[None, :, None, None]) * s[None, :, None, None] + T(bn + ".bias")[None, :, None, None])
    return v.numpy()


def simple_enc1a64(sd, x):
    """relu(enc1.0(x)) of SimpleUNet (src/models/simple_unet.py:94-128) in float64"""
    import torch
    import torch.nn.functional as F
    T = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    with torch.no_grad():
        return torch.relu(F.conv2d(T(x), T(sd["enc1.0.weight"]), T(sd["enc1.0.bias"]), padding=1)).numpy()


def bits_equal(a, b):
    """equal as bit patterns of float32 (+0.0 and -0.0 differ)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------- the generator
def test_generator_hashes(syn):
    got = {}
    for case, (_, _, shape, _, _) in CASES.items():
        for kind in syn.INPUT_KINDS:
            x = syn.make_inputs_f32(kind, *shape, SEED)
            assert x.dtype == np.float32 and x.shape == (shape[0], 3, shape[1], shape[2]) and x.flags.c_contiguous
            assert bits_equal(x, syn.make_inputs_f32(kind, *shape, SEED))
            got[f"{kind} {'x'.join(map(str, shape))}"] = hashlib.sha256(x.tobytes()).hexdigest()[:16]
    assert got == SHA, "\n".join(f'    "{k}": "{v}",' for k, v in got.items())


def test_generator_families_are_what_they_say(syn):
    B, H, W = 2, 32, 48
    g = lambda kind: syn.make_inputs_f32(kind, B, H, W, SEED)
    frames = syn.make_frames_u8(B, H, W, "smooth", SEED)
    unit = syn.frames_to_chw_f32(frames)
    assert bits_equal(g("unit"), unit) and bits_equal(g("negated"), -unit)
    assert np.array_equal(g("bytes"), np.transpose(frames[..., ::-1], (0, 3, 1, 2)).astype(np.float32))
    im = g("imagenet")
    assert -2.2 < im.min() < -1.0 and 1.5 < im.max() < 2.7
    wide = g("wide")
    assert wide.min() < -250 and wide.max() > 250 and np.abs(wide).max() < 255 and (wide != np.rint(wide)).mean() > 0.99
    half = lambda a: a.astype(np.float16).astype(np.float32)
    for kind in ("wide", "mantissa", "normal"):                    # a lo plane, and bits below it (lo is not the whole remainder)
        a = g(kind)
        assert ((a - half(a)) != 0).mean() > 0.95, kind
    assert (g("mantissa") >= 0).all() and (g("mantissa") < 1).all()
    small = g("small")
    assert np.abs(small).max() < 1e-2 and (np.abs(half(small)) < 2.0 ** -14).mean() > 0.04        # hi often an fp16 subnormal
    den = g("denormal")
    assert 0 < np.abs(den).max() <= 2.0 ** -127 and (den < 0).any() and (den > 0).any()
    assert not half(den).any() and np.signbit(half(den)).any()
    ls = g("logspan")
    m, e = np.frexp(ls)
    assert e.min() == -29 and e.max() == 7 and (ls < 0).any() and (ls > 0).any() and np.unique(e).size == 37
    assert 2.0 ** -30 <= np.abs(ls).min() and np.abs(ls).max() < 128 and ((ls - half(ls)) != 0).mean() > 0.9
    imp = g("impulses")
    pos = syn.impulse_positions(H, W)
    assert len(pos) == 16 and {(0, 0), (H - 1, W - 1), (15, 31), (16, 32), (15, 32), (16, 31)} <= set(pos)
    assert int((imp != 0).sum()) == B * 3 * len(pos) and all((np.abs(imp[:, :, r, c]) == 1).all() for r, c in pos)
    assert (imp == 1).any() and (imp == -1).any()
    assert syn.impulse_positions(24, 40) == [(r, c) for r in (0, 15, 16, 23) for c in (0, 31, 32, 39)]
    assert len(syn.impulse_positions(16, 16)) == 4                  # only the corners exist
    z, sz = g("zeros"), g("signed_zeros")
    assert not z.any() and not np.signbit(z).any() and not sz.any() and 0.3 < np.signbit(sz).mean() < 0.7
    with pytest.raises(ValueError):
        syn.make_inputs_f32("uint8", B, H, W, SEED)


# ----------------------------------------------------------------------------- what the device tests rest on
@pytest.mark.parametrize("case", list(CASES))
def test_conditions_and_emulations(case, syn):
    import torch
    torch.set_num_threads(8)
    arch = CASES[case][0]
    failures = []
    print(f"\n{case}: kind | largest oracle tensor | max|logit| | classes that win | emulated error / s per precision | device cap / s")
    for kind in syn.PARITY_INPUT_KINDS:
        ref, inter = reference(case, kind)
        top = max(float(np.abs(v).max()) for v in list(inter.values()) + [ref, inputs(case, kind)])
        wins = np.unique(np.argmax(ref, axis=1)).size
        s = scale_of(ref)
        row = f"  {kind:<9} {top:10.4g} {float(np.abs(ref).max()):9.4g} {wins} |"
        if not top < LIMIT:
            failures.append(f"{kind}: an oracle tensor reaches {top:.4g}")
        if wins < 2:
            failures.append(f"{kind}: one class wins everywhere")
        for prec in PRECISIONS:
            err = emulated_error(case, kind, prec)
            cap = device_cap(case, kind, prec)
            row += f" {prec}: " + ("-" if err is None else f"{err / s:.2e}") + f" / {cap / s:.2e} |"
            if err is not None and not err <= cap / 2:
                failures.append(f"{kind} {prec}: the emulation is {err:.3e} from the oracle, above half the device's cap {cap:.3e}")
        print(row)
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------- negative controls
def _with_first_conv(fn, sd, x):
    """exact_forward with conv0_0.conv1's input split replaced: (logits, x0_0)"""
    import exact8_emulation as em8
    import exact_emulation as em
    import torch.nn.functional as F

    def first_conv(xx, w, b):
        ws, k = em8._scaled(w)
        xh = em8._f16(xx); xl = fn(em8._f16(xx - xh))
        wh = em8._f16(ws); wl = em8._f16(ws - wh)
        c = lambda a, bb: F.conv2d(a, bb, padding=1)
        return em8._finish(c(xh, wh) + c(xl, wh) + c(xh, wl), k, b)
    keep = em._first_conv
    em._first_conv = first_conv
    try:
        lg, nodes = em.exact_forward(sd, x, return_nodes=True)
    finally:
        em._first_conv = keep
    return lg, nodes["x0_0"]


def test_negative_controls_of_the_first_conv(syn):
    """A first conv that drops the input's lo plane, or stores |lo|, must be visible at the `exact` bar on x0_0 and on the logits
    for every kind with a lo plane, and invisible for `bytes` (integers up to 255 are fp16 values).  The unchanged split is the
    control of the control: it passes."""
    import torch
    torch.set_num_threads(8)
    case = "nested-2x32x48"
    sd = state_dict(case)
    bar = EXACT_BAR["nested"]
    failures = []
    print("\nfirst conv, error / bar on (x0_0, logits): kind | documented | lo dropped | |lo|")
    for kind in LO_KINDS + ("bytes",):
        x = inputs(case, kind)
        ref, inter = reference(case, kind)
        s, s0 = scale_of(ref), scale_of(inter["x0_0"])
        row = f"  {kind:<9}"
        for tag, fn in (("documented", lambda l: l), ("lo dropped", lambda l: l * 0), ("|lo|", lambda l: l.abs())):
            lg, x00 = _with_first_conv(fn, sd, x)
            e0, e = float(np.abs(x00 - inter["x0_0"]).max()) / (bar * s0), float(np.abs(lg - ref).max()) / (bar * s)
            row += f" | {e0:7.2f} {e:7.2f}"
            seen = e0 > 1 and e > 1
            if tag == "documented" or kind == "bytes":
                if e0 > 1 or e > 1:
                    failures.append(f"{kind}, {tag}: above the bar ({e0:.2f}, {e:.2f}) where nothing is wrong")
            elif not seen:
                failures.append(f"{kind}, {tag}: inside the bar ({e0:.2f}, {e:.2f}): the device test could not see it")
        print(row)
    assert not failures, "\n".join(failures)


BGR_BLIND = ("denormal",)       # +-2^22 x 2^-149: below every plane of every mode, the channels carry nothing


def test_negative_control_bgr(syn):
    """A first conv that reads the channels in BGR order exceeds the `exact` bar on x0_0 and on the logits for every kind whose
    values reach the planes at all, and changes nothing on a grey input."""
    import exact_emulation as em
    import torch
    torch.set_num_threads(8)
    case = "nested-2x32x48"
    sd = state_dict(case)
    bar = EXACT_BAR["nested"]
    failures = []
    print("\nchannels read as BGR, error / bar on (x0_0, logits): kind")
    for kind in syn.PARITY_INPUT_KINDS:
        x = inputs(case, kind)
        ref, inter = reference(case, kind)
        lg, nodes = em.exact_forward(sd, np.ascontiguousarray(x[:, ::-1]), return_nodes=True)
        e0 = float(np.abs(nodes["x0_0"] - inter["x0_0"]).max()) / (bar * scale_of(inter["x0_0"]))
        e = float(np.abs(lg - ref).max()) / (bar * scale_of(ref))
        print(f"  {kind:<9} {e0:10.2f} {e:10.2f}")
        if (e0 > 1 and e > 1) == (kind in BGR_BLIND):
            failures.append(f"{kind}: ({e0:.2f}, {e:.2f})")
    grey = np.ascontiguousarray(np.repeat(inputs(case, "imagenet")[:, 1:2], 3, axis=1))
    a, b = em.exact_forward(sd, grey), em.exact_forward(sd, np.ascontiguousarray(grey[:, ::-1]))
    assert np.array_equal(a, b), "a grey input has no channel order"
    assert not failures, "\n".join(failures)
